// nz_chain_plan.hpp -- the tile plan of a chained filter grid (conv_chain_kernel, nz_filter.hip), built on the host.
//
// Plain C++, no HIP: the context builds a plan once per geometry (nz_runtime.cpp), the kernel reads one 32-byte record per
// workgroup, and tests/test_chain_plan.py compiles this header on its own against a brute-force restatement.
//
// L fused launches of depths T[0..L) over columns [0, cols) x rows [or0, or1) form ONE grid.  Launch l cuts the window into
// tiles_x[l] x tiles_y[l] tiles whose interiors are (TW - 2 HX) x (TH - 2 H) cells, H = T[l] * O, HX = nz_chain_hx(H); its
// tiles are the work items first[l] .. first[l + 1] - 1 (item = first[l] + tile, tile = by * tiles_x[l] + bx): the index of a
// tile's flag, and the number nz_debug_chain_delay names.
//
// Which item a workgroup takes: vb = blockIdx.x, class = vb & 7 (the XCD that receives the workgroup).  Launch l owns the
// positions first[l] <= vb < first[l + 1].  Within a launch the classes split the tiles into contiguous runs in class order,
// each as long as the number of the launch's positions of that class; a class works through its run in the order of its
// positions, even classes forwards and odd classes backwards (neighbouring classes finish a launch on the rows they share and
// start the next one at the far ends).
//
// What a tile waits for: the launch-(l-1) tiles whose interior meets its interior widened by max(H, Hp) rows and max(HX, HXp)
// columns (clipped to the window): those whose stores it reads and those that read the cells it overwrites.  A rectangle of
// nx x ny tiles; the kernel polls nine flags at most, a plan that would need more is refused.
#pragma once
#include <cstdint>

constexpr int NZ_CHAIN_MAXL = 8;
constexpr int NZ_CHAIN_MAXDEP = 3;  // awaited tiles per direction

constexpr int nz_chain_hx(int H) { return (H + 3) & ~3; }  // x halo: a multiple of four columns (16-byte accesses)

// what a plan depends on
struct nz_chain_key {
    int O;       // (taps - 1) / 2
    int TH, TW;  // tile rows and columns, halo included
    int cols, or0, or1;
    int L;
    int T[NZ_CHAIN_MAXL];
};
inline bool nz_chain_key_equal(const nz_chain_key &a, const nz_chain_key &b) {
    if (a.O != b.O || a.TH != b.TH || a.TW != b.TW || a.cols != b.cols || a.or0 != b.or0 || a.or1 != b.or1 || a.L != b.L) return false;
    for (int l = 0; l < a.L; l++)
        if (a.T[l] != b.T[l]) return false;
    return true;
}

// one work item, indexed by blockIdx.x
struct nz_chain_item {
    int32_t ox0, oz0;  // first column / row of the tile's interior
    int32_t tl;        // T | l << 16
    int32_t item;      // first[l] + tile
    int32_t dep0;      // flag index of the first awaited tile
    int32_t nx, ny;    // awaited tiles across and down (ny == 0: launch 0 waits for nobody)
    int32_t stride;    // flags between two rows of awaited tiles: tiles_x[l - 1]
};
static_assert(sizeof(nz_chain_item) == 32, "one s_load_dwordx8 per workgroup");

struct nz_chain_layout {
    int total;
    int first[NZ_CHAIN_MAXL + 1], tiles_x[NZ_CHAIN_MAXL], tiles_y[NZ_CHAIN_MAXL];
};

inline int nz_chain_class_count(int n, int c) { return n > c ? (n - c + 7) >> 3 : 0; }  // #{vb < n : vb % 8 == c}

// tiles per launch; total == 0: no such plan (L out of range, a depth without an interior, an empty window)
inline nz_chain_layout nz_chain_layout_of(const nz_chain_key &k) {
    nz_chain_layout lay{};
    if (k.L < 1 || k.L > NZ_CHAIN_MAXL || k.cols < 1 || k.or1 <= k.or0) return lay;
    for (int l = 0; l < k.L; l++) {
        const int H = k.T[l] * k.O, HX = nz_chain_hx(H);
        const int OW = k.TW - 2 * HX, OH = k.TH - 2 * H;
        if (k.T[l] < 1 || OW < 1 || OH < 1) return nz_chain_layout{};
        lay.tiles_x[l] = (k.cols + OW - 1) / OW;
        lay.tiles_y[l] = (k.or1 - k.or0 + OH - 1) / OH;
        const long long n = (long long)lay.first[l] + (long long)lay.tiles_x[l] * lay.tiles_y[l];
        if (n > 0x7fffffff) return nz_chain_layout{};
        lay.first[l + 1] = (int)n;
    }
    lay.total = lay.first[k.L];
    return lay;
}

// fills out[0 .. total); false: the plan does not exist or a tile would wait for more than 3 x 3 producers
inline bool nz_chain_plan_build(const nz_chain_key &k, nz_chain_item *out) {
    const nz_chain_layout lay = nz_chain_layout_of(k);
    if (lay.total < 1) return false;
    for (int l = 0; l < k.L; l++) {
        const int f0 = lay.first[l], f1 = lay.first[l + 1];
        const int T = k.T[l], H = T * k.O, HX = nz_chain_hx(H);
        const int OW = k.TW - 2 * HX, OH = k.TH - 2 * H;
        int Hw = 0, HXw = 0, OWp = 1, OHp = 1;
        if (l > 0) {
            const int Hp = k.T[l - 1] * k.O, HXp = nz_chain_hx(Hp);
            Hw = H > Hp ? H : Hp;
            HXw = HX > HXp ? HX : HXp;
            OWp = k.TW - 2 * HXp;
            OHp = k.TH - 2 * Hp;
        }
        int start[8], mine[8], seen[8];
        for (int c = 0, s = 0; c < 8; c++) {
            mine[c] = nz_chain_class_count(f1, c) - nz_chain_class_count(f0, c);
            start[c] = s;
            s += mine[c];
            seen[c] = 0;
        }
        for (int vb = f0; vb < f1; vb++) {
            const int c = vb & 7, j = seen[c]++;
            const int tile = start[c] + ((c & 1) ? mine[c] - 1 - j : j);
            const int by = tile / lay.tiles_x[l], bx = tile - by * lay.tiles_x[l];
            nz_chain_item it{};
            it.ox0 = bx * OW;
            it.oz0 = k.or0 + by * OH;
            it.tl = T | l << 16;
            it.item = f0 + tile;
            if (l > 0) {
                const int ix0 = it.ox0 - HXw > 0 ? it.ox0 - HXw : 0;
                const int ix1 = it.ox0 + OW + HXw - 1 < k.cols - 1 ? it.ox0 + OW + HXw - 1 : k.cols - 1;
                const int iz0 = it.oz0 - Hw > k.or0 ? it.oz0 - Hw : k.or0;
                const int iz1 = it.oz0 + OH + Hw - 1 < k.or1 - 1 ? it.oz0 + OH + Hw - 1 : k.or1 - 1;
                const int px0 = ix0 / OWp, px1 = ix1 / OWp, py0 = (iz0 - k.or0) / OHp, py1 = (iz1 - k.or0) / OHp;
                it.nx = px1 - px0 + 1;
                it.ny = py1 - py0 + 1;
                if (it.nx > NZ_CHAIN_MAXDEP || it.ny > NZ_CHAIN_MAXDEP) return false;
                it.stride = lay.tiles_x[l - 1];
                it.dep0 = lay.first[l - 1] + py0 * it.stride + px0;
            }
            out[vb] = it;
        }
    }
    return true;
}
