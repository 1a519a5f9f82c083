// nz_fill.hip -- depression filling: lakes and pit-free drainage (gfx950; new-framework feature).
//
// THE MODEL (include/noize_hip.h states it for the caller, tests/fill_ref.py restates it in numpy):
//   Square tile res x res, row-major z * res + x, float32 throughout, no contraction, the same in every float mode.
//   Neighbours k = 0..7 in the fluvial stage's order W E S N SW SE NW NE; a neighbour outside the tile does not exist.
//   Outlets are the fluvial stage's: border cells and cells with h[c] <= seaLevel.  W[c] = h[c] for an outlet.
//   Operator for every other cell: m = +inf; for k ascending: t = W[k] + epsilon; m = t < m ? t : m;
//   F(W)[c] = h[c] > m ? h[c] : m.  Start: W = +inf at the non-outlets.  Result: the fixed point reached from that start.
//   With epsilon == 0 it is the spill elevation (the minimax path height to an outlet; flats remain); with epsilon > 0 every
//   filled cell sits at least epsilon above some neighbour, so every non-outlet has a strictly lower neighbour.
// F is monotone and the start lies above every fixed point, so every order of updates -- Jacobi, tile-local sweeps, a
// priority queue -- goes down to the same floats, the greatest fixed point.  That is what lets the kernel below update in
// whatever order is fastest and still be tested for bit equality.  Two facts make the arithmetic order-free as well: no
// value is a NaN (heights are finite, +inf + epsilon = +inf), and t is never -0 (x + +0 and x + epsilon round to +0, not
// -0), so min_k (W[k] + epsilon) == (min_k W[k]) + epsilon bit for bit whatever the order of the minimum.
//
// One launch per PASS of W, on the geometry of nz_tile64.hpp (VEC: 16-byte accesses where planes and pitch allow), by the
// pass protocol of nz_relax_pass.hpp: gate, tile skip, sweeps, closing byte and word, and why.  What is the fill's own:
//   fill     the tile's own h into registers, its W at radius 1 into LDS (18 x 72 floats); ring cells outside the grid hold
//            +inf.  The first pass reads no W plane: it derives the start state from h.
//   sweeps   every thread updates its four cells left to right and back right to left in registers (Gauss-Seidel inside
//            the thread, Jacobi between threads).  W only ever falls, so "changed" is the net effect of a sweep.
// The finalise launch takes the protocol's verdict: at rest -> W to the heights and W - h to the depth plane; otherwise
// the heights stay and the depth is zero: all or nothing, a caller never sees +inf.
//
// WIN, the stripe form (nz_fill_stripe): one ROUND on the owned rows [r0, r1) of a stripe-shaped buffer with a pitch; the
// workgroups tile the owned rows, the grid's bounds are the global grid's seen from the buffer.  The one row of W on each
// side of the owned rows is FROZEN: read from the caller's plane in every pass (or, in a round that starts from the
// heights, derived from them), never written, whichever of the two planes the pass alternates between.  When the owned
// rows end inside a tile, the frozen row lies in a thread's own slot: it is loaded, marked fixed and not stored.  status[GO]
// (written by fill_round_begin from the caller's `proceed` word) lets every launch of the round return at once; pass 0 of
// a round that continues from W has no tile bytes to go by, so all of its tiles are live.  A pass 0 that moves a cell
// stores 1 to the caller's `changed` word: W only ever falls, so a moved cell differs from its value at entry for good.
//
// The cap, `sweeps`, is 16 (nz_stages.cpp): enough to carry a value across the tile's 16 rows and 64 columns.  4 to 64 were
// measured: DESIGN.md section 4, "depression filling".
#include "nz_internal.hpp"
#include "nz_relax_pass.hpp"
#include "nz_tile64.hpp"

namespace {

using namespace nz_tile64;  // the tile, its LDS layout, ring_cell
using namespace nz_relax;   // the status words and the pass protocol

// the plane a pass works on: tiles of res^2 cells back to back (pitch = res, the rest derived), or -- WIN -- the owned rows
// of one stripe-shaped buffer, rows in buffer coordinates
struct fill_win {
    int pitch;           // floats between rows; without WIN the tile's resolution
    int xhi;             // last column of the grid
    int zlo, zhi;        // first and last row of the global grid
    int r0, r1;          // owned rows [r0, r1)
    int ghost_from_h;    // the frozen rows are the start state derived from h (a round with `first`), else w_ghost's
    const float *w_ghost;  // the caller's W plane
    int *changed_out;    // the caller's word
};

template <bool FIRST, bool VEC, bool WIN>
__global__ __launch_bounds__(FT) void fill_pass_kernel(const float *__restrict__ h, const float *__restrict__ w_in,
                                                       float *__restrict__ w_out, int *status,
                                                       const unsigned char *__restrict__ flags_in,
                                                       unsigned char *__restrict__ flags_out, float eps, float sea,
                                                       fill_win win, int pass, int sweeps) {
    __shared__ __attribute__((aligned(16))) float W[(FZ + 2) * LP];  // radius 1: LDS row = plane row - z0 + 1
    const int tid = threadIdx.x;

    if constexpr (WIN) {
        if (!status[ST_GO]) return;
    }
    const bool all_live = WIN && pass == 0;  // a round's first pass: nothing is known about the pass before
    const bool t0 = tid == 0;
    const int prev = series_gate<FIRST>(status, t0, pass, all_live);
    if (!prev) return;
    const int tnx = gridDim.x, tnz = gridDim.y;
    const size_t tile0 = (size_t)blockIdx.z * tnx * tnz;
    const size_t me = tile0 + (size_t)blockIdx.y * tnx + blockIdx.x;  // this tile's byte
    if (!FIRST && !all_live) {
        // nz_relax::tile_live, written out: through the helper this kernel measures 0.5 % slower
        int live = 0;
        if (tid < 9) {
            const int bx = (int)blockIdx.x + tid % 3 - 1, bz = (int)blockIdx.y + tid / 3 - 1;
            if (bx >= 0 && bx < tnx && bz >= 0 && bz < tnz) live = flags_in[tile0 + (size_t)bz * tnx + bx];
        }
        if (!__syncthreads_or(live)) {
            if (t0) flags_out[me] = 0;
            return;
        }
    }

    const int res = win.pitch;  // (the pitch; without WIN the resolution)
    const int x0 = blockIdx.x * FX, z0 = (WIN ? win.r0 : 0) + blockIdx.y * FZ;
    const size_t base = WIN ? 0 : (size_t)blockIdx.z * res * res;
    const int hi = WIN ? win.xhi : res - 1;                                   // last column
    const int zlo = WIN ? win.zlo : 0, zhi = WIN ? win.zhi : res - 1;         // the grid's rows
    const int rlo = WIN ? (zlo > win.r0 - 1 ? zlo : win.r0 - 1) : 0, rhi = WIN ? (zhi < win.r1 ? zhi : win.r1) : hi;  // rows read
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= rlo && pz <= rhi; };
    auto on_border = [&](int px, int pz) { return px == 0 || px == hi || pz == zlo || pz == zhi; };
    const float INF = __builtin_inff();
    // WIN: W of a cell of a frozen row
    auto ghost = [&](int qx, int qz) {
        const size_t q = (size_t)qz * res + qx;
        if (!win.ghost_from_h) return win.w_ghost[q];
        const float hq = h[q];
        return on_border(qx, qz) || hq <= sea ? hq : INF;
    };

    // this thread's four cells
    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = WIN ? pz < win.r1 : pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;  // VEC: cols % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill ----
    float hc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wc[4] = {INF, INF, INF, INF};
    if (quad) {
        const float4 v = *reinterpret_cast<const float4 *>(h + c0);
        hc[0] = v.x, hc[1] = v.y, hc[2] = v.z, hc[3] = v.w;
        if constexpr (!FIRST) {
            const float4 w = *reinterpret_cast<const float4 *>(w_in + c0);
            wc[0] = w.x, wc[1] = w.y, wc[2] = w.z, wc[3] = w.w;
        }
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            hc[j] = h[c0 + j];
            if constexpr (!FIRST) wc[j] = w_in[c0 + j];
        }
    }
    unsigned fixed = 0;  // bit j: own cell j is an outlet or lies outside the grid; it is never updated
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool in = row_in && px + j <= hi;
        const bool outlet = in && (on_border(px + j, pz) || hc[j] <= sea);
        if (!in || outlet) fixed |= 1u << j;
        if (FIRST && outlet) wc[j] = hc[j];
    }
    if constexpr (WIN) {
        if (pz == win.r1 && pz <= zhi) {  // the frozen row below, inside the tile: fixed (row_in is false), and not stored
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (px + j <= hi) wc[j] = ghost(px + j, pz);
        }
    }
    *reinterpret_cast<float4 *>(&W[(tz + 1) * LP + LC + tx]) = make_float4(wc[0], wc[1], wc[2], wc[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        float v = INF;
        if (inside(qx, qz)) {
            const size_t q = base + (size_t)qz * res + qx;
            if (WIN && (qz < win.r0 || qz >= win.r1)) {
                v = ghost(qx, qz);
            } else if constexpr (FIRST) {
                const float hq = h[q];
                if (on_border(qx, qz) || hq <= sea) v = hq;
            } else {
                v = w_in[q];
            }
        }
        W[lz * LP + lx] = v;
    }
    __syncthreads();

    // ---- sweeps inside LDS, the ring frozen ----
    bool moved = FIRST;  // uniform over the workgroup
    for (int s = 0; s < sweeps; s++) {
        int ch = 0;
        if (fixed != 15u) {
            float up[6], v[6];  // up: the smaller of the rows above and below, columns px-1 .. px+4; v: the own row
            {
                const float *r0 = &W[tz * LP + LC + tx], *r1 = r0 + LP, *r2 = r1 + LP;
                const float4 a = *reinterpret_cast<const float4 *>(r0), b = *reinterpret_cast<const float4 *>(r1),
                             c = *reinterpret_cast<const float4 *>(r2);
                up[0] = fminf(r0[-1], r2[-1]), up[1] = fminf(a.x, c.x), up[2] = fminf(a.y, c.y), up[3] = fminf(a.z, c.z);
                up[4] = fminf(a.w, c.w), up[5] = fminf(r0[4], r2[4]);
                v[0] = r1[-1], v[1] = b.x, v[2] = b.y, v[3] = b.z, v[4] = b.w, v[5] = r1[4];
            }
            auto relax = [&](int j) {
                if (fixed >> j & 1u) return;
                const float mn = fminf(fminf(fminf(up[j], up[j + 1]), fminf(up[j + 2], v[j])), v[j + 2]);
                const float m = mn + eps;
                v[j + 1] = hc[j] > m ? hc[j] : m;
            };
            relax(0), relax(1), relax(2), relax(3);
            relax(2), relax(1), relax(0);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                ch |= __float_as_uint(v[j + 1]) != __float_as_uint(wc[j]);
                wc[j] = v[j + 1];
            }
        }
        if (!__syncthreads_or(ch)) break;  // (the barrier behind the read phase)
        moved = true;
        if (ch) *reinterpret_cast<float4 *>(&W[(tz + 1) * LP + LC + tx]) = make_float4(wc[0], wc[1], wc[2], wc[3]);
        __syncthreads();
    }

    // ---- store ----
    if (quad) {
        *reinterpret_cast<float4 *>(w_out + c0) = make_float4(wc[0], wc[1], wc[2], wc[3]);
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            w_out[c0 + j] = wc[j];
        }
    }
    if (t0) {
        close_tile<FIRST>(status, flags_out, me, pass, moved);
        if (WIN && !FIRST && pass == 0 && moved) *win.changed_out = 1;
    }
}

// a stripe round begins: go = the caller's proceed word (none: go), the status words of a fresh series, the caller's
// `changed` word = go && first
__global__ void fill_round_begin_kernel(int *status, const int *proceed, int *changed_out, int first) {
    const int go = proceed ? *proceed != 0 : 1;
    status[ST_GO] = go;
    status[ST_PASSES] = 0;
    status[ST_CHANGED] = status[ST_CHANGED + 1] = status[ST_CHANGED + 2] = 0;
    *changed_out = go && first ? 1 : 0;
}

// a stripe round of an odd number of passes ends in the work plane: when every pass ran, its owned rows go to the caller's
// plane (a round that came to rest earlier holds equal cells in both)
__global__ __launch_bounds__(256) void fill_round_end_kernel(float *__restrict__ w, const float *__restrict__ w_work,
                                                             const int *status, int passes, int pitch, int cols, int r0,
                                                             int r1) {
    if (!status[ST_GO] || status[ST_PASSES] != passes) return;
    const int x = blockIdx.x * 256 + threadIdx.x, z = r0 + blockIdx.y;
    if (x < cols && z < r1) w[(size_t)z * pitch + x] = w_work[(size_t)z * pitch + x];
}

// the stripe's all or nothing on the owned rows, by the caller's verdict
__global__ __launch_bounds__(256) void fill_stripe_finalise_kernel(float *__restrict__ h, const float *__restrict__ w,
                                                                   float *__restrict__ depth, const int *converged, int pitch,
                                                                   int cols, int r0, int r1) {
    const int x = blockIdx.x * 256 + threadIdx.x, z = r0 + blockIdx.y;
    if (x >= cols || z >= r1) return;
    const size_t i = (size_t)z * pitch + x;
    if (*converged) {
        const float hv = h[i], wv = w[i];
        h[i] = wv;
        if (depth) depth[i] = wv - hv;
    } else if (depth) {
        depth[i] = 0.0f;
    }
}

// all or nothing: the fixed point when the last pass that ran changed nothing, otherwise the heights as they were
__global__ __launch_bounds__(256) void fill_finalise_kernel(float *__restrict__ h, const float *__restrict__ w,
                                                            float *__restrict__ depth, int *status, size_t n) {
    const bool converged = series_at_rest(status);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[ST_CONVERGED] = converged ? 1 : 0;
    if (i >= n) return;
    if (converged) {
        const float hv = h[i], wv = w[i];
        h[i] = wv;
        if (depth) depth[i] = wv - hv;
    } else if (depth) {
        depth[i] = 0.0f;
    }
}

// the form of a pass by <FIRST, VEC, WIN>
template <bool FIRST, bool WIN>
void launch_pass(bool vec, dim3 grid, hipStream_t s, const float *h, const float *w_in, float *w_out, int *status,
                 const unsigned char *flags_in, unsigned char *flags_out, float eps, float sea, const fill_win &win, int pass,
                 int sweeps) {
    if (vec) NZ_LAUNCH((fill_pass_kernel<FIRST, true, WIN>), grid, dim3(FT), 0, s, h, w_in, w_out, status, flags_in, flags_out, eps, sea, win, pass, sweeps);
    else NZ_LAUNCH((fill_pass_kernel<FIRST, false, WIN>), grid, dim3(FT), 0, s, h, w_in, w_out, status, flags_in, flags_out, eps, sea, win, pass, sweeps);
}

}  // namespace

int32_t nz_launch_fill_pass(hipStream_t s, const float *h, const float *w_in, float *w_out, int *status,
                            const unsigned char *flags_in, unsigned char *flags_out, float eps, float sea, int res, int count,
                            int pass, int sweeps) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(w_in) | reinterpret_cast<uintptr_t>(w_out);
    const bool vec = (bits & 15) == 0 && res % 4 == 0;  // a row, and with it a tile of the batch, starts 16-byte aligned
    const fill_win win{res, res - 1, 0, res - 1, 0, res, 0, nullptr, nullptr};
    if (pass == 0) launch_pass<true, false>(vec, grid, s, h, w_in, w_out, status, flags_in, flags_out, eps, sea, win, pass, sweeps);
    else launch_pass<false, false>(vec, grid, s, h, w_in, w_out, status, flags_in, flags_out, eps, sea, win, pass, sweeps);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fill_round_begin(hipStream_t s, int *status, const int *proceed, int *changed, int first) {
    NZ_LAUNCH(fill_round_begin_kernel, dim3(1), dim3(1), 0, s, status, proceed, changed, first);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fill_stripe_pass(hipStream_t s, const float *h, const float *w_in, float *w_out, const float *w_ghost,
                                   int *status, const unsigned char *flags_in, unsigned char *flags_out, int *changed,
                                   float eps, float sea, const nz_geom &g, int zlo, int zhi, int first, int pass, int sweeps) {
    if (g.or1 <= g.or0 || g.cols <= 0) return NZ_OK;
    const dim3 grid(tiles_x(g.cols), tiles_z(g.or1 - g.or0), 1);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(w_in) | reinterpret_cast<uintptr_t>(w_out);
    const bool vec = (bits & 15) == 0 && g.cols % 4 == 0 && g.pitch % 4 == 0;  // every row starts 16-byte aligned
    const fill_win win{g.pitch, g.cols - 1, zlo, zhi, g.or0, g.or1, first, w_ghost, changed};
    if (first && pass == 0) launch_pass<true, true>(vec, grid, s, h, w_in, w_out, status, flags_in, flags_out, eps, sea, win, pass, sweeps);
    else launch_pass<false, true>(vec, grid, s, h, w_in, w_out, status, flags_in, flags_out, eps, sea, win, pass, sweeps);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fill_round_end(hipStream_t s, float *w, const float *w_work, const int *status, int passes, const nz_geom &g) {
    if (g.or1 <= g.or0 || g.cols <= 0) return NZ_OK;
    NZ_LAUNCH(fill_round_end_kernel, dim3((g.cols + 255) / 256, g.or1 - g.or0), dim3(256), 0, s, w, w_work, status, passes,
              g.pitch, g.cols, g.or0, g.or1);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fill_stripe_finalise(hipStream_t s, float *h, const float *w, float *depth, const int *converged,
                                       const nz_geom &g) {
    if (g.or1 <= g.or0 || g.cols <= 0) return NZ_OK;
    NZ_LAUNCH(fill_stripe_finalise_kernel, dim3((g.cols + 255) / 256, g.or1 - g.or0), dim3(256), 0, s, h, w, depth, converged,
              g.pitch, g.cols, g.or0, g.or1);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fill_finalise(hipStream_t s, float *h, const float *w, float *depth, int *status, size_t n) {
    if (n == 0) return NZ_OK;
    NZ_LAUNCH(fill_finalise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h, w, depth, status, n);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
