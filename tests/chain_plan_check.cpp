// chain_plan_check.cpp -- noize_job_amd/csrc/nz_chain_plan.hpp against a brute-force restatement of the rules it documents.
// A stand-alone host program (tests/test_chain_plan.py builds it with g++ under the address and undefined-behaviour
// sanitizers): for 5 and 9 taps, the three register-tile shapes, five grids and four depth lists it rebuilds every record of
// the plan the slow way -- the item of a grid position by listing each class's positions and runs, the awaited tiles by
// testing EVERY tile of the previous launch against the widened window -- and compares.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../noize_job_amd/csrc/nz_chain_plan.hpp"

static int g_fail = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (g_fail++ < 20) {                  \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);         \
                std::printf("\n");                \
            }                                     \
        }                                         \
    } while (0)

struct rect { int x0, x1, z0, z1; };  // half open
static bool meets(const rect &a, const rect &b) { return a.x0 < b.x1 && b.x0 < a.x1 && a.z0 < b.z1 && b.z0 < a.z1; }

struct launch {
    int T, H, HX, OW, OH, tx, ty, first;
    rect interior(int tile, const nz_chain_key &k) const {
        const int bx = tile % tx, by = tile / tx;
        return {bx * OW, std::min((bx + 1) * OW, k.cols), k.or0 + by * OH, std::min(k.or0 + (by + 1) * OH, k.or1)};
    }
};

static long check_plan(const nz_chain_key &k, const char *what) {
    // the layout, restated
    std::vector<launch> ls;
    bool exists = k.L >= 1 && k.L <= NZ_CHAIN_MAXL;
    int total = 0;
    for (int l = 0; exists && l < k.L; l++) {
        launch a{};
        a.T = k.T[l];
        a.H = a.T * k.O;
        a.HX = (a.H + 3) / 4 * 4;
        a.OW = k.TW - 2 * a.HX;
        a.OH = k.TH - 2 * a.H;
        if (a.T < 1 || a.OW < 1 || a.OH < 1) { exists = false; break; }
        a.tx = (k.cols + a.OW - 1) / a.OW;
        a.ty = (k.or1 - k.or0 + a.OH - 1) / a.OH;
        a.first = total;
        total += a.tx * a.ty;
        ls.push_back(a);
    }
    const nz_chain_layout lay = nz_chain_layout_of(k);
    if (!exists) {
        CHECK(lay.total == 0, "%s: a plan without an interior has %d items", what, lay.total);
        std::vector<nz_chain_item> none(1);
        CHECK(!nz_chain_plan_build(k, none.data()), "%s: a plan without an interior was built", what);
        return 0;
    }
    CHECK(lay.total == total, "%s: total %d, restated %d", what, lay.total, total);
    for (int l = 0; l < k.L; l++)
        CHECK(lay.first[l] == ls[l].first && lay.tiles_x[l] == ls[l].tx && lay.tiles_y[l] == ls[l].ty, "%s: layout of launch %d", what, l);
    CHECK(lay.first[k.L] == total, "%s: first[L]", what);

    // the item of every grid position, by the class rule: per launch, the positions of each class in order; the classes' runs
    // of tiles one after the other in class order, each as long as the class has positions; odd classes backwards
    std::vector<int> item_of(total, -1), launch_of(total, -1);
    for (int l = 0; l < k.L; l++) {
        const int f0 = ls[l].first, f1 = f0 + ls[l].tx * ls[l].ty;
        int run = 0;
        for (int c = 0; c < 8; c++) {
            std::vector<int> pos;
            for (int vb = f0; vb < f1; vb++)
                if (vb % 8 == c) pos.push_back(vb);
            for (size_t j = 0; j < pos.size(); j++) {
                const int tile = run + (int)((c & 1) ? pos.size() - 1 - j : j);
                item_of[pos[j]] = f0 + tile;
                launch_of[pos[j]] = l;
            }
            run += (int)pos.size();
        }
    }
    // the awaited tiles, restated: does any tile want more than 3 x 3?
    std::vector<std::set<int>> awaited(total);
    bool fits = true;
    for (int vb = 0; vb < total; vb++) {
        const int l = launch_of[vb];
        if (l == 0) continue;
        const launch &a = ls[l], &p = ls[l - 1];
        const rect in = a.interior(item_of[vb] - a.first, k);
        const int Hw = std::max(a.H, p.H), HXw = std::max(a.HX, p.HX);
        // (the interior's nominal extent: a clipped tile waits as an unclipped one would, the window is clipped to the grid)
        const int ox0 = in.x0, oz0 = in.z0;
        const rect w = {std::max(ox0 - HXw, 0), std::min(ox0 + a.OW + HXw, k.cols), std::max(oz0 - Hw, k.or0), std::min(oz0 + a.OH + Hw, k.or1)};
        int bx0 = 1 << 30, bx1 = -1, by0 = 1 << 30, by1 = -1;
        for (int t = 0; t < p.tx * p.ty; t++)
            if (meets(p.interior(t, k), w)) {
                awaited[vb].insert(p.first + t);
                bx0 = std::min(bx0, t % p.tx); bx1 = std::max(bx1, t % p.tx);
                by0 = std::min(by0, t / p.tx); by1 = std::max(by1, t / p.tx);
            }
        CHECK(!awaited[vb].empty(), "%s: position %d waits for nobody", what, vb);
        if (bx1 - bx0 + 1 > NZ_CHAIN_MAXDEP || by1 - by0 + 1 > NZ_CHAIN_MAXDEP) fits = false;
    }

    std::vector<nz_chain_item> plan((size_t)total + 1);
    const nz_chain_item guard = {-7, -7, -7, -7, -7, -7, -7, -7};
    plan[total] = guard;
    const bool built = nz_chain_plan_build(k, plan.data());
    CHECK(built == fits, "%s: built %d, the restated windows fit 3 x 3: %d", what, (int)built, (int)fits);
    CHECK(plan[total].ox0 == -7 && plan[total].stride == -7, "%s: wrote past the plan", what);
    if (!built || !fits) return 0;

    std::vector<int> seen(total, 0);
    for (int vb = 0; vb < total; vb++) {
        const nz_chain_item &it = plan[vb];
        const int l = launch_of[vb];
        const launch &a = ls[l];
        CHECK(it.item == item_of[vb], "%s: position %d is item %d, restated %d", what, vb, it.item, item_of[vb]);
        if (it.item < 0 || it.item >= total) continue;
        seen[it.item]++;
        const int tile = it.item - a.first;
        CHECK((it.tl >> 16) == l && (it.tl & 0xffff) == a.T, "%s: position %d launch / depth", what, vb);
        CHECK(it.ox0 == tile % a.tx * a.OW && it.oz0 == k.or0 + tile / a.tx * a.OH, "%s: position %d origin", what, vb);
        if (l == 0) {
            CHECK(it.ny == 0, "%s: position %d of launch 0 waits", what, vb);
            continue;
        }
        CHECK(it.nx >= 1 && it.nx <= 3 && it.ny >= 1 && it.ny <= 3, "%s: position %d awaits %d x %d", what, vb, it.nx, it.ny);
        std::set<int> got;
        for (int r = 0; r < it.ny; r++)
            for (int c = 0; c < it.nx; c++) got.insert(it.dep0 + r * it.stride + c);
        CHECK((int)got.size() == it.nx * it.ny && got == awaited[vb], "%s: position %d (item %d) awaits %zu flags, restated %zu", what, vb,
              it.item, got.size(), awaited[vb].size());
    }
    for (int i = 0; i < total; i++) CHECK(seen[i] == 1, "%s: item %d appears %d times", what, i, seen[i]);
    return total;
}

int main() {
    const int shapes[3][2] = {{512, 8}, {512, 4}, {1024, 2}};  // threads x rows per thread: 128-, 64- and 64-row tiles
    const int grids[5][3] = {{352, 0, 352}, {1000, 0, 360}, {301, 0, 263}, {4096, 0, 4096}, {1000, 37, 397}};  // cols, or0, or1
    const int lists[4][5] = {{4, 4, 4, 4, 5}, {3, 4, 4, 5, 0}, {2, 9, 8, 0, 0}, {2, 1, 1, 0, 0}};               // L, depths
    long plans = 0, items = 0;
    for (int taps : {5, 9})
        for (const auto &sh : shapes)
            for (const auto &g : grids)
                for (const auto &ts : lists) {
                    nz_chain_key k{};
                    k.O = (taps - 1) / 2;
                    k.TH = sh[0] / 32 * sh[1];
                    k.TW = 128;
                    k.cols = g[0];
                    k.or0 = g[1];
                    k.or1 = g[2];
                    k.L = ts[0];
                    for (int l = 0; l < k.L; l++) k.T[l] = ts[1 + l];
                    char what[128];
                    std::snprintf(what, sizeof what, "%d taps, %d x %d threads, %d cols x rows [%d, %d), depths %d %d %d %d", taps, sh[0],
                                  sh[1], g[0], g[1], g[2], ts[1], ts[2], ts[3], ts[4]);
                    const long n = check_plan(k, what);
                    plans += n > 0;
                    items += n;
                }
    // the key: equal only with every field and every depth equal; depths beyond L do not count
    nz_chain_key a{}, b{};
    a.O = b.O = 2; a.TH = b.TH = 128; a.TW = b.TW = 128; a.cols = b.cols = 352; a.or1 = b.or1 = 352; a.L = b.L = 2;
    a.T[0] = b.T[0] = 4; a.T[1] = b.T[1] = 5; a.T[2] = 7;
    CHECK(nz_chain_key_equal(a, b), "equal keys differ");
    b.T[1] = 4;
    CHECK(!nz_chain_key_equal(a, b), "keys of different depths are equal");
    b = a; b.or0 = 1;
    CHECK(!nz_chain_key_equal(a, b), "keys of different windows are equal");
    // refusals
    nz_chain_key bad = a;
    bad.L = 0;
    CHECK(nz_chain_layout_of(bad).total == 0, "L = 0 has a layout");
    bad = a; bad.L = NZ_CHAIN_MAXL + 1;
    CHECK(nz_chain_layout_of(bad).total == 0, "L = 9 has a layout");
    bad = a; bad.or1 = bad.or0;
    CHECK(nz_chain_layout_of(bad).total == 0, "an empty window has a layout");
    if (g_fail) {
        std::printf("chain_plan_check: %d failures\n", g_fail);
        return 1;
    }
    std::printf("%ld plans, %ld items\nchain_plan_check: ok\n", plans, items);
    return plans >= 40 ? 0 : 1;
}
