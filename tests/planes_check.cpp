// planes_check.cpp -- stand-alone check of noize_job_amd/csrc/nz_planes.hpp (the stripe geometry and aliasing helpers of the
// terrain entry points).  Plain host C++, built and run by tests/test_planes_header.py under the address and undefined-
// behaviour sanitizers; exit status 0 = every check held.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <iterator>

#include "../noize_job_amd/csrc/nz_planes.hpp"

static char last_error[256];
void nz_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            fprintf(stderr, "%s:%d: %s  (last error: \"%s\")\n", __FILE__, __LINE__, #cond, last_error); \
            return 1;                                                                                \
        }                                                                                            \
    } while (0)

// ---- the window of launch j: nz_stripe_window against the two expressions it replaced ----------------------------------
static int check_windows() {
    long accepted = 0, top = 0, bottom = 0, interior = 0, whole = 0, empty = 0;
    const int cols = 5;
    for (int grows = 1; grows <= 10; grows++)
    for (int rows = 1; rows <= 10; rows++)
    for (int own0 = 0; own0 <= rows; own0++)
    for (int own1 = own0; own1 <= rows; own1++)
    for (int grow0 = -rows; grow0 <= grows; grow0++)
    for (int pitch : {0, cols + 3}) {
        const nz_stripe s{cols, rows, grow0, grows, own0, own1, pitch};
        const nz_stripe *st = &s;
        for (int radius = 2; radius <= 3; radius++)
        for (int n = 1; n <= 3; n++) {
            if (nz_check_stripe(st, radius * n) != NZ_OK) continue;
            accepted++;
            const bool at_top = own0 + grow0 == 0, at_bottom = own1 + grow0 == grows;
            if (own0 == own1) empty++;
            else if (at_top && at_bottom) whole++;
            else if (at_top) top++;
            else if (at_bottom) bottom++;
            else interior++;
            for (int j = 0; j < n; j++) {
                int or0, or1;
                nz_stripe_window(s, radius * (n - 1 - j), &or0, &or1);
                CHECK(0 <= or0 && or0 <= or1 && or1 <= rows);
                {  // nz_hydraulic_stripe before the helper; g0 = nz_geom_from_stripe(*st), whose zc0 is max(-grow0, 0)
                    struct { int zc0; } g0{-st->grow0 > 0 ? -st->grow0 : 0};
                    const int glo = g0.zc0 > -st->grow0 ? g0.zc0 : -st->grow0, ghi = st->grows - st->grow0;
                    const int widen = radius * (n - 1 - j);
                    const int g_or0 = st->own0 - widen > glo ? st->own0 - widen : glo;
                    const int g_or1 = st->own1 + widen < ghi ? st->own1 + widen : ghi;
                    CHECK(or0 == g_or0 && or1 == g_or1);
                }
                {  // nz_fluvial_stripe before the helper
                    const int zlo = -st->grow0, zhi = st->grows - 1 - st->grow0;
                    const int widen = radius * (n - 1 - j);
                    const int g_or0 = st->own0 - widen > zlo ? st->own0 - widen : zlo;
                    const int g_or1 = st->own1 + widen < zhi + 1 ? st->own1 + widen : zhi + 1;
                    CHECK(or0 == g_or0 && or1 == g_or1);
                    CHECK(nz_stripe_grid_lo(s) == zlo && nz_stripe_grid_hi(s) - 1 == zhi);
                }
            }
        }
    }
    CHECK(top > 0 && bottom > 0 && interior > 0 && whole > 0 && empty > 0);
    printf("windows: %ld accepted stripes (top %ld, bottom %ld, interior %ld, whole grid %ld, no owned rows %ld)\n", accepted,
           top, bottom, interior, whole, empty);
    return 0;
}

// ---- pitch, span, plane size ---------------------------------------------------------------------------------------------
static int check_sizes() {
    // {cols, rows, grow0, grows, own0, own1, pitch}
    const nz_stripe tight{7, 4, 0, 4, 0, 4, 0}, same{7, 4, 0, 4, 0, 4, 7}, padded{7, 4, 0, 4, 0, 4, 10}, one_row{7, 1, 0, 1, 0, 1, 10};
    CHECK(nz_stripe_pitch(tight) == 7 && nz_stripe_span(tight) == 28 && nz_stripe_plane_floats(&tight) == 28);
    CHECK(nz_stripe_pitch(same) == 7 && nz_stripe_span(same) == 28 && nz_stripe_plane_floats(&same) == 28);
    CHECK(nz_stripe_pitch(padded) == 10 && nz_stripe_span(padded) == 37 && nz_stripe_plane_floats(&padded) == 40);
    CHECK(nz_stripe_span(one_row) == 7 && nz_stripe_plane_floats(&one_row) == 10);
    const nz_stripe no_rows{7, 0, 0, 4, 0, 0, 0}, neg_rows{7, -1, 0, 4, 0, 0, 0}, no_cols{0, 4, 0, 4, 0, 4, 0},
        neg_cols{-3, 4, 0, 4, 0, 4, 0}, neg_pitch{7, 4, 0, 4, 0, 4, -1};
    CHECK(nz_stripe_plane_floats(nullptr) == 0);
    for (const nz_stripe *st : {&no_rows, &neg_rows, &no_cols, &neg_cols, &neg_pitch}) CHECK(nz_stripe_plane_floats(st) == 0);
    return 0;
}

// ---- the overlap predicate -----------------------------------------------------------------------------------------------
static float arena[40 * 32];

static int check_overlap() {
    const float *a = arena + 100;
    const struct { const float *b; size_t nb; bool want; const char *what; } cases[] = {
        {a + 64, 16, false, "apart"},         {a + 16, 16, false, "touching behind"}, {a - 16, 16, false, "touching in front"},
        {a + 15, 16, true, "one float behind"}, {a - 15, 16, true, "one float in front"}, {a + 4, 4, true, "nested"},
        {a - 4, 40, true, "nesting"},         {a, 16, true, "identical"},              {nullptr, 16, false, "NULL"}};
    for (const auto &c : cases) {
        snprintf(last_error, sizeof last_error, "case: %s", c.what);
        CHECK(nz_planes_overlap(a, 16, c.b, c.nb) == c.want && nz_planes_overlap(c.b, c.nb, a, 16) == c.want);
        CHECK(nz_bytes_overlap(a, 64, c.b, c.nb * 4) == c.want && nz_bytes_overlap(c.b, c.nb * 4, a, 64) == c.want);
    }
    CHECK(!nz_planes_overlap(nullptr, 16, nullptr, 16) && !nz_bytes_overlap(nullptr, 4, nullptr, 4));
    // a word of 4 bytes against a plane, as nz_fill_stripe checks `changed`: inside the last float, just behind it
    CHECK(nz_bytes_overlap(a + 15, 4, a, 64) && !nz_bytes_overlap(a + 16, 4, a, 64));
    CHECK(nz_bytes_overlap((const char *)a + 63, 4, a, 64) && !nz_bytes_overlap((const char *)a - 4, 4, a, 64));
    return 0;
}

// ---- nz_require_disjoint on the layouts of the two stripe entries ---------------------------------------------------------
// planes of a 4 x 5 stripe at pitch 8: 29 floats touched, 32 floats apart
constexpr size_t SPAN = 29, PLANE = 32;
static float *slot(int i) { return arena + (size_t)i * PLANE; }

// the planes of a nz_hydraulic_stripe call, as the entry lists them
struct hyd_call {
    const float *height_in;
    float *height_out;
    const float *rainMap, *hardness;
    float *wear, *deposits, *work;
    const float *state_in[6];
    float *state_out[6];
    bool first;
    int n;
};
static hyd_call hyd_clean() {
    hyd_call c{slot(0), slot(1), slot(2), slot(3), slot(4), slot(5), slot(6), {}, {}, false, 2};  // work: slots 6..12
    for (int i = 0; i < 6; i++) c.state_in[i] = slot(13 + i), c.state_out[i] = slot(19 + i);
    return c;
}
static int32_t hyd_check(const hyd_call &c) {
    nz_named_plane reads[3 + 6] = {{"height_in", c.height_in, SPAN}, {"rainMap", c.rainMap, SPAN}, {"hardness", c.hardness, SPAN}};
    nz_named_plane writes[4 + 6] = {{"height_out", c.height_out, SPAN}, {"wear", c.wear, SPAN}, {"deposits", c.deposits, SPAN},
                                    {"work", c.n > 1 ? c.work : nullptr, 7 * PLANE}};
    for (int i = 0; i < 6; i++) {
        reads[3 + i] = {"state_in", c.first ? nullptr : c.state_in[i], SPAN};
        writes[4 + i] = {"state_out", c.state_out[i], SPAN};
    }
    last_error[0] = 0;
    return nz_require_disjoint(writes, std::size(writes), reads, std::size(reads));
}

// ... and of a nz_fluvial_stripe call
struct flu_call {
    const float *height_in;
    float *height_out, *drainage_out, *work;
    const float *drainageIn, *rainMap, *hardness, *upliftMap;
    int n;
};
static flu_call flu_clean() { return flu_call{slot(0), slot(1), slot(2), slot(3), slot(5), slot(6), slot(7), slot(8), 2}; }  // work: 3, 4
static int32_t flu_check(const flu_call &c) {
    const nz_named_plane reads[] = {{"height_in", c.height_in, SPAN},
                                    {"drainageIn", c.drainageIn, SPAN},
                                    {"rainMap", c.rainMap, SPAN},
                                    {"hardness", c.hardness, SPAN},
                                    {"upliftMap", c.upliftMap, SPAN}};
    const nz_named_plane writes[] = {{"height_out", c.height_out, SPAN},
                                     {"drainage_out", c.drainage_out, SPAN},
                                     {"work", c.n > 1 ? c.work : nullptr, 2 * PLANE}};
    last_error[0] = 0;
    return nz_require_disjoint(writes, std::size(writes), reads, std::size(reads));
}

#define REFUSED(call, text) CHECK((call) == NZ_ERR_INVALID && strcmp(last_error, text) == 0)

static int check_disjoint() {
    hyd_call h = hyd_clean();
    CHECK(hyd_check(h) == NZ_OK && last_error[0] == 0);
    // the clashes tests/test_gpu_hydraulic_stripe.py provokes
    h.height_out = const_cast<float *>(h.height_in) + 8;  // one row further
    REFUSED(hyd_check(h), "height_out overlaps height_in");
    h = hyd_clean(), h.wear = h.work + 100;
    REFUSED(hyd_check(h), "wear overlaps work");
    h = hyd_clean();
    for (int i = 0; i < 6; i++) h.state_in[i] = h.state_out[i];
    REFUSED(hyd_check(h), "state_out overlaps state_in");
    h.first = true;  // ... which a first call does not read
    CHECK(hyd_check(h) == NZ_OK);
    // the mask clashes of tests/test_gpu_hydraulic_ex.py, on the stripe entry's names
    h = hyd_clean(), h.wear = const_cast<float *>(h.height_in);
    REFUSED(hyd_check(h), "wear overlaps height_in");
    h = hyd_clean(), h.deposits = const_cast<float *>(h.rainMap);
    REFUSED(hyd_check(h), "deposits overlaps rainMap");
    h = hyd_clean(), h.deposits = h.wear;
    REFUSED(hyd_check(h), "wear overlaps deposits");
    // without `work` (one iteration) a plane may lie where it would be
    h = hyd_clean(), h.wear = h.work + 100, h.n = 1;
    CHECK(hyd_check(h) == NZ_OK);
    // the last launch of a `last` call of one iteration has five NULL state_out planes
    h = hyd_clean(), h.n = 1;
    for (int i = 1; i < 6; i++) h.state_out[i] = nullptr;
    CHECK(hyd_check(h) == NZ_OK);
    // planes that merely touch are apart; one float less is a clash
    h = hyd_clean(), h.height_out = const_cast<float *>(h.height_in) + SPAN;
    CHECK(hyd_check(h) == NZ_OK);
    h.height_out -= 1;
    REFUSED(hyd_check(h), "height_out overlaps height_in");
    // two clashes: the earlier write is reported, and for one write its reads before the writes behind it
    h = hyd_clean(), h.deposits = h.work, h.height_out = const_cast<float *>(h.hardness);
    REFUSED(hyd_check(h), "height_out overlaps hardness");
    h = hyd_clean(), h.wear = h.state_out[2], h.rainMap = h.wear;
    REFUSED(hyd_check(h), "wear overlaps rainMap");
    h = hyd_clean(), h.state_out[5] = h.work + 6 * PLANE, h.state_out[0] = h.state_out[1];
    REFUSED(hyd_check(h), "work overlaps state_out");
    // reads may alias each other
    h = hyd_clean(), h.rainMap = h.hardness = h.height_in;
    for (int i = 0; i < 6; i++) h.state_in[i] = h.height_in;
    CHECK(hyd_check(h) == NZ_OK);

    flu_call f = flu_clean();
    CHECK(flu_check(f) == NZ_OK && last_error[0] == 0);
    // the clashes tests/test_gpu_fluvial_stripe.py provokes
    f.height_out = const_cast<float *>(f.height_in) + 8;
    REFUSED(flu_check(f), "height_out overlaps height_in");
    f = flu_clean(), f.drainage_out = f.height_out + 8;  // (the earlier write names the pair)
    REFUSED(flu_check(f), "height_out overlaps drainage_out");
    f = flu_clean(), f.drainageIn = f.drainage_out + 8;
    REFUSED(flu_check(f), "drainage_out overlaps drainageIn");
    f = flu_clean(), f.rainMap = f.work + 40;
    REFUSED(flu_check(f), "work overlaps rainMap");
    f.n = 1;
    CHECK(flu_check(f) == NZ_OK);
    // two clashes: height_out against a read comes before drainage_out against anything
    f = flu_clean(), f.drainage_out = f.work + PLANE, f.upliftMap = f.height_out;
    REFUSED(flu_check(f), "height_out overlaps upliftMap");
    f = flu_clean(), f.drainage_out = f.work + PLANE, f.hardness = f.drainage_out;
    REFUSED(flu_check(f), "drainage_out overlaps hardness");
    // reads may alias each other
    f = flu_clean(), f.drainageIn = f.rainMap = f.hardness = f.upliftMap = f.height_in;
    CHECK(flu_check(f) == NZ_OK);
    return 0;
}

int main() {
    if (check_windows() || check_sizes() || check_overlap() || check_disjoint()) return 1;
    puts("planes_check: ok");
    return 0;
}
