// nz_terrain_stages.cpp -- the extern "C" entry points of the terrain stages the reference does not have (grid hydraulic
// erosion, fluvial erosion, depression filling, drainage area, watershed, stream order, implicit fluvial erosion, hillslope diffusion,
// multiple-flow drainage and multiple-flow implicit fluvial erosion, resampling; include/noize_hip.h): tile, batch,
// read/write-pair and row-stripe forms.  The stripe geometry and the aliasing checks they share are in nz_planes.hpp.
#include <atomic>
#include <cmath>
#include <iterator>
#include <utility>

#include "nz_internal.hpp"
#include "nz_tile64.hpp"  // the tile counts of the fill and drainage launches

// Launch j of a series of n that ping-pongs between two plane sets writes set (n-1-j) & 1, so that the last launch lands in
// set 0.  The stripe entries: 0 = the caller's output planes, 1 = `work`.
static int pingpong_set(int n, int j) { return (n - 1 - j) & 1; }

// The height ping-pong of the in-place series: `iterations` >= 1 launches, each reading *cur and writing *nxt before the
// caller swaps the two.  *cur starts at h0, which holds the input, so the result lands in h0 when `iterations` is even and
// in h1 when it is odd (*in_h1).  keep_h0: the caller wants it in h0 whatever the count, and an odd count copies h0 to h1
// (n floats) first and starts there.
static int32_t height_pingpong(nz_ctx *ctx, float *h0, float *h1, size_t n, int iterations, bool keep_h0, float **cur,
                               float **nxt, bool *in_h1) {
    *cur = h0, *nxt = h1;
    *in_h1 = !keep_h0 && (iterations & 1);
    if (keep_h0 && (iterations & 1)) {
        NZ_TRY(nz_launch_copy(ctx->stream, h1, h0, n));
        std::swap(*cur, *nxt);
    }
    return NZ_OK;
}

// ---------------------------------------------------------------------------------------------
// grid hydraulic erosion with sediment transport (new-framework feature, include/noize_hip.h, nz_hydraulic.hip)
// ---------------------------------------------------------------------------------------------
// work planes of count * res^2 floats each: 0 the final water, 1-6 and 7-12 the state sets {d, s, fN, fS, fE, fW} the
// launches ping-pong between, 13 the in-place forms' second height plane
constexpr int HYD_PLANES = 14;

extern "C" size_t nz_hydraulic_erosion_work_floats(int32_t resolution, int32_t count) {
    return resolution > 0 && count > 0 ? (size_t)HYD_PLANES * resolution * resolution * count : 0;
}

// the scalars of a nz_hydraulic_desc as the launches take them
static int32_t check_hydraulic(const nz_hydraulic_desc &d, nz_hydraulic_params *k) {
    NZ_REQUIRE(d.iterations >= 0, "iterations %d < 0", d.iterations);
    const struct { const char *name; float v; float lo, hi; } args[] = {
        {"initialWater", d.initialWater, 0.0f, INFINITY}, {"rain", d.rain, 0.0f, INFINITY},
        {"evaporation", d.evaporation, 0.0f, 1.0f},       {"capacity", d.capacity, 0.0f, INFINITY},
        {"dissolve", d.dissolve, 0.0f, 1.0f},             {"deposit", d.deposit, 0.0f, 1.0f},
        {"minTilt", d.minTilt, 0.0f, INFINITY}};
    for (const auto &a : args) {
        NZ_REQUIRE(std::isfinite(a.v), "%s is not finite", a.name);
        if (a.hi == INFINITY) NZ_REQUIRE(a.v >= a.lo, "%s %g < 0", a.name, (double)a.v);
        else NZ_REQUIRE(a.v >= a.lo && a.v <= a.hi, "%s %g outside [0, 1]", a.name, (double)a.v);
    }
    *k = nz_hydraulic_params{d.initialWater, d.rain, 1.0f - d.evaporation, d.capacity, d.dissolve, d.deposit, d.minTilt};
    return NZ_OK;
}

// ... and its options (border, maps, masks)
static int32_t hydraulic_ex_of(const nz_hydraulic_desc &d, nz_hydraulic_ex *ex) {
    NZ_REQUIRE(d.border == NZ_HYDRAULIC_BORDER_CLOSED || d.border == NZ_HYDRAULIC_BORDER_OPEN, "border %d is not a mode",
               d.border);
    *ex = nz_hydraulic_ex{d.border == NZ_HYDRAULIC_BORDER_OPEN, d.rainMap, d.hardness, d.wear, d.deposits};
    return NZ_OK;
}

// The masks of a tile-shaped call.  h0 / h1: the height plane(s) the call reads or writes (h1 may be NULL), n floats each
// like every plane of the desc; the masks may overlap none of them, nor the maps, each other or `work`
static int32_t check_hydraulic_masks(const nz_hydraulic_desc &d, const float *h0, const float *h1, const float *work,
                                     size_t n) {
    const nz_named_plane masks[] = {{"wear", d.wear, n}, {"deposits", d.deposits, n}};
    const nz_named_plane others[] = {{"src", h0, n}, {"the write plane", h1, n}, {"work", work, (size_t)HYD_PLANES * n},
                                     {"rainMap", d.rainMap, n}, {"hardness", d.hardness, n}};
    for (const auto &m : masks)
        for (const auto &o : others) NZ_REQUIRE(!nz_planes_overlap(m.p, n, o.p, o.floats), "%s overlaps %s", m.name, o.name);
    NZ_REQUIRE(!nz_planes_overlap(d.wear, n, d.deposits, n), "wear overlaps deposits");
    return NZ_OK;
}

// The body of every tile-shaped entry behind its NULL checks: the desc's checks, then desc.iterations launches on `count`
// tiles.  The height ping-pongs between h0 and h1 (height_pingpong); h1 NULL: the in-place forms, which keep the result in
// h0 and take work plane 13 as h1.  The state ping-pongs between the two sets of `work`.  Ends with the final water in work plane 0 (initialWater itself when there is
// no iteration).  The masks are written by the first launch, or cleared here when there is none.
static int32_t hydraulic_series(nz_ctx *ctx, float *h0, float *h1, float *work, int res, int count, const nz_hydraulic_desc &d,
                                nz_handle *out, bool *in_h1) {
    const size_t n = (size_t)res * res * count;
    const int iterations = d.iterations;
    nz_hydraulic_params k;
    NZ_TRY(check_hydraulic(d, &k));
    nz_hydraulic_ex ex;
    NZ_TRY(hydraulic_ex_of(d, &ex));
    NZ_TRY(check_hydraulic_masks(d, h0, h1, work, n));
    const bool keep_h0 = !h1;
    if (keep_h0) h1 = work + (size_t)(HYD_PLANES - 1) * n;
    nz_ctx_handle_rides(ctx, out != nullptr);  // (the last launch below is armed)
    if (iterations == 0) {
        *in_h1 = false;
        if (ex.wear) NZ_TRY(nz_launch_fill(ctx->stream, ex.wear, n, 0.0f));
        if (ex.deposits) NZ_TRY(nz_launch_fill(ctx->stream, ex.deposits, n, 0.0f));
        nz_ctx_arm_last_launch(ctx);
        return nz_launch_fill(ctx->stream, work, n, k.initial_water);
    }
    float *cur, *nxt;
    NZ_TRY(height_pingpong(ctx, h0, h1, n, iterations, keep_h0, &cur, &nxt, in_h1));
    nz_hydraulic_planes sets[2];
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 6; i++) sets[j].in[i] = sets[j].out[i] = work + (size_t)(1 + 6 * j + i) * n;
    for (int it = 0; it < iterations; it++) {
        const int first = it == 0, last = it == iterations - 1;
        nz_hydraulic_planes p;
        for (int i = 0; i < 6; i++) {
            p.in[i] = sets[it & 1].in[i];
            p.out[i] = last ? (i == 0 ? work : nullptr) : sets[(it + 1) & 1].out[i];
        }
        if (last) nz_ctx_arm_last_launch(ctx);
        NZ_TRY(nz_launch_hydraulic(ctx->stream, cur, nxt, p, k, res, count, first, last, &ex));
        std::swap(cur, nxt);
    }
    return NZ_OK;
}

// every in-place entry: the old ones come with a desc of their scalars and every option off
static int32_t hydraulic_stage_impl(nz_ctx *ctx, float *src, float *work, const nz_hydraulic_desc *desc, int32_t resolution,
                                    int32_t count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    NZ_REQUIRE(src && work, "src/work is NULL");
    NZ_REQUIRE(desc, "desc is NULL");
    bool in_h1;
    NZ_TRY(hydraulic_series(ctx, src, nullptr, work, resolution, count, *desc, out, &in_h1));
    return nz_ctx_finish(ctx, out);
}

static int32_t hydraulic_rw_impl(nz_ctx *ctx, nz_rw_tile *tile, float *work, const nz_hydraulic_desc *desc, nz_handle dep,
                                 nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_rw(tile));
    NZ_REQUIRE(work, "work is NULL");
    NZ_REQUIRE(desc, "desc is NULL");
    bool in_h1;
    NZ_TRY(hydraulic_series(ctx, tile->read, tile->write, work, tile->resolution, tile->count, *desc, out, &in_h1));
    rw_swap(tile, in_h1);
    return nz_ctx_finish(ctx, out);
}

static nz_hydraulic_desc hydraulic_plain_desc(int32_t iterations, float initialWater, float rain, float evaporation,
                                              float capacity, float dissolve, float deposit, float minTilt) {
    return nz_hydraulic_desc{iterations, initialWater, rain,    evaporation, capacity, dissolve, deposit,
                             minTilt,    NZ_HYDRAULIC_BORDER_CLOSED, nullptr, nullptr, nullptr, nullptr};
}

extern "C" int32_t nz_hydraulic_erosion_stage(nz_ctx *ctx, float *src, float *work, int32_t iterations, float initialWater,
                                              float rain, float evaporation, float capacity, float dissolve, float deposit,
                                              float minTilt, int32_t resolution, nz_handle dep, nz_handle *out) {
    const nz_hydraulic_desc d =
        hydraulic_plain_desc(iterations, initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt);
    return hydraulic_stage_impl(ctx, src, work, &d, resolution, 1, dep, out);
}

extern "C" int32_t nz_hydraulic_erosion_stage_batch(nz_ctx *ctx, float *src, float *work, int32_t iterations,
                                                    float initialWater, float rain, float evaporation, float capacity,
                                                    float dissolve, float deposit, float minTilt, int32_t resolution,
                                                    int32_t count, nz_handle dep, nz_handle *out) {
    const nz_hydraulic_desc d =
        hydraulic_plain_desc(iterations, initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt);
    return hydraulic_stage_impl(ctx, src, work, &d, resolution, count, dep, out);
}

extern "C" int32_t nz_hydraulic_erosion_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, int32_t iterations,
                                                 float initialWater, float rain, float evaporation, float capacity,
                                                 float dissolve, float deposit, float minTilt, nz_handle dep,
                                                 nz_handle *out) {
    const nz_hydraulic_desc d =
        hydraulic_plain_desc(iterations, initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt);
    return hydraulic_rw_impl(ctx, tile, work, &d, dep, out);
}

extern "C" int32_t nz_hydraulic_erosion_ex(nz_ctx *ctx, float *src, float *work, const nz_hydraulic_desc *desc,
                                           int32_t resolution, nz_handle dep, nz_handle *out) {
    return hydraulic_stage_impl(ctx, src, work, desc, resolution, 1, dep, out);
}

extern "C" int32_t nz_hydraulic_erosion_ex_batch(nz_ctx *ctx, float *src, float *work, const nz_hydraulic_desc *desc,
                                                 int32_t resolution, int32_t count, nz_handle dep, nz_handle *out) {
    return hydraulic_stage_impl(ctx, src, work, desc, resolution, count, dep, out);
}

extern "C" int32_t nz_hydraulic_erosion_ex_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, const nz_hydraulic_desc *desc,
                                              nz_handle dep, nz_handle *out) {
    return hydraulic_rw_impl(ctx, tile, work, desc, dep, out);
}

// ---- the stripe form (include/noize_hip.h): n iterations of one call on a row stripe, one launch each ----
constexpr int HYD_STRIPE_RADIUS = 3;  // ghost rows one iteration reads beyond the rows it produces (nz_hydraulic.hip's HR)
constexpr int HYD_STRIPE_PLANES = 7;  // the height and the six state planes

extern "C" int32_t nz_hydraulic_stripe_halo_rows(int32_t iterations) {
    return iterations > 0 ? HYD_STRIPE_RADIUS * iterations : 0;
}

extern "C" size_t nz_hydraulic_stripe_work_floats(const nz_stripe *st, int32_t iterations) {
    return iterations > 1 ? (size_t)HYD_STRIPE_PLANES * nz_stripe_plane_floats(st) : 0;
}

extern "C" int32_t nz_hydraulic_stripe(nz_ctx *ctx, const float *height_in, float *height_out, const float *const *state_in,
                                       float *const *state_out, float *work, const nz_stripe *st,
                                       const nz_hydraulic_desc *desc, int32_t first, int32_t last, nz_handle dep,
                                       nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(desc, "desc is NULL");
    const int n = desc->iterations;
    NZ_REQUIRE(n >= 1, "iterations %d < 1", n);
    nz_hydraulic_params k;
    NZ_TRY(check_hydraulic(*desc, &k));
    nz_hydraulic_ex ex;
    NZ_TRY(hydraulic_ex_of(*desc, &ex));
    NZ_REQUIRE(n <= INT32_MAX / HYD_STRIPE_RADIUS, "iterations %d out of range", n);
    NZ_TRY(nz_check_stripe(st, HYD_STRIPE_RADIUS * n));
    NZ_REQUIRE(height_in && height_out, "height_in/height_out is NULL");
    NZ_REQUIRE(first || state_in, "state_in is NULL");
    NZ_REQUIRE(state_out, "state_out is NULL");
    NZ_REQUIRE(n == 1 || work, "work is NULL");
    for (int i = 0; i < 6; i++) {
        NZ_REQUIRE(first || state_in[i], "state_in[%d] is NULL", i);
        // the last launch of a `last` call writes the water only; the launches before it ping-pong through all six
        NZ_REQUIRE(state_out[i] || (last && n == 1 && i > 0), "state_out[%d] is NULL", i);
    }
    const size_t span = nz_stripe_span(*st), plane = nz_stripe_plane_floats(st);
    nz_named_plane reads[3 + 6] = {{"height_in", height_in, span}, {"rainMap", desc->rainMap, span},
                                   {"hardness", desc->hardness, span}};
    nz_named_plane writes[4 + 6] = {{"height_out", height_out, span}, {"wear", desc->wear, span},
                                    {"deposits", desc->deposits, span},
                                    {"work", n > 1 ? work : nullptr, HYD_STRIPE_PLANES * plane}};
    nz_hydraulic_planes sets[2];  // pingpong_set
    float *hs[2] = {height_out, work};
    for (int i = 0; i < 6; i++) {
        reads[3 + i] = {"state_in", first ? nullptr : state_in[i], span};
        writes[4 + i] = {"state_out", state_out[i], span};
        sets[0].in[i] = sets[0].out[i] = state_out[i];
        sets[1].in[i] = sets[1].out[i] = n > 1 ? work + (size_t)(1 + i) * plane : nullptr;
    }
    NZ_TRY(nz_require_disjoint(writes, std::size(writes), reads, std::size(reads)));
    nz_geom g = nz_geom_from_stripe(*st);
    nz_ctx_handle_rides(ctx, out != nullptr);
    for (int j = 0; j < n; j++) {
        const int to = pingpong_set(n, j);
        nz_stripe_window(*st, HYD_STRIPE_RADIUS * (n - 1 - j), &g.or0, &g.or1);
        nz_hydraulic_planes p;
        for (int i = 0; i < 6; i++) {
            p.in[i] = j == 0 ? (first ? nullptr : state_in[i]) : sets[to ^ 1].in[i];
            p.out[i] = sets[to].out[i];
        }
        if (j == n - 1) nz_ctx_arm_last_launch(ctx);
        NZ_TRY(nz_launch_hydraulic_stripe(ctx->stream, j == 0 ? height_in : hs[to ^ 1], hs[to], p, k, g, st->own0, st->own1,
                                          first && j == 0, last && j == n - 1, ex));
    }
    return nz_ctx_finish(ctx, out);
}

// ---------------------------------------------------------------------------------------------
// stream-power fluvial erosion with drainage area (new-framework feature, include/noize_hip.h, nz_fluvial.hip)
// ---------------------------------------------------------------------------------------------
// work planes of count * res^2 floats each: 0 and 1 the drainage planes the launches ping-pong between -- in such an order
// that the last launch writes plane 0 -- and 2 the in-place forms' second height plane
constexpr int FLU_PLANES = 3;

extern "C" size_t nz_fluvial_erosion_work_floats(int32_t resolution, int32_t count) {
    return resolution > 0 && count > 0 ? (size_t)FLU_PLANES * resolution * resolution * count : 0;
}

// the scalars of a nz_fluvial_desc as the launches take them
static int32_t check_fluvial(const nz_fluvial_desc *d, nz_fluvial_params *k) {
    NZ_REQUIRE(d, "desc is NULL");
    NZ_REQUIRE(d->iterations >= 0, "iterations %d < 0", d->iterations);
    const struct { const char *name; float v; bool signed_; } args[] = {
        {"erodibility", d->erodibility, false}, {"uplift", d->uplift, false}, {"dt", d->dt, false},
        {"rain", d->rain, false},               {"seaLevel", d->seaLevel, true}};
    for (const auto &a : args) {
        NZ_REQUIRE(std::isfinite(a.v), "%s is not finite", a.name);
        NZ_REQUIRE(a.signed_ || a.v >= 0.0f, "%s %g < 0", a.name, (double)a.v);
    }
    *k = nz_fluvial_params{d->erodibility, d->uplift, d->dt, d->rain, d->seaLevel};
    return NZ_OK;
}

// The read-only planes of the desc of a tile-shaped call against the planes the call writes: h0 / h1 the height plane(s)
// (h1 may be NULL), n floats each like every plane of the desc, and `work`
static int32_t check_fluvial_planes(const nz_fluvial_desc &d, const float *h0, const float *h1, const float *work, size_t n) {
    const nz_named_plane reads[] = {
        {"drainageIn", d.drainageIn, n}, {"rainMap", d.rainMap, n}, {"hardness", d.hardness, n}, {"upliftMap", d.upliftMap, n}};
    const nz_named_plane writes[] = {{"src", h0, n}, {"the write plane", h1, n}, {"work", work, (size_t)FLU_PLANES * n}};
    for (const auto &r : reads)
        for (const auto &w : writes) NZ_REQUIRE(!nz_planes_overlap(r.p, n, w.p, w.floats), "%s overlaps %s", r.name, w.name);
    return NZ_OK;
}

// The body of every tile-shaped entry behind its NULL checks: the desc's checks, then desc->iterations launches on `count`
// tiles.  The height ping-pongs between h0 and h1 (height_pingpong); h1 NULL: the in-place forms, which keep the result in
// h0 and take work plane 2 as h1.  The drainage ping-pongs between work planes 0 and 1 (pingpong_set).  The first launch reads
// drainageIn, or the start state rain * rainMap written here into the plane it does not write, or -- without either -- no
// drainage plane at all.  Without an iteration plane 0 receives the start state.
static int32_t fluvial_series(nz_ctx *ctx, float *h0, float *h1, float *work, int res, int count, const nz_fluvial_desc *desc,
                              nz_handle *out, bool *in_h1) {
    const size_t n = (size_t)res * res * count;
    nz_fluvial_params k;
    NZ_TRY(check_fluvial(desc, &k));
    const nz_fluvial_desc &d = *desc;
    NZ_TRY(check_fluvial_planes(d, h0, h1, work, n));
    const bool keep_h0 = !h1;
    if (keep_h0) h1 = work + (size_t)(FLU_PLANES - 1) * n;
    nz_ctx_handle_rides(ctx, out != nullptr);  // (the last launch below is armed)
    const int iterations = d.iterations;
    float *planes[2] = {work, work + n};
    if (iterations == 0) {
        *in_h1 = false;
        nz_ctx_arm_last_launch(ctx);
        if (d.drainageIn) return nz_launch_copy(ctx->stream, work, d.drainageIn, n);
        if (d.rainMap) return nz_launch_fluvial_start(ctx->stream, work, d.rainMap, k.rain, n);
        return nz_launch_fill(ctx->stream, work, n, k.rain);
    }
    float *cur, *nxt;
    NZ_TRY(height_pingpong(ctx, h0, h1, n, iterations, keep_h0, &cur, &nxt, in_h1));
    const float *a_in = d.drainageIn;
    if (!a_in && d.rainMap) {
        NZ_TRY(nz_launch_fluvial_start(ctx->stream, planes[iterations & 1], d.rainMap, k.rain, n));
        a_in = planes[iterations & 1];
    }
    for (int it = 0; it < iterations; it++) {
        float *a_out = planes[pingpong_set(iterations, it)];
        if (it == iterations - 1) nz_ctx_arm_last_launch(ctx);
        NZ_TRY(nz_launch_fluvial(ctx->stream, cur, nxt, a_in, a_out, k, res, count, d.rainMap, d.hardness, d.upliftMap));
        a_in = a_out;
        std::swap(cur, nxt);
    }
    return NZ_OK;
}

static int32_t fluvial_stage_impl(nz_ctx *ctx, float *src, float *work, const nz_fluvial_desc *desc, int32_t resolution,
                                  int32_t count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    NZ_REQUIRE(src && work, "src/work is NULL");
    bool in_h1;
    NZ_TRY(fluvial_series(ctx, src, nullptr, work, resolution, count, desc, out, &in_h1));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_fluvial_erosion(nz_ctx *ctx, float *src, float *work, const nz_fluvial_desc *desc, int32_t resolution,
                                      nz_handle dep, nz_handle *out) {
    return fluvial_stage_impl(ctx, src, work, desc, resolution, 1, dep, out);
}

extern "C" int32_t nz_fluvial_erosion_batch(nz_ctx *ctx, float *src, float *work, const nz_fluvial_desc *desc,
                                            int32_t resolution, int32_t count, nz_handle dep, nz_handle *out) {
    return fluvial_stage_impl(ctx, src, work, desc, resolution, count, dep, out);
}

extern "C" int32_t nz_fluvial_erosion_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, const nz_fluvial_desc *desc,
                                         nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_rw(tile));
    NZ_REQUIRE(work, "work is NULL");
    bool in_h1;
    NZ_TRY(fluvial_series(ctx, tile->read, tile->write, work, tile->resolution, tile->count, desc, out, &in_h1));
    rw_swap(tile, in_h1);
    return nz_ctx_finish(ctx, out);
}

// ---- the stripe form (include/noize_hip.h): n iterations of one call on a row stripe, one launch each ----
constexpr int FLU_STRIPE_RADIUS = 2;  // rows one iteration reads beyond the rows it produces: receivers at 1, their heights at 2

extern "C" int32_t nz_fluvial_stripe_halo_rows(int32_t iterations) {
    return iterations > 0 ? FLU_STRIPE_RADIUS * iterations : 0;
}

extern "C" size_t nz_fluvial_stripe_work_floats(const nz_stripe *st, int32_t iterations) {
    return iterations > 1 ? 2 * nz_stripe_plane_floats(st) : 0;
}

extern "C" int32_t nz_fluvial_stripe(nz_ctx *ctx, const float *height_in, float *height_out, float *drainage_out, float *work,
                                     const nz_stripe *st, const nz_fluvial_desc *desc, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(desc, "desc is NULL");
    const int n = desc->iterations;
    NZ_REQUIRE(n >= 1, "iterations %d < 1", n);
    NZ_REQUIRE(n <= INT32_MAX / FLU_STRIPE_RADIUS, "iterations %d out of range", n);
    nz_fluvial_params k;
    NZ_TRY(check_fluvial(desc, &k));
    NZ_TRY(nz_check_stripe(st, FLU_STRIPE_RADIUS * n));
    NZ_REQUIRE(height_in && height_out && drainage_out, "height_in/height_out/drainage_out is NULL");
    NZ_REQUIRE(n == 1 || work, "work is NULL");
    const size_t span = nz_stripe_span(*st), plane = nz_stripe_plane_floats(st);
    const nz_named_plane reads[] = {{"height_in", height_in, span},   {"drainageIn", desc->drainageIn, span},
                                    {"rainMap", desc->rainMap, span}, {"hardness", desc->hardness, span},
                                    {"upliftMap", desc->upliftMap, span}};
    const nz_named_plane writes[] = {{"height_out", height_out, span}, {"drainage_out", drainage_out, span},
                                     {"work", n > 1 ? work : nullptr, 2 * plane}};
    NZ_TRY(nz_require_disjoint(writes, std::size(writes), reads, std::size(reads)));
    float *hs[2] = {height_out, work}, *as[2] = {drainage_out, n > 1 ? work + plane : nullptr};  // pingpong_set
    const int zlo = nz_stripe_grid_lo(*st), zhi = nz_stripe_grid_hi(*st) - 1;
    nz_geom g = nz_geom_from_stripe(*st);
    nz_ctx_handle_rides(ctx, out != nullptr);
    for (int j = 0; j < n; j++) {
        const int to = pingpong_set(n, j);
        nz_stripe_window(*st, FLU_STRIPE_RADIUS * (n - 1 - j), &g.or0, &g.or1);
        if (j == n - 1) nz_ctx_arm_last_launch(ctx);
        NZ_TRY(nz_launch_fluvial_stripe(ctx->stream, j == 0 ? height_in : hs[to ^ 1], hs[to],
                                        j == 0 ? desc->drainageIn : as[to ^ 1], as[to], k, g, zlo, zhi, desc->rainMap,
                                        desc->hardness, desc->upliftMap));
    }
    return nz_ctx_finish(ctx, out);
}

// ---------------------------------------------------------------------------------------------
// depression filling (new-framework feature, include/noize_hip.h, nz_fill.hip)
// ---------------------------------------------------------------------------------------------
// The seven stages that iterate to rest -- this one, drainage area, multiple-flow drainage, watershed, stream order, implicit
// fluvial erosion and its multiple-flow form -- share what follows.
//
// `work` in floats begins the same way for all of them: 16 status words (nz_relax_pass.hpp; the rest spare) and two
// generations of per-tile bytes (nz_tile64.hpp); then come the stage's own byte planes (one byte per cell) and 4-byte
// planes.  Bytes are rounded up to 16 per part.  relax_work lays the plane out by being asked for the parts in order;
// run on a null base it yields the total alone, so a *_work_floats entry and the entry that carves are one sequence of
// requests (the *_work_of functions) and cannot disagree.  One pass is one launch whatever its depth, so the launch-series
// planner (nz_split_iterations) has nothing to split here.
namespace {
struct relax_shape { size_t tiles, n; };  // the tiles of the call and the cells of one of its planes
relax_shape tile_shape(int res, int count) {
    return {(size_t)nz_tile64::tiles_x(res) * nz_tile64::tiles_z(res) * count, (size_t)res * res * count};
}
relax_shape stripe_shape(const nz_stripe &st) {  // the tiles cover the owned rows, a plane has the stripe's shape
    return {(size_t)nz_tile64::tiles_x(st.cols) * nz_tile64::tiles_z(st.own1 - st.own0), nz_stripe_plane_floats(&st)};
}
bool stripe_has_work(const nz_stripe *st) { return nz_stripe_plane_floats(st) && st->own0 >= 0 && st->own1 >= st->own0; }

struct relax_work {
    float *base;
    size_t total = 0;  // floats handed out so far; in the end, the size of `work`
    int *status;
    unsigned char *flags[2];
    relax_work(float *work, const relax_shape &sh)
        : base(work), status(ints(16)), flags{bytes(sh.tiles), bytes(sh.tiles)} {}
    float *floats(size_t n) {
        float *p = base ? base + total : nullptr;
        total += n;
        return p;
    }
    unsigned char *bytes(size_t n) { return reinterpret_cast<unsigned char *>(floats((n + 15) / 16 * 4)); }
    int *ints(size_t n) { return reinterpret_cast<int *>(floats(n)); }
};

// The sweep cap of a stage: 16 for each of the seven.  Six were measured at caps of 4 to 64, the multiple-flow implicit
// solve at 16 only.  The debug entry may be called while another thread runs an entry; it returns the
// cap before, and a value < 1 puts the default back.
constexpr int RELAX_SWEEPS = 16;
struct sweep_cap {
    std::atomic<int> cap{RELAX_SWEEPS};
    int load() const { return cap.load(); }  // an entry reads it once: one cap for the whole series
    int exchange(int sweeps) { return cap.exchange(sweeps > 0 ? sweeps : RELAX_SWEEPS); }
};
sweep_cap fill_sweeps, drainage_sweeps, watershed_sweeps, stream_order_sweeps, fluvial_implicit_sweeps;

// One series on whole tiles: pass(p, flags_in, flags_out) launches pass p, which reads byte generation (p - 1) & 1 and
// writes generation p & 1 -- which plane it reads and writes is the stage's business; finalise() launches last.
template <class Pass, class Finalise>
int32_t run_tile_series(nz_ctx *ctx, nz_handle *out, int maxPasses, const relax_work &hd, Pass pass, Finalise finalise) {
    nz_ctx_handle_rides(ctx, out != nullptr);
    for (int p = 0; p < maxPasses; p++) NZ_TRY(pass(p, hd.flags[(p - 1) & 1], hd.flags[p & 1]));
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(finalise());
    return nz_ctx_finish(ctx, out);
}

// One round on the owned rows of a stripe: the round's begin launch, mask() (a stage without one launches nothing),
// `passes` times pass(p, plane_in, plane_out, flags_in, flags_out) -- pass p reads plane p & 1 and writes the other, plane
// 0 the caller's -- and, when the last pass wrote the work plane, the round's end launch, which copies it back.
template <class Mask, class Pass>
int32_t run_stripe_round(nz_ctx *ctx, nz_handle *out, int passes, const relax_work &hd, float *callers, float *second,
                         const int32_t *proceed, int32_t *changed, int32_t first, const nz_geom &g, Mask mask, Pass pass) {
    float *planes[2] = {callers, second};
    nz_ctx_handle_rides(ctx, out != nullptr);
    NZ_TRY(nz_launch_fill_round_begin(ctx->stream, hd.status, proceed, changed, first != 0));
    NZ_TRY(mask());
    for (int p = 0; p < passes; p++) {
        if (p == passes - 1 && !(passes & 1)) nz_ctx_arm_last_launch(ctx);
        NZ_TRY(pass(p, planes[p & 1], planes[(p + 1) & 1], hd.flags[(p + 1) & 1], hd.flags[p & 1]));
    }
    if (passes & 1) {  // the last pass wrote the work plane
        nz_ctx_arm_last_launch(ctx);
        NZ_TRY(nz_launch_fill_round_end(ctx->stream, callers, second, hd.status, passes, g));
    }
    return nz_ctx_finish(ctx, out);
}

// the fill's `work`: the head and the W planes the passes alternate between -- both of them in the tile forms, one in the
// stripe form, whose other W plane is the caller's `w`
struct fill_work { relax_work hd; float *w[2]; };
fill_work fill_work_of(float *work, const relax_shape &sh, int w_planes) {
    fill_work k{relax_work(work, sh), {}};
    for (int i = 0; i < w_planes; i++) k.w[i] = k.hd.floats(sh.n);
    return k;
}
}  // namespace

static int32_t check_fill_desc(const nz_fill_desc *d) {
    NZ_REQUIRE(d, "desc is NULL");
    NZ_REQUIRE(std::isfinite(d->epsilon), "epsilon is not finite");
    NZ_REQUIRE(std::isfinite(d->seaLevel), "seaLevel is not finite");
    NZ_REQUIRE(d->epsilon >= 0.0f, "epsilon %g < 0", (double)d->epsilon);
    NZ_REQUIRE(d->maxPasses >= 1, "maxPasses %d < 1", d->maxPasses);
    return NZ_OK;
}

extern "C" size_t nz_fill_depressions_work_floats(int32_t resolution, int32_t count) {
    return resolution > 0 && count > 0 ? fill_work_of(nullptr, tile_shape(resolution, count), 2).hd.total : 0;
}

extern "C" int32_t nz_debug_fill_sweeps(int32_t sweeps) { return fill_sweeps.exchange(sweeps); }

// h: the plane that holds the input and receives the result; other: the write plane of an _rw pair or NULL
static int32_t fill_impl(nz_ctx *ctx, float *h, const float *other, float *work, const nz_fill_desc *d, int res, int count,
                         nz_handle *out) {
    NZ_REQUIRE(h && work, "src/work is NULL");
    NZ_TRY(check_fill_desc(d));
    const relax_shape sh = tile_shape(res, count);
    const fill_work k = fill_work_of(work, sh, 2);
    const size_t n = sh.n;
    NZ_REQUIRE(!nz_planes_overlap(d->depth, n, h, n), "depth overlaps src");
    NZ_REQUIRE(!nz_planes_overlap(d->depth, n, other, n), "depth overlaps the write plane");
    NZ_REQUIRE(!nz_planes_overlap(d->depth, n, work, k.hd.total), "depth overlaps work");
    const float eps = d->epsilon + 0.0f;  // -0 -> +0
    const int sweeps = fill_sweeps.load();
    return run_tile_series(
        ctx, out, d->maxPasses, k.hd,
        [&](int p, const unsigned char *flags_in, unsigned char *flags_out) {  // pass p writes plane p & 1
            return nz_launch_fill_pass(ctx->stream, h, p ? k.w[(p - 1) & 1] : nullptr, k.w[p & 1], k.hd.status, flags_in,
                                       flags_out, eps, d->seaLevel, res, count, p, sweeps);
        },
        // a converged series holds the fixed point in both planes, so either serves
        [&] { return nz_launch_fill_finalise(ctx->stream, h, k.w[0], d->depth, k.hd.status, n); });
}

extern "C" int32_t nz_fill_depressions(nz_ctx *ctx, float *src, float *work, const nz_fill_desc *desc, int32_t resolution,
                                       nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, 1));
    return fill_impl(ctx, src, nullptr, work, desc, resolution, 1, out);
}

extern "C" int32_t nz_fill_depressions_batch(nz_ctx *ctx, float *src, float *work, const nz_fill_desc *desc,
                                             int32_t resolution, int32_t count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    return fill_impl(ctx, src, nullptr, work, desc, resolution, count, out);
}

extern "C" int32_t nz_fill_depressions_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, const nz_fill_desc *desc, nz_handle dep,
                                          nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_rw(tile));
    return fill_impl(ctx, tile->read, tile->write, work, desc, tile->resolution, tile->count, out);
}

// ---- the stripe form (include/noize_hip.h): one round of passes on the owned rows against one frozen row on each side ----
extern "C" int32_t nz_fill_stripe_halo_rows(void) { return 1; }

extern "C" size_t nz_fill_stripe_work_floats(const nz_stripe *st) {
    return stripe_has_work(st) ? fill_work_of(nullptr, stripe_shape(*st), 1).hd.total : 0;
}

extern "C" int32_t nz_fill_stripe(nz_ctx *ctx, const float *height, float *w, float *work, const nz_stripe *st,
                                  const nz_fill_desc *desc, int32_t first, const int32_t *proceed, int32_t *changed,
                                  nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_fill_desc(desc));
    NZ_TRY(nz_check_stripe(st, 1));
    NZ_REQUIRE(height && w && work, "height/w/work is NULL");
    NZ_REQUIRE(changed, "changed is NULL");
    const nz_geom g = nz_geom_from_stripe(*st);
    const fill_work k = fill_work_of(work, stripe_shape(*st), 1);
    const size_t span = nz_stripe_span(*st), total = k.hd.total;
    NZ_REQUIRE(!nz_planes_overlap(w, span, height, span), "w overlaps height");
    NZ_REQUIRE(!nz_planes_overlap(work, total, height, span), "work overlaps height");
    NZ_REQUIRE(!nz_planes_overlap(work, total, w, span), "work overlaps w");
    const nz_named_plane planes_of_call[] = {{"height", height, span}, {"w", w, span}, {"work", work, total}};
    for (const auto &p : planes_of_call) {  // the two words are ints, not planes of floats
        NZ_REQUIRE(!nz_bytes_overlap(changed, 4, p.p, p.floats * 4), "changed overlaps a plane");
        NZ_REQUIRE(!nz_bytes_overlap(proceed, 4, p.p, p.floats * 4), "proceed overlaps a plane");
    }
    const float eps = desc->epsilon + 0.0f;  // -0 -> +0
    const int sweeps = fill_sweeps.load();
    const int zlo = nz_stripe_grid_lo(*st), zhi = nz_stripe_grid_hi(*st) - 1;
    return run_stripe_round(
        ctx, out, desc->maxPasses, k.hd, w, k.w[0], proceed, changed, first, g, [] { return (int32_t)NZ_OK; },
        [&](int p, const float *w_in, float *w_out, const unsigned char *flags_in, unsigned char *flags_out) {
            return nz_launch_fill_stripe_pass(ctx->stream, height, w_in, w_out, w, k.hd.status, flags_in, flags_out, changed,
                                              eps, desc->seaLevel, g, zlo, zhi, first != 0, p, sweeps);
        });
}

extern "C" int32_t nz_fill_stripe_finalise(nz_ctx *ctx, float *height, const float *w, float *depth, const nz_stripe *st,
                                           const int32_t *converged, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(nz_check_stripe(st, 0));
    NZ_REQUIRE(height && w, "height/w is NULL");
    NZ_REQUIRE(converged, "converged is NULL");
    const size_t span = nz_stripe_span(*st);
    NZ_REQUIRE(!nz_planes_overlap(height, span, w, span), "height overlaps w");
    NZ_REQUIRE(!nz_planes_overlap(depth, span, height, span), "depth overlaps height");
    NZ_REQUIRE(!nz_planes_overlap(depth, span, w, span), "depth overlaps w");
    nz_ctx_handle_rides(ctx, out != nullptr);
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_fill_stripe_finalise(ctx->stream, height, w, depth, converged, nz_geom_from_stripe(*st)));
    return nz_ctx_finish(ctx, out);
}

// ---------------------------------------------------------------------------------------------
// drainage area (new-framework feature, include/noize_hip.h, nz_drainage.hip)
// ---------------------------------------------------------------------------------------------
// `work`, in the tile and in the stripe form: the head, one donor byte per cell and one A plane; the other A plane is the
// caller's.  (The stripe form counts the tile bytes over the owned rows and keeps a donor byte at the cell's index in the
// stripe's plane, of which only the owned rows are used.)
namespace {
struct drainage_work { relax_work hd; unsigned char *donors; float *a; };
drainage_work drainage_work_of(float *work, const relax_shape &sh) {
    drainage_work k{relax_work(work, sh), nullptr, nullptr};
    k.donors = k.hd.bytes(sh.n);
    k.a = k.hd.floats(sh.n);
    return k;
}
}  // namespace

extern "C" size_t nz_drainage_area_work_floats(int32_t resolution, int32_t count) {
    return resolution > 0 && count > 0 ? drainage_work_of(nullptr, tile_shape(resolution, count)).hd.total : 0;
}

extern "C" int32_t nz_debug_drainage_sweeps(int32_t sweeps) { return drainage_sweeps.exchange(sweeps); }

static int32_t check_drainage_desc(const nz_drainage_desc *d) {
    NZ_REQUIRE(d, "desc is NULL");
    NZ_REQUIRE(std::isfinite(d->rain), "rain is not finite");
    NZ_REQUIRE(std::isfinite(d->seaLevel), "seaLevel is not finite");
    NZ_REQUIRE(d->rain >= 0.0f, "rain %g < 0", (double)d->rain);
    NZ_REQUIRE(d->maxPasses >= 1, "maxPasses %d < 1", d->maxPasses);
    return NZ_OK;
}

static int32_t drainage_impl(nz_ctx *ctx, const float *height, float *drainage, float *work, const nz_drainage_desc *d, int res,
                             int count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    if (res == 0 || count == 0) return nz_ctx_finish(ctx, out);  // an empty payload: nothing to do
    NZ_TRY(check_batch(res, count));
    NZ_REQUIRE(d, "desc is NULL");
    NZ_REQUIRE(height, "height is NULL");
    NZ_REQUIRE(drainage, "drainage is NULL");
    NZ_REQUIRE(work, "work is NULL");
    NZ_TRY(check_drainage_desc(d));
    const relax_shape sh = tile_shape(res, count);
    const drainage_work k = drainage_work_of(work, sh);
    const size_t n = sh.n;
    const nz_named_plane writes[] = {{"drainage", drainage, n}, {"work", work, k.hd.total}};
    const nz_named_plane reads[] = {{"height", height, n}, {"rainMap", d->rainMap, n}};
    NZ_TRY(nz_require_disjoint(writes, std::size(writes), reads, std::size(reads)));
    float *planes[2] = {drainage, k.a};
    const int sweeps = drainage_sweeps.load();
    NZ_TRY(nz_launch_drainage_mask(ctx->stream, height, k.donors, d->seaLevel, res, count));
    return run_tile_series(
        ctx, out, d->maxPasses, k.hd,
        [&](int p, const unsigned char *flags_in, unsigned char *flags_out) {  // pass p writes plane p & 1
            return nz_launch_drainage_pass(ctx->stream, k.donors, d->rainMap, p ? planes[(p - 1) & 1] : nullptr, planes[p & 1],
                                           k.hd.status, flags_in, flags_out, d->rain, res, count, p, sweeps);
        },
        // a series at rest holds the fixed point in both planes, so `drainage` has it whichever plane was written last
        [&] { return nz_launch_drainage_finalise(ctx->stream, drainage, d->rainMap, k.hd.status, d->rain, n); });
}

extern "C" int32_t nz_drainage_area(nz_ctx *ctx, const float *height, float *drainage, float *work,
                                    const nz_drainage_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out) {
    return drainage_impl(ctx, height, drainage, work, desc, resolution, 1, dep, out);
}

extern "C" int32_t nz_drainage_area_batch(nz_ctx *ctx, const float *height, float *drainage, float *work,
                                          const nz_drainage_desc *desc, int32_t resolution, int32_t count, nz_handle dep,
                                          nz_handle *out) {
    return drainage_impl(ctx, height, drainage, work, desc, resolution, count, dep, out);
}

// ---- the stripe form (include/noize_hip.h): one round of passes on the owned rows against one frozen row of A on each side ----
// `work` is laid out as in the tile form.  The round's begin and end launches are the fill stripe's: they know status words
// and planes only.
extern "C" int32_t nz_drainage_stripe_halo_rows(void) { return 2; }

extern "C" size_t nz_drainage_stripe_work_floats(const nz_stripe *st) {
    return stripe_has_work(st) ? drainage_work_of(nullptr, stripe_shape(*st)).hd.total : 0;
}

// the two words of a stripe call are ints, not planes of floats: apart from every plane of the call and from each other
static int32_t check_stripe_words(const int32_t *changed, const char *cname, const int32_t *other, const char *oname,
                                  const nz_named_plane *planes, size_t n) {
    for (size_t i = 0; i < n; i++) {
        NZ_REQUIRE(!nz_bytes_overlap(changed, 4, planes[i].p, planes[i].floats * 4), "%s overlaps %s", cname, planes[i].name);
        NZ_REQUIRE(!nz_bytes_overlap(other, 4, planes[i].p, planes[i].floats * 4), "%s overlaps %s", oname, planes[i].name);
    }
    NZ_REQUIRE(!nz_bytes_overlap(changed, 4, other, 4), "%s overlaps %s", cname, oname);
    return NZ_OK;
}

extern "C" int32_t nz_drainage_stripe_round(nz_ctx *ctx, const float *height, float *a, float *work, const nz_stripe *st,
                                      const nz_drainage_desc *desc, int32_t first, const int32_t *proceed, int32_t *changed,
                                      nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_drainage_desc(desc));
    NZ_TRY(nz_check_stripe(st, first ? 2 : 1));  // the heights at radius 2, A and the rain map at radius 1
    NZ_REQUIRE(height, "height is NULL");
    NZ_REQUIRE(a, "a is NULL");
    NZ_REQUIRE(work, "work is NULL");
    NZ_REQUIRE(changed, "changed is NULL");
    const nz_geom g = nz_geom_from_stripe(*st);
    const drainage_work k = drainage_work_of(work, stripe_shape(*st));
    const size_t span = nz_stripe_span(*st);
    const nz_named_plane writes[] = {{"a", a, span}, {"work", work, k.hd.total}};
    const nz_named_plane reads[] = {{"height", height, span}, {"rainMap", desc->rainMap, span}};
    NZ_TRY(nz_require_disjoint(writes, std::size(writes), reads, std::size(reads)));
    const nz_named_plane all[] = {writes[0], writes[1], reads[0], reads[1]};
    NZ_TRY(check_stripe_words(changed, "changed", proceed, "proceed", all, std::size(all)));
    const int sweeps = drainage_sweeps.load();
    const int zlo = nz_stripe_grid_lo(*st), zhi = nz_stripe_grid_hi(*st) - 1;
    return run_stripe_round(
        ctx, out, desc->maxPasses, k.hd, a, k.a, proceed, changed, first, g,
        [&]() -> int32_t {  // the donor bytes of a round that continues stand in `work`
            if (!first) return NZ_OK;
            return nz_launch_drainage_stripe_mask(ctx->stream, height, k.donors, k.hd.status, desc->seaLevel, g, zlo, zhi);
        },
        [&](int p, const float *a_in, float *a_out, const unsigned char *flags_in, unsigned char *flags_out) {
            return nz_launch_drainage_stripe_pass(ctx->stream, k.donors, desc->rainMap, a_in, a_out, k.hd.status, flags_in,
                                                  flags_out, changed, desc->rain, g, zlo, zhi, first != 0, p, sweeps);
        });
}

extern "C" int32_t nz_drainage_stripe_finalise(nz_ctx *ctx, float *a, const nz_stripe *st, const nz_drainage_desc *desc,
                                               const int32_t *converged, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_drainage_desc(desc));
    NZ_TRY(nz_check_stripe(st, 0));
    NZ_REQUIRE(a, "a is NULL");
    NZ_REQUIRE(converged, "converged is NULL");
    const size_t span = nz_stripe_span(*st);
    NZ_REQUIRE(!nz_planes_overlap(a, span, desc->rainMap, span), "a overlaps rainMap");
    NZ_REQUIRE(!nz_bytes_overlap(converged, 4, a, span * 4), "converged overlaps a");
    nz_ctx_handle_rides(ctx, out != nullptr);
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_drainage_stripe_finalise(ctx->stream, a, desc->rainMap, converged, desc->rain, nz_geom_from_stripe(*st)));
    return nz_ctx_finish(ctx, out);
}

// ---------------------------------------------------------------------------------------------
// multiple-flow drainage (new-framework feature, include/noize_hip.h, nz_drainage_mfd.hip)
// ---------------------------------------------------------------------------------------------
// `work`: the head, eight planes of incoming weights and one A plane; the other A plane is the caller's.  Everything that
// is not about weights is drainage_impl's; the finalise launch is the same one.
namespace {
struct drainage_mfd_work { relax_work hd; float *wts; float *a; };
drainage_mfd_work drainage_mfd_work_of(float *work, const relax_shape &sh) {
    drainage_mfd_work k{relax_work(work, sh), nullptr, nullptr};
    k.wts = k.hd.floats(8 * sh.n);
    k.a = k.hd.floats(sh.n);
    return k;
}
sweep_cap drainage_mfd_sweeps;
}  // namespace

extern "C" size_t nz_drainage_mfd_work_floats(int32_t resolution, int32_t count) {
    return resolution > 0 && count > 0 ? drainage_mfd_work_of(nullptr, tile_shape(resolution, count)).hd.total : 0;
}

extern "C" int32_t nz_debug_drainage_mfd_sweeps(int32_t sweeps) { return drainage_mfd_sweeps.exchange(sweeps); }

static int32_t drainage_mfd_impl(nz_ctx *ctx, const float *height, float *drainage, float *work, const nz_drainage_mfd_desc *d,
                                 int res, int count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    if (res == 0 || count == 0) return nz_ctx_finish(ctx, out);  // an empty payload: nothing to do
    NZ_TRY(check_batch(res, count));
    NZ_REQUIRE(d, "desc is NULL");
    NZ_REQUIRE(height, "height is NULL");
    NZ_REQUIRE(drainage, "drainage is NULL");
    NZ_REQUIRE(work, "work is NULL");
    NZ_REQUIRE(std::isfinite(d->rain), "rain is not finite");
    NZ_REQUIRE(std::isfinite(d->seaLevel), "seaLevel is not finite");
    NZ_REQUIRE(d->rain >= 0.0f, "rain %g < 0", (double)d->rain);
    NZ_REQUIRE(d->maxPasses >= 1, "maxPasses %d < 1", d->maxPasses);
    NZ_REQUIRE(d->exponent >= 1 && d->exponent <= 16, "exponent %d outside 1..16", d->exponent);
    const relax_shape sh = tile_shape(res, count);
    const drainage_mfd_work k = drainage_mfd_work_of(work, sh);
    const size_t n = sh.n;
    const nz_named_plane writes[] = {{"drainage", drainage, n}, {"work", work, k.hd.total}};
    const nz_named_plane reads[] = {{"height", height, n}, {"rainMap", d->rainMap, n}};
    NZ_TRY(nz_require_disjoint(writes, std::size(writes), reads, std::size(reads)));
    float *planes[2] = {drainage, k.a};
    const int sweeps = drainage_mfd_sweeps.load();
    NZ_TRY(nz_launch_drainage_mfd_setup(ctx->stream, height, k.wts, d->seaLevel, res, count, d->exponent));
    return run_tile_series(
        ctx, out, d->maxPasses, k.hd,
        [&](int p, const unsigned char *flags_in, unsigned char *flags_out) {  // pass p writes plane p & 1
            return nz_launch_drainage_mfd_pass(ctx->stream, k.wts, d->rainMap, p ? planes[(p - 1) & 1] : nullptr, planes[p & 1],
                                               k.hd.status, flags_in, flags_out, d->rain, res, count, p, sweeps);
        },
        // a series at rest holds the fixed point in both planes, so `drainage` has it whichever plane was written last
        [&] { return nz_launch_drainage_finalise(ctx->stream, drainage, d->rainMap, k.hd.status, d->rain, n); });
}

extern "C" int32_t nz_drainage_mfd(nz_ctx *ctx, const float *height, float *drainage, float *work,
                                   const nz_drainage_mfd_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out) {
    return drainage_mfd_impl(ctx, height, drainage, work, desc, resolution, 1, dep, out);
}

extern "C" int32_t nz_drainage_mfd_batch(nz_ctx *ctx, const float *height, float *drainage, float *work,
                                         const nz_drainage_mfd_desc *desc, int32_t resolution, int32_t count, nz_handle dep,
                                         nz_handle *out) {
    return drainage_mfd_impl(ctx, height, drainage, work, desc, resolution, count, dep, out);
}

// ---------------------------------------------------------------------------------------------
// watershed: basin labels, flow length, receiver codes (new-framework feature, include/noize_hip.h, nz_watershed.hip)
// ---------------------------------------------------------------------------------------------
// `work`: the head, one receiver byte per cell (unused when the caller has a `receivers` plane), the second label plane of
// count * res^2 int32 and, with a length, the second length plane; the first planes are the caller's `basin` and `length`.
namespace {
constexpr float WATERSHED_SQRT2 = 0x1.6a09e6p+0f;  // the diagonal step is cellSize times this, rounded once
struct watershed_work { relax_work hd; unsigned char *recv; int *basin; float *length; };
watershed_work watershed_work_of(float *work, const relax_shape &sh, bool with_length) {
    watershed_work k{relax_work(work, sh), nullptr, nullptr, nullptr};
    k.recv = k.hd.bytes(sh.n);
    k.basin = k.hd.ints(sh.n);
    if (with_length) k.length = k.hd.floats(sh.n);
    return k;
}
}  // namespace

extern "C" size_t nz_watershed_work_floats(int32_t resolution, int32_t count, int32_t withLength) {
    if (resolution <= 0 || count <= 0) return 0;
    return watershed_work_of(nullptr, tile_shape(resolution, count), withLength != 0).hd.total;
}

extern "C" int32_t nz_debug_watershed_sweeps(int32_t sweeps) { return watershed_sweeps.exchange(sweeps); }

static int32_t watershed_impl(nz_ctx *ctx, const float *height, int32_t *basin, float *length, uint8_t *receivers, float *work,
                              const nz_watershed_desc *d, int res, int count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    if (res == 0 || count == 0) return nz_ctx_finish(ctx, out);  // an empty payload: nothing to do
    NZ_TRY(check_batch(res, count));
    NZ_REQUIRE(d, "desc is NULL");
    NZ_REQUIRE(height, "height is NULL");
    NZ_REQUIRE(basin, "basin is NULL");
    NZ_REQUIRE(work, "work is NULL");
    NZ_REQUIRE(std::isfinite(d->cellSize), "cellSize is not finite");
    NZ_REQUIRE(!std::isnan(d->seaLevel), "seaLevel is NaN");
    NZ_REQUIRE(d->cellSize > 0.0f, "cellSize %g <= 0", (double)d->cellSize);
    NZ_REQUIRE(d->maxPasses >= 1, "maxPasses %d < 1", d->maxPasses);
    const relax_shape sh = tile_shape(res, count);
    const watershed_work k = watershed_work_of(work, sh, length != nullptr);
    const size_t n = sh.n;
    NZ_REQUIRE(n <= (size_t)INT32_MAX, "count %d x resolution %d^2: %zu cells are beyond int32", count, res, n);
    const float *labels = reinterpret_cast<const float *>(basin);  // a plane of n 4-byte cells
    const nz_named_plane writes[] = {{"basin", labels, n}, {"length", length, n}, {"work", work, k.hd.total}};
    const nz_named_plane reads[] = {{"height", height, n}};
    NZ_TRY(nz_require_disjoint(writes, std::size(writes), reads, std::size(reads)));
    for (const auto &p : {reads[0], writes[0], writes[1], writes[2]})  // the receiver plane is bytes, not floats
        NZ_REQUIRE(!nz_bytes_overlap(receivers, n, p.p, p.floats * sizeof(float)), "receivers overlaps %s", p.name);
    unsigned char *recv = receivers ? receivers : k.recv;
    int *labels2[2] = {basin, k.basin};
    float *lengths[2] = {length, k.length};
    const float cell = d->cellSize, diag = d->cellSize * WATERSHED_SQRT2;
    const int sweeps = watershed_sweeps.load();
    NZ_TRY(nz_launch_watershed_receivers(ctx->stream, height, recv, d->seaLevel, res, count));
    return run_tile_series(
        ctx, out, d->maxPasses, k.hd,
        [&](int p, const unsigned char *flags_in, unsigned char *flags_out) {  // pass p writes plane p & 1 of each pair
            return nz_launch_watershed_pass(ctx->stream, recv, p ? labels2[(p - 1) & 1] : nullptr, labels2[p & 1],
                                            p ? lengths[(p - 1) & 1] : nullptr, lengths[p & 1], k.hd.status, flags_in,
                                            flags_out, cell, diag, res, count, p, sweeps);
        },
        // a series at rest holds the fixed point in both planes of a pair, so the caller's have it whichever was written last
        [&] { return nz_launch_watershed_finalise(ctx->stream, basin, length, k.hd.status, res, n); });
}

extern "C" int32_t nz_watershed(nz_ctx *ctx, const float *height, int32_t *basin, float *length, uint8_t *receivers,
                                float *work, const nz_watershed_desc *desc, int32_t resolution, nz_handle dep,
                                nz_handle *out) {
    return watershed_impl(ctx, height, basin, length, receivers, work, desc, resolution, 1, dep, out);
}

extern "C" int32_t nz_watershed_batch(nz_ctx *ctx, const float *height, int32_t *basin, float *length, uint8_t *receivers,
                                      float *work, const nz_watershed_desc *desc, int32_t resolution, int32_t count,
                                      nz_handle dep, nz_handle *out) {
    return watershed_impl(ctx, height, basin, length, receivers, work, desc, resolution, count, dep, out);
}

// ---------------------------------------------------------------------------------------------
// stream order: Strahler order and river links (new-framework feature, include/noize_hip.h, nz_stream_order.hip)
// ---------------------------------------------------------------------------------------------
// `work`: the head, one channel-donor byte per cell, the second order plane of one byte per cell and, with links, the second
// link plane of count * res^2 int32; the first planes are the caller's `order` and `link`.
namespace {
struct stream_order_work { relax_work hd; unsigned char *donors, *order; int *link; };
stream_order_work stream_order_work_of(float *work, const relax_shape &sh, bool with_links) {
    stream_order_work k{relax_work(work, sh), nullptr, nullptr, nullptr};
    k.donors = k.hd.bytes(sh.n);
    k.order = k.hd.bytes(sh.n);
    if (with_links) k.link = k.hd.ints(sh.n);
    return k;
}
}  // namespace

extern "C" size_t nz_stream_order_work_floats(int32_t resolution, int32_t count, int32_t withLinks) {
    if (resolution <= 0 || count <= 0) return 0;
    return stream_order_work_of(nullptr, tile_shape(resolution, count), withLinks != 0).hd.total;
}

extern "C" int32_t nz_debug_stream_order_sweeps(int32_t sweeps) { return stream_order_sweeps.exchange(sweeps); }

static int32_t stream_order_impl(nz_ctx *ctx, const float *height, uint8_t *order, int32_t *link, float *work,
                                 const nz_stream_order_desc *d, int res, int count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    if (res == 0 || count == 0) return nz_ctx_finish(ctx, out);  // an empty payload: nothing to do
    NZ_TRY(check_batch(res, count));
    NZ_REQUIRE(d, "desc is NULL");
    NZ_REQUIRE(height, "height is NULL");
    NZ_REQUIRE(order, "order is NULL");
    NZ_REQUIRE(work, "work is NULL");
    NZ_REQUIRE(std::isfinite(d->threshold), "threshold is not finite");
    NZ_REQUIRE(!std::isnan(d->seaLevel), "seaLevel is NaN");
    NZ_REQUIRE(d->maxPasses >= 1, "maxPasses %d < 1", d->maxPasses);
    const relax_shape sh = tile_shape(res, count);
    const stream_order_work k = stream_order_work_of(work, sh, link != nullptr);
    const size_t n = sh.n;
    NZ_REQUIRE(n <= (size_t)INT32_MAX, "count %d x resolution %d^2: %zu cells are beyond int32", count, res, n);
    const float *links = reinterpret_cast<const float *>(link);  // a plane of n 4-byte cells
    const nz_named_plane writes[] = {{"link", links, n}, {"work", work, k.hd.total}};
    const nz_named_plane reads[] = {{"height", height, n}, {"drainage", d->drainage, n}};
    NZ_TRY(nz_require_disjoint(writes, std::size(writes), reads, std::size(reads)));
    for (const auto &p : {reads[0], reads[1], writes[0], writes[1]})  // the order plane is bytes, not floats
        NZ_REQUIRE(!nz_bytes_overlap(order, n, p.p, p.floats * sizeof(float)), "order overlaps %s", p.name);
    unsigned char *orders[2] = {order, k.order};
    int *links2[2] = {link, k.link};
    const int sweeps = stream_order_sweeps.load();
    NZ_TRY(nz_launch_stream_mask(ctx->stream, height, d->drainage, k.donors, order, d->seaLevel, d->threshold, res, count));
    return run_tile_series(
        ctx, out, d->maxPasses, k.hd,
        // pass p READS plane p & 1 of each pair and writes the other: the mask launch left the start state in plane 0
        [&](int p, const unsigned char *flags_in, unsigned char *flags_out) {
            return nz_launch_stream_pass(ctx->stream, k.donors, orders[p & 1], orders[(p + 1) & 1], p ? links2[p & 1] : nullptr,
                                         links2[(p + 1) & 1], k.hd.status, flags_in, flags_out, res, count, p, sweeps);
        },
        // a series at rest holds the fixed point in both planes of a pair, so the caller's have it whichever was written last
        [&] { return nz_launch_stream_finalise(ctx->stream, order, link, d->drainage, k.hd.status, d->threshold, res, n); });
}

extern "C" int32_t nz_stream_order(nz_ctx *ctx, const float *height, uint8_t *order, int32_t *link, float *work,
                                   const nz_stream_order_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out) {
    return stream_order_impl(ctx, height, order, link, work, desc, resolution, 1, dep, out);
}

extern "C" int32_t nz_stream_order_batch(nz_ctx *ctx, const float *height, uint8_t *order, int32_t *link, float *work,
                                         const nz_stream_order_desc *desc, int32_t resolution, int32_t count, nz_handle dep,
                                         nz_handle *out) {
    return stream_order_impl(ctx, height, order, link, work, desc, resolution, count, dep, out);
}

// ---------------------------------------------------------------------------------------------
// implicit fluvial erosion: one large time step as one solve (new-framework feature, include/noize_hip.h,
// nz_fluvial_implicit.hip)
// ---------------------------------------------------------------------------------------------
// `work`: the head, one receiver byte per cell, the coefficient planes b and f and the second h' plane; the first h' plane
// is the caller's `out`.
namespace {
// What nz_fluvial_implicit_desc and nz_fluvial_implicit_mfd_desc have in common, and the checks on it and on the planes:
// the two entries refuse word for word because they run the same text.
struct implicit_args {
    float erodibility, uplift, dt, seaLevel;
    int maxPasses;
    const float *hardness, *upliftMap;
    const int32_t *proceed;
    int32_t *tally;
};
template <class Desc>
implicit_args implicit_args_of(const Desc &d) {
    return {d.erodibility, d.uplift, d.dt, d.seaLevel, d.maxPasses, d.hardness, d.upliftMap, d.proceed, d.tally};
}
int32_t check_implicit_scalars(const float *height, const float *drainage, const float *outp, const float *work,
                               const implicit_args &a) {
    NZ_REQUIRE(height, "height is NULL");
    NZ_REQUIRE(drainage, "drainage is NULL");
    NZ_REQUIRE(outp, "out is NULL");
    NZ_REQUIRE(work, "work is NULL");
    NZ_REQUIRE(std::isfinite(a.erodibility), "erodibility is not finite");
    NZ_REQUIRE(std::isfinite(a.uplift), "uplift is not finite");
    NZ_REQUIRE(std::isfinite(a.dt), "dt is not finite");
    NZ_REQUIRE(std::isfinite(a.seaLevel), "seaLevel is not finite");
    NZ_REQUIRE(a.erodibility >= 0.0f, "erodibility %g < 0", (double)a.erodibility);
    NZ_REQUIRE(a.uplift >= 0.0f, "uplift %g < 0", (double)a.uplift);
    NZ_REQUIRE(a.dt >= 0.0f, "dt %g < 0", (double)a.dt);
    NZ_REQUIRE(a.maxPasses >= 1, "maxPasses %d < 1", a.maxPasses);
    return NZ_OK;
}
// n: the cells of one plane; work_floats: what the entry's *_work_of hands out
int32_t check_implicit_planes(const float *height, const float *drainage, float *outp, float *work, size_t work_floats,
                              const implicit_args &a, int res, int count, size_t n) {
    NZ_REQUIRE(n <= (size_t)INT32_MAX, "count %d x resolution %d^2: %zu cells are beyond int32", count, res, n);
    const nz_named_plane writes[] = {{"out", outp, n}, {"work", work, work_floats}};
    const nz_named_plane reads[] = {{"height", height, n}, {"drainage", drainage, n}, {"hardness", a.hardness, n},
                                    {"upliftMap", a.upliftMap, n}};
    NZ_TRY(nz_require_disjoint(writes, std::size(writes), reads, std::size(reads)));
    for (const auto &p : {writes[0], writes[1], reads[0], reads[1], reads[2], reads[3]})  // the words are ints, not planes
        NZ_REQUIRE(!nz_bytes_overlap(a.tally, 8, p.p, p.floats * sizeof(float)), "tally overlaps %s", p.name);
    for (const auto &p : {writes[0], writes[1]})
        NZ_REQUIRE(!nz_bytes_overlap(a.proceed, 4, p.p, p.floats * sizeof(float)), "proceed overlaps %s", p.name);
    NZ_REQUIRE(!nz_bytes_overlap(a.tally, 8, a.proceed, 4), "tally overlaps proceed");
    return NZ_OK;
}

struct fluvial_implicit_work { relax_work hd; unsigned char *recv; float *b, *f, *h2; };
fluvial_implicit_work fluvial_implicit_work_of(float *work, const relax_shape &sh) {
    fluvial_implicit_work k{relax_work(work, sh), nullptr, nullptr, nullptr, nullptr};
    k.recv = k.hd.bytes(sh.n);
    k.b = k.hd.floats(sh.n);
    k.f = k.hd.floats(sh.n);
    k.h2 = k.hd.floats(sh.n);
    return k;
}
}  // namespace

extern "C" size_t nz_fluvial_implicit_work_floats(int32_t resolution, int32_t count) {
    if (resolution <= 0 || count <= 0) return 0;
    return fluvial_implicit_work_of(nullptr, tile_shape(resolution, count)).hd.total;
}

extern "C" int32_t nz_debug_fluvial_implicit_sweeps(int32_t sweeps) { return fluvial_implicit_sweeps.exchange(sweeps); }

static int32_t fluvial_implicit_impl(nz_ctx *ctx, const float *height, const float *drainage, float *outp, float *work,
                                     const nz_fluvial_implicit_desc *d, int res, int count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    if (res == 0 || count == 0) return nz_ctx_finish(ctx, out);  // an empty payload: nothing to do
    NZ_TRY(check_batch(res, count));
    NZ_REQUIRE(d, "desc is NULL");
    const implicit_args a = implicit_args_of(*d);
    NZ_TRY(check_implicit_scalars(height, drainage, outp, work, a));
    const relax_shape sh = tile_shape(res, count);
    const fluvial_implicit_work k = fluvial_implicit_work_of(work, sh);
    const size_t n = sh.n;
    NZ_TRY(check_implicit_planes(height, drainage, outp, work, k.hd.total, a, res, count, n));
    float *planes[2] = {outp, k.h2};
    const int sweeps = fluvial_implicit_sweeps.load();
    NZ_TRY(nz_launch_fluvial_implicit_begin(ctx->stream, k.hd.status, d->proceed));
    NZ_TRY(nz_launch_fluvial_implicit_setup(ctx->stream, height, drainage, d->hardness, d->upliftMap, k.recv, k.b, k.f,
                                            k.hd.status, d->erodibility, d->uplift, d->dt, d->seaLevel, res, count));
    return run_tile_series(
        ctx, out, d->maxPasses, k.hd,
        [&](int p, const unsigned char *flags_in, unsigned char *flags_out) {  // pass p writes plane p & 1
            return nz_launch_fluvial_implicit_pass(ctx->stream, k.recv, k.b, k.f, p ? planes[(p - 1) & 1] : nullptr,
                                                   planes[p & 1], k.hd.status, flags_in, flags_out, res, count, p, sweeps);
        },
        // a series at rest holds the fixed point in both planes, so `out` has it whichever plane was written last
        [&] { return nz_launch_fluvial_implicit_finalise(ctx->stream, height, outp, k.hd.status, d->tally, n); });
}

extern "C" int32_t nz_fluvial_implicit(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                                       const nz_fluvial_implicit_desc *desc, int32_t resolution, nz_handle dep,
                                       nz_handle *out_handle) {
    return fluvial_implicit_impl(ctx, height, drainage, out, work, desc, resolution, 1, dep, out_handle);
}

extern "C" int32_t nz_fluvial_implicit_batch(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                                             const nz_fluvial_implicit_desc *desc, int32_t resolution, int32_t count,
                                             nz_handle dep, nz_handle *out_handle) {
    return fluvial_implicit_impl(ctx, height, drainage, out, work, desc, resolution, count, dep, out_handle);
}

// ---- the stripe form (include/noize_hip.h): one round of passes on the owned rows against one frozen row of h' on each side ----
// `work` is laid out as in the tile form, over the stripe's plane.  The round's begin and end launches are the fill stripe's:
// they know status words and planes only.
extern "C" int32_t nz_implicit_fluvial_stripe_halo_rows(void) { return 1; }

extern "C" size_t nz_implicit_fluvial_stripe_work_floats(const nz_stripe *st) {
    return stripe_has_work(st) ? fluvial_implicit_work_of(nullptr, stripe_shape(*st)).hd.total : 0;
}

extern "C" int32_t nz_implicit_fluvial_stripe_round(nz_ctx *ctx, const float *height, const float *drainage, float *outp,
                                                    float *work, const nz_stripe *st, const nz_fluvial_implicit_desc *desc,
                                                    int32_t first, const int32_t *proceed, int32_t *changed, nz_handle dep,
                                                    nz_handle *out_handle) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(desc, "desc is NULL");
    const implicit_args a = implicit_args_of(*desc);
    NZ_TRY(check_implicit_scalars(height, drainage, outp, work, a));
    NZ_REQUIRE(!desc->proceed, "desc->proceed must be NULL in a stripe round: the round has its own proceed word");
    NZ_REQUIRE(!desc->tally, "desc->tally must be NULL in a stripe round: the driver counts");
    NZ_TRY(nz_check_stripe(st, 1));  // the heights, and `out` between rounds, at radius 1
    NZ_REQUIRE(changed, "changed is NULL");
    const nz_geom g = nz_geom_from_stripe(*st);
    const fluvial_implicit_work k = fluvial_implicit_work_of(work, stripe_shape(*st));
    const size_t span = nz_stripe_span(*st);
    NZ_REQUIRE(nz_stripe_plane_floats(st) <= (size_t)INT32_MAX, "stripe: %zu cells are beyond int32", nz_stripe_plane_floats(st));
    const nz_named_plane writes[] = {{"out", outp, span}, {"work", work, k.hd.total}};
    const nz_named_plane reads[] = {{"height", height, span}, {"drainage", drainage, span}, {"hardness", a.hardness, span},
                                    {"upliftMap", a.upliftMap, span}};
    NZ_TRY(nz_require_disjoint(writes, std::size(writes), reads, std::size(reads)));
    const nz_named_plane all[] = {writes[0], writes[1], reads[0], reads[1], reads[2], reads[3]};
    NZ_TRY(check_stripe_words(changed, "changed", proceed, "proceed", all, std::size(all)));
    const int sweeps = fluvial_implicit_sweeps.load();
    const int zlo = nz_stripe_grid_lo(*st), zhi = nz_stripe_grid_hi(*st) - 1;
    return run_stripe_round(
        ctx, out_handle, desc->maxPasses, k.hd, outp, k.h2, proceed, changed, first, g,
        [&]() -> int32_t {  // the receiver bytes and coefficients of a round that continues stand in `work`
            if (!first) return NZ_OK;
            return nz_launch_fluvial_implicit_stripe_setup(ctx->stream, height, drainage, a.hardness, a.upliftMap, k.recv, k.b,
                                                           k.f, k.hd.status, a.erodibility, a.uplift, a.dt, a.seaLevel, g, zlo,
                                                           zhi);
        },
        [&](int p, const float *h_in, float *h_out, const unsigned char *flags_in, unsigned char *flags_out) {
            return nz_launch_fluvial_implicit_stripe_pass(ctx->stream, k.recv, k.b, k.f, h_in, h_out, height, k.hd.status,
                                                          flags_in, flags_out, changed, g, zlo, zhi, first != 0, p, sweeps);
        });
}

extern "C" int32_t nz_implicit_fluvial_stripe_finalise(nz_ctx *ctx, const float *height, float *outp, const nz_stripe *st,
                                                       const int32_t *converged, nz_handle dep, nz_handle *out_handle) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(nz_check_stripe(st, 0));
    NZ_REQUIRE(height, "height is NULL");
    NZ_REQUIRE(outp, "out is NULL");
    NZ_REQUIRE(converged, "converged is NULL");
    const size_t span = nz_stripe_span(*st);
    NZ_REQUIRE(!nz_planes_overlap(outp, span, height, span), "out overlaps height");
    NZ_REQUIRE(!nz_bytes_overlap(converged, 4, outp, span * 4), "converged overlaps out");
    nz_ctx_handle_rides(ctx, out_handle != nullptr);
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_fluvial_implicit_stripe_finalise(ctx->stream, height, outp, converged, nz_geom_from_stripe(*st)));
    return nz_ctx_finish(ctx, out_handle);
}

// ---------------------------------------------------------------------------------------------
// multiple-flow implicit fluvial erosion: the implicit step along every descent (new-framework feature,
// include/noize_hip.h, nz_fluvial_implicit_mfd.hip)
// ---------------------------------------------------------------------------------------------
// `work`: the head, one gate byte per cell, the plane b, the eight planes f and the second h' plane; the first h' plane is
// the caller's `out`.  The checks (check_implicit_scalars, check_implicit_planes), the begin and the finalise launch are
// fluvial_implicit_impl's.
namespace {
struct fluvial_mfd_work { relax_work hd; unsigned char *gate; float *b, *f, *h2; };
fluvial_mfd_work fluvial_mfd_work_of(float *work, const relax_shape &sh) {
    fluvial_mfd_work k{relax_work(work, sh), nullptr, nullptr, nullptr, nullptr};
    k.gate = k.hd.bytes(sh.n);
    k.b = k.hd.floats(sh.n);
    k.f = k.hd.floats(8 * sh.n);
    k.h2 = k.hd.floats(sh.n);
    return k;
}
sweep_cap fluvial_implicit_mfd_sweeps;
}  // namespace

extern "C" size_t nz_fluvial_implicit_mfd_work_floats(int32_t resolution, int32_t count) {
    if (resolution <= 0 || count <= 0) return 0;
    return fluvial_mfd_work_of(nullptr, tile_shape(resolution, count)).hd.total;
}

extern "C" int32_t nz_debug_fluvial_implicit_mfd_sweeps(int32_t sweeps) { return fluvial_implicit_mfd_sweeps.exchange(sweeps); }

static int32_t fluvial_implicit_mfd_impl(nz_ctx *ctx, const float *height, const float *drainage, float *outp, float *work,
                                         const nz_fluvial_implicit_mfd_desc *d, int res, int count, nz_handle dep,
                                         nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    if (res == 0 || count == 0) return nz_ctx_finish(ctx, out);  // an empty payload: nothing to do
    NZ_TRY(check_batch(res, count));
    NZ_REQUIRE(d, "desc is NULL");
    const implicit_args a = implicit_args_of(*d);
    NZ_TRY(check_implicit_scalars(height, drainage, outp, work, a));
    NZ_REQUIRE(d->exponent >= 1 && d->exponent <= 16, "exponent %d outside 1..16", d->exponent);
    const relax_shape sh = tile_shape(res, count);
    const fluvial_mfd_work k = fluvial_mfd_work_of(work, sh);
    const size_t n = sh.n;
    NZ_TRY(check_implicit_planes(height, drainage, outp, work, k.hd.total, a, res, count, n));
    float *planes[2] = {outp, k.h2};
    const int sweeps = fluvial_implicit_mfd_sweeps.load();
    NZ_TRY(nz_launch_fluvial_implicit_begin(ctx->stream, k.hd.status, d->proceed));
    NZ_TRY(nz_launch_fluvial_implicit_mfd_setup(ctx->stream, height, drainage, d->hardness, d->upliftMap, k.gate, k.b, k.f,
                                                k.hd.status, d->erodibility, d->uplift, d->dt, d->seaLevel, res, count,
                                                d->exponent));
    return run_tile_series(
        ctx, out, d->maxPasses, k.hd,
        [&](int p, const unsigned char *flags_in, unsigned char *flags_out) {  // pass p writes plane p & 1
            return nz_launch_fluvial_implicit_mfd_pass(ctx->stream, k.gate, k.b, k.f, p ? planes[(p - 1) & 1] : nullptr,
                                                       planes[p & 1], k.hd.status, flags_in, flags_out, res, count, p, sweeps);
        },
        // a series at rest holds the fixed point in both planes, so `out` has it whichever plane was written last
        [&] { return nz_launch_fluvial_implicit_finalise(ctx->stream, height, outp, k.hd.status, d->tally, n); });
}

extern "C" int32_t nz_fluvial_implicit_mfd(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                                           const nz_fluvial_implicit_mfd_desc *desc, int32_t resolution, nz_handle dep,
                                           nz_handle *out_handle) {
    return fluvial_implicit_mfd_impl(ctx, height, drainage, out, work, desc, resolution, 1, dep, out_handle);
}

extern "C" int32_t nz_fluvial_implicit_mfd_batch(nz_ctx *ctx, const float *height, const float *drainage, float *out,
                                                 float *work, const nz_fluvial_implicit_mfd_desc *desc, int32_t resolution,
                                                 int32_t count, nz_handle dep, nz_handle *out_handle) {
    return fluvial_implicit_mfd_impl(ctx, height, drainage, out, work, desc, resolution, count, dep, out_handle);
}

// ---------------------------------------------------------------------------------------------
// implicit fluvial erosion with sediment deposition: the xi-q iteration around the implicit solve (new-framework feature,
// include/noize_hip.h, nz_fluvial_sediment.hip)
// ---------------------------------------------------------------------------------------------
// `work`: the head -- words 0..2 the totals {passes, converged, residual}, words 8.. the solve's status words -- the
// accumulation's status words, one receiver and one donor byte per cell, the planes b0, f, e (which bk overwrites), two Q
// planes and two h' planes.  The checks (check_implicit_scalars, check_implicit_planes), the setup launch and every solve
// pass are fluvial_implicit_impl's.
namespace {
struct fluvial_sediment_work {
    relax_work hd;
    int *solve, *accum;
    unsigned char *recv, *donors;
    float *b0, *f, *eb, *q[2], *h[2];
};
fluvial_sediment_work fluvial_sediment_work_of(float *work, const relax_shape &sh) {
    fluvial_sediment_work k{relax_work(work, sh), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, {}, {}};
    k.solve = k.hd.status ? k.hd.status + 8 : nullptr;
    k.accum = k.hd.ints(16);
    k.recv = k.hd.bytes(sh.n);
    k.donors = k.hd.bytes(sh.n);
    k.b0 = k.hd.floats(sh.n);
    k.f = k.hd.floats(sh.n);
    k.eb = k.hd.floats(sh.n);
    for (float *&p : k.q) p = k.hd.floats(sh.n);
    for (float *&p : k.h) p = k.hd.floats(sh.n);
    return k;
}
sweep_cap fluvial_sediment_sweeps;
}  // namespace

extern "C" size_t nz_fluvial_sediment_work_floats(int32_t resolution, int32_t count) {
    if (resolution <= 0 || count <= 0) return 0;
    return fluvial_sediment_work_of(nullptr, tile_shape(resolution, count)).hd.total;
}

extern "C" int32_t nz_debug_fluvial_sediment_sweeps(int32_t sweeps) { return fluvial_sediment_sweeps.exchange(sweeps); }

static int32_t fluvial_sediment_impl(nz_ctx *ctx, const float *height, const float *drainage, float *outp, float *work,
                                     const nz_fluvial_sediment_desc *d, int res, int count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    if (res == 0 || count == 0) return nz_ctx_finish(ctx, out);  // an empty payload: nothing to do
    NZ_TRY(check_batch(res, count));
    NZ_REQUIRE(d, "desc is NULL");
    const implicit_args a = implicit_args_of(*d);
    NZ_TRY(check_implicit_scalars(height, drainage, outp, work, a));
    NZ_REQUIRE(std::isfinite(d->deposition), "deposition is not finite");
    NZ_REQUIRE(d->deposition >= 0.0f, "deposition %g < 0", (double)d->deposition);
    NZ_REQUIRE(d->iterations >= 0, "iterations %d < 0", d->iterations);
    const relax_shape sh = tile_shape(res, count);
    const fluvial_sediment_work k = fluvial_sediment_work_of(work, sh);
    const size_t n = sh.n;
    NZ_TRY(check_implicit_planes(height, drainage, outp, work, k.hd.total, a, res, count, n));
    const nz_named_plane others[] = {{"out", outp, n},           {"work", work, k.hd.total},  {"height", height, n},
                                     {"drainage", drainage, n}, {"hardness", a.hardness, n}, {"upliftMap", a.upliftMap, n}};
    for (const auto &p : others) NZ_REQUIRE(!nz_planes_overlap(d->flux, n, p.p, p.floats), "flux overlaps %s", p.name);
    NZ_REQUIRE(!nz_bytes_overlap(a.tally, 8, d->flux, n * sizeof(float)), "flux overlaps tally");
    NZ_REQUIRE(!nz_bytes_overlap(a.proceed, 4, d->flux, n * sizeof(float)), "flux overlaps proceed");
    const float G = d->deposition + 0.0f;  // -0 -> +0
    const int K = d->iterations, sweeps = fluvial_sediment_sweeps.load();
    int *totals = k.hd.status;
    hipStream_t s = ctx->stream;
    NZ_TRY(nz_launch_fluvial_sediment_begin(s, totals, k.solve, d->proceed));
    NZ_TRY(nz_launch_fluvial_implicit_setup(s, height, drainage, d->hardness, d->upliftMap, k.recv, k.b0, k.f, k.solve,
                                            d->erodibility, d->uplift, d->dt, d->seaLevel, res, count));
    if (K > 0) NZ_TRY(nz_launch_fluvial_sediment_mask(s, height, k.donors, k.solve, d->seaLevel, res, count));
    nz_ctx_handle_rides(ctx, out != nullptr);
    // solve series j reads the right-hand side b; series K alternates between `out` and h[1], the ones before between h[0]
    // and h[1]: h[0] keeps h(K-1), and `out` is written by the last series alone
    auto solve_series = [&](int j, const float *b) -> int32_t {
        float *planes[2] = {j == K ? outp : k.h[0], k.h[1]};
        for (int p = 0; p < d->maxPasses; p++)
            NZ_TRY(nz_launch_fluvial_implicit_pass(s, k.recv, b, k.f, p ? planes[(p - 1) & 1] : nullptr, planes[p & 1], k.solve,
                                                   k.hd.flags[(p - 1) & 1], k.hd.flags[p & 1], res, count, p, sweeps));
        return NZ_OK;
    };
    NZ_TRY(solve_series(0, k.b0));
    for (int j = 1; j <= K; j++) {
        NZ_TRY(nz_launch_fluvial_sediment_source(s, k.b0, k.h[0], k.eb, k.solve, k.accum, totals, n));
        for (int p = 0; p < d->maxPasses; p++)
            NZ_TRY(nz_launch_fluvial_sediment_gather_pass(s, k.donors, k.eb, p ? k.q[(p - 1) & 1] : nullptr, k.q[p & 1],
                                                          k.accum, k.hd.flags[(p - 1) & 1], k.hd.flags[p & 1], res, count, p,
                                                          sweeps));
        // a series at rest holds the fixed point in both planes
        NZ_TRY(nz_launch_fluvial_sediment_deposit(s, k.donors, k.q[0], k.b0, drainage, height, k.eb, k.accum, k.solve, totals, G,
                                                  d->seaLevel, res, count));
        NZ_TRY(solve_series(j, k.eb));
    }
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_fluvial_sediment_finalise(s, height, outp, K ? k.h[0] : nullptr, K ? k.q[0] : nullptr, d->flux, k.solve,
                                               totals, d->tally, n));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_fluvial_sediment(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                                       const nz_fluvial_sediment_desc *desc, int32_t resolution, nz_handle dep,
                                       nz_handle *out_handle) {
    return fluvial_sediment_impl(ctx, height, drainage, out, work, desc, resolution, 1, dep, out_handle);
}

extern "C" int32_t nz_fluvial_sediment_batch(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                                             const nz_fluvial_sediment_desc *desc, int32_t resolution, int32_t count,
                                             nz_handle dep, nz_handle *out_handle) {
    return fluvial_sediment_impl(ctx, height, drainage, out, work, desc, resolution, count, dep, out_handle);
}

// ---------------------------------------------------------------------------------------------
// hillslope diffusion: one implicit step of any size as two tridiagonal line solves (new-framework feature,
// include/noize_hip.h, nz_hillslope.hip)
// ---------------------------------------------------------------------------------------------
// `work`: the tables inv and cp, one entry per line position each, the second starting 16-byte aligned behind the first.
// The lines of every tile of a batch share them.
namespace {
size_t hillslope_table_floats(int res) { return ((size_t)res + 3) & ~(size_t)3; }
}  // namespace

extern "C" size_t nz_hillslope_diffusion_work_floats(int32_t resolution, int32_t count) {
    if (resolution <= 0 || count <= 0) return 0;
    return 2 * hillslope_table_floats(resolution);
}

static int32_t hillslope_impl(nz_ctx *ctx, const float *height, float *outp, float *work, const nz_hillslope_desc *d, int res,
                              int count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    if (res == 0 || count == 0) return nz_ctx_finish(ctx, out);  // an empty payload: nothing to do
    NZ_TRY(check_batch(res, count));
    NZ_REQUIRE(d, "desc is NULL");
    NZ_REQUIRE(height, "height is NULL");
    NZ_REQUIRE(outp, "out is NULL");
    NZ_REQUIRE(work, "work is NULL");
    NZ_REQUIRE(std::isfinite(d->diffusivity), "diffusivity is not finite");
    NZ_REQUIRE(std::isfinite(d->dt), "dt is not finite");
    NZ_REQUIRE(d->diffusivity >= 0.0f, "diffusivity %g < 0", (double)d->diffusivity);
    NZ_REQUIRE(d->dt >= 0.0f, "dt %g < 0", (double)d->dt);
    const float r = d->diffusivity * d->dt;  // the model's one product
    NZ_REQUIRE(std::isfinite(r), "diffusivity %g x dt %g: r is not finite", (double)d->diffusivity, (double)d->dt);
    NZ_REQUIRE(std::isfinite(1.0f + 2.0f * r), "diffusivity %g x dt %g: 1 + 2 r is not finite", (double)d->diffusivity,
               (double)d->dt);
    NZ_REQUIRE(d->iterations >= 1, "iterations %d < 1", d->iterations);
    const size_t n = (size_t)count * res * res;
    NZ_REQUIRE(n <= (size_t)INT32_MAX, "count %d x resolution %d^2: %zu cells are beyond int32", count, res, n);
    const size_t table = hillslope_table_floats(res);
    const bool in_place = outp == height;  // the same pointer: allowed; anything else must lie apart
    const nz_named_plane writes[] = {{"work", work, 2 * table}, {"out", outp, n}};
    const nz_named_plane reads[] = {{"height", in_place ? nullptr : height, n}};
    NZ_TRY(nz_require_disjoint(writes, std::size(writes), reads, std::size(reads)));
    if (res < 3 || r == 0.0f) {  // out = h bit for bit, by definition
        if (!in_place) NZ_TRY(nz_launch_copy(ctx->stream, outp, height, n));
        return nz_ctx_finish(ctx, out);
    }
    float *inv = work, *cp = work + table;
    NZ_TRY(nz_launch_hillslope_tables(ctx->stream, inv, cp, r, res));
    for (int i = 0; i < d->iterations; i++)  // the first step reads the heights, every later one runs in place on `out`
        NZ_TRY(nz_launch_hillslope_step(ctx->stream, i ? outp : height, outp, inv, cp, r, res, count));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_hillslope_diffusion(nz_ctx *ctx, const float *height, float *out, float *work,
                                          const nz_hillslope_desc *desc, int32_t resolution, nz_handle dep,
                                          nz_handle *out_handle) {
    return hillslope_impl(ctx, height, out, work, desc, resolution, 1, dep, out_handle);
}

extern "C" int32_t nz_hillslope_diffusion_batch(nz_ctx *ctx, const float *height, float *out, float *work,
                                                const nz_hillslope_desc *desc, int32_t resolution, int32_t count,
                                                nz_handle dep, nz_handle *out_handle) {
    return hillslope_impl(ctx, height, out, work, desc, resolution, count, dep, out_handle);
}

// ---------------------------------------------------------------------------------------------
// upsample / downsample (new-framework feature, include/noize_hip.h, nz_resample.hip)
// ---------------------------------------------------------------------------------------------
static int32_t check_resample(int32_t factor, int32_t filter) {
    NZ_REQUIRE(factor == 2 || factor == 4 || factor == 8, "factor %d is not 2, 4 or 8", factor);
    NZ_REQUIRE(filter >= NZ_RESAMPLE_NEAREST && filter <= NZ_RESAMPLE_CATMULL_ROM, "filter %d is not a resample filter",
               filter);
    return NZ_OK;
}

// the planes of a call: src read, dst written (fine_n / coarse_n floats each way round), base NULL, dst or apart from dst
static int32_t check_resample_planes(const float *src, size_t src_n, const float *dst, size_t dst_n, const float *base) {
    NZ_REQUIRE(src, "src is NULL");
    NZ_REQUIRE(dst, "dst is NULL");
    NZ_REQUIRE(dst_n < ((size_t)1 << 31), "dst: an output of %zu cells (2^31 or more)", dst_n);
    NZ_REQUIRE(!nz_planes_overlap(dst, dst_n, src, src_n), "dst overlaps src");
    NZ_REQUIRE(!base || base == dst || !nz_planes_overlap(dst, dst_n, base, dst_n), "base partly overlaps dst");
    return NZ_OK;
}

static int32_t upsample_impl(nz_ctx *ctx, const float *src, int32_t res, float *dst, int32_t factor, int32_t filter,
                             const float *base, int32_t count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_resample(factor, filter));
    NZ_REQUIRE(res >= 1, "srcResolution %d < 1", res);
    NZ_REQUIRE(count >= 1 && count <= 65535, "count %d out of range [1,65535]", count);
    // 46340^2 < 2^31 <= 46341^2: bounding the side first keeps every product below from wrapping
    NZ_REQUIRE(res <= 46340 / factor, "dst: an output of 2^31 cells or more (srcResolution %d x factor %d)", res, factor);
    const size_t fine = (size_t)res * factor;
    NZ_TRY(check_resample_planes(src, (size_t)count * res * res, dst, (size_t)count * fine * fine, base));
    nz_up_geom g{};
    g.ccols = g.cpitch = g.crows = g.cgrows = res;
    g.fcols = g.fpitch = g.w1 = (int)fine;
    g.cstride = (size_t)res * res;
    g.fstride = fine * fine;
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_upsample(ctx->stream, src, dst, base, g, factor, filter, count));
    return nz_ctx_finish(ctx, out);
}

static int32_t downsample_impl(nz_ctx *ctx, const float *src, int32_t res, float *dst, int32_t factor, int32_t count,
                               nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_resample(factor, NZ_RESAMPLE_NEAREST));
    NZ_REQUIRE(res >= 1, "srcResolution %d < 1", res);
    NZ_REQUIRE(res % factor == 0, "srcResolution %d is not divisible by factor %d", res, factor);
    NZ_REQUIRE(count >= 1 && count <= 65535, "count %d out of range [1,65535]", count);
    const size_t coarse = (size_t)(res / factor);
    NZ_REQUIRE(res <= 46340 && (size_t)count * res * res < ((size_t)1 << 31), "src: an input of 2^31 cells or more");
    NZ_TRY(check_resample_planes(src, (size_t)count * res * res, dst, (size_t)count * coarse * coarse, nullptr));
    nz_down_geom g{};
    g.ccols = g.cpitch = g.w1 = (int)coarse;
    g.fpitch = res;
    g.cstride = coarse * coarse;
    g.fstride = (size_t)res * res;
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_downsample(ctx->stream, src, dst, g, factor, count));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_upsample(nz_ctx *ctx, const float *src, int32_t srcResolution, float *dst, int32_t factor,
                               int32_t filter, const float *base, nz_handle dep, nz_handle *out) {
    return upsample_impl(ctx, src, srcResolution, dst, factor, filter, base, 1, dep, out);
}

extern "C" int32_t nz_upsample_batch(nz_ctx *ctx, const float *src, int32_t srcResolution, float *dst, int32_t factor,
                                     int32_t filter, const float *base, int32_t count, nz_handle dep, nz_handle *out) {
    return upsample_impl(ctx, src, srcResolution, dst, factor, filter, base, count, dep, out);
}

extern "C" int32_t nz_downsample(nz_ctx *ctx, const float *src, int32_t srcResolution, float *dst, int32_t factor,
                                 nz_handle dep, nz_handle *out) {
    return downsample_impl(ctx, src, srcResolution, dst, factor, 1, dep, out);
}

extern "C" int32_t nz_downsample_batch(nz_ctx *ctx, const float *src, int32_t srcResolution, float *dst, int32_t factor,
                                       int32_t count, nz_handle dep, nz_handle *out) {
    return downsample_impl(ctx, src, srcResolution, dst, factor, count, dep, out);
}

extern "C" int32_t nz_upsample_stripe_halo_rows(int32_t filter) {
    return filter >= NZ_RESAMPLE_NEAREST && filter <= NZ_RESAMPLE_CATMULL_ROM ? nz_resample_halo(filter) : 0;
}

// the two stripes of a resampling call: each a valid stripe of its own grid (no ghost rows demanded of the output), the
// fine grid f times the coarse one
static int32_t check_resample_stripes(const nz_stripe *coarse, const char *cname, const nz_stripe *fine, const char *fname,
                                      int factor) {
    NZ_REQUIRE(coarse, "%s is NULL", cname);
    NZ_REQUIRE(fine, "%s is NULL", fname);
    NZ_TRY(nz_check_stripe(coarse, 0));
    NZ_TRY(nz_check_stripe(fine, 0));
    NZ_REQUIRE((int64_t)coarse->cols * factor == fine->cols && (int64_t)coarse->grows * factor == fine->grows,
               "%s / %s: the fine grid %d x %d is not %d times the coarse grid %d x %d", cname, fname, fine->grows,
               fine->cols, factor, coarse->grows, coarse->cols);
    return NZ_OK;
}

extern "C" int32_t nz_upsample_stripe(nz_ctx *ctx, const float *src, const nz_stripe *srcSt, float *dst,
                                      const nz_stripe *dstSt, int32_t factor, int32_t filter, const float *base,
                                      nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_resample(factor, filter));
    NZ_TRY(check_resample_stripes(srcSt, "srcSt", dstSt, "dstSt", factor));
    NZ_REQUIRE(src, "src is NULL");
    NZ_REQUIRE(dst, "dst is NULL");
    NZ_REQUIRE(nz_stripe_plane_floats(dstSt) < ((size_t)1 << 31), "dst: an output of 2^31 cells or more");
    NZ_REQUIRE(!nz_planes_overlap(dst, nz_stripe_span(*dstSt), src, nz_stripe_span(*srcSt)), "dst overlaps src");
    NZ_REQUIRE(!base || base == dst || !nz_planes_overlap(dst, nz_stripe_span(*dstSt), base, nz_stripe_span(*dstSt)),
               "base partly overlaps dst");
    nz_up_geom g{};
    g.ccols = srcSt->cols;
    g.cpitch = nz_stripe_pitch(*srcSt);
    g.crows = srcSt->rows;
    g.cgrow0 = srcSt->grow0;
    g.cgrows = srcSt->grows;
    g.fcols = dstSt->cols;
    g.fpitch = nz_stripe_pitch(*dstSt);
    g.fgrow0 = dstSt->grow0;
    g.w0 = dstSt->own0;
    g.w1 = dstSt->own1;
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_upsample(ctx->stream, src, dst, base, g, factor, filter, 1));  // refuses a missing ghost row
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_downsample_stripe(nz_ctx *ctx, const float *src, const nz_stripe *srcSt, float *dst,
                                        const nz_stripe *dstSt, int32_t factor, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_resample(factor, NZ_RESAMPLE_NEAREST));
    NZ_TRY(check_resample_stripes(dstSt, "dstSt", srcSt, "srcSt", factor));
    NZ_REQUIRE(src, "src is NULL");
    NZ_REQUIRE(dst, "dst is NULL");
    NZ_REQUIRE(nz_stripe_plane_floats(srcSt) < ((size_t)1 << 31), "src: an input of 2^31 cells or more");
    NZ_REQUIRE(!nz_planes_overlap(dst, nz_stripe_span(*dstSt), src, nz_stripe_span(*srcSt)), "dst overlaps src");
    // output global rows [g0, g1) read fine global rows [f g0, f g1): all of them in the source buffer
    const int64_t f0 = (int64_t)(dstSt->own0 + dstSt->grow0) * factor - srcSt->grow0;
    const int64_t f1 = (int64_t)(dstSt->own1 + dstSt->grow0) * factor - srcSt->grow0;
    NZ_REQUIRE(dstSt->own1 == dstSt->own0 || (f0 >= 0 && f1 <= srcSt->rows),
               "srcSt: fine rows [%lld, %lld) of the buffer are required, it holds %d", (long long)f0, (long long)f1,
               srcSt->rows);
    nz_down_geom g{};
    g.ccols = dstSt->cols;
    g.cpitch = nz_stripe_pitch(*dstSt);
    g.cgrow0 = dstSt->grow0;
    g.fpitch = nz_stripe_pitch(*srcSt);
    g.fgrow0 = srcSt->grow0;
    g.w0 = dstSt->own0;
    g.w1 = dstSt->own1;
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_downsample(ctx->stream, src, dst, g, factor, 1));
    return nz_ctx_finish(ctx, out);
}
