// nz_stages.cpp -- the extern "C" stage entry points of libnoize_hip.so (one per reference job delegate or
// PipelineStage.Schedule body, include/noize_hip.h) and the launch planners behind them.
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "nz_internal.hpp"

// ---------------------------------------------------------------------------------------------
// helpers shared by the stage entry points
// ---------------------------------------------------------------------------------------------
int32_t nz_check_stripe(const nz_stripe *st, int halo, int halo_below) {
    if (halo_below < 0) halo_below = halo;  // symmetric stencil
    NZ_REQUIRE(st, "stripe is NULL");
    NZ_REQUIRE(st->cols > 0 && st->rows > 0 && st->grows > 0, "stripe: non-positive extent");
    NZ_REQUIRE(st->pitch == 0 || st->pitch >= st->cols, "stripe: pitch < cols");
    NZ_REQUIRE(st->own0 >= 0 && st->own0 <= st->own1 && st->own1 <= st->rows, "stripe: owned rows outside buffer");
    NZ_REQUIRE(st->own0 + st->grow0 >= 0 && st->own1 + st->grow0 <= st->grows,
               "stripe: owned rows outside the global grid");
    // every row within `halo` of the owned rows must be in the buffer unless it is beyond the border
    int need_lo = st->own0 - halo, need_hi = st->own1 - 1 + halo_below;
    int dom_lo = -st->grow0, dom_hi = st->grows - 1 - st->grow0;
    if (need_lo < dom_lo) need_lo = dom_lo;
    if (need_hi > dom_hi) need_hi = dom_hi;
    NZ_REQUIRE(need_lo >= 0 && need_hi <= st->rows - 1, "stripe: %d ghost rows required above, %d below", halo,
               halo_below);
    return NZ_OK;
}

static int32_t check_res(int32_t resolution) {
    NZ_REQUIRE(resolution >= 1 && resolution <= 46340, "resolution %d out of range", resolution);
    return NZ_OK;
}

// FractalJob.CalcFractalNormValue, Noise/Fractal/Fractal.cs:31-40 (startingAmplitude is ignored)
static float calc_fractal_norm(float hurst, int octaves) {
    float G = exp2f(-hurst);
    float a = 1.0f, t = 0.0f;
    for (int i = 0; i < octaves; i++) {
        t += a * 1.0f;
        a *= G;
    }
    return t;
}

// largest |f| of FractalGenerator.NoiseValue's recurrence (Fractal.cs:121-127): lets a kernel decide once per row
// whether every octave stays inside the range its lattice tables cover
static float fractal_fmax(float stepdown, float detune, int octaves) {
    float fmax = 0.0f, f = 1.0f, det = 0.0f;
    for (int i = 0; i < octaves; i++) {
        if (!(fabsf(f) <= fmax)) fmax = fabsf(f);
        det += detune;
        f *= (stepdown - det);
    }
    return fmax;
}

static int32_t fractal_impl(nz_ctx *ctx, hipStream_t stream, int noiseType, float *dst, int rows, int cols, int pitch,
                            float hurst,
                            float amp, float stepdown, float detune, int octaves, int xpos, int zpos_first_row,
                            int noiseSize, int count = 1, size_t bstride = 0, const int32_t *positions = nullptr,
                            int shape = NZ_SHAPE_FBM, float ridgeOffset = 1.0f, float ridgeGain = 2.0f,
                            const nz_warp_params *warp = nullptr) {
    NZ_REQUIRE(dst, "src is NULL");
    NZ_REQUIRE(noiseType >= 0 && noiseType <= NZ_NOISE_DOMAIN_ROTATED_SIMPLEX, "unknown noise type %d", noiseType);
    NZ_REQUIRE(octaves >= 0, "octaves < 0");
    NZ_REQUIRE(noiseSize != 0, "noiseSize == 0");
    nz_fractal_params p;
    p.posx = (float)xpos;  // SetPosition, Fractal.cs:109-112
    p.posz = (float)zpos_first_row;
    p.noise_size = (float)noiseSize;
    p.G = exp2f(-hurst);
    p.amp = amp;
    p.stepdown = stepdown;
    p.detune_rate = detune;
    p.norm = calc_fractal_norm(hurst, octaves);
    p.octaves = octaves;
    p.shape = shape;
    p.ridge.offset = ridgeOffset;
    p.ridge.gain = ridgeGain;
    p.fmax = fractal_fmax(stepdown, detune, octaves);
    // domain warp: the displacement loop's norm and frequency bound, the same two values for warp->octaves
    nz_warp_params wp;
    if (warp) {
        wp = *warp;
        wp.norm = calc_fractal_norm(hurst, wp.octaves);
        wp.fmax = fractal_fmax(stepdown, detune, wp.octaves);
    }
    return nz_launch_fractal(stream, noiseType, dst, rows, cols, pitch, p, ctx->d_rgrad, ctx->d_simplex, count, bstride,
                             positions, warp ? &wp : nullptr);
}

// SeparableKernelFilter tables, Filter/Kernel/KernelJob.cs:97-136.  Gaussian bodies are
// exp(-i^2/2s^2)/sum in double rounded to fp32, which reproduces the reference literals
// (tests/golden/gauss_tables.json).
static void gauss_coeffs(double sigma, int width, float *out) {
    int o = (width - 1) / 2;
    double w[NZ_MAX_KSIZE], sum = 0.0;
    for (int i = 0; i < width; i++) {
        double d = (double)(i - o);
        w[i] = exp(-(d * d) / (2.0 * sigma * sigma));
        sum += w[i];
    }
    for (int i = 0; i < width; i++) out[i] = (float)(w[i] / sum);
}

static int32_t filter_taps(int32_t filter, nz_kernel_taps *t) {
    memset(t, 0, sizeof *t);
    auto set3 = [&](float a0, float a1, float a2, float b0, float b1, float b2, float f) {
        t->kx[0] = a0; t->kx[1] = a1; t->kx[2] = a2;
        t->kz[0] = b0; t->kz[1] = b1; t->kz[2] = b2;
        t->factor = f;
        t->ksize = 3;
    };
    switch (filter) {
        case NZ_GAUSS9_S1: case NZ_GAUSS7_S1: case NZ_GAUSS5_S1: case NZ_GAUSS3_S1:
        case NZ_GAUSS9_S2: case NZ_GAUSS7_S2: case NZ_GAUSS5_S2: case NZ_GAUSS3_S2: {
            static const int sizes[4] = {9, 7, 5, 3};
            int w = sizes[filter & 3];
            double sigma = filter >= NZ_GAUSS9_S2 ? 2.0 : 1.0;
            gauss_coeffs(sigma, w, t->kx);
            gauss_coeffs(sigma, w, t->kz);
            t->factor = 1.0f;
            t->ksize = w;
            return NZ_OK;
        }
        case NZ_SMOOTH3: set3(1, 1, 1, 1, 1, 1, 1.0f / 3.0f); return NZ_OK;          // KernelJob.cs:107-108
        case NZ_SOBEL3_HORIZONTAL: set3(-1, 0, 1, 1, 2, 1, 1.0f); return NZ_OK;       // :110-116
        case NZ_SOBEL3_VERTICAL: set3(1, 2, 1, 1, 0, -1, 1.0f); return NZ_OK;         // :117-122
        case NZ_PREWITT3_HORIZONTAL: set3(1, 0, -1, 1, 1, 1, 1.0f); return NZ_OK;     // :124-130
        case NZ_PREWITT3_VERTICAL: set3(1, 1, 1, -1, 0, 1, 1.0f); return NZ_OK;       // :131-136
        case NZ_SOBEL3_2D:
            nz_set_error("Sobel3_2D is not a single separable pass (ScheduleReduce, KernelJob.cs:187-215)");
            return NZ_ERR_UNSUPPORTED;
    }
    nz_set_error("unknown KernelFilterType %d", filter);
    return NZ_ERR_INVALID;
}

// BlurHelper.limitWidth, Filter/Kernel/Blur/BlurKernels.cs:29-36
static int limit_width(int width) {
    if (width % 2 == 0) width += 1;
    if (width > 25) width = 25;
    return width < 3 ? 3 : width;
}

// GaussFilter.Schedule, Filter/Kernel/Blur/BlurJob.cs:11-21: body of limitWidth(width) taps, pass run
// with kernelSize = width as given
static int32_t gauss_taps(int32_t width, int32_t sigma, nz_kernel_taps *t) {
    memset(t, 0, sizeof *t);
    NZ_REQUIRE(sigma >= 0 && sigma <= 15, "GaussSigma %d out of range", sigma);
    int w = limit_width(width);
    NZ_REQUIRE(width >= 1 && width <= w, "gauss width %d indexes outside its %d-tap kernel", width, w);
    gauss_coeffs(0.5 * (double)(sigma + 1), w, t->kx);
    memcpy(t->kz, t->kx, sizeof t->kx);
    t->factor = 1.0f;
    t->ksize = width;
    return NZ_OK;
}

// SmoothFilter.Schedule BlurJob.cs:34-44; SmoothBlur.GetKernel BlurKernels.cs:39-43
static int32_t smooth_taps(int32_t width, nz_kernel_taps *t) {
    memset(t, 0, sizeof *t);
    NZ_REQUIRE(width >= 1 && width <= NZ_MAX_KSIZE, "smooth width %d out of range [1,25]", width);
    for (int i = 0; i < width; i++) t->kx[i] = t->kz[i] = 1.0f / (float)width;
    t->factor = 1.0f;
    t->ksize = width;
    return NZ_OK;
}

static int conv_tcap(int ksize) {
    int hw = nz_conv_max_fused(ksize);
    if (hw == 0) return 0;
    int cap;
    switch (ksize) {  // fusion depth per launch (tuned on MI355X; other depths lost every measurement, HISTORY.md)
        case 3: cap = 6; break;
        case 5: cap = 5; break;
        case 7: cap = 3; break;
        default: cap = 3; break;
    }
    return cap < hw ? cap : hw;
}

// the copy back that ends an in-place series with an odd launch count: rows [or0, or1) of every grid, `from` -> `to`.
// It is the series' last operation, so the entry's handle rides on it.
static int32_t copy_back(nz_ctx *ctx, const nz_geom &g, float *to, const float *from) {
    const size_t off = (size_t)g.or0 * g.pitch;
    nz_ctx_arm_last_launch(ctx);
    return nz_launch_copy(ctx->stream, to + off, from + off, nz_geom_span(g));
}

// One launch per entry of `depths`, step(from, to, depth), ping-ponging src <-> tmp.  swapped == nullptr: the result must
// be back in `src`, and an odd launch count is followed by a copy back; otherwise (READ / WRITE pair, nz_rw_tile) *swapped
// tells whether the result is in `tmp`.  The operation that ends the series carries the entry's handle.
template <class Step>
static int32_t run_series(nz_ctx *ctx, const nz_geom &g, float *src, float *tmp, const std::vector<int> &depths,
                          bool *swapped, Step step) {
    const int L = (int)depths.size();
    const bool copy = !swapped && (L & 1);
    float *cur = src, *other = tmp;
    for (int i = 0; i < L; i++) {
        if (i == L - 1 && !copy) nz_ctx_arm_last_launch(ctx);
        NZ_TRY_(step(cur, other, depths[i]));
        std::swap(cur, other);
    }
    if (swapped) *swapped = (L & 1) != 0;
    return copy ? copy_back(ctx, g, src, tmp) : NZ_OK;
}

// `iterations` applications of (X pass, Z pass) as a series of launches (run_series): in place (swapped == nullptr) the
// fused applications are grouped into an even number of launches where they can be.
static int32_t conv_iterations(nz_ctx *ctx, float *src, float *tmp, const nz_geom &g, const nz_kernel_taps &t,
                               int iterations, bool *swapped = nullptr) {
    NZ_REQUIRE(src && tmp && src != tmp, "src/tmp must be two distinct planes");
    NZ_REQUIRE(iterations >= 1, "iterations < 1");
    if (swapped) *swapped = false;
    if (nz_conv_has_wide(t.ksize))  // one launch per application
        return run_series(ctx, g, src, tmp, nz_split_iterations(iterations, 1), swapped,
                          [&](const float *from, float *to, int) { return nz_launch_conv_wide(ctx->stream, from, to, g, t); });
    int cap = (t.ksize & 1) ? conv_tcap(t.ksize) : 0;
    // a small grid is served by one round of workgroups whatever the depth: one launch less beats the deeper halo
    // (512^2 tiles, READ / WRITE pair, 17 applications as 6 + 6 + 5 instead of 5 + 4 + 4 + 4: 11 100 -> 11 700 tiles/s)
    // ... and a grid of the reference's own tile sizes (256^2 .. 512^2: a hundred 64-row tiles whatever the depth, all resident
    // at once) waits for the LATENCY of its dependent applications, not for throughput: nine applications per launch, 17 = 9 + 8
    // in two launches instead of three (round 5: Gauss5 x17 at 256^2 / 512^2 52 -> 42 / 43 us, 13 100 -> 13 900 tiles/s one at a
    // time; from 1024^2 on the deeper halo costs more than the launch it saves: 55 -> 59 us)
    if (t.ksize == 5 && cap == 5 && nz_conv_small_grid(t.ksize, g))
        cap = nz_conv_tiny_grid(t.ksize, g) ? 9 : 6;
    if (cap == 0) {  // even or out-of-table sizes: the two passes as launched by the reference
        if (g.count > 1) {  // no batched form of the generic passes: grid by grid
            nz_geom one = g;
            one.count = 1;
            one.bstride = 0;
            for (int b = 0; b < g.count; b++)
                NZ_TRY_(conv_iterations(ctx, src + b * g.bstride, tmp + b * g.bstride, one, t, iterations, nullptr));
            return NZ_OK;
        }
        for (int i = 0; i < iterations; i++) {
            NZ_TRY_(nz_launch_conv_pass_x(ctx->stream, src, tmp, g, t));
            NZ_TRY_(nz_launch_conv_pass_z(ctx->stream, tmp, src, g, t));
        }
        return NZ_OK;
    }
    const std::vector<int> Ts = nz_split_iterations(iterations, cap, !swapped);
    const int L = (int)Ts.size();
    // three or more launches of a 5..9-tap kernel run as ONE grid with tile-level dependencies (nz_filter.hip,
    // conv_chain_kernel): Gauss5 x17 0.212 -> 0.198 ms at 4096^2.  Two launches gain nothing (Gauss9 x6 -3 %, Gauss5 x6
    // +2.5 %, two single applications +15 %: a tile's poll and its sc1 accesses cost what the missing launch boundary
    // saves), and the 64-row tiles of the 3-tap kernels lose (x6: 0.131 vs 0.066 ms).  NZ_CONV_CHAIN=0: never;
    // NZ_CONV_CHAIN=2: whenever there are two launches or more (the test suite runs the parity tests under it).
    static const int chain_mode = getenv("NZ_CONV_CHAIN") ? atoi(getenv("NZ_CONV_CHAIN")) : 1;
    // (where the row-streaming form of a launch applies -- big grids, 3 / 5 taps -- plain launches of it are faster still)
    const bool streamed = nz_conv_stream_wanted(g, t.ksize, Ts.front()) && nz_conv_stream_wanted(g, t.ksize, Ts.back());
    // (A small grid -- fewer than ~7 M cells, 64-row tiles -- chains from TWO launches on since round 5: with the ticket gone and
    // four rows per thread the chained grid wins there too.  Gauss5 x17 2048^2 87.2 -> 67.9 us, 2560^2 110.9 -> 95.0; 1024^2 by
    // itself 45.6 -> 47.3 us, in a tile's pipeline 10 550 -> 11 020 tiles/s (one launch to enqueue and to start instead of three);
    // 512^2 18 000 -> 18 100.  Rounds 3 - 4 kept separate launches here: 512^2 55.7 against 51.7 us then.)
    const bool chain_on = !streamed && !ctx->chain_off &&
                          (chain_mode == 2 ? L >= 2 : (chain_mode == 1 && t.ksize >= 5 && L >= (nz_conv_small_grid(t.ksize, g) ? 2 : 3)));
    if (chain_on && L <= 8 && g.count == 1 && (size_t)g.rows * g.pitch * 4 < ((size_t)1 << 32) &&
        (swapped || !(L & 1))) {
        // T must not decrease along the chain: a tile of launch l + 1 waits for the launch-l tiles whose INTERIOR meets
        // its input window (read after write); its own stores land in the plane launch l reads, and the launch-l tiles
        // that read that region are all among the awaited ones only while H(l) <= H(l + 1) (write after read)
        int Tc[8];
        for (int i = 0; i < L; i++) Tc[i] = Ts[L - 1 - i];
        int *flags = nullptr;
        unsigned epoch = 0, *err_host = nullptr, *err_epoch = nullptr;
        NZ_TRY_(nz_ctx_chain_state(ctx, (size_t)nz_conv_chain_items(t.ksize, g, Tc, L), &flags, &epoch, &err_host, &err_epoch));
        nz_ctx_arm_last_launch(ctx);  // (one launch; no copy follows in either form: an even count or a pair)
        NZ_TRY_(nz_launch_conv_chain(ctx->stream, src, tmp, g, t, Tc, L, flags, epoch, err_host, err_epoch));
        if (swapped) *swapped = (L & 1) != 0;
        return NZ_OK;
    }
    return run_series(ctx, g, src, tmp, Ts, swapped,
                      [&](const float *from, float *to, int T) { return nz_launch_conv_fused(ctx->stream, from, to, g, t, T); });
}

// ErosionKernelJob.ScheduleSeries KernelJob.cs:318-335: min-X then min-Z (size 3) = the min over {x-1,x} x {z-1,z}, up to
// nz_erosion_max_fused() of them per launch; in place, a single iteration is one launch into tmp and the copy back that
// stands for the flush
static int32_t erosion_iterations(nz_ctx *ctx, float *src, float *tmp, const nz_geom &g, int iterations,
                                  bool *swapped = nullptr) {
    NZ_REQUIRE(src && tmp && src != tmp, "src/tmp must be two distinct planes");
    NZ_REQUIRE(iterations >= 1, "iterations < 1");
    return run_series(ctx, g, src, tmp, nz_split_iterations(iterations, nz_erosion_max_fused(), !swapped), swapped,
                      [&](const float *from, float *to, int E) { return nz_launch_erosion_fused(ctx->stream, from, to, g, E); });
}

// what nz_comm.cpp (the sharded plan) needs of the above
int32_t nz_filter_taps(int32_t filter, nz_kernel_taps *t) { return filter_taps(filter, t); }
int nz_conv_tcap(int ksize) { return conv_tcap(ksize); }
int32_t nz_fractal_rows(nz_ctx *ctx, hipStream_t stream, int noiseType, float *dst, int rows, int cols, int pitch, float hurst,
                        float amp, float stepdown, float detune, int octaves, int xpos, int zpos_first_row, int noiseSize) {
    return fractal_impl(ctx, stream, noiseType, dst, rows, cols, pitch, hurst, amp, stepdown, detune, octaves, xpos,
                        zpos_first_row, noiseSize);
}

#define NZ_BEGIN(ctx, dep)                   \
    do {                                     \
        int32_t rc_ = nz_ctx_begin(ctx, dep); \
        if (rc_) return rc_;                 \
    } while (0)

#define NZ_TRY(expr)              \
    do {                          \
        int32_t rc_ = (expr);     \
        if (rc_) return rc_;      \
    } while (0)

// ---------------------------------------------------------------------------------------------
// noise
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nz_fractal(nz_ctx *ctx, int32_t noiseType, float *src, int32_t resolution, float hurst,
                              float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                              int32_t xpos, int32_t zpos, int32_t noiseSize, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, and nothing behind it: the handle rides on it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(fractal_impl(ctx, ctx->stream, noiseType, src, resolution, resolution, resolution, hurst, startingAmplitude,
                        stepdown, detuneRate, octaves, xpos, zpos, noiseSize));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_fractal_stripe(nz_ctx *ctx, int32_t noiseType, float *buf, const nz_stripe *st, float hurst,
                                     float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                                     int32_t xpos, int32_t zpos, int32_t noiseSize, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(nz_check_stripe(st, 0));
    NZ_REQUIRE(buf, "buf is NULL");
    int pitch = st->pitch > 0 ? st->pitch : st->cols;
    int rows = st->own1 - st->own0;
    if (rows > 0) {
        NZ_TRY(fractal_impl(ctx, ctx->stream, noiseType, buf + (size_t)st->own0 * pitch, rows, st->cols, pitch, hurst,
                            startingAmplitude, stepdown, detuneRate, octaves, xpos, zpos + st->grow0 + st->own0,
                            noiseSize));
    }
    return nz_ctx_finish(ctx, out);
}

static int32_t check_shape(int32_t shape) {
    NZ_REQUIRE(shape >= NZ_SHAPE_FBM && shape <= NZ_SHAPE_RIDGED, "unknown octave shape %d", shape);
    return NZ_OK;
}

// nz_fractal / nz_fractal_stripe with an octave shape (new-framework feature, enum nz_fractal_shape)
extern "C" int32_t nz_fractal_shaped(nz_ctx *ctx, int32_t noiseType, float *src, int32_t resolution, float hurst,
                                     float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                                     int32_t xpos, int32_t zpos, int32_t noiseSize, int32_t shape, float ridgeOffset,
                                     float ridgeGain, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_TRY(check_shape(shape));
    nz_ctx_handle_rides(ctx, out != nullptr);
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(fractal_impl(ctx, ctx->stream, noiseType, src, resolution, resolution, resolution, hurst, startingAmplitude,
                        stepdown, detuneRate, octaves, xpos, zpos, noiseSize, 1, 0, nullptr, shape, ridgeOffset,
                        ridgeGain));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_fractal_shaped_stripe(nz_ctx *ctx, int32_t noiseType, float *buf, const nz_stripe *st, float hurst,
                                            float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                                            int32_t xpos, int32_t zpos, int32_t noiseSize, int32_t shape,
                                            float ridgeOffset, float ridgeGain, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(nz_check_stripe(st, 0));
    NZ_REQUIRE(buf, "buf is NULL");
    NZ_TRY(check_shape(shape));
    int pitch = st->pitch > 0 ? st->pitch : st->cols;
    int rows = st->own1 - st->own0;
    if (rows > 0) {
        NZ_TRY(fractal_impl(ctx, ctx->stream, noiseType, buf + (size_t)st->own0 * pitch, rows, st->cols, pitch, hurst,
                            startingAmplitude, stepdown, detuneRate, octaves, xpos, zpos + st->grow0 + st->own0,
                            noiseSize, 1, 0, nullptr, shape, ridgeOffset, ridgeGain));
    }
    return nz_ctx_finish(ctx, out);
}

// nz_fractal_shaped / _stripe read at domain-warped coordinates (new-framework feature, include/noize_hip.h).  The
// warp's arguments are checked here; no warp (strength 0 or no octaves) is the shaped path itself
static int32_t check_warp(float warpStrength, float warpScale, int32_t warpOctaves, nz_warp_params *wp) {
    NZ_REQUIRE(warpOctaves >= 0, "warpOctaves %d < 0", warpOctaves);
    NZ_REQUIRE(std::isfinite(warpStrength), "warpStrength is not finite");
    NZ_REQUIRE(std::isfinite(warpScale), "warpScale is not finite");
    wp->strength = warpStrength;
    wp->scale = warpScale;
    wp->octaves = warpOctaves;
    return NZ_OK;
}
static bool warps(const nz_warp_params &wp) { return wp.strength != 0.0f && wp.octaves > 0; }

extern "C" int32_t nz_fractal_warped(nz_ctx *ctx, int32_t noiseType, float *src, int32_t resolution, float hurst,
                                     float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                                     int32_t xpos, int32_t zpos, int32_t noiseSize, int32_t shape, float ridgeOffset,
                                     float ridgeGain, float warpStrength, float warpScale, int32_t warpOctaves,
                                     nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_TRY(check_shape(shape));
    nz_warp_params wp;
    NZ_TRY(check_warp(warpStrength, warpScale, warpOctaves, &wp));
    nz_ctx_handle_rides(ctx, out != nullptr);
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(fractal_impl(ctx, ctx->stream, noiseType, src, resolution, resolution, resolution, hurst, startingAmplitude,
                        stepdown, detuneRate, octaves, xpos, zpos, noiseSize, 1, 0, nullptr, shape, ridgeOffset,
                        ridgeGain, warps(wp) ? &wp : nullptr));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_fractal_warped_stripe(nz_ctx *ctx, int32_t noiseType, float *buf, const nz_stripe *st, float hurst,
                                            float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                                            int32_t xpos, int32_t zpos, int32_t noiseSize, int32_t shape,
                                            float ridgeOffset, float ridgeGain, float warpStrength, float warpScale,
                                            int32_t warpOctaves, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(nz_check_stripe(st, 0));
    NZ_REQUIRE(buf, "buf is NULL");
    NZ_TRY(check_shape(shape));
    nz_warp_params wp;
    NZ_TRY(check_warp(warpStrength, warpScale, warpOctaves, &wp));
    int pitch = st->pitch > 0 ? st->pitch : st->cols;
    int rows = st->own1 - st->own0;
    if (rows > 0) {
        NZ_TRY(fractal_impl(ctx, ctx->stream, noiseType, buf + (size_t)st->own0 * pitch, rows, st->cols, pitch, hurst,
                            startingAmplitude, stepdown, detuneRate, octaves, xpos, zpos + st->grow0 + st->own0,
                            noiseSize, 1, 0, nullptr, shape, ridgeOffset, ridgeGain, warps(wp) ? &wp : nullptr));
    }
    return nz_ctx_finish(ctx, out);
}

// ---------------------------------------------------------------------------------------------
// separable filters
// ---------------------------------------------------------------------------------------------
// the in-place and batched bodies of the filter and blur stages, once their taps are resolved
static int32_t conv_stage(nz_ctx *ctx, float *src, float *tmp, const nz_geom &g, const nz_kernel_taps &t, int32_t iterations,
                          nz_handle *out) {
    nz_ctx_handle_rides(ctx, out != nullptr);  // (conv_iterations arms the operation that ends it)
    NZ_TRY(conv_iterations(ctx, src, tmp, g, t, iterations));
    return nz_ctx_finish(ctx, out);
}

// SeparableKernelFilter.ScheduleReduce<RootSumSquaresTiles> (KernelJob.cs:187-215) for Sobel3_2D: the horizontal
// filter on src, the vertical filter on a copy of the ORIGINAL plane, then src = sqrt(src^2 + copy^2); both with
// kernelFactor 1.  (The reference takes its copy on the host at schedule time, i.e. before `dependency` has run --
// the README lists the filter as broken; here the copy is ordered after `dep` like every other job.)
static int32_t edge_2d(nz_ctx *ctx, float *src, float *tmp, int resolution, int iterations, int filterH, int filterV) {
    NZ_REQUIRE(src && tmp && src != tmp, "src/tmp must be two distinct planes");
    NZ_REQUIRE(iterations >= 1, "iterations < 1");
    size_t n = (size_t)resolution * resolution;
    float *original = nullptr;
    NZ_TRY(nz_ctx_scratch(ctx, n, &original));
    nz_kernel_taps th, tv;
    NZ_TRY(filter_taps(filterH, &th));
    NZ_TRY(filter_taps(filterV, &tv));
    th.factor = tv.factor = 1.0f;
    nz_geom g = nz_geom_tile(resolution);
    for (int i = 0; i < iterations; i++) {
        NZ_TRY(nz_launch_copy(ctx->stream, original, src, n));
        NZ_TRY(conv_iterations(ctx, src, tmp, g, th, 1));
        NZ_TRY(conv_iterations(ctx, original, tmp, g, tv, 1));
        NZ_TRY(nz_launch_reduce(ctx->stream, 2 /* ROOTSUMSQUARES */, src, original, n));
    }
    return NZ_OK;
}

extern "C" int32_t nz_kernel_filter_stage(nz_ctx *ctx, float *src, float *tmp, int32_t filter, int32_t iterations,
                                          int32_t resolution, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    if (filter == NZ_SOBEL3_2D) {
        NZ_TRY(edge_2d(ctx, src, tmp, resolution, iterations, NZ_SOBEL3_HORIZONTAL, NZ_SOBEL3_VERTICAL));
        return nz_ctx_finish(ctx, out);
    }
    nz_kernel_taps t;
    NZ_TRY(filter_taps(filter, &t));
    return conv_stage(ctx, src, tmp, nz_geom_tile(resolution), t, iterations, out);
}

// Edge1DFilter.Schedule / Edge2DFilter.Schedule, Filter/Kernel/Edge/EdgeJob.cs:11-44 (kernels: EdgeDetection.cs:23-84,
// the same numbers as the Sobel / Prewitt entries of KernelFilterType), kernelFactor 1
extern "C" int32_t nz_edge_1d_filter(nz_ctx *ctx, float *src, float *tmp, int32_t algo, int32_t dir, int32_t resolution,
                                     nz_handle dep, nz_handle *out) {
    NZ_REQUIRE((algo == 0 || algo == 1) && (dir == 0 || dir == 1), "EdgeAlgorithm %d / EdgeDirection %d out of range",
               algo, dir);
    int filter = algo == 0 ? (dir == 0 ? NZ_SOBEL3_HORIZONTAL : NZ_SOBEL3_VERTICAL)
                           : (dir == 0 ? NZ_PREWITT3_HORIZONTAL : NZ_PREWITT3_VERTICAL);
    return nz_kernel_filter_stage(ctx, src, tmp, filter, 1, resolution, dep, out);
}

extern "C" int32_t nz_edge_2d_filter(nz_ctx *ctx, float *src, float *tmp, int32_t algo, int32_t resolution,
                                     nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(algo == 0 || algo == 1, "EdgeAlgorithm %d out of range", algo);
    NZ_TRY(edge_2d(ctx, src, tmp, resolution, 1, algo == 0 ? NZ_SOBEL3_HORIZONTAL : NZ_PREWITT3_HORIZONTAL,
                   algo == 0 ? NZ_SOBEL3_VERTICAL : NZ_PREWITT3_VERTICAL));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_kernel_filter(nz_ctx *ctx, float *src, float *tmp, int32_t filter, int32_t resolution,
                                    nz_handle dep, nz_handle *out) {
    return nz_kernel_filter_stage(ctx, src, tmp, filter, 1, resolution, dep, out);
}

extern "C" int32_t nz_gauss_blur_stage(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t sigma,
                                       int32_t iterations, int32_t resolution, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    nz_kernel_taps t;
    NZ_TRY(gauss_taps(width, sigma, &t));
    return conv_stage(ctx, src, tmp, nz_geom_tile(resolution), t, iterations, out);
}

extern "C" int32_t nz_gauss_filter(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t sigma,
                                   int32_t resolution, nz_handle dep, nz_handle *out) {
    return nz_gauss_blur_stage(ctx, src, tmp, width, sigma, 1, resolution, dep, out);
}

extern "C" int32_t nz_smooth_blur_stage(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t iterations,
                                        int32_t resolution, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    nz_kernel_taps t;
    NZ_TRY(smooth_taps(width, &t));
    return conv_stage(ctx, src, tmp, nz_geom_tile(resolution), t, iterations, out);
}

extern "C" int32_t nz_smooth_filter(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t resolution,
                                    nz_handle dep, nz_handle *out) {
    return nz_smooth_blur_stage(ctx, src, tmp, width, 1, resolution, dep, out);
}

extern "C" int32_t nz_separable_series(nz_ctx *ctx, float *src, float *tmp, int32_t resolution, int32_t kernelSize,
                                       const float *kernelX, const float *kernelZ, float kernelFactor,
                                       nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(kernelX && kernelZ, "kernel body is NULL");
    NZ_REQUIRE(kernelSize >= 1 && kernelSize <= NZ_MAX_KSIZE, "kernelSize %d out of range [1,25]", kernelSize);
    nz_kernel_taps t;
    memset(&t, 0, sizeof t);
    int used = 2 * ((kernelSize - 1) / 2) + 1;  // taps an odd or even kernelSize actually touches
    memcpy(t.kx, kernelX, used * sizeof(float));
    memcpy(t.kz, kernelZ, used * sizeof(float));
    t.factor = kernelFactor;
    t.ksize = kernelSize;
    NZ_TRY(conv_iterations(ctx, src, tmp, nz_geom_tile(resolution), t, 1));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_erosion_stage(nz_ctx *ctx, float *src, float *tmp, int32_t iterations, int32_t resolution,
                                    nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    nz_ctx_handle_rides(ctx, out != nullptr);  // (as conv_iterations)
    NZ_TRY(erosion_iterations(ctx, src, tmp, nz_geom_tile(resolution), iterations));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_erosion_kernel(nz_ctx *ctx, float *src, int32_t resolution, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    // the reference allocates its own TempJob plane (KernelJob.cs:327); here it is ctx scratch
    float *tmp = nullptr;
    NZ_TRY(nz_ctx_scratch(ctx, (size_t)resolution * resolution, &tmp));
    nz_ctx_handle_rides(ctx, out != nullptr);
    NZ_TRY(erosion_iterations(ctx, src, tmp, nz_geom_tile(resolution), 1));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_erosion_max_fused_iterations(void) { return nz_erosion_max_fused(); }

extern "C" int32_t nz_kernel_filter_max_fused(int32_t filter) {
    nz_kernel_taps t;
    if (filter_taps(filter, &t) != NZ_OK) return 0;
    int cap = conv_tcap(t.ksize);
    return cap < 1 ? 1 : cap;
}

extern "C" int32_t nz_kernel_filter_halo_rows(int32_t filter, int32_t iterations) {
    nz_kernel_taps t;
    if (filter_taps(filter, &t) != NZ_OK) return -1;
    return iterations * ((t.ksize - 1) / 2);
}

extern "C" int32_t nz_kernel_filter_stripe(nz_ctx *ctx, const float *src, float *dst, const nz_stripe *st,
                                           int32_t filter, int32_t iterations, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    nz_kernel_taps t;
    NZ_TRY(filter_taps(filter, &t));
    NZ_REQUIRE(src && dst && src != dst, "src/dst must be two distinct planes");
    NZ_REQUIRE(iterations >= 1 && iterations <= nz_conv_max_fused(t.ksize), "iterations %d cannot be fused",
               iterations);
    NZ_TRY(nz_check_stripe(st, iterations * ((t.ksize - 1) / 2)));
    NZ_TRY(nz_launch_conv_fused(ctx->stream, src, dst, nz_geom_from_stripe(*st), t, iterations));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_erosion_stripe(nz_ctx *ctx, const float *src, float *dst, const nz_stripe *st,
                                     int32_t iterations, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(src && dst && src != dst, "src/dst must be two distinct planes");
    NZ_REQUIRE(iterations >= 1 && iterations <= nz_erosion_max_fused(), "iterations %d cannot be fused", iterations);
    NZ_TRY(nz_check_stripe(st, iterations, 0));  // the min window reaches upwards only
    NZ_TRY(nz_launch_erosion_fused(ctx->stream, src, dst, nz_geom_from_stripe(*st), iterations));
    return nz_ctx_finish(ctx, out);
}

// ---------------------------------------------------------------------------------------------
// flow map
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nz_flush_write_slice(nz_ctx *ctx, float *write_, const float *read_, size_t n_floats, nz_handle dep,
                                        nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(write_ && read_, "write/read is NULL");
    NZ_REQUIRE(write_ != read_, "write and read are the same slice");
    nz_ctx_handle_rides(ctx, out != nullptr);
    nz_ctx_arm_last_launch(ctx);
    if (n_floats) NZ_TRY(nz_launch_copy(ctx->stream, write_, read_, n_floats));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_fill_array(nz_ctx *ctx, float *data, int32_t resolution, float value, nz_handle dep,
                                 nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(data, "data is NULL");
    nz_ctx_handle_rides(ctx, out != nullptr);
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_fill(ctx->stream, data, (size_t)resolution * resolution, value));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_flowmap_compute_flow(nz_ctx *ctx, const float *src, const float *waterMap, float *flowMapN,
                                           float *flowMapN__buff, float *flowMapS, float *flowMapS__buff,
                                           float *flowMapE, float *flowMapE__buff, float *flowMapW,
                                           float *flowMapW__buff, int32_t resolution, nz_handle dep,
                                           nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(src && waterMap && flowMapN && flowMapS && flowMapE && flowMapW, "plane is NULL");
    // The reference writes the __buff planes and flushes them back (FlowMapJob.cs:70-77).  Each
    // cell reads only its own flux, so the update is done in place and the buffers stay untouched.
    (void)flowMapN__buff; (void)flowMapS__buff; (void)flowMapE__buff; (void)flowMapW__buff;
    NZ_TRY(nz_launch_flow_step(ctx->stream, src, waterMap, flowMapN, flowMapS, flowMapE, flowMapW, flowMapN, flowMapS,
                               flowMapE, flowMapW, nz_geom_tile(resolution)));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_flowmap_update_water(nz_ctx *ctx, float *waterMap, float *waterMap__buff,
                                           const float *flowMapN, const float *flowMapS, const float *flowMapE,
                                           const float *flowMapW, int32_t resolution, nz_handle dep,
                                           nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(waterMap && flowMapN && flowMapS && flowMapE && flowMapW, "plane is NULL");
    (void)waterMap__buff;
    NZ_TRY(nz_launch_water_step(ctx->stream, waterMap, waterMap, flowMapN, flowMapS, flowMapE, flowMapW,
                                nz_geom_tile(resolution)));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_flowmap_write_values(nz_ctx *ctx, float *src, const float *flowMapN, const float *flowMapS,
                                           const float *flowMapE, const float *flowMapW, int32_t resolution,
                                           nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(src && flowMapN && flowMapS && flowMapE && flowMapW, "plane is NULL");
    NZ_TRY(nz_launch_velocity(ctx->stream, src, flowMapN, flowMapS, flowMapE, flowMapW, nz_geom_tile(resolution), 0,
                              0.0f, 1.0f));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_map_normalize_values(nz_ctx *ctx, float *src, float *tmp, const float *args,
                                           int32_t resolution, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(src && args, "src/args is NULL");
    (void)tmp;  // element-wise: done in place, no flush copy
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_normalize(ctx->stream, src, src, (size_t)resolution * resolution, args[0], args[2]));
    return nz_ctx_finish(ctx, out);
}

// GetMapRangeJob.Schedule, Filter/NormalizeJob.cs:45-53: res = DEVICE {min, max, max - min}
extern "C" int32_t nz_get_map_range(nz_ctx *ctx, const float *map, size_t n_floats, float *res, float lim_min, float lim_max,
                                    nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(map && res, "map/res is NULL");
    NZ_REQUIRE(n_floats >= 1, "empty map");
    float *scratch = nullptr;
    NZ_TRY(nz_ctx_scratch(ctx, nz_map_range_scratch_floats(), &scratch));
    NZ_TRY(nz_launch_map_range(ctx->stream, map, n_floats, lim_min, lim_max, res, scratch));
    return nz_ctx_finish(ctx, out);
}

// MapNormalizeValuesDelegate with `args` left in device memory by nz_get_map_range (the reference's NativeSlice<float> args)
extern "C" int32_t nz_map_normalize_values_dev(nz_ctx *ctx, float *src, float *tmp, const float *args, int32_t resolution,
                                               nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(src && args, "src/args is NULL");
    (void)tmp;  // element-wise: done in place, no flush copy
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_normalize_args(ctx->stream, src, (size_t)resolution * resolution, args));
    return nz_ctx_finish(ctx, out);
}

// The same on any contiguous run of cells (a stripe's owned rows)
extern "C" int32_t nz_normalize_cells_dev(nz_ctx *ctx, float *data, size_t n_floats, const float *args, nz_handle dep,
                                          nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(data && args, "data/args is NULL");
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_normalize_args(ctx->stream, data, n_floats, args));
    return nz_ctx_finish(ctx, out);
}

extern "C" size_t nz_flowmap_stage_work_floats(int32_t resolution) {
    return resolution > 0 ? (size_t)11 * resolution * resolution : 0;  // the reference stage's 11 planes
}

// FlowMapStage (FlowMapStage.cs:52-194) on `g`: `iterations` split into launches of <= nz_flow_fused_max() iterations that
// keep the tile on chip, the state {water, fN, fS, fE, fW} ping-ponging between the READ and WRITE planes of `work`
// (FlowMapStage.cs:52-62, plane p of a batch = work + p * count * res^2).  The first launch implies water == 0.0001
// (fillStage, FlowMapStage.cs:129) and flux == 0 (defined); the last one ends in writeStage + normStage
// (FlowMapStage.cs:179-194), args = {normMin, normMax, normMax - normMin} (:48-51), and writes `dst`.
// hcopy == nullptr: every launch reads the heights from `h`, which nothing overwrites.  Otherwise the result overwrites
// the height plane (dst == h), which the last launch still reads with a halo: the first launch keeps a private copy of it
// in `hcopy` for the later ones, and a single launch writes `hcopy`, copied back to `dst` behind it.
static int32_t flow_series(nz_ctx *ctx, const nz_geom &g, float *work, int32_t iterations, float normMin, float normMax,
                           const float *h, float *dst, float *hcopy) {
    const size_t n = (size_t)g.cols * g.rows * g.count;
    float *A[5], *B[5];
    for (int i = 0; i < 5; i++) {
        A[i] = work + (size_t)i * n;
        B[i] = work + (size_t)(5 + i) * n;
    }
    const std::vector<int> its = nz_split_iterations(iterations, nz_flow_fused_max());
    const int L = (int)its.size();
    const bool copy = hcopy && L == 1;
    float **cur = A, **nxt = B;
    for (int i = 0; i < L; i++) {
        const int first = i == 0, last = i == L - 1;
        if (last && !copy) nz_ctx_arm_last_launch(ctx);
        NZ_TRY(nz_launch_flow_fused(ctx->stream, first || !hcopy ? h : hcopy, first ? nullptr : cur, last ? nullptr : nxt,
                                    !last ? nullptr : (copy ? hcopy : dst), first && !last ? hcopy : nullptr, g, its[i],
                                    first, last, normMin, normMax - normMin));
        std::swap(cur, nxt);
    }
    return copy ? copy_back(ctx, g, dst, hcopy) : NZ_OK;
}

static int32_t flowmap_stage_impl(nz_ctx *ctx, float *src, float *work, int32_t iterations, float normMin,
                                  float normMax, int32_t resolution, int32_t count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(src && work, "src/work is NULL");
    NZ_REQUIRE(iterations >= 1, "iterations < 1");
    NZ_REQUIRE(count >= 1 && count <= 65535, "count %d out of range [1,65535]", count);
    nz_geom g = count > 1 ? nz_geom_batch(resolution, count) : nz_geom_tile(resolution);
    float *hcopy = work + (size_t)10 * resolution * resolution * count;  // the stage's 11th plane
    nz_ctx_handle_rides(ctx, out != nullptr);  // (flow_series arms the operation that ends it)
    NZ_TRY(flow_series(ctx, g, work, iterations, normMin, normMax, src, src, hcopy));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_flowmap_stage(nz_ctx *ctx, float *src, float *work, int32_t iterations, float normMin,
                                    float normMax, int32_t resolution, nz_handle dep, nz_handle *out) {
    return flowmap_stage_impl(ctx, src, work, iterations, normMin, normMax, resolution, 1, dep, out);
}

extern "C" int32_t nz_flow_fused_max_iterations(void) { return nz_flow_fused_max(); }

// ---------------------------------------------------------------------------------------------
// batched stage bodies: `count` independent tiles of resolution^2 cells stored back to back, one launch
// sequence for all of them (new-framework feature: the reference runs one BasePipeline per tile request,
// Scripts/MeshTileGenerator.cs:181-211; small tiles cannot fill 256 CUs one at a time)
// ---------------------------------------------------------------------------------------------
static int32_t check_batch(int32_t resolution, int32_t count) {
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(count >= 1 && count <= 65535, "count %d out of range [1,65535]", count);
    return NZ_OK;
}

extern "C" int32_t nz_fractal_batch(nz_ctx *ctx, int32_t noiseType, float *data, int32_t resolution, int32_t count,
                                    const int32_t *positions, float hurst, float startingAmplitude, float stepdown,
                                    float detuneRate, int32_t octaves, int32_t noiseSize, nz_handle dep,
                                    nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    NZ_REQUIRE(positions, "positions is NULL");
    nz_ctx_handle_rides(ctx, out != nullptr);
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(fractal_impl(ctx, ctx->stream, noiseType, data, resolution, resolution, resolution, hurst, startingAmplitude,
                        stepdown, detuneRate, octaves, 0, 0, noiseSize, count, (size_t)resolution * resolution, positions));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_fractal_shaped_batch(nz_ctx *ctx, int32_t noiseType, float *data, int32_t resolution,
                                           int32_t count, const int32_t *positions, float hurst, float startingAmplitude,
                                           float stepdown, float detuneRate, int32_t octaves, int32_t noiseSize,
                                           int32_t shape, float ridgeOffset, float ridgeGain, nz_handle dep,
                                           nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    NZ_REQUIRE(positions, "positions is NULL");
    NZ_TRY(check_shape(shape));
    nz_ctx_handle_rides(ctx, out != nullptr);
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(fractal_impl(ctx, ctx->stream, noiseType, data, resolution, resolution, resolution, hurst, startingAmplitude,
                        stepdown, detuneRate, octaves, 0, 0, noiseSize, count, (size_t)resolution * resolution, positions,
                        shape, ridgeOffset, ridgeGain));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_fractal_warped_batch(nz_ctx *ctx, int32_t noiseType, float *data, int32_t resolution,
                                           int32_t count, const int32_t *positions, float hurst, float startingAmplitude,
                                           float stepdown, float detuneRate, int32_t octaves, int32_t noiseSize,
                                           int32_t shape, float ridgeOffset, float ridgeGain, float warpStrength,
                                           float warpScale, int32_t warpOctaves, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    NZ_REQUIRE(positions, "positions is NULL");
    NZ_TRY(check_shape(shape));
    nz_warp_params wp;
    NZ_TRY(check_warp(warpStrength, warpScale, warpOctaves, &wp));
    nz_ctx_handle_rides(ctx, out != nullptr);
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(fractal_impl(ctx, ctx->stream, noiseType, data, resolution, resolution, resolution, hurst, startingAmplitude,
                        stepdown, detuneRate, octaves, 0, 0, noiseSize, count, (size_t)resolution * resolution, positions,
                        shape, ridgeOffset, ridgeGain, warps(wp) ? &wp : nullptr));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_kernel_filter_stage_batch(nz_ctx *ctx, float *src, float *tmp, int32_t filter, int32_t iterations,
                                                int32_t resolution, int32_t count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    nz_kernel_taps t;
    NZ_TRY(filter_taps(filter, &t));
    return conv_stage(ctx, src, tmp, nz_geom_batch(resolution, count), t, iterations, out);
}

extern "C" int32_t nz_gauss_blur_stage_batch(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t sigma,
                                             int32_t iterations, int32_t resolution, int32_t count, nz_handle dep,
                                             nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    nz_kernel_taps t;
    NZ_TRY(gauss_taps(width, sigma, &t));
    return conv_stage(ctx, src, tmp, nz_geom_batch(resolution, count), t, iterations, out);
}

extern "C" int32_t nz_smooth_blur_stage_batch(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t iterations,
                                              int32_t resolution, int32_t count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    nz_kernel_taps t;
    NZ_TRY(smooth_taps(width, &t));
    return conv_stage(ctx, src, tmp, nz_geom_batch(resolution, count), t, iterations, out);
}

extern "C" int32_t nz_erosion_stage_batch(nz_ctx *ctx, float *src, float *tmp, int32_t iterations, int32_t resolution,
                                          int32_t count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    nz_ctx_handle_rides(ctx, out != nullptr);  // (as conv_iterations)
    NZ_TRY(erosion_iterations(ctx, src, tmp, nz_geom_batch(resolution, count), iterations));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_flowmap_stage_batch(nz_ctx *ctx, float *src, float *work, int32_t iterations, float normMin,
                                          float normMax, int32_t resolution, int32_t count, nz_handle dep,
                                          nz_handle *out) {
    return flowmap_stage_impl(ctx, src, work, iterations, normMin, normMax, resolution, count, dep, out);
}

// ---------------------------------------------------------------------------------------------
// READ / WRITE pair forms (nz_rw_tile): TileHelpers.SWAP_RWTILE (Pipeline/Tiles/TileData.cs:42-45) as a swap of the
// two pointers instead of a copy job
// ---------------------------------------------------------------------------------------------
static int32_t check_rw(const nz_rw_tile *t) {
    NZ_REQUIRE(t, "tile is NULL");
    NZ_TRY(check_batch(t->resolution, t->count));
    NZ_REQUIRE(t->read && t->write && t->read != t->write, "read/write must be two distinct planes");
    return NZ_OK;
}
static nz_geom rw_geom(const nz_rw_tile *t) {
    return t->count > 1 ? nz_geom_batch(t->resolution, t->count) : nz_geom_tile(t->resolution);
}
static void rw_swap(nz_rw_tile *t, bool swapped) {
    if (swapped) {
        float *r = t->read;
        t->read = t->write;
        t->write = r;
    }
}

static int32_t conv_rw(nz_ctx *ctx, nz_rw_tile *tile, const nz_kernel_taps &t, int32_t iterations, nz_handle *out) {
    bool swapped = false;
    nz_ctx_handle_rides(ctx, out != nullptr);  // conv_iterations' last launch is this entry's last operation
    NZ_TRY(conv_iterations(ctx, tile->read, tile->write, rw_geom(tile), t, iterations, &swapped));
    rw_swap(tile, swapped);
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_kernel_filter_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, int32_t filter, int32_t iterations,
                                             nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_rw(tile));
    NZ_REQUIRE(filter != NZ_SOBEL3_2D, "Sobel3_2D keeps a third plane: use nz_kernel_filter_stage");
    nz_kernel_taps t;
    NZ_TRY(filter_taps(filter, &t));
    return conv_rw(ctx, tile, t, iterations, out);
}

extern "C" int32_t nz_gauss_blur_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, int32_t width, int32_t sigma,
                                          int32_t iterations, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_rw(tile));
    nz_kernel_taps t;
    NZ_TRY(gauss_taps(width, sigma, &t));
    return conv_rw(ctx, tile, t, iterations, out);
}

extern "C" int32_t nz_smooth_blur_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, int32_t width, int32_t iterations,
                                           nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_rw(tile));
    nz_kernel_taps t;
    NZ_TRY(smooth_taps(width, &t));
    return conv_rw(ctx, tile, t, iterations, out);
}

extern "C" int32_t nz_erosion_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, int32_t iterations, nz_handle dep,
                                       nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_rw(tile));
    bool swapped = false;
    nz_ctx_handle_rides(ctx, out != nullptr);  // erosion_iterations' last launch is this entry's last operation
    NZ_TRY(erosion_iterations(ctx, tile->read, tile->write, rw_geom(tile), iterations, &swapped));
    rw_swap(tile, swapped);
    return nz_ctx_finish(ctx, out);
}

extern "C" size_t nz_flowmap_stage_rw_work_floats(int32_t resolution, int32_t count) {
    return resolution > 0 && count > 0 ? (size_t)10 * resolution * resolution * count : 0;
}

extern "C" int32_t nz_flowmap_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, int32_t iterations, float normMin,
                                       float normMax, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_rw(tile));
    NZ_REQUIRE(work, "work is NULL");
    NZ_REQUIRE(iterations >= 1, "iterations < 1");
    nz_ctx_handle_rides(ctx, out != nullptr);  // (flow_series arms its last launch)
    NZ_TRY(flow_series(ctx, rw_geom(tile), work, iterations, normMin, normMax, tile->read, tile->write, nullptr));
    rw_swap(tile, true);
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_flow_fused_stripe(nz_ctx *ctx, const float *height, const float *const *state_in,
                                        float *const *state_out, float *dst, const nz_stripe *st, int32_t iterations,
                                        int32_t first, int32_t last, float normMin, float normMax, nz_handle dep,
                                        nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(iterations >= 1 && iterations <= nz_flow_fused_max(), "iterations %d cannot be fused", iterations);
    NZ_TRY(nz_check_stripe(st, 2 * iterations));
    NZ_REQUIRE(height, "height is NULL");
    NZ_REQUIRE(first || state_in, "state_in is NULL");
    NZ_REQUIRE(!last || dst, "dst is NULL");
    NZ_REQUIRE(last || state_out, "state_out is NULL");
    for (int i = 0; i < 5; i++) {
        NZ_REQUIRE(first || state_in[i], "state_in[%d] is NULL", i);
        NZ_REQUIRE(last || state_out[i], "state_out[%d] is NULL", i);
    }
    NZ_REQUIRE(!last || dst != height, "dst must not alias height");
    NZ_TRY(nz_launch_flow_fused(ctx->stream, height, first ? nullptr : state_in, last ? nullptr : state_out,
                                last ? dst : nullptr, nullptr, nz_geom_from_stripe(*st), iterations, first, last, normMin,
                                normMax - normMin));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_flow_launch_form(nz_ctx *ctx, int32_t cols, int32_t rows, int32_t count, int32_t iterations,
                                       int32_t first, int32_t last) {
    NZ_REQUIRE(ctx, "ctx is NULL");
    // (the rule's CU count, nz_cu_count, is taken once per process from the device current at its first use: the launcher
    // and this query share it)
    NZ_HIP(hipSetDevice(ctx->device));
    NZ_REQUIRE(cols >= 1 && rows >= 1 && count >= 1, "flow_launch_form: cols %d, rows %d, count %d", cols, rows, count);
    NZ_REQUIRE(iterations >= 1 && iterations <= nz_flow_fused_max(), "iterations %d cannot be fused", iterations);
    nz_geom g{cols, cols, rows, 0, rows - 1, 0, rows};
    g.count = count;
    g.bstride = (size_t)cols * rows;
    return nz_flow_form(g, iterations, first, last);
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

static int32_t check_hydraulic(int32_t iterations, float initialWater, float rain, float evaporation, float capacity,
                               float dissolve, float deposit, float minTilt, nz_hydraulic_params *k) {
    NZ_REQUIRE(iterations >= 0, "iterations %d < 0", iterations);
    const struct { const char *name; float v; float lo, hi; } args[] = {
        {"initialWater", initialWater, 0.0f, INFINITY}, {"rain", rain, 0.0f, INFINITY},
        {"evaporation", evaporation, 0.0f, 1.0f},       {"capacity", capacity, 0.0f, INFINITY},
        {"dissolve", dissolve, 0.0f, 1.0f},             {"deposit", deposit, 0.0f, 1.0f},
        {"minTilt", minTilt, 0.0f, INFINITY}};
    for (const auto &a : args) {
        NZ_REQUIRE(std::isfinite(a.v), "%s is not finite", a.name);
        if (a.hi == INFINITY) NZ_REQUIRE(a.v >= a.lo, "%s %g < 0", a.name, (double)a.v);
        else NZ_REQUIRE(a.v >= a.lo && a.v <= a.hi, "%s %g outside [0, 1]", a.name, (double)a.v);
    }
    *k = nz_hydraulic_params{initialWater, rain, 1.0f - evaporation, capacity, dissolve, deposit, minTilt};
    return NZ_OK;
}

// the options of a nz_hydraulic_desc as the launches take them.  h0 / h1: the height plane(s) the call reads or writes
// (h1 may be NULL), n floats each like every plane of the desc; the masks may overlap none of them, nor the maps, each
// other or `work`
static int32_t check_hydraulic_planes(const nz_hydraulic_desc &d, const float *h0, const float *h1, const float *work,
                                      size_t n, nz_hydraulic_ex *ex) {
    NZ_REQUIRE(d.border == NZ_HYDRAULIC_BORDER_CLOSED || d.border == NZ_HYDRAULIC_BORDER_OPEN, "border %d is not a mode",
               d.border);
    auto overlap = [](const float *a, size_t na, const float *b, size_t nb) {
        return a && b && (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
    };
    const struct { const char *name; const float *p; } masks[] = {{"wear", d.wear}, {"deposits", d.deposits}};
    for (const auto &m : masks) {
        const struct { const char *name; const float *p; size_t n; } others[] = {
            {"src", h0, n}, {"the write plane", h1, n}, {"work", work, (size_t)HYD_PLANES * n},
            {"rainMap", d.rainMap, n}, {"hardness", d.hardness, n}};
        for (const auto &o : others) NZ_REQUIRE(!overlap(m.p, n, o.p, o.n), "%s overlaps %s", m.name, o.name);
    }
    NZ_REQUIRE(!overlap(d.wear, n, d.deposits, n), "wear overlaps deposits");
    *ex = nz_hydraulic_ex{d.border == NZ_HYDRAULIC_BORDER_OPEN, d.rainMap, d.hardness, d.wear, d.deposits};
    return NZ_OK;
}

// `iterations` launches on `count` tiles; the height ping-pongs between h0 (which holds the input) and h1, the state
// between the two sets of `work`.  The result lands in h0 when `iterations` is even and in h1 when it is odd (*in_h1);
// keep_h0: the caller wants it in h0 whatever the count, and an odd count copies h0 to h1 first.  Ends with the final
// water in work plane 0 (initialWater itself when there is no iteration).  ex: the _ex options (all off: the default
// kernels); its masks are written by the first launch, or cleared here when there is none.
static int32_t hydraulic_series(nz_ctx *ctx, float *h0, float *h1, float *work, int res, int count, int32_t iterations,
                                const nz_hydraulic_params &k, const nz_hydraulic_ex &ex, bool keep_h0, bool *in_h1) {
    const size_t n = (size_t)res * res * count;
    *in_h1 = false;
    if (iterations == 0) {
        if (ex.wear) NZ_TRY(nz_launch_fill(ctx->stream, ex.wear, n, 0.0f));
        if (ex.deposits) NZ_TRY(nz_launch_fill(ctx->stream, ex.deposits, n, 0.0f));
        nz_ctx_arm_last_launch(ctx);
        return nz_launch_fill(ctx->stream, work, n, k.initial_water);
    }
    float *cur = h0, *nxt = h1;
    if (keep_h0 && (iterations & 1)) {
        NZ_TRY(nz_launch_copy(ctx->stream, h1, h0, n));
        std::swap(cur, nxt);
    }
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
    *in_h1 = cur == h1;
    return NZ_OK;
}

// every in-place entry: the old ones come with a desc of their scalars and every option off
static int32_t hydraulic_stage_impl(nz_ctx *ctx, float *src, float *work, const nz_hydraulic_desc *desc, int32_t resolution,
                                    int32_t count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    NZ_REQUIRE(src && work, "src/work is NULL");
    NZ_REQUIRE(desc, "desc is NULL");
    nz_hydraulic_params k;
    NZ_TRY(check_hydraulic(desc->iterations, desc->initialWater, desc->rain, desc->evaporation, desc->capacity, desc->dissolve,
                           desc->deposit, desc->minTilt, &k));
    nz_hydraulic_ex ex;
    NZ_TRY(check_hydraulic_planes(*desc, src, nullptr, work, (size_t)resolution * resolution * count, &ex));
    float *h1 = work + (size_t)(HYD_PLANES - 1) * resolution * resolution * count;
    bool in_h1;
    nz_ctx_handle_rides(ctx, out != nullptr);  // (hydraulic_series arms its last launch)
    NZ_TRY(hydraulic_series(ctx, src, h1, work, resolution, count, desc->iterations, k, ex, true, &in_h1));
    return nz_ctx_finish(ctx, out);
}

static int32_t hydraulic_rw_impl(nz_ctx *ctx, nz_rw_tile *tile, float *work, const nz_hydraulic_desc *desc, nz_handle dep,
                                 nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_rw(tile));
    NZ_REQUIRE(work, "work is NULL");
    NZ_REQUIRE(desc, "desc is NULL");
    nz_hydraulic_params k;
    NZ_TRY(check_hydraulic(desc->iterations, desc->initialWater, desc->rain, desc->evaporation, desc->capacity, desc->dissolve,
                           desc->deposit, desc->minTilt, &k));
    nz_hydraulic_ex ex;
    NZ_TRY(check_hydraulic_planes(*desc, tile->read, tile->write, work,
                                  (size_t)tile->resolution * tile->resolution * tile->count, &ex));
    bool in_h1;
    nz_ctx_handle_rides(ctx, out != nullptr);  // (hydraulic_series arms its last launch)
    NZ_TRY(hydraulic_series(ctx, tile->read, tile->write, work, tile->resolution, tile->count, desc->iterations, k, ex, false,
                            &in_h1));
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

static size_t stripe_plane_floats(const nz_stripe &st) { return (size_t)st.rows * (st.pitch > 0 ? st.pitch : st.cols); }

extern "C" size_t nz_hydraulic_stripe_work_floats(const nz_stripe *st, int32_t iterations) {
    if (!st || st->rows <= 0 || st->cols <= 0 || st->pitch < 0 || iterations <= 1) return 0;
    return (size_t)HYD_STRIPE_PLANES * stripe_plane_floats(*st);
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
    NZ_TRY(check_hydraulic(n, desc->initialWater, desc->rain, desc->evaporation, desc->capacity, desc->dissolve,
                           desc->deposit, desc->minTilt, &k));
    NZ_REQUIRE(desc->border == NZ_HYDRAULIC_BORDER_CLOSED || desc->border == NZ_HYDRAULIC_BORDER_OPEN,
               "border %d is not a mode", desc->border);
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
    // every plane the call writes lies apart from every other plane of the call; planes that are only read may alias
    const nz_geom g0 = nz_geom_from_stripe(*st);
    const size_t span = (size_t)(st->rows - 1) * g0.pitch + st->cols, plane = stripe_plane_floats(*st);
    struct named { const char *name; const float *p; size_t n; };
    std::vector<named> reads{{"height_in", height_in, span}, {"rainMap", desc->rainMap, span}, {"hardness", desc->hardness, span}};
    std::vector<named> writes{{"height_out", height_out, span}, {"wear", desc->wear, span}, {"deposits", desc->deposits, span}};
    if (n > 1) writes.push_back({"work", work, HYD_STRIPE_PLANES * plane});
    for (int i = 0; i < 6; i++) {
        if (!first) reads.push_back({"state_in", state_in[i], span});
        writes.push_back({"state_out", state_out[i], span});
    }
    auto overlap = [](const named &a, const named &b) {
        return a.p && b.p && (uintptr_t)a.p < (uintptr_t)(b.p + b.n) && (uintptr_t)b.p < (uintptr_t)(a.p + a.n);
    };
    for (size_t i = 0; i < writes.size(); i++) {
        for (const auto &r : reads) NZ_REQUIRE(!overlap(writes[i], r), "%s overlaps %s", writes[i].name, r.name);
        for (size_t j = i + 1; j < writes.size(); j++)
            NZ_REQUIRE(!overlap(writes[i], writes[j]), "%s overlaps %s", writes[i].name, writes[j].name);
    }
    const nz_hydraulic_ex ex{desc->border == NZ_HYDRAULIC_BORDER_OPEN, desc->rainMap, desc->hardness, desc->wear,
                             desc->deposits};
    // launch j writes set (n-1-j) & 1: 0 = the caller's output planes, where the last launch lands; 1 = `work`
    nz_hydraulic_planes sets[2];
    float *hs[2] = {height_out, work};
    for (int i = 0; i < 6; i++) {
        sets[0].in[i] = sets[0].out[i] = state_out[i];
        sets[1].in[i] = sets[1].out[i] = n > 1 ? work + (size_t)(1 + i) * plane : nullptr;
    }
    const int glo = g0.zc0 > -st->grow0 ? g0.zc0 : -st->grow0, ghi = st->grows - st->grow0;  // the global grid in buffer rows
    nz_ctx_handle_rides(ctx, out != nullptr);
    for (int j = 0; j < n; j++) {
        const int to = (n - 1 - j) & 1, widen = HYD_STRIPE_RADIUS * (n - 1 - j);
        nz_geom g = g0;
        g.or0 = st->own0 - widen > glo ? st->own0 - widen : glo;
        g.or1 = st->own1 + widen < ghi ? st->own1 + widen : ghi;
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

// the scalars' ranges, and the read-only planes of the desc against the planes the call writes: h0 / h1 the height
// plane(s) (h1 may be NULL), n floats each like every plane of the desc, and `work`
static int32_t check_fluvial(const nz_fluvial_desc *d, const float *h0, const float *h1, const float *work, size_t n,
                             nz_fluvial_params *k) {
    NZ_REQUIRE(d, "desc is NULL");
    NZ_REQUIRE(d->iterations >= 0, "iterations %d < 0", d->iterations);
    const struct { const char *name; float v; bool signed_; } args[] = {
        {"erodibility", d->erodibility, false}, {"uplift", d->uplift, false}, {"dt", d->dt, false},
        {"rain", d->rain, false},               {"seaLevel", d->seaLevel, true}};
    for (const auto &a : args) {
        NZ_REQUIRE(std::isfinite(a.v), "%s is not finite", a.name);
        NZ_REQUIRE(a.signed_ || a.v >= 0.0f, "%s %g < 0", a.name, (double)a.v);
    }
    auto overlap = [](const float *a, size_t na, const float *b, size_t nb) {
        return a && b && (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
    };
    const struct { const char *name; const float *p; } reads[] = {
        {"drainageIn", d->drainageIn}, {"rainMap", d->rainMap}, {"hardness", d->hardness}, {"upliftMap", d->upliftMap}};
    const struct { const char *name; const float *p; size_t n; } writes[] = {
        {"src", h0, n}, {"the write plane", h1, n}, {"work", work, (size_t)FLU_PLANES * n}};
    for (const auto &r : reads)
        for (const auto &w : writes) NZ_REQUIRE(!overlap(r.p, n, w.p, w.n), "%s overlaps %s", r.name, w.name);
    *k = nz_fluvial_params{d->erodibility, d->uplift, d->dt, d->rain, d->seaLevel};
    return NZ_OK;
}

// `iterations` launches on `count` tiles; the height ping-pongs between h0 (which holds the input) and h1 as in
// hydraulic_series (*in_h1, keep_h0), the drainage between work planes 0 and 1: launch `it` writes plane (iterations-1-it)&1,
// so the last one writes plane 0.  The first launch reads drainageIn, or the start state rain * rainMap written here into
// the plane it does not write, or -- without either -- no drainage plane at all.  Without an iteration plane 0 receives
// the start state.
static int32_t fluvial_series(nz_ctx *ctx, float *h0, float *h1, float *work, int res, int count, const nz_fluvial_desc &d,
                              const nz_fluvial_params &k, bool keep_h0, bool *in_h1) {
    const size_t n = (size_t)res * res * count;
    const int iterations = d.iterations;
    float *planes[2] = {work, work + n};
    *in_h1 = false;
    if (iterations == 0) {
        nz_ctx_arm_last_launch(ctx);
        if (d.drainageIn) return nz_launch_copy(ctx->stream, work, d.drainageIn, n);
        if (d.rainMap) return nz_launch_fluvial_start(ctx->stream, work, d.rainMap, k.rain, n);
        return nz_launch_fill(ctx->stream, work, n, k.rain);
    }
    float *cur = h0, *nxt = h1;
    if (keep_h0 && (iterations & 1)) {
        NZ_TRY(nz_launch_copy(ctx->stream, h1, h0, n));
        std::swap(cur, nxt);
    }
    const float *a_in = d.drainageIn;
    if (!a_in && d.rainMap) {
        NZ_TRY(nz_launch_fluvial_start(ctx->stream, planes[iterations & 1], d.rainMap, k.rain, n));
        a_in = planes[iterations & 1];
    }
    for (int it = 0; it < iterations; it++) {
        float *a_out = planes[(iterations - 1 - it) & 1];
        if (it == iterations - 1) nz_ctx_arm_last_launch(ctx);
        NZ_TRY(nz_launch_fluvial(ctx->stream, cur, nxt, a_in, a_out, k, res, count, d.rainMap, d.hardness, d.upliftMap));
        a_in = a_out;
        std::swap(cur, nxt);
    }
    *in_h1 = cur == h1;
    return NZ_OK;
}

static int32_t fluvial_stage_impl(nz_ctx *ctx, float *src, float *work, const nz_fluvial_desc *desc, int32_t resolution,
                                  int32_t count, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_batch(resolution, count));
    NZ_REQUIRE(src && work, "src/work is NULL");
    const size_t n = (size_t)resolution * resolution * count;
    nz_fluvial_params k;
    NZ_TRY(check_fluvial(desc, src, nullptr, work, n, &k));
    bool in_h1;
    nz_ctx_handle_rides(ctx, out != nullptr);  // (fluvial_series arms its last launch)
    NZ_TRY(fluvial_series(ctx, src, work + (size_t)(FLU_PLANES - 1) * n, work, resolution, count, *desc, k, true, &in_h1));
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
    nz_fluvial_params k;
    NZ_TRY(check_fluvial(desc, tile->read, tile->write, work, (size_t)tile->resolution * tile->resolution * tile->count, &k));
    bool in_h1;
    nz_ctx_handle_rides(ctx, out != nullptr);  // (fluvial_series arms its last launch)
    NZ_TRY(fluvial_series(ctx, tile->read, tile->write, work, tile->resolution, tile->count, *desc, k, false, &in_h1));
    rw_swap(tile, in_h1);
    return nz_ctx_finish(ctx, out);
}

// ---- the stripe form (include/noize_hip.h): n iterations of one call on a row stripe, one launch each ----
constexpr int FLU_STRIPE_RADIUS = 2;  // rows one iteration reads beyond the rows it produces: receivers at 1, their heights at 2

extern "C" int32_t nz_fluvial_stripe_halo_rows(int32_t iterations) {
    return iterations > 0 ? FLU_STRIPE_RADIUS * iterations : 0;
}

extern "C" size_t nz_fluvial_stripe_work_floats(const nz_stripe *st, int32_t iterations) {
    if (!st || st->rows <= 0 || st->cols <= 0 || st->pitch < 0 || iterations <= 1) return 0;
    return 2 * stripe_plane_floats(*st);
}

extern "C" int32_t nz_fluvial_stripe(nz_ctx *ctx, const float *height_in, float *height_out, float *drainage_out, float *work,
                                     const nz_stripe *st, const nz_fluvial_desc *desc, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(desc, "desc is NULL");
    const int n = desc->iterations;
    NZ_REQUIRE(n >= 1, "iterations %d < 1", n);
    NZ_REQUIRE(n <= INT32_MAX / FLU_STRIPE_RADIUS, "iterations %d out of range", n);
    nz_fluvial_params k;
    NZ_TRY(check_fluvial(desc, nullptr, nullptr, nullptr, 0, &k));  // the scalars; the planes below
    NZ_TRY(nz_check_stripe(st, FLU_STRIPE_RADIUS * n));
    NZ_REQUIRE(height_in && height_out && drainage_out, "height_in/height_out/drainage_out is NULL");
    NZ_REQUIRE(n == 1 || work, "work is NULL");
    // every plane the call writes lies apart from every other plane of the call; planes that are only read may alias
    const nz_geom g0 = nz_geom_from_stripe(*st);
    const size_t span = (size_t)(st->rows - 1) * g0.pitch + st->cols, plane = stripe_plane_floats(*st);
    struct named { const char *name; const float *p; size_t n; };
    const named reads[] = {{"height_in", height_in, span},     {"drainageIn", desc->drainageIn, span},
                           {"rainMap", desc->rainMap, span},   {"hardness", desc->hardness, span},
                           {"upliftMap", desc->upliftMap, span}};
    const named writes[] = {{"height_out", height_out, span}, {"drainage_out", drainage_out, span},
                            {"work", n > 1 ? work : nullptr, 2 * plane}};
    auto overlap = [](const named &a, const named &b) {
        return a.p && b.p && (uintptr_t)a.p < (uintptr_t)(b.p + b.n) && (uintptr_t)b.p < (uintptr_t)(a.p + a.n);
    };
    for (size_t i = 0; i < 3; i++) {
        for (const auto &r : reads) NZ_REQUIRE(!overlap(writes[i], r), "%s overlaps %s", writes[i].name, r.name);
        for (size_t j = i + 1; j < 3; j++)
            NZ_REQUIRE(!overlap(writes[i], writes[j]), "%s overlaps %s", writes[i].name, writes[j].name);
    }
    // launch j writes set (n-1-j) & 1: 0 = the caller's output planes, where the last launch lands; 1 = `work`
    float *hs[2] = {height_out, work}, *as[2] = {drainage_out, n > 1 ? work + plane : nullptr};
    const int zlo = -st->grow0, zhi = st->grows - 1 - st->grow0;  // the global grid in buffer rows
    nz_ctx_handle_rides(ctx, out != nullptr);
    for (int j = 0; j < n; j++) {
        const int to = (n - 1 - j) & 1, widen = FLU_STRIPE_RADIUS * (n - 1 - j);
        nz_geom g = g0;
        g.or0 = st->own0 - widen > zlo ? st->own0 - widen : zlo;
        g.or1 = st->own1 + widen < zhi + 1 ? st->own1 + widen : zhi + 1;
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
// `work` in floats: 16 status words ({passes, converged, changed[3]}, the rest spare), two generations of per-tile bytes,
// each rounded up to 16 bytes, and the two W planes of count * res^2 floats the passes alternate between.  One pass is one
// launch whatever its depth, so the launch-series planner (nz_split_iterations) has nothing to split here.
namespace {
constexpr size_t FILL_STATUS = 16;
constexpr int FILL_SWEEPS = 16;  // measured: DESIGN.md section 4
std::atomic<int> fill_sweeps{FILL_SWEEPS};  // nz_debug_fill_sweeps may be called while another thread runs an entry
struct fill_layout {
    size_t gen_floats, n;  // one generation of tile bytes in floats, cells of the payload
    size_t total() const { return FILL_STATUS + 2 * gen_floats + 2 * n; }
};
fill_layout fill_layout_of(int res, int count) {
    const size_t tiles = (size_t)((res + 63) / 64) * ((res + 15) / 16) * count;
    return fill_layout{(tiles + 15) / 16 * 4, (size_t)res * res * count};
}
}  // namespace

extern "C" size_t nz_fill_depressions_work_floats(int32_t resolution, int32_t count) {
    return resolution > 0 && count > 0 ? fill_layout_of(resolution, count).total() : 0;
}

extern "C" int32_t nz_debug_fill_sweeps(int32_t sweeps) {
    return fill_sweeps.exchange(sweeps > 0 ? sweeps : FILL_SWEEPS);
}

// h: the plane that holds the input and receives the result; other: the write plane of an _rw pair or NULL
static int32_t fill_impl(nz_ctx *ctx, float *h, const float *other, float *work, const nz_fill_desc *d, int res, int count,
                         nz_handle *out) {
    NZ_REQUIRE(h && work, "src/work is NULL");
    NZ_REQUIRE(d, "desc is NULL");
    NZ_REQUIRE(std::isfinite(d->epsilon), "epsilon is not finite");
    NZ_REQUIRE(std::isfinite(d->seaLevel), "seaLevel is not finite");
    NZ_REQUIRE(d->epsilon >= 0.0f, "epsilon %g < 0", (double)d->epsilon);
    NZ_REQUIRE(d->maxPasses >= 1, "maxPasses %d < 1", d->maxPasses);
    const fill_layout L = fill_layout_of(res, count);
    auto overlap = [](const float *a, size_t na, const float *b, size_t nb) {
        return a && b && (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
    };
    NZ_REQUIRE(!overlap(d->depth, L.n, h, L.n), "depth overlaps src");
    NZ_REQUIRE(!overlap(d->depth, L.n, other, L.n), "depth overlaps the write plane");
    NZ_REQUIRE(!overlap(d->depth, L.n, work, L.total()), "depth overlaps work");
    int *status = reinterpret_cast<int *>(work);
    unsigned char *flags[2] = {reinterpret_cast<unsigned char *>(work + FILL_STATUS),
                               reinterpret_cast<unsigned char *>(work + FILL_STATUS + L.gen_floats)};
    float *planes[2] = {work + FILL_STATUS + 2 * L.gen_floats, work + FILL_STATUS + 2 * L.gen_floats + L.n};
    const float eps = d->epsilon + 0.0f;  // -0 -> +0
    const int sweeps = fill_sweeps.load();  // one cap for the whole series
    nz_ctx_handle_rides(ctx, out != nullptr);
    for (int p = 0; p < d->maxPasses; p++)  // pass p writes plane p & 1 and byte generation p & 1
        NZ_TRY(nz_launch_fill_pass(ctx->stream, h, p ? planes[(p - 1) & 1] : nullptr, planes[p & 1], status,
                                   flags[(p - 1) & 1], flags[p & 1], eps, d->seaLevel, res, count, p, sweeps));
    nz_ctx_arm_last_launch(ctx);
    // a converged series holds the fixed point in both planes, so either serves
    NZ_TRY(nz_launch_fill_finalise(ctx->stream, h, planes[0], d->depth, status, L.n));
    return nz_ctx_finish(ctx, out);
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
static fill_layout fill_stripe_layout(const nz_stripe &st) {
    const size_t tiles = (size_t)((st.cols + 63) / 64) * ((st.own1 - st.own0 + 15) / 16);
    return fill_layout{(tiles + 15) / 16 * 4, stripe_plane_floats(st)};
}

extern "C" int32_t nz_fill_stripe_halo_rows(void) { return 1; }

// 16 status words, two generations of tile bytes, the second W plane
extern "C" size_t nz_fill_stripe_work_floats(const nz_stripe *st) {
    if (!st || st->rows <= 0 || st->cols <= 0 || st->pitch < 0 || st->own0 < 0 || st->own1 < st->own0) return 0;
    const fill_layout L = fill_stripe_layout(*st);
    return FILL_STATUS + 2 * L.gen_floats + L.n;
}

extern "C" int32_t nz_fill_stripe(nz_ctx *ctx, const float *height, float *w, float *work, const nz_stripe *st,
                                  const nz_fill_desc *desc, int32_t first, const int32_t *proceed, int32_t *changed,
                                  nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(desc, "desc is NULL");
    NZ_REQUIRE(std::isfinite(desc->epsilon), "epsilon is not finite");
    NZ_REQUIRE(std::isfinite(desc->seaLevel), "seaLevel is not finite");
    NZ_REQUIRE(desc->epsilon >= 0.0f, "epsilon %g < 0", (double)desc->epsilon);
    NZ_REQUIRE(desc->maxPasses >= 1, "maxPasses %d < 1", desc->maxPasses);
    NZ_TRY(nz_check_stripe(st, 1));
    NZ_REQUIRE(height && w && work, "height/w/work is NULL");
    NZ_REQUIRE(changed, "changed is NULL");
    const nz_geom g = nz_geom_from_stripe(*st);
    const fill_layout L = fill_stripe_layout(*st);
    const size_t span = (size_t)(st->rows - 1) * g.pitch + st->cols, total = FILL_STATUS + 2 * L.gen_floats + L.n;
    auto overlap = [](const void *a, size_t na, const void *b, size_t nb) {
        return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    NZ_REQUIRE(!overlap(w, span * 4, height, span * 4), "w overlaps height");
    NZ_REQUIRE(!overlap(work, total * 4, height, span * 4), "work overlaps height");
    NZ_REQUIRE(!overlap(work, total * 4, w, span * 4), "work overlaps w");
    for (const void *p : {(const void *)height, (const void *)w, (const void *)work}) {
        NZ_REQUIRE(!overlap(changed, 4, p, p == work ? total * 4 : span * 4), "changed overlaps a plane");
        NZ_REQUIRE(!proceed || !overlap(proceed, 4, p, p == work ? total * 4 : span * 4), "proceed overlaps a plane");
    }
    int *status = reinterpret_cast<int *>(work);
    unsigned char *flags[2] = {reinterpret_cast<unsigned char *>(work + FILL_STATUS),
                               reinterpret_cast<unsigned char *>(work + FILL_STATUS + L.gen_floats)};
    float *planes[2] = {w, work + FILL_STATUS + 2 * L.gen_floats};  // pass p reads plane p & 1 and writes the other
    const float eps = desc->epsilon + 0.0f;  // -0 -> +0
    const int sweeps = fill_sweeps.load(), passes = desc->maxPasses;
    const int zlo = -st->grow0, zhi = st->grows - 1 - st->grow0;  // the global grid in buffer rows
    nz_ctx_handle_rides(ctx, out != nullptr);
    NZ_TRY(nz_launch_fill_round_begin(ctx->stream, status, proceed, changed, first != 0));
    for (int p = 0; p < passes; p++) {
        if (p == passes - 1 && !(passes & 1)) nz_ctx_arm_last_launch(ctx);
        NZ_TRY(nz_launch_fill_stripe_pass(ctx->stream, height, planes[p & 1], planes[(p + 1) & 1], w, status, flags[(p + 1) & 1],
                                          flags[p & 1], changed, eps, desc->seaLevel, g, zlo, zhi, first != 0, p, sweeps));
    }
    if (passes & 1) {  // the last pass wrote the work plane
        nz_ctx_arm_last_launch(ctx);
        NZ_TRY(nz_launch_fill_round_end(ctx->stream, w, planes[1], status, passes, g));
    }
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_fill_stripe_finalise(nz_ctx *ctx, float *height, const float *w, float *depth, const nz_stripe *st,
                                           const int32_t *converged, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(nz_check_stripe(st, 0));
    NZ_REQUIRE(height && w, "height/w is NULL");
    NZ_REQUIRE(converged, "converged is NULL");
    const nz_geom g = nz_geom_from_stripe(*st);
    const size_t span = ((size_t)(st->rows - 1) * g.pitch + st->cols) * 4;
    auto overlap = [](const void *a, size_t na, const void *b, size_t nb) {
        return a && b && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    NZ_REQUIRE(!overlap(height, span, w, span), "height overlaps w");
    NZ_REQUIRE(!overlap(depth, span, height, span), "depth overlaps height");
    NZ_REQUIRE(!overlap(depth, span, w, span), "depth overlaps w");
    nz_ctx_handle_rides(ctx, out != nullptr);
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_fill_stripe_finalise(ctx->stream, height, w, depth, converged, g));
    return nz_ctx_finish(ctx, out);
}

// ---------------------------------------------------------------------------------------------
// upsample / downsample (new-framework feature, include/noize_hip.h, nz_resample.hip)
// ---------------------------------------------------------------------------------------------
static bool planes_overlap(const float *a, size_t na, const float *b, size_t nb) {
    return (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
}

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
    NZ_REQUIRE(!planes_overlap(dst, dst_n, src, src_n), "dst overlaps src");
    NZ_REQUIRE(!base || base == dst || !planes_overlap(dst, dst_n, base, dst_n), "base partly overlaps dst");
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

static size_t stripe_span(const nz_stripe &st) { return (size_t)(st.rows - 1) * (st.pitch > 0 ? st.pitch : st.cols) + st.cols; }

extern "C" int32_t nz_upsample_stripe(nz_ctx *ctx, const float *src, const nz_stripe *srcSt, float *dst,
                                      const nz_stripe *dstSt, int32_t factor, int32_t filter, const float *base,
                                      nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_resample(factor, filter));
    NZ_TRY(check_resample_stripes(srcSt, "srcSt", dstSt, "dstSt", factor));
    NZ_REQUIRE(src, "src is NULL");
    NZ_REQUIRE(dst, "dst is NULL");
    NZ_REQUIRE(stripe_plane_floats(*dstSt) < ((size_t)1 << 31), "dst: an output of 2^31 cells or more");
    NZ_REQUIRE(!planes_overlap(dst, stripe_span(*dstSt), src, stripe_span(*srcSt)), "dst overlaps src");
    NZ_REQUIRE(!base || base == dst || !planes_overlap(dst, stripe_span(*dstSt), base, stripe_span(*dstSt)),
               "base partly overlaps dst");
    nz_up_geom g{};
    g.ccols = srcSt->cols;
    g.cpitch = srcSt->pitch > 0 ? srcSt->pitch : srcSt->cols;
    g.crows = srcSt->rows;
    g.cgrow0 = srcSt->grow0;
    g.cgrows = srcSt->grows;
    g.fcols = dstSt->cols;
    g.fpitch = dstSt->pitch > 0 ? dstSt->pitch : dstSt->cols;
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
    NZ_REQUIRE(stripe_plane_floats(*srcSt) < ((size_t)1 << 31), "src: an input of 2^31 cells or more");
    NZ_REQUIRE(!planes_overlap(dst, stripe_span(*dstSt), src, stripe_span(*srcSt)), "dst overlaps src");
    // output global rows [g0, g1) read fine global rows [f g0, f g1): all of them in the source buffer
    const int64_t f0 = (int64_t)(dstSt->own0 + dstSt->grow0) * factor - srcSt->grow0;
    const int64_t f1 = (int64_t)(dstSt->own1 + dstSt->grow0) * factor - srcSt->grow0;
    NZ_REQUIRE(dstSt->own1 == dstSt->own0 || (f0 >= 0 && f1 <= srcSt->rows),
               "srcSt: fine rows [%lld, %lld) of the buffer are required, it holds %d", (long long)f0, (long long)f1,
               srcSt->rows);
    nz_down_geom g{};
    g.ccols = dstSt->cols;
    g.cpitch = dstSt->pitch > 0 ? dstSt->pitch : dstSt->cols;
    g.cgrow0 = dstSt->grow0;
    g.fpitch = srcSt->pitch > 0 ? srcSt->pitch : srcSt->cols;
    g.fgrow0 = srcSt->grow0;
    g.w0 = dstSt->own0;
    g.w1 = dstSt->own1;
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_downsample(ctx->stream, src, dst, g, factor, 1));
    return nz_ctx_finish(ctx, out);
}

// ---------------------------------------------------------------------------------------------
// mesh
// ---------------------------------------------------------------------------------------------
extern "C" size_t nz_mesh_vertex_count(int32_t resolution) {  // VertexCount, Overshoot :26
    return resolution > 0 ? (size_t)(resolution + 1) * (resolution + 1) : 0;
}

extern "C" size_t nz_mesh_index_count(int32_t resolution) {  // IndexCount, Overshoot :28
    return resolution > 0 ? (size_t)6 * resolution * resolution : 0;
}

static int32_t heightmap_mesh_impl(nz_ctx *ctx, int32_t meshType, void *vertices, uint32_t *indices,
                                   int32_t resolution, int32_t inputResolution, int32_t marginPix, float tileHeight,
                                   float tileSize, const float *heights, int32_t count, nz_handle dep, nz_handle *out,
                                   int index16 = 0) {
    NZ_BEGIN(ctx, dep);
    (void)marginPix;  // MarginScale is commented out of the vertex path (Overshoot :64)
    NZ_REQUIRE(vertices && indices && heights, "buffer is NULL");
    NZ_REQUIRE(resolution >= 1 && resolution <= 26754, "resolution %d out of range", resolution);
    NZ_REQUIRE(inputResolution >= resolution && inputResolution <= 46340, "inputResolution %d out of range",
               inputResolution);
    int off = (inputResolution - resolution) / 2;  // PixOffset, Overshoot :33
    // shapes for which the reference would index outside the height plane are rejected
    if (meshType == NZ_MESH_OVERSHOOT_SQUARE_GRID) {
        int hi = resolution + 1 < resolution + off ? resolution + 1 : resolution + off;
        NZ_REQUIRE(hi + off <= inputResolution - 1, "overshoot mesh: margin too small for resolution %d / input %d",
                   resolution, inputResolution);
    } else if (meshType == NZ_MESH_SQUARE_GRID) {
        NZ_REQUIRE(resolution + off <= inputResolution - 1, "square mesh: inputResolution must exceed resolution");
    } else {
        nz_set_error("unknown MeshType %d", meshType);
        return NZ_ERR_INVALID;
    }
    nz_ctx_handle_rides(ctx, out != nullptr);  // vertex launch, then the index launch: the handle rides on that one
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_mesh(ctx->stream, meshType, vertices, indices, resolution, inputResolution, tileHeight, tileSize,
                          heights, count, index16));
    return nz_ctx_finish(ctx, out);
}

// HeightMapMeshJob<G, PositionStream16>: the same vertex stream, TriangleUInt16 indices (the reference's own caveat:
// only valid while the vertex count fits 16 bits, Mesh/Streams/PositionStream.cs:12)
extern "C" int32_t nz_heightmap_mesh16(nz_ctx *ctx, int32_t meshType, void *vertices, uint16_t *indices,
                                       int32_t resolution, int32_t inputResolution, int32_t marginPix,
                                       float tileHeight, float tileSize, const float *heights, nz_handle dep,
                                       nz_handle *out) {
    return heightmap_mesh_impl(ctx, meshType, vertices, reinterpret_cast<uint32_t *>(indices), resolution, inputResolution,
                               marginPix, tileHeight, tileSize, heights, 1, dep, out, 1);
}

extern "C" int32_t nz_heightmap_mesh(nz_ctx *ctx, int32_t meshType, void *vertices, uint32_t *indices,
                                     int32_t resolution, int32_t inputResolution, int32_t marginPix,
                                     float tileHeight, float tileSize, const float *heights, nz_handle dep,
                                     nz_handle *out) {
    return heightmap_mesh_impl(ctx, meshType, vertices, indices, resolution, inputResolution, marginPix, tileHeight,
                               tileSize, heights, 1, dep, out);
}

// MeshJobScheduleDelegate(Mesh, MeshData, resolution, dep, TileSize, Height), Mesh/Job/MeshJob.cs:37-60, with
// G = SharedSquareGridPosition: TileSize and Height only set mesh.bounds, the vertices span the unit square
extern "C" int32_t nz_square_grid_mesh(nz_ctx *ctx, void *vertices, uint32_t *indices, int32_t resolution, nz_handle dep,
                                       nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_REQUIRE(vertices && indices, "buffer is NULL");
    NZ_REQUIRE(resolution >= 1 && resolution <= 26754, "resolution %d out of range", resolution);
    nz_ctx_handle_rides(ctx, out != nullptr);  // vertex launch, then the index launch: the handle rides on that one
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_mesh_planar(ctx->stream, vertices, indices, resolution));
    return nz_ctx_finish(ctx, out);
}

// `count` meshes from `count` height planes stored back to back; mesh k at vertices + k * vertex_count * 48 bytes
// and indices + k * index_count
extern "C" int32_t nz_heightmap_mesh_batch(nz_ctx *ctx, int32_t meshType, void *vertices, uint32_t *indices,
                                           int32_t resolution, int32_t inputResolution, int32_t marginPix,
                                           float tileHeight, float tileSize, const float *heights, int32_t count,
                                           nz_handle dep, nz_handle *out) {
    NZ_REQUIRE(count >= 1 && count <= 65535, "count %d out of range [1,65535]", count);
    return heightmap_mesh_impl(ctx, meshType, vertices, indices, resolution, inputResolution, marginPix, tileHeight,
                               tileSize, heights, count, dep, out);
}

// ---------------------------------------------------------------------------------------------
// element-wise stages
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nz_constant_job(nz_ctx *ctx, int32_t operation, float *srcL, float *tmp, float constantValue,
                                   int32_t resolution, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(srcL, "srcL is NULL");
    (void)tmp;  // element-wise: updated in place, no flush copy
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_constant(ctx->stream, operation, srcL, (size_t)resolution * resolution, constantValue));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_reduction_job(nz_ctx *ctx, int32_t operation, float *srcL, const float *srcR, float *tmp,
                                    int32_t resolution, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(srcL && srcR, "srcL/srcR is NULL");
    (void)tmp;
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_reduce(ctx->stream, operation, srcL, srcR, (size_t)resolution * resolution));
    return nz_ctx_finish(ctx, out);
}

extern "C" int32_t nz_curve_job(nz_ctx *ctx, float *src, float *tmp, const float *curve, int32_t curveSize,
                                int32_t resolution, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(src && curve, "src/curve is NULL");
    NZ_REQUIRE(curveSize >= 2 && curveSize <= 16384, "curve length %d out of range [2,16384]", curveSize);
    (void)tmp;
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_curve(ctx->stream, src, (size_t)resolution * resolution, curve, curveSize));
    return nz_ctx_finish(ctx, out);
}

// ---- live erosion: the deterministic grid jobs ----------------------------------------
// UpdateFlowFromTrackJob.Schedule, Geologic/ParticleErosion/MultiThreadErosionJob.cs:240-261
extern "C" int32_t nz_update_flow_from_track(nz_ctx *ctx, float *pool, float *flow, float *track, float flowLossRate,
                                             float surfaceEvaporationRate, float tileHeight, int32_t resolution,
                                             nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(pool && flow && track, "pool/flow/track is NULL");
    NZ_TRY(nz_launch_flow_from_track(ctx->stream, pool, flow, track, (size_t)resolution * resolution, flowLossRate,
                                     surfaceEvaporationRate / tileHeight));
    return nz_ctx_finish(ctx, out);
}

// PoolAutomataJob (MultiThreadErosionJob.cs:264-327): `iterations` x four colour passes of WorldTile.SpreadPool.
//   NZ_POOL_RUNS=0   one lane per row, as the reference walks it (no mask);
//   otherwise        parallel runs of acting steps (nz_elementwise.hip): a masks launch, then
//       * the sparse form -- ONE launch of one workgroup that runs the whole job from the list of non-empty mask words --
//         when the last job that reported (at most 8 jobs ago) found few of them: 2 launches instead of ~50;
//       * the dense form otherwise: the sparse launch first (it still takes a job with few words and then turns the dense
//         launches into no-ops; and it reports), then 4 launches per iteration and a clean between iterations.
//   NZ_POOL_SPARSE=0: never the sparse launch; =2: always, and nothing follows it (the test matrix).
static int32_t pool_job(nz_ctx *ctx, float *pool, const float *height, int res, int iterations, int32_t *hdr, nz_particle *data) {
    static const int runs = [] { const char *e = getenv("NZ_POOL_RUNS"); return e ? atoi(e) : 1; }();
    static const int sparse = [] { const char *e = getenv("NZ_POOL_SPARSE"); return e ? atoi(e) : 1; }();
    if (!runs) {
        for (int i = 0; i < iterations; i++)
            for (int xoff = 0; xoff < 2; xoff++)
                for (int zoff = 0; zoff < 2; zoff++)
                    NZ_TRY(nz_launch_pool_automata_pass(ctx->stream, pool, height, res, xoff, zoff, hdr, data, nullptr, nullptr));
        return NZ_OK;
    }
    if (iterations == 0) return NZ_OK;
    float *p = nullptr;
    NZ_TRY(nz_ctx_scratch(ctx, nz_pool_automata_mask_words(res), &p));
    unsigned *mask = reinterpret_cast<unsigned *>(p);
    int *ctl = nullptr;
    bool dense = true;
    if (sparse) {
        NZ_TRY(nz_ctx_pool_state(ctx));
        ctl = ctx->pool_ctl;
        constexpr int LIMIT = 1024;  // non-empty words the one workgroup takes on: one per thread and pass
        const unsigned long long seq = ++ctx->pool_seq;
        const unsigned long long hint = *reinterpret_cast<volatile unsigned long long *>(ctx->pool_hint);
        const unsigned long long hint_seq = hint >> 32;
        const bool fresh = hint_seq != 0 && seq - hint_seq <= 8 && seq > hint_seq;
        dense = sparse == 2 ? false : !(fresh && (unsigned)hint <= LIMIT / 2);
        NZ_TRY(nz_launch_pool_automata_masks(ctx->stream, pool, res, mask, ctl, 1));
        NZ_TRY(nz_launch_pool_automata_sparse(ctx->stream, pool, height, res, iterations, LIMIT, dense ? 1 : 0, hdr, data, mask, ctl,
                                              ctx->pool_hint_dev, seq & 0xffffffffull));
    } else {
        NZ_TRY(nz_launch_pool_automata_masks(ctx->stream, pool, res, mask, nullptr, 0));
    }
    if (!dense) return NZ_OK;
    for (int i = 0; i < iterations; i++) {
        if (i > 0) NZ_TRY(nz_launch_pool_automata_clean(ctx->stream, pool, res, mask, ctl));
        for (int xoff = 0; xoff < 2; xoff++)
            for (int zoff = 0; zoff < 2; zoff++)
                NZ_TRY(nz_launch_pool_automata_pass(ctx->stream, pool, height, res, xoff, zoff, hdr, data, mask, ctl));
    }
    return NZ_OK;
}

// PoolAutomataJob.Schedule, MultiThreadErosionJob.cs:289-325, with drainParticles == false (the other setting feeds
// the particle queue, which is outside the deterministic part)
extern "C" int32_t nz_pool_automata(nz_ctx *ctx, float *pool, const float *height, int32_t iterations, int32_t resolution,
                                    nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(pool && height && pool != height, "pool/height must be two distinct planes");
    NZ_REQUIRE(resolution >= 2 && iterations >= 0, "resolution < 2 or iterations < 0");
    NZ_TRY(pool_job(ctx, pool, height, resolution, iterations, nullptr, nullptr));
    return nz_ctx_finish(ctx, out);
}

// PoolAutomataJob.Schedule with its whole argument list (:289-325); drainParticles feeds the particle queue
extern "C" int32_t nz_pool_automata_job(nz_ctx *ctx, float *pool, const float *height, nz_particle_queue *particleQueue,
                                        const nz_erosion_params *ep, const nz_tile_set_meta *tm, int32_t iterations,
                                        int32_t res, int32_t drainParticles, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    (void)ep;
    (void)tm;
    NZ_TRY(check_res(res));
    NZ_REQUIRE(pool && height && pool != height, "pool/height must be two distinct planes");
    NZ_REQUIRE(res >= 2 && iterations >= 0, "resolution < 2 or iterations < 0");
    NZ_REQUIRE(!drainParticles || particleQueue, "drainParticles needs a particle queue");
    int32_t *hdr = drainParticles ? nz_particle_queue_hdr(particleQueue) : nullptr;
    nz_particle *data = drainParticles ? nz_particle_queue_data(particleQueue) : nullptr;
    NZ_TRY(pool_job(ctx, pool, height, res, iterations, hdr, data));
    return nz_ctx_finish(ctx, out);
}

// CropJobDelegate, Filter/Sample/CropJob.cs:62-68
extern "C" int32_t nz_crop_job(nz_ctx *ctx, const float *input, int32_t inputResolution, float *output,
                               int32_t outputResolution, nz_handle dep, nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(inputResolution));
    NZ_TRY(check_res(outputResolution));
    NZ_REQUIRE(input && output && input != output, "input/output must be two distinct planes");
    nz_ctx_handle_rides(ctx, out != nullptr);  // one launch, nothing behind it
    nz_ctx_arm_last_launch(ctx);
    NZ_TRY(nz_launch_crop(ctx->stream, input, inputResolution, output, outputResolution));
    return nz_ctx_finish(ctx, out);
}

// ThermalErosionFilterDelegate, Filter/Kernel/Blur/ThermalErosionFilter.cs:149-157 (Schedule :117-144)
extern "C" int32_t nz_thermal_erosion(nz_ctx *ctx, float *src, float talus, float incrementRatio,
                                      float meshHeightWidthRatio, int32_t iterations, int32_t resolution, nz_handle dep,
                                      nz_handle *out) {
    NZ_BEGIN(ctx, dep);
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(src, "src is NULL");
    NZ_REQUIRE(iterations >= 0, "iterations < 0");
    float t = (talus / 90.0f) * 3.14159f / 2.0f;                             // :131
    float maxDiff = (tanf(t) * meshHeightWidthRatio) / (float)resolution;   // :132
    nz_ctx_handle_rides(ctx, out != nullptr);  // the handle rides on the last phase's launch
    for (int i = 0; i < iterations; i++) {
        const bool last = i == iterations - 1;
        if (nz_thermal_pair_fits(resolution)) {  // two phases per pass over the plane (a row beyond the LDS strip: one launch per phase)
            NZ_TRY(nz_launch_thermal_pair(ctx->stream, src, resolution, 0, maxDiff, incrementRatio));
            if (last) nz_ctx_arm_last_launch(ctx);
            NZ_TRY(nz_launch_thermal_pair(ctx->stream, src, resolution, 1, maxDiff, incrementRatio));
        } else {
            for (int flip = 0; flip < 4; flip++) {
                if (last && flip == 3) nz_ctx_arm_last_launch(ctx);
                NZ_TRY(nz_launch_thermal_phase(ctx->stream, src, resolution, flip, maxDiff, incrementRatio));
            }
        }
    }
    return nz_ctx_finish(ctx, out);
}
