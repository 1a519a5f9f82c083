/*
 * noize_hip.h -- C ABI of libnoize_hip.so: the MI355X (gfx950) replacement for the Burst job
 * structs on noize-job's per-cell terrain path.
 *
 * Every entry point replaces one reference *static delegate* (the seam the C# stages call,
 * SURVEY.md 8b) or one `PipelineStage.Schedule` body.  Conventions:
 *   - `NativeSlice<float>` / `NativeArray<float>`  ->  `float*` DEVICE pointer (nz_tile_alloc, or any
 *     hipMalloc'd / torch allocation on the ctx's device); planes are row-major, index z*res + x
 *     (Pipeline/Tiles/TileData.cs:72-77).
 *   - ALIGNMENT: a plane, map, mask, scratch (`tmp`, `work`) or argument array may be any 4-byte-aligned device pointer -- a
 *     NativeSlice(start, length) of a larger allocation, tile k of a batch of odd resolution.  The launchers take their
 *     16-byte paths where base and row pitch allow it and their scalar paths otherwise; results are the same bits, and no
 *     entry reads or writes outside the planes it is given.  16-bit index streams need 2-byte alignment, RGBA32 textures
 *     none.  The one exception: VERTEX STREAMS MUST BE 16-BYTE ALIGNED (48-byte records stored as float4); the mesh entries
 *     refuse another address with NZ_ERR_INVALID ("vertex buffer must be 16-byte aligned") before any launch.
 *   - `JobHandle dependency` -> `nz_handle dep` (0 = default(JobHandle)); the returned JobHandle ->
 *     `nz_handle* out` (may be NULL: no handle, stream order only).  Work is enqueued asynchronously on the ctx's HIP stream;
 *     where an entry ends in a kernel launch its handle is that launch's completion event (no event record of its own).
 *   - exceptions -> negative `int32` status; `nz_last_error()` gives the message.
 *   - scalar argument order is the delegate's.
 * One nz_ctx is driven by one host thread at a time (the reference schedules everything from the
 * Unity main thread, Pipeline/Executable/Pipeline.cs:29-30,154-181).
 * All citations are relative to /root/reference.
 */
#ifndef NOIZE_HIP_H
#define NOIZE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NZ_VERSION 100

typedef struct nz_ctx nz_ctx;
typedef uint64_t nz_handle;

enum nz_status {
    NZ_OK = 0,
    NZ_ERR_INVALID = -1,     /* bad argument (reference: undefined behaviour or C# exception) */
    NZ_ERR_UNSUPPORTED = -2, /* combination without an implementation (e.g. Sobel3_2D in a batched launch) */
    NZ_ERR_HIP = -3,         /* HIP runtime error */
    NZ_ERR_NOMEM = -4,
    NZ_ERR_NO_DEVICE = -5,   /* no gfx950 device / HIP runtime unavailable */
    NZ_ERR_COMM = -6,        /* RCCL error, or librccl.so.1 could not be opened */
    NZ_ERR_RETRY = -7        /* a chained kernel-filter launch timed out (nz_handle_wait / nz_ctx_synchronize report it): the
                                planes computed since are invalid, the context has switched to separate launches -- schedule
                                the work item again (the hosts' BasePipeline does, once) */
};

/* NoiseStage.FractalNoise, Noise/NoiseStage.cs:15-24 */
enum nz_noise_type {
    NZ_NOISE_SIN = 0, NZ_NOISE_PERLIN, NZ_NOISE_PERIODIC_PERLIN, NZ_NOISE_SIMPLEX,
    NZ_NOISE_ROTATED_SIMPLEX, NZ_NOISE_CELLULAR, NZ_NOISE_DOMAIN_ROTATED_PERLIN,
    NZ_NOISE_DOMAIN_ROTATED_SIMPLEX
};

/* octave shape of nz_fractal_shaped* (new-framework feature; v = the basis value the fBm sums, in [0, 1]):
 *   FBM     t += a * v                                   (what nz_fractal computes)
 *   BILLOW  t += a * |2v - 1|
 *   RIDGED  r = (ridgeOffset - |2v - 1|)^2 * w;  t += a * r;  w = clamp(r * ridgeGain, 0, 1)   (w = 1 before octave 0)
 * the result is t / CalcFractalNormValue in every shape */
enum nz_fractal_shape { NZ_SHAPE_FBM = 0, NZ_SHAPE_BILLOW = 1, NZ_SHAPE_RIDGED = 2 };

/* KernelFilterType, Filter/Kernel/KernelJob.cs:79-94 */
enum nz_kernel_filter_type {
    NZ_GAUSS9_S1 = 0, NZ_GAUSS7_S1, NZ_GAUSS5_S1, NZ_GAUSS3_S1,
    NZ_GAUSS9_S2, NZ_GAUSS7_S2, NZ_GAUSS5_S2, NZ_GAUSS3_S2,
    NZ_SMOOTH3, NZ_SOBEL3_HORIZONTAL, NZ_SOBEL3_VERTICAL, NZ_SOBEL3_2D,
    NZ_PREWITT3_HORIZONTAL, NZ_PREWITT3_VERTICAL
};

/* MeshType, Mesh/Stage/MeshTileStage.cs:23-26 */
enum nz_mesh_type { NZ_MESH_SQUARE_GRID = 0, NZ_MESH_OVERSHOOT_SQUARE_GRID = 1 };

/* Row-stripe view of a (grows x cols) global grid held by one rank (new-framework feature,
 * SURVEY.md 8e).  The buffer holds `rows` rows of `cols` floats; buffer row b is global row
 * b + grow0.  Stencil reads clamp to the global border only; rows [own0, own1) are produced, the
 * others are ghost rows the caller fills by halo exchange.  A single reference tile is
 * {res, res, 0, res, 0, res, 0}. */
typedef struct nz_stripe {
    int32_t cols;  /* cells per row */
    int32_t rows;  /* rows held in the buffer */
    int32_t grow0; /* global row of buffer row 0 (negative when ghost rows hang over the top border) */
    int32_t grows; /* rows of the global grid */
    int32_t own0;  /* owned rows [own0, own1) in buffer coordinates */
    int32_t own1;
    int32_t pitch; /* floats between consecutive rows; 0 = cols */
} nz_stripe;

/* The READ / WRITE slice pair of one tile, device resident: the reference's RWTileData
 * (Pipeline/Tiles/TileData.cs:49-93: `src` is read with a clamp, `dst` is written) together with
 * TileHelpers.SWAP_RWTILE (TileData.cs:42-45), which the reference implements as a copy job WRITE -> READ after
 * every job.  Here the swap is a swap: an `_rw` stage entry reads `read`, may use `write` as its ping-pong plane,
 * and RETURNS WITH `read` POINTING AT THE PLANE THAT HOLDS THE RESULT (the two pointers exchanged, or not) -- no
 * flush copy, and no constraint on the number of launches.  The struct is updated when the call returns (enqueue
 * time); both planes belong to the caller and stay valid until the returned handle has completed.
 * `count` tiles of resolution^2 floats stored back to back form a batch (1 = a single tile). */
typedef struct nz_rw_tile {
    float *read;
    float *write;
    int32_t resolution;
    int32_t count;
} nz_rw_tile;

/* ---- runtime ---------------------------------------------------------------------------- */
int32_t nz_version(void);
const char *nz_last_error(void);
int32_t nz_device_count(int32_t *count);

/* own stream */
int32_t nz_ctx_create(int32_t device, nz_ctx **out);
/* borrow an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream; NULL = default) */
int32_t nz_ctx_create_on_stream(int32_t device, void *hip_stream, nz_ctx **out);
int32_t nz_ctx_destroy(nz_ctx *ctx);
int32_t nz_ctx_synchronize(nz_ctx *ctx);
void *nz_ctx_stream(nz_ctx *ctx);
int32_t nz_ctx_device(nz_ctx *ctx); /* the HIP device the context was created on (-1 for NULL) */

/* Floating-point mode of a context's kernels.  The reference compiles every hot job with
 * [BurstCompile(FloatPrecision.Standard/High, FloatMode.Fast)] (Noise/Fractal/Fractal.cs:19, Filter/Kernel/KernelJob.cs:17,
 * Geologic/FlowMap/FlowMapJob.cs:16): Burst may contract and re-associate, so the reference's own results are only defined to
 * a tolerance (1e-5 relative, 1e-6 absolute is the contract of this path).
 *   NZ_FLOAT_STRICT (default): every kernel reproduces the operation sequence of the C# source, IEEE binary32, no
 *     contraction -- results are a pure function of the inputs, equal across every launch shape;
 *   NZ_FLOAT_FAST: the smooth tail of the simplex fBm octave (corner falloffs, gradient dots, octave accumulation) and the
 *     convolution tap sums are FMA-contracted; every discrete decision and every cancellation (skew / unskew, floors, lattice
 *     hashes, selects, clamps, the min filter) stays exact.  Every stage stays within 1e-5 relative / 1e-6 absolute of the strict
 *     result for the same input plane (measured at 4096^2: fBm 9e-7, Gauss5 x17 4.5e-7);
 *   NZ_FLOAT_RELAXED: FAST, and the flow map's iterations use a reciprocal (v_rcp_f32) for the outflow scale's division, an FMA
 *     in the water update, v_sqrt_f32 and a reciprocal multiply in the velocity / normalise epilogue.  The flow map itself
 *     amplifies a change of one ulp: total = water + height rounds the water (~1e-4) to the height's ulp (6e-8), so a 1e-11
 *     change of a cell's water moves its outflows by 6e-8 wherever it crosses a rounding boundary -- ~1e-4 of the cells of the
 *     metric tile leave the 1e-5 band (largest deviation 2e-5 of the normalised range), with ANY arithmetic that is not
 *     bit-identical, Burst's own FloatMode.Fast builds included.
 * Within a mode sharded == monolithic and all launch shapes of a stage still agree bit for bit.  Kernels without a tolerance
 * form run their strict one.  Applies to work enqueued after the call. */
enum nz_float_mode { NZ_FLOAT_STRICT = 0, NZ_FLOAT_FAST = 1, NZ_FLOAT_RELAXED = 2 };
int32_t nz_ctx_set_float_mode(nz_ctx *ctx, int32_t mode);
int32_t nz_ctx_float_mode(nz_ctx *ctx); /* -1 for NULL */

/* NativeArray<float>(n, Allocator.Persistent, UninitializedMemory) / Dispose() */
int32_t nz_tile_alloc(nz_ctx *ctx, size_t n_floats, float **out_dev);
int32_t nz_tile_free(nz_ctx *ctx, float *dev);
/* host NativeArray interop (async on the ctx stream; host memory must stay valid until `out` completes) */
int32_t nz_tile_upload(nz_ctx *ctx, float *dev, const float *host, size_t n_floats, nz_handle dep, nz_handle *out);
int32_t nz_tile_download(nz_ctx *ctx, const float *dev, float *host, size_t n_floats, nz_handle dep, nz_handle *out);
int32_t nz_bytes_download(nz_ctx *ctx, const void *dev, void *host, size_t n_bytes, nz_handle dep, nz_handle *out);

/* FlushWriteSliceDelegate(write_, read_, deps), Pipeline/Tiles/TileData.cs:15-42: write_.CopyFrom(read_) as a
 * job -- device to device here.  What Read/WriteGeneratorContextStage schedule
 * (Pipeline/PipelineState/Stage/ReadGeneratorContextStage.cs:36-44, WriteGeneratorContextStage.cs:30-44). */
int32_t nz_flush_write_slice(nz_ctx *ctx, float *write_, const float *read_, size_t n_floats, nz_handle dep,
                             nz_handle *out);

/* JobHandle: marker recorded on the stream after the last kernel of a call.  A handle value names the context that
 * issued it (context id in the bits above bit 40), so it may be passed as `dep` to ANY context of the process:
 * a dependency on another context's handle makes this context's stream wait for that marker on the device
 * (hipStreamWaitEvent) without blocking the host -- the reference's JobHandle dependencies between pipelines
 * (Pipeline/Executable/ReducePipeline.cs:82-148) and the job-fence locks of
 * Pipeline/PipelineState/PipelineStateLock.cs:12-39.  Handles of a destroyed context read as completed. */
int32_t nz_handle_record(nz_ctx *ctx, nz_handle *out);
/* `ctx` may be any live context: the handle names its owner */
int32_t nz_handle_query(nz_ctx *ctx, nz_handle h, int32_t *is_completed); /* JobHandle.IsCompleted */
int32_t nz_handle_wait(nz_ctx *ctx, nz_handle h);                          /* JobHandle.Complete() */
/* JobHandle.CombineDependencies(h0, h1, ...): a marker on ctx's stream that completes after all of them (handles of
 * any context; count may be 0) */
int32_t nz_handle_combine(nz_ctx *ctx, const nz_handle *handles, int32_t count, nz_handle *out);
/* the id (>= 1) of a context, and of the context a handle was issued by (0 for default(JobHandle)) */
int32_t nz_ctx_id(nz_ctx *ctx);
int32_t nz_handle_context_id(nz_handle h);
/* GPU time between two handles of `ctx` in ms (hipEventElapsedTime); both must have completed */
int32_t nz_handle_elapsed_ms(nz_ctx *ctx, nz_handle start, nz_handle stop, float *ms);

/* ---- noise: FractalJobDelegate, Noise/Fractal/Fractal.cs:76-88 ------------------------------ */
int32_t nz_fractal(nz_ctx *ctx, int32_t noiseType, float *src, int32_t resolution, float hurst,
                   float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                   int32_t xpos, int32_t zpos, int32_t noiseSize, nz_handle dep, nz_handle *out);
/* same on the owned rows of a stripe: cell (x, b) is world cell (x + xpos, b + grow0 + zpos) */
int32_t nz_fractal_stripe(nz_ctx *ctx, int32_t noiseType, float *buf, const nz_stripe *st, float hurst,
                          float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                          int32_t xpos, int32_t zpos, int32_t noiseSize, nz_handle dep, nz_handle *out);

/* nz_fractal / nz_fractal_stripe with an octave shape (enum nz_fractal_shape; ridgeOffset / ridgeGain are read by
 * NZ_SHAPE_RIDGED only, 1 and 2 are the usual values).  A shape outside the enum is NZ_ERR_INVALID and writes nothing;
 * NZ_SHAPE_FBM returns the bits of nz_fractal in every float mode. */
int32_t nz_fractal_shaped(nz_ctx *ctx, int32_t noiseType, float *src, int32_t resolution, float hurst,
                          float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                          int32_t xpos, int32_t zpos, int32_t noiseSize, int32_t shape, float ridgeOffset,
                          float ridgeGain, nz_handle dep, nz_handle *out);
int32_t nz_fractal_shaped_stripe(nz_ctx *ctx, int32_t noiseType, float *buf, const nz_stripe *st, float hurst,
                                 float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                                 int32_t xpos, int32_t zpos, int32_t noiseSize, int32_t shape, float ridgeOffset,
                                 float ridgeGain, nz_handle dep, nz_handle *out);

/* nz_fractal_shaped / nz_fractal_shaped_stripe read at domain-warped coordinates (Quilez's f(p + s q(p))).  Cell (c, r)
 * at X = c + xpos, Z = r + zpos (world cells, so adjacent tiles agree on shared cells), ns = noiseSize:
 *   u = X / ns * warpScale, v = Z / ns * warpScale;  qx = D(u, v), qz = D(u + 5.2, v + 1.3)
 *   the shaped octave loop at ((X + (2 qx - 1) warpStrength) / ns, (Z + (2 qz - 1) warpStrength) / ns)
 * D is the plain fBm of the same basis, hurst, amplitude, stepdown and detune over warpOctaves octaves, divided by its
 * norm, and is evaluated with the strict sequence in every float mode.  warpStrength is in cells (a cell moves by at most
 * about |warpStrength|); warpScale is the displacement's frequency relative to the noise.  warpStrength == 0 or
 * warpOctaves == 0 returns the bits of nz_fractal_shaped.  warpOctaves < 0, a non-finite warpStrength / warpScale or an
 * unknown shape is NZ_ERR_INVALID and writes nothing. */
int32_t nz_fractal_warped(nz_ctx *ctx, int32_t noiseType, float *src, int32_t resolution, float hurst,
                          float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                          int32_t xpos, int32_t zpos, int32_t noiseSize, int32_t shape, float ridgeOffset,
                          float ridgeGain, float warpStrength, float warpScale, int32_t warpOctaves, nz_handle dep,
                          nz_handle *out);
int32_t nz_fractal_warped_stripe(nz_ctx *ctx, int32_t noiseType, float *buf, const nz_stripe *st, float hurst,
                                 float startingAmplitude, float stepdown, float detuneRate, int32_t octaves,
                                 int32_t xpos, int32_t zpos, int32_t noiseSize, int32_t shape, float ridgeOffset,
                                 float ridgeGain, float warpStrength, float warpScale, int32_t warpOctaves,
                                 nz_handle dep, nz_handle *out);

/* ---- separable kernel filters ------------------------------------------------------------- */
/* SeperableKernelFilterDelegate, Filter/Kernel/KernelJob.cs:308-314 (one X+Z application) */
int32_t nz_kernel_filter(nz_ctx *ctx, float *src, float *tmp, int32_t filter, int32_t resolution,
                         nz_handle dep, nz_handle *out);
/* Edge1DFilterDelegate(src, tmp, EdgeAlgorithm algo, EdgeDirection dir, resolution, dep) and
 * Edge2DFilterDelegate(src, tmp, algo, resolution, dep), Filter/Kernel/Edge/EdgeJob.cs:22-43.
 * algo: 0 SOBEL, 1 PREWITT; dir: 0 HORIZONTAL, 1 VERTICAL (EdgeDetection.cs:13-21).  The 2-D form is
 * ScheduleReduce<RootSumSquaresTiles>: sqrt(horizontal^2 + vertical^2). */
int32_t nz_edge_1d_filter(nz_ctx *ctx, float *src, float *tmp, int32_t algo, int32_t dir, int32_t resolution,
                          nz_handle dep, nz_handle *out);
int32_t nz_edge_2d_filter(nz_ctx *ctx, float *src, float *tmp, int32_t algo, int32_t resolution, nz_handle dep,
                          nz_handle *out);
/* GaussFilter.GaussFilterDelegate, Filter/Kernel/Blur/BlurJob.cs:23-30 (sigma = GaussSigma enum 0..15) */
int32_t nz_gauss_filter(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t sigma,
                        int32_t resolution, nz_handle dep, nz_handle *out);
/* SmoothFilter.SmoothFilterDelegate, BlurJob.cs:46-52 */
int32_t nz_smooth_filter(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t resolution,
                         nz_handle dep, nz_handle *out);
/* SeparableKernelFilter.ScheduleSeries, KernelJob.cs:165-185; kernelX/kernelZ are HOST arrays of
 * kernelSize floats (the NativeArray<float> kernel bodies) */
int32_t nz_separable_series(nz_ctx *ctx, float *src, float *tmp, int32_t resolution, int32_t kernelSize,
                            const float *kernelX, const float *kernelZ, float kernelFactor,
                            nz_handle dep, nz_handle *out);
/* ErosionKernelJobDelegate, KernelJob.cs:350 (min-X then min-Z, window {-1,0}) */
int32_t nz_erosion_kernel(nz_ctx *ctx, float *src, int32_t resolution, nz_handle dep, nz_handle *out);

/* Stage bodies: the `iterations` loops of KernelFilterStage.Schedule (Filter/KernelFilterStage.cs:31-43),
 * StageGaussianBlur.Schedule / StageSmoothBlur.Schedule (Filter/Kernel/Blur/Stage*.cs) fused into
 * as few launches as halo growth allows.  Result lands in `src`; `tmp` is stage scratch. */
int32_t nz_kernel_filter_stage(nz_ctx *ctx, float *src, float *tmp, int32_t filter, int32_t iterations,
                               int32_t resolution, nz_handle dep, nz_handle *out);
int32_t nz_gauss_blur_stage(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t sigma,
                            int32_t iterations, int32_t resolution, nz_handle dep, nz_handle *out);
int32_t nz_smooth_blur_stage(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t iterations,
                             int32_t resolution, nz_handle dep, nz_handle *out);
/* ErosionKernelJob applied `iterations` times (the reference has no stage wrapper for it) */
int32_t nz_erosion_stage(nz_ctx *ctx, float *src, float *tmp, int32_t iterations, int32_t resolution,
                         nz_handle dep, nz_handle *out);

/* The same stage bodies on a READ / WRITE pair (nz_rw_tile above): the result is in tile->read when the call
 * returns; the flush copies of the in-place forms are gone and the launch count is free (five erosion iterations
 * are one launch, a single filter application is one launch without a copy). */
int32_t nz_kernel_filter_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, int32_t filter, int32_t iterations, nz_handle dep,
                                  nz_handle *out);
int32_t nz_gauss_blur_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, int32_t width, int32_t sigma, int32_t iterations,
                               nz_handle dep, nz_handle *out);
int32_t nz_smooth_blur_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, int32_t width, int32_t iterations, nz_handle dep,
                                nz_handle *out);
int32_t nz_erosion_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, int32_t iterations, nz_handle dep, nz_handle *out);

/* stripe forms: one launch that advances `iterations` applications on rows [own0, own1); the filter needs
 * nz_kernel_filter_halo_rows(...) valid ghost rows on each side, the min erosion `iterations` rows ABOVE only
 * (its window is {-1, 0}); rows beyond the global border are never needed.  Reads `src`, writes `dst`
 * (owned rows only). */
int32_t nz_kernel_filter_halo_rows(int32_t filter, int32_t iterations);
int32_t nz_kernel_filter_max_fused(int32_t filter);
int32_t nz_erosion_max_fused_iterations(void);
int32_t nz_kernel_filter_stripe(nz_ctx *ctx, const float *src, float *dst, const nz_stripe *st,
                                int32_t filter, int32_t iterations, nz_handle dep, nz_handle *out);
int32_t nz_erosion_stripe(nz_ctx *ctx, const float *src, float *dst, const nz_stripe *st,
                          int32_t iterations, nz_handle dep, nz_handle *out);

/* ---- flow map ------------------------------------------------------------------------------ */
/* FillArrayJobDelegate, Geologic/FlowMap/FlowMapComponents.cs:204 */
int32_t nz_fill_array(nz_ctx *ctx, float *data, int32_t resolution, float value, nz_handle dep, nz_handle *out);
/* FlowMapStepComputeFlowDelegate, Geologic/FlowMap/FlowMapJob.cs:82-98 */
int32_t nz_flowmap_compute_flow(nz_ctx *ctx, const float *src, const float *waterMap, float *flowMapN,
                                float *flowMapN__buff, float *flowMapS, float *flowMapS__buff,
                                float *flowMapE, float *flowMapE__buff, float *flowMapW,
                                float *flowMapW__buff, int32_t resolution, nz_handle dep, nz_handle *out);
/* FlowMapStepUpdateWaterDelegate, FlowMapJob.cs:154-165 */
int32_t nz_flowmap_update_water(nz_ctx *ctx, float *waterMap, float *waterMap__buff, const float *flowMapN,
                                const float *flowMapS, const float *flowMapE, const float *flowMapW,
                                int32_t resolution, nz_handle dep, nz_handle *out);
/* FlowMapWriteValuesDelegate, FlowMapJob.cs:220-228 */
int32_t nz_flowmap_write_values(nz_ctx *ctx, float *src, const float *flowMapN, const float *flowMapS,
                                const float *flowMapE, const float *flowMapW, int32_t resolution,
                                nz_handle dep, nz_handle *out);
/* MapNormalizeValuesDelegate, Filter/NormalizeJob.cs:94-100; args = HOST {min, max, range} */
int32_t nz_map_normalize_values(nz_ctx *ctx, float *src, float *tmp, const float *args,
                                int32_t resolution, nz_handle dep, nz_handle *out);
/* GetMapRangeJob.Schedule, Filter/NormalizeJob.cs:17-55: res = DEVICE {min, max, max - min} of the plane, folded from
 * lim_min / lim_max (the reference's defaults: +infinity / -infinity) with math.min / math.max: NaN cells are skipped,
 * and where the extreme is zero its sign is that of the last zero cell, as the sequential fold leaves it */
int32_t nz_get_map_range(nz_ctx *ctx, const float *map, size_t n_floats, float *res, float lim_min, float lim_max,
                         nz_handle dep, nz_handle *out);
/* MapNormalizeValuesDelegate with args = DEVICE {min, max, range} (what nz_get_map_range leaves; on a sharded grid,
 * after the ranks have all-reduced min and max) */
int32_t nz_map_normalize_values_dev(nz_ctx *ctx, float *src, float *tmp, const float *args, int32_t resolution,
                                    nz_handle dep, nz_handle *out);
/* ... on any contiguous run of cells (the owned rows of a stripe) */
int32_t nz_normalize_cells_dev(nz_ctx *ctx, float *data, size_t n_floats, const float *args, nz_handle dep,
                               nz_handle *out);
/* FlowMapStage.Schedule, Geologic/Stage/FlowMapStage.cs:124-214: fill -> iterations x (flow, water)
 * -> velocity -> normalise, result in `src`.  `work` = stage-owned scratch of
 * nz_flowmap_stage_work_floats(resolution) floats (the stage's 11 planes; flux is defined as zero
 * at the start of every run). */
size_t nz_flowmap_stage_work_floats(int32_t resolution);
int32_t nz_flowmap_stage(nz_ctx *ctx, float *src, float *work, int32_t iterations, float normMin,
                         float normMax, int32_t resolution, nz_handle dep, nz_handle *out);

/* FlowMapStage.Schedule on a READ / WRITE pair: heights are read from tile->read, the normalised flow map is
 * written to tile->write and the pair is swapped; `work` = nz_flowmap_stage_rw_work_floats(resolution, count) floats
 * (the two sets of five state planes; no private copy of the heights is needed). */
size_t nz_flowmap_stage_rw_work_floats(int32_t resolution, int32_t count);
int32_t nz_flowmap_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, int32_t iterations, float normMin,
                            float normMax, nz_handle dep, nz_handle *out);

/* stripe forms for sharded runs: state = {water, fN, fS, fE, fW} planes of the stripe's shape. */
/* `iterations` (<= nz_flow_fused_max_iterations()) whole iterations in one launch on an on-chip tile; needs
 * 2*iterations valid ghost rows of height (and of every state_in plane unless `first`).  first != 0: the
 * initial state (water 1e-4, flux 0) is implied and state_in is not read.  last != 0: the launch ends in
 * velocity + normalise and writes `dst` only; otherwise it writes the five state_out planes. */
int32_t nz_flow_fused_max_iterations(void);
int32_t nz_flow_fused_stripe(nz_ctx *ctx, const float *height, const float *const *state_in, float *const *state_out,
                             float *dst, const nz_stripe *st, int32_t iterations, int32_t first, int32_t last,
                             float normMin, float normMax, nz_handle dep, nz_handle *out);
/* The launch forms of a fused flow launch: tiles of 48 rows (512 threads), 32 or 64 rows (1024 threads) held on chip, or
 * the row-streaming kernel (whole stages only: first and last).  Within one float mode every form computes the same bits. */
enum nz_flow_form { NZ_FLOW_FORM_TILE48 = 0, NZ_FLOW_FORM_TILE32 = 1, NZ_FLOW_FORM_TILE64 = 2, NZ_FLOW_FORM_STREAM = 3 };
/* the form nz_flow_fused_stripe / one launch of the stage entries takes for `rows` produced rows of `cols` cells,
 * `count` grids, `iterations` (1..nz_flow_fused_max_iterations()) fused iterations; NZ_ERR_INVALID otherwise, NZ_ERR_HIP
 * if the context's device cannot be made current.  The rule counts the CUs of the device that was current when the process
 * first launched or queried; launcher and query share that count. */
int32_t nz_flow_launch_form(nz_ctx *ctx, int32_t cols, int32_t rows, int32_t count, int32_t iterations,
                            int32_t first, int32_t last);

/* ---- grid hydraulic erosion with sediment transport (new-framework feature) ---------------------------
 * Takes material from where water runs fast and steep and lays it down where the water slows (the subtractive flow
 * stage Geologic/Stage/ErosionStageSubtractiveFlow.cs leaves commented out).  Cell state: height b, water d, suspended
 * sediment s and the four outflows fN fS fE fW of the flow map (N is +z, E is +x).  Start: d = initialWater, s = 0, flux 0.
 * DT = 0.2, the flow map's TIMESTEP.  "Clamped": a clamp-to-edge read, as in the flow map.  Every iteration, in float32 in
 * this order, no contraction:
 *   1. d1 = d + rain
 *   2. new flux: ComputeFlowStep with totalHt = b + d1 and water_0 = d1 over the clamped neighbours' b + d1 and the old
 *      flux (nz_flowmap_compute_flow's arithmetic)
 *   3. d2 = UpdateWaterStep(d1, new flux), its in-terms clamped at the border (nz_flowmap_update_water's arithmetic)
 *   4. discharge q = CreateVelocityField's magnitude of the new flux, not normalised
 *   5. gx = (b[x+1] - b[x-1]) * 0.5, gz = (b[z+1] - b[z-1]) * 0.5 (clamped, b before this iteration's erosion),
 *      g2 = gx*gx + gz*gz, S = max(minTilt, sqrt(g2 / (1 + g2))) (the sine of the tilt)
 *   6. C = (capacity * q) * S
 *   7. C > s:     e = min(dissolve * (C - s), max(0, b - bmin4)), b -= e, s += e  (bmin4: the lowest of the four clamped
 *                 neighbours -- erosion never digs a pit);
 *      otherwise: e = deposit * (s - C), b += e, s -= e
 *   8. r = d1 >= 2^-126 ? DT / d1 : 0 (water shallower than the smallest normal float carries nothing: DT / d1 would
 *      overflow and 0 * inf lose the sediment); a_X = s * (fX * r) for X in W E S N; out = ((a_W + a_E) + a_S) + a_N;
 *      in = ((a_E[x-1] + a_W[x+1]) + a_N[z-1]) + a_S[z+1], a neighbour outside the tile contributing 0 (no flux leaves
 *      through the border, so the sediment is conserved); s = max(0, (s - out) + in)
 *   9. d = d2 * (1 - evaporation)
 * min(a, c) = c < a ? c : a and max(lo, v) = v > lo ? v : lo (a tie keeps the first operand).  After the last iteration
 * the sediment settles: the result is b + s, so the sum of the heights is conserved up to rounding.  iterations == 0
 * leaves the heights unchanged.  Strict arithmetic in every float mode (nz_ctx_set_float_mode does not apply), equal
 * bit for bit across the in-place, _rw and _batch forms and across batch positions; each tile is clamped at its own border.
 * Ranges: every argument finite; initialWater, rain, capacity, minTilt >= 0; evaporation, dissolve, deposit in [0, 1];
 * iterations >= 0 -- otherwise NZ_ERR_INVALID, the message names the argument, and nothing is written.
 * Stable range: the defaults of the hosts' HydraulicErosionStage (initialWater 1e-4, rain 1e-4, evaporation 0.01,
 * capacity 1, dissolve 0.3, deposit 0.3, minTilt 0.01) stay finite over thousands of iterations on a smoothed fBm
 * tile; capacity 0 leaves the heights unchanged, and capacities up to ~4 stay finite over 1000 iterations.
 * `work` = nz_hydraulic_erosion_work_floats(resolution, count) floats, stage-owned.  After the call completes, its first
 * count * resolution^2 floats hold the final water depth d (initialWater with no iteration) -- a river and lake mask.
 * The result lands in `src`; the _rw form reads tile->read, ping-pongs between the pair and returns with tile->read holding
 * the result; the _batch form runs `count` tiles stored back to back. */
size_t nz_hydraulic_erosion_work_floats(int32_t resolution, int32_t count);
int32_t nz_hydraulic_erosion_stage(nz_ctx *ctx, float *src, float *work, int32_t iterations, float initialWater, float rain,
                                   float evaporation, float capacity, float dissolve, float deposit, float minTilt,
                                   int32_t resolution, nz_handle dep, nz_handle *out);
int32_t nz_hydraulic_erosion_stage_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, int32_t iterations, float initialWater,
                                      float rain, float evaporation, float capacity, float dissolve, float deposit,
                                      float minTilt, nz_handle dep, nz_handle *out);
int32_t nz_hydraulic_erosion_stage_batch(nz_ctx *ctx, float *src, float *work, int32_t iterations, float initialWater,
                                         float rain, float evaporation, float capacity, float dissolve, float deposit,
                                         float minTilt, int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);

/* The same model opened up: four independent options.  With all four off the arithmetic is the one above, operation for
 * operation, and the _ex entries give the entries above bit for bit (which are the _ex entries with everything off).
 *   a. border: NZ_HYDRAULIC_BORDER_CLOSED is the model above.  NZ_HYDRAULIC_BORDER_OPEN differs in two places; every other
 *      clamped read (the discharge of step 4, the gradient of step 5, bmin4 of step 7) stays a clamp-to-edge read:
 *      step 2: a neighbour beyond the border has the total height b of the border cell itself -- its bed with no water on
 *              it -- instead of the clamped b + d1, so dX = (b + d1) - b: the cell's own water column is its head towards
 *              the outside, and the outflow over the border is scaled by the same K as the other three;
 *      step 3: the in-term of a neighbour beyond the border is +0 instead of the clamped read.
 *      Step 8 takes 0 from beyond the border and counts every a_X in `out` in both modes, so with an open border the
 *      sediment leaves with the water.  A corner cell has two neighbours outside; both rules apply per direction.
 *   b. rainMap (plane like the heights, every value finite and >= 0): step 1 is d1 = d + rain * rainMap[c], one multiply
 *      and one add, no contraction.  A plane of ones gives the no-map result bit for bit.
 *   c. hardness (plane, values in [0, 1]; 1 = cannot be eroded): in the erosion branch of step 7 `dissolve` is replaced by
 *      kd = dissolve * (1 - hardness[c]).  Deposition is not affected.  A plane of zeros gives the no-map result bit for
 *      bit.
 *   d. wear, deposits (output planes, either or both): wear[c] is the sum of e over the iterations in which cell c took the
 *      erosion branch of step 7, deposits[c] the sum of e over the iterations in which it took the other branch, plus the
 *      sediment s that settles on the cell after the last iteration: float32 running sums in iteration order, starting
 *      from +0, every iteration adding e to the mask of the branch taken and +0 to the other.  The planes need not be
 *      cleared by the caller; iterations == 0 writes zeros.  result = input - wear + deposits cell by cell up to rounding.
 * nz_hydraulic_desc carries the eight scalars of the entries above (same ranges), `border`, and the four planes; a NULL
 * plane is an option left off.  Each plane holds count * resolution^2 floats, the tiles of a batch back to back like `src`.
 * The masks may not overlap `src` (either plane of an _rw pair), the maps, each other or `work`; the maps are read-only and
 * may alias each other.  A NULL desc, a border mode other than the two, or an overlapping mask is NZ_ERR_INVALID, the
 * message names the argument, and nothing is written.  The CONTENTS of the maps are not validated on the device: values
 * outside the ranges above are the caller's.  `work` keeps its size and layout; the maps and masks are the caller's planes. */
enum nz_hydraulic_border { NZ_HYDRAULIC_BORDER_CLOSED = 0, NZ_HYDRAULIC_BORDER_OPEN = 1 };
typedef struct nz_hydraulic_desc {
    int32_t iterations;
    float initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt;
    int32_t border;          /* enum nz_hydraulic_border */
    const float *rainMap;    /* NULL: rain everywhere */
    const float *hardness;   /* NULL: dissolve everywhere */
    float *wear;             /* NULL: not recorded */
    float *deposits;         /* NULL: not recorded */
} nz_hydraulic_desc;
int32_t nz_hydraulic_erosion_ex(nz_ctx *ctx, float *src, float *work, const nz_hydraulic_desc *desc, int32_t resolution,
                                nz_handle dep, nz_handle *out);
int32_t nz_hydraulic_erosion_ex_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, const nz_hydraulic_desc *desc, nz_handle dep,
                                   nz_handle *out);
int32_t nz_hydraulic_erosion_ex_batch(nz_ctx *ctx, float *src, float *work, const nz_hydraulic_desc *desc,
                                      int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);

/* The same model on a row stripe of a larger grid (nz_stripe; sharded runs and grids that are not square).  All planes --
 * the heights, the six state planes {d, s, fN, fS, fE, fW}, the maps and the masks -- have the stripe's shape and pitch.
 * The result on the owned rows equals the monolithic model on the grows x cols grid bit for bit: the only clamps and the
 * only open border are at the global border (global rows 0 and grows-1, columns 0 and cols-1).
 *   Launches.  desc->iterations = n >= 1 iterations of this call, one launch each.  An iteration reads heights and state
 *     3 rows beyond the rows it produces (nz_hydraulic_stripe_halo_rows(n) = 3 * n for the call).  Launch j (from 0)
 *     produces the owned rows widened by 3 * (n-1-j) rows on each side, clipped to the global grid: the ghost rows the
 *     later launches need are recomputed, and the last launch produces exactly [own0, own1).
 *   Ghost rows.  Every input plane must be valid up to 3 * n rows beyond the owned rows, or up to the global border
 *     (checked against the buffer: too few rows in the buffer is NZ_ERR_INVALID).
 *   first != 0: the start state is implied (d = initialWater, s = 0, flux 0); state_in is not read and may be NULL, so only
 *     height_in needs ghost rows.
 *   last != 0: the last launch writes b + s to height_out and the water to state_out[0], on the owned rows;
 *     state_out[1..5] may be NULL when n == 1.  Without `last` the owned rows of height_out and of all six state_out planes
 *     hold the state, to be handed to the next call as height_in / state_in once their ghost rows are exchanged.
 *   Rows of the output planes inside the first launch's widened window but not owned hold unspecified values; rows outside
 *     it, and the floats between cols and pitch, are not written.
 *   `work` = nz_hydraulic_stripe_work_floats(st, n) floats: nothing for n == 1 (may be NULL), otherwise a second set of the
 *     seven planes the launches ping-pong through.  The inputs are not modified.  No plane the call writes (height_out,
 *     state_out, work, wear, deposits) may overlap any other plane of the call; planes that are only read may alias.
 *   Maps.  rainMap is read on 3 * n rows beyond the owned ones, hardness on 3 * (n-1) + 1.
 *   Masks.  wear and deposits are touched on the owned rows only (a ghost row is recomputed by two ranks and belongs to
 *     one).  With `first` they are written instead of added to; with `last` the settled sediment joins deposits.
 *   One stripe {cols, rows, 0, rows, 0, rows, 0} with first and last set is the monolithic model on a rows x cols grid,
 *     square or not; on a square grid it equals nz_hydraulic_erosion_ex bit for bit.
 * NZ_ERR_INVALID, the message naming the argument, and nothing written: the scalar ranges above; n < 1; a NULL state_in
 * without `first`; a NULL plane that is required; too few ghost rows; any overlap. */
/* ghost rows on each side a call of `iterations` iterations reads beyond the owned rows: 3 * iterations */
int32_t nz_hydraulic_stripe_halo_rows(int32_t iterations);
/* floats of `work`: 0 for one iteration, otherwise a second set of the seven planes of the stripe's shape */
size_t nz_hydraulic_stripe_work_floats(const nz_stripe *st, int32_t iterations);
int32_t nz_hydraulic_stripe(nz_ctx *ctx, const float *height_in, float *height_out, const float *const *state_in,
                            float *const *state_out, float *work, const nz_stripe *st, const nz_hydraulic_desc *desc,
                            int32_t first, int32_t last, nz_handle dep, nz_handle *out);

/* ---- batched stage bodies (new-framework feature) ------------------------------------------------
 * `count` independent tiles of resolution^2 cells stored back to back (tile k at data + k * resolution^2) go
 * through one launch sequence: the reference runs one BasePipeline per tile request
 * (Scripts/MeshTileGenerator.cs:181-211, default resolution 512), and a 512^2 tile alone cannot fill 256 CUs.
 * Every tile is clamped at its own border exactly as in the single-tile entry points; results are identical.
 * `positions` = DEVICE array of 2 * count int32 {xpos, zpos} (GeneratorData.xpos/zpos per tile).
 * Flow-map work buffer: count * nz_flowmap_stage_work_floats(resolution) floats, plane-major. */
int32_t nz_fractal_batch(nz_ctx *ctx, int32_t noiseType, float *data, int32_t resolution, int32_t count,
                         const int32_t *positions, float hurst, float startingAmplitude, float stepdown,
                         float detuneRate, int32_t octaves, int32_t noiseSize, nz_handle dep, nz_handle *out);
int32_t nz_fractal_shaped_batch(nz_ctx *ctx, int32_t noiseType, float *data, int32_t resolution, int32_t count,
                                const int32_t *positions, float hurst, float startingAmplitude, float stepdown,
                                float detuneRate, int32_t octaves, int32_t noiseSize, int32_t shape, float ridgeOffset,
                                float ridgeGain, nz_handle dep, nz_handle *out);
int32_t nz_fractal_warped_batch(nz_ctx *ctx, int32_t noiseType, float *data, int32_t resolution, int32_t count,
                                const int32_t *positions, float hurst, float startingAmplitude, float stepdown,
                                float detuneRate, int32_t octaves, int32_t noiseSize, int32_t shape, float ridgeOffset,
                                float ridgeGain, float warpStrength, float warpScale, int32_t warpOctaves,
                                nz_handle dep, nz_handle *out);
int32_t nz_kernel_filter_stage_batch(nz_ctx *ctx, float *src, float *tmp, int32_t filter, int32_t iterations,
                                     int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);
int32_t nz_gauss_blur_stage_batch(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t sigma,
                                  int32_t iterations, int32_t resolution, int32_t count, nz_handle dep,
                                  nz_handle *out);
int32_t nz_smooth_blur_stage_batch(nz_ctx *ctx, float *src, float *tmp, int32_t width, int32_t iterations,
                                   int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);
int32_t nz_erosion_stage_batch(nz_ctx *ctx, float *src, float *tmp, int32_t iterations, int32_t resolution,
                               int32_t count, nz_handle dep, nz_handle *out);
int32_t nz_flowmap_stage_batch(nz_ctx *ctx, float *src, float *work, int32_t iterations, float normMin,
                               float normMax, int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);
/* `count` meshes from height planes stored back to back (inputResolution^2 floats each); mesh k is written at
 * vertices + k * nz_mesh_vertex_count(resolution) * 48 bytes and indices + k * nz_mesh_index_count(resolution) */
int32_t nz_heightmap_mesh_batch(nz_ctx *ctx, int32_t meshType, void *vertices, uint32_t *indices,
                                int32_t resolution, int32_t inputResolution, int32_t marginPix, float tileHeight,
                                float tileSize, const float *heights, int32_t count, nz_handle dep, nz_handle *out);

/* ---- mesh: HeightMapMeshJobScheduleDelegate, Mesh/Job/HeightMapMeshJob.cs:55-65 -------------- */
/* (Mesh, MeshData) -> device vertex stream of (resolution+1)^2 records
 * {float3 position; float3 normal; float4 tangent; float2 texCoord0} = 48 B
 * (PositionStream32.Stream0, Mesh/Streams/PositionStream.cs:77-82) and device index buffer of
 * 6*resolution^2 uint32 (TriangleUInt32, Mesh/Streams/Triangle.cs:19-27).
 * `vertices` must be 16-byte aligned (NZ_ERR_INVALID otherwise, nothing written; the same for nz_heightmap_mesh16,
 * nz_heightmap_mesh_batch and nz_square_grid_mesh); `heights` and `indices` may be any 4-byte-aligned (uint16 indices:
 * 2-byte-aligned) device pointer. */
size_t nz_mesh_vertex_count(int32_t resolution);
size_t nz_mesh_index_count(int32_t resolution);
int32_t nz_heightmap_mesh(nz_ctx *ctx, int32_t meshType, void *vertices, uint32_t *indices,
                          int32_t resolution, int32_t inputResolution, int32_t marginPix,
                          float tileHeight, float tileSize, const float *heights, nz_handle dep,
                          nz_handle *out);

/* HeightMapMeshJob<G, PositionStream16> (Mesh/Streams/PositionStream.cs:11-74, TriangleUInt16 Triangle.cs:7-17): the
 * same 48-byte vertex records, indices truncated to 16 bits as `(ushort)` does -- "only valid for square mesh up to
 * resolution 256*256" (:12).  `indices`: 6 * resolution^2 uint16. */
int32_t nz_heightmap_mesh16(nz_ctx *ctx, int32_t meshType, void *vertices, uint16_t *indices, int32_t resolution,
                            int32_t inputResolution, int32_t marginPix, float tileHeight, float tileSize,
                            const float *heights, nz_handle dep, nz_handle *out);

/* ---- element-wise stages either side of the path ------------------------------ */
/* ConstantJobScheduleDelegate, Filter/ConstantJob.cs:47-53; operation = ConstantStage.ConstantOperationType
 * {MULTIPLY = 0, BINARIZE = 1} (Filter/ConstantStage.cs:15-18) */
int32_t nz_constant_job(nz_ctx *ctx, int32_t operation, float *srcL, float *tmp, float constantValue,
                        int32_t resolution, nz_handle dep, nz_handle *out);
/* ReductionJobScheduleDelegate, Filter/ReductionJob.cs:54-60; operation = ReductionType {SUBTRACT, MULTIPLY,
 * ROOTSUMSQUARES, MAX, MIN} (Filter/Reduce/ReduceStage.cs:12-18); the result lands in srcL */
int32_t nz_reduction_job(nz_ctx *ctx, int32_t operation, float *srcL, const float *srcR, float *tmp,
                         int32_t resolution, nz_handle dep, nz_handle *out);
/* CurveJobScheduleDelegate, Filter/Curve/CurveJob.cs:91-97; `curve` = DEVICE array of curveSize samples */
int32_t nz_curve_job(nz_ctx *ctx, float *src, float *tmp, const float *curve, int32_t curveSize,
                     int32_t resolution, nz_handle dep, nz_handle *out);

/* ---- live erosion: the deterministic grid jobs (planes indexed x * resolution + z, WorldTile.getIdx,
 * Geologic/ParticleErosion/LiveErosionDataTypes.cs:608-610) ------------------------------------------------
 * UpdateFlowFromTrackJob.Schedule(pool, flow, track, ep, tm, res, deps), MultiThreadErosionJob.cs:240-261:
 * ep.FLOW_LOSS_RATE, ep.SURFACE_EVAPORATION_RATE and tm.HEIGHT are passed as scalars. */
int32_t nz_update_flow_from_track(nz_ctx *ctx, float *pool, float *flow, float *track, float flowLossRate,
                                  float surfaceEvaporationRate, float tileHeight, int32_t resolution,
                                  nz_handle dep, nz_handle *out);
/* PoolAutomataJob.Schedule(pool, height, particleQueue, ep, tm, iterations, res, drainParticles, deps),
 * MultiThreadErosionJob.cs:289-325, with drainParticles == false: `iterations` x four colour passes of
 * WorldTile.SpreadPool (LiveErosionDataTypes.cs:938-1010).  The neighbour order comes from NativeArray.Sort() of
 * com.unity.collections 1.4.0 (not in the reference tree; restated: insertion sort for 4 elements). */
int32_t nz_pool_automata(nz_ctx *ctx, float *pool, const float *height, int32_t iterations, int32_t resolution,
                         nz_handle dep, nz_handle *out);

/* ---- live erosion: the particle half (BASELINE config 4).  LiveErosion.TriggerQueuedBeyerMT
 * (Geologic/ParticleErosion/Component/LiveErosion.cs:378-436) chains these jobs per cycle.  The reference is
 * deterministic per particle but not per run; this library fixes the three free choices (see nz_live.hip): the random
 * seed is an argument, per-cell event sums are 2^-40 fixed point (order-independent), and ErodeHeightMaps applies the
 * per-cell sediment events in the order one worker would have produced them (all KernelDisperse events, then the
 * PileSolver events).  Same seed, same planes -> same result, bit for bit, on every run. ------------------------- */
/* ErosionParameters, Geologic/ParticleErosion/LiveErosionDataTypes.cs:78-100 (field order kept) */
typedef struct nz_erosion_params {
    float INERTIA, GRAVITY, DRAG, FRICTION, EVAP, EROSION, DEPOSITION, FLOW_HEIGHT_CONTRIBUTION;
    float SLOW_CULL_ANGLE, SLOW_CULL_SPEED, CAPACITY;
    int32_t MAXAGE;
    float TERMINAL_VELOCITY;
    float SURFACE_EVAPORATION_RATE, POOL_PLACEMENT_MULTIPLIER, TRACK_PLACEMENT_MULTIPLIER, FLOW_LOSS_RATE;
    int32_t PILING_RADIUS;
    float MIN_PILE_INCREMENT, PILE_THRESHOLD;
} nz_erosion_params;
/* TileSetMeta, Pipeline/Tiles/TileTypes.cs:15-27 (field order kept); the jobs read GENERATOR_RES, PATCH_RES.x, HEIGHT */
typedef struct nz_tile_set_meta {
    int32_t TILE_RES[2], TILE_SIZE[2], GENERATOR_RES[2];
    float PATCH_RES[2];
    int32_t HEIGHT;
    float HEIGHT_F;
    int32_t MARGIN;
} nz_tile_set_meta;
/* a queued BeyerParticle: what its constructors set that is not a constant (LiveErosionDataTypes.cs:221-237) */
typedef struct nz_particle {
    int32_t px, pz; /* pos */
    float water;
    uint32_t pid;
} nz_particle;
/* NativeQueue<BeyerParticle> (+ the NativeList it is copied to, CopyBeyerQueueJob) in device memory */
typedef struct nz_particle_queue nz_particle_queue;
/* NativeParallelMultiHashMap<int, ErosiveEvent> events + NativeQueue<ErosiveEvent> erosions: per-cell sums, the cells
 * that received an event, and the per-cell sediment event as a dense plane */
typedef struct nz_erosive_events nz_erosive_events;

int32_t nz_particle_queue_create(nz_ctx *ctx, int32_t capacity, nz_particle_queue **out);
int32_t nz_particle_queue_destroy(nz_ctx *ctx, nz_particle_queue *queue);
/* NativeQueue.Count / ToArray (the host waits for the ctx's stream); NZ_ERR_NOMEM if a job found the queue too small */
int32_t nz_particle_queue_count(nz_ctx *ctx, nz_particle_queue *queue, int32_t *count);
int32_t nz_particle_queue_download(nz_ctx *ctx, nz_particle_queue *queue, nz_particle *host, int32_t max_count,
                                   int32_t *count);
int32_t nz_particle_queue_upload(nz_ctx *ctx, nz_particle_queue *queue, const nz_particle *host, int32_t count);
/* ClearQueueJob<BeyerParticle>.ScheduleRun(queue, deps), MultiThreadErosionJob.cs:133-153 */
int32_t nz_clear_particle_queue(nz_ctx *ctx, nz_particle_queue *queue, nz_handle dep, nz_handle *out);
int32_t nz_erosive_events_create(nz_ctx *ctx, int32_t resolution, nz_erosive_events **out);
int32_t nz_erosive_events_destroy(nz_ctx *ctx, nz_erosive_events *events);
/* device plane, x * res + z: the per-cell sediment events nz_process_beyer_erosive_events left.  READ ONLY for hosts:
 * nz_erode_height_maps finds the events through the cycle's cell list, not by scanning this plane */
float *nz_erosive_events_sediment(nz_erosive_events *events);
int32_t nz_erosive_events_count(nz_ctx *ctx, nz_erosive_events *events, int32_t *count); /* events of the last descent */

/* FillBeyerQueueJob.ScheduleParallel(particles, ep, tm, generationRound, res, maxParticles, deps, concurrency),
 * MultiThreadErosionJob.cs:37-71; `seed` replaces UnityEngine.Random.Range(0, Int32.MaxValue) (:50).  The number of
 * particles already queued is read when the job RUNS (the reference reads particles.Count when it schedules). */
int32_t nz_fill_beyer_queue(nz_ctx *ctx, nz_particle_queue *particles, const nz_erosion_params *ep,
                            const nz_tile_set_meta *tm, int32_t generationRound, int32_t res, int32_t maxParticles,
                            int32_t seed, int32_t concurrency, nz_handle dep, nz_handle *out);
/* QueuedBeyerCycleMultiThreadJob.ScheduleParallel(height, pool, flow, track, particles, events, ep, tm, eventLimit, res,
 * deps), :196-223: every queued particle descends until it is dead; the planes are read only */
int32_t nz_queued_beyer_cycle(nz_ctx *ctx, const float *height, const float *pool, const float *flow, const float *track,
                              nz_particle_queue *particles, nz_erosive_events *events, const nz_erosion_params *ep,
                              const nz_tile_set_meta *tm, int32_t eventLimit, int32_t res, nz_handle dep, nz_handle *out);
/* ProcessBeyerErosiveEventsJob.ScheduleRun(height, pool, flow, track, erosions, events, ep, tm, res, deps), :356-384 */
int32_t nz_process_beyer_erosive_events(nz_ctx *ctx, float *height, float *pool, float *flow, float *track,
                                        nz_erosive_events *events, const nz_erosion_params *ep,
                                        const nz_tile_set_meta *tm, int32_t res, nz_handle dep, nz_handle *out);
/* ErodeHeightMaps.ScheduleRun(height, erosions, ep, tm, res, deps), :459-479: applies the events of the LAST
 * nz_process_beyer_erosive_events on `events` (in place on `height`).  The PileSolver events of all four block colours run as
 * ONE launch whose busy blocks wait for their lower-coloured busy neighbours (NZ_PILE_TICKET=0: a launch per colour); that
 * wait is bounded.  A block that gives up (never, while resident waves hold the lower tickets) makes the context's next wait /
 * synchronisation return NZ_ERR_HIP -- the height plane is then invalid, and the context runs a launch per colour from then on.
 * SAFE MODE, nz_ctx_set_pile_safe(ctx, 1): the job keeps a copy of `height` as it found it (one plane copy per call), waits for
 * its ticket launch, and, should a block have given up, puts the plane back and runs itself again colour by colour: the caller
 * sees a job that succeeded (nz_ctx_pile_retries counts them).  The three hosts expose it as LiveErosion's `safe` option. */
int32_t nz_ctx_set_pile_safe(nz_ctx *ctx, int32_t on);
int32_t nz_ctx_pile_retries(nz_ctx *ctx);
/* test hook: polls after which a block of the ticket launch gives up; <= 0: the default (2^22, seconds) */
int32_t nz_debug_pile_poll_limit(int32_t polls);
int32_t nz_erode_height_maps(nz_ctx *ctx, float *height, nz_erosive_events *events, const nz_erosion_params *ep,
                             const nz_tile_set_meta *tm, int32_t res, nz_handle dep, nz_handle *out);
/* ErodeHeightMaps and UpdateFlowFromTrackJob as ONE call.  The reference schedules the two on the same dependency and
 * combines their handles (Component/LiveErosion.cs:408-412): siblings in its job graph, run side by side by the worker
 * threads.  Here the pile solver's launch -- a few thousand waves that wait for memory and for each other on an otherwise idle
 * chip -- carries the flow update's workgroups behind its own.  Results: exactly those of nz_erode_height_maps followed by
 * nz_update_flow_from_track(pool, flow, track, ep->FLOW_LOSS_RATE, ep->SURFACE_EVAPORATION_RATE, tm->HEIGHT) -- the two jobs
 * share no plane (pool / flow / track must not be `height`).  (A pile solver with more than 16 KB of
 * LDS -- PILING_RADIUS beyond ~18 -- runs the two launches one after the other.) */
int32_t nz_erode_height_maps_and_flow(nz_ctx *ctx, float *height, nz_erosive_events *events, float *pool, float *flow,
                                      float *track, const nz_erosion_params *ep, const nz_tile_set_meta *tm, int32_t res,
                                      nz_handle dep, nz_handle *out);
/* PoolAutomataJob.Schedule(pool, height, particleQueue, ep, tm, iterations, res, drainParticles, deps), :289-325:
 * with drainParticles != 0 a pool that finds a dry, lower neighbour leaves as one particle (pid 64000) in the queue */
int32_t nz_pool_automata_job(nz_ctx *ctx, float *pool, const float *height, nz_particle_queue *particleQueue,
                             const nz_erosion_params *ep, const nz_tile_set_meta *tm, int32_t iterations, int32_t res,
                             int32_t drainParticles, nz_handle dep, nz_handle *out);
/* Test hooks of the pool automaton (both entries above), whose job runs in one of several launch forms with the same results.
 * nz_debug_pool_forms sets the two process-wide switches for jobs enqueued after the call: runs == 0 = one lane per row, no
 * masks (NZ_POOL_RUNS=0); sparse == 0 = dense runs with no list and no control block, 1 = the default rule, 2 = always the
 * one-workgroup launch (NZ_POOL_SPARSE).  A negative argument restores what the environment gave (default 1 / 1); sparse
 * above 2 is NZ_ERR_INVALID.  Atomic, like nz_debug_fill_sweeps.
 * nz_debug_pool_last_job synchronises the context and reports how its last pool job (of one iteration or more) ran, six ints:
 *   [0] runs and [1] sparse as the job read them; [2] 1 if the host enqueued the dense launches; [3] 1 if the one-workgroup
 *   launch took the whole job; [4] 1 if the dense passes walked whole rows (at least seven steps in eight acted); [5] the
 *   non-empty mask words the one-workgroup launch reported for THIS job (what the next job's choice rests on), -1 if the
 *   report is another job's or there was no such launch.  With runs == 0 or sparse == 0: [3] = [4] = 0, [5] = -1.
 * NZ_ERR_INVALID: a NULL argument, or a context that has run no pool job. */
int32_t nz_debug_pool_forms(int32_t runs, int32_t sparse);
int32_t nz_debug_pool_last_job(nz_ctx *ctx, int32_t *info);
/* CurvitureMapJob.ScheduleRun(texture, height, tm, target, res, deps), :413-435: `texture` = device RGBA32 pixels of a
 * meshRes^2 texture (4 bytes per pixel), target = ColorChannelByte {R, G, B, A} */
int32_t nz_curviture_map(nz_ctx *ctx, uint8_t *texture, const float *height, const nz_tile_set_meta *tm, int32_t target,
                         int32_t res, int32_t meshRes, nz_handle dep, nz_handle *out);
/* SetRGBA32Job.ScheduleRun(src, texture, target, deps, scale), :506-528 (dataRes = sqrt(src.Length)) */
int32_t nz_set_rgba32(nz_ctx *ctx, const float *src, uint8_t *texture, int32_t target, int32_t dataRes, int32_t meshRes,
                      float scale, nz_handle dep, nz_handle *out);

/* MeshJobScheduleDelegate with G = SharedSquareGridPosition (Mesh/Job/MeshJob.cs:37-60,
 * Mesh/Generators/SharedSquareGridPosition.cs:20-50; MeshHelper.makeSquarePlanarMesh): the flat unit-square grid,
 * same vertex / index layout and counts as nz_heightmap_mesh.  TileSize / Height of the delegate only set
 * mesh.bounds and are not needed here. */
int32_t nz_square_grid_mesh(nz_ctx *ctx, void *vertices, uint32_t *indices, int32_t resolution, nz_handle dep,
                            nz_handle *out);

/* CropJobDelegate(input, inputResolution, output, outputResolution, dep), Filter/Sample/CropJob.cs:62-68.
 * As in the reference, Offset stays 0 (ScheduleParallel :43-59 never sets it): the top-left
 * outputResolution^2 corner, reads clamped to the input plane. */
int32_t nz_crop_job(nz_ctx *ctx, const float *input, int32_t inputResolution, float *output,
                    int32_t outputResolution, nz_handle dep, nz_handle *out);

/* ThermalErosionFilterDelegate, Filter/Kernel/Blur/ThermalErosionFilter.cs:149-157: `iterations` x 4 phases of
 * in-place talus relaxation on disjoint 2x2 blocks (talus in degrees) */
int32_t nz_thermal_erosion(nz_ctx *ctx, float *src, float talus, float incrementRatio, float meshHeightWidthRatio,
                           int32_t iterations, int32_t resolution, nz_handle dep, nz_handle *out);

/* Test hook for the chained filter launches (a stage of three or more fused launches runs as ONE grid whose tiles wait
 * for the tiles of the previous launch they depend on): the workgroup that takes work item `item` (items count through
 * the chain, launch 0's tiles first) sleeps `sleeps` x ~3.4 us before it loads its tile -- a straggler that reads a plane
 * later launches overwrite.  Results must not change.  item < 0: off. */
int32_t nz_debug_chain_delay(int32_t item, int32_t sleeps);
/* Test hook: polls (~2 us each) after which a tile of a chained launch gives up waiting for a producer; <= 0 restores the
 * default (2^21: seconds).  With a small limit and a long nz_debug_chain_delay the time-out path can be exercised. */
int32_t nz_debug_chain_poll_limit(int32_t polls);
/* Test hook: the kernel-filter stage on a grid that is a window of its two planes: `st` names it as a stripe whose owned
 * rows are the whole grid (own0 + grow0 == 0, own1 + grow0 == grows): columns [0, cols) of buffer rows [own0, own1), rows
 * `pitch` floats apart.  Cells of the planes outside the window are neither read nor written.  Runs the launches
 * nz_kernel_filter_stage_rw runs on a square tile (chained under the same rules); *swapped = 1: the result is in `other`. */
int32_t nz_debug_kernel_filter_window(nz_ctx *ctx, float *plane, float *other, const nz_stripe *st, int32_t filter,
                                      int32_t iterations, int32_t *swapped, nz_handle dep, nz_handle *out);
/* Context statistic: tile plans of chained filter launches this context has built and uploaded so far.  A context keeps the
 * plans of its last four geometries (columns, row window, kernel size, launch depths), so a pipeline that calls a stage
 * with the same geometry for every tile uploads once.  -1: ctx is NULL. */
int32_t nz_ctx_chain_plan_uploads(nz_ctx *ctx);

/* ---- upsample and downsample: coarse-to-fine terrain (new-framework feature) ------------------------------------------
 * The two changes of resolution the stage list lacks: erode a reduced copy of a tile, carry the change back up and add it
 * to the full-size detail (nz_downsample, nz_hydraulic_erosion_stage, nz_reduction_job SUBTRACT, nz_upsample with `base`).
 *
 * THE MODEL (tests/resample_ref.py restates it in numpy; the kernels, nz_resample.hip, follow it bit for bit):
 *   - float32 arithmetic in the order given, no contraction; identical in every float mode (nz_ctx_set_float_mode does not
 *     apply).  Factor f in {2, 4, 8}; R = the source resolution.
 *   - samples are cell-centred: fine cell j = i f + p (0 <= p < f) lies at coarse coordinate i + (2p+1)/(2f) - 1/2.
 *   UPSAMPLE, R^2 -> (R f)^2, separable.  The X pass runs on every source row needed and each result is rounded to float32;
 *   the Z pass runs over those row results with the weights of the row's phase.  Per axis:
 *       p <  f/2:  i0 = i - 1,  t = (2p+1)/(2f) + 1/2
 *       p >= f/2:  i0 = i,      t = (2p+1)/(2f) - 1/2
 *     source indices clamp to [0, R-1] (clamp to edge, as everywhere else).
 *       NZ_RESAMPLE_NEAREST      the value at i, copied with its bits
 *       NZ_RESAMPLE_BILINEAR     taps i0, i0+1, weights 1-t, t
 *       NZ_RESAMPLE_CATMULL_ROM  taps i0-1 .. i0+2, weights (-t^3+2t^2-t)/2, (3t^3-5t^2+2)/2, (-3t^3+4t^2+t)/2, (t^3-t^2)/2
 *     a tap sum is s = +0; s += v w in ascending tap order.  Every weight at these phases is a dyadic rational, exact in
 *     float32, and each tap set sums to exactly 1 (f = 2: -3/128, 29/128, 111/128, -9/128): the weights are compile-time
 *     constants per phase.  Seeded with +0, a sum never returns -0; NEAREST does.
 *     `base` (optional, fine-sized): out = base[c] + s, one add -- the detail-transfer form.  base may be dst itself (in
 *     place) or lie apart from dst.
 *   DOWNSAMPLE, R^2 -> (R/f)^2, f | R: the mean of the f x f block.  Per block row r = ((v0 + v1) + v2) + ... left to right,
 *     then m = ((r0 + r1) + r2) + ... top to bottom, then m (1/f^2), an exact power of two.
 *   - a NaN produced by this arithmetic (a tap sum, the base add, the mean) is stored as the canonical quiet NaN
 *     0x7FC00000: sign and payload of an arithmetic NaN differ between processors, and the model is one set of bits.
 *     NEAREST without base moves bits and keeps whatever NaN it is given.
 *   - each tile of a batch clamps at its own border; a stripe clamps at the global border only.
 *
 * Refused with NZ_ERR_INVALID, the argument named and nothing written: a factor outside {2, 4, 8}, an unknown filter, a
 * resolution < 1, for downsample a resolution the factor does not divide, an output of 2^31 cells or more, NULL planes,
 * dst overlapping src, base partly overlapping dst, mismatched stripe geometry.
 *
 * _batch: `count` tiles stored back to back in src, dst and base, like every _batch entry.
 * _stripe: srcSt describes the source buffer, dstSt the output buffer; the fine stripe's cols and grows are f times the
 *   coarse stripe's (the grid may be non-square), pitch is honoured on both and pad floats are not written; only the owned
 *   rows of dstSt are written.  Upsampling the owned fine global rows [g0, g1) reads the coarse global rows
 *   floor(g0/f) - halo .. floor((g1-1)/f) + halo clipped to the grid, halo = nz_upsample_stripe_halo_rows(filter) = 0
 *   nearest, 1 bilinear, 2 Catmull-Rom; downsampling output rows [g0, g1) reads fine rows [f g0, f g1).  A row that is not
 *   in the source buffer means NZ_ERR_INVALID.  `base` has dstSt's shape.  The owned rows of any split equal the
 *   monolithic result bit for bit. */
enum nz_resample_filter { NZ_RESAMPLE_NEAREST = 0, NZ_RESAMPLE_BILINEAR = 1, NZ_RESAMPLE_CATMULL_ROM = 2 };
int32_t nz_upsample(nz_ctx *ctx, const float *src, int32_t srcResolution, float *dst, int32_t factor, int32_t filter,
                    const float *base /* NULL */, nz_handle dep, nz_handle *out);
int32_t nz_upsample_batch(nz_ctx *ctx, const float *src, int32_t srcResolution, float *dst, int32_t factor, int32_t filter,
                          const float *base /* NULL */, int32_t count, nz_handle dep, nz_handle *out);
int32_t nz_downsample(nz_ctx *ctx, const float *src, int32_t srcResolution, float *dst, int32_t factor, nz_handle dep,
                      nz_handle *out);
int32_t nz_downsample_batch(nz_ctx *ctx, const float *src, int32_t srcResolution, float *dst, int32_t factor, int32_t count,
                            nz_handle dep, nz_handle *out);
int32_t nz_upsample_stripe_halo_rows(int32_t filter);
int32_t nz_upsample_stripe(nz_ctx *ctx, const float *src, const nz_stripe *srcSt, float *dst, const nz_stripe *dstSt,
                           int32_t factor, int32_t filter, const float *base /* NULL */, nz_handle dep, nz_handle *out);
int32_t nz_downsample_stripe(nz_ctx *ctx, const float *src, const nz_stripe *srcSt, float *dst, const nz_stripe *dstSt,
                             int32_t factor, nz_handle dep, nz_handle *out);

/* ---- stream-power fluvial erosion with drainage area (new-framework feature) --------------------------------------------
 * A connected river network: every cell drains to its steepest-descent neighbour of eight, the drainage area A is
 * accumulated down that tree, and the bed is lowered by k sqrt(A) slope against an uplift (the parallel form of Schott et al.
 * 2023, "Large-scale terrain authoring through interactive erosion simulation").  Besides the heights it yields the
 * drainage plane, the river map.
 *
 * THE MODEL (tests/fluvial_ref.py restates it in numpy; the kernel, nz_fluvial.hip, follows it operation for operation):
 *   Square tile res x res, row-major z * res + x, float32 throughout, no contraction, the same in every float mode
 *   (nz_ctx_set_float_mode does not apply).  State: height h, drainage A.  Start: A = drainageIn[c] when that plane is
 *   given, otherwise A = rain_c.  rain_c = rain * rainMap[c] (one multiply), without a map rain.
 *   Neighbours k = 0..7 as (dx, dz): W(-1,0) E(+1,0) S(0,-1) N(0,+1) SW(-1,-1) SE(+1,-1) NW(-1,+1) NE(+1,+1).  A neighbour
 *   outside the tile does not exist; nothing is clamped.
 *   Outlets: a cell on the tile's border (x or z is 0 or res-1), or with h[c] <= seaLevel.  An outlet has no receiver and
 *   keeps its height; it does accumulate drainage.
 *   One iteration reads h, A and writes h', A':
 *   1. receiver r(c) and slope S(c): best = +0, r = none, drop = +0; for k ascending over the existing neighbours:
 *      d = h[c] - h[k]; s = d for k < 4, otherwise s = d * 0x1.6a09e6p-1f (0.70710678f, bits 0x3F3504F3); if s > best
 *      then best = s, r = k, drop = d.  The comparison is strict: a tie keeps the earlier k.  S = best.  For an outlet
 *      r = none and S = drop = 0.
 *   2. A'[c] = rain_c; then, for k ascending over the existing neighbours whose receiver (step 1, same h) is c -- the
 *      direction opposite to k -- A'[c] = A'[c] + A[k].
 *   3. an outlet keeps h' = h.  Otherwise kc = erodibility * (1 - hardness[c]) (without a map erodibility);
 *      e = ((kc * sqrt(A'[c])) * S) * dt; lim = drop * 0.5f; e = lim < e ? lim : e; du = (dt * uplift) * upliftMap[c]
 *      (without a map dt * uplift); h' = (h - e) + du.  sqrt is the correctly rounded float32 square root.
 *   After the last iteration the heights are the result and A is the drainage plane.  iterations == 0 leaves the heights
 *   unchanged; the drainage is then the start state.
 * What follows from it: the receiver is strictly lower, so the drainage tree has no cycles.  The half-drop limit keeps
 * h' >= the old height of the receiver (a limit of the whole drop lands cells on their receiver's old height and breeds
 * flats), so no height ever falls below the input's minimum, and none rises by more than iterations * dt * uplift *
 * max(upliftMap) plus rounding.  With rain == 1 and no map the drainage values are integers, exact in float32 below 2^24.
 * With erodibility = uplift = 0 the drainage reaches, after as many iterations as the longest flow path has cells, the
 * exact accumulation over the receiver tree, and its sum over the receiver-less cells is res^2.
 * Defaults of the hosts' FluvialErosionStage: erodibility 0.05, uplift 0.002, dt 1, rain 1, seaLevel -FLT_MAX (off).
 *
 * nz_fluvial_desc carries the scalars and four optional read-only planes of count * resolution^2 floats each (NULL: the
 * option is off).  The maps are read at the cell itself only; their contents are the caller's.  A rainMap of ones, a
 * hardness of zeros and an upliftMap of ones each give the no-map result bit for bit.
 * Refused with NZ_ERR_INVALID, the message naming the argument and nothing written: a scalar that is not finite;
 * erodibility, uplift, dt or rain < 0; iterations < 0; a NULL desc; drainageIn overlapping src (either plane of an _rw
 * pair) or work; a map overlapping a plane that is written (the same planes).
 * `work` = nz_fluvial_erosion_work_floats(resolution, count) floats, stage-owned.  After the call completes, its first
 * count * resolution^2 floats hold the drainage.  The result lands in `src`; the _rw form reads tile->read, ping-pongs
 * between the pair and returns with tile->read holding the result; the _batch form runs `count` tiles stored back to back,
 * each with its own border.  The three forms and every batch position agree bit for bit. */
typedef struct nz_fluvial_desc {
    int32_t iterations;
    float erodibility, uplift, dt, rain, seaLevel;
    const float *rainMap;     /* NULL: rain everywhere */
    const float *hardness;    /* NULL: erodibility everywhere */
    const float *upliftMap;   /* NULL: uplift everywhere */
    const float *drainageIn;  /* NULL: the drainage starts at rain_c */
} nz_fluvial_desc;
size_t nz_fluvial_erosion_work_floats(int32_t resolution, int32_t count);
int32_t nz_fluvial_erosion(nz_ctx *ctx, float *src, float *work, const nz_fluvial_desc *desc, int32_t resolution,
                           nz_handle dep, nz_handle *out);
int32_t nz_fluvial_erosion_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, const nz_fluvial_desc *desc, nz_handle dep,
                              nz_handle *out);
int32_t nz_fluvial_erosion_batch(nz_ctx *ctx, float *src, float *work, const nz_fluvial_desc *desc, int32_t resolution,
                                 int32_t count, nz_handle dep, nz_handle *out);

/* The same model on a row stripe of a larger grid (nz_stripe; sharded runs and grids that are not square).  All planes --
 * the heights, the drainage, the three maps and desc->drainageIn -- have the stripe's shape and pitch.  The result on the
 * owned rows equals the monolithic model on the grows x cols grid bit for bit, heights and drainage both: outlets are the
 * cells of the global border (global rows 0 and grows-1, columns 0 and cols-1) and the cells with h <= seaLevel, a
 * neighbour outside the global grid does not exist, and a cut that is not the global border is not a border.
 *   Launches.  desc->iterations = n >= 1 iterations of this call, one launch each.  An iteration reads the receivers of the
 *     cells 1 row beyond the rows it produces, and so the heights 2 rows beyond them (nz_fluvial_stripe_halo_rows(n) = 2 * n
 *     for the call).  Launch j (from 0) produces the owned rows widened by 2 * (n-1-j) rows on each side, clipped to the
 *     global grid: the ghost rows the later launches need are recomputed, and the last launch produces exactly [own0, own1).
 *   Ghost rows.  Every input plane must be valid up to 2 * n rows beyond the owned rows, or up to the global border
 *     (checked against the buffer: too few rows in the buffer is NZ_ERR_INVALID).
 *   desc->drainageIn == NULL: the drainage starts at rain_c, as in the tile entry.  Otherwise it is the drainage carried
 *     over from the previous call (its drainage_out, once the ghost rows are exchanged).
 *   After the call the owned rows of height_out and drainage_out hold the result.  Rows of the output planes inside the
 *     first launch's widened window but not owned hold unspecified values; rows outside it, and the floats between cols and
 *     pitch, are not written.
 *   `work` = nz_fluvial_stripe_work_floats(st, n) floats: nothing for n == 1 (may be NULL), otherwise a second height and
 *     drainage plane the launches ping-pong through.  The inputs are not modified.  No plane the call writes (height_out,
 *     drainage_out, work) may overlap any other plane of the call; planes that are only read may alias.
 *   The 16-byte path runs when every plane is 16-byte aligned and cols and the pitch are multiples of 4; the 4-byte path
 *     otherwise.  Both give the same bits.
 *   One stripe {cols, rows, 0, rows, 0, rows, 0} is the model on a rows x cols grid, square or not; on a square grid it
 *     equals nz_fluvial_erosion bit for bit.  The owned rows of any split, with any number of iterations per call, equal the
 *     monolithic grid.
 * NZ_ERR_INVALID, the message naming the argument, and nothing written: the scalar ranges above; n < 1; a NULL desc or a
 * NULL plane that is required; too few ghost rows; any overlap. */
/* ghost rows on each side a call of `iterations` iterations reads beyond the owned rows: 2 * iterations */
int32_t nz_fluvial_stripe_halo_rows(int32_t iterations);
/* floats of `work`: 0 for one iteration, otherwise a second height and drainage plane of the stripe's shape */
size_t nz_fluvial_stripe_work_floats(const nz_stripe *st, int32_t iterations);
int32_t nz_fluvial_stripe(nz_ctx *ctx, const float *height_in, float *height_out, float *drainage_out, float *work,
                          const nz_stripe *st, const nz_fluvial_desc *desc, nz_handle dep, nz_handle *out);

/* ---- depression filling: lakes and pit-free drainage (new-framework feature) --------------------------------------------
 * Raises every closed hollow of a tile to its spill level (Planchon & Darboux 2001, "A fast, simple and versatile algorithm
 * to fill the depressions of digital elevation models"; Barnes et al. 2014, "Priority-flood"), so that the drainage network
 * of nz_fluvial_erosion reaches the border from its first iteration.  Filled surface minus bed is the lake depth.
 *
 * THE MODEL (tests/fill_ref.py restates it in numpy; the kernel is nz_fill.hip):
 *   Square tile res x res, row-major z * res + x, float32 throughout, no contraction, the same in every float mode
 *   (nz_ctx_set_float_mode does not apply).  Neighbours k = 0..7 in the fluvial stage's order; a neighbour outside the tile
 *   does not exist.
 *   Outlets are exactly the fluvial stage's: border cells, and cells with h[c] <= seaLevel.  W[c] = h[c] for an outlet.
 *   Operator for every other cell: m = +inf; for k ascending: t = W[k] + epsilon; m = t < m ? t : m;
 *   F(W)[c] = h[c] > m ? h[c] : m.
 *   Start: W = +inf at the non-outlets.  Result: the fixed point reached from that start.
 *   With epsilon == 0 it is the spill elevation, the minimax path height to an outlet; flats remain.  With epsilon > 0 every
 *   filled cell sits at least epsilon above some neighbour, so every non-outlet cell has a strictly lower neighbour and the
 *   fluvial stage finds a receiver for it -- as long as epsilon is not absorbed by rounding at the tile's magnitudes.
 * What follows from it: F is monotone and the start lies above every fixed point, so the result is the greatest fixed point
 * and does not depend on the order of updates (Jacobi, tile-local sweeps and a priority flood give the same floats).
 * W >= h; outlets are unchanged; filling a filled tile changes nothing; a tile without pits is returned bit for bit (with
 * epsilon == 0; with epsilon > 0, a tile whose every non-outlet cell already lies epsilon above a neighbour); the result is
 * never below the input's minimum.  Heights must be finite; otherwise the result is unspecified, but the call terminates,
 * since the number of launches is fixed.
 *
 * The entry enqueues maxPasses pass launches and one finalise launch, stream-ordered like every other entry.  A pass sweeps
 * every 64 x 16 tile on chip against its frozen ring, skips tiles whose neighbourhood was at rest in the pass before, and
 * returns at once when the pass before changed nothing (a launch of that kind costs a few microseconds: tools/bench_fill.py
 * measures it).  The result is ALL OR NOTHING: when the last pass that ran changed nothing, W lands in the heights and, where
 * asked, W - h in `depth`; otherwise -- the budget was too small -- the heights stay as they were, `depth` is zero, and that
 * is not an error.  After the call completes the first two int32 of `work` hold {passes that did work, converged 0/1}.
 * Default of the hosts' DepressionFillStage: epsilon 1e-4, seaLevel -FLT_MAX (off), maxPasses 64 + resolution / 4.  The
 * evidence (tools/bench_fill.py): an unfiltered 13-octave simplex fBm tile, 45 % of whose cells lie in
 * hollows at 1024^2 and 68 % at 4096^2, converges in 50 and 152 passes; the defaults allow 320 and 1088.  As a rule of
 * thumb, not a bound: a straight front crosses a tile (16 rows or 64 columns) per pass, so resolution / 16 passes cross the
 * plane once and the default leaves four crossings; a winding spill path needs more passes per crossing.  A budget that
 * runs out shows as converged == 0.  The unused launches cost 2 to 6 microseconds each.
 *
 * `work` = nz_fill_depressions_work_floats(resolution, count) floats, stage-owned; the size depends on the number of 64 x 16
 * tiles, so two payloads of equal cell count may need different sizes.  The result lands in `src`, or in
 * tile->read for the _rw form (the pair is not swapped; tile->write is left alone).  The _batch form runs `count` tiles stored
 * back to back, each with its own border; the status words cover the whole batch.  The three forms and every batch position
 * agree bit for bit.
 * Refused with NZ_ERR_INVALID, the message naming the argument and nothing written: epsilon or seaLevel not finite
 * (-FLT_MAX switches the sea off); epsilon < 0; maxPasses < 1; a NULL desc; depth overlapping src, either plane of an _rw
 * pair, or work. */
typedef struct nz_fill_desc {
    float epsilon, seaLevel;
    int32_t maxPasses;
    float *depth;  /* NULL: not wanted */
} nz_fill_desc;
size_t nz_fill_depressions_work_floats(int32_t resolution, int32_t count);
int32_t nz_fill_depressions(nz_ctx *ctx, float *src, float *work, const nz_fill_desc *desc, int32_t resolution, nz_handle dep,
                            nz_handle *out);
int32_t nz_fill_depressions_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, const nz_fill_desc *desc, nz_handle dep,
                               nz_handle *out);
int32_t nz_fill_depressions_batch(nz_ctx *ctx, float *src, float *work, const nz_fill_desc *desc, int32_t resolution,
                                  int32_t count, nz_handle dep, nz_handle *out);
/* The same model on a row stripe of a larger grid (nz_stripe), one ROUND per call; the rounds of all stripes, with one row
 * of W exchanged between them, go down to the monolithic fixed point bit for bit, because the operator is monotone and its
 * fixed point does not depend on the order of updates.  All planes have the stripe's shape and pitch.
 *   nz_fill_stripe runs at most desc->maxPasses passes of the pass kernel's scheme (64 x 16 tiles swept on chip, quiet tiles
 *     skipped, early return once a pass changed nothing) over the owned rows.  The one ghost row of `w` on each side is
 *     FROZEN: read, never written.  Outlets, and neighbours that do not exist, follow the global grid (global rows 0 and
 *     grows-1, columns 0 and cols-1; h <= seaLevel); a cut is no border.  Rows of the buffers beyond the one ghost row are
 *     neither read nor written, nor are the floats between cols and pitch.
 *   first != 0: the start state is derived from `height` on the owned rows and the ghost rows (outlets take h, every other
 *     cell +inf); `height` needs one valid ghost row and `w` is not read.  Otherwise the current W is read from `w`, whose
 *     ghost rows the caller has exchanged.
 *   On return the owned rows of `w` hold the stripe's W.  `changed` (device) receives 1 with `first`, 1 if any owned cell of
 *     `w` differs from its value at entry (a budget that ran out before rest included), otherwise 0.
 *   proceed (device, may be NULL): a word of zero makes every launch of the call return at once -- `w` untouched, `changed`
 *     0 -- so that a host can enqueue a fixed budget of rounds without reading anything back.
 *   desc->depth is not used.  `work` = nz_fill_stripe_work_floats(st) floats: status words, tile bytes, a second W plane.
 *   nz_fill_stripe_finalise, on the owned rows: where *converged != 0, height = w and depth = w - h; otherwise height stays
 *     and depth = 0 -- all or nothing, no +inf ever reaches the caller.  `converged` is the caller's verdict: the vote over
 *     all ranks after the last round was 0 (nz_comm_allreduce_max_i32).
 *   One stripe over a square grid with `first`, followed by finalise with a word of 1, equals nz_fill_depressions bit for
 *     bit, depth included, provided the budget suffices.
 * NZ_ERR_INVALID, the message naming the argument, and nothing written: epsilon or seaLevel not finite; epsilon < 0;
 * maxPasses < 1; a NULL desc, plane or word; a missing ghost row; height, w and work (finalise: height, w, depth)
 * overlapping each other or the words. */
int32_t nz_fill_stripe_halo_rows(void); /* 1 */
size_t nz_fill_stripe_work_floats(const nz_stripe *st);
int32_t nz_fill_stripe(nz_ctx *ctx, const float *height, float *w, float *work, const nz_stripe *st, const nz_fill_desc *desc,
                       int32_t first, const int32_t *proceed, int32_t *changed, nz_handle dep, nz_handle *out);
int32_t nz_fill_stripe_finalise(nz_ctx *ctx, float *height, const float *w, float *depth, const nz_stripe *st,
                                const int32_t *converged, nz_handle dep, nz_handle *out);
/* Test hook: the cap on a pass's on-chip sweeps per tile (process-wide; <= 0 restores the default, 16).  Results must not
 * change: the fixed point does not depend on the schedule.  Returns the cap that was in force.  Atomic: it may be called
 * while entries run on other threads; a call that has begun keeps the cap it read. */
int32_t nz_debug_fill_sweeps(int32_t sweeps);

/* ---- drainage area: the exact river map of a heightmap in one call (new-framework feature) ------------------------------
 * The flow accumulation over the steepest-descent tree: what nz_fluvial_erosion's drainage plane turns into when the bed
 * stands still, computed directly.  Feed it a filled tile (nz_fill_depressions) and every river reaches the border.
 *
 * THE MODEL (tests/drainage_ref.py restates it as a topological walk; the kernels are nz_drainage.hip):
 *   Square tile res x res, row-major z * res + x, float32 throughout, no contraction, the same in every float mode
 *   (nz_ctx_set_float_mode does not apply).  Outlets, the neighbour order W E S N SW SE NW NE, "a neighbour outside the
 *   tile does not exist" and the receiver r(c) with its strict comparison and tie rule are exactly step 1 of the fluvial
 *   model above.
 *   rain_c = rain * rainMap[c] (one multiply), or rain without a map.
 *   The result is the plane A with, for every cell: A[c] = rain_c; then, for k ascending over the existing neighbours whose
 *   receiver is c, A[c] = A[c] + A[k].
 * That is step 2 of the fluvial model at rest.  A receiver is strictly lower than its donor, so the receiver graph has no
 * cycle, every cell's value is a fixed function of its donors' values, and the plane is unique whatever the order of updates
 * (Jacobi, tile-local sweeps and a topological walk give the same floats).  What follows:
 *   - the result equals what nz_fluvial_erosion with erodibility = uplift = 0 reaches after enough iterations, bit for bit;
 *   - it is a valid nz_fluvial_desc.drainageIn: the fluvial stage then erodes with the formed river network from its first
 *     iteration instead of starting at A = rain_c;
 *   - outlets and pits accumulate and pass nothing on;
 *   - with rain == 1 and no map every value is an integer, and the sum over the receiver-less cells is res^2.
 * `height` is read only.
 *
 * The entry enqueues one mask launch (heights -> one donor byte per cell: bit k set when neighbour k drains into the cell),
 * maxPasses pass launches and one finalise launch, stream-ordered; nothing is read back.  A pass is nz_fill_depressions'
 * scheme applied to A: every 64 x 16 tile is swept on chip against its frozen ring, tiles whose neighbourhood was at rest in
 * the pass before are skipped, and a launch returns at once when the pass before changed nothing.  After completion the
 * first two int32 of `work` hold {passes that did work, converged 0/1}.  The result is ALL OR NOTHING: when the last pass
 * that ran changed nothing, `drainage` holds the fixed point; otherwise -- the budget was too small -- `drainage` holds the
 * start state rain_c in every cell and converged == 0, which is not an error.  A partial state would depend on the schedule
 * and never reaches the caller.  A pass is at least one Jacobi step, so a budget of "cells of the longest flow path" + 1
 * always suffices; the hosts' default is far below that and measured ("drainage area").
 * Defaults of the hosts' DrainageAreaStage: rain 1, seaLevel -FLT_MAX (off), maxPasses 64 + resolution / 4.
 * The evidence (tools/bench_drainage.py): the 13-octave simplex fBm tile behind nz_fill_depressions
 * comes to rest in 82 passes at 1024^2 and 192 at 4096^2; the defaults allow 320 and 1088.  Not a bound: a path that winds
 * through many tiles needs more, and a budget that runs out shows as converged == 0.
 *
 * `work` = nz_drainage_area_work_floats(resolution, count) floats, stage-owned: status words, tile bytes, the donor bytes
 * and one A plane (the other is `drainage`).  The _batch form runs `count` tiles stored back to back, each with its own
 * border; every batch position equals the single-tile call bit for bit, and the status words cover the whole batch.
 * resolution == 0 or count == 0 does nothing and returns NZ_OK.  The 16-byte path runs when every plane is 16-byte aligned
 * and resolution % 4 == 0, the 4-byte path otherwise; both give the same bits.
 * Refused with NZ_ERR_INVALID, the message naming the argument and nothing written: rain or seaLevel not finite (-FLT_MAX
 * switches the sea off); rain < 0; maxPasses < 1; a NULL desc, height, drainage or work; drainage overlapping height, work
 * or rainMap; work overlapping height or rainMap.
 * There is no _rw form (the heights do not change) and no receiver-code output: nz_watershed, below, has one. */
typedef struct nz_drainage_desc {
    float rain, seaLevel;
    int32_t maxPasses;
    const float *rainMap;   /* NULL: rain everywhere */
} nz_drainage_desc;
size_t nz_drainage_area_work_floats(int32_t resolution, int32_t count);
int32_t nz_drainage_area(nz_ctx *ctx, const float *height, float *drainage, float *work, const nz_drainage_desc *desc,
                         int32_t resolution, nz_handle dep, nz_handle *out);
int32_t nz_drainage_area_batch(nz_ctx *ctx, const float *height, float *drainage, float *work, const nz_drainage_desc *desc,
                               int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);
/* The same model on a row stripe of a larger grid (nz_stripe), one ROUND per call, in the wording of nz_fill_stripe.  The
 * receiver graph is a forest, so rounds of per-stripe relaxation against one frozen ghost row of A on each side, with one
 * row of A exchanged between them, reach the monolithic plane bit for bit: a cell whose donors all hold their final values
 * takes its final value in the next round at the latest, and by induction over the height of the forest the rounds end --
 * with a signed rainMap too.  All planes have the stripe's shape and pitch, desc->rainMap included.
 *   (The round entry carries _round in its name: one call is one round.)
 *   nz_drainage_stripe_round runs at most desc->maxPasses passes of the pass kernel's scheme (64 x 16 tiles swept on chip against
 *     their frozen ring, quiet tiles skipped, early return once a pass changed nothing) over the owned rows; the first pass
 *     of a round starts a fresh series and visits every tile, because the ghost rows may have changed.  The one ghost row
 *     of `a` on each side is FROZEN: read, never written.  Outlets, and neighbours that do not exist, follow the global grid
 *     (global rows 0 and grows-1, columns 0 and cols-1; h <= seaLevel); a cut is no border.  Rows beyond what is needed are
 *     neither read nor written, nor are the floats between cols and pitch.
 *   first != 0: a mask launch turns `height` into donor bytes in `work`; a ghost-row cell's receiver looks one row further
 *     out, so `height` needs TWO valid ghost rows towards every cut.  The start state is rain_c on the owned rows and the
 *     ghost row: rainMap needs one valid ghost row, `a` is not read.
 *   first == 0: `height` is not read; `work` must be the buffer of the round before, untouched in between (it carries the
 *     donor bytes); the current A is read from `a`, whose ghost rows the caller has exchanged.
 *   On return the owned rows of `a` hold the stripe's A, whatever the parity of the passes that ran.  `changed` (device)
 *     receives 1 with `first`; otherwise 1 if any single update of any pass of the round changed a value (values may move
 *     both ways, so this is not "differs from the entry state"), a budget that ran out before rest included; 0 only when
 *     the round's first pass found every owned cell at rest against the ghost rows.
 *   proceed (device, may be NULL): a word of zero makes every launch of the call return at once -- `a` untouched, `changed`
 *     0 -- so that a host can enqueue a fixed budget of rounds without reading anything back.
 *   `work` = nz_drainage_stripe_work_floats(st) floats: status words and tile bytes as nz_fill_stripe leaves them, the donor
 *     bytes, a second A plane.
 *   nz_drainage_stripe_finalise, on the owned rows: where *converged != 0, `a` stays; otherwise a = rain_c -- all or
 *     nothing, as in the tile entry.  `converged` is the caller's verdict: the vote over all ranks after the last round was
 *     0 (nz_comm_allreduce_max_i32).
 *   One stripe over a square grid with `first`, followed by finalise with the verdict "`changed` of a second round == 0",
 *     equals nz_drainage_area bit for bit, on the 16-byte path (all planes 16-byte aligned, pitch % 4 == 0) and the 4-byte one.
 * NZ_ERR_INVALID, the message naming the argument, and nothing written: rain or seaLevel not finite; rain < 0;
 * maxPasses < 1; a NULL desc, plane or word; a missing ghost row (2 with `first`, else 1); height, a, work, rainMap or the
 * words overlapping where one of them is written. */
int32_t nz_drainage_stripe_halo_rows(void); /* 2: the heights; A and rainMap need 1 */
size_t nz_drainage_stripe_work_floats(const nz_stripe *st);
int32_t nz_drainage_stripe_round(nz_ctx *ctx, const float *height, float *a, float *work, const nz_stripe *st,
                           const nz_drainage_desc *desc, int32_t first, const int32_t *proceed, int32_t *changed,
                           nz_handle dep, nz_handle *out);
int32_t nz_drainage_stripe_finalise(nz_ctx *ctx, float *a, const nz_stripe *st, const nz_drainage_desc *desc,
                                    const int32_t *converged, nz_handle dep, nz_handle *out);
/* Test hook, the twin of nz_debug_fill_sweeps: the cap on a drainage pass's on-chip sweeps per tile (process-wide; <= 0
 * restores the default).  Results must not change.  Returns the cap that was in force. */
int32_t nz_debug_drainage_sweeps(int32_t sweeps);

/* ---- multiple-flow drainage: slope-weighted flow accumulation (new-framework feature) ------------------------------------
 * nz_drainage_area gives all of a cell's water to its steepest neighbour, which draws parallel one-cell lines along the
 * eight grid directions on hillsides and cannot spread water on a fan.  This entry routes the area with multiple flow
 * directions (Freeman 1991; Quinn et al. 1991; Holmgren 1994): every lower neighbour takes a share that grows with its
 * slope.  The plane is a drop-in for nz_drainage_area's wherever a drainage plane is read (nz_fluvial_implicit,
 * nz_stream_order, nz_fluvial_desc.drainageIn).
 *
 * THE MODEL (tests/drainage_mfd_ref.py restates it in numpy; the kernels are nz_drainage_mfd.hip):
 *   Square tile res x res, row-major z * res + x, float32 throughout, every operation rounded once, no contraction, the
 *   same in every float mode (nz_ctx_set_float_mode does not apply).  The outlets (global border, or h <= seaLevel), the
 *   neighbour order W E S N SW SE NW NE, "a neighbour outside the tile does not exist" and DIAG = 0x1.6a09e6p-1f are
 *   exactly step 1 of the fluvial model above.  rain_c = rain * rainMap[c] (one multiply), or rain without a map.
 *   Per cell c that is not an outlet, with `best` the S of its receiver rule (the largest s_k, +0 when none):
 *     for k ascending over the existing neighbours: d = h[c] - h[k]; s_k = d for k < 4, else d * DIAG;
 *     neighbour k takes flow iff s_k > 0;
 *     q_k = s_k / best (one correctly rounded division; the steepest neighbour has q == 1 exactly, nothing overflows, and
 *       subnormal slopes work);
 *     g_k = q_k, then exponent - 1 times g_k = g_k * q_k, left to right;
 *     T = +0; for k ascending with g_k > 0: T = T + g_k;
 *     w_k = g_k / T for g_k > 0 (one correctly rounded division), else the edge carries nothing -- a g_k that underflowed
 *       to 0 is "nothing".
 *   Outlets and cells without a lower neighbour send nothing.
 *   The plane A: for every cell A[c] = rain_c; then, for k ascending over the existing neighbours whose weight towards c is
 *   w > 0: A[c] = A[c] + (w * A[k]) -- product first, then sum.  The gate is w > 0, never the value of A.
 * What follows from it:
 *   - flow goes strictly downhill, so the graph has no cycle; a cell's value is a fixed function of higher cells' values, so
 *     Jacobi, tile sweeps and a walk highest cell first end in the same bits;
 *   - a cell with exactly one lower neighbour sends w == 1: it behaves as in nz_drainage_area;
 *   - a cell's outgoing weights sum to 1 within 2^-20;
 *   - with rain >= 0 and no map, A >= rain;
 *   - NaN heights send and receive nothing.
 * HEIGHT DIFFERENCES MUST BE FINITE.  An infinite s gives NaN weights, and the gate drops them: such a cell sends nothing
 * at all, and no NaN reaches the plane, but that is not the flow of any terrain.
 * exponent 1 is Quinn's rule without contour lengths, larger exponents concentrate the flow on the steepest neighbours
 * (Holmgren), and the limit is nz_drainage_area.  `height` is read only.
 *
 * Everything that is not about weights is nz_drainage_area's: the entry enqueues one setup launch (heights -> per cell the
 * eight INCOMING weights, eight float planes in `work`; it holds all the divisions, and after it no launch reads a
 * height), maxPasses pass launches and one finalise launch, stream-ordered; nothing is read back.  After completion the
 * first two int32 of `work` hold {passes that did work, converged 0/1}; the converged word is usable as
 * nz_fluvial_implicit_desc.proceed.  The result is ALL OR NOTHING: a budget that runs out leaves rain_c in every cell and
 * converged == 0, and that is no error.  A pass is at least one Jacobi step, so "cells of the longest path of the flow
 * graph" + 1 always suffices; paths are longer than the steepest-descent tree's, and the hosts' default is twice
 * DrainageAreaStage's: rain 1, seaLevel -FLT_MAX (off), exponent 1, maxPasses 128 + resolution / 2 (DESIGN.md section 4,
 * "multiple-flow drainage").
 * `work` = nz_drainage_mfd_work_floats(resolution, count) floats, stage-owned: status words, tile bytes, eight weight planes
 * and one A plane (the other is `drainage`).  The _batch form runs `count` tiles stored back to back, each with its own
 * border; every batch position equals the single-tile call bit for bit, and the status words cover the whole batch.
 * resolution == 0 or count == 0 does nothing and returns NZ_OK.  The 16-byte path runs when every plane is 16-byte aligned
 * and resolution % 4 == 0, the 4-byte path otherwise; both give the same bits.
 * Refused with NZ_ERR_INVALID, the message naming the argument and nothing written: rain or seaLevel not finite (-FLT_MAX
 * switches the sea off); rain < 0; maxPasses < 1; exponent outside 1..16; a NULL desc, height, drainage or work; drainage
 * overlapping height, work or rainMap; work overlapping height or rainMap.
 * There is no row-stripe form and no _rw form (the heights do not change). */
typedef struct nz_drainage_mfd_desc {
    float rain, seaLevel;
    int32_t maxPasses;
    int32_t exponent;       /* 1..16 */
    const float *rainMap;   /* NULL: rain everywhere */
} nz_drainage_mfd_desc;
size_t nz_drainage_mfd_work_floats(int32_t resolution, int32_t count);
int32_t nz_drainage_mfd(nz_ctx *ctx, const float *height, float *drainage, float *work, const nz_drainage_mfd_desc *desc,
                        int32_t resolution, nz_handle dep, nz_handle *out);
int32_t nz_drainage_mfd_batch(nz_ctx *ctx, const float *height, float *drainage, float *work,
                              const nz_drainage_mfd_desc *desc, int32_t resolution, int32_t count, nz_handle dep,
                              nz_handle *out);
/* Test hook, the twin of nz_debug_drainage_sweeps: the cap on a multiple-flow pass's on-chip sweeps per tile (process-wide;
 * <= 0 restores the default).  Results must not change.  Returns the cap that was in force. */
int32_t nz_debug_drainage_mfd_sweeps(int32_t sweeps);

/* ---- watershed: basin labels, flow length and receiver codes of a heightmap (new-framework feature) --------------------
 * The steepest-descent tree read the other way: which outlet a cell drains to, how far along the river it lies, and the
 * tree itself.  Catchment labels give lake and basin masks and regions per river system, the flow length a distance to the
 * mouth, the receiver plane lets a host trace river polylines.  Feed it a filled tile (nz_fill_depressions) and every label
 * lies on the border.
 *
 * THE MODEL (tests/watershed_ref.py restates it as a walk lowest cell first; the kernels are nz_watershed.hip):
 *   Square tile res x res, row-major c = z * res + x, float32 heights, read only.  Outlets, the neighbour order
 *   W E S N SW SE NW NE, "a neighbour outside the tile does not exist" and the receiver r(c) with its strict comparison and
 *   tie rule are exactly step 1 of the fluvial model above: border cells and cells <= seaLevel have no receiver, and an
 *   interior cell without a strictly lower neighbour, a pit, has none either.  For every cell:
 *     r(c) == NONE:  basin[c] = c (int32) and length[c] = +0;
 *     otherwise, with q the neighbour r(c) names:  basin[c] = basin[q] and length[c] = length[q] + step_k,
 *   step_k = cellSize for k < 4 and cellSize * 0x1.6a09e6p+0f (one product, rounded once to float32) for k >= 4.  No
 *   contraction, the same in every float mode (nz_ctx_set_float_mode does not apply).  In a batch c is the index inside the
 *   cell's own tile.
 * A receiver is strictly lower than its donor, so the graph is a forest, a cell's value is a fixed function of one other
 * cell's final value and the fixed point is unique: a walk lowest cell first, Jacobi and tile sweeps end in the same bits.
 * What follows:
 *   - every label names a cell without a receiver, and basin[basin[c]] == basin[c];
 *   - the number of cells that carry label o is what nz_drainage_area with rain 1 holds at o;
 *   - length with cellSize 2 is twice length with cellSize 1, bit for bit.
 * `receivers` (optional, NULL: not wanted) receives one byte per cell: the code 0..7, or 8 for outlets and pits alike.
 * `length` is optional too (NULL): a labels-only call carries no float plane at all.
 *
 * The entry enqueues one receiver launch (heights -> one receiver byte per cell, into `receivers` or `work`), maxPasses
 * pass launches and one finalise launch, stream-ordered; nothing is read back.  A pass is nz_drainage_area's scheme with
 * the data flow reversed: every 64 x 16 tile is swept on chip against its frozen ring, each cell reading the one cell its
 * code names; tiles whose neighbourhood was at rest in the pass before are skipped, and a launch returns at once when the
 * pass before changed nothing.  After completion the first two int32 of `work` hold {passes that did work, converged 0/1}.
 * The result is ALL OR NOTHING: when the last pass that ran changed nothing, `basin` and `length` hold the fixed point;
 * otherwise -- the budget was too small -- they hold the start state, own index and +0, and converged == 0, which is not
 * an error (`receivers` is complete either way).  A pass is at least one Jacobi step, so a budget of "moves of the longest
 * flow path" + 2 always suffices; the hosts' default is far below that and measured ("watershed").
 * Defaults of the hosts' WatershedStage: seaLevel -FLT_MAX (off), cellSize 1, maxPasses 64 + resolution / 4, with length,
 * without receivers.
 * The evidence (tools/bench_watershed.py): the 13-octave simplex fBm tile behind nz_fill_depressions
 * comes to rest in 82 passes at 1024^2 and 192 at 4096^2, as nz_drainage_area does; the defaults allow 320 and 1088.  Not
 * a bound: a path that winds through many tiles needs more, and a budget that runs out shows as converged == 0.
 *
 * `work` = nz_watershed_work_floats(resolution, count, withLength) floats, stage-owned, withLength != 0 for a call with a
 * `length` plane: status words, tile bytes, the receiver bytes and the second plane of each pair (the first is the
 * caller's).  0 for resolution <= 0 or count <= 0.  The _batch form runs `count` tiles stored back to back, each with its
 * own border and its own labels; every batch position equals the single-tile call bit for bit, and the status words cover
 * the whole batch.  resolution == 0 or count == 0 does nothing and returns NZ_OK.  The 16-byte path runs when every plane is
 * 16-byte aligned (the receiver bytes 4-byte) and resolution % 4 == 0, the 4-byte path otherwise; both give the same bits.
 * Refused with NZ_ERR_INVALID, the message naming the argument and nothing written: a NULL desc, height, basin or work;
 * cellSize not finite or not > 0; a NaN seaLevel (-FLT_MAX switches the sea off); maxPasses < 1; count * resolution^2
 * beyond int32; basin, length, receivers or work overlapping height or each other.
 * A row-stripe form is not built yet. */
typedef struct nz_watershed_desc {
    float seaLevel, cellSize;
    int32_t maxPasses;
} nz_watershed_desc;
size_t nz_watershed_work_floats(int32_t resolution, int32_t count, int32_t withLength);
int32_t nz_watershed(nz_ctx *ctx, const float *height, int32_t *basin, float *length, uint8_t *receivers, float *work,
                     const nz_watershed_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out);
int32_t nz_watershed_batch(nz_ctx *ctx, const float *height, int32_t *basin, float *length, uint8_t *receivers, float *work,
                           const nz_watershed_desc *desc, int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);
/* Test hook, the twin of nz_debug_drainage_sweeps: the cap on a watershed pass's on-chip sweeps per tile (process-wide;
 * <= 0 restores the default, 16).  Results must not change.  Returns the cap that was in force. */
int32_t nz_debug_watershed_sweeps(int32_t sweeps);

/* ---- stream order: Strahler order and river links of a heightmap (new-framework feature) ----------------------------
 * The last product of a river-network extraction: which cells are channel, how big each channel is as a class (Strahler
 * order: brook, stream, river) and which cells form one unbranched reach, a link, that can become one polyline, one width,
 * one spline.  Feed it a filled tile (nz_fill_depressions) and the plane nz_drainage_area wrote, with a threshold.
 *
 * THE MODEL (tests/stream_order_ref.py restates it as a walk highest cell first; the kernels are nz_stream_order.hip):
 *   Square tile res x res, row-major c = z * res + x, float32 heights, read only.  Outlets, the neighbour order
 *   W E S N SW SE NW NE, "a neighbour outside the tile does not exist" and the receiver r(c) with its strict comparison and
 *   tie rule are exactly step 1 of the fluvial model above: border cells and cells <= seaLevel have no receiver.  The same
 *   in every float mode (nz_ctx_set_float_mode does not apply).
 *   ch(c), the channel predicate: drainage == NULL ? true : drainage[c] >= threshold -- one float32 comparison, so a NaN is
 *   not a channel; static, read once, and nothing else decides it.  A sea or border cell is a channel cell like any other
 *   when its drainage says so, so a river keeps its order at its mouth.
 *   D(c): the existing neighbours k of c with r(k) == c and ch(k).
 *   order[c] (uint8):  !ch(c): 0;  D(c) empty: 1;  otherwise, with m = max order[D(c)] and n = #{d in D(c) : order[d] == m},
 *     order[c] = m + (n >= 2 ? 1 : 0).
 *   link[c] (int32, optional plane):  !ch(c): -1;  |D(c)| != 1: c, a channel head or a confluence: a link starts here;
 *     otherwise link[d] of the one donor.  In a batch c is the index inside the cell's own tile.
 * A receiver is strictly lower than its donor, so the graph is a forest, every value is a fixed function of the donors'
 * final values and the fixed point is unique: a walk highest cell first, Jacobi and tile-local sweeps end in the same
 * bytes.  Order w needs at least 2^(w-1) channel heads upstream; the entries refuse count * resolution^2 >= 2^31, so
 * order <= 31 and a byte never saturates.  The start state, and the "nothing" of all or nothing: order = ch ? 1 : 0,
 * link = ch ? c : -1.  What follows:
 *   - order > 0 <=> ch <=> link >= 0, and order never falls along a receiver step between channel cells;
 *   - link[link[c]] == link[c], and the distinct links are exactly the channel cells with |D| != 1;
 *   - without `drainage`, order[c] <= 1 + floor(log2(A[c])) for A the rain-1 nz_drainage_area.
 * `link` is optional (NULL): an order-only call carries no 4-byte plane at all.
 *
 * The entry enqueues one mask launch (heights and drainage -> one channel-donor byte per cell into `work`, the start state
 * into `order`), maxPasses pass launches and one finalise launch, stream-ordered; nothing is read back.  A pass is
 * nz_drainage_area's scheme on small integers, max and count in place of a float sum: every 64 x 16 tile is swept on chip
 * against its frozen ring; tiles whose neighbourhood was at rest in the pass before are skipped, and a launch returns at
 * once when the pass before changed nothing.  After completion the first two int32 of `work` hold {passes that did work,
 * converged 0/1}.  The result is ALL OR NOTHING: when the last pass that ran changed nothing, `order` and `link` hold the
 * fixed point; otherwise -- the budget was too small -- they hold the start state and converged == 0, which is not an
 * error.  A pass is at least one Jacobi step, so a budget of "cells of the longest chain of channel donors" + 2 always
 * suffices; the hosts' default is far below that and measured ("stream order").
 * Defaults of the hosts' StreamOrderStage: seaLevel -FLT_MAX (off), threshold 0, maxPasses 64 + resolution / 4, without
 * drainage, without links.
 * The evidence (tools/bench_stream_order.py): the 13-octave simplex fBm tile behind
 * nz_fill_depressions, with the plane of nz_drainage_area and threshold 100, comes to rest in 59 passes at 1024^2 and 94 at
 * 4096^2 (51 and 88 without a drainage plane), where nz_drainage_area takes 82 and 192; the defaults allow 320 and 1088.
 * Not a bound: a channel that winds through many tiles needs more, and a budget that runs out shows as converged == 0.
 *
 * `work` = nz_stream_order_work_floats(resolution, count, withLinks) floats, stage-owned, any withLinks != 0 counting as 1,
 * for a call with a `link` plane: status words, tile bytes, one channel-donor byte per cell, the second `order` plane and,
 * with links, the second `link` plane (the first of each pair is the caller's).  0 for resolution <= 0 or count <= 0.  The
 * _batch form runs `count` tiles stored back to back, each with its own border and its own link indices; every batch
 * position equals the single-tile call bit for bit, and the status words cover the whole batch.  resolution == 0 or
 * count == 0 does nothing and returns NZ_OK.  The wide path runs when resolution % 4 == 0, the byte planes are 4-byte
 * aligned and height, drainage and link 16-byte aligned, the narrow path otherwise; both give the same bytes.
 * Refused with NZ_ERR_INVALID, the message naming the argument and nothing written: a NULL desc, height, order or work;
 * threshold not finite; a NaN seaLevel (-FLT_MAX switches the sea off); maxPasses < 1; count * resolution^2 beyond int32;
 * order, link or work overlapping height, drainage or each other.
 * A row-stripe form is not built; Strahler streams, as opposed to links, are the host's to derive
 * from `order` and `link`. */
typedef struct nz_stream_order_desc {
    float seaLevel, threshold;
    int32_t maxPasses;
    const float *drainage;   /* NULL: every cell is a channel cell, threshold is not compared */
} nz_stream_order_desc;
size_t nz_stream_order_work_floats(int32_t resolution, int32_t count, int32_t withLinks);
int32_t nz_stream_order(nz_ctx *ctx, const float *height, uint8_t *order, int32_t *link, float *work,
                        const nz_stream_order_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out);
int32_t nz_stream_order_batch(nz_ctx *ctx, const float *height, uint8_t *order, int32_t *link, float *work,
                              const nz_stream_order_desc *desc, int32_t resolution, int32_t count, nz_handle dep,
                              nz_handle *out);
/* Test hook, the twin of nz_debug_watershed_sweeps: the cap on a stream-order pass's on-chip sweeps per tile
 * (process-wide; <= 0 restores the default, 16).  Results must not change.  Returns the cap that was in force. */
int32_t nz_debug_stream_order_sweeps(int32_t sweeps);

/* ---- implicit fluvial erosion: a large time step of the stream-power model in one solve (new-framework feature) ---------
 * nz_fluvial_erosion above is the explicit scheme: one small step per launch, a drainage plane that is a transient, and a
 * half-drop limiter in place of a stability bound.  The model is linear in the slope, so the implicit Euler step has a
 * closed form along the receiver tree (the FastScape scheme, Braun & Willett 2013): stable for every dt, and one call
 * carries "10 000 years".  Its drainage input is the exact plane nz_drainage_area delivers in one call.
 *
 * THE MODEL (tests/fluvial_implicit_ref.py restates it as a walk lowest cell first; the kernels are
 * nz_fluvial_implicit.hip):
 *   Square tile res x res, row-major c = z * res + x, float32 throughout, no contraction, the same in every float mode
 *   (nz_ctx_set_float_mode does not apply).  Outlets, the neighbour order W E S N SW SE NW NE, "a neighbour outside the
 *   tile does not exist" and the receiver r(c) with its strict comparison and tie rule are exactly step 1 of the fluvial
 *   model above.  Inputs, all read only: heights h, a drainage plane A (required; e.g. nz_drainage_area on the same
 *   heights) and the optional planes hardness and upliftMap as in nz_fluvial_desc.  Per cell:
 *     du = dt * uplift (one product; with a map du * upliftMap[c]);  kc = erodibility * (1 - hardness[c]) (without a map
 *     erodibility);
 *     outlet (global border or h <= seaLevel):  h'[c] = h[c];
 *     pit (interior, no receiver):              h'[c] = h[c] + du;
 *     otherwise, with q the cell r(c) = k names:
 *       b = h[c] + du,   f = ((kc * sqrt(A[c])) * invL_k) * dt,   invL_k = 1 for k < 4 and 0x1.6a09e6p-1f for k >= 4,
 *       h'[c] = (b + f * h'[q]) / (1 + f)
 *     each operation rounded once, in that order: product, sum, sum, one correctly rounded float32 division; sqrt is
 *     correctly rounded as in nz_fluvial_erosion.
 * A receiver is strictly lower than its donor, so the graph is a forest whose roots, the outlets and pits, are fixed from
 * the start; a cell's new height is a fixed function of the new height of one other cell, so the fixed point is unique: a
 * walk lowest cell first, Jacobi and tile sweeps end in the same bits, from any start state (the kernels start from b).
 * The "nothing" of all or nothing is h' = h.  What follows:
 *   - erodibility == 0 gives h + du off the outlets;
 *   - outlets keep their bits;
 *   - in exact arithmetic and without an upliftMap, h'[q] <= h'[c] <= h[c] + du: no cell rises above its uplifted height
 *     or sinks below its receiver.  In float32 rounding can decide otherwise on tiles of tiny or equal heights.
 * Say it plainly: an f that overflows (erodibility * sqrt(A) * dt beyond FLT_MAX) gives inf / inf = NaN in that cell and
 * in every cell upstream of it; A must be finite and >= 0 (sqrt of a negative is NaN, and NaN travels upstream the same
 * way); and pits stay pits -- a pit only rises by du and everything that drains to it is pulled towards it -- so put
 * nz_fill_depressions (DepressionFillStage) in front.
 *
 * The entry enqueues one begin launch (a single thread), one setup launch (heights at radius 1, A and the maps -> one
 * receiver byte and the coefficients b and f per cell, into `work`), maxPasses pass launches and one finalise launch,
 * stream-ordered; nothing is read back.  After the setup launch no pass looks at a height, A or a map.  A pass is
 * nz_watershed's scheme with a float recurrence in place of the label copy: every 64 x 16 tile is swept on chip against
 * its frozen ring, each cell reading the one cell its code names; tiles whose neighbourhood was at rest in the pass before
 * are skipped, and a launch returns at once when the pass before changed nothing.  After completion the first two int32 of
 * `work` hold {passes that did work, converged 0/1}.  The result is ALL OR NOTHING: when the last pass that ran changed
 * nothing, `out` holds the fixed point; otherwise -- the budget was too small -- out = h bit for bit and converged == 0,
 * which is not an error.  A pass is at least one Jacobi step, so a budget of "moves of the longest flow path" + 2 always
 * suffices.  Defaults of the hosts' ImplicitFluvialStage: iterations 1, erodibility 0.05, uplift 0.002, dt 1, rain 1,
 * seaLevel -FLT_MAX (off), maxPasses 64 + resolution / 4 for the drainage and for the solve, no maps.
 * The evidence (tools/bench_fluvial_implicit.py): the 13-octave simplex fBm tile behind
 * nz_fill_depressions comes to rest in 23 passes at dt 1 and 82 at dt 100 at 1024^2, in 62 and 192 at 4096^2; the passes
 * grow with dt up to those of nz_drainage_area and nz_watershed on the same tile (82 and 192: at a large f a cell follows
 * its receiver to the last bit, as a label does), and the defaults allow 320 and 1088.  Not a bound: a path that winds
 * through many tiles needs more, and a budget that runs out shows as converged == 0.
 *
 * `proceed` (device, optional) lets a host chain nz_drainage_area -> this entry without reading anything back: pass the
 * address of the drainage call's converged word (the second int32 of its `work`).  The begin launch reads the word when it
 * runs; with a zero word every launch of the call returns at once, out = h, the status is {0, 0} and `tally` is untouched.
 * `tally` (device, two int32, optional): the finalise launch adds 1 to tally[0] when the step was applied and the passes
 * that did work to tally[1]; calls on one context are ordered by its stream, so a host sums a series of steps there.
 *
 * `work` = nz_fluvial_implicit_work_floats(resolution, count) floats, stage-owned: status words, tile bytes, the receiver
 * bytes, the planes b and f and the second h' plane (the first is `out`).  0 for resolution <= 0 or count <= 0.  The _batch
 * form runs `count` tiles stored back to back, each with its own border; every batch position equals the single-tile call
 * bit for bit, and the status words cover the whole batch.  resolution == 0 or count == 0 does nothing and returns NZ_OK.
 * The 16-byte path runs when every plane is 16-byte aligned and resolution % 4 == 0, the 4-byte path otherwise; both give
 * the same bits.
 * Refused with NZ_ERR_INVALID, the message naming the argument and nothing written: a NULL desc, height, drainage, out or
 * work; erodibility, uplift, dt or seaLevel not finite (-FLT_MAX switches the sea off); erodibility, uplift or dt < 0;
 * maxPasses < 1; count * resolution^2 beyond int32; out or work overlapping height, drainage, a map or each other (`out`
 * must not be `height`: the solve is not in place); tally overlapping a plane or proceed; proceed inside out or work.
 * The row-stripe form is nz_implicit_fluvial_stripe_round / _finalise, below; there is no _rw pair form (DESIGN.md
 * section 9). */
typedef struct nz_fluvial_implicit_desc {
    float erodibility, uplift, dt, seaLevel;
    int32_t maxPasses;
    const float *hardness;    /* NULL: erodibility everywhere */
    const float *upliftMap;   /* NULL: uplift everywhere */
    const int32_t *proceed;   /* device word, NULL: always run; a word of 0: the step is not applied */
    int32_t *tally;           /* device, 2 words, NULL: off; tally[0] += 1 when the step was applied, tally[1] += passes that did work */
} nz_fluvial_implicit_desc;
size_t nz_fluvial_implicit_work_floats(int32_t resolution, int32_t count);
int32_t nz_fluvial_implicit(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                            const nz_fluvial_implicit_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out_handle);
int32_t nz_fluvial_implicit_batch(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                                  const nz_fluvial_implicit_desc *desc, int32_t resolution, int32_t count, nz_handle dep,
                                  nz_handle *out_handle);
/* Test hook, the twin of nz_debug_watershed_sweeps: the cap on an implicit-fluvial pass's on-chip sweeps per tile
 * (process-wide; <= 0 restores the default, 16).  Results must not change.  Returns the cap that was in force. */
int32_t nz_debug_fluvial_implicit_sweeps(int32_t sweeps);
/* The same model on a row stripe of a larger grid (nz_stripe), one ROUND per call, in the wording of
 * nz_drainage_stripe_round.  The receiver graph is a forest whose roots are fixed and a cell's h' is a fixed function of one
 * other cell's h', so rounds of per-stripe relaxation against one frozen ghost row of h' on each side, with one row of
 * `out` exchanged between them, reach the monolithic plane bit for bit, from any start state.  All planes have the stripe's
 * shape and pitch, `drainage`, desc->hardness and desc->upliftMap included; grids may be rectangular.
 *   (The four entries carry the hosts' word order, nz_implicit_fluvial_stripe_*, after ImplicitFluvialStripe: the prefix
 *   nz_fluvial_implicit_ stays that of the tile and batch entries, the test hook and the desc.)
 *   nz_implicit_fluvial_stripe_round runs at most desc->maxPasses passes of the tile entry's pass (the sweep cap
 *     nz_debug_fluvial_implicit_sweeps included) over the owned rows; the first pass of a round starts a fresh series and
 *     visits every tile, because the ghost rows may have changed.  The one ghost row of `out` on each side is FROZEN: read,
 *     never written, whichever plane a pass alternates to.  Outlets, and neighbours that do not exist, follow the GLOBAL grid
 *     (global rows 0 and grows-1, columns 0 and cols-1; h <= seaLevel); a cut is no border.  Rows beyond the ghost row are
 *     neither read nor written, nor are the floats between cols and pitch.
 *   first != 0: a stripe form of the setup launch stores, for the owned rows only, the receiver byte, b and f into `work`.
 *     The heights are read at radius 1, so `height` needs ONE valid ghost row towards every cut; `drainage`, hardness and
 *     upliftMap are read on the owned rows only.  `out` is not read: the start state is b on the owned rows, and the frozen
 *     rows are the ghost rows of `height` as they stand (any start gives the same fixed point, and this needs no ghost row
 *     of the maps).  `changed` receives 1.
 *   first == 0: `height`, `drainage` and the maps are not read; `work` must be the buffer of the round before, untouched in
 *     between (it carries the receiver bytes and the coefficients); the current h' is read from `out`, whose ghost rows the
 *     caller has exchanged.  `changed` (device) receives 1 if any single update of any pass of the round changed a bit, a
 *     budget that ran out before rest included; 0 only when the round's first pass found every owned cell at rest against
 *     the ghost rows.
 *   On return the owned rows of `out` hold the stripe's h', whatever the parity of the passes that ran.
 *   proceed (device, may be NULL): a word of zero makes every launch of the call return at once -- `out` untouched,
 *     `changed` 0 -- so that a host can enqueue a fixed budget of rounds without reading anything back.  desc->proceed and
 *     desc->tally must be NULL here: the round's own argument and the driver take their place.
 *   `work` = nz_implicit_fluvial_stripe_work_floats(st) floats, the tile entry's layout over the stripe's plane: status
 *     words and tile bytes (over the owned rows), the receiver bytes, b, f, a second h' plane.
 *   nz_implicit_fluvial_stripe_finalise, on the owned rows: where *converged != 0, `out` stays; otherwise out = height bit
 *     for bit -- all or nothing, as in the tile entry.  `converged` is the caller's verdict: the vote over all ranks after
 *     the last round was 0 (nz_comm_allreduce_max_i32).
 *   One stripe over a square grid with `first`, a second round whose `changed` is 0, then finalise with a word of 1, equals
 *     nz_fluvial_implicit bit for bit, on the 16-byte path (all planes 16-byte aligned, pitch % 4 == 0) and the 4-byte one.
 * NZ_ERR_INVALID, the message naming the argument, and nothing written: everything nz_fluvial_implicit refuses; a non-NULL
 * desc->proceed or desc->tally; a missing ghost row; a NULL plane or word; out, work, the read planes or the two words
 * overlapping where one of them is written. */
int32_t nz_implicit_fluvial_stripe_halo_rows(void); /* 1: the heights, and `out` between rounds */
size_t nz_implicit_fluvial_stripe_work_floats(const nz_stripe *st);
int32_t nz_implicit_fluvial_stripe_round(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                                         const nz_stripe *st, const nz_fluvial_implicit_desc *desc, int32_t first,
                                         const int32_t *proceed, int32_t *changed, nz_handle dep, nz_handle *out_handle);
int32_t nz_implicit_fluvial_stripe_finalise(nz_ctx *ctx, const float *height, float *out, const nz_stripe *st,
                                            const int32_t *converged, nz_handle dep, nz_handle *out_handle);

/* ---- hillslope diffusion: dh/dt = kappa * laplace(h) in one implicit step of any size (new-framework feature) ------------
 * The second term of every landscape-evolution model beside stream power (FastScape pairs the two): linear diffusion rounds
 * the knife-edge ridges and one-cell gullies the fluvial solve leaves.  An explicit step is unstable above kappa * dt = 1/4;
 * this entry is a direct solve, stable and free of oscillation for every dt, with no pass budget and no verdict.
 *
 * THE MODEL (tests/hillslope_ref.py restates it in numpy; the kernels are nz_hillslope.hip):
 *   Square tile res x res, row-major c = z * res + x, float32 throughout, every operation rounded once, no contraction, the
 *   same in every float mode (nz_ctx_set_float_mode does not apply).  The scheme is backward Euler split by direction,
 *   (I - r Lx)(I - r Lz) h' = h, with the border cells held (Dirichlet): they keep their bits -- they are the outlets of the
 *   fluvial stages.  The amplification 1 / ((1 + r lx)(1 + r lz)) is positive for every r, so nothing oscillates at a large
 *   dt; this is why the scheme is not Peaceman-Rachford, which tends to -1 there.
 *   Coefficients, shared by every line:  r = diffusivity * dt (one product),  B = 1 + 2 * r.
 *   Tables for i = 1 .. res-2:  den_1 = B,  den_i = B - r * cp_{i-1},  inv_i = 1 / den_i (a correctly rounded division),
 *                               cp_i = r * inv_i.
 *   One line solve over the values v_0 .. v_{n-1}:
 *     p_0 = v_0;          p_i = (v_i + r * p_{i-1}) * inv_i   for i = 1 .. n-2;
 *     x_{n-1} = v_{n-1};  x_i = p_i + cp_i * x_{i+1}          for i = n-2 .. 1;     x_0 = v_0.
 *   One step is two half-steps: half-step X solves every row z = 1 .. res-2 along x (rows 0 and res-1 are copied), half-step
 *   Z solves every column x = 1 .. res-2 of that result along z.  `iterations` steps are applied one after another with the
 *   same tables.  What follows:
 *   - res < 3 gives out = h;
 *   - r == 0 gives out = h bit for bit, by definition: it does not go through the recurrence, which would flip the sign of a
 *     -0.0;
 *   - border cells keep their bits;
 *   - in exact arithmetic the result stays within the input's minimum and maximum;
 *   - a NaN or inf in a line spreads along that line and then across it.
 * Defaults of the hosts' HillslopeDiffusionStage: diffusivity 0.01, dt 1, iterations 1 -- a choice, not pinned by any
 * picture.  The evolution loop is [DepressionFillStage, ImplicitFluvialStage(dt=T), HillslopeDiffusionStage(dt=T)], repeated.
 *
 * The entry enqueues one table launch (inv and cp into `work`, on the device: no host buffer whose lifetime the entry would
 * have to manage) and per step three launches -- the rows' forward sweep, the rows' backward sweep, the columns' two sweeps
 * -- stream-ordered; nothing is read back and there are no status words.  p lives in `out`, so `work` holds only the tables:
 * nz_hillslope_diffusion_work_floats(resolution, count) floats (0 for resolution <= 0 or count <= 0; the tables are shared
 * by the tiles of a batch).  out == height, the same pointer, means in place and is allowed; otherwise the two planes must be
 * disjoint.  The _batch form runs `count` tiles stored back to back, each with its own border; every batch position equals
 * the single-tile call bit for bit.  resolution == 0 or count == 0 does nothing and returns NZ_OK.  The 16-byte path runs
 * when every plane is 16-byte aligned and resolution % 4 == 0, the 4-byte path otherwise; both give the same bits.
 * Refused with NZ_ERR_INVALID, the message naming the argument and nothing written: a NULL desc, height, out or work;
 * diffusivity or dt not finite or < 0; r or 1 + 2 r not finite; iterations < 1; count * resolution^2 beyond int32; out partly
 * overlapping height; work overlapping either plane.
 * No sea-level cells are held, there is no per-cell diffusivity map (either would break the shared tables) and there is no
 * row-stripe form. */
typedef struct nz_hillslope_desc {
    float diffusivity, dt;
    int32_t iterations;
} nz_hillslope_desc;
size_t nz_hillslope_diffusion_work_floats(int32_t resolution, int32_t count);
int32_t nz_hillslope_diffusion(nz_ctx *ctx, const float *height, float *out, float *work, const nz_hillslope_desc *desc,
                               int32_t resolution, nz_handle dep, nz_handle *out_handle);
int32_t nz_hillslope_diffusion_batch(nz_ctx *ctx, const float *height, float *out, float *work, const nz_hillslope_desc *desc,
                                     int32_t resolution, int32_t count, nz_handle dep, nz_handle *out_handle);

/* ---- multiple-flow implicit fluvial erosion: the implicit step along every descent (new-framework feature) ---------------
 * nz_fluvial_implicit above lowers each cell along its ONE steepest receiver, whatever plane A it is given: behind
 * nz_drainage_mfd the water is spread over a fan and then cut into eight-direction grooves.  This entry takes the implicit
 * Euler step of the same stream-power law along EVERY lower neighbour, with nz_drainage_mfd's weights: the step that goes
 * with that drainage plane (fastscapelib solves its multiple-flow stream power the same way).
 *
 * THE MODEL (tests/fluvial_implicit_mfd_ref.py restates it as a walk lowest cell first; the kernels are
 * nz_fluvial_implicit_mfd.hip):
 *   Square tile res x res, row-major c = z * res + x, float32 throughout, every operation rounded once, no contraction, the
 *   same in every float mode (nz_ctx_set_float_mode does not apply).  Outlets, the neighbour order W E S N SW SE NW NE,
 *   DIAG, du, kc and b are exactly nz_fluvial_implicit's; the outgoing weights w_k of a cell are exactly nz_drainage_mfd's
 *   at `exponent` (1..16) -- the same device code.  Inputs, all read only: heights h, a drainage plane A (required; e.g.
 *   nz_drainage_mfd on the same heights with the same exponent) and the optional planes hardness and upliftMap.  Per cell c:
 *     outlet (global border or h <= seaLevel):  h'[c] = h[c];
 *     no k with w_k > 0 (a pit, a flat):        h'[c] = b = h[c] + du     (not through the division);
 *     otherwise:  e = kc * sqrt(A[c]);
 *                 f_k = ((e * invL_k) * dt) * w_k   for every k with w_k > 0, invL_k = 1 for k < 4 and 0x1.6a09e6p-1f else;
 *                 N = b;  D = 1;  for k ascending with w_k > 0:  N = N + (f_k * h'[k]);  D = D + f_k;
 *                 h'[c] = N / D                     one correctly rounded float32 division.
 *   The gate is w_k > 0, never the value of f_k or of h'.
 * Every neighbour that takes flow is strictly lower in the old heights, so the flow graph is a DAG whose leaves -- outlets,
 * pits, flats -- are fixed from the start; a cell's new height is a fixed function of the new heights of lower cells, so
 * the fixed point is unique: a walk lowest cell first, Jacobi and tile sweeps end in the same bits, from any start state
 * (the kernels start from b).  The "nothing" of all or nothing is h' = h.  What follows:
 *   - a cell with exactly one positive weight has w == 1 and takes nz_fluvial_implicit's value bit for bit, given the same
 *     A and an equal h' below it;
 *   - erodibility == 0 gives h + du off the outlets;
 *   - outlets keep their bits;
 *   - in exact arithmetic and without an upliftMap, min_k h'[k] <= h'[c] <= h[c] + du over the k with w_k > 0: no cell
 *     rises above its uplifted height or sinks below the lowest cell it drains to.  In float32 rounding can decide
 *     otherwise on tiles of tiny or equal heights;
 *   - NaN heights send and receive nothing (HEIGHT DIFFERENCES MUST BE FINITE, as for nz_drainage_mfd); a NaN or negative
 *     A gives a NaN in that cell and travels upstream, as in nz_fluvial_implicit.
 * Say it plainly: an f that overflows gives inf / inf = NaN in that cell and in every cell upstream of it; and pits stay
 * pits, so put nz_fill_depressions (DepressionFillStage) in front.
 *
 * The entry enqueues nz_fluvial_implicit's begin launch, one setup launch (heights at radius 1, A and the maps -> one gate
 * byte, bit k: w_k > 0, the plane b and the eight planes f_k per cell, +0 where w_k is not > 0, into `work`; every square
 * root and every weight division is here), maxPasses pass launches and nz_fluvial_implicit's finalise launch,
 * stream-ordered; nothing is read back.  After the setup launch no pass looks at a height, A or a map.  A pass is
 * nz_drainage_mfd's gather with h' in place of A, closed by the division; D is rebuilt from the f in registers, not stored.
 * After completion the first two int32 of `work` hold {passes that did work, converged 0/1}.  The result is ALL OR NOTHING:
 * when the last pass that ran changed nothing, `out` holds the fixed point; otherwise -- the budget was too small --
 * out = h bit for bit and converged == 0, which is not an error.  A pass is at least one Jacobi step, so a budget of
 * "cells of the longest path of the flow DAG" + 2 always suffices.  Defaults of the hosts' MfdFluvialStage: iterations 1,
 * erodibility 0.05, uplift 0.002, dt 1, rain 1, seaLevel -FLT_MAX (off), exponent 1, maxPasses 128 + resolution / 2 for
 * the drainage and for the solve, no maps.
 *
 * `proceed`, `tally`, the status words, the zero-size behaviour and the batch form are nz_fluvial_implicit's word for word;
 * `proceed` takes the converged word of nz_drainage_mfd (the second int32 of its `work`) as it takes nz_drainage_area's.
 * `work` = nz_fluvial_implicit_mfd_work_floats(resolution, count) floats, stage-owned: status words, tile bytes, the gate
 * bytes, the plane b, the eight planes f and the second h' plane (the first is `out`).  0 for resolution <= 0 or count <= 0.
 * The 16-byte path runs when every plane is 16-byte aligned and resolution % 4 == 0, the 4-byte path otherwise; both give
 * the same bits.
 * Refused with NZ_ERR_INVALID, the message naming the argument and nothing written: everything nz_fluvial_implicit
 * refuses, and exponent outside 1..16.
 * There is no row-stripe form and no _rw form. */
typedef struct nz_fluvial_implicit_mfd_desc {
    float erodibility, uplift, dt, seaLevel;
    int32_t maxPasses;
    int32_t exponent;         /* 1..16, nz_drainage_mfd_desc.exponent */
    const float *hardness;    /* NULL: erodibility everywhere */
    const float *upliftMap;   /* NULL: uplift everywhere */
    const int32_t *proceed;   /* device word, NULL: always run; a word of 0: the step is not applied */
    int32_t *tally;           /* device, 2 words, NULL: off; tally[0] += 1 when the step was applied, tally[1] += passes that did work */
} nz_fluvial_implicit_mfd_desc;
size_t nz_fluvial_implicit_mfd_work_floats(int32_t resolution, int32_t count);
int32_t nz_fluvial_implicit_mfd(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                                const nz_fluvial_implicit_mfd_desc *desc, int32_t resolution, nz_handle dep,
                                nz_handle *out_handle);
int32_t nz_fluvial_implicit_mfd_batch(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                                      const nz_fluvial_implicit_mfd_desc *desc, int32_t resolution, int32_t count,
                                      nz_handle dep, nz_handle *out_handle);
/* Test hook, the twin of nz_debug_fluvial_implicit_sweeps with a cap of its own: the cap on a multiple-flow implicit pass's
 * on-chip sweeps per tile (process-wide; <= 0 restores the default, 16).  Results must not change.  Returns the cap that
 * was in force. */
int32_t nz_debug_fluvial_implicit_mfd_sweeps(int32_t sweeps);

/* ---- implicit fluvial erosion with sediment deposition: the xi-q model (new-framework feature) --------------------------
 * nz_fluvial_implicit is detachment-limited: eroded material leaves the tile, valleys cut and never aggrade.  This entry
 * adds the deposition term of Yuan, Braun, Guerit, Rouby & Cordonnier (2019), the one fastscape's StreamPowerLaw has: what
 * the cells upstream gave up comes down the receiver tree as a sediment flux Q, and a cell takes G * Qin / A of it back.
 * The term sits in the right-hand side of nz_fluvial_implicit's solve, and K Gauss-Seidel iterations bring flux and heights
 * to agree.
 *
 * THE MODEL (tests/fluvial_sediment_ref.py restates it as walks; the kernels are nz_fluvial_sediment.hip):
 *   Tile, neighbours, outlets, receivers r(c), du, kc, b0 = b, f and invL are exactly nz_fluvial_implicit's; A is the
 *   caller's drainage plane; G = deposition >= 0, dimensionless; K = iterations >= 0.  Every operation is rounded once to
 *   float32, no contraction, divisions correctly rounded.  solve(b) is nz_fluvial_implicit's recurrence with right-hand
 *   side b: a cell without a receiver takes h' = b, otherwise h' = (b + f * h'[q]) / (1 + f).
 *     h0 = solve(b0)                                   -- nz_fluvial_implicit's result bit for bit
 *     for k = 1 .. K:
 *       e[c]   = b0[c] - h(k-1)[c]                     -- what the cell gave up this step, uplift included; +0 on outlets,
 *                                                         may be negative
 *       Q[c]   = e[c] + Q[d] over the donors d of c, added one by one onto e[c] in neighbour order 0..7 -- the drainage
 *                recurrence of nz_drainage_area with a signed per-cell source
 *       Qin[c] = the same gather of the final Q started from +0 (the flux entering the cell, its own share excluded),
 *                then Qin < 0 ? +0 : Qin; a NaN passes
 *       bk[c]  = b0[c] on outlets; elsewhere, pits included, b0[c] + (G * Qin[c]) / A[c] where A[c] > 0 and b0[c] where not
 *       hk     = solve(bk)
 *     out = hK;  residual = max over c of |hK[c] - h(K-1)[c]|, taken with d > m so a NaN cell does not enter, +0 when
 *     K == 0: how far the iteration still was from rest.  flux (optional plane) = the Q of iteration K, +0 when K == 0: the
 *     sediment-flux map.
 *   Q is a fixed function of the final values of strictly higher cells and a solve of strictly lower ones, so both fixed
 *   points are unique and every schedule ends in the same bits.  Every operation of solve is monotone in b and bk >= b0, so
 *   hK >= h0 cell by cell where neither is NaN.  deposition == 0 or iterations == 0 gives nz_fluvial_implicit's plane bit
 *   for bit.
 * THE LIMITS, plainly.  The iteration is a contraction for G up to about 1, slower as G * dt grows: on a filled 97^2 tile
 *   at dt 100 the residual falls by 3.5 per iteration at G 0.5 and by 1.75 at G 1, and at G 2 with a large dt it stalls
 *   (DESIGN.md sections 4 and 9) -- read `residual`.  Receivers, f and A are those of the INCOMING heights for the whole
 *   call, as in nz_fluvial_implicit: deposition may lift a cell above a donor, the next step's receivers see that, and
 *   nz_fill_depressions (DepressionFillStage) belongs in front as before.  There is no lake trapping: a pit takes the same
 *   deposit term as any cell.  The multiple-flow solve (nz_fluvial_implicit_mfd) has no sediment form.
 *
 * The entry enqueues, without waiting for the device: a begin launch; nz_fluvial_implicit's setup launch and one donor-byte
 * launch (nz_drainage_area's mask), once per call; solve series 0 (maxPasses launches of nz_fluvial_implicit's pass); per k
 * a source launch (e, a fresh series), an accumulation series of maxPasses pass launches (nz_drainage_area's gather with
 * source e, quiet tiles skipped), a deposit launch (Qin at radius 1 from the final Q, bk) and a solve series of maxPasses
 * launches on bk; and the finalise launch.  A series at rest lets its remaining launches return at the gate, and a series
 * that did not come to rest stops every launch behind it.  After completion the first three words of `work` hold {passes
 * that did work over all series, converged 0/1, residual as float bits}.  The result is ALL OR NOTHING: when any of the
 * 2K + 1 series did not come to rest within maxPasses, or the call was told not to proceed, out = height bit for bit, `flux`
 * is untouched, converged == 0 and residual == +0.  `proceed` and `tally` are nz_fluvial_implicit's; tally[1] grows by the
 * passes of all series.
 *
 * `work` = nz_fluvial_sediment_work_floats(resolution, count) floats, stage-owned (seven planes and two bytes per cell).
 * resolution == 0 or count == 0 does nothing and returns NZ_OK; the _batch form runs `count` tiles stored back to back, each
 * position equal to the single-tile call bit for bit, with status words and residual over the whole batch.  The 16-byte
 * path runs when every plane is 16-byte aligned and resolution % 4 == 0, the 4-byte path otherwise.  Neither an
 * _rw pair form nor a row-stripe form exists.
 * Refused with NZ_ERR_INVALID, the message naming the argument and nothing written: everything nz_fluvial_implicit
 * refuses; deposition negative or not finite; iterations < 0; flux overlapping out, work, height, drainage, a map, tally or
 * proceed.
 * Defaults of the hosts' SedimentFluvialStage: ImplicitFluvialStage's, deposition 0.5, sedimentIterations 4 (the smallest
 * K whose residual is <= 1 % of max |b0 - h0| on the filled 97^2 test tile at dt 100: DESIGN.md section 4), recordFlux
 * off. */
typedef struct nz_fluvial_sediment_desc {
    float erodibility, uplift, dt, seaLevel;
    int32_t maxPasses;        /* the budget of each of the 2K + 1 series */
    const float *hardness;    /* NULL: erodibility everywhere */
    const float *upliftMap;   /* NULL: uplift everywhere */
    const int32_t *proceed;   /* device word, NULL: always run; a word of 0: the step is not applied */
    int32_t *tally;           /* device, 2 words, NULL: off; tally[0] += 1 when the step was applied, tally[1] += passes that did work */
    float deposition;         /* G >= 0 */
    int32_t iterations;       /* K >= 0 */
    float *flux;              /* device plane, NULL: off; the Q of iteration K */
} nz_fluvial_sediment_desc;
size_t nz_fluvial_sediment_work_floats(int32_t resolution, int32_t count);
int32_t nz_fluvial_sediment(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                            const nz_fluvial_sediment_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out_handle);
int32_t nz_fluvial_sediment_batch(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work,
                                  const nz_fluvial_sediment_desc *desc, int32_t resolution, int32_t count, nz_handle dep,
                                  nz_handle *out_handle);
/* Test hook, the twin of nz_debug_fluvial_implicit_sweeps with a cap of its own: one cap on the on-chip sweeps per tile of
 * both kinds of series, solve and accumulation (process-wide; <= 0 restores the default, 16).  Results must not change.
 * Returns the cap that was in force. */
int32_t nz_debug_fluvial_sediment_sweeps(int32_t sweeps);

/* ---- the stock stage list as a parameter block --------------------------------------------------------------------
 * NoiseStage -> [KernelFilterStage] -> [FlowMapStage] -> [ErosionKernelJob x n] (README.md:23-32, the metric pipeline) as
 * nz_sharded_create takes it; an iteration count of 0 leaves a stage out.  (Rounds 3 and 4 also offered the list as ONE call
 * on a single tile, nz_terrain_pipeline: two row stripes on two streams of the context.  With the round-3 kernels the
 * overlap bought nothing -- 0.6595 against 0.6413 ms per 4096^2 step stage by stage -- and it was removed in round 5.) */
typedef struct nz_terrain_params {
    int32_t noiseType;            /* NoiseStage.FractalNoise, Noise/NoiseStage.cs:15-24 */
    float hurst, startingAmplitude, stepdown, detuneRate;
    int32_t octaves, noiseSize;
    int32_t filter;               /* KernelFilterType */
    int32_t filterIterations;     /* KernelFilterStage.iterations, 0 = no filter stage */
    int32_t flowIterations;       /* FlowMapStage.iterations, 0 = no flow stage */
    float normMin, normMax;
    int32_t erosionIterations;    /* ErosionKernelJob applications, 0 = none */
} nz_terrain_params;

/* ---- one large grid over the GPUs of a node: row stripes + RCCL neighbour halo exchange (new-framework feature,
 * SURVEY.md 8e; the reference only has independent clamped tiles, Scripts/MeshTileGenerator.cs:166-192, which a host
 * requests one by one through BasePipeline.Schedule, Pipeline/Executable/Pipeline.cs:104-128).  One process per GPU;
 * every process creates a context on its device and joins ONE communicator.  RCCL (librccl.so.1) is opened when the
 * first communicator entry is called: a host that never shards never loads it.
 *
 * nz_comm_unique_id  = ncclGetUniqueId: called by ONE rank, the 128 bytes travel to the others out of band (a file, a
 *                      socket, the launcher's store);
 * nz_comm_init       = ncclCommInitRank on ctx's device (blocks until all `world` ranks have called it) plus the
 *                      communicator's own HIP stream: exchanges run there, ordered against ctx's stream by events, so that
 *                      kernels which read no ghost row overlap them. */
typedef struct nz_comm nz_comm;
#define NZ_COMM_ID_BYTES 128
int32_t nz_comm_unique_id(uint8_t *id_out /* NZ_COMM_ID_BYTES */);
int32_t nz_comm_init(nz_ctx *ctx, const uint8_t *id, int32_t rank, int32_t world, nz_comm **out);
int32_t nz_comm_destroy(nz_comm *comm);
int32_t nz_comm_rank(const nz_comm *comm);
int32_t nz_comm_world(const nz_comm *comm);
int32_t nz_comm_rccl_version(int32_t *version); /* ncclGetVersion of the library actually loaded, e.g. 22606 */

/* Neighbour halo exchange of the stripe `st` that rank comm->rank holds of a grid split into comm->world row stripes
 * (rank r above rank r + 1): for each of the n_planes planes (all of the stripe's shape) the `up_rows` ghost rows above
 * the owned rows are received from rank - 1, which sends the last up_rows rows it owns, and the `down_rows` ghost rows
 * below from rank + 1 (its first down_rows owned rows) -- ncclGroupStart; ncclSend / ncclRecv with rank +- 1;
 * ncclGroupEnd on the communicator's stream, behind everything enqueued on ctx's stream so far.  Ranks at the global
 * border have no neighbour on that side (clamp-to-edge applies there).  Every rank must make the same call.
 *   nz_halo_exchange_begin  : posts the batch and returns; kernels enqueued on ctx afterwards run concurrently with it
 *                             (they must not touch the ghost rows);
 *   nz_halo_exchange_finish : ctx's stream waits for the batch; `out` completes after it;
 *   nz_halo_exchange        : begin + finish. */
int32_t nz_halo_exchange_begin(nz_ctx *ctx, nz_comm *comm, float *const *planes, int32_t n_planes, const nz_stripe *st,
                               int32_t up_rows, int32_t down_rows, nz_handle dep);
int32_t nz_halo_exchange_finish(nz_ctx *ctx, nz_comm *comm, nz_handle *out);
int32_t nz_halo_exchange(nz_ctx *ctx, nz_comm *comm, float *const *planes, int32_t n_planes, const nz_stripe *st,
                         int32_t up_rows, int32_t down_rows, nz_handle dep, nz_handle *out);

/* GetMapRangeJob (Filter/NormalizeJob.cs:17-55) of a grid whose rows are spread over the ranks: `res` = DEVICE {min,
 * max, max - min} of the WHOLE grid on every rank.  Each rank folds its `n_floats` cells (nz_get_map_range), one
 * ncclAllGather carries the per-rank triples, and the same fold runs over the gathered minima and maxima in rank order
 * -- the order the monolithic job walks the grid in, so the result is the monolithic one down to the sign of a zero
 * extreme.  The path's one collective.  comm == NULL: one rank. */
int32_t nz_comm_allgather_range(nz_ctx *ctx, nz_comm *comm, const float *map, size_t n_floats, float *res, float lim_min,
                                float lim_max, nz_handle dep, nz_handle *out);
/* In-place maximum of `n` int32 words (device) over the ranks: ncclAllReduce(ncclMax, ncclInt32), stream-ordered like
 * nz_comm_allgather_range.  The vote of the sharded depression fill: "did any rank change in this round".  comm NULL: one
 * rank, the words stay. */
int32_t nz_comm_allreduce_max_i32(nz_ctx *ctx, nz_comm *comm, int32_t *words, int32_t n, nz_handle dep, nz_handle *out);

/* The stock stage list (nz_terrain_params) on a grows x cols grid cut into `stripes` row stripes over all ranks; rank r
 * holds stripes [r * S, (r + 1) * S), S = stripes / world.  The object owns the stripes' planes and the launch plan,
 * which is compiled once: nz_sharded_pipeline replays it.  haloMode:
 *   NZ_HALO_RECOMPUTE     every stripe evaluates the noise on its rows plus the stencil radius of everything downstream
 *                         and each launch produces a window that shrinks by the radius it consumed: no data-path
 *                         communication (closed-form source only);
 *   NZ_HALO_EXCHANGE      before each launch the stripes exchange exactly the ghost rows it consumes.  `overlap`:
 *                         0  the transfers are enqueued on the compute stream itself, between the launch that produced the
 *                            rows and the launch that reads them (no second stream, no event hand-off) -- the fastest form
 *                            on MI355X: a transfer kernel takes ~14 us, and one running beside a stencil launch that fills
 *                            the chip does not finish before that launch does (measured);
 *                         1  on the communicator's stream, while the launch's interior rows, which read no ghost row, run;
 *                            its border rows follow after the wait;
 *                         2  a launch produces the rows its neighbours need first, the exchange for the NEXT launch travels
 *                            while its interior rows run;
 *   NZ_HALO_EXCHANGE_ONCE the source plane's ghost rows for the whole pipeline are exchanged once, then as RECOMPUTE.
 * Transfers between stripes of different ranks AND between two stripes of one rank go through ncclSend / ncclRecv (RCCL
 * runs a send and its matching receive on one device), so that a one-GPU box executes the very code path of a node;
 * comm == NULL (one rank, no RCCL): device copies on the context's stream.
 * externalSource != 0: no noise stage; the caller fills the owned rows of every stripe's source plane (an uploaded
 * height map) before nz_sharded_pipeline.  asRank / asWorld (asWorld > 0): rehearsal on one rank of the geometry rank
 * asRank of asWorld would have; neighbours beyond the process are played by its own stripes (timing only).
 * Same kernels, same operation order as the single-tile entries: the sharded result equals the monolithic grid bit for
 * bit (the only clamps are at the global border). */
typedef struct nz_sharded nz_sharded;
enum nz_halo_mode { NZ_HALO_RECOMPUTE = 0, NZ_HALO_EXCHANGE = 1, NZ_HALO_EXCHANGE_ONCE = 2 };
typedef struct nz_sharded_desc {
    int32_t grows, cols;    /* the global grid */
    int32_t stripes;        /* over all ranks; a multiple of the world size */
    int32_t haloMode;       /* enum nz_halo_mode */
    int32_t overlap;        /* NZ_HALO_EXCHANGE: 0 inline on the compute stream, 1 interior rows first, 2 border rows first */
    int32_t xpos, zpos;     /* GeneratorData.xpos / zpos of the grid's first cell */
    int32_t externalSource;
    int32_t asRank, asWorld;
} nz_sharded_desc;
int32_t nz_sharded_create(nz_ctx *ctx, nz_comm *comm, const nz_sharded_desc *desc, const nz_terrain_params *params,
                          nz_sharded **out);
int32_t nz_sharded_destroy(nz_sharded *sh);
int32_t nz_sharded_local_stripes(const nz_sharded *sh);
/* geometry of local stripe i, its source plane (what the noise stage fills, or the caller) and the plane whose owned
 * rows hold the result after nz_sharded_pipeline; any pointer may be NULL */
int32_t nz_sharded_stripe(const nz_sharded *sh, int32_t i, nz_stripe *st, float **source, float **result);
/* The compiled plan as records of 8 int32 {op, local stripe (-1: all), n, a, b, own0, own1, planes}:
 *   op 1 noise                       rows [own0, own1) of plane `planes`
 *   op 2 exchange begin              n = planes per stripe, a = up_rows, b = down_rows, planes = first plane id
 *   op 3 exchange finish
 *   op 4 kernel filter   n = fused applications, rows [own0, own1), planes = src | dst << 8
 *   op 5 flow map        n = fused iterations, a = first, b = last, planes = src | dst << 8 | state_in << 16 | state_out << 24
 *   op 6 value erosion   n = fused applications
 *   op 7 stage marker    n = 0 noise, 1 filter, 2 flow, 3 erosion, 4 end
 * `records` may be NULL to query the count. */
int32_t nz_sharded_plan(const nz_sharded *sh, int32_t *records, int32_t max_records, int32_t *count);
/* The transfers of the plan's exchanges in the order this rank posts them, as records of 4 int32 {exchange, source rank,
 * destination rank, floats}: a rank posts ncclSend for the records it is the source of and ncclRecv for those it is the
 * destination of, in this order inside one group per exchange.  On a plan-only object (ctx == NULL at creation, asRank of
 * asWorld) these are the lists of that rank of the real job: laid side by side for all ranks, the k-th send of rank a to
 * rank b must be the k-th receive rank b posts from rank a, with the same size (tests/test_sharded_native.py). */
int32_t nz_sharded_transfers(const nz_sharded *sh, int32_t *records, int32_t max_records, int32_t *count);
/* one pass of the pipeline on every local stripe (enqueue only); `marks` (nullable, 5 handles): markers on the context's
 * stream where the noise, filter, flow and erosion launches begin, and at the end */
int32_t nz_sharded_pipeline(nz_ctx *ctx, nz_sharded *sh, nz_handle *marks, nz_handle dep, nz_handle *out);
/* exchanges and payload bytes this rank sends per pass */
int32_t nz_sharded_traffic(const nz_sharded *sh, int32_t *exchanges, size_t *bytes_sent);
/* with timing on, every wait of the compute stream for an exchange (overlap 0: every exchange itself) is bracketed by
 * events; nz_sharded_exchange_ms sums and forgets the brackets recorded so far (host blocks until they have completed; at
 * most 1024 are kept) */
int32_t nz_sharded_set_timing(nz_sharded *sh, int32_t on);
int32_t nz_sharded_exchange_ms(nz_sharded *sh, float *ms);
/* GetMapRangeJob + MapNormalizeValues over the result planes of the whole grid (nz_comm_allgather_range over all
 * stripes of all ranks, then NormalizeMap on the owned rows with the device args) */
int32_t nz_sharded_map_range(nz_ctx *ctx, nz_sharded *sh, float *res, float lim_min, float lim_max, nz_handle dep,
                             nz_handle *out);
int32_t nz_sharded_normalize(nz_ctx *ctx, nz_sharded *sh, const float *args, nz_handle dep, nz_handle *out);

#ifdef __cplusplus
}
#endif
#endif /* NOIZE_HIP_H */
