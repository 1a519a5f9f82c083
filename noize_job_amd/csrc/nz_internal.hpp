// nz_internal.hpp -- shared declarations of libnoize_hip (host side + launcher prototypes).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/noize_hip.h"
#include "nz_chain_plan.hpp"  // the chained filter grid's tile plan (plain C++)
#include "nz_planes.hpp"  // nz_set_error, NZ_REQUIRE, nz_check_stripe: the host-only geometry and aliasing helpers

// ---- error plumbing -------------------------------------------------------------------------
#define NZ_HIP(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            nz_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                         __LINE__);                                                       \
            return NZ_ERR_HIP;                                                            \
        }                                                                                 \
    } while (0)

#define NZ_TRY(expr)              \
    do {                          \
        int32_t rc_ = (expr);     \
        if (rc_) return rc_;      \
    } while (0)

// ---- context --------------------------------------------------------------------------------
struct nz_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    // JobHandle ring: the handle with sequence number q lives in events[q % size] while q > last_seq - size.
    // A handle VALUE is (ctx id << NZ_HANDLE_SEQ_BITS) | q, so that a handle names its context: a dependency on
    // another context's handle becomes a hipStreamWaitEvent (JobHandle dependencies across pipelines,
    // Pipeline/Executable/ReducePipeline.cs:82-148).  `hmx` guards the ring against a foreign context's lookup.
    std::vector<hipEvent_t> events;
    uint64_t last_seq = 0;
    uint32_t id = 0;
    std::mutex hmx;
    // psrnoise gradient tables (rot 0 and rot 0.62), built with the host libm
    float *d_rgrad = nullptr;
    // snoise lattice tables: int T1[292] (16*permute(i)) followed by float4 T2[580] (gradient of permute(j))
    void *d_simplex = nullptr;
    // stage scratch owned by the ctx (grown on demand)
    float *scratch = nullptr;
    size_t scratch_floats = 0;
    // chained launches (nz_launch_conv_chain): tile flags (grown on demand, never cleared: they carry an epoch)
    int *chain_flags = nullptr;
    size_t chain_flags_n = 0;
    // the error words in mapped host memory ([0]: a chained filter launch gave up waiting, [1]: the pile solver's ticket launch
    // did -- one word per kind, so neither overwrites the other), and their device address
    unsigned *chain_err = nullptr, *chain_err_dev = nullptr;
    unsigned chain_epoch = 0;
    // ... and their tile plans (nz_chain_plan.hpp): a pipeline calls the stage with the same geometry for every tile, so a
    // plan is built and uploaded once (nz_ctx_chain_plan).  Four plans, the least recently used one is replaced.  Every slot
    // owns its pinned staging copy, so a replacement waits for that slot's own last upload (`uploaded`) and nothing else.
    struct chain_plan_slot {
        nz_chain_key key{};
        int total = 0;  // 0: empty
        nz_chain_item *dev = nullptr, *pinned = nullptr;
        size_t cap = 0;  // records both buffers hold
        hipEvent_t uploaded = nullptr;
        uint64_t used = 0;  // chain_plan_clock at the last hit
    };
    chain_plan_slot chain_plans[4];
    uint64_t chain_plan_clock = 0, chain_plan_uploads = 0;
    bool chain_off = false;  // a chained launch once timed out on this context: separate launches from then on
    // Which work a chained launch's time-out belongs to: a failing tile lowers *chain_err_epoch (device memory, atomicMin) to
    // its launch's epoch before it raises the flag; the host remembers the handle sequence number each of its last chained
    // launches was issued at.  Once seen, the failure is reported (NZ_ERR_RETRY) by every wait on a handle in [retry_lo,
    // retry_hi] -- issued at or after the failing launch and before the failure was first REPORTED (retry_open: the window's
    // upper end follows last_seq until then) -- and by the next nz_ctx_synchronize; a wait on an older handle (another
    // pipeline's, a fence recorded before the stage) completes clean.
    unsigned *chain_err_epoch = nullptr;
    struct chain_mark { unsigned epoch; uint64_t seq; };
    chain_mark chain_marks[64] = {};
    uint64_t retry_lo = 0, retry_hi = 0;
    bool retry_sync_pending = false, retry_open = false;
    // live erosion, the pile solver's ticket launch (nz_live.hip): safe mode (nz_ctx_set_pile_safe) waits for it and runs the job
    // again colour by colour should it ever give up -- for good on this context (pile_ticket_off)
    bool pile_safe = false, pile_ticket_off = false;
    int pile_retries = 0;
    bool handle_rides = false;    // this entry's handle may ride on its last kernel launch (nz_ctx_handle_rides)
    uint64_t armed_seq = 0;       // ... and this is the sequence number reserved for it (nz_ctx_arm_last_launch)
    // pool automaton, sparse form (nz_pool_job in nz_stages.cpp): {entries, done, -} in device memory, and in mapped host
    // memory what the last job that ran reported: job number << 32 | non-empty mask words it found
    int *pool_ctl = nullptr;
    unsigned long long *pool_hint = nullptr, *pool_hint_dev = nullptr;
    unsigned long long pool_seq = 0;
    // how the last pool job ran (nz_debug_pool_last_job): the two switches as it read them, and whether the host enqueued the
    // dense launches; -1: no job yet
    int pool_last_runs = -1, pool_last_sparse = -1, pool_last_dense = 0;
    int float_mode = NZ_FLOAT_STRICT;  // nz_ctx_set_float_mode
};
int32_t nz_ctx_pool_state(nz_ctx *ctx);  // allocates the three on first use

#define NZ_TRY_(expr)             \
    do {                          \
        int32_t rc_t_ = (expr);    \
        if (rc_t_) return rc_t_;    \
    } while (0)

constexpr int NZ_HANDLE_SEQ_BITS = 40;
constexpr uint64_t NZ_HANDLE_SEQ_MASK = (1ull << NZ_HANDLE_SEQ_BITS) - 1;
int32_t nz_ctx_begin(nz_ctx *ctx, nz_handle dep);           // set device, order the stream after `dep`
int32_t nz_ctx_finish(nz_ctx *ctx, nz_handle *out);         // record the JobHandle marker
int32_t nz_ctx_scratch(nz_ctx *ctx, size_t floats, float **out);

// how every stage entry point opens
#define NZ_BEGIN(ctx, dep)                   \
    do {                                     \
        int32_t rc_ = nz_ctx_begin(ctx, dep); \
        if (rc_) return rc_;                 \
    } while (0)

// ---- kernel parameter blocks ----------------------------------------------------------------
constexpr int NZ_MAX_KSIZE = 25;
// psrnoise tables.  The hash arguments are iu = xw + 0.5 yw and yw with xw = fmod(., 1010), yw = fmod(., 102):
// integers in (-1061, 1061) and (-102, 102), negative for negative lattice coordinates (C fmod keeps the sign).
//   T1[i] = 8 * (permute(i - O1) + O2): the first, un-reduced permute, argument in [-O1, T1 - O1)
//   T2[rot][j] = (cos u, sin u) of the gradient hashed from a = j - O2 (second permute + rgrad2), a = permute + yw
constexpr int NZ_PSR_O1 = 1064, NZ_PSR_T1 = NZ_PSR_O1 + 1064;
constexpr int NZ_PSR_O2 = 104, NZ_PSR_T2 = NZ_PSR_O2 + 392;

struct nz_kernel_taps {
    float kx[NZ_MAX_KSIZE];
    float kz[NZ_MAX_KSIZE];
    float factor;
    int ksize;
};

// what every fractal kernel takes by value (64 bytes: the kernel argument offsets behind it are part of the tuned code)
struct nz_fractal_kparams {
    float posx, posz;     // (float)xpos, (float)(zpos + first row)
    float noise_size;     // (float)NoiseSize
    float G;              // exp2f(-hurst), host libm
    float amp;            // StartingAmplitude
    float stepdown, detune_rate;
    float norm;           // CalcFractalNormValue
    float fmax;           // max over the octaves of |frequency| (same fp32 recurrence as the kernels; NaN if it overflows)
    int octaves;
    // batched launch (one grid per blockIdx.y): grids `bstride` floats apart, {xpos, zpos} of grid b at positions[2b]
    const int32_t *positions = nullptr;
    size_t bstride = 0;
    int rows_per_wg = 8;  // rows one workgroup walks through (8 amortises the table staging; fewer for small grids)
    int shape = 0;        // octave shape (enum nz_fractal_shape; the kernels have it as a template argument), 0 = fBm
};
// the ridged shape's two constants: a trailing kernel argument, so the shape-0 kernels keep their argument layout
struct nz_ridge_params {
    float offset = 1.0f, gain = 2.0f;
};
// The octaves' frequencies and amplitudes, f_0 = 1, f_{i+1} = f_i * (stepdown - detune_{i+1}), a_0 = amp, a_{i+1} = a_i * G:
// wave-uniform, and gfx9 has no scalar float ALU, so a kernel that runs the recurrence pays three VALU instructions per
// wave and octave for values the host knows.  fractal_impl fills them with the kernels' own fp32 operation sequence
// (nz_stages.cpp is compiled without contraction) for up to NZ_OCT_TAB octaves; `n` is 0 beyond that, and the kernel keeps
// its recurrence.  A trailing kernel argument of the simplex table kernel, read with scalar loads.
constexpr int NZ_OCT_TAB = 16;
struct nz_octave_table {
    float f[NZ_OCT_TAB], a[NZ_OCT_TAB];
    int n = 0;  // entries filled: the octave count, or 0 (no table)
    // Power-of-two ladder (appended: kernels that ignore it keep their argument layout).  > 0 when the table is filled and
    // every f[i] is a positive, normal, exact power of two (stepdown 2, 4 or 0.5 without detune): then octave i's skewed
    // simplex coordinates are octave 0's times f[i], bit for bit, for coordinates that are zero or at least this large in
    // magnitude: 2^-64 / min(1, min f[i]) (fractal_simplex_tab_kernel has the proof).  0: no ladder.
    float ladder_lo = 0.0f;
};
struct nz_fractal_params : nz_fractal_kparams {
    nz_ridge_params ridge;  // NZ_SHAPE_RIDGED only
    nz_octave_table oct;
};
// the domain warp's constants (nz_fractal_warped*): a trailing kernel argument of the warped kernels.  norm / fmax are the
// displacement loop's CalcFractalNormValue and max |frequency| (as fractal_impl computes them for the main loop); the
// kernels bound the displacement coordinates u = x * scale themselves, the 5.2 / 1.3 offsets of D's second evaluation included
struct nz_warp_params {
    float strength = 0.0f, scale = 1.0f;
    int octaves = 0;
    float norm = 0.0f, fmax = 0.0f;
};

// plane geometry handed to every stencil kernel: clamp rows are the global border seen from the
// buffer, intersected with the buffer itself.
struct nz_geom {
    int cols;      // row length
    int pitch;     // floats between rows
    int rows;      // rows in the buffer
    int zc0, zc1;  // inclusive clamp range for row reads (buffer coordinates)
    int or0, or1;  // rows to produce [or0, or1)
    // batched launches: `count` independent grids of this geometry, `bstride` floats apart in every plane;
    // the kernels take the grid index from blockIdx.y
    int count = 1;
    size_t bstride = 0;
};

inline nz_geom nz_geom_batch(int res, int count) {
    nz_geom g{res, res, res, 0, res - 1, 0, res};
    g.count = count;
    g.bstride = (size_t)res * res;
    return g;
}
// floats covered by rows [or0, or1) of every grid of the batch when the grids are stored back to back
inline size_t nz_geom_span(const nz_geom &g) {
    return g.count > 1 ? (size_t)g.count * g.bstride : (size_t)(g.or1 - g.or0) * g.pitch;
}

inline nz_geom nz_geom_from_stripe(const nz_stripe &s) {
    nz_geom g;
    g.cols = s.cols;
    g.pitch = s.pitch > 0 ? s.pitch : s.cols;
    g.rows = s.rows;
    int lo = -s.grow0, hi = s.grows - 1 - s.grow0;
    g.zc0 = lo > 0 ? lo : 0;
    g.zc1 = hi < s.rows - 1 ? hi : s.rows - 1;
    g.or0 = s.own0;
    g.or1 = s.own1;
    return g;
}

inline nz_geom nz_geom_tile(int res) { return nz_geom{res, res, res, 0, res - 1, 0, res}; }

// ---- handles that ride on a launch --------------------------------------------------------------------------------------
// A JobHandle used to be a hipEventRecord behind the entry's work: a barrier packet of its own, ~2.8 us of the stream.  A
// kernel launch can carry the event instead (hipExtLaunchKernelGGL's stop event: the dispatch's own completion signal,
// tools/probe_write_value.hip measures no cost at all).  An entry whose LAST enqueued operation is the last launch of a
// helper says so (nz_ctx_handle_rides); the helper arms the launch it knows to be its last (nz_ctx_arm_last_launch); that
// launch -- NZ_LAUNCH instead of hipLaunchKernelGGL -- takes the event; nz_ctx_finish hands out the handle, or records an
// event the old way when nothing took it.  nz_ctx_begin disarms whatever an entry that failed left behind.
extern thread_local hipEvent_t nz_tls_stop_event;
// the float mode of the context whose entry this thread is running (set by nz_ctx_begin: every launcher runs behind one)
extern thread_local int nz_tls_float_mode;
#define NZ_LAUNCH(kernel, grid, block, lds, stream, ...)                                                  \
    do {                                                                                                   \
        if (nz_tls_stop_event) {                                                                           \
            hipEvent_t nz_stop_ = nz_tls_stop_event;                                                       \
            nz_tls_stop_event = nullptr;                                                                   \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, nullptr, nz_stop_, 0, __VA_ARGS__);    \
        } else {                                                                                           \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                             \
        }                                                                                                  \
    } while (0)
// the four instantiations of a tap-sum kernel: calls f(UNIT, FAST) with std::bool_constant arguments.  UNIT: the taps'
// factor is 1 (no final multiply); FAST: the context runs NZ_FLOAT_FAST (contracted tap sums)
template <class F>
inline void nz_with_unit_fast(const nz_kernel_taps &k, F &&f) {
    const bool fast = nz_tls_float_mode >= NZ_FLOAT_FAST;
    if (k.factor == 1.0f) {
        if (fast) f(std::true_type(), std::true_type()); else f(std::true_type(), std::false_type());
    } else {
        if (fast) f(std::false_type(), std::true_type()); else f(std::false_type(), std::false_type());
    }
}
// the 2^n instantiations of a kernel with n bool template arguments: calls f with each run-time bool as a std::true_type or
// std::false_type argument, in the order given (the kernel's argument is then `decltype(x)::value`)
template <class F, class... Bools>
inline void nz_with_bools(F &&f, Bools... picked) {
    f(picked...);
}
template <class F, class... Rest>
inline void nz_with_bools(F &&f, bool b, Rest... rest) {
    if (b) nz_with_bools(f, rest..., std::true_type());
    else nz_with_bools(f, rest..., std::false_type());
}
void nz_ctx_handle_rides(nz_ctx *ctx, bool wanted);
void nz_ctx_arm_last_launch(nz_ctx *ctx);

// `n` >= 1 iterations as the fewest launches of at most `cap` each, split as evenly as they go: the depth of every launch,
// larger ones first.  even: the series ping-pongs in place and must leave its result where it started, so an odd launch
// count takes one launch more while every launch still gets an iteration (it stays odd only when each launch holds one
// iteration already: the caller copies back)
inline std::vector<int> nz_split_iterations(int n, int cap, bool even = false) {
    int L = (n + cap - 1) / cap;
    if (even && (L & 1) && L + 1 <= n) L += 1;
    std::vector<int> d(L);
    for (int i = 0; i < L; i++) d[i] = n / L + (i < n % L ? 1 : 0);
    return d;
}

// ---- argument checks shared by the stage entry points (nz_stages.cpp, nz_terrain_stages.cpp) ----------------------------
static inline int32_t check_res(int32_t resolution) {
    NZ_REQUIRE(resolution >= 1 && resolution <= 46340, "resolution %d out of range", resolution);
    return NZ_OK;
}
static inline int32_t check_batch(int32_t resolution, int32_t count) {
    NZ_TRY(check_res(resolution));
    NZ_REQUIRE(count >= 1 && count <= 65535, "count %d out of range [1,65535]", count);
    return NZ_OK;
}
// READ / WRITE pair forms (nz_rw_tile): TileHelpers.SWAP_RWTILE (Pipeline/Tiles/TileData.cs:42-45) as a swap of the two
// pointers instead of a copy job
static inline int32_t check_rw(const nz_rw_tile *t) {
    NZ_REQUIRE(t, "tile is NULL");
    NZ_TRY(check_batch(t->resolution, t->count));
    NZ_REQUIRE(t->read && t->write && t->read != t->write, "read/write must be two distinct planes");
    return NZ_OK;
}
static inline nz_geom rw_geom(const nz_rw_tile *t) {
    return t->count > 1 ? nz_geom_batch(t->resolution, t->count) : nz_geom_tile(t->resolution);
}
static inline void rw_swap(nz_rw_tile *t, bool swapped) {
    if (swapped) {
        float *r = t->read;
        t->read = t->write;
        t->write = r;
    }
}

// nz_stages.cpp, for the sharded plan (nz_comm.cpp)
int32_t nz_filter_taps(int32_t filter, nz_kernel_taps *t);  // KernelFilterType -> taps
int nz_conv_tcap(int ksize);                                // applications fused per launch (0: no fused kernel)
int32_t nz_fractal_rows(nz_ctx *ctx, hipStream_t stream, int noiseType, float *dst, int rows, int cols, int pitch, float hurst,
                        float amp, float stepdown, float detune, int octaves, int xpos, int zpos_first_row, int noiseSize);

// ---- launchers (defined in the .hip files) ---------------------------------------------------
// `positions` (nullable, device): {xpos, zpos} per grid of a batched launch of `count` grids `bstride` floats apart
int32_t nz_launch_fractal(hipStream_t s, int noiseType, float *dst, int rows, int cols, int pitch,
                          const nz_fractal_params &p, const float *d_rgrad, const void *d_simplex, int count = 1,
                          size_t bstride = 0, const int32_t *positions = nullptr, const nz_warp_params *warp = nullptr);
// the billow / ridged kernels (nz_fractal_shaped.hip); p complete, rows_per_wg / positions / bstride included
int32_t nz_launch_fractal_shaped(hipStream_t s, int noiseType, float *dst, int rows, int cols, int pitch,
                                 const nz_fractal_params &p, const float *d_rgrad, const void *d_simplex, int count);
// the domain-warped kernels (nz_fractal_warped.hip); p complete as above, wp.octaves >= 1
int32_t nz_launch_fractal_warped(hipStream_t s, int noiseType, float *dst, int rows, int cols, int pitch,
                                 const nz_fractal_params &p, const nz_warp_params &wp, const float *d_rgrad,
                                 const void *d_simplex, int count);

int nz_conv_max_fused(int ksize);
// T fused applications of (X pass, Z pass) src -> dst on rows [or0, or1)
int32_t nz_launch_conv_fused(hipStream_t s, const float *src, float *dst, const nz_geom &g,
                             const nz_kernel_taps &k, int T);
// the same as one row-streaming launch (nz_conv_stream.hip; 3 and 5 taps)
int nz_conv_stream_max(int ksize);
bool nz_conv_stream_wanted(const nz_geom &g, int ksize, int T);
int32_t nz_launch_conv_stream(hipStream_t s, const float *src, float *dst, const nz_geom &g, const nz_kernel_taps &k, int T);
// L launches as one grid with tile-level dependencies; see nz_filter.hip
int nz_conv_chain_items(int ksize, const nz_geom &g, const int *Ts, int L);
int nz_cu_count();  // compute units of the current device (256 on MI355X): a launch of at most this many workgroups is one round
bool nz_conv_small_grid(int ksize, const nz_geom &g);  // 64-row tiles
bool nz_conv_tiny_grid(int ksize, const nz_geom &g);
bool nz_conv_chain_key(int ksize, const nz_geom &g, const int *Ts, int L, nz_chain_key *key);  // false: no chained form
int32_t nz_launch_conv_chain(hipStream_t s, float *plane0, float *plane1, const nz_geom &g, const nz_kernel_taps &k,
                             const nz_chain_item *items, int total, int *flags, unsigned epoch, unsigned *err_host,
                             unsigned *err_epoch);
// the plan of `key` in device memory, uploaded on the context's stream unless the context already holds it
int32_t nz_ctx_chain_plan(nz_ctx *ctx, const nz_chain_key &key, const nz_chain_item **items, int *total);
int32_t nz_ctx_chain_state(nz_ctx *ctx, size_t items, int **flags, unsigned *epoch, unsigned **err_host, unsigned **err_epoch);
int32_t nz_ctx_error_word(nz_ctx *ctx, unsigned **err_host);  // mapped host memory, device address: [0] chained filter, [1] pile solver
// one whole application of a wide odd kernel (11..25 taps), src -> dst
bool nz_conv_has_wide(int ksize);
int32_t nz_launch_conv_wide(hipStream_t s, const float *src, float *dst, const nz_geom &g, const nz_kernel_taps &k);
// single unfused passes (src -> dst): any kernelSize <= 25, and single applications
int32_t nz_launch_conv_pass_x(hipStream_t s, const float *src, float *dst, const nz_geom &g,
                              const nz_kernel_taps &k);
int32_t nz_launch_conv_pass_z(hipStream_t s, const float *src, float *dst, const nz_geom &g,
                              const nz_kernel_taps &k);
// E fused applications of the {-1,0} min window: src -> dst
int nz_erosion_max_fused();
int32_t nz_launch_erosion_fused(hipStream_t s, const float *src, float *dst, const nz_geom &g, int E);
// one reference min pass, window k in [-k_off, k_off), along x (along_z == 0) or z

int32_t nz_launch_fill(hipStream_t s, float *data, size_t n, float value);
int32_t nz_launch_copy(hipStream_t s, float *dst, const float *src, size_t n);
// delegate-level flow kernels (single tile semantics, global-memory stencils)
int32_t nz_launch_flow_step(hipStream_t s, const float *h, const float *w, const float *fN, const float *fS,
                            const float *fE, const float *fW, float *oN, float *oS, float *oE, float *oW,
                            const nz_geom &g);
int32_t nz_launch_water_step(hipStream_t s, const float *w, float *w_out, const float *fN, const float *fS,
                             const float *fE, const float *fW, const nz_geom &g);
int32_t nz_launch_velocity(hipStream_t s, float *dst, const float *fN, const float *fS, const float *fE,
                           const float *fW, const nz_geom &g, int normalize, float nmin, float nrange);
int32_t nz_launch_normalize(hipStream_t s, const float *src, float *dst, size_t n, float nmin, float nrange);
// n <= nz_flow_fused_max() iterations per launch on an on-chip tile; state planes are {water,fN,fS,fE,fW}
int nz_flow_fused_max();
// h_out (nullable): the launch also stores its interior height cells there (a private copy, so that a
// later launch may overwrite the caller's plane)
int32_t nz_launch_flow_fused(hipStream_t s, const float *h, const float *const in[5], float *const out[5], float *dst,
                             float *h_out, const nz_geom &g, int n, int first, int last, float nmin, float nrange);

// the whole stage (first && last) as one row-streaming launch (nz_flow_stream.hip)
bool nz_flow_stream_wanted(const nz_geom &g, int n);
int nz_flow_form(const nz_geom &g, int n, int first, int last);  // enum nz_flow_form: the form one fused launch takes
int32_t nz_launch_flow_stream(hipStream_t s, const float *h, float *dst, const nz_geom &g, int n, float nmin, float nrange);

// grid hydraulic erosion (nz_hydraulic.hip): one iteration per launch on `count` tiles of res^2 cells stored back to back.
// State planes {d, s, fN, fS, fE, fW}; `in` is not read by the first launch (the start state is implied), the last launch
// writes b + s to h_out and the water to out[0] only
struct nz_hydraulic_planes {
    const float *in[6];
    float *out[6];
};
struct nz_hydraulic_params {
    float initial_water, rain, keep;  // keep = 1 - evaporation
    float capacity, dissolve, deposit, min_tilt;
};
// the _ex entries' options (include/noize_hip.h): open border, the two read-only maps, the two running-sum masks; a NULL
// plane is an option left off.  Planes of count * res^2 floats like the heights
struct nz_hydraulic_ex {
    int open = 0;
    const float *rain_map = nullptr, *hardness = nullptr;
    float *wear = nullptr, *deposits = nullptr;
};
enum { NZ_HYD_OPEN = 1, NZ_HYD_MAPS = 2, NZ_HYD_MASKS = 4 };  // the kernel's compile-time option groups
// ex: NULL or all off -> the default kernels
int32_t nz_launch_hydraulic(hipStream_t s, const float *h_in, float *h_out, const nz_hydraulic_planes &p,
                            const nz_hydraulic_params &k, int res, int count, int first, int last,
                            const nz_hydraulic_ex *ex = nullptr);
// the stripe form: one iteration on rows [g.or0, g.or1) of one stripe-shaped plane set (g: nz_geom_from_stripe with the
// launch's window as its produced rows); the clamps and the open border are at g's clamp range, the masks are updated on
// rows [own0, own1) only
int32_t nz_launch_hydraulic_stripe(hipStream_t s, const float *h_in, float *h_out, const nz_hydraulic_planes &p,
                                   const nz_hydraulic_params &k, const nz_geom &g, int own0, int own1, int first, int last,
                                   const nz_hydraulic_ex &ex);

// stream-power fluvial erosion (nz_fluvial.hip): one iteration per launch on `count` tiles of res^2 cells stored back to
// back, heights h_in -> h_out and drainage a_in -> a_out.  a_in NULL: the drainage read is the constant k.rain (the start
// state without rain map and drainageIn).  A NULL map is an option left off
struct nz_fluvial_params {
    float erodibility, uplift, dt, rain, sea_level;
};
int32_t nz_launch_fluvial(hipStream_t s, const float *h_in, float *h_out, const float *a_in, float *a_out,
                          const nz_fluvial_params &k, int res, int count, const float *rain_map, const float *hardness,
                          const float *uplift_map);
// the stripe form: one iteration on rows [g.or0, g.or1) of one stripe-shaped plane set (g: nz_geom_from_stripe with the
// launch's window as its produced rows); [zlo, zhi] are the first and last row of the global grid in buffer rows, which may
// lie outside the buffer.  Reads reach 2 rows beyond the window, never beyond the grid.  a_in NULL with a rain map: the
// start state rain * rain_map is formed in the kernel
int32_t nz_launch_fluvial_stripe(hipStream_t s, const float *h_in, float *h_out, const float *a_in, float *a_out,
                                 const nz_fluvial_params &k, const nz_geom &g, int zlo, int zhi, const float *rain_map,
                                 const float *hardness, const float *uplift_map);
// the start state with a rain map: a[i] = rain * rain_map[i]
int32_t nz_launch_fluvial_start(hipStream_t s, float *a, const float *rain_map, float rain, size_t n);

// depression filling (nz_fill.hip): pass `pass` of the series on `count` tiles of res^2 cells stored back to back, W planes
// w_in -> w_out (pass 0 reads none: it derives the start state from h), the per-tile "changed" bytes flags_in -> flags_out,
// at most `sweeps` in-LDS sweeps per tile.  status: {passes, converged, changed[3]}, maintained by the launches themselves
int32_t nz_launch_fill_pass(hipStream_t s, const float *h, const float *w_in, float *w_out, int *status,
                            const unsigned char *flags_in, unsigned char *flags_out, float eps, float sea, int res, int count,
                            int pass, int sweeps);
// converged: h = w and (depth given) depth = w - h; otherwise h stays and depth = 0.  Sets status[1]
int32_t nz_launch_fill_finalise(hipStream_t s, float *h, const float *w, float *depth, int *status, size_t n);
// the stripe form, one round (nz_fill_stripe): begin sets the status words from the caller's proceed word and the caller's
// `changed` word; a pass works on the owned rows [g.or0, g.or1) of stripe-shaped planes against the frozen rows or0 - 1 and
// or1 of w_ghost (first: derived from h), [zlo, zhi] the global grid in buffer rows; end brings the owned rows of the work
// plane to w when all `passes` passes ran; finalise is all or nothing on the owned rows by the caller's verdict
int32_t nz_launch_fill_round_begin(hipStream_t s, int *status, const int *proceed, int *changed, int first);
int32_t nz_launch_fill_stripe_pass(hipStream_t s, const float *h, const float *w_in, float *w_out, const float *w_ghost,
                                   int *status, const unsigned char *flags_in, unsigned char *flags_out, int *changed,
                                   float eps, float sea, const nz_geom &g, int zlo, int zhi, int first, int pass, int sweeps);
int32_t nz_launch_fill_round_end(hipStream_t s, float *w, const float *w_work, const int *status, int passes, const nz_geom &g);
int32_t nz_launch_fill_stripe_finalise(hipStream_t s, float *h, const float *w, float *depth, const int *converged,
                                       const nz_geom &g);

// drainage area (nz_drainage.hip) on `count` tiles of res^2 cells stored back to back.  mask: one donor byte per cell from
// the heights (bit k: neighbour k drains into the cell).  pass `pass` of the series: A planes a_in -> a_out (pass 0 reads
// none: it derives the start state rain * rain_map, rain_map NULL: rain), tile bytes flags_in -> flags_out, at most `sweeps`
// in-LDS sweeps per tile; status: {passes, converged, changed[3]}, maintained by the launches themselves.  finalise sets
// status[1] and, when the series did not come to rest, writes the start state to `drainage`
int32_t nz_launch_drainage_mask(hipStream_t s, const float *h, unsigned char *donors, float sea, int res, int count);
int32_t nz_launch_drainage_pass(hipStream_t s, const unsigned char *donors, const float *rain_map, const float *a_in,
                                float *a_out, int *status, const unsigned char *flags_in, unsigned char *flags_out, float rain,
                                int res, int count, int pass, int sweeps);
int32_t nz_launch_drainage_finalise(hipStream_t s, float *drainage, const float *rain_map, int *status, float rain, size_t n);
// the stripe form, one round (nz_drainage_stripe_round), between the fill stripe's round_begin and round_end launches: mask stores
// the donor bytes of the owned rows [g.or0, g.or1) at the cells' plane indices, from heights up to two rows beyond them; a pass
// works on the owned rows of stripe-shaped planes against the frozen rows or0 - 1 and or1 of the caller's plane -- a_in of an
// even pass, a_out of an odd one -- or, with first, of rain_c; [zlo, zhi] the global grid in buffer rows; finalise is all or nothing on the owned rows by the caller's verdict
int32_t nz_launch_drainage_stripe_mask(hipStream_t s, const float *h, unsigned char *donors, int *status, float sea,
                                       const nz_geom &g, int zlo, int zhi);
int32_t nz_launch_drainage_stripe_pass(hipStream_t s, const unsigned char *donors, const float *rain_map, const float *a_in,
                                       float *a_out, int *status, const unsigned char *flags_in,
                                       unsigned char *flags_out, int *changed, float rain, const nz_geom &g, int zlo, int zhi,
                                       int first, int pass, int sweeps);
int32_t nz_launch_drainage_stripe_finalise(hipStream_t s, float *a, const float *rain_map, const int *converged, float rain,
                                           const nz_geom &g);

// multiple-flow drainage (nz_drainage_mfd.hip) on `count` tiles of res^2 cells stored back to back.  setup: heights -> eight
// planes of count * res^2 incoming weights each (plane k: what neighbour k sends to the cell, +0: nothing), wts + k * count *
// res^2.  pass: as nz_launch_drainage_pass, the weights in place of the donor bytes.  The finalise launch is
// nz_launch_drainage_finalise
int32_t nz_launch_drainage_mfd_setup(hipStream_t s, const float *h, float *wts, float sea, int res, int count, int exponent);
int32_t nz_launch_drainage_mfd_pass(hipStream_t s, const float *wts, const float *rain_map, const float *a_in, float *a_out,
                                    int *status, const unsigned char *flags_in, unsigned char *flags_out, float rain, int res,
                                    int count, int pass, int sweeps);

// watershed (nz_watershed.hip) on `count` tiles of res^2 cells stored back to back.  receivers: one receiver byte per cell
// from the heights (the code 0..7, or 8 without a receiver).  pass `pass` of the series: label planes b_in -> b_out and,
// when l_out is not NULL, length planes l_in -> l_out (pass 0 reads none: it derives the start state, own index and +0),
// tile bytes flags_in -> flags_out, at most `sweeps` in-LDS sweeps per tile; cell / diag: the step of a straight and of a
// diagonal move; status as in the drainage launches.  finalise sets status[1] and, when the series did not come to rest,
// writes the start state to `basin` and (not NULL) `length`
int32_t nz_launch_watershed_receivers(hipStream_t s, const float *h, unsigned char *recv, float sea, int res, int count);
int32_t nz_launch_watershed_pass(hipStream_t s, const unsigned char *recv, const int *b_in, int *b_out, const float *l_in,
                                 float *l_out, int *status, const unsigned char *flags_in, unsigned char *flags_out,
                                 float cell, float diag, int res, int count, int pass, int sweeps);
int32_t nz_launch_watershed_finalise(hipStream_t s, int *basin, float *length, int *status, int res, size_t n);

// stream order (nz_stream_order.hip) on `count` tiles of res^2 cells stored back to back.  mask: one channel-donor byte per
// cell from the heights and `drainage` (bit k: neighbour k drains into the cell and is a channel cell; drainage NULL: every
// cell is one), and the start state ch ? 1 : 0 to `order`.  pass `pass` of the series: order planes o_in -> o_out and, when
// l_out is not NULL, link planes l_in -> l_out (pass 0 reads the start state from o_in and no link plane: it derives
// ch ? own index : -1), tile bytes flags_in -> flags_out, at most `sweeps` in-LDS sweeps per tile; status as in the
// drainage launches.  finalise sets status[1] and, when the series did not come to rest, writes the start state to
// `order` and (not NULL) `link`
int32_t nz_launch_stream_mask(hipStream_t s, const float *h, const float *drainage, unsigned char *donors,
                              unsigned char *order, float sea, float threshold, int res, int count);
int32_t nz_launch_stream_pass(hipStream_t s, const unsigned char *donors, const unsigned char *o_in, unsigned char *o_out,
                              const int *l_in, int *l_out, int *status, const unsigned char *flags_in,
                              unsigned char *flags_out, int res, int count, int pass, int sweeps);
int32_t nz_launch_stream_finalise(hipStream_t s, unsigned char *order, int *link, const float *drainage, int *status,
                                  float threshold, int res, size_t n);

// implicit fluvial erosion (nz_fluvial_implicit.hip) on `count` tiles of res^2 cells stored back to back.  begin: status[5]
// (ST_GO) from the caller's `proceed` word (NULL: go) and the status words of a fresh series; with ST_GO == 0 every later
// launch returns at once.  setup: heights, drainage `area` and the maps (NULL: none) -> one receiver byte per cell and the
// coefficient planes bco, fco.  pass `pass` of the series: h' planes h_in -> h_out (pass 0 reads none: it starts from bco),
// tile bytes flags_in -> flags_out, at most `sweeps` in-LDS sweeps per tile; status as in the drainage launches.  finalise
// sets status[1], adds {1, passes} to `tally` (NULL: off) when the series came to rest, and otherwise writes h to `out`
int32_t nz_launch_fluvial_implicit_begin(hipStream_t s, int *status, const int *proceed);
int32_t nz_launch_fluvial_implicit_setup(hipStream_t s, const float *h, const float *area, const float *hardness,
                                         const float *uplift_map, unsigned char *recv, float *bco, float *fco,
                                         const int *status, float erodibility, float uplift, float dt, float sea, int res,
                                         int count);
int32_t nz_launch_fluvial_implicit_pass(hipStream_t s, const unsigned char *recv, const float *bco, const float *fco,
                                        const float *h_in, float *h_out, int *status, const unsigned char *flags_in,
                                        unsigned char *flags_out, int res, int count, int pass, int sweeps);
int32_t nz_launch_fluvial_implicit_finalise(hipStream_t s, const float *h, float *out, int *status, int *tally, size_t n);
// the stripe form, one round (nz_implicit_fluvial_stripe_round), between the fill stripe's round_begin and round_end launches:
// setup stores the receiver byte, b and f of the owned rows [g.or0, g.or1) at the cells' plane indices, from heights up to one
// row beyond them; a pass works on the owned rows of stripe-shaped planes against the frozen rows or0 - 1 and or1 of the
// caller's plane -- h_in of an even pass, h_out of an odd one -- or, with first, of ghost_h, the heights; [zlo, zhi] the
// global grid in buffer rows; finalise is all or nothing on the owned rows by the caller's verdict
int32_t nz_launch_fluvial_implicit_stripe_setup(hipStream_t s, const float *h, const float *area, const float *hardness,
                                                const float *uplift_map, unsigned char *recv, float *bco, float *fco,
                                                const int *status, float erodibility, float uplift, float dt, float sea,
                                                const nz_geom &g, int zlo, int zhi);
int32_t nz_launch_fluvial_implicit_stripe_pass(hipStream_t s, const unsigned char *recv, const float *bco, const float *fco,
                                               const float *h_in, float *h_out, const float *ghost_h, int *status,
                                               const unsigned char *flags_in, unsigned char *flags_out, int *changed,
                                               const nz_geom &g, int zlo, int zhi, int first, int pass, int sweeps);
int32_t nz_launch_fluvial_implicit_stripe_finalise(hipStream_t s, const float *h, float *out, const int *converged,
                                                   const nz_geom &g);

// multiple-flow implicit fluvial erosion (nz_fluvial_implicit_mfd.hip); begin and finalise are the two launches above.
// setup: heights, drainage `area` and the maps (NULL: none) -> one gate byte per cell (bit k: the weight towards neighbour k
// is > 0), the plane bco and the eight planes fco (plane k at k * count * res^2).  pass: as nz_launch_fluvial_implicit_pass
int32_t nz_launch_fluvial_implicit_mfd_setup(hipStream_t s, const float *h, const float *area, const float *hardness,
                                             const float *uplift_map, unsigned char *gate, float *bco, float *fco,
                                             const int *status, float erodibility, float uplift, float dt, float sea, int res,
                                             int count, int exponent);
int32_t nz_launch_fluvial_implicit_mfd_pass(hipStream_t s, const unsigned char *gate, const float *bco, const float *fco,
                                            const float *h_in, float *h_out, int *status, const unsigned char *flags_in,
                                            unsigned char *flags_out, int res, int count, int pass, int sweeps);

// implicit fluvial erosion with sediment deposition (nz_fluvial_sediment.hip); the setup and the solve passes are the
// implicit launches above, on the status words `solve`.  begin: totals {passes, converged, residual} = 0 and `solve` as the
// implicit begin.  mask: one donor byte per cell (behind solve[ST_GO]).  source: e = b0 - hprev, the status words `accum` of a
// fresh accumulation series whose ST_GO is the verdict on `solve`, whose passes join the totals.  gather_pass: pass `pass` of
// Q, planes q_in -> q_out (pass 0 reads none: it starts from e), as the drainage pass.  deposit: bk (may be e) from the final
// Q, fresh `solve` words whose ST_GO is the verdict on `accum`.  finalise: the verdict, totals, tally, the residual against
// hprev (NULL: none), flux = q (NULL: +0) when flux is not NULL, and out = h when the call did not come to rest
int32_t nz_launch_fluvial_sediment_begin(hipStream_t s, int *totals, int *solve, const int *proceed);
int32_t nz_launch_fluvial_sediment_mask(hipStream_t s, const float *h, unsigned char *donors, const int *solve, float sea,
                                        int res, int count);
int32_t nz_launch_fluvial_sediment_source(hipStream_t s, const float *b0, const float *hprev, float *e, const int *solve,
                                          int *accum, int *totals, size_t n);
int32_t nz_launch_fluvial_sediment_gather_pass(hipStream_t s, const unsigned char *donors, const float *e, const float *q_in,
                                               float *q_out, int *status, const unsigned char *flags_in,
                                               unsigned char *flags_out, int res, int count, int pass, int sweeps);
int32_t nz_launch_fluvial_sediment_deposit(hipStream_t s, const unsigned char *donors, const float *q, const float *b0,
                                           const float *area, const float *h, float *bk, const int *accum, int *solve,
                                           int *totals, float deposition, float sea, int res, int count);
int32_t nz_launch_fluvial_sediment_finalise(hipStream_t s, const float *h, float *out, const float *hprev, const float *q,
                                            float *flux, const int *solve, int *totals, int *tally, size_t n);

// hillslope diffusion (nz_hillslope.hip).  tables: inv[i] and cp[i], i = 1 .. res-2, of r (res floats each; res >= 3).
// step: one step on `count` tiles of res^2 cells stored back to back, `in` -> `out` (the same pointer: in place; otherwise
// disjoint), as three launches: the rows' forward sweep, their backward sweep, the columns' two sweeps
int32_t nz_launch_hillslope_tables(hipStream_t s, float *inv, float *cp, float r, int res);
int32_t nz_launch_hillslope_step(hipStream_t s, const float *in, float *out, const float *inv, const float *cp, float r,
                                 int res, int count);

// resampling (nz_resample.hip).  One geometry for the tile, batch and stripe forms: `c` names the coarse plane, `f` the fine
// one; buffer row b of a plane is global row b + grow0 of its grid; fine grid = factor x coarse grid
struct nz_up_geom {
    int ccols, cpitch, crows;  // the coarse buffer
    int cgrow0, cgrows;        // its first global row, the coarse grid's rows (the clamp range of row reads)
    int fcols, fpitch;         // the fine buffer
    int fgrow0;                // its first global row
    int w0, w1;                // fine buffer rows to produce [w0, w1)
    size_t cstride, fstride;   // floats between the planes of a batch
    int cz_first, cz_last;     // (set by the launcher) global coarse rows of the window
    int rd0, rd1;              // (set by the launcher) coarse buffer rows the window's taps read, inclusive
};
struct nz_down_geom {
    int ccols, cpitch, cgrow0;  // the coarse (output) buffer
    int fpitch, fgrow0;         // the fine (input) buffer
    int w0, w1;                 // coarse buffer rows to produce [w0, w1)
    size_t cstride, fstride;
};
int nz_resample_halo(int filter);  // coarse rows an upsampled row reads beyond its own: 0 nearest, 1 bilinear, 2 Catmull-Rom
// base: NULL, dst itself or a plane apart from dst.  NZ_ERR_INVALID when a coarse row the window reads is not in the buffer
int32_t nz_launch_upsample(hipStream_t s, const float *src, float *dst, const float *base, nz_up_geom g, int factor,
                           int filter, int count);
int32_t nz_launch_downsample(hipStream_t s, const float *src, float *dst, const nz_down_geom &g, int factor, int count);

int32_t nz_launch_mesh_planar(hipStream_t s, void *vertices, uint32_t *indices, int res);
int32_t nz_launch_mesh(hipStream_t s, int meshType, void *vertices, uint32_t *indices, int res, int in_res,
                       float tile_height, float tile_size, const float *heights, int count = 1, int index16 = 0);

// element-wise stages (nz_elementwise.hip)
int32_t nz_launch_constant(hipStream_t s, int op, float *data, size_t n, float c);
int32_t nz_launch_reduce(hipStream_t s, int op, float *l, const float *r, size_t n);
int32_t nz_launch_flow_from_track(hipStream_t s, float *pool, float *flow, float *track, size_t n, float flowLossRate,
                                  float evaporation);
// drain_hdr / drain_data (nullable): the particle queue a drained pool leaves through (PoolAutomataJob, drainParticles)
size_t nz_map_range_scratch_floats();
int32_t nz_launch_map_range(hipStream_t s, const float *map, size_t n, float lim_min, float lim_max, float *res, void *scratch);
int32_t nz_launch_normalize_args(hipStream_t s, float *data, size_t n, const float *args);
// gathered {min, max, range} triples -> mins[n], maxs[n]; {lo[0], hi[1]} -> res = {min, max, max - min}
int32_t nz_launch_range_split(hipStream_t s, const float *triples, int n, float *mins, float *maxs);
int32_t nz_launch_range_compose(hipStream_t s, const float *lo, const float *hi, float *res);
size_t nz_pool_automata_mask_words(int res);
int32_t nz_launch_pool_automata_masks(hipStream_t s, const float *pool, int res, unsigned *mask, int *ctl, int with_list);
int32_t nz_launch_pool_automata_clean(hipStream_t s, const float *pool, int res, unsigned *mask, int *ctl);
int32_t nz_launch_pool_automata_pass(hipStream_t s, float *pool, const float *height, int res, int xoff, int zoff,
                                     int32_t *drain_hdr = nullptr, nz_particle *drain_data = nullptr,
                                     unsigned *mask = nullptr, int *ctl = nullptr);
// the whole job as one launch of one workgroup, from the list of non-empty mask words (nz_elementwise.hip)
int32_t nz_launch_pool_automata_sparse(hipStream_t s, float *pool, const float *height, int res, int iterations, int limit,
                                       int dense_follows, int32_t *drain_hdr, nz_particle *drain_data, unsigned *mask, int *ctl,
                                       unsigned long long *hint_dev, unsigned long long seq);
int32_t *nz_particle_queue_hdr(nz_particle_queue *q);
nz_particle *nz_particle_queue_data(nz_particle_queue *q);
int32_t nz_launch_crop(hipStream_t s, const float *in, int in_res, float *out, int out_res);
int32_t nz_launch_curve(hipStream_t s, float *data, size_t n, const float *curve, int curveSize);
bool nz_thermal_pair_fits(int resolution);
int32_t nz_launch_thermal_pair(hipStream_t s, float *data, int resolution, int zodd, float maxDiff, float increment);
int32_t nz_launch_thermal_phase(hipStream_t s, float *data, int resolution, int flip, float maxDiff, float increment);
