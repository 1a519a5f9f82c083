// nz_hydraulic.hip -- grid hydraulic erosion with sediment transport (gfx950; new-framework feature, the stage
// Geologic/Stage/ErosionStageSubtractiveFlow.cs leaves commented out).  The model is stated in include/noize_hip.h and
// restated step by step in tests/hydraulic_ref.py; the pipe-model flux, the water update and the discharge are the flow
// map's own arithmetic (nz_flow_common.hpp), so with capacity 0 the water and flux are the flow map's state bit for bit.
//
// One launch per iteration.  A workgroup produces an HX x HZ tile of one plane and stages its halo through LDS:
//   fill     heights b and water d1 = d + rain on the tile at radius 3
//   phase A  the new flux (compute_flow) at radius 2
//   phase B  discharge, slope, erosion / deposition and the sediment's outflows a_X at radius 1
//   phase C  the water update and the sediment's in-flow on the tile itself
// Every LDS cell holds the value of the clamped plane cell it stands for: a cell beyond the border is a copy of the border
// cell, and a clamped neighbour read is a read at the clamped plane coordinate -- which always lies inside the next larger
// radius -- so the clamp-to-edge reads are the flow map's.  The sediment's in-flow alone reads unclamped neighbours (0
// beyond the border).  Strict IEEE binary32 in every float mode, no contraction (-ffp-contract=off, Makefile); every step
// is a radius-1 stencil with no atomics, so the result is independent of the launch shape.
//
// The _ex entries' options are compile-time flags of the same kernel (OPT = NZ_HYD_OPEN | NZ_HYD_MAPS | NZ_HYD_MASKS); with
// all of them off it is the kernel above with the same arguments, and keeps its own four instantiations:
//   OPEN   open border: a neighbour beyond the border stands at the border cell's bed height in the flux (phase A) and
//          sends nothing back in the water update (phase C).  "Beyond the border" is a test on the plane coordinate of
//          the cell an LDS cell stands for, so the halo copies of a border cell compute the border cell's own flux
//   MAPS   rain map (read in the fill, radius 3, clamped coordinates like b) and hardness map.  The hardness scales the
//          erosion of every cell whose sediment the tile reads -- radius 1 -- so it is read straight from the plane at the
//          clamped coordinate in phase B, next to the cell's sediment, and takes no LDS.  A NULL map of the pair reads
//          as ones / zeros, which is the no-map arithmetic bit for bit (rain * 1, dissolve * (1 - 0))
//   MASKS  wear / deposits: phase B leaves the tile cell's e of this iteration in LDS (WE / DE, +0 in the branch not
//          taken), phase C's owner of the cell adds it to the plane: a read-modify-write of one element by one thread
//
// The stripe form (nz_hydraulic_stripe) is one more compile-time flag of the same kernel, STRIPE, with the stripe's geometry
// as a trailing argument: columns clamp to [0, cols-1] and rows to [zc0, zc1] -- the global border in buffer rows -- so
// "beyond the border" is a test against that range; rows are `pitch` floats apart; the launch produces buffer rows
// [w0, w1) only, blockIdx.y counting 16-row tiles from w0; the masks are updated on rows [m0, m1) only (the owned rows: the
// ghost rows of a widened window are recomputed by two ranks and must not be summed twice); no batch.  Every arithmetic
// statement is shared with the tile form.
#include "nz_internal.hpp"
#include "nz_flow_common.hpp"

namespace {

constexpr int HX = 64, HZ = 16;  // tile produced by one workgroup
constexpr int HT = 512;          // threads: 8 waves
constexpr int HR = 3;           // halo radius of the staged state
constexpr int LW = HX + 2 * HR, LH = HZ + 2 * HR, LN = LW * LH;

// the stripe form's geometry (nz_geom_from_stripe), the window of this launch and the rows whose masks it updates
struct hyd_stripe {
    int cols, pitch;
    int zc0, zc1;  // inclusive clamp range of row reads: the global border in buffer rows
    int w0, w1;    // rows produced [w0, w1)
    int m0, m1;    // rows whose wear / deposits are updated [m0, m1)
};
// the trailing kernel arguments: none, the options' planes, or the options' planes and the stripe's geometry
struct hyd_extra {
    nz_hydraulic_ex x;
    hyd_stripe g;
};
__device__ __forceinline__ hyd_extra hyd_extra_of() { return hyd_extra{}; }
__device__ __forceinline__ hyd_extra hyd_extra_of(const nz_hydraulic_ex &x) { return hyd_extra{x, {}}; }
__device__ __forceinline__ hyd_extra hyd_extra_of(const nz_hydraulic_ex &x, const hyd_stripe &g) { return hyd_extra{x, g}; }

// tie-keeping selects (tests/hydraulic_ref.py): max(lo, v) keeps lo unless v is larger, min(a, c) keeps a unless c is smaller
__device__ __forceinline__ float smax(float lo, float v) { return v > lo ? v : lo; }
__device__ __forceinline__ float smin(float a, float c) { return c < a ? c : a; }

// FIRST: the state is the start state (water initialWater, no sediment, no flux) and `in` is not read.
// LAST: the launch writes b + s to h_out and the water to out[0] only.
// OPT: the _ex options (above).  STRIPE: the stripe form (above); `res` is not read.
// X: nothing; one nz_hydraulic_ex with the options' planes when OPT != 0; that and a hyd_stripe when STRIPE.
template <bool FIRST, bool LAST, int OPT = 0, bool STRIPE = false, class... X>
__global__ __launch_bounds__(HT) void hydraulic_kernel(const float *__restrict__ h_in, float *__restrict__ h_out,
                                                       nz_hydraulic_planes p, nz_hydraulic_params k, int res, X... xs) {
    static_assert(sizeof...(X) == (STRIPE ? 2 : OPT ? 1 : 0), "the trailing arguments travel with OPT != 0 / STRIPE only");
    constexpr bool OPEN = (OPT & NZ_HYD_OPEN) != 0, MAPS = (OPT & NZ_HYD_MAPS) != 0, MASKS = (OPT & NZ_HYD_MASKS) != 0;
    const hyd_extra extra = hyd_extra_of(xs...);
    const nz_hydraulic_ex &x = extra.x;
    const hyd_stripe &g = extra.g;
    __shared__ float B[LN], D1[LN];           // radius 3
    __shared__ float FN[LN], FS[LN], FE[LN], FW[LN];  // radius 2 (same layout)
    __shared__ float AN[LN], AS[LN], AE[LN], AW[LN];  // radius 1 (same layout)
    __shared__ float BN[HX * HZ], PS[HX * HZ];        // the tile: eroded height, s - out
    __shared__ float WE[MASKS ? HX * HZ : 1], DE[MASKS ? HX * HZ : 1];  // the tile: this iteration's wear, deposit

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * HX, z0 = STRIPE ? g.w0 + blockIdx.y * HZ : blockIdx.y * HZ;
    const int pitch = STRIPE ? g.pitch : res;
    const size_t base = STRIPE ? 0 : (size_t)blockIdx.z * res * res;
    // the clamp ranges: the border of the tile, or the global border seen from the stripe's buffer
    const int xhi = STRIPE ? g.cols - 1 : res - 1;
    const int zlo = STRIPE ? g.zc0 : 0, zhi = STRIPE ? g.zc1 : res - 1;
    // LDS column / row of plane column / row v (v within the staged radius)
    auto lx_of = [&](int v) { return v - x0 + HR; };
    auto lz_of = [&](int v) { return v - z0 + HR; };

    // ---- fill: radius 3 ----
    for (int i = tid; i < LN; i += HT) {
        const int lz = i / LW, lx = i - lz * LW;
        const int px = clampi(x0 - HR + lx, 0, xhi), pz = clampi(z0 - HR + lz, zlo, zhi);
        const size_t c = base + (size_t)pz * pitch + px;
        B[i] = h_in[c];
        if (MAPS) D1[i] = (FIRST ? k.initial_water : p.in[0][c]) + k.rain * (x.rain_map ? x.rain_map[c] : 1.0f);
        else D1[i] = (FIRST ? k.initial_water : p.in[0][c]) + k.rain;
    }
    __syncthreads();

    // ---- phase A: new flux at radius 2 (ComputeFlowStep with water_0 = d1) ----
    for (int i = tid; i < (LW - 2) * (LH - 2); i += HT) {
        const int lz = 1 + i / (LW - 2), lx = 1 + i % (LW - 2);
        const int px = clampi(x0 - HR + lx, 0, xhi), pz = clampi(z0 - HR + lz, zlo, zhi);
        const int l = lz * LW + lx;
        const int lW = lz * LW + lx_of(clampi(px - 1, 0, xhi)), lE = lz * LW + lx_of(clampi(px + 1, 0, xhi));
        const int lS = lz_of(clampi(pz - 1, zlo, zhi)) * LW + lx, lN = lz_of(clampi(pz + 1, zlo, zhi)) * LW + lx;
        flux4 old{0.0f, 0.0f, 0.0f, 0.0f};
        if (!FIRST) {
            const size_t c = base + (size_t)pz * pitch + px;
            old.w = p.in[5][c];
            old.e = p.in[4][c];
            old.s = p.in[3][c];
            old.n = p.in[2][c];
        }
        // totalHt = water + height, as nzo_flow_step / flow_step_kernel add them
        flux4 f;
        if (OPEN) {  // beyond the border: the border cell's own bed with no water on it
            const float b = B[l];
            f = compute_flow(D1[l] + b, D1[l], px - 1 < 0 ? b : D1[lW] + B[lW], px + 1 > xhi ? b : D1[lE] + B[lE],
                             pz - 1 < zlo ? b : D1[lS] + B[lS], pz + 1 > zhi ? b : D1[lN] + B[lN], old);
        } else {
            f = compute_flow(D1[l] + B[l], D1[l], D1[lW] + B[lW], D1[lE] + B[lE], D1[lS] + B[lS], D1[lN] + B[lN], old);
        }
        FW[l] = f.w;
        FE[l] = f.e;
        FS[l] = f.s;
        FN[l] = f.n;
    }
    __syncthreads();

    // ---- phase B: discharge, slope, erosion / deposition, sediment outflows at radius 1 ----
    for (int i = tid; i < (LW - 4) * (LH - 4); i += HT) {
        const int lz = 2 + i / (LW - 4), lx = 2 + i % (LW - 4);
        const int px = clampi(x0 - HR + lx, 0, xhi), pz = clampi(z0 - HR + lz, zlo, zhi);
        const int l = lz * LW + lx;
        const int lW = lz * LW + lx_of(clampi(px - 1, 0, xhi)), lE = lz * LW + lx_of(clampi(px + 1, 0, xhi));
        const int lS = lz_of(clampi(pz - 1, zlo, zhi)) * LW + lx, lN = lz_of(clampi(pz + 1, zlo, zhi)) * LW + lx;
        // CreateVelocityField's magnitude (normalised by min 0, range 1: the identity)
        const float q = velocity_norm_m<false>(FE[lW] - FW[l], FE[l] - FW[lE], FS[lN] - FN[l], FS[l] - FN[lS], 0.0f, 1.0f,
                                               1.0f);
        const float b = B[l];
        const float bW = B[lW], bE = B[lE], bS = B[lS], bN = B[lN];
        const float gx = (bE - bW) * 0.5f;
        const float gz = (bN - bS) * 0.5f;
        const float g2 = gx * gx + gz * gz;
        const float S = smax(k.min_tilt, sqrtf(g2 / (1.0f + g2)));
        const float C = (k.capacity * q) * S;
        float s = FIRST ? 0.0f : p.in[1][base + (size_t)pz * pitch + px];
        float kd = k.dissolve;
        if (MAPS) kd = k.dissolve * (1.0f - (x.hardness ? x.hardness[base + (size_t)pz * pitch + px] : 0.0f));
        float bb, we = 0.0f, de = 0.0f;  // this iteration's wear / deposit of the cell: e in the branch taken
        if (C > s) {
            const float bmin4 = smin(smin(smin(bW, bE), bS), bN);
            const float e = smin(kd * (C - s), smax(0.0f, b - bmin4));
            bb = b - e;
            s = s + e;
            we = e;
        } else {
            const float e = k.deposit * (s - C);
            bb = b + e;
            s = s - e;
            de = e;
        }
        const float d1 = D1[l];
        const float r = d1 >= 0x1p-126f ? TIMESTEP / d1 : 0.0f;  // the smallest normal: DT / d1 stays finite
        const float aW = s * (FW[l] * r), aE = s * (FE[l] * r), aS = s * (FS[l] * r), aN = s * (FN[l] * r);
        AW[l] = aW;
        AE[l] = aE;
        AS[l] = aS;
        AN[l] = aN;
        const int tx = lx - HR, tz = lz - HR;
        if (tx >= 0 && tx < HX && tz >= 0 && tz < HZ) {
            BN[tz * HX + tx] = bb;
            PS[tz * HX + tx] = s - (((aW + aE) + aS) + aN);
            if (MASKS) {
                WE[tz * HX + tx] = we;
                DE[tz * HX + tx] = de;
            }
        }
    }
    __syncthreads();

    // ---- phase C: water update and sediment in-flow on the tile ----
    for (int i = tid; i < HX * HZ; i += HT) {
        const int tz = i / HX, tx = i % HX;
        const int px = x0 + tx, pz = z0 + tz;
        if (px > xhi || pz > (STRIPE ? g.w1 - 1 : zhi)) continue;
        const int lx = tx + HR, lz = tz + HR;
        const int l = lz * LW + lx;
        const int lW = lz * LW + lx_of(clampi(px - 1, 0, xhi)), lE = lz * LW + lx_of(clampi(px + 1, 0, xhi));
        const int lS = lz_of(clampi(pz - 1, zlo, zhi)) * LW + lx, lN = lz_of(clampi(pz + 1, zlo, zhi)) * LW + lx;
        const flux4 own{FW[l], FE[l], FS[l], FN[l]};
        float d2;
        if (OPEN)  // nothing comes back from beyond the border
            d2 = update_water(D1[l], own, px > 0 ? FE[lW] : 0.0f, px < xhi ? FW[lE] : 0.0f, pz > zlo ? FN[lS] : 0.0f,
                              pz < zhi ? FS[lN] : 0.0f);
        else d2 = update_water(D1[l], own, FE[lW], FW[lE], FN[lS], FS[lN]);
        // in-flow: 0 from beyond the border (with a closed border no flux leaves the tile, so the sediment is conserved)
        const float inW = px > 0 ? AE[l - 1] : 0.0f;
        const float inE = px < xhi ? AW[l + 1] : 0.0f;
        const float inS = pz > zlo ? AN[l - LW] : 0.0f;
        const float inN = pz < zhi ? AS[l + LW] : 0.0f;
        const float s = smax(0.0f, PS[i] + (((inW + inE) + inS) + inN));
        const float d = d2 * k.keep;
        const size_t c = base + (size_t)pz * pitch + px;
        if (LAST) {
            h_out[c] = BN[i] + s;
            p.out[0][c] = d;
        } else {
            h_out[c] = BN[i];
            p.out[0][c] = d;
            p.out[1][c] = s;
            p.out[2][c] = own.n;
            p.out[3][c] = own.s;
            p.out[4][c] = own.e;
            p.out[5][c] = own.w;
        }
        if (MASKS && (!STRIPE || (pz >= g.m0 && pz < g.m1))) {  // running sums in iteration order from +0; the settled sediment joins the deposits last
            if (x.wear) x.wear[c] = (FIRST ? 0.0f : x.wear[c]) + WE[i];
            if (x.deposits) {
                const float dep = (FIRST ? 0.0f : x.deposits[c]) + DE[i];
                x.deposits[c] = LAST ? dep + s : dep;
            }
        }
    }
}

// launches hydraulic_kernel<FIRST, LAST, opt> for opt in 1 .. 7
template <bool FIRST, bool LAST, int OPT = 7>
void launch_ex(int opt, dim3 grid, hipStream_t s, const float *h_in, float *h_out, const nz_hydraulic_planes &p,
               const nz_hydraulic_params &k, int res, const nz_hydraulic_ex &x) {
    if constexpr (OPT > 0) {
        if (opt == OPT) NZ_LAUNCH((hydraulic_kernel<FIRST, LAST, OPT, false, nz_hydraulic_ex>), grid, dim3(HT), 0, s, h_in, h_out, p, k, res, x);
        else launch_ex<FIRST, LAST, OPT - 1>(opt, grid, s, h_in, h_out, p, k, res, x);
    }
}

// launches the stripe form hydraulic_kernel<FIRST, LAST, opt, true> for opt in 0 .. 7
template <bool FIRST, bool LAST, int OPT = 7>
void launch_stripe(int opt, dim3 grid, hipStream_t s, const float *h_in, float *h_out, const nz_hydraulic_planes &p,
                   const nz_hydraulic_params &k, const nz_hydraulic_ex &x, const hyd_stripe &g) {
    if (opt == OPT) NZ_LAUNCH((hydraulic_kernel<FIRST, LAST, OPT, true, nz_hydraulic_ex, hyd_stripe>), grid, dim3(HT), 0, s, h_in, h_out, p, k, 0, x, g);
    else if constexpr (OPT > 0) launch_stripe<FIRST, LAST, OPT - 1>(opt, grid, s, h_in, h_out, p, k, x, g);
}

}  // namespace

int32_t nz_launch_hydraulic_stripe(hipStream_t s, const float *h_in, float *h_out, const nz_hydraulic_planes &p,
                                   const nz_hydraulic_params &k, const nz_geom &geom, int own0, int own1, int first,
                                   int last, const nz_hydraulic_ex &ex) {
    if (geom.cols <= 0 || geom.or1 <= geom.or0) return NZ_OK;
    // the window lies inside the clamp range, so every staged row is a row of the buffer and every tile reads its own halo
    NZ_REQUIRE(geom.or0 >= geom.zc0 && geom.or1 <= geom.zc1 + 1 && geom.zc0 >= 0 && geom.zc1 < geom.rows &&
                   geom.pitch >= geom.cols,
               "hydraulic stripe: rows [%d, %d) outside the clamp range [%d, %d]", geom.or0, geom.or1, geom.zc0, geom.zc1);
    const hyd_stripe g{geom.cols, geom.pitch, geom.zc0, geom.zc1, geom.or0, geom.or1, own0, own1};
    const dim3 grid((g.cols + HX - 1) / HX, (g.w1 - g.w0 + HZ - 1) / HZ, 1);
    const int opt = (ex.open ? NZ_HYD_OPEN : 0) | (ex.rain_map || ex.hardness ? NZ_HYD_MAPS : 0) |
                    (ex.wear || ex.deposits ? NZ_HYD_MASKS : 0);
    if (first && last) launch_stripe<true, true>(opt, grid, s, h_in, h_out, p, k, ex, g);
    else if (first) launch_stripe<true, false>(opt, grid, s, h_in, h_out, p, k, ex, g);
    else if (last) launch_stripe<false, true>(opt, grid, s, h_in, h_out, p, k, ex, g);
    else launch_stripe<false, false>(opt, grid, s, h_in, h_out, p, k, ex, g);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_hydraulic(hipStream_t s, const float *h_in, float *h_out, const nz_hydraulic_planes &p,
                            const nz_hydraulic_params &k, int res, int count, int first, int last,
                            const nz_hydraulic_ex *ex) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid((res + HX - 1) / HX, (res + HZ - 1) / HZ, count);
    const int opt = !ex ? 0
                        : (ex->open ? NZ_HYD_OPEN : 0) | (ex->rain_map || ex->hardness ? NZ_HYD_MAPS : 0) |
                              (ex->wear || ex->deposits ? NZ_HYD_MASKS : 0);
    if (opt) {
        if (first && last) launch_ex<true, true>(opt, grid, s, h_in, h_out, p, k, res, *ex);
        else if (first) launch_ex<true, false>(opt, grid, s, h_in, h_out, p, k, res, *ex);
        else if (last) launch_ex<false, true>(opt, grid, s, h_in, h_out, p, k, res, *ex);
        else launch_ex<false, false>(opt, grid, s, h_in, h_out, p, k, res, *ex);
    } else if (first && last) NZ_LAUNCH((hydraulic_kernel<true, true>), grid, dim3(HT), 0, s, h_in, h_out, p, k, res);
    else if (first) NZ_LAUNCH((hydraulic_kernel<true, false>), grid, dim3(HT), 0, s, h_in, h_out, p, k, res);
    else if (last) NZ_LAUNCH((hydraulic_kernel<false, true>), grid, dim3(HT), 0, s, h_in, h_out, p, k, res);
    else NZ_LAUNCH((hydraulic_kernel<false, false>), grid, dim3(HT), 0, s, h_in, h_out, p, k, res);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
