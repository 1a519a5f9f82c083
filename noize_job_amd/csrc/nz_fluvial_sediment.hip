// nz_fluvial_sediment.hip -- sediment deposition on top of the implicit stream-power step: the xi-q model (Yuan, Braun,
// Guerit, Rouby & Cordonnier 2019) as K Gauss-Seidel iterations around nz_fluvial_implicit's solve (gfx950; new-framework
// feature).
//
// THE MODEL (include/noize_hip.h states it for the caller, tests/fluvial_sediment_ref.py restates it as walks):
//   Tile, neighbours, outlets, receivers r(c), du, kc, b0, f and invL are nz_fluvial_implicit's; A is the caller's drainage
//   plane, G = deposition, K = iterations.  solve(b): h' = b without a receiver, else (b + f * h'[q]) / (1 + f).
//     h0 = solve(b0)
//     k = 1 .. K:  e = b0 - h(k-1);   Q[c] = e[c] + Q[d] over the donors d of c, k ascending;
//                  Qin[c] = +0 + Q[d] over the same donors, then Qin < 0 ? +0 : Qin;
//                  bk = b0 on outlets and where not A > 0, else b0 + (G * Qin) / A;   hk = solve(bk)
//   every operation rounded once, no contraction.  Q is a fixed function of the final values of strictly higher cells, a
//   solve of strictly lower ones: both fixed points are unique and every schedule ends in the same bits.
//
// What is here and what is not.  The receiver byte, b0 and f come from nz_fluvial_implicit's setup launch and every solve
// pass IS nz_fluvial_implicit's pass launch, given the plane bk in place of b0 (nz_launch_fluvial_implicit_setup / _pass:
// that file and its code objects are untouched).  This file adds what lies between the solves:
//   begin     one thread: the totals {passes, converged, residual} = 0 and the solve's status words as the parent's begin.
//   mask      once per call: nz_donor_front.hpp's donor byte per cell, behind the solve's ST_GO.
//   source    once per k: the verdict on solve series k - 1 becomes ST_GO of the accumulation's status words (a fresh
//             series), its passes join the total, and e = b0 - h(k-1) per cell.
//   gather    one launch per PASS of Q by the pass protocol of nz_relax_pass.hpp on the tiles of nz_tile64.hpp: the drainage
//             stage's downstream gather with the plane e as its per-cell source.  The first pass reads no Q plane.
//   deposit   once per k: the verdict on the accumulation becomes ST_GO of a fresh solve series; Q at radius 1 into LDS, Qin
//             gathered from +0 by the donor byte, bk written over e (which no launch reads again).
//   finalise  the verdict of the last solve -- with ST_GO handed on from series to series it is the verdict of all 2K + 1
//             -- the totals, the caller's tally, the residual max |hK - h(K-1)| as one launch-wide maximum of non-negative
//             float bits (a vector atomic), the flux copy; when the call did not come to rest or did not run, out = h.
// Every series starts from its right-hand side (bk, e), as the parent does: the start state decides pass counts only.
// The solve series 0 .. K - 1 alternate between two planes of `work`, series K between the caller's `out` and the second of
// them: the first keeps h(K-1) for the residual, and nothing is written to `out` before the last series.
#include "nz_internal.hpp"
#include "nz_receiver.hpp"
#include "nz_relax_pass.hpp"
#include "nz_tile64.hpp"
#include "nz_donor_front.hpp"

namespace {

using namespace nz_tile64;  // the tile, its LDS layout, ring_cell
using namespace nz_relax;   // the status words and the pass protocol

constexpr int TOT_PASSES = 0, TOT_CONVERGED = 1, TOT_RESIDUAL = 2;  // the totals: the first three words of `work`

__device__ __forceinline__ void fresh_series(int *status, int go) {
    status[ST_GO] = go;
    status[ST_PASSES] = 0;
    status[ST_CONVERGED] = 0;
    status[ST_CHANGED] = status[ST_CHANGED + 1] = status[ST_CHANGED + 2] = 0;
}

// did the series these words belong to run and come to rest?
__device__ __forceinline__ bool series_done(const int *status) { return status[ST_GO] != 0 && series_at_rest(status); }

__global__ void sediment_begin_kernel(int *totals, int *solve, const int *proceed) {
    totals[TOT_PASSES] = totals[TOT_CONVERGED] = totals[TOT_RESIDUAL] = 0;
    fresh_series(solve, proceed ? *proceed != 0 : 1);
}

template <bool VEC, bool WORD>
__global__ __launch_bounds__(FT) void sediment_mask_kernel(const float *__restrict__ h, unsigned char *__restrict__ donors,
                                                           const int *solve, float sea, int res) {
    if (!solve[ST_GO]) return;
    nz_front::donor_front<VEC, WORD, false, false>(h, nullptr, donors, nullptr, sea, 0.0f, res, nz_front::win_rows{});
}

// ---- source: e = b0 - h(k-1), and a fresh accumulation series ----
__global__ __launch_bounds__(256) void sediment_source_kernel(const float *__restrict__ b0, const float *__restrict__ hprev,
                                                              float *__restrict__ e, const int *solve, int *accum,
                                                              int *totals, size_t n) {
    const bool go = series_done(solve);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        fresh_series(accum, go ? 1 : 0);
        if (solve[ST_GO]) totals[TOT_PASSES] += solve[ST_PASSES];
    }
    if (i >= n || !go) return;
    e[i] = b0[i] - hprev[i];
}

// ---- a pass of Q ----
// FIRST: the start state e, no Q plane is read; VEC: 16-byte accesses to the float planes and a 32-bit one to the donor
// bytes (all planes 16-byte aligned, the bytes 4-byte, res % 4 == 0)
template <bool FIRST, bool VEC>
__global__ __launch_bounds__(FT) void sediment_gather_pass_kernel(const unsigned char *__restrict__ donors,
                                                                  const float *__restrict__ e, const float *__restrict__ q_in,
                                                                  float *__restrict__ q_out, int *status,
                                                                  const unsigned char *__restrict__ flags_in,
                                                                  unsigned char *__restrict__ flags_out, int res, int pass,
                                                                  int sweeps) {
    __shared__ __attribute__((aligned(16))) float A[(FZ + 2) * LP];  // Q at radius 1: LDS row = plane row - z0 + 1
    const int tid = threadIdx.x;
    if (!status[ST_GO]) return;
    const bool t0 = tid == 0;
    const int prev = series_gate<FIRST>(status, t0, pass, false);
    if (!prev) return;
    const int tnx = gridDim.x, tnz = gridDim.y;
    const size_t tile0 = (size_t)blockIdx.z * tnx * tnz;
    const size_t me = tile0 + (size_t)blockIdx.y * tnx + blockIdx.x;  // this tile's byte
    if (!FIRST) {
        if (!__syncthreads_or(tile_live(flags_in, tile0, tnx, tnz, tid))) {
            if (t0) flags_out[me] = 0;
            return;
        }
    }

    const int x0 = blockIdx.x * FX, z0 = blockIdx.y * FZ;
    const size_t base = (size_t)blockIdx.z * res * res;
    const int hi = res - 1;
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= 0 && pz <= hi; };

    // this thread's four cells
    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;  // VEC: res % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill ----
    float rc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ac[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned don = 0;  // the donor bytes of the own cells; a cell outside the grid has none and stays +0
    if (quad) {
        don = *reinterpret_cast<const unsigned *>(donors + c0);
        const float4 m = *reinterpret_cast<const float4 *>(e + c0);
        rc[0] = m.x, rc[1] = m.y, rc[2] = m.z, rc[3] = m.w;
        if constexpr (!FIRST) {
            const float4 a = *reinterpret_cast<const float4 *>(q_in + c0);
            ac[0] = a.x, ac[1] = a.y, ac[2] = a.z, ac[3] = a.w;
        }
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            don |= (unsigned)donors[c0 + j] << (8 * j);
            rc[j] = e[c0 + j];
            if constexpr (!FIRST) ac[j] = q_in[c0 + j];
        }
    }
    if constexpr (FIRST) {
#pragma unroll
        for (int j = 0; j < 4; j++) ac[j] = rc[j];
    }
    *reinterpret_cast<float4 *>(&A[(tz + 1) * LP + LC + tx]) = make_float4(ac[0], ac[1], ac[2], ac[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        A[lz * LP + lx] = inside(qx, qz) ? (FIRST ? e : q_in)[base + (size_t)qz * res + qx] : 0.0f;
    }
    __syncthreads();

    // ---- sweeps inside LDS, the ring frozen ----
    bool moved = FIRST;  // uniform over the workgroup
    for (int s = 0; s < sweeps; s++) {
        int ch = 0;
        if (don) {  // a thread without a donor holds e for good
            float lo[6], up[6], v[6];  // rows pz-1 (S), pz+1 (N) and the own row, columns px-1 .. px+4
            {
                const float *r0 = &A[tz * LP + LC + tx], *r1 = r0 + LP, *r2 = r1 + LP;
                const float4 a = *reinterpret_cast<const float4 *>(r0), b = *reinterpret_cast<const float4 *>(r1),
                             c = *reinterpret_cast<const float4 *>(r2);
                lo[0] = r0[-1], lo[1] = a.x, lo[2] = a.y, lo[3] = a.z, lo[4] = a.w, lo[5] = r0[4];
                v[0] = r1[-1], v[1] = b.x, v[2] = b.y, v[3] = b.z, v[4] = b.w, v[5] = r1[4];
                up[0] = r2[-1], up[1] = c.x, up[2] = c.y, up[3] = c.z, up[4] = c.w, up[5] = r2[4];
            }
            // One update of own cell j: the model's gather, k ascending.  `ch` sees EVERY update, not the net effect of
            // the sweep: e is signed, values may move both ways
            auto relax = [&](int j) {
                const unsigned d = don >> (8 * j);
                float a = rc[j];
                if (d & 1u) a = a + v[j];
                if (d & 2u) a = a + v[j + 2];
                if (d & 4u) a = a + lo[j + 1];
                if (d & 8u) a = a + up[j + 1];
                if (d & 16u) a = a + lo[j];
                if (d & 32u) a = a + lo[j + 2];
                if (d & 64u) a = a + up[j];
                if (d & 128u) a = a + up[j + 2];
                ch |= __float_as_uint(a) != __float_as_uint(v[j + 1]);
                v[j + 1] = a;
            };
            relax(0), relax(1), relax(2), relax(3);
            relax(2), relax(1), relax(0);
#pragma unroll
            for (int j = 0; j < 4; j++) ac[j] = v[j + 1];
        }
        if (!__syncthreads_or(ch)) break;  // (the barrier behind the read phase)
        moved = true;
        if (ch) *reinterpret_cast<float4 *>(&A[(tz + 1) * LP + LC + tx]) = make_float4(ac[0], ac[1], ac[2], ac[3]);
        __syncthreads();
    }

    // ---- store ----
    if (quad) {
        *reinterpret_cast<float4 *>(q_out + c0) = make_float4(ac[0], ac[1], ac[2], ac[3]);
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            q_out[c0 + j] = ac[j];
        }
    }
    if (t0) close_tile<FIRST>(status, flags_out, me, pass, moved);
}

// ---- deposit: Qin from the final Q, bk, and a fresh solve series ----
// bk may be the plane e: no launch reads e behind the accumulation
template <bool VEC>
__global__ __launch_bounds__(FT) void sediment_deposit_kernel(const unsigned char *__restrict__ donors,
                                                              const float *__restrict__ q, const float *__restrict__ b0,
                                                              const float *__restrict__ area, const float *__restrict__ h,
                                                              float *bk, const int *accum, int *solve, int *totals,
                                                              float deposition, float sea, int res) {
    __shared__ __attribute__((aligned(16))) float A[(FZ + 2) * LP];  // Q at radius 1: LDS row = plane row - z0 + 1
    const int tid = threadIdx.x;
    const bool go = series_done(accum);
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
        fresh_series(solve, go ? 1 : 0);
        if (accum[ST_GO]) totals[TOT_PASSES] += accum[ST_PASSES];
    }
    if (!go) return;

    const int x0 = blockIdx.x * FX, z0 = blockIdx.y * FZ;
    const size_t base = (size_t)blockIdx.z * res * res;
    const int hi = res - 1;
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= 0 && pz <= hi; };
    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;

    float qc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, bc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ac[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float hc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned don = 0;
    auto load4 = [&](const float *p, float (&o)[4]) {
        if (quad) {
            const float4 v = *reinterpret_cast<const float4 *>(p + c0);
            o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
        } else if (!VEC && row_in) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (px + j <= hi) o[j] = p[c0 + j];
        }
    };
    load4(q, qc);
    load4(b0, bc);
    load4(area, ac);
    load4(h, hc);
    if (quad) {
        don = *reinterpret_cast<const unsigned *>(donors + c0);
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (px + j <= hi) don |= (unsigned)donors[c0 + j] << (8 * j);
    }
    *reinterpret_cast<float4 *>(&A[(tz + 1) * LP + LC + tx]) = make_float4(qc[0], qc[1], qc[2], qc[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        A[lz * LP + lx] = inside(qx, qz) ? q[base + (size_t)qz * res + qx] : 0.0f;
    }
    __syncthreads();
    if (!row_in || px > hi) return;

    float lo[6], up[6], v[6];  // rows pz-1 (S), pz+1 (N) and the own row, columns px-1 .. px+4
    {
        const float *r0 = &A[tz * LP + LC + tx], *r1 = r0 + LP, *r2 = r1 + LP;
        const float4 a = *reinterpret_cast<const float4 *>(r0), b = *reinterpret_cast<const float4 *>(r1),
                     c = *reinterpret_cast<const float4 *>(r2);
        lo[0] = r0[-1], lo[1] = a.x, lo[2] = a.y, lo[3] = a.z, lo[4] = a.w, lo[5] = r0[4];
        v[0] = r1[-1], v[1] = b.x, v[2] = b.y, v[3] = b.z, v[4] = b.w, v[5] = r1[4];
        up[0] = r2[-1], up[1] = c.x, up[2] = c.y, up[3] = c.z, up[4] = c.w, up[5] = r2[4];
    }
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned d = don >> (8 * j);
        float a = 0.0f;  // the flux entering the cell: the gather of Q started from +0
        if (d & 1u) a = a + v[j];
        if (d & 2u) a = a + v[j + 2];
        if (d & 4u) a = a + lo[j + 1];
        if (d & 8u) a = a + up[j + 1];
        if (d & 16u) a = a + lo[j];
        if (d & 32u) a = a + lo[j + 2];
        if (d & 64u) a = a + up[j];
        if (d & 128u) a = a + up[j + 2];
        a = a < 0.0f ? 0.0f : a;  // a NaN passes
        const bool outlet = px + j == 0 || px + j == hi || pz == 0 || pz == hi || hc[j] <= sea;
        o[j] = outlet || !(ac[j] > 0.0f) ? bc[j] : bc[j] + (deposition * a) / ac[j];
    }
    if (quad) {
        *reinterpret_cast<float4 *>(bk + c0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            bk[c0 + j] = o[j];
        }
    }
}

// all or nothing over the 2K + 1 series; ST_GO was handed on from each to the next, so the last solve's verdict is the call's.
// hprev: h(K-1), NULL when K == 0; q: the Q of iteration K, NULL when K == 0
__global__ __launch_bounds__(256) void sediment_finalise_kernel(const float *__restrict__ h, float *__restrict__ out,
                                                                const float *__restrict__ hprev, const float *__restrict__ q,
                                                                float *__restrict__ flux, const int *solve, int *totals,
                                                                int *tally, size_t n) {
    const bool converged = series_done(solve);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        const int passes = totals[TOT_PASSES] + (solve[ST_GO] ? solve[ST_PASSES] : 0);
        totals[TOT_PASSES] = passes;
        totals[TOT_CONVERGED] = converged ? 1 : 0;
        if (converged && tally) {
            tally[0] += 1;
            tally[1] += passes;
        }
    }
    if (!converged) {
        if (i < n) out[i] = h[i];
        return;
    }
    if (i < n && flux) flux[i] = q ? q[i] : 0.0f;
    if (!hprev) return;
    // max |hK - h(K-1)| with d > m: a NaN never enters.  Non-negative floats order as their bits do.
    float m = 0.0f;
    if (i < n) {
        const float d = fabsf(out[i] - hprev[i]);
        if (d > 0.0f) m = d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) {
        unsigned *word = reinterpret_cast<unsigned *>(totals + TOT_RESIDUAL);
        if (__float_as_uint(m) > __atomic_load_n(word, __ATOMIC_RELAXED)) atomicMax(word, __float_as_uint(m));
    }
}

}  // namespace

int32_t nz_launch_fluvial_sediment_begin(hipStream_t s, int *totals, int *solve, const int *proceed) {
    NZ_LAUNCH(sediment_begin_kernel, dim3(1), dim3(1), 0, s, totals, solve, proceed);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_sediment_mask(hipStream_t s, const float *h, unsigned char *donors, const int *solve, float sea,
                                        int res, int count) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const bool word = res % 4 == 0 && (reinterpret_cast<uintptr_t>(donors) & 3) == 0;
    const bool vec = res % 4 == 0 && (reinterpret_cast<uintptr_t>(h) & 15) == 0;
    if (vec && word) NZ_LAUNCH((sediment_mask_kernel<true, true>), grid, dim3(FT), 0, s, h, donors, solve, sea, res);
    else if (word) NZ_LAUNCH((sediment_mask_kernel<false, true>), grid, dim3(FT), 0, s, h, donors, solve, sea, res);
    else NZ_LAUNCH((sediment_mask_kernel<false, false>), grid, dim3(FT), 0, s, h, donors, solve, sea, res);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_sediment_source(hipStream_t s, const float *b0, const float *hprev, float *e, const int *solve,
                                          int *accum, int *totals, size_t n) {
    if (n == 0) return NZ_OK;
    NZ_LAUNCH(sediment_source_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, b0, hprev, e, solve, accum, totals, n);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_sediment_gather_pass(hipStream_t s, const unsigned char *donors, const float *e, const float *q_in,
                                               float *q_out, int *status, const unsigned char *flags_in,
                                               unsigned char *flags_out, int res, int count, int pass, int sweeps) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(q_in) | reinterpret_cast<uintptr_t>(q_out);
    const bool vec = (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(donors) & 3) == 0 && res % 4 == 0;
    nz_with_bools([&](auto first, auto v) {
        NZ_LAUNCH((sediment_gather_pass_kernel<decltype(first)::value, decltype(v)::value>), grid, dim3(FT), 0, s, donors, e,
                  q_in, q_out, status, flags_in, flags_out, res, pass, sweeps);
    }, pass == 0, vec);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_sediment_deposit(hipStream_t s, const unsigned char *donors, const float *q, const float *b0,
                                           const float *area, const float *h, float *bk, const int *accum, int *solve,
                                           int *totals, float deposition, float sea, int res, int count) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(b0) | reinterpret_cast<uintptr_t>(area) |
                           reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(bk);
    const bool vec = (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(donors) & 3) == 0 && res % 4 == 0;
    if (vec)
        NZ_LAUNCH((sediment_deposit_kernel<true>), grid, dim3(FT), 0, s, donors, q, b0, area, h, bk, accum, solve, totals,
                  deposition, sea, res);
    else
        NZ_LAUNCH((sediment_deposit_kernel<false>), grid, dim3(FT), 0, s, donors, q, b0, area, h, bk, accum, solve, totals,
                  deposition, sea, res);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_sediment_finalise(hipStream_t s, const float *h, float *out, const float *hprev, const float *q,
                                            float *flux, const int *solve, int *totals, int *tally, size_t n) {
    if (n == 0) return NZ_OK;
    NZ_LAUNCH(sediment_finalise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h, out, hprev, q, flux, solve,
              totals, tally, n);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
