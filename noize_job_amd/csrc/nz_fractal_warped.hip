// nz_fractal_warped.hip -- domain-warped fractal noise (nz_fractal_warped*, nz_launch_fractal_warped).
//
// The octave loop of nz_fractal_shaped read at coordinates displaced by a plain fBm of the same basis (Quilez's
// f(p + s q(p))).  Per cell, in this order (float32, the numpy driver tests/fractal_warp_ref.py restates it):
//   X = (float)c + xpos, Z = (float)r + zpos;  u = X / ns * scale, v = Z / ns * scale
//   qx = D(u, v), qz = D(u + 5.2, v + 1.3)        D: fBm of warpOctaves octaves / its norm, STRICT in every float mode
//   px = (X + (2 qx - 1) strength) / ns, pz = (Z + (2 qz - 1) strength) / ns
//   result = the shaped octave loop at (px, pz) / norm
// Phase 1 (D) runs at unwarped coordinates: v f once per row and a row-level table-range decision, as the fBm kernels.
// Phase 2 has a coordinate pair per cell and no bound from the row: a thread takes the table loop when all its cells stay
// inside NZ_TAB_LIMIT at the top frequency, and the guarded loop (the per-cell table-or-direct choice) otherwise.
//
// Same source as nz_fractal.hip, own translation unit: the basis functions, octave_add / shape_fold and the table layouts
// come from there, and the fBm and shaped modules stay instruction for instruction what they were.
#define NZ_FRACTAL_WARPED_TU 1
#include "nz_fractal.hip"

namespace {

// the LDS tables of one basis (the layouts the fBm families stage; FAST simplex adds the halved tolerance-mode pair)
template <int BASIS, bool FAST>
struct warp_lds {
    static constexpr bool SIMPLEX = BASIS == NZ_NOISE_SIMPLEX;
    static constexpr bool TAB2 = BASIS == NZ_NOISE_PERLIN || BASIS == NZ_NOISE_CELLULAR;
    static constexpr bool TAB3 = BASIS == NZ_NOISE_DOMAIN_ROTATED_PERLIN || BASIS == NZ_NOISE_DOMAIN_ROTATED_SIMPLEX;
    static constexpr bool PSR = BASIS == NZ_NOISE_PERIODIC_PERLIN || BASIS == NZ_NOISE_ROTATED_SIMPLEX;
    static constexpr int T1_PAIRS = 2 * NZ_T1_N * 4;  // simplex T1 as staged: stage_t1_pairs, 2336 bytes (a multiple of 16)
    static constexpr int BYTES = SIMPLEX ? T1_PAIRS + NZ_T2_N * 16 + (FAST ? T1_PAIRS + NZ_T2_N * 8 : 0)
                                 : TAB2  ? NZ_TB1_N * 4 + NZ_TB2_N * 8
                                 : TAB3  ? NZ_P3_N * 4 + NZ_G3_N * 16
                                 : PSR   ? NZ_PSR_T2 * 8 + NZ_PSR_T1 * 4
                                         : 16;
    const int *i1;      // simplex T1 (pairs) / P1 / C1 / P3 / psr T1
    const void *t2;     // simplex T2 (float4) / P2 / C2 (float2) / G3 (float4) / psr T2 (float2)
    const int *i1f;     // FAST simplex: T1 / 2 (pairs)
    const float2 *t2f;  // FAST simplex: {a0, h} * norm

    // stage the tables from `tab` (the context's table block of this basis, see nz_launch_fractal_warped) into `s`
    __device__ __forceinline__ warp_lds(float4 *s, const void *tab) {
        char *b = reinterpret_cast<char *>(s);
        if constexpr (SIMPLEX) {
            int *t1 = reinterpret_cast<int *>(b);
            float4 *g = reinterpret_cast<float4 *>(b + T1_PAIRS);
            const int *t1g = reinterpret_cast<const int *>(tab);
            const float4 *t2g = reinterpret_cast<const float4 *>(t1g + NZ_T1_N);
            stage_t1_pairs<0>(t1, t1g);
            for (int i = threadIdx.x; i < NZ_T2_N; i += 256) g[i] = t2g[i];
            i1 = t1;
            t2 = g;
            if constexpr (FAST) {
                int *h1 = reinterpret_cast<int *>(b + T1_PAIRS + NZ_T2_N * 16);
                float2 *h2 = reinterpret_cast<float2 *>(b + 2 * T1_PAIRS + NZ_T2_N * 16);
                stage_t1_pairs<1>(h1, t1g);
                for (int i = threadIdx.x; i < NZ_T2_N; i += 256) {
                    const float4 v = t2g[i];
                    h2[i] = make_float2(v.x * v.z, v.y * v.z);
                }
                i1f = h1;
                t2f = h2;
            }
        } else if constexpr (TAB2) {
            int *t1 = reinterpret_cast<int *>(b);
            float2 *g = reinterpret_cast<float2 *>(b + NZ_TB1_N * 4);
            const int *t1g = reinterpret_cast<const int *>(tab);
            const float2 *t2g = reinterpret_cast<const float2 *>(t1g + NZ_TB1_N);
            for (int i = threadIdx.x; i < NZ_TB1_N; i += 256) t1[i] = t1g[i];
            for (int i = threadIdx.x; i < NZ_TB2_N; i += 256) g[i] = t2g[i];
            i1 = t1;
            t2 = g;
        } else if constexpr (TAB3) {
            int *p3 = reinterpret_cast<int *>(b);
            float4 *g = reinterpret_cast<float4 *>(b + NZ_P3_N * 4);
            const int *p3g = reinterpret_cast<const int *>(tab);
            const float4 *g3g = reinterpret_cast<const float4 *>(p3g + NZ_P3_N) +
                                (BASIS == NZ_NOISE_DOMAIN_ROTATED_SIMPLEX ? NZ_G3_N : 0);
            for (int i = threadIdx.x; i < NZ_P3_N; i += 256) p3[i] = p3g[i];
            for (int i = threadIdx.x; i < NZ_G3_N; i += 256) g[i] = g3g[i];
            i1 = p3;
            t2 = g;
        } else if constexpr (PSR) {
            float2 *g = reinterpret_cast<float2 *>(b);
            int *t1 = reinterpret_cast<int *>(b + NZ_PSR_T2 * 8);
            const int *t1g = reinterpret_cast<const int *>(tab);
            const float2 *src = reinterpret_cast<const float2 *>(t1g + NZ_PSR_T1) +
                                (BASIS == NZ_NOISE_ROTATED_SIMPLEX ? NZ_PSR_T2 : 0);
            for (int i = threadIdx.x; i < NZ_PSR_T1; i += 256) t1[i] = t1g[i];
            for (int i = threadIdx.x; i < NZ_PSR_T2; i += 256) g[i] = src[i];
            i1 = t1;
            t2 = g;
        }
        __syncthreads();
    }

    // the strict basis value v of noise_value<BASIS> at (x, z).  GUARD: the caller has not shown |x|, |z| < NZ_TAB_LIMIT,
    // so this cell chooses between the tables and the direct evaluation itself (the periodic bases and Sin decide inside
    // psrnoise2 / need no tables)
    template <bool GUARD>
    __device__ __forceinline__ float value(float x, float z) const {
        if constexpr (SIMPLEX || TAB2 || TAB3) {
            if (GUARD && !(fmaxf(fabsf(x), fabsf(z)) < NZ_TAB_LIMIT)) {
                asm volatile("; direct evaluation" ::: "memory");  // a real branch, never if-converted
                return noise_value<BASIS>(x, z, psr_tables{nullptr, nullptr});
            }
            if constexpr (SIMPLEX) {
                return rectify_half(snoise2_tab(x, z, i1, static_cast<const float4 *>(t2)));
            } else if constexpr (BASIS == NZ_NOISE_PERLIN) {
                return rectify(cnoise2_tab(x, z, i1, static_cast<const float2 *>(t2)));
            } else if constexpr (BASIS == NZ_NOISE_CELLULAR) {
                return cellular_rect_tab(x, z, i1, static_cast<const float2 *>(t2));
            } else {
                float xr, zr, yr;
                domain_rotate(x, z, xr, zr, yr);
                const float4 *g = static_cast<const float4 *>(t2);
                return rectify(BASIS == NZ_NOISE_DOMAIN_ROTATED_PERLIN ? cnoise3_tab(xr, zr, yr, i1, g)
                                                                       : snoise3_tab(xr, zr, yr, i1, g));
            }
        } else {
            return noise_value<BASIS>(x, z, psr_tables{i1, static_cast<const float2 *>(t2)});
        }
    }
};

// the displacement of one row: (qx, qz) = (D(u, v), D(u + 5.2, v + 1.3)) for the thread's VEC cells
template <int BASIS, bool FAST, int VEC, bool GUARD>
__device__ __forceinline__ void warp_displacement(const warp_lds<BASIS, FAST> &L, const nz_fractal_kparams &p,
                                                  const nz_warp_params &wp, const float (&u0)[VEC],
                                                  const float (&u1)[VEC], float v0, float v1, float (&qx)[VEC],
                                                  float (&qz)[VEC]) {
    const nz_ridge_params rp{};
    float w = 1.0f;  // (fBm: unused)
    float detune = 0.0f, f = 1.0f, a = p.amp;
#pragma unroll
    for (int c = 0; c < VEC; c++) qx[c] = 0.0f, qz[c] = 0.0f;
    for (int i = 0; i < wp.octaves; i++) {
        const float zV0 = f * v0, zV1 = f * v1;
#pragma unroll
        for (int c = 0; c < VEC; c++) {
            octave_add<NZ_SHAPE_FBM>(qx[c], w, a, L.template value<GUARD>(f * u0[c], zV0), rp);
            octave_add<NZ_SHAPE_FBM>(qz[c], w, a, L.template value<GUARD>(f * u1[c], zV1), rp);
        }
        detune += p.detune_rate;
        f *= (p.stepdown - detune);
        a *= p.G;
    }
#pragma unroll
    for (int c = 0; c < VEC; c++) qx[c] = qx[c] / wp.norm, qz[c] = qz[c] / wp.norm;
}

// the shaped octave loop at per-cell coordinates (px, pz), strict; the sum before the division by the norm
template <int BASIS, bool FAST, int SHAPE, int VEC, bool GUARD>
__device__ __forceinline__ void warp_octaves(const warp_lds<BASIS, FAST> &L, const nz_fractal_kparams &p,
                                             const nz_ridge_params &rp, const float (&px)[VEC], const float (&pz)[VEC],
                                             float (&t)[VEC]) {
    float w[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) t[c] = 0.0f, w[c] = 1.0f;
    float detune = 0.0f, f = 1.0f, a = p.amp;
    for (int i = 0; i < p.octaves; i++) {
#pragma unroll
        for (int c = 0; c < VEC; c++) octave_add<SHAPE>(t[c], w[c], a, L.template value<GUARD>(f * px[c], f * pz[c]), rp);
        detune += p.detune_rate;
        f *= (p.stepdown - detune);
        a *= p.G;
    }
}

// the same loop in tolerance mode (simplex only, every coordinate inside the tables' range): the forms of
// fractal_simplex_tab_kernel<FAST = true>
template <int SHAPE, int VEC>
__device__ __forceinline__ void warp_octaves_fast(const warp_lds<NZ_NOISE_SIMPLEX, true> &L, const nz_fractal_kparams &p,
                                                  const nz_ridge_params &rp, const float (&px)[VEC],
                                                  const float (&pz)[VEC], float (&t)[VEC]) {
    float w[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) t[c] = 0.0f, w[c] = 1.0f;
    float detune = 0.0f, f = 1.0f, a = p.amp, bias = 0.0f;
    for (int i = 0; i < p.octaves; i++) {
        const float a65 = 65.0f * a;
#pragma unroll
        for (int c = 0; c < VEC; c++) {
            const float n = snoise2_tab_fast(f * px[c], f * pz[c], L.i1f, L.t2f);  // snoise / 130
            if constexpr (SHAPE == NZ_SHAPE_FBM) {
                t[c] = __builtin_fmaf(a65, n, t[c]);
            } else {
                shape_fold<SHAPE>(t[c], w[c], a, fabsf(130.0f * n), rp);
            }
        }
        if constexpr (SHAPE == NZ_SHAPE_FBM) bias = __builtin_fmaf(0.5f, a, bias);
        detune += p.detune_rate;
        f *= (p.stepdown - detune);
        a *= p.G;
    }
#pragma unroll
    for (int c = 0; c < VEC; c++) t[c] += bias;
}

template <int BASIS, int SHAPE, bool FAST, int VEC>
__global__ __launch_bounds__(256) void fractal_warped_kernel(float *__restrict__ dst, int rows, int cols, int pitch,
                                                            int blocks_per_row, nz_fractal_kparams p,
                                                            const void *__restrict__ tab, nz_ridge_params rp,
                                                            nz_warp_params wp) {
    using lds_t = warp_lds<BASIS, FAST>;
    __shared__ float4 s_lds[(lds_t::BYTES + 15) / 16];
    const lds_t L(s_lds, tab);
    fractal_batch_enter(p, dst);
    int by = blockIdx.x / blocks_per_row;
    int bx = blockIdx.x - by * blocks_per_row;
    int x0 = (bx * 256 + threadIdx.x) * VEC;
    if (x0 >= cols) return;
    float X[VEC], u0[VEC], u1[VEC];
    float ureach = 0.0f;
#pragma unroll
    for (int c = 0; c < VEC; c++) {
        X[c] = (float)(x0 + c) + p.posx;
        u0[c] = X[c] / p.noise_size * wp.scale;
        u1[c] = u0[c] + 5.2f;
        ureach = fmaxf(ureach, fmaxf(fabsf(u0[c]), fabsf(u1[c])));
    }
    int zend = min(rows, (by + 1) * p.rows_per_wg);
    for (int z = by * p.rows_per_wg; z < zend; z++) {
        const float Z = (float)z + p.posz;
        const float v0 = Z / p.noise_size * wp.scale, v1 = v0 + 1.3f;
        // phase 1: the displacement at unwarped coordinates (one decision per row, as the fBm kernels)
        float qx[VEC], qz[VEC];
        if (wp.fmax * fmaxf(ureach, fmaxf(fabsf(v0), fabsf(v1))) < NZ_TAB_LIMIT) {
            warp_displacement<BASIS, FAST, VEC, false>(L, p, wp, u0, u1, v0, v1, qx, qz);
        } else {
            asm volatile("; guarded displacement" ::: "memory");
            warp_displacement<BASIS, FAST, VEC, true>(L, p, wp, u0, u1, v0, v1, qx, qz);
        }
        // the warped coordinates (2 q is exact: twice_minus_one is the separate multiply and add)
        float px[VEC], pz[VEC], reach = 0.0f;
#pragma unroll
        for (int c = 0; c < VEC; c++) {
            px[c] = (X[c] + twice_minus_one(qx[c]) * wp.strength) / p.noise_size;
            pz[c] = (Z + twice_minus_one(qz[c]) * wp.strength) / p.noise_size;
            reach = fmaxf(reach, fmaxf(fabsf(px[c]), fabsf(pz[c])));
        }
        // phase 2: the octave loop; the table loop when every octave of this thread's cells stays inside the tables' range
        // (NaN compares false: the guarded loop)
        float t[VEC];
        if (p.fmax * reach < NZ_TAB_LIMIT) {
            if constexpr (FAST && BASIS == NZ_NOISE_SIMPLEX)
                warp_octaves_fast<SHAPE, VEC>(L, p, rp, px, pz, t);
            else
                warp_octaves<BASIS, FAST, SHAPE, VEC, false>(L, p, rp, px, pz, t);
        } else {
            asm volatile("; guarded octave loop" ::: "memory");  // a real branch, never if-converted
            warp_octaves<BASIS, FAST, SHAPE, VEC, true>(L, p, rp, px, pz, t);
        }
        float *row = dst + (size_t)z * pitch;
        float o[VEC];
#pragma unroll
        for (int c = 0; c < VEC; c++) o[c] = t[c] / p.norm;
        bool full = x0 + VEC <= cols && ((reinterpret_cast<uintptr_t>(row + x0) & (VEC * 4 - 1)) == 0);
        if (full) {
            if constexpr (VEC == 4) {
                *reinterpret_cast<float4 *>(row + x0) = make_float4(o[0], o[1], o[2], o[3]);
            } else if constexpr (VEC == 2) {
                *reinterpret_cast<float2 *>(row + x0) = make_float2(o[0], o[1]);
            } else {
                row[x0] = o[0];
            }
        } else {
#pragma unroll
            for (int c = 0; c < VEC; c++)
                if (x0 + c < cols) row[x0 + c] = o[c];
        }
    }
}

// cells per thread, per basis (the fBm families' choice where the registers allow it; see DESIGN.md "Domain warp")
template <int BASIS>
constexpr int warp_vec() {
    return BASIS == NZ_NOISE_DOMAIN_ROTATED_PERLIN || BASIS == NZ_NOISE_DOMAIN_ROTATED_SIMPLEX ? 1 : 2;
}

template <int BASIS, int SHAPE>
int32_t launch_warped_basis(hipStream_t s, float *dst, int rows, int cols, int pitch, const nz_fractal_params &p,
                            const nz_warp_params &wp, const void *tab, int count) {
    constexpr int VEC = warp_vec<BASIS>();
    int bpr = (cols + 256 * VEC - 1) / (256 * VEC);
    long long blocks = (long long)bpr * ((rows + p.rows_per_wg - 1) / p.rows_per_wg);
    if (blocks > 0x7fffffffLL) {
        nz_set_error("fractal grid too large");
        return NZ_ERR_INVALID;
    }
    if (BASIS == NZ_NOISE_SIMPLEX && nz_tls_float_mode >= NZ_FLOAT_FAST)
        NZ_LAUNCH((fractal_warped_kernel<BASIS, SHAPE, BASIS == NZ_NOISE_SIMPLEX, VEC>), dim3((unsigned)blocks, count),
                  dim3(256), 0, s, dst, rows, cols, pitch, bpr, static_cast<const nz_fractal_kparams &>(p), tab, p.ridge, wp);
    else
        NZ_LAUNCH((fractal_warped_kernel<BASIS, SHAPE, false, VEC>), dim3((unsigned)blocks, count), dim3(256), 0, s, dst,
                  rows, cols, pitch, bpr, static_cast<const nz_fractal_kparams &>(p), tab, p.ridge, wp);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

template <int SHAPE>
int32_t launch_warped(hipStream_t s, int noiseType, float *dst, int rows, int cols, int pitch, const nz_fractal_params &p,
                      const nz_warp_params &wp, const float *d_rgrad, const void *d_simplex, int count) {
    // the context's table block (build_simplex_tables in nz_runtime.cpp): simplex T1 / T2, Perlin P1 / P2, cellular
    // C1 / C2, then P3 and the two G3 (the kernel picks its G3); the periodic bases read d_rgrad
    const char *b = reinterpret_cast<const char *>(d_simplex);
    const char *tab2 = b + (NZ_T1_N * 4 + NZ_T2_N * 16);
    const size_t tab2_n = NZ_TB1_N * 4 + NZ_TB2_N * 8;
    switch (noiseType) {
        case NZ_NOISE_SIN: return launch_warped_basis<NZ_NOISE_SIN, SHAPE>(s, dst, rows, cols, pitch, p, wp, nullptr, count);
        case NZ_NOISE_PERLIN: return launch_warped_basis<NZ_NOISE_PERLIN, SHAPE>(s, dst, rows, cols, pitch, p, wp, tab2, count);
        case NZ_NOISE_PERIODIC_PERLIN:
            return launch_warped_basis<NZ_NOISE_PERIODIC_PERLIN, SHAPE>(s, dst, rows, cols, pitch, p, wp, d_rgrad, count);
        case NZ_NOISE_SIMPLEX: return launch_warped_basis<NZ_NOISE_SIMPLEX, SHAPE>(s, dst, rows, cols, pitch, p, wp, b, count);
        case NZ_NOISE_ROTATED_SIMPLEX:
            return launch_warped_basis<NZ_NOISE_ROTATED_SIMPLEX, SHAPE>(s, dst, rows, cols, pitch, p, wp, d_rgrad, count);
        case NZ_NOISE_CELLULAR:
            return launch_warped_basis<NZ_NOISE_CELLULAR, SHAPE>(s, dst, rows, cols, pitch, p, wp, tab2 + tab2_n, count);
        case NZ_NOISE_DOMAIN_ROTATED_PERLIN:
            return launch_warped_basis<NZ_NOISE_DOMAIN_ROTATED_PERLIN, SHAPE>(s, dst, rows, cols, pitch, p, wp,
                                                                              tab2 + 2 * tab2_n, count);
        case NZ_NOISE_DOMAIN_ROTATED_SIMPLEX:
            return launch_warped_basis<NZ_NOISE_DOMAIN_ROTATED_SIMPLEX, SHAPE>(s, dst, rows, cols, pitch, p, wp,
                                                                               tab2 + 2 * tab2_n, count);
    }
    nz_set_error("unknown noise type %d", noiseType);
    return NZ_ERR_INVALID;
}

}  // namespace

int32_t nz_launch_fractal_warped(hipStream_t s, int noiseType, float *dst, int rows, int cols, int pitch,
                                 const nz_fractal_params &p, const nz_warp_params &wp, const float *d_rgrad,
                                 const void *d_simplex, int count) {
    NZ_REQUIRE(d_rgrad && d_simplex, "noise tables missing");
    switch (p.shape) {
        case NZ_SHAPE_FBM: return launch_warped<NZ_SHAPE_FBM>(s, noiseType, dst, rows, cols, pitch, p, wp, d_rgrad, d_simplex, count);
        case NZ_SHAPE_BILLOW: return launch_warped<NZ_SHAPE_BILLOW>(s, noiseType, dst, rows, cols, pitch, p, wp, d_rgrad, d_simplex, count);
        case NZ_SHAPE_RIDGED: return launch_warped<NZ_SHAPE_RIDGED>(s, noiseType, dst, rows, cols, pitch, p, wp, d_rgrad, d_simplex, count);
    }
    nz_set_error("unknown octave shape %d", p.shape);
    return NZ_ERR_INVALID;
}
