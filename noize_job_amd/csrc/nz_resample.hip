// nz_resample.hip -- upsample and downsample by a factor f in {2, 4, 8} (gfx950; new-framework feature).  The model is
// stated in include/noize_hip.h and restated in tests/resample_ref.py: cell-centred samples, clamp to edge, a separable X
// then Z pass whose row results are rounded to binary32, tap sums seeded with +0 in ascending tap order, no contraction
// (-ffp-contract=off, Makefile), the same in every float mode.  Every weight is a dyadic rational known at compile time
// (resample_weights below): nothing is evaluated per cell.
//
// Upsample.  A workgroup of 256 threads produces UX = 256 fine columns of UR = 8 coarse rows (8 f fine rows) of one plane:
//   X pass   one item per (staged source row, coarse column): the up to five coarse cells i-2 .. i+2 of that row are read
//            from the plane at their clamped coordinates (neighbouring lanes read neighbouring cells) and the f fine cells
//            of coarse cell i -- one per phase, each with its phase's constant weights -- go to LDS as one 8, 16 or 2 x 16
//            byte write.  The staged rows are the tile's coarse rows plus the filter's halo (0, 1, 2) on either side; LDS
//            row l stands for the clamped coarse row it is read from, so the Z pass needs no clamp of its own
//   barrier
//   Z pass   one thread per (coarse row, 4 fine columns): the up to five staged rows i-2 .. i+2 are read as 16-byte LDS reads
//            once and serve all f fine rows of coarse row i; each fine row is one 16-byte store (VEC: plane, base and pitch
//            16-byte aligned; otherwise four 4-byte stores), a wave's 64 lanes cover 1 KiB of one row.  With `base` the f
//            16-byte base loads of a coarse row are issued back to back before any of its sums and stores -- those of the
//            thread's first coarse row ahead of the X pass -- instead of one load, wait, store per fine row
// A NaN result of a tap sum or of the base add is stored as the canonical quiet NaN 0x7FC00000 (the model's rule: sign and
// payload of an arithmetic NaN differ between processors); NEAREST without base moves bits and never looks at them.
// `base` may be dst itself: a thread reads the base cells it is about to store and no others.
//
// Downsample.  One thread per output cell (two for f = 2): the f rows of its block are read as 16-byte loads (VEC: plane and
// pitch 16-byte aligned; otherwise 4-byte loads), summed left to right, then top to bottom, times 1 / f^2; a wave writes 64
// (128) consecutive outputs.
//
// The geometry is one struct for the tile, batch and stripe forms (include/noize_hip.h): rows are global rows of the fine /
// coarse grid minus the buffer's first global row, the coarse clamp range is the global border seen from the buffer, and
// only buffer rows [w0, w1) of the output are written.  The arithmetic of a cell depends on its global position alone, so
// any split into stripes or tiles of a launch gives the same bits.
#include "nz_internal.hpp"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float canon(float v) { return v != v ? __uint_as_float(0x7FC00000u) : v; }

// ---- the weights ------------------------------------------------------------------------------------------------------
// Phase p of factor F: i0 = i - 1, t = (2p+1)/(2F) + 1/2 for p < F/2; i0 = i, t = (2p+1)/(2F) - 1/2 otherwise.  Seen from
// the window v[0 .. 4] = cells i-2 .. i+2, the first tap of phase p sits at window index `first`; `n` taps follow.
// t is a multiple of 1/16, every weight a multiple of 2^-13 below 2: exact in double, exact in binary32.
template <int F, int FILT>
struct resample_weights {
    float w[F][4];
    int first[F];
    static constexpr int n = FILT == NZ_RESAMPLE_NEAREST ? 1 : FILT == NZ_RESAMPLE_BILINEAR ? 2 : 4;
    constexpr resample_weights() : w{}, first{} {
        for (int p = 0; p < F; p++) {
            const bool low = p < F / 2;
            const double t = (2 * p + 1) / (2.0 * F) + (low ? 0.5 : -0.5);
            const int i0 = low ? 1 : 2;  // window index of cell i0
            if (FILT == NZ_RESAMPLE_NEAREST) {
                first[p] = 2;
                w[p][0] = 1.0f;
            } else if (FILT == NZ_RESAMPLE_BILINEAR) {
                first[p] = i0;
                w[p][0] = (float)(1.0 - t);
                w[p][1] = (float)t;
            } else {
                first[p] = i0 - 1;
                w[p][0] = (float)((-t * t * t + 2 * t * t - t) / 2);
                w[p][1] = (float)((3 * t * t * t - 5 * t * t + 2) / 2);
                w[p][2] = (float)((-3 * t * t * t + 4 * t * t + t) / 2);
                w[p][3] = (float)((t * t * t - t * t) / 2);
            }
        }
    }
};

// the fine cell of phase P from the window v[0 .. 4]: NEAREST moves the bits, the others sum s = +0; s += v * w
template <int F, int FILT, int P>
__device__ __forceinline__ float tap_sum(const float (&v)[5]) {
    constexpr resample_weights<F, FILT> W{};
    if constexpr (FILT == NZ_RESAMPLE_NEAREST) {
        return v[2];
    } else {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < W.n; k++) s = s + v[W.first[P] + k] * W.w[P][k];
        return s;
    }
}

template <int F, int FILT, int P = 0>
__device__ __forceinline__ void x_phases(const float (&v)[5], float *o) {
    if constexpr (P < F) {
        o[P] = tap_sum<F, FILT, P>(v);
        x_phases<F, FILT, P + 1>(v, o);
    }
}

constexpr int UX = 256;  // fine columns of an upsample tile: one wave's 64 lanes x 4 columns
constexpr int UR = 8;    // coarse rows of an upsample tile
constexpr int UT = 256;  // threads

template <int F, int FILT, bool BASE, bool VEC>
__global__ __launch_bounds__(UT) void upsample_kernel(const float *__restrict__ src, float *dst, const float *base,
                                                      nz_up_geom g) {
    constexpr int HL = FILT == NZ_RESAMPLE_NEAREST ? 0 : FILT == NZ_RESAMPLE_BILINEAR ? 1 : 2;  // halo rows either side
    constexpr int NR = UR + 2 * HL;  // staged rows
    constexpr int CW = UX / F;       // coarse columns of the tile
    constexpr int K0 = 2 - HL, K1 = 2 + HL;  // window indices in use
    __shared__ __attribute__((aligned(16))) float XS[NR][UX];

    const int tid = threadIdx.x;
    src += (size_t)blockIdx.z * g.cstride;
    dst += (size_t)blockIdx.z * g.fstride;
    if (BASE) base += (size_t)blockIdx.z * g.fstride;
    const int cx0 = blockIdx.x * CW;              // first coarse column of the tile
    const int cz0 = g.cz_first + blockIdx.y * UR;  // first coarse row of the tile (global)

    // ---- the base cells of this thread's first coarse row: issued ahead of the X pass, so that they travel while it runs ----
    // A thread stores exactly the cells whose base it loads, so hoisting the loads above the stores of other rows is right
    // with base == dst too (the compiler, which must assume that base and dst alias, cannot do it).  b[p]: fine row p of the
    // coarse row at hand; only the 16-byte path prefetches, the 4-byte path reads its base cell where it adds it
    const int lane4 = (tid & 63) * 4;
    const int fx = blockIdx.x * UX + lane4;  // first of this thread's four fine columns
    const bool quad = VEC && fx + 3 < g.fcols;
    float4 b[BASE ? F : 1] = {};
    auto load_base = [&](int li) {
        if constexpr (BASE) {
            const int cz = cz0 + li;
            if (!quad || cz > g.cz_last) return;
#pragma unroll
            for (int p = 0; p < F; p++) {
                const int fb = cz * F + p - g.fgrow0;
                if (fb >= g.w0 && fb < g.w1) b[p] = *reinterpret_cast<const float4 *>(base + (size_t)fb * g.fpitch + fx);
            }
        }
    };
    load_base(tid >> 6);

    // ---- X pass ----
    for (int it = tid; it < NR * CW; it += UT) {
        const int l = it / CW, cc = it - l * CW;
        const int cx = cx0 + cc;
        if (cx >= g.ccols) continue;  // its fine cells lie beyond the row's end
        // the clamped global row this staged row stands for, as a buffer row; a row no output of the window uses may lie
        // outside the buffer and is read from the nearest row inside it (nz_launch_upsample: rows in use are inside)
        const int row = clampi(clampi(cz0 - HL + l, 0, g.cgrows - 1) - g.cgrow0, g.rd0, g.rd1);
        const float *r = src + (size_t)row * g.cpitch;
        float v[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = K0; k <= K1; k++) v[k] = r[clampi(cx - 2 + k, 0, g.ccols - 1)];
        float o[F];
        x_phases<F, FILT>(v, o);
        float *x = &XS[l][cc * F];
        if constexpr (F == 2) {
            *reinterpret_cast<float2 *>(x) = make_float2(o[0], o[1]);
        } else {
#pragma unroll
            for (int q = 0; q < F; q += 4) *reinterpret_cast<float4 *>(x + q) = make_float4(o[q], o[q + 1], o[q + 2], o[q + 3]);
        }
    }
    __syncthreads();

    // ---- Z pass ----
    if (fx >= g.fcols) return;
    for (int li = tid >> 6; li < UR; li += UT / 64) {
        const int cz = cz0 + li;
        if (cz > g.cz_last) break;
        if (li != (tid >> 6)) load_base(li);  // the later rows' base cells: all f loads back to back, ahead of the sums
        float4 rows[5] = {};
#pragma unroll
        for (int k = K0; k <= K1; k++) rows[k] = *reinterpret_cast<const float4 *>(&XS[li + HL - 2 + k][lane4]);
        const float vx[5] = {rows[0].x, rows[1].x, rows[2].x, rows[3].x, rows[4].x};
        const float vy[5] = {rows[0].y, rows[1].y, rows[2].y, rows[3].y, rows[4].y};
        const float vz[5] = {rows[0].z, rows[1].z, rows[2].z, rows[3].z, rows[4].z};
        const float vw[5] = {rows[0].w, rows[1].w, rows[2].w, rows[3].w, rows[4].w};
        float ox[F], oy[F], oz[F], ow[F];
        x_phases<F, FILT>(vx, ox);
        x_phases<F, FILT>(vy, oy);
        x_phases<F, FILT>(vz, oz);
        x_phases<F, FILT>(vw, ow);
#pragma unroll
        for (int p = 0; p < F; p++) {
            const int fb = cz * F + p - g.fgrow0;  // buffer row of the fine plane
            if (fb < g.w0 || fb >= g.w1) continue;
            const size_t c = (size_t)fb * g.fpitch + fx;
            float e[4] = {ox[p], oy[p], oz[p], ow[p]};
            if (quad) {
                if constexpr (BASE) {
                    e[0] = b[p].x + e[0];
                    e[1] = b[p].y + e[1];
                    e[2] = b[p].z + e[2];
                    e[3] = b[p].w + e[3];
                }
                if (BASE || FILT != NZ_RESAMPLE_NEAREST) {
#pragma unroll
                    for (int q = 0; q < 4; q++) e[q] = canon(e[q]);
                }
                *reinterpret_cast<float4 *>(dst + c) = make_float4(e[0], e[1], e[2], e[3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (fx + q >= g.fcols) break;
                    float s = e[q];
                    if (BASE) s = base[c + q] + s;
                    if (BASE || FILT != NZ_RESAMPLE_NEAREST) s = canon(s);
                    dst[c + q] = s;
                }
            }
        }
    }
}

constexpr int DX = 64, DZ = 4;  // downsample block: 64 lanes along a row, 4 rows

template <int F, bool VEC>
__global__ __launch_bounds__(DX *DZ) void downsample_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                            nz_down_geom g) {
    constexpr int OPT = F == 2 ? 2 : 1;  // outputs per thread: one 16-byte load per block row at least
    constexpr int NV = F * OPT;          // floats a thread reads per fine row
    src += (size_t)blockIdx.z * g.fstride;
    dst += (size_t)blockIdx.z * g.cstride;
    const int ox = (blockIdx.x * DX + threadIdx.x) * OPT;
    const int ob = g.w0 + blockIdx.y * DZ + threadIdx.y;  // output buffer row
    if (ox >= g.ccols || ob >= g.w1) return;
    const bool whole = ox + OPT <= g.ccols;
    const float *f = src + (size_t)((ob + g.cgrow0) * F - g.fgrow0) * g.fpitch + (size_t)ox * F;
    float m[OPT];
#pragma unroll
    for (int r = 0; r < F; r++, f += g.fpitch) {
        float v[NV];
        if (VEC && whole) {
#pragma unroll
            for (int q = 0; q < NV; q += 4) {
                const float4 t = *reinterpret_cast<const float4 *>(f + q);
                v[q] = t.x;
                v[q + 1] = t.y;
                v[q + 2] = t.z;
                v[q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < NV; q++) v[q] = (whole || q < F) ? f[q] : 0.0f;
        }
#pragma unroll
        for (int o = 0; o < OPT; o++) {
            float s = v[o * F];
#pragma unroll
            for (int q = 1; q < F; q++) s = s + v[o * F + q];
            m[o] = r == 0 ? s : m[o] + s;
        }
    }
    float *out = dst + (size_t)ob * g.cpitch + ox;
#pragma unroll
    for (int o = 0; o < OPT; o++)
        if (o == 0 || whole) out[o] = canon(m[o] * (1.0f / (F * F)));
}

template <int F, int FILT>
void launch_up(hipStream_t s, dim3 grid, const float *src, float *dst, const float *base, const nz_up_geom &g, bool vec) {
    if (base) {
        if (vec) NZ_LAUNCH((upsample_kernel<F, FILT, true, true>), grid, dim3(UT), 0, s, src, dst, base, g);
        else NZ_LAUNCH((upsample_kernel<F, FILT, true, false>), grid, dim3(UT), 0, s, src, dst, base, g);
    } else {
        if (vec) NZ_LAUNCH((upsample_kernel<F, FILT, false, true>), grid, dim3(UT), 0, s, src, dst, base, g);
        else NZ_LAUNCH((upsample_kernel<F, FILT, false, false>), grid, dim3(UT), 0, s, src, dst, base, g);
    }
}

template <int F>
void launch_up_f(hipStream_t s, dim3 grid, int filter, const float *src, float *dst, const float *base, const nz_up_geom &g,
                 bool vec) {
    if (filter == NZ_RESAMPLE_NEAREST) launch_up<F, NZ_RESAMPLE_NEAREST>(s, grid, src, dst, base, g, vec);
    else if (filter == NZ_RESAMPLE_BILINEAR) launch_up<F, NZ_RESAMPLE_BILINEAR>(s, grid, src, dst, base, g, vec);
    else launch_up<F, NZ_RESAMPLE_CATMULL_ROM>(s, grid, src, dst, base, g, vec);
}

template <int F>
void launch_down_f(hipStream_t s, dim3 grid, const float *src, float *dst, const nz_down_geom &g, bool vec) {
    if (vec) NZ_LAUNCH((downsample_kernel<F, true>), grid, dim3(DX, DZ), 0, s, src, dst, g);
    else NZ_LAUNCH((downsample_kernel<F, false>), grid, dim3(DX, DZ), 0, s, src, dst, g);
}

}  // namespace

int nz_resample_halo(int filter) { return filter == NZ_RESAMPLE_NEAREST ? 0 : filter == NZ_RESAMPLE_BILINEAR ? 1 : 2; }

int32_t nz_launch_upsample(hipStream_t s, const float *src, float *dst, const float *base, nz_up_geom g, int factor,
                           int filter, int count) {
    if (g.w1 <= g.w0 || g.fcols <= 0 || count <= 0) return NZ_OK;
    const int halo = nz_resample_halo(filter);
    // the coarse rows of the window, and the rows of the buffer its taps read: inside the buffer, or the launch is refused
    g.cz_first = (g.w0 + g.fgrow0) / factor;
    g.cz_last = (g.w1 - 1 + g.fgrow0) / factor;
    const int lo = g.cz_first - halo > 0 ? g.cz_first - halo : 0;
    const int hi = g.cz_last + halo < g.cgrows - 1 ? g.cz_last + halo : g.cgrows - 1;
    g.rd0 = lo - g.cgrow0;
    g.rd1 = hi - g.cgrow0;
    NZ_REQUIRE(g.rd0 >= 0 && g.rd1 < g.crows && g.rd0 <= g.rd1,
               "srcSt: coarse rows [%d, %d] of the grid are required, the buffer holds [%d, %d)", lo, hi, g.cgrow0,
               g.cgrow0 + g.crows);
    const bool vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(base) | (uintptr_t)g.fpitch * 4 |
                       (uintptr_t)(g.fstride * 4)) & 15) == 0;
    const dim3 grid((g.fcols + UX - 1) / UX, (g.cz_last - g.cz_first) / UR + 1, count);
    if (factor == 2) launch_up_f<2>(s, grid, filter, src, dst, base, g, vec);
    else if (factor == 4) launch_up_f<4>(s, grid, filter, src, dst, base, g, vec);
    else launch_up_f<8>(s, grid, filter, src, dst, base, g, vec);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_downsample(hipStream_t s, const float *src, float *dst, const nz_down_geom &g, int factor, int count) {
    if (g.w1 <= g.w0 || g.ccols <= 0 || count <= 0) return NZ_OK;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)g.fpitch * 4 | (uintptr_t)(g.fstride * 4)) & 15) == 0;
    const int opt = factor == 2 ? 2 : 1;
    const dim3 grid((g.ccols + DX * opt - 1) / (DX * opt), (g.w1 - g.w0 + DZ - 1) / DZ, count);
    if (factor == 2) launch_down_f<2>(s, grid, src, dst, g, vec);
    else if (factor == 4) launch_down_f<4>(s, grid, src, dst, g, vec);
    else launch_down_f<8>(s, grid, src, dst, g, vec);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
