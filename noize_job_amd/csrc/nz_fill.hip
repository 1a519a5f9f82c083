// nz_fill.hip -- depression filling: lakes and pit-free drainage (gfx950; new-framework feature).
//
// THE MODEL (include/noize_hip.h states it for the caller, tests/fill_ref.py restates it in numpy):
//   Square tile res x res, row-major z * res + x, float32 throughout, no contraction, the same in every float mode.
//   Neighbours k = 0..7 in the fluvial stage's order W E S N SW SE NW NE; a neighbour outside the tile does not exist.
//   Outlets are the fluvial stage's: border cells and cells with h[c] <= seaLevel.  W[c] = h[c] for an outlet.
//   Operator for every other cell: m = +inf; for k ascending: t = W[k] + epsilon; m = t < m ? t : m;
//   F(W)[c] = h[c] > m ? h[c] : m.  Start: W = +inf at the non-outlets.  Result: the fixed point reached from that start.
//   With epsilon == 0 it is the spill elevation (the minimax path height to an outlet; flats remain); with epsilon > 0 every
//   filled cell sits at least epsilon above some neighbour, so every non-outlet has a strictly lower neighbour.
// F is monotone and the start lies above every fixed point, so every order of updates -- Jacobi, tile-local sweeps, a
// priority queue -- goes down to the same floats, the greatest fixed point.  That is what lets the kernel below update in
// whatever order is fastest and still be tested for bit equality.  Two facts make the arithmetic order-free as well: no
// value is a NaN (heights are finite, +inf + epsilon = +inf), and t is never -0 (x + +0 and x + epsilon round to +0, not
// -0), so min_k (W[k] + epsilon) == (min_k W[k]) + epsilon bit for bit whatever the order of the minimum.
//
// One launch per PASS on the fluvial stage's geometry: a workgroup of 256 threads owns an FX x FZ = 64 x 16 tile, a thread
// four consecutive cells of a row (16-byte accesses where planes and pitch allow, VEC), batch tiles on blockIdx.z.  A pass
// reads W_in and writes W_out, two planes that alternate, so no workgroup waits for another and no launch has a race:
//   skip     (pass > 0) when neither this tile nor one of its eight neighbours changed in the pass before -- one byte per
//            tile, two generations alternating with the planes -- the tile is at rest against an unchanged ring: it writes
//            a zero byte and returns.  No copy is needed: a tile that did not change has equal cells in both planes.
//   fill     the tile's own h into registers, its W at radius 1 into LDS (18 x 72 floats); ring cells outside the grid hold
//            +inf.  The first pass reads no W plane: it derives the start state from h.
//   sweeps   with the ring frozen: every thread reads its 3 x 6 window, updates its four cells left to right and back right
//            to left in registers (Gauss-Seidel inside the thread, Jacobi between threads), a workgroup-wide OR of "changed"
//            doubles as the barrier behind the read phase, then the write phase and a second barrier.  The loop ends when a
//            sweep changes nothing, or after `sweeps` of them.
//   store    the own cells to W_out, the tile's byte, and one ordinary global atomic on changed[pass % 3] when they changed.
// Convergence without the host: pass p first reads changed[(p - 1) % 3]; zero means the pass before changed nothing, both
// planes hold the fixed point, and the whole launch returns at once -- as does every later one.  Three words in turn are
// enough: pass p reads word p - 1, bumps word p and (one thread of the grid) zeroes word p + 1.  The first pass changes every
// tile by decree (its predecessor is the +inf start, which exists in no plane), so pass 1 writes all of the second plane.
// The finalise launch looks at the word of the last pass that ran: zero -> W to the heights and W - h to the depth plane;
// otherwise the heights stay and the depth is zero: all or nothing, a caller never sees +inf.
//
// The cap, `sweeps`, is 16 (nz_stages.cpp): enough to carry a value across the tile's 16 rows and 64 columns.  4 to 64 were
// measured: DESIGN.md section 4, "depression filling".
#include "nz_internal.hpp"

namespace {

constexpr int FX = 64, FZ = 16;  // tile of one workgroup
constexpr int FT = 256;          // threads: one per four cells of a row
constexpr int LP = 72;           // LDS row pitch in cells; plane column x0 + i is LDS column LC + i
constexpr int LC = 4;            // keeps a thread's four cells 16-byte aligned in LDS
constexpr int NRING = 2 * (FX + 2) + 2 * FZ;  // cells at radius 1 around the tile
constexpr int ST_PASSES = 0, ST_CONVERGED = 1, ST_CHANGED = 2;  // the status words: changed[3] from ST_CHANGED on

// the ring at radius 1 of the tile, cell i of NRING: its LDS row and column
__device__ __forceinline__ void ring_cell(int i, int &lz, int &lx) {
    if (i < 2 * (FX + 2)) {
        const int rr = i / (FX + 2);
        lz = rr ? FZ + 1 : 0;
        lx = LC - 1 + (i - rr * (FX + 2));
    } else {
        const int j = i - 2 * (FX + 2);
        lz = 1 + (j >> 1);
        lx = (j & 1) ? LC + FX : LC - 1;
    }
}

template <bool FIRST, bool VEC>
__global__ __launch_bounds__(FT) void fill_pass_kernel(const float *__restrict__ h, const float *__restrict__ w_in,
                                                       float *__restrict__ w_out, int *status,
                                                       const unsigned char *__restrict__ flags_in,
                                                       unsigned char *__restrict__ flags_out, float eps, float sea, int res,
                                                       int pass, int sweeps) {
    __shared__ __attribute__((aligned(16))) float W[(FZ + 2) * LP];  // radius 1: LDS row = plane row - z0 + 1
    const int tid = threadIdx.x;
    int *changed = status + ST_CHANGED;

    // ---- did the pass before change anything at all? ----
    const int prev = FIRST ? 1 : changed[(pass + 2) % 3];
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
        changed[(pass + 1) % 3] = 0;
        if (FIRST) changed[0] = 1;  // by decree; no workgroup bumps it
        if (prev) status[ST_PASSES] = pass + 1;
    }
    if (!prev) return;

    // ---- did this tile's neighbourhood? ----
    const int tnx = gridDim.x, tnz = gridDim.y;
    const size_t tile0 = (size_t)blockIdx.z * tnx * tnz;
    const size_t me = tile0 + (size_t)blockIdx.y * tnx + blockIdx.x;
    if (!FIRST) {
        int live = 0;
        if (tid < 9) {
            const int bx = (int)blockIdx.x + tid % 3 - 1, bz = (int)blockIdx.y + tid / 3 - 1;
            if (bx >= 0 && bx < tnx && bz >= 0 && bz < tnz) live = flags_in[tile0 + (size_t)bz * tnx + bx];
        }
        if (!__syncthreads_or(live)) {
            if (tid == 0) flags_out[me] = 0;
            return;
        }
    }

    const int x0 = blockIdx.x * FX, z0 = blockIdx.y * FZ;
    const size_t base = (size_t)blockIdx.z * res * res;
    const int hi = res - 1;
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= 0 && pz <= hi; };
    auto on_border = [&](int px, int pz) { return px == 0 || px == hi || pz == 0 || pz == hi; };
    const float INF = __builtin_inff();

    // this thread's four cells
    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;  // VEC: res % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill ----
    float hc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wc[4] = {INF, INF, INF, INF};
    if (quad) {
        const float4 v = *reinterpret_cast<const float4 *>(h + c0);
        hc[0] = v.x, hc[1] = v.y, hc[2] = v.z, hc[3] = v.w;
        if constexpr (!FIRST) {
            const float4 w = *reinterpret_cast<const float4 *>(w_in + c0);
            wc[0] = w.x, wc[1] = w.y, wc[2] = w.z, wc[3] = w.w;
        }
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            hc[j] = h[c0 + j];
            if constexpr (!FIRST) wc[j] = w_in[c0 + j];
        }
    }
    unsigned fixed = 0;  // bit j: own cell j is an outlet or lies outside the grid; it is never updated
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool in = row_in && px + j <= hi;
        const bool outlet = in && (on_border(px + j, pz) || hc[j] <= sea);
        if (!in || outlet) fixed |= 1u << j;
        if (FIRST && outlet) wc[j] = hc[j];
    }
    *reinterpret_cast<float4 *>(&W[(tz + 1) * LP + LC + tx]) = make_float4(wc[0], wc[1], wc[2], wc[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        float v = INF;
        if (inside(qx, qz)) {
            const size_t q = base + (size_t)qz * res + qx;
            if constexpr (FIRST) {
                const float hq = h[q];
                if (on_border(qx, qz) || hq <= sea) v = hq;
            } else {
                v = w_in[q];
            }
        }
        W[lz * LP + lx] = v;
    }
    __syncthreads();

    // ---- sweeps inside LDS, the ring frozen ----
    bool moved = FIRST;  // uniform over the workgroup
    for (int s = 0; s < sweeps; s++) {
        int ch = 0;
        if (fixed != 15u) {
            float up[6], v[6];  // up: the smaller of the rows above and below, columns px-1 .. px+4; v: the own row
            {
                const float *r0 = &W[tz * LP + LC + tx], *r1 = r0 + LP, *r2 = r1 + LP;
                const float4 a = *reinterpret_cast<const float4 *>(r0), b = *reinterpret_cast<const float4 *>(r1),
                             c = *reinterpret_cast<const float4 *>(r2);
                up[0] = fminf(r0[-1], r2[-1]), up[1] = fminf(a.x, c.x), up[2] = fminf(a.y, c.y), up[3] = fminf(a.z, c.z);
                up[4] = fminf(a.w, c.w), up[5] = fminf(r0[4], r2[4]);
                v[0] = r1[-1], v[1] = b.x, v[2] = b.y, v[3] = b.z, v[4] = b.w, v[5] = r1[4];
            }
            auto relax = [&](int j) {
                if (fixed >> j & 1u) return;
                const float mn = fminf(fminf(fminf(up[j], up[j + 1]), fminf(up[j + 2], v[j])), v[j + 2]);
                const float m = mn + eps;
                v[j + 1] = hc[j] > m ? hc[j] : m;
            };
            relax(0), relax(1), relax(2), relax(3);
            relax(2), relax(1), relax(0);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                ch |= __float_as_uint(v[j + 1]) != __float_as_uint(wc[j]);
                wc[j] = v[j + 1];
            }
        }
        if (!__syncthreads_or(ch)) break;  // (the barrier behind the read phase)
        moved = true;
        if (ch) *reinterpret_cast<float4 *>(&W[(tz + 1) * LP + LC + tx]) = make_float4(wc[0], wc[1], wc[2], wc[3]);
        __syncthreads();
    }

    // ---- store ----
    if (quad) {
        *reinterpret_cast<float4 *>(w_out + c0) = make_float4(wc[0], wc[1], wc[2], wc[3]);
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            w_out[c0 + j] = wc[j];
        }
    }
    if (tid == 0) {
        flags_out[me] = moved ? 1 : 0;
        if (!FIRST && moved) atomicAdd(&changed[pass % 3], 1);
    }
}

// all or nothing: the fixed point when the last pass that ran changed nothing, otherwise the heights as they were
__global__ __launch_bounds__(256) void fill_finalise_kernel(float *__restrict__ h, const float *__restrict__ w,
                                                            float *__restrict__ depth, int *status, size_t n) {
    const int passes = status[ST_PASSES];
    const bool converged = status[ST_CHANGED + (passes + 2) % 3] == 0;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[ST_CONVERGED] = converged ? 1 : 0;
    if (i >= n) return;
    if (converged) {
        const float hv = h[i], wv = w[i];
        h[i] = wv;
        if (depth) depth[i] = wv - hv;
    } else if (depth) {
        depth[i] = 0.0f;
    }
}

}  // namespace

int32_t nz_launch_fill_pass(hipStream_t s, const float *h, const float *w_in, float *w_out, int *status,
                            const unsigned char *flags_in, unsigned char *flags_out, float eps, float sea, int res, int count,
                            int pass, int sweeps) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid((res + FX - 1) / FX, (res + FZ - 1) / FZ, count);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(w_in) | reinterpret_cast<uintptr_t>(w_out);
    const bool vec = (bits & 15) == 0 && res % 4 == 0;  // a row, and with it a tile of the batch, starts 16-byte aligned
    if (pass == 0) {
        if (vec) NZ_LAUNCH((fill_pass_kernel<true, true>), grid, dim3(FT), 0, s, h, w_in, w_out, status, flags_in, flags_out, eps, sea, res, pass, sweeps);
        else NZ_LAUNCH((fill_pass_kernel<true, false>), grid, dim3(FT), 0, s, h, w_in, w_out, status, flags_in, flags_out, eps, sea, res, pass, sweeps);
    } else {
        if (vec) NZ_LAUNCH((fill_pass_kernel<false, true>), grid, dim3(FT), 0, s, h, w_in, w_out, status, flags_in, flags_out, eps, sea, res, pass, sweeps);
        else NZ_LAUNCH((fill_pass_kernel<false, false>), grid, dim3(FT), 0, s, h, w_in, w_out, status, flags_in, flags_out, eps, sea, res, pass, sweeps);
    }
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fill_finalise(hipStream_t s, float *h, const float *w, float *depth, int *status, size_t n) {
    if (n == 0) return NZ_OK;
    NZ_LAUNCH(fill_finalise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h, w, depth, status, n);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
