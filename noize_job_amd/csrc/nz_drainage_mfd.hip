// nz_drainage_mfd.hip -- multiple-flow drainage: slope-weighted flow accumulation of a heightmap (gfx950; new-framework feature).
//
// THE MODEL (include/noize_hip.h states it for the caller, tests/drainage_mfd_ref.py restates it in numpy):
//   Square tile res x res, row-major z * res + x, float32 throughout, every operation rounded once, no contraction, the
//   same in every float mode.  Outlets, neighbours k = 0..7 in the order W E S N SW SE NW NE, "a neighbour outside the tile
//   does not exist" and DIAG are step 1 of the fluvial model (nz_receiver.hpp); rain_c = rain * rainMap[c], or rain.
//   A cell c that is no outlet sends to every lower neighbour: s_k = h[c] - h[k] (times DIAG for k >= 4), k takes flow iff
//   s_k > 0; q_k = s_k / best with best the largest s_k; g_k = q_k ^ exponent by repeated multiplication; T the sum of the
//   g_k > 0, k ascending; w_k = g_k / T.  The plane: A[c] = rain_c; for k ascending over the neighbours whose weight towards
//   c is w > 0: A[c] = A[c] + (w * A[k]).
// Flow goes strictly downhill, so the flow graph is a DAG: a cell's final value is a fixed function of higher cells' final
// values, the fixed point is unique and every order of updates ends in the same floats -- nz_drainage.hip's argument with
// "forest" replaced by "DAG"; nothing in it needs a single receiver.
//
// The setup launch, once per call, on the geometry of nz_tile64.hpp: heights at radius 2 into LDS as nz_donor_front.hpp
// stages them, `best` and T of the cells at radius 1 (+0 for a cell that sends nothing: an outlet, a cell outside the
// grid), and per own cell the eight INCOMING weights -- plane k holds what neighbour k sends to the cell, +0 where nothing
// arrives -- as eight float planes in `work`.  A border cell is an outlet, so a cell that sends has all eight neighbours,
// and "exists" needs no test of its own.  This launch holds all the divisions; after it no launch looks at a height.
//
// One launch per PASS of A, by the pass protocol of nz_relax_pass.hpp; the caller's `drainage` is plane 0.  A pass is
// nz_drainage.hip's with the donor byte replaced by the thread's 32 weights, loaded once (eight 16-byte loads on the vector
// path) and kept in registers across the sweeps: the passes are a pure gather with coalesced loads.  The gate of a gather
// is w > 0, never the value of A.  The finalise launch is nz_drainage.hip's (nz_launch_drainage_finalise).
// There is no row-stripe form.
#include "nz_internal.hpp"
#include "nz_mfd_weights.hpp"
#include "nz_receiver.hpp"
#include "nz_relax_pass.hpp"
#include "nz_tile64.hpp"

namespace {

using namespace nz_tile64;  // the tile, its LDS layout, ring_cell, halo2_cell
using namespace nz_relax;   // the status words and the pass protocol
using nz_mfd::mfd_power;     // the weights of a cell: shared with nz_fluvial_implicit_mfd.hip
using nz_mfd::mfd_send_terms;

// ---- the setup launch: heights -> eight planes of incoming weights ----
// VEC: 16-byte accesses to the float planes (all planes 16-byte aligned, res % 4 == 0); plane: the floats of one weight plane
template <bool VEC>
__global__ __launch_bounds__(FT) void mfd_setup_kernel(const float *__restrict__ h, float *__restrict__ wts, size_t plane,
                                                       float sea, int res, int exponent) {
    __shared__ __attribute__((aligned(16))) float H[(FZ + 4) * LP];  // radius 2: LDS row = plane row - z0 + 2
    __shared__ __attribute__((aligned(16))) float B[(FZ + 2) * LP];  // radius 1: `best`, +0 for a cell that sends nothing
    __shared__ __attribute__((aligned(16))) float T[(FZ + 2) * LP];  // radius 1: T
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FX, z0 = blockIdx.y * FZ;
    const size_t base = (size_t)blockIdx.z * res * res;
    const int hi = res - 1;
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= 0 && pz <= hi; };
    auto sends = [&](int px, int pz, float v) {  // no outlet: the border and the sea are; a cell outside the grid is none
        return px > 0 && px < hi && pz > 0 && pz < hi && !(v <= sea);
    };

    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = pz <= hi;
    const bool quad = row_in && px + 3 <= hi;

    // ---- fill: a cell outside the grid reads as +0 and sends nothing ----
    float hc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (VEC && quad) {
        const float4 v = *reinterpret_cast<const float4 *>(h + c0);
        hc[0] = v.x, hc[1] = v.y, hc[2] = v.z, hc[3] = v.w;
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            hc[j] = h[c0 + j];
        }
    }
    *reinterpret_cast<float4 *>(&H[(tz + 2) * LP + LC + tx]) = make_float4(hc[0], hc[1], hc[2], hc[3]);
    for (int i = tid; i < NHALO2; i += FT) {  // the heights at radius 1 and 2
        int lz, lx;
        halo2_cell(i, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 2;
        H[lz * LP + lx] = inside(qx, qz) ? h[base + (size_t)qz * res + qx] : 0.0f;
    }
    __syncthreads();

    // ---- `best` and T at radius 1 ----
    {
        float b[4] = {0.0f, 0.0f, 0.0f, 0.0f}, t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float *p = &H[(tz + 2) * LP + LC + tx + j];
            if (sends(px + j, pz, p[0])) mfd_send_terms(p, exponent, b[j], t[j]);
        }
        *reinterpret_cast<float4 *>(&B[(tz + 1) * LP + LC + tx]) = make_float4(b[0], b[1], b[2], b[3]);
        *reinterpret_cast<float4 *>(&T[(tz + 1) * LP + LC + tx]) = make_float4(t[0], t[1], t[2], t[3]);
    }
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const float *p = &H[(lz + 1) * LP + lx];
        float b = 0.0f, t = 0.0f;
        if (sends(x0 + lx - LC, z0 + lz - 1, p[0])) mfd_send_terms(p, exponent, b, t);
        B[lz * LP + lx] = b;
        T[lz * LP + lx] = t;
    }
    __syncthreads();

    // ---- the incoming weights of the own cells ----
    if (!row_in || px > hi) return;
    float w[8][4];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int dx = k == 2 || k == 3 ? 0 : (k & 1) ? 1 : -1;
        const int dz = k < 2 ? 0 : (k == 3 || k >= 6) ? 1 : -1;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int l = (tz + 1 + dz) * LP + LC + tx + j + dx;  // neighbour k in a radius-1 plane
            const float b = B[l];
            float v = 0.0f;
            if (b > 0.0f) {  // the neighbour sends; towards this cell it looks in the direction opposite to k
                const float d = H[l + LP] - H[(tz + 2) * LP + LC + tx + j];
                const float s = k < 4 ? d : d * nz_recv::DIAG;
                if (s > 0.0f) {
                    const float g = mfd_power(s / b, exponent);
                    if (g > 0.0f) v = g / T[l];
                }
            }
            w[k][j] = v;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        float *out = wts + (size_t)k * plane + c0;
        if (VEC && quad) {
            *reinterpret_cast<float4 *>(out) = make_float4(w[k][0], w[k][1], w[k][2], w[k][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (px + j > hi) break;
                out[j] = w[k][j];
            }
        }
    }
}

// ---- a pass ----
// FIRST: the start state rain_c, no A plane is read; VEC: 16-byte accesses to the float planes (all planes 16-byte aligned,
// res % 4 == 0); MAP: rain_c = rain * rain_map[c]
template <bool FIRST, bool VEC, bool MAP>
__global__ __launch_bounds__(FT) void mfd_pass_kernel(const float *__restrict__ wts, size_t plane,
                                                      const float *__restrict__ rain_map, const float *__restrict__ a_in,
                                                      float *__restrict__ a_out, int *status,
                                                      const unsigned char *__restrict__ flags_in,
                                                      unsigned char *__restrict__ flags_out, float rain, int res, int pass,
                                                      int sweeps) {
    __shared__ __attribute__((aligned(16))) float A[(FZ + 2) * LP];  // radius 1: LDS row = plane row - z0 + 1
    const int tid = threadIdx.x;
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
    auto rain_at = [&](size_t q) { return MAP ? rain * rain_map[q] : rain; };

    // this thread's four cells
    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;  // VEC: res % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill ----
    float rc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ac[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float w[8][4];  // the incoming weights of the own cells; a cell outside the grid has none
#pragma unroll
    for (int k = 0; k < 8; k++) w[k][0] = w[k][1] = w[k][2] = w[k][3] = 0.0f;
    if (quad) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float4 v = *reinterpret_cast<const float4 *>(wts + (size_t)k * plane + c0);
            w[k][0] = v.x, w[k][1] = v.y, w[k][2] = v.z, w[k][3] = v.w;
        }
        if constexpr (MAP) {
            const float4 m = *reinterpret_cast<const float4 *>(rain_map + c0);
            rc[0] = rain * m.x, rc[1] = rain * m.y, rc[2] = rain * m.z, rc[3] = rain * m.w;
        } else {
            rc[0] = rc[1] = rc[2] = rc[3] = rain;
        }
        if constexpr (!FIRST) {
            const float4 a = *reinterpret_cast<const float4 *>(a_in + c0);
            ac[0] = a.x, ac[1] = a.y, ac[2] = a.z, ac[3] = a.w;
        }
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
#pragma unroll
            for (int k = 0; k < 8; k++) w[k][j] = wts[(size_t)k * plane + c0 + j];
            rc[j] = rain_at(c0 + j);
            if constexpr (!FIRST) ac[j] = a_in[c0 + j];
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
        float v = 0.0f;  // a ring cell outside the grid holds +0 and is never gathered: its weight is +0
        if (inside(qx, qz)) {
            const size_t q = base + (size_t)qz * res + qx;
            if constexpr (FIRST) v = rain_at(q);
            else v = a_in[q];
        }
        A[lz * LP + lx] = v;
    }
    bool gathers = false;  // a thread without a positive weight holds rain_c for good
#pragma unroll
    for (int k = 0; k < 8; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) gathers |= w[k][j] > 0.0f;
    __syncthreads();

    // ---- sweeps inside LDS, the ring frozen ----
    bool moved = FIRST;  // uniform over the workgroup
    for (int s = 0; s < sweeps; s++) {
        int ch = 0;
        if (gathers) {
            float lo[6], up[6], v[6];  // rows pz-1 (S), pz+1 (N) and the own row, columns px-1 .. px+4
            {
                const float *r0 = &A[tz * LP + LC + tx], *r1 = r0 + LP, *r2 = r1 + LP;
                const float4 a = *reinterpret_cast<const float4 *>(r0), b = *reinterpret_cast<const float4 *>(r1),
                             c = *reinterpret_cast<const float4 *>(r2);
                lo[0] = r0[-1], lo[1] = a.x, lo[2] = a.y, lo[3] = a.z, lo[4] = a.w, lo[5] = r0[4];
                v[0] = r1[-1], v[1] = b.x, v[2] = b.y, v[3] = b.z, v[4] = b.w, v[5] = r1[4];
                up[0] = r2[-1], up[1] = c.x, up[2] = c.y, up[3] = c.z, up[4] = c.w, up[5] = r2[4];
            }
            // One update of own cell j: the model's gather, k ascending, product first, then sum.  `ch` sees EVERY update,
            // not the net effect of the sweep (nz_drainage.hip, `relax`).
            auto relax = [&](int j) {
                float a = rc[j];
                if (w[0][j] > 0.0f) a = a + w[0][j] * v[j];
                if (w[1][j] > 0.0f) a = a + w[1][j] * v[j + 2];
                if (w[2][j] > 0.0f) a = a + w[2][j] * lo[j + 1];
                if (w[3][j] > 0.0f) a = a + w[3][j] * up[j + 1];
                if (w[4][j] > 0.0f) a = a + w[4][j] * lo[j];
                if (w[5][j] > 0.0f) a = a + w[5][j] * lo[j + 2];
                if (w[6][j] > 0.0f) a = a + w[6][j] * up[j];
                if (w[7][j] > 0.0f) a = a + w[7][j] * up[j + 2];
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
        *reinterpret_cast<float4 *>(a_out + c0) = make_float4(ac[0], ac[1], ac[2], ac[3]);
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            a_out[c0 + j] = ac[j];
        }
    }
    if (t0) close_tile<FIRST>(status, flags_out, me, pass, moved);
}

}  // namespace

int32_t nz_launch_drainage_mfd_setup(hipStream_t s, const float *h, float *wts, float sea, int res, int count, int exponent) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const size_t plane = (size_t)res * res * count;
    const bool vec = res % 4 == 0 && ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(wts)) & 15) == 0;
    if (vec) NZ_LAUNCH(mfd_setup_kernel<true>, grid, dim3(FT), 0, s, h, wts, plane, sea, res, exponent);
    else NZ_LAUNCH(mfd_setup_kernel<false>, grid, dim3(FT), 0, s, h, wts, plane, sea, res, exponent);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_drainage_mfd_pass(hipStream_t s, const float *wts, const float *rain_map, const float *a_in, float *a_out,
                                    int *status, const unsigned char *flags_in, unsigned char *flags_out, float rain, int res,
                                    int count, int pass, int sweeps) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const size_t plane = (size_t)res * res * count;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(rain_map) | reinterpret_cast<uintptr_t>(a_in) |
                           reinterpret_cast<uintptr_t>(a_out) | reinterpret_cast<uintptr_t>(wts);
    const bool vec = (bits & 15) == 0 && res % 4 == 0;  // a row, a tile of the batch and a weight plane start 16-byte aligned
    nz_with_bools([&](auto first, auto v, auto map) {
        NZ_LAUNCH((mfd_pass_kernel<decltype(first)::value, decltype(v)::value, decltype(map)::value>), grid, dim3(FT), 0, s, wts,
                  plane, rain_map, a_in, a_out, status, flags_in, flags_out, rain, res, pass, sweeps);
    }, pass == 0, vec, rain_map != nullptr);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
