// nz_fluvial_implicit_mfd.hip -- multiple-flow implicit stream-power erosion: one large time step as one solve along EVERY
// descent of a cell (gfx950; new-framework feature).
//
// THE MODEL (include/noize_hip.h states it for the caller, tests/fluvial_implicit_mfd_ref.py restates it as a walk lowest
// cell first):
//   Square tile res x res, row-major c = z * res + x, float32 heights and drainage A, read only.  Outlets, neighbours
//   k = 0..7 in the order W E S N SW SE NW NE, DIAG, du, kc and b are nz_fluvial_implicit's (nz_fluvial_implicit.hip); the
//   outgoing weights w_k of a cell are nz_drainage_mfd's at `exponent` (nz_mfd_weights.hpp: the same device code).
//   outlet:                         h'[c] = h[c]
//   no k with w_k > 0 (pit, flat):  h'[c] = b = h[c] + du           (not through the division)
//   otherwise:  e = kc * sqrt(A[c]),  f_k = ((e * invL_k) * dt) * w_k for every k with w_k > 0,
//               N = b, D = 1; for k ascending with w_k > 0: N = N + (f_k * h'[k]), D = D + f_k;  h'[c] = N / D
//   invL_k = 1 for k < 4, 0x1.6a09e6p-1f for k >= 4; every operation rounded once to float32, no contraction, the
//   division and the square root correctly rounded.  The gate is w_k > 0, never the value of f_k or of h'.
// Every neighbour that takes flow is strictly lower in the OLD heights, so the flow graph is a DAG whose leaves (outlets,
// pits, flats) are fixed from the start: a cell's final value is a fixed function of the final values of lower cells, the
// fixed point is unique and every order of updates -- a walk lowest cell first, Jacobi, tile-local sweeps -- ends in the
// same bits, from any start.  It is nz_fluvial_implicit.hip's argument with "forest" replaced by "DAG", as
// nz_drainage_mfd.hip's is nz_drainage.hip's.  A cell with exactly one positive weight has w == 1 (g / g) and so the f, N
// and D of nz_fluvial_implicit: the same bits, given the same A and an equal h' below it.
//
// The begin launch and the finalise launch are nz_fluvial_implicit.hip's (nz_launch_fluvial_implicit_begin / _finalise):
// status[ST_GO] from the caller's `proceed` word; the verdict, the tally and out = h when the series did not come to rest.
//
// The setup launch, once per call, on the geometry of nz_tile64.hpp: heights at radius 1 into LDS (outgoing weights need
// no radius 2), A and the two maps of the own cells, and per own cell into `work` the GATE BYTE (bit k: w_k > 0), b (the
// final value of a cell without a gate: h on an outlet, h + du in a pit) and the eight planes f_k, +0 where w_k is not > 0.
// This launch holds every square root and every weight division; after it no pass looks at a height, A or a map.
// D is NOT stored: a thread rebuilds the D of its four cells once per pass from the f it holds in registers anyway, at
// most eight additions per cell.  A stored D plane was built and timed beside this form: no faster,
// and four more bytes per cell of `work`.
//
// One launch per PASS, by the pass protocol of nz_relax_pass.hpp; the caller's `out` is plane 0 of the h' pair.  A pass is
// nz_drainage_mfd.hip's with A replaced by h', rain_c by b, and the sum closed by one division: the thread's 32 f are
// loaded once (eight 16-byte loads on the vector path) and kept in registers across the sweeps, h' sits at radius 1 in LDS
// (18 x 72 floats), every thread updates its four cells left to right and back with a W or E neighbour among its own four
// taken from the register, "changed" looks at every single update, by bits.  The first pass starts every cell at its b.
// A thread whose four cells have no gate skips the sweeps.  A ring cell outside the grid holds +0 and is never read: a
// border cell is an outlet.
// There is no row-stripe form and no in-place form.
#include "nz_internal.hpp"
#include "nz_mfd_weights.hpp"
#include "nz_receiver.hpp"
#include "nz_relax_pass.hpp"
#include "nz_tile64.hpp"

namespace {

using namespace nz_tile64;  // the tile, its LDS layout, ring_cell
using namespace nz_relax;   // the status words and the pass protocol

constexpr float INV_DIAG = 0x1.6a09e6p-1f;  // 1 / L of a diagonal move, as in nz_fluvial_implicit.hip

// ---- the setup launch: heights, A, maps -> gate bytes, b, eight planes f ----
// VEC: 16-byte accesses to every float plane and a 32-bit store of the four gate bytes (res % 4 == 0); plane: the floats
// of one f plane
template <bool VEC>
__global__ __launch_bounds__(FT) void fluvial_mfd_setup_kernel(const float *__restrict__ h, const float *__restrict__ area,
                                                               const float *__restrict__ hardness,
                                                               const float *__restrict__ uplift_map,
                                                               unsigned char *__restrict__ gate, float *__restrict__ bco,
                                                               float *__restrict__ fco, size_t plane, const int *status,
                                                               float erodibility, float uplift, float dt, float sea, int res,
                                                               int exponent) {
    __shared__ __attribute__((aligned(16))) float H[(FZ + 2) * LP];  // radius 1: LDS row = plane row - z0 + 1
    if (!status[ST_GO]) return;

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FX, z0 = blockIdx.y * FZ;
    const size_t base = (size_t)blockIdx.z * res * res;
    const int hi = res - 1;  // last column and row
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= 0 && pz <= hi; };
    auto on_border = [&](int px, int pz) { return px == 0 || px == hi || pz == 0 || pz == hi; };

    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;  // VEC: res % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill: a cell outside the grid reads as +0 and decides nothing (a border cell sends nothing by rule) ----
    float hc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ac[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float hd[4] = {0.0f, 0.0f, 0.0f, 0.0f}, um[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    auto load4 = [&](const float *p, float (&o)[4]) {
        if (!p) return;
        if (quad) {
            const float4 v = *reinterpret_cast<const float4 *>(p + c0);
            o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
        } else if (!VEC && row_in) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (px + j <= hi) o[j] = p[c0 + j];
        }
    };
    load4(h, hc);
    load4(area, ac);
    load4(hardness, hd);
    load4(uplift_map, um);
    *reinterpret_cast<float4 *>(&H[(tz + 1) * LP + LC + tx]) = make_float4(hc[0], hc[1], hc[2], hc[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        H[lz * LP + lx] = inside(qx, qz) ? h[base + (size_t)qz * res + qx] : 0.0f;
    }
    __syncthreads();

    // ---- the gates of the own cells, none for an outlet, a pit and a flat, and the coefficients ----
    if (!row_in || px > hi) return;
    const float dtu = dt * uplift;
    unsigned word = 0;
    float b[4], f[8][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool outlet = on_border(px + j, pz) || hc[j] <= sea;
        const float du = uplift_map ? dtu * um[j] : dtu;
        const float kc = hardness ? erodibility * (1.0f - hd[j]) : erodibility;
        b[j] = outlet ? hc[j] : hc[j] + du;
        float w[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        // no outlet and inside the grid: all eight neighbours exist (a cell past the last column is never stored)
        if (!outlet && px + j <= hi) nz_mfd::mfd_out_weights(&H[(tz + 1) * LP + LC + tx + j], exponent, w);
        const float e = kc * sqrtf(ac[j]);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const bool on = w[k] > 0.0f;
            f[k][j] = on ? ((e * (k < 4 ? 1.0f : INV_DIAG)) * dt) * w[k] : 0.0f;
            word |= (on ? 1u : 0u) << (8 * j + k);
        }
    }
    if (quad) {
        *reinterpret_cast<unsigned *>(gate + c0) = word;
        *reinterpret_cast<float4 *>(bco + c0) = make_float4(b[0], b[1], b[2], b[3]);
#pragma unroll
        for (int k = 0; k < 8; k++)
            *reinterpret_cast<float4 *>(fco + (size_t)k * plane + c0) = make_float4(f[k][0], f[k][1], f[k][2], f[k][3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            gate[c0 + j] = (unsigned char)(word >> (8 * j));
            bco[c0 + j] = b[j];
#pragma unroll
            for (int k = 0; k < 8; k++) fco[(size_t)k * plane + c0 + j] = f[k][j];
        }
    }
}

// ---- a pass ----
// FIRST: the start state h' = b, no h' plane is read; VEC: 16-byte accesses to the float planes and a 32-bit one to the
// gate bytes (all planes 16-byte aligned, the bytes 4-byte, res % 4 == 0)
template <bool FIRST, bool VEC>
__global__ __launch_bounds__(FT) void fluvial_mfd_pass_kernel(const unsigned char *__restrict__ gate,
                                                              const float *__restrict__ bco, const float *__restrict__ fco,
                                                              size_t plane, const float *__restrict__ h_in,
                                                              float *__restrict__ h_out, int *status,
                                                              const unsigned char *__restrict__ flags_in,
                                                              unsigned char *__restrict__ flags_out, int res, int pass,
                                                              int sweeps) {
    __shared__ __attribute__((aligned(16))) float HN[(FZ + 2) * LP];  // h' at radius 1: LDS row = plane row - z0 + 1
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
    const int hi = res - 1;  // last column and row
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= 0 && pz <= hi; };

    // this thread's four cells
    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;  // VEC: res % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill ----
    unsigned msk = 0;  // the gate bytes of the own cells; a cell outside the grid has none and is not stored
    float bc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, hc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float fc[8][4];
#pragma unroll
    for (int k = 0; k < 8; k++) fc[k][0] = fc[k][1] = fc[k][2] = fc[k][3] = 0.0f;
    if (quad) {
        msk = *reinterpret_cast<const unsigned *>(gate + c0);
        const float4 b = *reinterpret_cast<const float4 *>(bco + c0);
        bc[0] = b.x, bc[1] = b.y, bc[2] = b.z, bc[3] = b.w;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float4 v = *reinterpret_cast<const float4 *>(fco + (size_t)k * plane + c0);
            fc[k][0] = v.x, fc[k][1] = v.y, fc[k][2] = v.z, fc[k][3] = v.w;
        }
        if constexpr (!FIRST) {
            const float4 v = *reinterpret_cast<const float4 *>(h_in + c0);
            hc[0] = v.x, hc[1] = v.y, hc[2] = v.z, hc[3] = v.w;
        }
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            msk |= (unsigned)gate[c0 + j] << (8 * j);
            bc[j] = bco[c0 + j];
#pragma unroll
            for (int k = 0; k < 8; k++) fc[k][j] = fco[(size_t)k * plane + c0 + j];
            if constexpr (!FIRST) hc[j] = h_in[c0 + j];
        }
    }
    if constexpr (FIRST) {
#pragma unroll
        for (int j = 0; j < 4; j++) hc[j] = bc[j];
    }
    *reinterpret_cast<float4 *>(&HN[(tz + 1) * LP + LC + tx]) = make_float4(hc[0], hc[1], hc[2], hc[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        float v = 0.0f;  // a ring cell outside the grid holds +0 and is never read: no gate points at it
        if (inside(qx, qz)) v = (FIRST ? bco : h_in)[base + (size_t)qz * res + qx];
        HN[lz * LP + lx] = v;
    }
    // D of the own cells, the model's sum: k ascending over the gates
    float dn[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float d = 1.0f;
#pragma unroll
        for (int k = 0; k < 8; k++)
            if ((msk >> (8 * j + k)) & 1u) d = d + fc[k][j];
        dn[j] = d;
    }
    __syncthreads();

    // ---- sweeps inside LDS, the ring frozen ----
    bool moved = FIRST;  // uniform over the workgroup
    for (int s = 0; s < sweeps; s++) {
        int ch = 0;
        if (msk != 0u) {  // a thread without a gate holds its final values from the start
            float lo[6], up[6], v[6];  // rows pz-1 (S), pz+1 (N) and the own row, columns px-1 .. px+4
            {
                const float *r0 = &HN[tz * LP + LC + tx], *r1 = r0 + LP, *r2 = r1 + LP;
                const float4 a = *reinterpret_cast<const float4 *>(r0), c = *reinterpret_cast<const float4 *>(r2);
                lo[0] = r0[-1], lo[1] = a.x, lo[2] = a.y, lo[3] = a.z, lo[4] = a.w, lo[5] = r0[4];
                v[0] = r1[-1], v[1] = hc[0], v[2] = hc[1], v[3] = hc[2], v[4] = hc[3], v[5] = r1[4];
                up[0] = r2[-1], up[1] = c.x, up[2] = c.y, up[3] = c.z, up[4] = c.w, up[5] = r2[4];
            }
            // One update of own cell j: the model's sums, k ascending, product first, and the one division.  `ch` sees
            // EVERY update, not the net effect of the sweep (nz_fluvial_implicit.hip, `relax`).
            auto relax = [&](int j) {
                const unsigned m = (msk >> (8 * j)) & 255u;
                if (!m) return;
                float n = bc[j];
                if (m & 1u) n = n + fc[0][j] * v[j];
                if (m & 2u) n = n + fc[1][j] * v[j + 2];
                if (m & 4u) n = n + fc[2][j] * lo[j + 1];
                if (m & 8u) n = n + fc[3][j] * up[j + 1];
                if (m & 16u) n = n + fc[4][j] * lo[j];
                if (m & 32u) n = n + fc[5][j] * lo[j + 2];
                if (m & 64u) n = n + fc[6][j] * up[j];
                if (m & 128u) n = n + fc[7][j] * up[j + 2];
                const float r = n / dn[j];
                ch |= __float_as_uint(r) != __float_as_uint(v[j + 1]);
                v[j + 1] = r;
            };
            relax(0), relax(1), relax(2), relax(3);
            relax(2), relax(1), relax(0);
#pragma unroll
            for (int j = 0; j < 4; j++) hc[j] = v[j + 1];
        }
        if (!__syncthreads_or(ch)) break;  // (the barrier behind the read phase)
        moved = true;
        if (ch) *reinterpret_cast<float4 *>(&HN[(tz + 1) * LP + LC + tx]) = make_float4(hc[0], hc[1], hc[2], hc[3]);
        __syncthreads();
    }

    // ---- store ----
    if (quad) {
        *reinterpret_cast<float4 *>(h_out + c0) = make_float4(hc[0], hc[1], hc[2], hc[3]);
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            h_out[c0 + j] = hc[j];
        }
    }
    if (t0) close_tile<FIRST>(status, flags_out, me, pass, moved);
}

}  // namespace

int32_t nz_launch_fluvial_implicit_mfd_setup(hipStream_t s, const float *h, const float *area, const float *hardness,
                                             const float *uplift_map, unsigned char *gate, float *bco, float *fco,
                                             const int *status, float erodibility, float uplift, float dt, float sea, int res,
                                             int count, int exponent) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const size_t plane = (size_t)res * res * count;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(area) |
                           reinterpret_cast<uintptr_t>(hardness) | reinterpret_cast<uintptr_t>(uplift_map) |
                           reinterpret_cast<uintptr_t>(bco) | reinterpret_cast<uintptr_t>(fco);
    // a row, a tile of the batch and an f plane start 16-byte aligned
    const bool vec = (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(gate) & 3) == 0 && res % 4 == 0;
    if (vec)
        NZ_LAUNCH(fluvial_mfd_setup_kernel<true>, grid, dim3(FT), 0, s, h, area, hardness, uplift_map, gate, bco, fco, plane,
                  status, erodibility, uplift, dt, sea, res, exponent);
    else
        NZ_LAUNCH(fluvial_mfd_setup_kernel<false>, grid, dim3(FT), 0, s, h, area, hardness, uplift_map, gate, bco, fco, plane,
                  status, erodibility, uplift, dt, sea, res, exponent);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_implicit_mfd_pass(hipStream_t s, const unsigned char *gate, const float *bco, const float *fco,
                                            const float *h_in, float *h_out, int *status, const unsigned char *flags_in,
                                            unsigned char *flags_out, int res, int count, int pass, int sweeps) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const size_t plane = (size_t)res * res * count;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(bco) | reinterpret_cast<uintptr_t>(fco) |
                           reinterpret_cast<uintptr_t>(h_in) | reinterpret_cast<uintptr_t>(h_out);
    const bool vec = (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(gate) & 3) == 0 && res % 4 == 0;
    nz_with_bools([&](auto first, auto v) {
        NZ_LAUNCH((fluvial_mfd_pass_kernel<decltype(first)::value, decltype(v)::value>), grid, dim3(FT), 0, s, gate, bco, fco,
                  plane, h_in, h_out, status, flags_in, flags_out, res, pass, sweeps);
    }, pass == 0, vec);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
