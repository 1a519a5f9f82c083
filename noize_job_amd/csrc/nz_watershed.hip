// nz_watershed.hip -- watershed: basin labels, flow length and receiver codes of a heightmap (gfx950; new-framework feature).
//
// THE MODEL (include/noize_hip.h states it for the caller, tests/watershed_ref.py restates it as a walk lowest cell first):
//   Square tile res x res, row-major c = z * res + x, float32 heights, read only.  Outlets, neighbours k = 0..7 in the order
//   W E S N SW SE NW NE and the receiver r(c) are step 1 of the fluvial model (nz_receiver.hpp).  For every cell,
//   r(c) == NONE:  basin[c] = c (int32, the index inside the cell's own tile), length[c] = +0;
//   otherwise, q the neighbour r(c) names:  basin[c] = basin[q], length[c] = length[q] + step_k,
//   step_k = cellSize for k < 4 and cellSize * sqrt2 (0x1.6a09e6p+0f, one product rounded once, formed by the host) for k >= 4.
// A receiver is strictly lower than its donor, so the receiver graph is a forest: a cell's final value is a fixed function
// of ONE other cell's final value, the fixed point is unique and every order of updates -- a walk lowest cell first, Jacobi,
// tile-local sweeps -- ends in the same bits.  The data flow is nz_drainage.hip's reversed: a cell reads the one neighbour
// its code names instead of gathering up to eight donors, and it carries an int32 and a float plane together.
//
// The receiver launch, once per call, on the geometry of nz_tile64.hpp (16-byte accesses where planes and pitch allow):
// heights at radius 1 into LDS and per own cell one RECEIVER BYTE, the code 0..7 or NONE (receiver_codes4 of
// nz_donor_front.hpp) -- to the caller's `receivers` plane when it wants one, else to `work`.  After it no launch looks at
// a height.
//
// One launch per PASS, by the pass protocol of nz_relax_pass.hpp -- gate, tile skip, sweeps against a frozen ring, the
// closing byte and word, and the argument for them; the caller's `basin` and `length` are plane 0 of each pair.  What is
// this stage's own:
//   fill     the four receiver codes of the thread's cells in one register word, basin and length at radius 1 into LDS
//            (18 x 72 int32 and 18 x 72 floats); a ring cell outside the grid holds 0 and is never read (no own cell's
//            receiver points off the grid).  The first pass reads no plane: it derives the start state, own index and +0.
//   sweeps   every thread updates its four cells from the LDS cell its code names, left to right and back, a W or E
//            neighbour among its own four taken from the register (Gauss-Seidel inside the thread, Jacobi between
//            threads); "changed" looks at every single update of either value, by bits.  A thread whose four cells all
//            have no receiver is at rest for good.
// LEN, a template parameter as MAP is in the drainage kernel: a labels-only call carries no float plane, in LDS or registers.
// A series at rest holds the fixed point in BOTH planes of a pair, so the finalise launch has nothing to copy: it sets the
// protocol's verdict and, when the last pass that ran did change something, puts the start state back: all or nothing.
#include "nz_internal.hpp"
#include "nz_receiver.hpp"
#include "nz_relax_pass.hpp"
#include "nz_tile64.hpp"
#include "nz_donor_front.hpp"

namespace {

using nz_recv::NONE;
using namespace nz_tile64;  // the tile, its LDS layout, ring_cell, neighbour_lds
using namespace nz_relax;   // the status words and the pass protocol

constexpr unsigned NONE4 = NONE * 0x01010101u;  // the code word of four cells without a receiver

// ---- the receiver launch: heights -> receiver bytes ----
// VEC: 16-byte height reads; WORD: the four codes of a thread as one 32-bit store (res % 4 == 0)
template <bool VEC, bool WORD>
__global__ __launch_bounds__(FT) void watershed_receiver_kernel(const float *__restrict__ h, unsigned char *__restrict__ recv,
                                                                float sea, int res) {
    __shared__ __attribute__((aligned(16))) float H[(FZ + 2) * LP];  // radius 1: LDS row = plane row - z0 + 1

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
    const bool quad = row_in && px + 3 <= hi;

    // ---- fill: a cell outside the grid reads as +0 and decides nothing (a border cell has no receiver by rule) ----
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
    *reinterpret_cast<float4 *>(&H[(tz + 1) * LP + LC + tx]) = make_float4(hc[0], hc[1], hc[2], hc[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        H[lz * LP + lx] = inside(qx, qz) ? h[base + (size_t)qz * res + qx] : 0.0f;
    }
    __syncthreads();

    // ---- the receiver codes of the own cells: NONE for an outlet and for a pit ----
    if (!row_in || px > hi) return;
    const unsigned word = nz_front::receiver_codes4(H, tz, tx, sea, [&](int j) { return on_border(px + j, pz); });
    if (WORD && quad) {
        *reinterpret_cast<unsigned *>(recv + c0) = word;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            recv[c0 + j] = (unsigned char)(word >> (8 * j));
        }
    }
}

// ---- a pass ----
// FIRST: the start state, own index and +0, no plane is read; VEC: 16-byte accesses to the planes and a 32-bit one to the
// receiver bytes (all planes 16-byte aligned, res % 4 == 0); LEN: the length plane travels with the labels
template <bool FIRST, bool VEC, bool LEN>
__global__ __launch_bounds__(FT) void watershed_pass_kernel(const unsigned char *__restrict__ recv,
                                                            const int *__restrict__ b_in, int *__restrict__ b_out,
                                                            const float *__restrict__ l_in, float *__restrict__ l_out,
                                                            int *status, const unsigned char *__restrict__ flags_in,
                                                            unsigned char *__restrict__ flags_out, float cell, float diag,
                                                            int res, int pass, int sweeps) {
    __shared__ __attribute__((aligned(16))) int B[(FZ + 2) * LP];                // radius 1: LDS row = plane row - z0 + 1
    __shared__ __attribute__((aligned(16))) float L[LEN ? (FZ + 2) * LP : 4];  // (no plane without LEN)
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
    const int hi = res - 1;  // last column and row
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= 0 && pz <= hi; };

    // this thread's four cells
    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const int own = (int)((unsigned)pz * (unsigned)res + (unsigned)px);  // the index inside the tile: the start label
    const bool row_in = pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;  // VEC: res % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill ----
    unsigned cod = NONE4;  // the receiver codes of the own cells; a cell outside the grid has none and is not stored
    int bc[4] = {0, 0, 0, 0};
    float lc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (quad) {
        cod = *reinterpret_cast<const unsigned *>(recv + c0);
        if constexpr (!FIRST) {
            const int4 b = *reinterpret_cast<const int4 *>(b_in + c0);
            bc[0] = b.x, bc[1] = b.y, bc[2] = b.z, bc[3] = b.w;
            if constexpr (LEN) {
                const float4 l = *reinterpret_cast<const float4 *>(l_in + c0);
                lc[0] = l.x, lc[1] = l.y, lc[2] = l.z, lc[3] = l.w;
            }
        }
    } else if (!VEC && row_in) {
        cod = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool in = px + j <= hi;
            cod |= (in ? (unsigned)recv[c0 + j] : NONE) << (8 * j);
            if constexpr (!FIRST) {
                if (in) {
                    bc[j] = b_in[c0 + j];
                    if constexpr (LEN) lc[j] = l_in[c0 + j];
                }
            }
        }
    }
    if constexpr (FIRST) {
#pragma unroll
        for (int j = 0; j < 4; j++) bc[j] = own + j;
    }
    *reinterpret_cast<int4 *>(&B[(tz + 1) * LP + LC + tx]) = make_int4(bc[0], bc[1], bc[2], bc[3]);
    if constexpr (LEN) *reinterpret_cast<float4 *>(&L[(tz + 1) * LP + LC + tx]) = make_float4(lc[0], lc[1], lc[2], lc[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        int b = 0;
        float l = 0.0f;
        if (inside(qx, qz)) {
            const int q = qz * res + qx;
            if constexpr (FIRST) {
                b = q;
            } else {
                b = b_in[base + (size_t)q];
                if constexpr (LEN) l = l_in[base + (size_t)q];
            }
        }
        B[lz * LP + lx] = b;
        if constexpr (LEN) L[lz * LP + lx] = l;
    }

    // where each own cell looks: the LDS cell its code names (its own without a receiver), and the step of that move
    int at[4];
    float st[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned k = (cod >> (8 * j)) & 255u;
        at[j] = neighbour_lds(tz, tx, j, (int)k);
        st[j] = k < 4u ? cell : diag;
    }
    __syncthreads();

    // ---- sweeps inside LDS, the ring frozen ----
    bool moved = FIRST;  // uniform over the workgroup
    for (int s = 0; s < sweeps; s++) {
        int ch = 0;
        if (cod != NONE4) {  // a thread without a receiver holds its start state for good
            int nb[4];
            float nl[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                nb[j] = B[at[j]];
                nl[j] = LEN ? L[at[j]] : 0.0f;
            }
            // One update of own cell j: the model's assignment from the cell its code names.  `ch` sees EVERY update of
            // either value, not the net effect of the sweep: a sweep that reports nothing has evaluated each cell on the
            // values now standing and found it at rest, which is what "fixed point against the ring" means.
            auto relax = [&](int j) {
                const unsigned k = (cod >> (8 * j)) & 255u;
                if (k >= NONE) return;
                int b = nb[j];
                float l = nl[j];
                if (k == 0u && j > 0) b = bc[j > 0 ? j - 1 : 0], l = lc[j > 0 ? j - 1 : 0];  // W, E among the own four
                if (k == 1u && j < 3) b = bc[j < 3 ? j + 1 : 3], l = lc[j < 3 ? j + 1 : 3];
                ch |= b != bc[j];
                bc[j] = b;
                if constexpr (LEN) {
                    l = l + st[j];
                    ch |= __float_as_uint(l) != __float_as_uint(lc[j]);
                    lc[j] = l;
                }
            };
            relax(0), relax(1), relax(2), relax(3);
            relax(2), relax(1), relax(0);
        }
        if (!__syncthreads_or(ch)) break;  // (the barrier behind the read phase)
        moved = true;
        if (ch) {
            *reinterpret_cast<int4 *>(&B[(tz + 1) * LP + LC + tx]) = make_int4(bc[0], bc[1], bc[2], bc[3]);
            if constexpr (LEN) *reinterpret_cast<float4 *>(&L[(tz + 1) * LP + LC + tx]) = make_float4(lc[0], lc[1], lc[2], lc[3]);
        }
        __syncthreads();
    }

    // ---- store ----
    if (quad) {
        *reinterpret_cast<int4 *>(b_out + c0) = make_int4(bc[0], bc[1], bc[2], bc[3]);
        if constexpr (LEN) *reinterpret_cast<float4 *>(l_out + c0) = make_float4(lc[0], lc[1], lc[2], lc[3]);
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            b_out[c0 + j] = bc[j];
            if constexpr (LEN) l_out[c0 + j] = lc[j];
        }
    }
    if (t0) close_tile<FIRST>(status, flags_out, me, pass, moved);
}

// all or nothing: the fixed point stands in `basin` and `length` when the last pass that ran changed nothing (nz_watershed
// keeps them as plane 0 of each pair, and a series at rest holds equal planes); otherwise the start state goes back in
template <bool LEN>
__global__ __launch_bounds__(256) void watershed_finalise_kernel(int *__restrict__ basin, float *__restrict__ length, int *status,
                                                                 unsigned cells, size_t n) {
    const bool converged = series_at_rest(status);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[ST_CONVERGED] = converged ? 1 : 0;
    if (i >= n || converged) return;
    basin[i] = (int)((unsigned)i % cells);  // n < 2^31 (the entry); the index inside the cell's own tile
    if constexpr (LEN) length[i] = 0.0f;
}

}  // namespace

int32_t nz_launch_watershed_receivers(hipStream_t s, const float *h, unsigned char *recv, float sea, int res, int count) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const bool word = res % 4 == 0 && (reinterpret_cast<uintptr_t>(recv) & 3) == 0;
    const bool vec = res % 4 == 0 && (reinterpret_cast<uintptr_t>(h) & 15) == 0;
    if (vec && word) NZ_LAUNCH((watershed_receiver_kernel<true, true>), grid, dim3(FT), 0, s, h, recv, sea, res);
    else if (word) NZ_LAUNCH((watershed_receiver_kernel<false, true>), grid, dim3(FT), 0, s, h, recv, sea, res);
    else NZ_LAUNCH((watershed_receiver_kernel<false, false>), grid, dim3(FT), 0, s, h, recv, sea, res);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_watershed_pass(hipStream_t s, const unsigned char *recv, const int *b_in, int *b_out, const float *l_in,
                                 float *l_out, int *status, const unsigned char *flags_in, unsigned char *flags_out,
                                 float cell, float diag, int res, int count, int pass, int sweeps) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(b_in) | reinterpret_cast<uintptr_t>(b_out) |
                           reinterpret_cast<uintptr_t>(l_in) | reinterpret_cast<uintptr_t>(l_out);
    // a row, and with it a tile of the batch, starts 16-byte aligned in the planes and 4-byte aligned in the receiver bytes
    const bool vec = (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(recv) & 3) == 0 && res % 4 == 0;
    nz_with_bools([&](auto first, auto v, auto len) {
        NZ_LAUNCH((watershed_pass_kernel<decltype(first)::value, decltype(v)::value, decltype(len)::value>), grid, dim3(FT), 0,
                  s, recv, b_in, b_out, l_in, l_out, status, flags_in, flags_out, cell, diag, res, pass, sweeps);
    }, pass == 0, vec, l_out != nullptr);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_watershed_finalise(hipStream_t s, int *basin, float *length, int *status, int res, size_t n) {
    if (n == 0) return NZ_OK;
    const dim3 grid((unsigned)((n + 255) / 256));
    const unsigned cells = (unsigned)res * (unsigned)res;
    if (length) NZ_LAUNCH(watershed_finalise_kernel<true>, grid, dim3(256), 0, s, basin, length, status, cells, n);
    else NZ_LAUNCH(watershed_finalise_kernel<false>, grid, dim3(256), 0, s, basin, length, status, cells, n);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
