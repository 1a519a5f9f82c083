// nz_stream_order.hip -- stream order: Strahler order and river links of a heightmap (gfx950; new-framework feature).
//
// THE MODEL (include/noize_hip.h states it for the caller, tests/stream_order_ref.py restates it as a walk highest cell first):
//   Square tile res x res, row-major c = z * res + x, float32 heights, read only.  Outlets, neighbours k = 0..7 in the order
//   W E S N SW SE NW NE and the receiver r(c) are step 1 of the fluvial model (nz_receiver.hpp).
//   ch(c) = drainage == NULL ? true : drainage[c] >= threshold (one float32 comparison: a NaN is no channel), static.
//   D(c) = the existing neighbours k of c with r(k) == c and ch(k).
//   order[c] (uint8): !ch(c): 0; D(c) empty: 1; otherwise, m = max order[D(c)], n = #{d in D(c): order[d] == m}:
//   order[c] = m + (n >= 2 ? 1 : 0).
//   link[c] (int32, optional): !ch(c): -1; |D(c)| != 1: c (the index inside the cell's own tile); otherwise link[d] of the
//   one donor.
// A receiver is strictly lower than its donor, so the graph is a forest: a cell's final value is a fixed function of its
// donors' final values, the fixed point is unique and every order of updates -- a walk highest cell first, Jacobi,
// tile-local sweeps -- ends in the same bytes.  The data flow is nz_drainage.hip's, the same downstream gather over donor
// bits, on small integers.  The order rule is evaluated as max(m1, m2 + 1) with m1 >= m2 the two largest donor orders (0
// where there is none): m2 == m1 is "n >= 2", m2 < m1 leaves m1, no donor gives 1 -- the same value in every case, and a
// function that is monotone in every donor, so a series that starts at 1 never passes the fixed point and a byte holds
// every value on the way (the entry refuses 2^31 cells: order <= 31).
//
// The mask launch, once per call, on the geometry of nz_tile64.hpp (16-byte accesses where planes and pitch allow), is
// nz_donor_front.hpp's with the channel predicate on:
// heights at radius 2 into LDS, receiver codes at radius 1 with ch folded in -- a cell that is no channel gets the code
// NONE, it donates to nothing -- and per own cell one CHANNEL-DONOR BYTE: bit k set when neighbour k exists, drains into the
// cell and is a channel cell.  `drainage` is read at radius 1 only.  The start state of `order`, ch ? 1 : 0, goes into
// the caller's plane, so the cell's own ch needs no plane of its own: order > 0 <=> ch in every plane of the series.
// After it no launch looks at a height or at `drainage`, except finalise when it restores the start state.
//
// One launch per PASS, by the pass protocol of nz_relax_pass.hpp -- gate, tile skip, sweeps against a frozen ring, the
// closing byte and word, and the argument for them.  The caller's `order` and `link` are plane 0 of each pair; pass p reads
// plane p & 1 and writes the other (the first pass reads the start state the mask launch left in `order`), and pass 1
// writes all of plane 0, so a series at rest holds the fixed point in both.  What is this stage's own:
//   fill     the four donor bytes and the four orders of the thread's cells as one register word each, `order` at radius 1
//            into LDS as bytes (18 x 72 B, held as words), with LINK an int32 plane beside it (18 x 72 x 4 B); a ring cell
//            outside the grid holds 0 and is never gathered (its donor bit is clear).  The first pass reads no link plane:
//            it derives the start state, ch ? own index : -1, from the order bytes.
//   sweeps   every thread updates its four cells left to right and back (Gauss-Seidel inside the thread, Jacobi between
//            threads); "changed" looks at every single update of either plane (`relax`).  `link` is a copy from the one
//            donor when the donor byte has one bit, else the own index, which the start state holds already.  A thread
//            whose channel cells all have no donor is at rest for good.
// LINK, a template parameter as LEN is in the watershed kernel: an order-only call carries no 4-byte plane.
// The finalise launch sets the protocol's verdict and, when the last pass that ran did change something, puts the start
// state back from `drainage` and `threshold`: all or nothing.
#include "nz_internal.hpp"
#include "nz_receiver.hpp"
#include "nz_relax_pass.hpp"
#include "nz_tile64.hpp"
#include "nz_donor_front.hpp"

namespace {

using namespace nz_tile64;  // the tile, its LDS layout, ring_cell, window_bytes, neighbour_lds
using namespace nz_relax;   // the status words and the pass protocol

// ---- the mask launch: heights and drainage -> channel-donor bytes and the start state of `order` (nz_donor_front.hpp,
// with the channel predicate) ----
template <bool VEC, bool WORD>
__global__ __launch_bounds__(FT) void stream_mask_kernel(const float *__restrict__ h, const float *__restrict__ drainage,
                                                         unsigned char *__restrict__ donors, unsigned char *__restrict__ order,
                                                         float sea, float threshold, int res) {
    nz_front::donor_front<VEC, WORD, false, true>(h, drainage, donors, order, sea, threshold, res, nz_front::win_rows{});
}

// ---- a pass ----
// FIRST: o_in holds the start state and no link plane is read; VEC: 32-bit accesses to the byte planes and 16-byte ones to
// the link planes (byte planes 4-byte and link planes 16-byte aligned, res % 4 == 0); LINK: the link plane travels with
// the orders
// The cap of 102 SGPRs is what eight waves per SIMD allow, as on the drainage pass.  Without it every form takes 104 to
// 106 and seven waves; with it the compiler keeps the values over in VGPR lanes (the table: DESIGN.md section 4, "stream
// order")
template <bool FIRST, bool VEC, bool LINK>
__global__ __launch_bounds__(FT) __attribute__((amdgpu_num_sgpr(102))) void stream_pass_kernel(const unsigned char *__restrict__ donors,
                                                         const unsigned char *__restrict__ o_in, unsigned char *__restrict__ o_out,
                                                         const int *__restrict__ l_in, int *__restrict__ l_out, int *status,
                                                         const unsigned char *__restrict__ flags_in,
                                                         unsigned char *__restrict__ flags_out, int res, int pass, int sweeps) {
    __shared__ __attribute__((aligned(16))) unsigned OW[(FZ + 2) * LP / 4];    // radius 1, one byte per cell: LDS row = plane row - z0 + 1
    __shared__ __attribute__((aligned(16))) int K[LINK ? (FZ + 2) * LP : 4];  // (no plane without LINK)
    unsigned char *OB = reinterpret_cast<unsigned char *>(OW);
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
    const int own = (int)((unsigned)pz * (unsigned)res + (unsigned)px);  // the index inside the tile: the start link
    const bool row_in = pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;  // VEC: res % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill ----
    unsigned don = 0, ow = 0;  // the donor bytes and the orders of the own cells; a cell outside the grid has 0 and 0
    int lc[4] = {-1, -1, -1, -1};
    if (quad) {
        don = *reinterpret_cast<const unsigned *>(donors + c0);
        ow = *reinterpret_cast<const unsigned *>(o_in + c0);
        if constexpr (LINK && !FIRST) {
            const int4 l = *reinterpret_cast<const int4 *>(l_in + c0);
            lc[0] = l.x, lc[1] = l.y, lc[2] = l.z, lc[3] = l.w;
        }
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            don |= (unsigned)donors[c0 + j] << (8 * j);
            ow |= (unsigned)o_in[c0 + j] << (8 * j);
            if constexpr (LINK && !FIRST) lc[j] = l_in[c0 + j];
        }
    }
    if constexpr (LINK && FIRST) {
#pragma unroll
        for (int j = 0; j < 4; j++) lc[j] = (ow >> (8 * j)) & 255u ? own + j : -1;
    }
    OW[((tz + 1) * LP + LC + tx) >> 2] = ow;
    if constexpr (LINK) *reinterpret_cast<int4 *>(&K[(tz + 1) * LP + LC + tx]) = make_int4(lc[0], lc[1], lc[2], lc[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        unsigned o = 0;
        int l = -1;
        if (inside(qx, qz)) {
            const int q = qz * res + qx;
            o = o_in[base + (size_t)q];
            if constexpr (LINK) l = FIRST ? (o ? q : -1) : l_in[base + (size_t)q];
        }
        OB[lz * LP + lx] = (unsigned char)o;
        if constexpr (LINK) K[lz * LP + lx] = l;
    }

    // order > 0 <=> ch: a cell that is no channel keeps 0 and -1 whatever drains into it, so its donor byte is dropped
    // here; what is left decides who has work at all
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (!((ow >> (8 * j)) & 255u)) don &= ~(255u << (8 * j));
    // LINK: where an own cell with ONE donor finds it, as an LDS cell (any other cell: itself, and it is not read)
    int at[4];
    if constexpr (LINK) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned d = (don >> (8 * j)) & 255u;
            at[j] = neighbour_lds(tz, tx, j, __popc(d) == 1 ? __ffs(d) - 1 : 8);
        }
    }
    __syncthreads();

    // ---- sweeps inside LDS, the ring frozen ----
    bool moved = FIRST;  // uniform over the workgroup
    for (int s = 0; s < sweeps; s++) {
        int ch = 0;
        if (don) {  // a thread whose channel cells have no donor holds its start state for good
            unsigned w[3][6];  // rows pz-1 (S) .. pz+1 (N), columns px-1 .. px+4
            window_bytes(OW, tz, tx, w);
            int nl[4] = {0, 0, 0, 0};
            if constexpr (LINK) {
#pragma unroll
                for (int j = 0; j < 4; j++) nl[j] = K[at[j]];
            }
            // One update of own cell j: the model's gather over the set bits, as the two largest donor orders.  `ch` sees
            // EVERY update of either plane, not the net effect of the sweep: a sweep that reports nothing has evaluated
            // each cell on the values now standing and found it at rest, which is what "fixed point against the ring"
            // means.
            auto relax = [&](int j) {
                const unsigned d = (don >> (8 * j)) & 255u;
                if (!d) return;  // no channel, or a head: the start state stands
                unsigned m1 = 0, m2 = 0;
                auto take = [&](int k, unsigned v) {
                    v &= (unsigned)((int)(d << (31 - k)) >> 31);  // bit k of d as a mask: 0 where neighbour k is no donor
                    m2 = max(m2, min(m1, v));
                    m1 = max(m1, v);
                };
                take(0, w[1][j]), take(1, w[1][j + 2]), take(2, w[0][j + 1]), take(3, w[2][j + 1]);
                take(4, w[0][j]), take(5, w[0][j + 2]), take(6, w[2][j]), take(7, w[2][j + 2]);
                const unsigned o = max(m1, m2 + 1u);
                ch |= o != w[1][j + 1];
                w[1][j + 1] = o;
                if constexpr (LINK) {
                    if (d & (d - 1u)) return;  // a confluence: its own index, which the start state holds
                    int l = nl[j];
                    if (d == 1u && j > 0) l = lc[j > 0 ? j - 1 : 0];  // a W or E donor among the own four
                    if (d == 2u && j < 3) l = lc[j < 3 ? j + 1 : 3];
                    ch |= l != lc[j];
                    lc[j] = l;
                }
            };
            relax(0), relax(1), relax(2), relax(3);
            relax(2), relax(1), relax(0);
            ow = w[1][1] | w[1][2] << 8 | w[1][3] << 16 | w[1][4] << 24;
        }
        if (!__syncthreads_or(ch)) break;  // (the barrier behind the read phase)
        moved = true;
        if (ch) {
            OW[((tz + 1) * LP + LC + tx) >> 2] = ow;
            if constexpr (LINK) *reinterpret_cast<int4 *>(&K[(tz + 1) * LP + LC + tx]) = make_int4(lc[0], lc[1], lc[2], lc[3]);
        }
        __syncthreads();
    }

    // ---- store ----
    if (quad) {
        *reinterpret_cast<unsigned *>(o_out + c0) = ow;
        if constexpr (LINK) *reinterpret_cast<int4 *>(l_out + c0) = make_int4(lc[0], lc[1], lc[2], lc[3]);
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            o_out[c0 + j] = (unsigned char)(ow >> (8 * j));
            if constexpr (LINK) l_out[c0 + j] = lc[j];
        }
    }
    if (t0) close_tile<FIRST>(status, flags_out, me, pass, moved);
}

// all or nothing: the fixed point stands in `order` and `link` when the last pass that ran changed nothing (a series at
// rest holds equal planes); otherwise the start state goes back in, from the one comparison that defines ch
template <bool LINK>
__global__ __launch_bounds__(256) void stream_finalise_kernel(unsigned char *__restrict__ order, int *__restrict__ link,
                                                              const float *__restrict__ drainage, int *status,
                                                              float threshold, unsigned cells, size_t n) {
    const bool converged = series_at_rest(status);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[ST_CONVERGED] = converged ? 1 : 0;
    if (i >= n || converged) return;
    const bool ch = drainage == nullptr || drainage[i] >= threshold;
    order[i] = ch ? 1 : 0;
    if constexpr (LINK) link[i] = ch ? (int)((unsigned)i % cells) : -1;  // n < 2^31 (the entry); the index inside the cell's own tile
}

}  // namespace

int32_t nz_launch_stream_mask(hipStream_t s, const float *h, const float *drainage, unsigned char *donors,
                              unsigned char *order, float sea, float threshold, int res, int count) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const bool word = res % 4 == 0 && ((reinterpret_cast<uintptr_t>(donors) | reinterpret_cast<uintptr_t>(order)) & 3) == 0;
    const bool vec = word && ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(drainage)) & 15) == 0;
    if (vec) NZ_LAUNCH((stream_mask_kernel<true, true>), grid, dim3(FT), 0, s, h, drainage, donors, order, sea, threshold, res);
    else if (word) NZ_LAUNCH((stream_mask_kernel<false, true>), grid, dim3(FT), 0, s, h, drainage, donors, order, sea, threshold, res);
    else NZ_LAUNCH((stream_mask_kernel<false, false>), grid, dim3(FT), 0, s, h, drainage, donors, order, sea, threshold, res);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_stream_pass(hipStream_t s, const unsigned char *donors, const unsigned char *o_in, unsigned char *o_out,
                              const int *l_in, int *l_out, int *status, const unsigned char *flags_in,
                              unsigned char *flags_out, int res, int count, int pass, int sweeps) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const uintptr_t bytes = reinterpret_cast<uintptr_t>(donors) | reinterpret_cast<uintptr_t>(o_in) |
                            reinterpret_cast<uintptr_t>(o_out);
    const uintptr_t ints = reinterpret_cast<uintptr_t>(l_in) | reinterpret_cast<uintptr_t>(l_out);
    // a row, and with it a tile of the batch, starts 4-byte aligned in the byte planes and 16-byte aligned in the links
    const bool vec = (bytes & 3) == 0 && (ints & 15) == 0 && res % 4 == 0;
    nz_with_bools([&](auto first, auto v, auto link) {
        NZ_LAUNCH((stream_pass_kernel<decltype(first)::value, decltype(v)::value, decltype(link)::value>), grid, dim3(FT), 0, s,
                  donors, o_in, o_out, l_in, l_out, status, flags_in, flags_out, res, pass, sweeps);
    }, pass == 0, vec, l_out != nullptr);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_stream_finalise(hipStream_t s, unsigned char *order, int *link, const float *drainage, int *status,
                                  float threshold, int res, size_t n) {
    if (n == 0) return NZ_OK;
    const dim3 grid((unsigned)((n + 255) / 256));
    const unsigned cells = (unsigned)res * (unsigned)res;
    if (link) NZ_LAUNCH(stream_finalise_kernel<true>, grid, dim3(256), 0, s, order, link, drainage, status, threshold, cells, n);
    else NZ_LAUNCH(stream_finalise_kernel<false>, grid, dim3(256), 0, s, order, link, drainage, status, threshold, cells, n);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
