// nz_fluvial_implicit.hip -- implicit stream-power erosion: one large time step as one solve along the receiver tree
// (gfx950; new-framework feature).
//
// THE MODEL (include/noize_hip.h states it for the caller, tests/fluvial_implicit_ref.py restates it as a walk lowest cell
// first):
//   Square tile res x res, row-major c = z * res + x, float32 heights and drainage A, read only.  Outlets, neighbours
//   k = 0..7 in the order W E S N SW SE NW NE and the receiver r(c) are step 1 of the fluvial model (nz_receiver.hpp).
//   du = dt * uplift (times upliftMap[c] with a map), kc = erodibility (times 1 - hardness[c] with a map).
//   outlet:          h'[c] = h[c]
//   pit:             h'[c] = h[c] + du
//   otherwise, q the neighbour r(c) = k names:  b = h[c] + du,  f = ((kc * sqrt(A[c])) * invL_k) * dt,
//                    h'[c] = (b + f * h'[q]) / (1 + f),   invL_k = 1 for k < 4, 0x1.6a09e6p-1f for k >= 4
//   every operation rounded once to float32, no contraction, the division and the square root correctly rounded.
// This is the implicit Euler step of dh/dt = u - k sqrt(A) (h - h_r) / L (Braun & Willett 2013): stable for every dt.
// A receiver is strictly lower than its donor, so the receiver graph is a forest whose roots (outlets and pits) are fixed
// from the start: a cell's final value is a fixed function of ONE other cell's final value, the fixed point is unique and
// every order of updates -- a walk lowest cell first, Jacobi, tile-local sweeps -- ends in the same bits, from any start.
// It is nz_watershed.hip's data flow with a float recurrence in place of a label copy.
//
// The begin launch, one thread: status[ST_GO] from the caller's `proceed` word (none: go), the status words of a fresh
// series.  With ST_GO == 0 every later launch returns at once and the finalise launch writes out = h.
//
// The setup launch, once per call, on the geometry of nz_tile64.hpp (16-byte accesses where planes and pitch allow):
// heights at radius 1 into LDS, A and the maps of the own cells, and per own cell the RECEIVER BYTE (receiver_codes4 of
// nz_donor_front.hpp), b and f into `work`; a cell without a receiver gets its final value as b (h on an outlet, h + du in
// a pit) and f = +0.  The coefficients are STORED, not recomputed per pass: a pass then reads 13 bytes per cell and h',
// whatever maps the call has, instead of heights at radius 1, A and two maps, and runs no square root.  After the setup
// launch no pass looks at a height, A or a map.
//
// One launch per PASS, by the pass protocol of nz_relax_pass.hpp -- gate, tile skip, sweeps against a frozen ring, the
// closing byte and word; the caller's `out` is plane 0 of the h' pair.  What is this stage's own:
//   fill     the four receiver codes of the thread's cells in one register word, their b and f in registers, h' at radius
//            1 into LDS (18 x 72 floats); a ring cell outside the grid holds 0 and is never read.  The first pass reads no
//            h' plane: it starts every cell at its b -- the heights after uplift alone, and already final on the roots.
//            (The start state decides nothing but the pass count; the "nothing" of all or nothing is h, below.)
//   sweeps   every thread updates its four cells from the LDS cell its code names, left to right and back, a W or E
//            neighbour among its own four taken from the register; "changed" looks at every single update, by bits (a NaN
//            keeps its bits under the same operations, so a tile that holds one still comes to rest).
// The finalise launch: the verdict, the caller's tally, and when the series did not come to rest (or did not run) out = h:
// all or nothing.  It is the one launch behind the setup that reads a height, and only then.
//
// WIN, the stripe form (nz_implicit_fluvial_stripe_round), on the pattern of nz_drainage.hip's: one ROUND on the owned rows
// [r0, r1) of a stripe-shaped buffer with a pitch; the workgroups tile the owned rows, `res` is the pitch, the grid's bounds
// are the global grid's seen from the buffer.  The setup launch of a round with `first` reads heights one row beyond the
// owned ones and stores the receiver byte, b and f of the owned rows only, at the cells' plane indices.  The one row of h'
// on each side of the owned rows is FROZEN: read from the caller's plane in every pass (in a round with `first`: from the
// heights as they stand -- any start gives the same fixed point, and it needs no ghost row of A or of a map), never
// written, whichever of the two planes the pass alternates between.  When the owned rows end inside a tile, the frozen row
// lies in a thread's own slot: it is loaded, has no receiver byte and is not stored.  The round's begin and end launches
// are the fill stripe's; only the setup launch and pass 0 read status[GO] (the later passes of a round that does not go
// return at their gate); pass 0 of a round that continues from h' visits every tile, and stores 1 to the caller's
// `changed` word when any single update changed a bit.
#include "nz_internal.hpp"
#include "nz_receiver.hpp"
#include "nz_relax_pass.hpp"
#include "nz_tile64.hpp"
#include "nz_donor_front.hpp"

namespace {

using nz_recv::NONE;
using namespace nz_tile64;  // the tile, its LDS layout, ring_cell, neighbour_lds
using namespace nz_relax;   // the status words and the pass protocol

// WIN: the owned rows of one stripe-shaped buffer (nz_front::win_rows) and what the launches of a round need beside them
struct implicit_win : nz_front::win_rows {
    const float *ghost_h;  // a round with `first`: the heights, whose rows beside the owned ones are the frozen rows; else NULL
    int *changed_out;      // the caller's word
};

__device__ __forceinline__ implicit_win win_of() { return {}; }  // the tile forms
__device__ __forceinline__ const implicit_win &win_of(const implicit_win &w) { return w; }

constexpr unsigned NONE4 = NONE * 0x01010101u;  // the code word of four cells without a receiver
constexpr float INV_DIAG = 0x1.6a09e6p-1f;      // 1 / L of a diagonal move, as in nz_receiver.hpp's slopes

// ---- begin: go or not, and a fresh series ----
__global__ void fluvial_implicit_begin_kernel(int *status, const int *proceed) {
    status[ST_GO] = proceed ? *proceed != 0 : 1;
    status[ST_PASSES] = 0;
    status[ST_CONVERGED] = 0;
    status[ST_CHANGED] = status[ST_CHANGED + 1] = status[ST_CHANGED + 2] = 0;
}

// ---- the setup launch: heights, A, maps -> receiver bytes, b, f ----
// VEC: 16-byte accesses to every float plane and a 32-bit store of the four codes (res % 4 == 0); WIN: res is the pitch,
// the heights are read on the owned rows and the one beside them, everything else on the owned rows
// Win: the window as a trailing argument of the stripe form, {implicit_win}; the tile forms have none, {}, and keep their
// argument list.  Their bounds tests stay in their own words (`if constexpr` in inside / on_border): stated through
// zlo / zhi / rlo / rhi folded to constants, the tile forms compiled to 264 bytes and 8 SGPRs more.  The same holds for the
// pass (4 bytes).
template <bool VEC, bool WIN, class... Win>
__global__ __launch_bounds__(FT) void fluvial_implicit_setup_kernel(const float *__restrict__ h, const float *__restrict__ area,
                                                                    const float *__restrict__ hardness,
                                                                    const float *__restrict__ uplift_map,
                                                                    unsigned char *__restrict__ recv, float *__restrict__ bco,
                                                                    float *__restrict__ fco, const int *status,
                                                                    float erodibility, float uplift, float dt, float sea,
                                                                    int res, Win... window) {
    static_assert(sizeof...(Win) == (WIN ? 1 : 0));
    const implicit_win win = win_of(window...);
    __shared__ __attribute__((aligned(16))) float H[(FZ + 2) * LP];  // radius 1: LDS row = plane row - z0 + 1
    if (!status[ST_GO]) return;

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FX, z0 = (WIN ? win.r0 : 0) + blockIdx.y * FZ;
    const size_t base = WIN ? 0 : (size_t)blockIdx.z * res * res;
    const int hi = WIN ? win.xhi : res - 1;                            // last column
    const int zlo = WIN ? win.zlo : 0, zhi = WIN ? win.zhi : res - 1;  // the grid's rows
    const int rlo = WIN ? (zlo > win.r0 - 1 ? zlo : win.r0 - 1) : 0, rhi = WIN ? (zhi < win.r1 ? zhi : win.r1) : hi;  // rows read
    auto inside = [&](int px, int pz) {
        if constexpr (WIN) return px >= 0 && px <= hi && pz >= rlo && pz <= rhi;
        else return px >= 0 && px <= hi && pz >= 0 && pz <= hi;
    };
    auto on_border = [&](int px, int pz) {
        if constexpr (WIN) return px == 0 || px == hi || pz == zlo || pz == zhi;
        else return px == 0 || px == hi || pz == 0 || pz == hi;
    };

    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = WIN ? pz < win.r1 : pz <= hi;  // an owned row
    const bool quad = VEC && row_in && px + 3 <= hi;   // VEC: res % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill: a cell outside the grid reads as +0 and decides nothing (a border cell has no receiver by rule) ----
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
    if constexpr (WIN) {
        if (pz == win.r1 && pz <= zhi) {  // the row beside the owned ones, inside the tile: its heights, and nothing else
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (px + j <= hi) hc[j] = h[c0 + j];
        }
    }
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

    // ---- the receiver codes of the own cells, NONE for an outlet and for a pit, and the two coefficients ----
    if (!row_in || px > hi) return;
    const unsigned word = nz_front::receiver_codes4(H, tz, tx, sea, [&](int j) { return on_border(px + j, pz); });
    const float dtu = dt * uplift;
    float b[4], f[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned k = (word >> (8 * j)) & 255u;
        const bool outlet = on_border(px + j, pz) || hc[j] <= sea;
        const float du = uplift_map ? dtu * um[j] : dtu;
        const float kc = hardness ? erodibility * (1.0f - hd[j]) : erodibility;
        b[j] = outlet ? hc[j] : hc[j] + du;
        f[j] = k < NONE ? ((kc * sqrtf(ac[j])) * (k < 4u ? 1.0f : INV_DIAG)) * dt : 0.0f;
    }
    if (quad) {
        *reinterpret_cast<unsigned *>(recv + c0) = word;
        *reinterpret_cast<float4 *>(bco + c0) = make_float4(b[0], b[1], b[2], b[3]);
        *reinterpret_cast<float4 *>(fco + c0) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            recv[c0 + j] = (unsigned char)(word >> (8 * j));
            bco[c0 + j] = b[j];
            fco[c0 + j] = f[j];
        }
    }
}

// ---- a pass ----
// FIRST: the start state h' = b, no h' plane is read; VEC: 16-byte accesses to the float planes and a 32-bit one to the
// receiver bytes (all planes 16-byte aligned, the bytes 4-byte, res % 4 == 0); WIN: res is the pitch
template <bool FIRST, bool VEC, bool WIN, class... Win>
__global__ __launch_bounds__(FT) void fluvial_implicit_pass_kernel(const unsigned char *__restrict__ recv,
                                                                   const float *__restrict__ bco, const float *__restrict__ fco,
                                                                   const float *__restrict__ h_in, float *__restrict__ h_out,
                                                                   int *status, const unsigned char *__restrict__ flags_in,
                                                                   unsigned char *__restrict__ flags_out, int res, int pass,
                                                                   int sweeps, Win... window) {
    static_assert(sizeof...(Win) == (WIN ? 1 : 0));
    const implicit_win win = win_of(window...);
    __shared__ __attribute__((aligned(16))) float HN[(FZ + 2) * LP];  // h' at radius 1: LDS row = plane row - z0 + 1
    const int tid = threadIdx.x;

    if constexpr (WIN) {
        // pass 0 alone asks: round_begin has zeroed the three words, so behind a pass 0 that returned here every later
        // pass finds "the pass before changed nothing" at its gate, without a load of its own
        if (pass == 0 && !status[ST_GO]) return;
    } else {
        if (!status[ST_GO]) return;
    }
    const bool all_live = WIN && pass == 0;  // a round's first pass: nothing is known about the pass before
    const bool t0 = tid == 0;
    const int prev = series_gate<FIRST>(status, t0, pass, all_live);
    if (!prev) return;
    const int tnx = gridDim.x, tnz = gridDim.y;
    const size_t tile0 = (size_t)blockIdx.z * tnx * tnz;
    const size_t me = tile0 + (size_t)blockIdx.y * tnx + blockIdx.x;  // this tile's byte
    if (!FIRST && !all_live) {
        if (!__syncthreads_or(tile_live(flags_in, tile0, tnx, tnz, tid))) {
            if (t0) flags_out[me] = 0;
            return;
        }
    }

    const int x0 = blockIdx.x * FX, z0 = (WIN ? win.r0 : 0) + blockIdx.y * FZ;
    const size_t base = WIN ? 0 : (size_t)blockIdx.z * res * res;
    const int hi = WIN ? win.xhi : res - 1;                            // last column
    const int zlo = WIN ? win.zlo : 0, zhi = WIN ? win.zhi : res - 1;  // the grid's rows
    const int rlo = WIN ? (zlo > win.r0 - 1 ? zlo : win.r0 - 1) : 0, rhi = WIN ? (zhi < win.r1 ? zhi : win.r1) : hi;  // rows read
    auto inside = [&](int px, int pz) {
        if constexpr (WIN) return px >= 0 && px <= hi && pz >= rlo && pz <= rhi;
        else return px >= 0 && px <= hi && pz >= 0 && pz <= hi;
    };
    // WIN: h' of a cell of a frozen row.  The caller's plane is one of the two a round alternates between: pass p reads it
    // when p is even and writes it (its owned rows) when p is odd; a round with `first` takes the heights instead
    auto ghost = [&](size_t q) { return (win.ghost_h ? win.ghost_h : pass & 1 ? h_out : h_in)[q]; };

    // this thread's four cells
    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = WIN ? pz < win.r1 : pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;  // VEC: res % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill ----
    unsigned cod = NONE4;  // the receiver codes of the own cells; a cell outside the grid has none and is not stored
    float bc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, fc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, hc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (quad) {
        cod = *reinterpret_cast<const unsigned *>(recv + c0);
        const float4 b = *reinterpret_cast<const float4 *>(bco + c0);
        const float4 f = *reinterpret_cast<const float4 *>(fco + c0);
        bc[0] = b.x, bc[1] = b.y, bc[2] = b.z, bc[3] = b.w;
        fc[0] = f.x, fc[1] = f.y, fc[2] = f.z, fc[3] = f.w;
        if constexpr (!FIRST) {
            const float4 v = *reinterpret_cast<const float4 *>(h_in + c0);
            hc[0] = v.x, hc[1] = v.y, hc[2] = v.z, hc[3] = v.w;
        }
    } else if (!VEC && row_in) {
        cod = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool in = px + j <= hi;
            cod |= (in ? (unsigned)recv[c0 + j] : NONE) << (8 * j);
            if (in) {
                bc[j] = bco[c0 + j];
                fc[j] = fco[c0 + j];
                if constexpr (!FIRST) hc[j] = h_in[c0 + j];
            }
        }
    }
    if constexpr (FIRST) {
#pragma unroll
        for (int j = 0; j < 4; j++) hc[j] = bc[j];
    }
    if constexpr (WIN) {
        if (pz == win.r1 && pz <= zhi) {  // the frozen row below, inside the tile: no receiver byte (row_in is false), not stored
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (px + j <= hi) hc[j] = ghost(c0 + j);
        }
    }
    *reinterpret_cast<float4 *>(&HN[(tz + 1) * LP + LC + tx]) = make_float4(hc[0], hc[1], hc[2], hc[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        float v = 0.0f;
        if constexpr (WIN) {
            if (inside(qx, qz)) {
                const size_t q = (size_t)qz * res + qx;
                v = qz < win.r0 || qz >= win.r1 ? ghost(q) : (FIRST ? bco : h_in)[q];
            }
        } else {
            if (inside(qx, qz)) v = (FIRST ? bco : h_in)[base + (size_t)qz * res + qx];
        }
        HN[lz * LP + lx] = v;
    }

    // where each own cell looks: the LDS cell its code names (its own without a receiver)
    int at[4];
#pragma unroll
    for (int j = 0; j < 4; j++) at[j] = neighbour_lds(tz, tx, j, (int)((cod >> (8 * j)) & 255u));
    __syncthreads();

    // ---- sweeps inside LDS, the ring frozen ----
    bool moved = FIRST;  // uniform over the workgroup
    for (int s = 0; s < sweeps; s++) {
        int ch = 0;
        if (cod != NONE4) {  // a thread without a receiver holds its final values from the start
            float nq[4];
#pragma unroll
            for (int j = 0; j < 4; j++) nq[j] = HN[at[j]];
            // One update of own cell j: the model's assignment from the cell its code names.  `ch` sees EVERY update, not
            // the net effect of the sweep: a sweep that reports nothing has evaluated each cell on the values now standing
            // and found it at rest, which is what "fixed point against the ring" means.
            auto relax = [&](int j) {
                const unsigned k = (cod >> (8 * j)) & 255u;
                if (k >= NONE) return;
                float q = nq[j];
                if (k == 0u && j > 0) q = hc[j > 0 ? j - 1 : 0];  // W, E among the own four
                if (k == 1u && j < 3) q = hc[j < 3 ? j + 1 : 3];
                const float v = (bc[j] + fc[j] * q) / (1.0f + fc[j]);
                ch |= __float_as_uint(v) != __float_as_uint(hc[j]);
                hc[j] = v;
            };
            relax(0), relax(1), relax(2), relax(3);
            relax(2), relax(1), relax(0);
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
    if (t0) {
        close_tile<FIRST>(status, flags_out, me, pass, moved);
        if constexpr (WIN) {
            if (!FIRST && pass == 0 && moved) *win.changed_out = 1;
        }
    }
}

// all or nothing: the fixed point stands in `out` when the last pass that ran changed nothing (nz_fluvial_implicit keeps it
// as plane 0 of the pair, and a series at rest holds equal planes); otherwise, and when the call was told not to proceed,
// the heights go in unchanged.  One thread keeps the caller's tally; the stream orders the calls, so it needs no atomics.
__global__ __launch_bounds__(256) void fluvial_implicit_finalise_kernel(const float *__restrict__ h, float *__restrict__ out,
                                                                        int *status, int *tally, size_t n) {
    const bool converged = status[ST_GO] != 0 && series_at_rest(status);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        status[ST_CONVERGED] = converged ? 1 : 0;
        if (converged && tally) {
            tally[0] += 1;
            tally[1] += status[ST_PASSES];
        }
    }
    if (i >= n || converged) return;
    out[i] = h[i];
}

// the stripe's all or nothing on the owned rows, by the caller's verdict
__global__ __launch_bounds__(256) void fluvial_implicit_stripe_finalise_kernel(const float *__restrict__ h,
                                                                               float *__restrict__ out, const int *converged,
                                                                               int pitch, int cols, int r0, int r1) {
    const int x = blockIdx.x * 256 + threadIdx.x, z = r0 + blockIdx.y;
    if (x >= cols || z >= r1 || *converged) return;
    const size_t i = (size_t)z * pitch + x;
    out[i] = h[i];
}

}  // namespace

int32_t nz_launch_fluvial_implicit_begin(hipStream_t s, int *status, const int *proceed) {
    NZ_LAUNCH(fluvial_implicit_begin_kernel, dim3(1), dim3(1), 0, s, status, proceed);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_implicit_setup(hipStream_t s, const float *h, const float *area, const float *hardness,
                                         const float *uplift_map, unsigned char *recv, float *bco, float *fco,
                                         const int *status, float erodibility, float uplift, float dt, float sea, int res,
                                         int count) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(area) |
                           reinterpret_cast<uintptr_t>(hardness) | reinterpret_cast<uintptr_t>(uplift_map) |
                           reinterpret_cast<uintptr_t>(bco) | reinterpret_cast<uintptr_t>(fco);
    const bool vec = (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(recv) & 3) == 0 && res % 4 == 0;
    if (vec)
        NZ_LAUNCH((fluvial_implicit_setup_kernel<true, false>), grid, dim3(FT), 0, s, h, area, hardness, uplift_map, recv, bco, fco,
                  status, erodibility, uplift, dt, sea, res);
    else
        NZ_LAUNCH((fluvial_implicit_setup_kernel<false, false>), grid, dim3(FT), 0, s, h, area, hardness, uplift_map, recv, bco, fco,
                  status, erodibility, uplift, dt, sea, res);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

// every row of a stripe-shaped plane starts 16-byte aligned, and 4-byte aligned in the receiver bytes
static bool stripe_vec(const nz_geom &g, uintptr_t float_bits, const unsigned char *recv) {
    return (float_bits & 15) == 0 && (reinterpret_cast<uintptr_t>(recv) & 3) == 0 && g.cols % 4 == 0 && g.pitch % 4 == 0;
}

int32_t nz_launch_fluvial_implicit_stripe_setup(hipStream_t s, const float *h, const float *area, const float *hardness,
                                                const float *uplift_map, unsigned char *recv, float *bco, float *fco,
                                                const int *status, float erodibility, float uplift, float dt, float sea,
                                                const nz_geom &g, int zlo, int zhi) {
    if (g.or1 <= g.or0 || g.cols <= 0) return NZ_OK;
    const dim3 grid(tiles_x(g.cols), tiles_z(g.or1 - g.or0), 1);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(area) |
                           reinterpret_cast<uintptr_t>(hardness) | reinterpret_cast<uintptr_t>(uplift_map) |
                           reinterpret_cast<uintptr_t>(bco) | reinterpret_cast<uintptr_t>(fco);
    const implicit_win win{{g.cols - 1, zlo, zhi, g.or0, g.or1}, h, nullptr};
    if (stripe_vec(g, bits, recv))
        NZ_LAUNCH((fluvial_implicit_setup_kernel<true, true, implicit_win>), grid, dim3(FT), 0, s, h, area, hardness, uplift_map, recv, bco,
                  fco, status, erodibility, uplift, dt, sea, g.pitch, win);
    else
        NZ_LAUNCH((fluvial_implicit_setup_kernel<false, true, implicit_win>), grid, dim3(FT), 0, s, h, area, hardness, uplift_map, recv, bco,
                  fco, status, erodibility, uplift, dt, sea, g.pitch, win);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_implicit_pass(hipStream_t s, const unsigned char *recv, const float *bco, const float *fco,
                                        const float *h_in, float *h_out, int *status, const unsigned char *flags_in,
                                        unsigned char *flags_out, int res, int count, int pass, int sweeps) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(bco) | reinterpret_cast<uintptr_t>(fco) |
                           reinterpret_cast<uintptr_t>(h_in) | reinterpret_cast<uintptr_t>(h_out);
    // a row, and with it a tile of the batch, starts 16-byte aligned in the planes and 4-byte aligned in the receiver bytes
    const bool vec = (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(recv) & 3) == 0 && res % 4 == 0;
    nz_with_bools([&](auto first, auto v) {
        NZ_LAUNCH((fluvial_implicit_pass_kernel<decltype(first)::value, decltype(v)::value, false>), grid, dim3(FT), 0, s, recv, bco,
                  fco, h_in, h_out, status, flags_in, flags_out, res, pass, sweeps);
    }, pass == 0, vec);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_implicit_stripe_pass(hipStream_t s, const unsigned char *recv, const float *bco, const float *fco,
                                               const float *h_in, float *h_out, const float *ghost_h, int *status,
                                               const unsigned char *flags_in, unsigned char *flags_out, int *changed,
                                               const nz_geom &g, int zlo, int zhi, int first, int pass, int sweeps) {
    if (g.or1 <= g.or0 || g.cols <= 0) return NZ_OK;
    const dim3 grid(tiles_x(g.cols), tiles_z(g.or1 - g.or0), 1);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(bco) | reinterpret_cast<uintptr_t>(fco) |
                           reinterpret_cast<uintptr_t>(h_in) | reinterpret_cast<uintptr_t>(h_out);
    const implicit_win win{{g.cols - 1, zlo, zhi, g.or0, g.or1}, first ? ghost_h : nullptr, changed};
    nz_with_bools([&](auto start, auto v) {
        NZ_LAUNCH((fluvial_implicit_pass_kernel<decltype(start)::value, decltype(v)::value, true, implicit_win>), grid, dim3(FT), 0, s,
                  recv, bco, fco, h_in, h_out, status, flags_in, flags_out, g.pitch, pass, sweeps, win);
    }, first && pass == 0, stripe_vec(g, bits, recv));
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_implicit_stripe_finalise(hipStream_t s, const float *h, float *out, const int *converged,
                                                   const nz_geom &g) {
    if (g.or1 <= g.or0 || g.cols <= 0) return NZ_OK;
    const dim3 grid((g.cols + 255) / 256, g.or1 - g.or0);
    NZ_LAUNCH(fluvial_implicit_stripe_finalise_kernel, grid, dim3(256), 0, s, h, out, converged, g.pitch, g.cols, g.or0,
              g.or1);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_implicit_finalise(hipStream_t s, const float *h, float *out, int *status, int *tally, size_t n) {
    if (n == 0) return NZ_OK;
    const dim3 grid((unsigned)((n + 255) / 256));
    NZ_LAUNCH(fluvial_implicit_finalise_kernel, grid, dim3(256), 0, s, h, out, status, tally, n);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
