// nz_drainage.hip -- drainage area: the exact flow accumulation of a heightmap (gfx950; new-framework feature).
//
// THE MODEL (include/noize_hip.h states it for the caller, tests/drainage_ref.py restates it as a topological walk):
//   Square tile res x res, row-major z * res + x, float32 throughout, no contraction, the same in every float mode.
//   Outlets, neighbours k = 0..7 in the order W E S N SW SE NW NE and the receiver r(c) are step 1 of the fluvial model
//   (nz_receiver.hpp); rain_c = rain * rainMap[c], or rain.  The result is the plane A with, for every cell,
//   A[c] = rain_c; for k ascending over the existing neighbours whose receiver is c: A[c] = A[c] + A[k]
//   -- step 2 of the fluvial model at rest.
// A receiver is strictly lower than its donor, so the receiver graph is a forest: a cell's final value is a fixed function
// of its donors' final values, the fixed point is unique and every order of updates -- Jacobi, tile-local sweeps, a
// topological walk -- ends in the same floats.  No monotonicity is needed (a rain map may be negative), only that a test
// "nothing changed" looks at every single update: see `relax` below.
//
// The mask launch, once per call, on the geometry of nz_tile64.hpp (16-byte accesses where planes and pitch allow), is
// nz_donor_front.hpp's: heights at radius 2 into LDS, receiver codes at radius 1, and per own cell one DONOR BYTE -- bit k
// set when neighbour k exists and its receiver is the direction opposite to k.  After it no launch looks at a height.
//
// One launch per PASS of A, by the pass protocol of nz_relax_pass.hpp -- gate, tile skip, sweeps against a frozen ring,
// the closing byte and word, and the argument for them; the caller's `drainage` is plane 0.  What is this stage's own:
//   fill     the four donor bytes and rain_c of the thread's cells into registers, A at radius 1 into LDS (18 x 72
//            floats); a ring cell outside the grid holds +0 and is never gathered (its donor bit is clear).  The first
//            pass reads no A plane: it derives the start state rain_c.
//   sweeps   every thread updates its four cells left to right and back (Gauss-Seidel inside the thread, Jacobi between
//            threads); "changed" looks at every single update (`relax`).
// A series at rest holds the fixed point in BOTH planes, so the finalise launch has nothing to copy: it sets the protocol's
// verdict and, when the last pass that ran did change something, puts rain_c back into every cell: all or nothing.
//
// WIN, the stripe form (nz_drainage_stripe_round), on the pattern of nz_fill.hip's: one ROUND on the owned rows [r0, r1) of a
// stripe-shaped buffer with a pitch; the workgroups tile the owned rows, the grid's bounds are the global grid's seen from
// the buffer.  The mask launch of a round with `first` reads heights two rows beyond the owned ones (the receiver of a cell
// of a ghost row looks one row further out) and stores donor bytes for the owned rows only.  The one row of A on each side
// of the owned rows is FROZEN: read from the caller's plane in every pass (in a round with `first`: rain_c), never written,
// whichever of the two planes the pass alternates between.  When the owned rows end inside a tile, the frozen row lies in
// a thread's own slot: it is loaded, has no donor byte and is not stored.  status[GO], pass 0 of a round that continues
// from A (all tiles live) and the caller's `changed` word are the fill stripe's (nz_relax_pass.hpp), except that only the
// mask launch and pass 0 read status[GO]: the later passes of a round that does not go return at their gate; `changed` follows
// `relax`: a pass 0 in which any single update changed a value stores 1, and a pass 0 that stores nothing has found every
// owned cell at rest against the frozen rows.
#include "nz_internal.hpp"
#include "nz_receiver.hpp"
#include "nz_relax_pass.hpp"
#include "nz_tile64.hpp"
#include "nz_donor_front.hpp"

namespace {

// WIN: the owned rows of one stripe-shaped buffer (nz_front::win_rows) and what the passes of a round need beside them
struct drain_win : nz_front::win_rows {
    int ghost_from_rain;    // the frozen rows are the start state rain_c (a round with `first`), else the caller's plane's
    int *status;            // the round's status words (the mask launch reads status[GO])
    int *changed_out;       // the caller's word
};

using namespace nz_tile64;  // the tile, its LDS layout, ring_cell
using namespace nz_relax;   // the status words and the pass protocol

// ---- the mask launch: heights -> donor bytes (nz_donor_front.hpp, no channel predicate) ----
template <bool VEC, bool WORD, bool WIN>
__global__ __launch_bounds__(FT) void drainage_mask_kernel(const float *__restrict__ h, unsigned char *__restrict__ donors,
                                                           float sea, int res, drain_win win) {
    if (WIN && !win.status[ST_GO]) return;
    nz_front::donor_front<VEC, WORD, WIN, false>(h, nullptr, donors, nullptr, sea, 0.0f, res, win);
}

// ---- a pass ----
// FIRST: the start state rain_c, no A plane is read; VEC: 16-byte accesses to the float planes and a 32-bit one to the
// donor bytes (all planes 16-byte aligned, res % 4 == 0); MAP: rain_c = rain * rain_map[c]; WIN: res is the pitch
// The cap of 102 SGPRs is what eight waves per SIMD allow.  The tile forms take 96 to 99 and compile as without it; the
// stripe forms that read A would take 103 to 106 and seven waves, and keep one value in a VGPR lane instead (measured:
// DESIGN.md section 4, "drainage area on row stripes")
template <bool FIRST, bool VEC, bool MAP, bool WIN>
__global__ __launch_bounds__(FT) __attribute__((amdgpu_num_sgpr(102)))
void drainage_pass_kernel(const unsigned char *__restrict__ donors, const float *__restrict__ rain_map,
                          const float *__restrict__ a_in, float *__restrict__ a_out, int *status,
                          const unsigned char *__restrict__ flags_in, unsigned char *__restrict__ flags_out, float rain, int res,
                          int pass, int sweeps, drain_win win) {
    __shared__ __attribute__((aligned(16))) float A[(FZ + 2) * LP];  // radius 1: LDS row = plane row - z0 + 1
    const int tid = threadIdx.x;

    if constexpr (WIN) {
        // pass 0 alone asks: round_begin has zeroed the three words, so behind a pass 0 that returned here every later
        // pass finds "the pass before changed nothing" at its gate, without a load of its own
        if (pass == 0 && !status[ST_GO]) return;
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
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= rlo && pz <= rhi; };
    auto rain_at = [&](size_t q) { return MAP ? rain * rain_map[q] : rain; };
    // WIN: A of a cell of a frozen row.  The caller's plane is one of the two a round alternates between: pass p reads it
    // when p is even and writes it (its owned rows) when p is odd
    const float *a_ghost = pass & 1 ? a_out : a_in;
    auto ghost = [&](size_t q) { return win.ghost_from_rain ? rain_at(q) : a_ghost[q]; };

    // this thread's four cells
    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = WIN ? pz < win.r1 : pz <= hi;
    const bool quad = VEC && row_in && px + 3 <= hi;  // VEC: res % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill ----
    float rc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ac[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned don = 0;  // the donor bytes of the own cells; a cell outside the grid has none and stays +0
    if (quad) {
        don = *reinterpret_cast<const unsigned *>(donors + c0);
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
            don |= (unsigned)donors[c0 + j] << (8 * j);
            rc[j] = rain_at(c0 + j);
            if constexpr (!FIRST) ac[j] = a_in[c0 + j];
        }
    }
    if constexpr (FIRST) {
#pragma unroll
        for (int j = 0; j < 4; j++) ac[j] = rc[j];
    }
    if constexpr (WIN) {
        if (pz == win.r1 && pz <= zhi) {  // the frozen row below, inside the tile: no donor byte (row_in is false), not stored
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (px + j <= hi) ac[j] = ghost(c0 + j);
        }
    }
    *reinterpret_cast<float4 *>(&A[(tz + 1) * LP + LC + tx]) = make_float4(ac[0], ac[1], ac[2], ac[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        float v = 0.0f;
        if (inside(qx, qz)) {
            const size_t q = base + (size_t)qz * res + qx;
            if (WIN && (qz < win.r0 || qz >= win.r1)) v = ghost(q);
            else if constexpr (FIRST) v = rain_at(q);
            else v = a_in[q];
        }
        A[lz * LP + lx] = v;
    }
    __syncthreads();

    // ---- sweeps inside LDS, the ring frozen ----
    bool moved = FIRST;  // uniform over the workgroup
    for (int s = 0; s < sweeps; s++) {
        int ch = 0;
        if (don) {  // a thread without a donor holds rain_c for good
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
            // the sweep: a sweep that reports nothing has evaluated each cell on the values now standing and found it
            // at rest, which is what "fixed point against the ring" means when values may move both ways.
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
        *reinterpret_cast<float4 *>(a_out + c0) = make_float4(ac[0], ac[1], ac[2], ac[3]);
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            a_out[c0 + j] = ac[j];
        }
    }
    if (t0) {
        close_tile<FIRST>(status, flags_out, me, pass, moved);
        if constexpr (WIN) {
            if (!FIRST && pass == 0 && moved) *win.changed_out = 1;
        }
    }
}

// all or nothing: the fixed point stands in `drainage` when the last pass that ran changed nothing (nz_drainage_area keeps
// `drainage` as one of the two planes, and a series at rest holds equal planes); otherwise the start state goes back in
template <bool MAP>
__global__ __launch_bounds__(256) void drainage_finalise_kernel(float *__restrict__ drainage,
                                                                const float *__restrict__ rain_map, int *status, float rain,
                                                                size_t n) {
    const bool converged = series_at_rest(status);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[ST_CONVERGED] = converged ? 1 : 0;
    if (i >= n || converged) return;
    drainage[i] = MAP ? rain * rain_map[i] : rain;
}

// the stripe's all or nothing on the owned rows, by the caller's verdict
template <bool MAP>
__global__ __launch_bounds__(256) void drainage_stripe_finalise_kernel(float *__restrict__ a, const float *__restrict__ rain_map,
                                                                       const int *converged, float rain, int pitch, int cols,
                                                                       int r0, int r1) {
    const int x = blockIdx.x * 256 + threadIdx.x, z = r0 + blockIdx.y;
    if (x >= cols || z >= r1 || *converged) return;
    const size_t i = (size_t)z * pitch + x;
    a[i] = MAP ? rain * rain_map[i] : rain;
}

const drain_win NO_WIN{};  // the tile forms

}  // namespace

int32_t nz_launch_drainage_mask(hipStream_t s, const float *h, unsigned char *donors, float sea, int res, int count) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const bool word = res % 4 == 0 && (reinterpret_cast<uintptr_t>(donors) & 3) == 0;
    const bool vec = res % 4 == 0 && (reinterpret_cast<uintptr_t>(h) & 15) == 0;
    if (vec && word) NZ_LAUNCH((drainage_mask_kernel<true, true, false>), grid, dim3(FT), 0, s, h, donors, sea, res, NO_WIN);
    else if (word) NZ_LAUNCH((drainage_mask_kernel<false, true, false>), grid, dim3(FT), 0, s, h, donors, sea, res, NO_WIN);
    else NZ_LAUNCH((drainage_mask_kernel<false, false, false>), grid, dim3(FT), 0, s, h, donors, sea, res, NO_WIN);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_drainage_stripe_mask(hipStream_t s, const float *h, unsigned char *donors, int *status, float sea,
                                       const nz_geom &g, int zlo, int zhi) {
    if (g.or1 <= g.or0 || g.cols <= 0) return NZ_OK;
    const dim3 grid(tiles_x(g.cols), tiles_z(g.or1 - g.or0), 1);
    const bool word = g.cols % 4 == 0 && g.pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(donors) & 3) == 0;
    const bool vec = word && (reinterpret_cast<uintptr_t>(h) & 15) == 0;  // every row starts 16-byte aligned
    const drain_win win{{g.cols - 1, zlo, zhi, g.or0, g.or1}, 0, status, nullptr};
    if (vec) NZ_LAUNCH((drainage_mask_kernel<true, true, true>), grid, dim3(FT), 0, s, h, donors, sea, g.pitch, win);
    else if (word) NZ_LAUNCH((drainage_mask_kernel<false, true, true>), grid, dim3(FT), 0, s, h, donors, sea, g.pitch, win);
    else NZ_LAUNCH((drainage_mask_kernel<false, false, true>), grid, dim3(FT), 0, s, h, donors, sea, g.pitch, win);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_drainage_pass(hipStream_t s, const unsigned char *donors, const float *rain_map, const float *a_in,
                                float *a_out, int *status, const unsigned char *flags_in, unsigned char *flags_out, float rain,
                                int res, int count, int pass, int sweeps) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(rain_map) | reinterpret_cast<uintptr_t>(a_in) |
                           reinterpret_cast<uintptr_t>(a_out) | reinterpret_cast<uintptr_t>(donors);
    const bool vec = (bits & 15) == 0 && res % 4 == 0;  // a row, and with it a tile of the batch, starts 16-byte aligned
    nz_with_bools([&](auto first, auto v, auto map) {
        NZ_LAUNCH((drainage_pass_kernel<decltype(first)::value, decltype(v)::value, decltype(map)::value, false>), grid,
                  dim3(FT), 0, s, donors, rain_map, a_in, a_out, status, flags_in, flags_out, rain, res, pass, sweeps, NO_WIN);
    }, pass == 0, vec, rain_map != nullptr);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_drainage_stripe_pass(hipStream_t s, const unsigned char *donors, const float *rain_map, const float *a_in,
                                       float *a_out, int *status, const unsigned char *flags_in,
                                       unsigned char *flags_out, int *changed, float rain, const nz_geom &g, int zlo, int zhi,
                                       int first, int pass, int sweeps) {
    if (g.or1 <= g.or0 || g.cols <= 0) return NZ_OK;
    const dim3 grid(tiles_x(g.cols), tiles_z(g.or1 - g.or0), 1);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(rain_map) | reinterpret_cast<uintptr_t>(a_in) |
                           reinterpret_cast<uintptr_t>(a_out) | reinterpret_cast<uintptr_t>(donors);
    const bool vec = (bits & 15) == 0 && g.cols % 4 == 0 && g.pitch % 4 == 0;  // every row starts 16-byte aligned
    const drain_win win{{g.cols - 1, zlo, zhi, g.or0, g.or1}, first, status, changed};
    nz_with_bools([&](auto start, auto v, auto map) {
        NZ_LAUNCH((drainage_pass_kernel<decltype(start)::value, decltype(v)::value, decltype(map)::value, true>), grid,
                  dim3(FT), 0, s, donors, rain_map, a_in, a_out, status, flags_in, flags_out, rain, g.pitch, pass, sweeps, win);
    }, first && pass == 0, vec, rain_map != nullptr);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_drainage_stripe_finalise(hipStream_t s, float *a, const float *rain_map, const int *converged, float rain,
                                           const nz_geom &g) {
    if (g.or1 <= g.or0 || g.cols <= 0) return NZ_OK;
    const dim3 grid((g.cols + 255) / 256, g.or1 - g.or0);
    if (rain_map) NZ_LAUNCH(drainage_stripe_finalise_kernel<true>, grid, dim3(256), 0, s, a, rain_map, converged, rain, g.pitch, g.cols, g.or0, g.or1);
    else NZ_LAUNCH(drainage_stripe_finalise_kernel<false>, grid, dim3(256), 0, s, a, rain_map, converged, rain, g.pitch, g.cols, g.or0, g.or1);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_drainage_finalise(hipStream_t s, float *drainage, const float *rain_map, int *status, float rain, size_t n) {
    if (n == 0) return NZ_OK;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (rain_map) NZ_LAUNCH(drainage_finalise_kernel<true>, grid, dim3(256), 0, s, drainage, rain_map, status, rain, n);
    else NZ_LAUNCH(drainage_finalise_kernel<false>, grid, dim3(256), 0, s, drainage, rain_map, status, rain, n);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
