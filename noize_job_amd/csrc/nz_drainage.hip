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
// The mask launch, once per call, on the geometry of nz_tile64.hpp (16-byte accesses where planes and pitch allow):
// heights at radius 2 into LDS, receiver codes at radius 1, and per own cell one DONOR BYTE -- bit k set when neighbour k
// exists and its receiver is the direction opposite to k.  After it no launch looks at a height.
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
#include "nz_internal.hpp"
#include "nz_receiver.hpp"
#include "nz_relax_pass.hpp"
#include "nz_tile64.hpp"

namespace {

using nz_recv::NONE;
using nz_recv::receiver;
using namespace nz_tile64;  // the tile, its LDS layout, ring_cell, halo2_cell
using namespace nz_relax;   // the status words and the pass protocol

// ---- the mask launch: heights -> donor bytes ----
// VEC: 16-byte height reads; WORD: the four donor bytes of a thread as one 32-bit store (res % 4 == 0)
template <bool VEC, bool WORD>
__global__ __launch_bounds__(FT) void drainage_mask_kernel(const float *__restrict__ h, unsigned char *__restrict__ donors,
                                                           float sea, int res) {
    __shared__ __attribute__((aligned(16))) float H[(FZ + 4) * LP];          // radius 2: LDS row = plane row - z0 + 2
    __shared__ __attribute__((aligned(16))) unsigned RW[(FZ + 2) * LP / 4];  // radius 1, one byte per cell
    unsigned char *RC = reinterpret_cast<unsigned char *>(RW);

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FX, z0 = blockIdx.y * FZ;
    const size_t base = (size_t)blockIdx.z * res * res;
    const int hi = res - 1;
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= 0 && pz <= hi; };
    auto on_border = [&](int px, int pz) { return px == 0 || px == hi || pz == 0 || pz == hi; };

    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = pz <= hi;
    const bool quad = row_in && px + 3 <= hi;

    // ---- fill: a cell outside the grid reads as +0 and is never looked at ----
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

    // ---- receivers at radius 1: NONE for an outlet and for a cell outside the grid ----
    {
        float w[3][6];  // rows pz-1 .. pz+1, columns px-1 .. px+4
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float *row = &H[(tz + 1 + r) * LP + LC + tx];
            const float4 v = *reinterpret_cast<const float4 *>(row);
            w[r][0] = row[-1], w[r][1] = v.x, w[r][2] = v.y, w[r][3] = v.z, w[r][4] = v.w, w[r][5] = row[4];
        }
        unsigned codes = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float s, d;
            unsigned r = receiver(w[1][j + 1], w[1][j], w[1][j + 2], w[0][j + 1], w[2][j + 1], w[0][j], w[0][j + 2], w[2][j],
                                  w[2][j + 2], s, d);
            if (!inside(px + j, pz) || on_border(px + j, pz) || w[1][j + 1] <= sea) r = NONE;
            codes |= r << (8 * j);
        }
        RW[((tz + 1) * LP + LC + tx) >> 2] = codes;
    }
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        unsigned r = NONE;
        if (inside(qx, qz) && !on_border(qx, qz)) {
            const float *row = &H[(lz + 1) * LP + lx];
            float s, d;
            if (!(row[0] <= sea))
                r = receiver(row[0], row[-1], row[1], row[-LP], row[LP], row[-LP - 1], row[-LP + 1], row[LP - 1], row[LP + 1], s,
                             d);
        }
        RC[lz * LP + lx] = (unsigned char)r;
    }
    __syncthreads();

    // ---- the donor bytes of the own cells ----
    if (!row_in || px > hi) return;
    unsigned cw[3][6];  // the receiver codes of the window
    window_bytes(RW, tz, tx, cw);
    unsigned word = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) word |= nz_recv::donor_mask(cw, j) << (8 * j);
    if (WORD && quad) {
        *reinterpret_cast<unsigned *>(donors + c0) = word;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            donors[c0 + j] = (unsigned char)(word >> (8 * j));
        }
    }
}

// ---- a pass ----
// FIRST: the start state rain_c, no A plane is read; VEC: 16-byte accesses to the float planes and a 32-bit one to the
// donor bytes (all planes 16-byte aligned, res % 4 == 0); MAP: rain_c = rain * rain_map[c]
template <bool FIRST, bool VEC, bool MAP>
__global__ __launch_bounds__(FT) void drainage_pass_kernel(const unsigned char *__restrict__ donors,
                                                           const float *__restrict__ rain_map,
                                                           const float *__restrict__ a_in, float *__restrict__ a_out,
                                                           int *status, const unsigned char *__restrict__ flags_in,
                                                           unsigned char *__restrict__ flags_out, float rain, int res,
                                                           int pass, int sweeps) {
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
    *reinterpret_cast<float4 *>(&A[(tz + 1) * LP + LC + tx]) = make_float4(ac[0], ac[1], ac[2], ac[3]);
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        float v = 0.0f;
        if (inside(qx, qz)) {
            const size_t q = base + (size_t)qz * res + qx;
            if constexpr (FIRST) v = rain_at(q);
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
    if (t0) close_tile<FIRST>(status, flags_out, me, pass, moved);
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

}  // namespace

int32_t nz_launch_drainage_mask(hipStream_t s, const float *h, unsigned char *donors, float sea, int res, int count) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const bool word = res % 4 == 0 && (reinterpret_cast<uintptr_t>(donors) & 3) == 0;
    const bool vec = res % 4 == 0 && (reinterpret_cast<uintptr_t>(h) & 15) == 0;
    if (vec && word) NZ_LAUNCH((drainage_mask_kernel<true, true>), grid, dim3(FT), 0, s, h, donors, sea, res);
    else if (word) NZ_LAUNCH((drainage_mask_kernel<false, true>), grid, dim3(FT), 0, s, h, donors, sea, res);
    else NZ_LAUNCH((drainage_mask_kernel<false, false>), grid, dim3(FT), 0, s, h, donors, sea, res);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

namespace {
template <bool FIRST, bool VEC>
void launch_pass(bool map, dim3 grid, hipStream_t s, const unsigned char *donors, const float *rain_map, const float *a_in,
                 float *a_out, int *status, const unsigned char *flags_in, unsigned char *flags_out, float rain, int res,
                 int pass, int sweeps) {
    if (map) NZ_LAUNCH((drainage_pass_kernel<FIRST, VEC, true>), grid, dim3(FT), 0, s, donors, rain_map, a_in, a_out, status, flags_in, flags_out, rain, res, pass, sweeps);
    else NZ_LAUNCH((drainage_pass_kernel<FIRST, VEC, false>), grid, dim3(FT), 0, s, donors, rain_map, a_in, a_out, status, flags_in, flags_out, rain, res, pass, sweeps);
}
}  // namespace

int32_t nz_launch_drainage_pass(hipStream_t s, const unsigned char *donors, const float *rain_map, const float *a_in,
                                float *a_out, int *status, const unsigned char *flags_in, unsigned char *flags_out, float rain,
                                int res, int count, int pass, int sweeps) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const uintptr_t bits = reinterpret_cast<uintptr_t>(rain_map) | reinterpret_cast<uintptr_t>(a_in) |
                           reinterpret_cast<uintptr_t>(a_out) | reinterpret_cast<uintptr_t>(donors);
    const bool vec = (bits & 15) == 0 && res % 4 == 0;  // a row, and with it a tile of the batch, starts 16-byte aligned
    const bool map = rain_map != nullptr;
    if (pass == 0) {
        if (vec) launch_pass<true, true>(map, grid, s, donors, rain_map, a_in, a_out, status, flags_in, flags_out, rain, res, pass, sweeps);
        else launch_pass<true, false>(map, grid, s, donors, rain_map, a_in, a_out, status, flags_in, flags_out, rain, res, pass, sweeps);
    } else {
        if (vec) launch_pass<false, true>(map, grid, s, donors, rain_map, a_in, a_out, status, flags_in, flags_out, rain, res, pass, sweeps);
        else launch_pass<false, false>(map, grid, s, donors, rain_map, a_in, a_out, status, flags_in, flags_out, rain, res, pass, sweeps);
    }
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
