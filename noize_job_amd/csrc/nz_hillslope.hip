// nz_hillslope.hip -- linear hillslope diffusion, dh/dt = kappa * laplace(h), as one implicit step of any size: a pair of
// tridiagonal line solves over the whole plane (gfx950; new-framework feature).
//
// THE MODEL (include/noize_hip.h states it for the caller, tests/hillslope_ref.py restates it in numpy):
//   Square tile res x res, row-major c = z * res + x, float32 throughout, every operation rounded once, no contraction,
//   the same in every float mode.  Backward Euler split by direction, (I - r Lx)(I - r Lz) h' = h, with the border cells
//   held (Dirichlet): they keep their bits.  The amplification 1 / ((1 + r lx)(1 + r lz)) is positive for every r, so
//   nothing oscillates at a large dt (Peaceman-Rachford tends to -1 there).
//   Coefficients, shared by every line:  r = diffusivity * dt (one product),  B = 1 + 2 * r.
//   Tables for i = 1 .. res-2:  den_1 = B,  den_i = B - r * cp_{i-1},  inv_i = 1 / den_i (correctly rounded),
//                               cp_i = r * inv_i.
//   One line solve over v_0 .. v_{n-1}:
//     p_0 = v_0;      p_i = (v_i + r * p_{i-1}) * inv_i   for i = 1 .. n-2;
//     x_{n-1} = v_{n-1};  x_i = p_i + cp_i * x_{i+1}      for i = n-2 .. 1;   x_0 = v_0.
//   One step: half-step X solves every row z = 1 .. res-2 along x (rows 0 and res-1 are copied), half-step Z solves every
//   column x = 1 .. res-2 of that result along z.  `iterations` steps follow one another on the same tables.
//   res < 3 and r == 0 give out = h bit for bit by definition (the entry copies; no kernel of this file runs).
//
// THE LAUNCHES.  The hot chain has no division: the tables come from one launch per call.
//   tables    one wave.  Lane 0 walks the recurrence; den_{i+1} is a function of cp_i alone, so once cp_i has the bits of
//             cp_{i-1} every later entry has the bits of entry i, and the 64 lanes fill the rest together (after 64
//             entries at r = 100, about 1 900 at r = 1e6).
//   rows      (lines along x, the contiguous axis) a wave owns 64 rows and marches over 64-column blocks.  A block is
//             loaded coalesced, lanes along x, and goes through LDS with the row pitch padded by one word: ds_write_b32
//             and ds_read_b32 bank on (address / 4) % 32 within a 32-lane half, and both the block-shaped accesses
//             (bank = row + lane + const) and the row-shaped ones (bank = lane + k + const) hit 32 banks with 32 lanes.  A
//             lane then walks its own row's 64 values in registers, the carry of the recurrence stays in a register from
//             block to block, and the block goes back the way it came.  The next block is loaded before the chain of this
//             one starts.  The forward sweep (left to right, writes p into `out`) and the backward sweep (right to left,
//             overwrites p with x) are TWO launches: the lane that stores a cell is not the lane that reloads it.
//   columns   (lines along z) a lane owns one column, a wave 64 consecutive columns, so every step is one coalesced row
//             segment.  Rows are loaded a batch (64) ahead of the chain together with the batch's table entries.  Forward
//             and backward share one launch: a lane reloads only what it stored itself.  Four columns per lane on the
//             16-byte path (four independent chains, a quarter of the waves) were measured at 4096^2 and lost.
// p lives in `out`, so a step moves 8 planes and `work` holds only the two tables.
#include "nz_internal.hpp"

namespace {

constexpr int LN = 64;      // lanes of a wave = rows of a row-solve wave = columns of a block
constexpr int TP = LN + 1;  // LDS row pitch of a block, in words
constexpr int COLUMN_ROWS_AHEAD = 64;  // a batch of the column solve: 16, 32 and 64 measured, DESIGN.md section 4

__device__ __forceinline__ float lane_value(float v, int lane) {  // a table entry held by `lane`, to every lane
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// ---- the tables ----
__global__ __launch_bounds__(LN) void hillslope_tables_kernel(float *__restrict__ inv, float *__restrict__ cp, float r,
                                                              int res) {
    __shared__ int stop;
    __shared__ float rest[2];
    const int lane = threadIdx.x, last = res - 2;
    if (lane == 0) {
        const float B = 1.0f + 2.0f * r;
        float c = 0.0f, iv = 0.0f;
        int i = 1;
        for (; i <= last; i++) {
            const float den = i == 1 ? B : B - r * c;
            iv = 1.0f / den;
            const float cn = r * iv;
            inv[i] = iv;
            cp[i] = cn;
            const bool fixed = i > 1 && __float_as_int(cn) == __float_as_int(c);
            c = cn;
            if (fixed) break;
        }
        stop = i;  // the last entry written (or last + 1: the walk reached the end)
        rest[0] = iv;
        rest[1] = c;
        inv[0] = cp[0] = inv[res - 1] = cp[res - 1] = 0.0f;  // never read by a chain
    }
    __syncthreads();
    const float iv = rest[0], c = rest[1];
    for (int i = stop + 1 + lane; i <= last; i += LN) {
        inv[i] = iv;
        cp[i] = c;
    }
}

// ---- a wave's 64 x 64 block: global <-> registers <-> LDS ----
// 4-byte form: register j of lane l is cell (row j, column l).  16-byte form: registers 4j .. 4j+3 of lane l are the four
// cells of row 4j + (l & 3) from column 4 (l >> 2) on -- 32 consecutive lanes then touch 32 banks in LDS.
template <bool VEC>
__device__ __forceinline__ void block_load(const float *src, int res, int z0, int x0, int lane, float (&v)[LN]) {
    // a cell beyond the tile reads the tile's last row or column instead: loads without a condition, and nothing of it is
    // ever stored (block_store asks)
    if constexpr (VEC) {
        const int x = min(x0 + 4 * (lane >> 2), res - 4);
#pragma unroll
        for (int j = 0; j < LN / 4; j++) {
            const int z = min(z0 + 4 * j + (lane & 3), res - 1);
            const float4 q = *reinterpret_cast<const float4 *>(src + (size_t)z * res + x);
            v[4 * j] = q.x, v[4 * j + 1] = q.y, v[4 * j + 2] = q.z, v[4 * j + 3] = q.w;
        }
    } else {
        const int x = min(x0 + lane, res - 1);
#pragma unroll
        for (int j = 0; j < LN; j++) v[j] = src[(size_t)min(z0 + j, res - 1) * res + x];
    }
}

template <bool VEC>
__device__ __forceinline__ void block_store(float *dst, int res, int z0, int x0, int lane, const float (&v)[LN]) {
    if constexpr (VEC) {
        const int x = x0 + 4 * (lane >> 2);
#pragma unroll
        for (int j = 0; j < LN / 4; j++) {
            const int z = z0 + 4 * j + (lane & 3);
            if (z < res && x < res)
                *reinterpret_cast<float4 *>(dst + (size_t)z * res + x) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
        }
    } else {
        const int x = x0 + lane;
#pragma unroll
        for (int j = 0; j < LN; j++) {
            const int z = z0 + j;
            if (z < res && x < res) dst[(size_t)z * res + x] = v[j];
        }
    }
}

template <bool VEC>
__device__ __forceinline__ int block_word(int lane, int j) {  // the LDS word of register j
    if constexpr (VEC) return (4 * (j >> 2) + (lane & 3)) * TP + 4 * (lane >> 2) + (j & 3);
    else return j * TP + lane;
}

// One sweep of the row solve over the tile blockIdx.y: rows z0 .. z0 + 63, BACK false: p_i left to right, true: x_i right
// to left.  src == dst is the in-place form; the forward sweep of an out-of-place step reads the heights and writes every
// cell of `dst`, the copied rows and columns included.  tab: inv for the forward sweep, cp for the backward one.
template <bool VEC, bool BACK>
__global__ __launch_bounds__(LN) void hillslope_row_kernel(const float *src, float *dst, const float *__restrict__ tab,
                                                           float r, int res) {
    __shared__ float T[LN * TP];
    const int lane = threadIdx.x;
    const int z0 = blockIdx.x * LN, z = z0 + lane;
    const size_t base = (size_t)blockIdx.y * res * res;
    src += base;
    dst += base;
    const bool solve = z >= 1 && z <= res - 2;  // rows 0 and res-1, and rows beyond the tile, pass through
    const int nb = (res + LN - 1) / LN, hi = res - 1;

    float v[LN], nx[LN];
    float carry = 0.0f, tv, tnx = 0.0f;
    int b = BACK ? nb - 1 : 0;
    block_load<VEC>(src, res, z0, b * LN, lane, v);
    tv = tab[min(b * LN + lane, hi)];
    // the first block is waited for here, once, so that the loop is never entered with loads in flight: see column_sweep
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0); expcnt and lgkmcnt left alone
    for (int done = 0; done < nb; done++) {
        const int x0 = b * LN, bn = BACK ? b - 1 : b + 1;
        if (done + 1 < nb) {  // the next block and its table entries, in flight behind this block's chain
            block_load<VEC>(src, res, z0, bn * LN, lane, nx);
            tnx = tab[min(bn * LN + lane, hi)];
        }
#pragma unroll
        for (int j = 0; j < LN; j++) T[block_word<VEC>(lane, j)] = v[j];
        __syncthreads();
        // the lane's own row: positions x0 + k for k = klo .. khi are unknowns of the line, the line's two ends are held
        const int klo = b == 0 ? 1 : 0, khi = min(LN - 1, hi - 1 - x0);
        if (done == 0) carry = T[lane * TP + (BACK ? hi - x0 : 0)];  // v_{n-1}, or v_0
#pragma unroll
        for (int k = 0; k < LN; k++) v[k] = T[lane * TP + k];
        auto chain = [&](auto whole) {  // whole: every position of the block is an unknown, nothing to ask per position
#pragma unroll
            for (int kk = 0; kk < LN; kk++) {
                const int k = BACK ? LN - 1 - kk : kk;
                if (decltype(whole)::value || (k >= klo && k <= khi)) {
                    const float t = lane_value(tv, k);
                    if (BACK) carry = v[k] + t * carry;   // x_i = p_i + cp_i * x_{i+1}
                    else carry = (v[k] + r * carry) * t;  // p_i = (v_i + r * p_{i-1}) * inv_i
                    v[k] = carry;
                }
            }
        };
        if (klo == 0 && khi == LN - 1) chain(std::true_type());
        else chain(std::false_type());
        if (solve) {
#pragma unroll
            for (int k = 0; k < LN; k++) T[lane * TP + k] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LN; j++) v[j] = T[block_word<VEC>(lane, j)];
        block_store<VEC>(dst, res, z0, x0, lane, v);
        __syncthreads();  // T is free for the next block
#pragma unroll
        for (int j = 0; j < LN; j++) v[j] = nx[j];
        tv = tnx;
        b = bn;
    }
}

// The column solve of the tile blockIdx.y, in place: a lane owns the column x, the forward sweep runs down the rows, the
// backward sweep up again.  The columns 0 and res-1 are held and the columns beyond the tile do not exist: their lanes
// load like the others (from a column of the tile: loads without a condition keep a batch straight-line code), run the
// chain on what they loaded and store nothing; no lane leaves early -- every lane holds table entries the others read.
// The rows go in batches of CU with the next batch and its table entries in flight behind the chain of this one; a whole
// batch is straight-line code, the last, shorter one asks per row.
template <bool BACK, int CU>
__device__ __forceinline__ void column_sweep(float *col, const float *__restrict__ tab, float r, int res, int lane, bool act,
                                             float carry) {
    const int first = 1, last = res - 2;
    const ptrdiff_t pitch = BACK ? -(ptrdiff_t)res : (ptrdiff_t)res;  // the sweep's next row
    const int dir = BACK ? -1 : 1;
    float *row = col + (size_t)(BACK ? last : first) * res;  // the row the sweep stands at
    int z = BACK ? last : first, left = last - first + 1;
    float cur[CU], nxt[CU], tv = 0.0f, tnx = 0.0f;
    auto fetch = [&](float *from, int zf, int rows, float (&into)[CU], float &t) {  // a short batch repeats its last row
#pragma unroll
        for (int u = 0; u < CU; u++) into[u] = from[min(u, rows - 1) * pitch];
        t = tab[zf + dir * min(lane & (CU - 1), rows - 1)];
    };
    fetch(row, z, min(left, CU), cur, tv);
    // The first batch is waited for here, once.  Without it the loop below is entered with these loads in flight, the
    // compiler's wait in front of the chain has to cover that entry too, and it then waits for the batch that was only just
    // requested on every trip: the loads ahead would hide nothing.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0); expcnt and lgkmcnt left alone
    for (; left > 0; left -= CU, z += dir * CU, row += CU * pitch) {
        const int rows = min(left, CU);
        if (left > CU) fetch(row + CU * pitch, z + dir * CU, min(left - CU, CU), nxt, tnx);
        auto batch = [&](auto whole) {
#pragma unroll
            for (int u = 0; u < CU; u++) {
                if (decltype(whole)::value || u < rows) {
                    const float t = lane_value(tv, u);
                    if (BACK) carry = cur[u] + t * carry;   // x_z = p_z + cp_z * x_{z+1}
                    else carry = (cur[u] + r * carry) * t;  // p_z = (v_z + r * p_{z-1}) * inv_z
                    cur[u] = carry;
                }
            }
            if (act) {  // asked once per batch, not per row
#pragma unroll
                for (int u = 0; u < CU; u++)
                    if (decltype(whole)::value || u < rows) row[u * pitch] = cur[u];
            }
        };
        if (rows == CU) batch(std::true_type());
        else batch(std::false_type());
#pragma unroll
        for (int u = 0; u < CU; u++) cur[u] = nxt[u];
        tv = tnx;
    }
}

template <int CU>
__global__ __launch_bounds__(LN) void hillslope_column_kernel(float *plane, const float *__restrict__ inv,
                                                              const float *__restrict__ cp, float r, int res) {
    const int lane = threadIdx.x;
    const int x = blockIdx.x * LN + lane, hi = res - 1;
    const bool act = x >= 1 && x <= hi - 1;
    float *col = plane + (size_t)blockIdx.y * res * res + min(x, hi);  // a lane beyond the tile reads the last column
    column_sweep<false, CU>(col, inv, r, res, lane, act, col[0]);               // p over v, from v_0
    column_sweep<true, CU>(col, cp, r, res, lane, act, col[(size_t)hi * res]);  // x over p, from v_{n-1}: this lane stored
                                                                                // every p it reloads
}

}  // namespace

int32_t nz_launch_hillslope_tables(hipStream_t s, float *inv, float *cp, float r, int res) {
    if (res < 3) return NZ_OK;
    NZ_LAUNCH(hillslope_tables_kernel, dim3(1), dim3(LN), 0, s, inv, cp, r, res);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_hillslope_step(hipStream_t s, const float *in, float *out, const float *inv, const float *cp, float r,
                                 int res, int count) {
    if (res < 3 || count <= 0) return NZ_OK;
    // a row, and with it a tile of the batch, starts 16-byte aligned when the plane does and res % 4 == 0
    const bool vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 && res % 4 == 0;
    const dim3 rows((res + LN - 1) / LN, count);
    if (vec) {
        NZ_LAUNCH((hillslope_row_kernel<true, false>), rows, dim3(LN), 0, s, in, out, inv, r, res);
        NZ_LAUNCH((hillslope_row_kernel<true, true>), rows, dim3(LN), 0, s, out, out, cp, r, res);
    } else {
        NZ_LAUNCH((hillslope_row_kernel<false, false>), rows, dim3(LN), 0, s, in, out, inv, r, res);
        NZ_LAUNCH((hillslope_row_kernel<false, true>), rows, dim3(LN), 0, s, out, out, cp, r, res);
    }
    // one column per lane on both paths: four columns per lane on the 16-byte path were measured and lost
    NZ_LAUNCH(hillslope_column_kernel<COLUMN_ROWS_AHEAD>, rows, dim3(LN), 0, s, out, inv, cp, r, res);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
