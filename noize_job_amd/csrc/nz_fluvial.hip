// nz_fluvial.hip -- stream-power fluvial erosion with drainage area (gfx950; new-framework feature).  The model is stated in
// include/noize_hip.h and restated step by step in tests/fluvial_ref.py: every cell drains to its steepest-descent
// neighbour of eight, the drainage area A takes one Jacobi step down that tree as a gather, and the bed is lowered by
// k sqrt(A) slope against an uplift.  Strict IEEE binary32 in every float mode, no contraction (-ffp-contract=off, Makefile),
// no atomics and a fixed summation order, so the result is independent of the launch shape.
//
// One launch per iteration on the geometry of nz_tile64.hpp: a workgroup produces a 64 x 16 tile of one plane, a thread
// four consecutive cells of a row (one 16-byte access per plane where plane and pitch allow, VEC), batch tiles on blockIdx.z:
//   fill     heights at radius 2 (5.6 KB) and drainage at radius 1 (5.1 KB) into LDS; a cell outside the grid reads as +0 and
//            is never looked at (below)
//   barrier
//   step 1   the receiver code of every cell at radius 1 into an LDS byte plane: a thread's own four cells as one 32-bit
//            write -- their slope and drop stay in registers -- and the 164 cells of the ring one per thread
//   barrier
//   step 2   the gather on the own cells: three code words and three 16-byte drainage reads per row of the 3 x 6 window
//   step 3   the square root and the update, one 16-byte store each to the height and the drainage plane
// "Outside the grid" never enters the arithmetic as a value: a border cell is an outlet and has no receiver, every other
// cell has all eight neighbours, and a ring cell outside the grid carries the code NONE so that nothing is gathered from
// it.  Every test is one on the cell's position (px, pz) against the grid's bounds [0, xhi] x [zlo, zhi], so a row stripe of
// a larger grid is this kernel on a window: WIN.  There the plane is one stripe-shaped buffer with a pitch, the bounds are
// the global grid's seen from the buffer (they may lie outside it), the workgroups tile the rows [r0, r1) the launch produces
// and a row is read when it lies within 2 rows of them and inside the grid -- the ghost rows the entry has checked for.  A
// row of the tile at or beyond r1 is read, since the rows above it need its receivers, but not produced.  Without WIN the
// window is the tile itself and the instantiations are what they were.
//
// CONSTA: the drainage read is the constant `rain` everywhere (the start state without rain map and drainageIn) and no
// drainage plane is read or staged.  MAPS: the three read-only maps travel as a trailing argument, each read at the cell
// itself only; a NULL map of the three reads as ones / zeros, which is the no-map arithmetic bit for bit.  The drainage
// planes alternate so that the last launch writes the plane the caller reads (nz_stages.cpp), so the last launch is no
// form of its own.
#include "nz_internal.hpp"
#include "nz_receiver.hpp"
#include "nz_tile64.hpp"

namespace {

using namespace nz_tile64;  // the tile, its LDS layout, ring_cell, halo2_cell
using nz_recv::NONE;      // receiver code of a cell without one
using nz_recv::receiver;  // step 1 at one cell (nz_receiver.hpp, shared with nz_drainage.hip)

// the plane a launch works on: tiles of res^2 cells back to back (pitch = res, everything else derived), or -- WIN -- a
// window of one stripe-shaped buffer, rows in buffer coordinates
struct fluvial_win {
    int pitch;     // floats between rows; without WIN the tile's resolution
    int xhi;       // last column of the grid
    int zlo, zhi;  // first and last row of the global grid
    int r0, r1;    // rows produced [r0, r1)
};

struct fluvial_maps {
    const float *rain_map, *hardness, *uplift_map;
};
__device__ __forceinline__ fluvial_maps maps_of() { return fluvial_maps{}; }
__device__ __forceinline__ fluvial_maps maps_of(const fluvial_maps &m) { return m; }

template <bool CONSTA, bool MAPS, bool VEC, bool WIN, class... M>
__global__ __launch_bounds__(FT) void fluvial_kernel(const float *__restrict__ h_in, float *__restrict__ h_out,
                                                     const float *__restrict__ a_in, float *__restrict__ a_out,
                                                     nz_fluvial_params k, fluvial_win win, M... ms) {
    static_assert(sizeof...(M) == (MAPS ? 1 : 0), "the maps travel with MAPS only");
    const fluvial_maps m = maps_of(ms...);
    __shared__ __attribute__((aligned(16))) float H[(FZ + 4) * LP];            // radius 2: LDS row = plane row - z0 + 2
    __shared__ __attribute__((aligned(16))) float A[CONSTA ? 4 : (FZ + 2) * LP];  // radius 1: LDS row = plane row - z0 + 1
    __shared__ __attribute__((aligned(16))) unsigned RW[(FZ + 2) * LP / 4];    // radius 1, one byte per cell
    unsigned char *RC = reinterpret_cast<unsigned char *>(RW);

    const int tid = threadIdx.x;
    const int pitch = win.pitch;
    const int x0 = blockIdx.x * FX, z0 = (WIN ? win.r0 : 0) + blockIdx.y * FZ;
    const size_t base = WIN ? 0 : (size_t)blockIdx.z * pitch * pitch;
    const int xhi = WIN ? win.xhi : pitch - 1, zlo = WIN ? win.zlo : 0, zhi = WIN ? win.zhi : pitch - 1;  // the grid's bounds
    // the rows that are read: the grid's, WIN: no further than 2 rows from the rows produced
    const int rlo = WIN ? (zlo > win.r0 - 2 ? zlo : win.r0 - 2) : zlo, rhi = WIN ? (zhi < win.r1 + 1 ? zhi : win.r1 + 1) : zhi;
    auto inside = [&](int px, int pz) { return px >= 0 && px <= xhi && pz >= rlo && pz <= rhi; };
    auto on_border = [&](int px, int pz) { return px == 0 || px == xhi || pz == zlo || pz == zhi; };
    // WIN without a drainage plane, with a rain map: the start state rain * rainMap[c], formed where it is read
    const bool a_start = WIN && MAPS && !CONSTA && a_in == nullptr;
    auto drain = [&](size_t q) { return a_start ? k.rain * m.rain_map[q] : a_in[q]; };

    // this thread's four cells
    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * pitch + px;
    const bool row_in = pz <= rhi;                    // read
    const bool row_out = WIN ? pz < win.r1 : row_in;  // and produced
    const bool quad = VEC && row_in && px + 3 <= xhi;  // VEC: cols % 4 == 0, so a quad lies inside or outside as a whole

    // ---- fill ----
    float hc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ac[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (quad) {
        const float4 v = *reinterpret_cast<const float4 *>(h_in + c0);
        hc[0] = v.x, hc[1] = v.y, hc[2] = v.z, hc[3] = v.w;
        if constexpr (!CONSTA) {
            if (a_start) {
                const float4 a = *reinterpret_cast<const float4 *>(m.rain_map + c0);
                ac[0] = k.rain * a.x, ac[1] = k.rain * a.y, ac[2] = k.rain * a.z, ac[3] = k.rain * a.w;
            } else {
                const float4 a = *reinterpret_cast<const float4 *>(a_in + c0);
                ac[0] = a.x, ac[1] = a.y, ac[2] = a.z, ac[3] = a.w;
            }
        }
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > xhi) break;
            hc[j] = h_in[c0 + j];
            if constexpr (!CONSTA) ac[j] = drain(c0 + j);
        }
    }
    *reinterpret_cast<float4 *>(&H[(tz + 2) * LP + LC + tx]) = make_float4(hc[0], hc[1], hc[2], hc[3]);
    if constexpr (!CONSTA) *reinterpret_cast<float4 *>(&A[(tz + 1) * LP + LC + tx]) = make_float4(ac[0], ac[1], ac[2], ac[3]);
    for (int i = tid; i < NHALO2; i += FT) {  // the heights at radius 1 and 2
        int lz, lx;
        halo2_cell(i, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 2;
        H[lz * LP + lx] = inside(qx, qz) ? h_in[base + (size_t)qz * pitch + qx] : 0.0f;
    }
    if constexpr (!CONSTA) {
        for (int i = tid; i < NRING; i += FT) {  // the drainage at radius 1
            int lz, lx;
            ring_cell(i, lz, lx);
            const int qx = x0 + lx - LC, qz = z0 + lz - 1;
            A[lz * LP + lx] = inside(qx, qz) ? drain(base + (size_t)qz * pitch + qx) : 0.0f;
        }
    }
    __syncthreads();

    // ---- step 1: receivers at radius 1 ----
    float S[4], drop[4];
    unsigned outlet = 0;  // bit j: own cell j is an outlet
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
            unsigned r = receiver(w[1][j + 1], w[1][j], w[1][j + 2], w[0][j + 1], w[2][j + 1], w[0][j], w[0][j + 2], w[2][j],
                                  w[2][j + 2], S[j], drop[j]);
            if (!inside(px + j, pz) || on_border(px + j, pz) || w[1][j + 1] <= k.sea_level) {
                r = NONE;
                S[j] = 0.0f;
                drop[j] = 0.0f;
                outlet |= 1u << j;
            }
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
            if (!(row[0] <= k.sea_level))
                r = receiver(row[0], row[-1], row[1], row[-LP], row[LP], row[-LP - 1], row[-LP + 1], row[LP - 1], row[LP + 1], s,
                             d);
        }
        RC[lz * LP + lx] = (unsigned char)r;
    }
    __syncthreads();

    // ---- steps 2 and 3 on the own cells ----
    if (!row_out || px > xhi) return;
    unsigned cw[3][6];  // the receiver codes of the window
    float aw[3][6];     // its drainage
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int l = (tz + r) * LP + LC + tx;
        const unsigned q = RW[l >> 2];
        cw[r][0] = RC[l - 1], cw[r][1] = q & 255u, cw[r][2] = (q >> 8) & 255u, cw[r][3] = (q >> 16) & 255u, cw[r][4] = q >> 24;
        cw[r][5] = RC[l + 4];
        if constexpr (CONSTA) {
#pragma unroll
            for (int j = 0; j < 6; j++) aw[r][j] = k.rain;
        } else {
            const float4 v = *reinterpret_cast<const float4 *>(&A[l]);
            aw[r][0] = A[l - 1], aw[r][1] = v.x, aw[r][2] = v.y, aw[r][3] = v.z, aw[r][4] = v.w, aw[r][5] = A[l + 4];
        }
    }
    float rm[4] = {1.0f, 1.0f, 1.0f, 1.0f}, hd[4] = {0.0f, 0.0f, 0.0f, 0.0f}, um[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (MAPS) {
        auto load4 = [&](const float *p, float (&o)[4]) {
            if (!p) return;
            if (quad) {
                const float4 v = *reinterpret_cast<const float4 *>(p + c0);
                o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (px + j <= xhi) o[j] = p[c0 + j];
            }
        };
        load4(m.rain_map, rm);
        load4(m.hardness, hd);
        load4(m.uplift_map, um);
    }
    const float dtu = k.dt * k.uplift;
    float hn[4], an[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        // neighbour k drains here: nz_recv::donor_mask's comparisons, written out (the mask changes this code object)
        float a = MAPS ? k.rain * rm[j] : k.rain;
        if (cw[1][j] == 1u) a = a + aw[1][j];
        if (cw[1][j + 2] == 0u) a = a + aw[1][j + 2];
        if (cw[0][j + 1] == 3u) a = a + aw[0][j + 1];
        if (cw[2][j + 1] == 2u) a = a + aw[2][j + 1];
        if (cw[0][j] == 7u) a = a + aw[0][j];
        if (cw[0][j + 2] == 6u) a = a + aw[0][j + 2];
        if (cw[2][j] == 5u) a = a + aw[2][j];
        if (cw[2][j + 2] == 4u) a = a + aw[2][j + 2];
        an[j] = a;
        if (outlet >> j & 1u) {
            hn[j] = hc[j];
        } else {
            const float kc = MAPS ? k.erodibility * (1.0f - hd[j]) : k.erodibility;
            float e = ((kc * sqrtf(a)) * S[j]) * k.dt;
            const float lim = drop[j] * 0.5f;
            e = lim < e ? lim : e;
            const float du = MAPS ? dtu * um[j] : dtu;
            hn[j] = (hc[j] - e) + du;
        }
    }
    if (quad) {
        *reinterpret_cast<float4 *>(h_out + c0) = make_float4(hn[0], hn[1], hn[2], hn[3]);
        *reinterpret_cast<float4 *>(a_out + c0) = make_float4(an[0], an[1], an[2], an[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > xhi) break;
            h_out[c0 + j] = hn[j];
            a_out[c0 + j] = an[j];
        }
    }
}

// the start state with a rain map: A = rain * rainMap[c]
__global__ __launch_bounds__(256) void fluvial_start_kernel(float *__restrict__ a, const float *__restrict__ rain_map,
                                                            float rain, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = rain * rain_map[i];
}

template <bool CONSTA, bool MAPS, bool WIN>
void launch(bool vec, dim3 grid, hipStream_t s, const float *h_in, float *h_out, const float *a_in, float *a_out,
            const nz_fluvial_params &k, const fluvial_win &w, const fluvial_maps &m) {
    if constexpr (MAPS) {
        if (vec) NZ_LAUNCH((fluvial_kernel<CONSTA, true, true, WIN, fluvial_maps>), grid, dim3(FT), 0, s, h_in, h_out, a_in, a_out, k, w, m);
        else NZ_LAUNCH((fluvial_kernel<CONSTA, true, false, WIN, fluvial_maps>), grid, dim3(FT), 0, s, h_in, h_out, a_in, a_out, k, w, m);
    } else {
        if (vec) NZ_LAUNCH((fluvial_kernel<CONSTA, false, true, WIN>), grid, dim3(FT), 0, s, h_in, h_out, a_in, a_out, k, w);
        else NZ_LAUNCH((fluvial_kernel<CONSTA, false, false, WIN>), grid, dim3(FT), 0, s, h_in, h_out, a_in, a_out, k, w);
    }
}

// the form by the planes given: no drainage plane and no rain map is CONSTA; no drainage plane with a rain map is, WIN, the
// start state formed in the kernel (the tile entry writes it to a plane first, nz_stages.cpp)
template <bool WIN>
void dispatch(bool vec, dim3 grid, hipStream_t s, const float *h_in, float *h_out, const float *a_in, float *a_out,
              const nz_fluvial_params &k, const fluvial_win &w, const fluvial_maps &m) {
    const bool maps = m.rain_map || m.hardness || m.uplift_map;
    if (!a_in && !(WIN && m.rain_map)) {
        if (maps) launch<true, true, WIN>(vec, grid, s, h_in, h_out, a_in, a_out, k, w, m);
        else launch<true, false, WIN>(vec, grid, s, h_in, h_out, a_in, a_out, k, w, m);
    } else {
        if (maps) launch<false, true, WIN>(vec, grid, s, h_in, h_out, a_in, a_out, k, w, m);
        else launch<false, false, WIN>(vec, grid, s, h_in, h_out, a_in, a_out, k, w, m);
    }
}

}  // namespace

int32_t nz_launch_fluvial_start(hipStream_t s, float *a, const float *rain_map, float rain, size_t n) {
    if (n == 0) return NZ_OK;
    NZ_LAUNCH(fluvial_start_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, rain_map, rain, n);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial(hipStream_t s, const float *h_in, float *h_out, const float *a_in, float *a_out,
                          const nz_fluvial_params &k, int res, int count, const float *rain_map, const float *hardness,
                          const float *uplift_map) {
    if (res <= 0 || count <= 0) return NZ_OK;
    const dim3 grid(tiles_x(res), tiles_z(res), count);
    const fluvial_maps m{rain_map, hardness, uplift_map};
    uintptr_t bits = reinterpret_cast<uintptr_t>(h_in) | reinterpret_cast<uintptr_t>(h_out) |
                     reinterpret_cast<uintptr_t>(a_in) | reinterpret_cast<uintptr_t>(a_out) |
                     reinterpret_cast<uintptr_t>(rain_map) | reinterpret_cast<uintptr_t>(hardness) |
                     reinterpret_cast<uintptr_t>(uplift_map);
    const bool vec = (bits & 15) == 0 && res % 4 == 0;  // a row, and with it a tile of the batch, starts 16-byte aligned
    dispatch<false>(vec, grid, s, h_in, h_out, a_in, a_out, k, fluvial_win{res, res - 1, 0, res - 1, 0, res}, m);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}

int32_t nz_launch_fluvial_stripe(hipStream_t s, const float *h_in, float *h_out, const float *a_in, float *a_out,
                                 const nz_fluvial_params &k, const nz_geom &g, int zlo, int zhi, const float *rain_map,
                                 const float *hardness, const float *uplift_map) {
    if (g.or1 <= g.or0 || g.cols <= 0) return NZ_OK;
    const dim3 grid(tiles_x(g.cols), tiles_z(g.or1 - g.or0), 1);
    const fluvial_maps m{rain_map, hardness, uplift_map};
    uintptr_t bits = reinterpret_cast<uintptr_t>(h_in) | reinterpret_cast<uintptr_t>(h_out) |
                     reinterpret_cast<uintptr_t>(a_in) | reinterpret_cast<uintptr_t>(a_out) |
                     reinterpret_cast<uintptr_t>(rain_map) | reinterpret_cast<uintptr_t>(hardness) |
                     reinterpret_cast<uintptr_t>(uplift_map);
    const bool vec = (bits & 15) == 0 && g.cols % 4 == 0 && g.pitch % 4 == 0;  // every row starts 16-byte aligned
    dispatch<true>(vec, grid, s, h_in, h_out, a_in, a_out, k, fluvial_win{g.pitch, g.cols - 1, zlo, zhi, g.or0, g.or1}, m);
    NZ_HIP(hipGetLastError());
    return NZ_OK;
}
