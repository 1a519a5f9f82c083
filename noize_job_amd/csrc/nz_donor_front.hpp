// nz_donor_front.hpp -- the front end of the stages that relax along the receiver graph, stated once: from heights to
// receiver codes (nz_recv::receiver) and from receiver codes to DONOR BYTES, on the geometry of nz_tile64.hpp.
// nz_drainage.hip's mask launch (tile and stripe form) and nz_stream_order.hip's are donor_front; nz_watershed.hip's
// receiver launch, which stops at the codes and needs heights at radius 1 only, takes receiver_codes4 from here.
// Include nz_receiver.hpp and nz_tile64.hpp first.
#pragma once

namespace nz_front {

using namespace nz_tile64;

// WIN: the owned rows of one stripe-shaped buffer, rows in buffer coordinates; the pitch travels as the kernels' `res`
struct win_rows {
    int xhi;       // last column of the grid
    int zlo, zhi;  // first and last row of the global grid
    int r0, r1;    // owned rows [r0, r1)
};

// The receiver codes of a thread's four cells as one word, from its 3 x 6 window (rows pz-1 .. pz+1, columns px-1 .. px+4)
// of the height plane H in LDS, `top` the LDS row of pz-1.  NONE where dead(j) says the rule gives own cell j no receiver
// (border, outside the grid, no channel) and for a cell at or below the sea.
template <class Dead>
__device__ __forceinline__ unsigned receiver_codes4(const float *H, int top, int tx, float sea, Dead dead) {
    float w[3][6];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float *row = &H[(top + r) * LP + LC + tx];
        const float4 v = *reinterpret_cast<const float4 *>(row);
        w[r][0] = row[-1], w[r][1] = v.x, w[r][2] = v.y, w[r][3] = v.z, w[r][4] = v.w, w[r][5] = row[4];
    }
    unsigned codes = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float s, d;
        unsigned r = nz_recv::receiver(w[1][j + 1], w[1][j], w[1][j + 2], w[0][j + 1], w[2][j + 1], w[0][j], w[0][j + 2],
                                       w[2][j], w[2][j + 2], s, d);
        if (dead(j) || w[1][j + 1] <= sea) r = nz_recv::NONE;
        codes |= r << (8 * j);
    }
    return codes;
}

// The body of a mask launch: heights at radius 2 into LDS, receiver codes at radius 1, and per own cell one donor byte --
// bit k set when neighbour k exists and its receiver is the direction opposite to k.  After it no launch looks at a height.
// VEC: 16-byte reads of the float planes; WORD: the four bytes of a thread as one 32-bit store (res % 4 == 0)
// WIN: res is the pitch; heights are read on the rows within 2 of the owned ones, bytes stored for the owned rows, at the
// cell's index in the plane
// CH: the channel predicate ch(c) = drainage == NULL || drainage[c] >= threshold, read at radius 1, is folded into the
// receiver codes -- a cell that is no channel gets NONE, it donates to nothing -- so the bytes are CHANNEL-donor bytes, and
// the start state ch ? 1 : 0 goes to `order` beside them.  Without CH `drainage` and `order` are not looked at.
template <bool VEC, bool WORD, bool WIN, bool CH>
__device__ __forceinline__ void donor_front(const float *__restrict__ h, const float *__restrict__ drainage,
                                            unsigned char *__restrict__ donors, unsigned char *__restrict__ order, float sea,
                                            float threshold, int res, const win_rows &win) {
    __shared__ __attribute__((aligned(16))) float H[(FZ + 4) * LP];          // radius 2: LDS row = plane row - z0 + 2
    __shared__ __attribute__((aligned(16))) unsigned RW[(FZ + 2) * LP / 4];  // radius 1, one byte per cell
    unsigned char *RC = reinterpret_cast<unsigned char *>(RW);

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FX, z0 = (WIN ? win.r0 : 0) + blockIdx.y * FZ;
    const size_t base = WIN ? 0 : (size_t)blockIdx.z * res * res;
    const int hi = WIN ? win.xhi : res - 1;                            // last column
    const int zlo = WIN ? win.zlo : 0, zhi = WIN ? win.zhi : res - 1;  // the grid's rows
    const int rlo = WIN ? (zlo > win.r0 - 2 ? zlo : win.r0 - 2) : 0, rhi = WIN ? (zhi < win.r1 + 1 ? zhi : win.r1 + 1) : hi;  // rows read
    const bool all = CH && drainage == nullptr;  // every cell is a channel cell
    auto inside = [&](int px, int pz) { return px >= 0 && px <= hi && pz >= rlo && pz <= rhi; };
    auto on_border = [&](int px, int pz) { return px == 0 || px == hi || pz == zlo || pz == zhi; };

    const int tz = tid >> 4, tx = (tid & 15) * 4;
    const int px = x0 + tx, pz = z0 + tz;
    const size_t c0 = base + (size_t)pz * res + px;
    const bool row_in = pz <= rhi;  // WIN: the two rows below the owned ones lie in own slots when the tile reaches them
    const bool quad = row_in && px + 3 <= hi;

    // ---- fill: a cell outside the grid reads as +0 and is never looked at; it is no channel ----
    float hc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned chw = 0;  // CH: ch of the own cells, one byte each: the start state of their order
    if (VEC && quad) {
        const float4 v = *reinterpret_cast<const float4 *>(h + c0);
        hc[0] = v.x, hc[1] = v.y, hc[2] = v.z, hc[3] = v.w;
        if constexpr (CH) {
            chw = 0x01010101u;
            if (!all) {
                const float4 a = *reinterpret_cast<const float4 *>(drainage + c0);
                chw = (unsigned)(a.x >= threshold) | (unsigned)(a.y >= threshold) << 8 | (unsigned)(a.z >= threshold) << 16 |
                      (unsigned)(a.w >= threshold) << 24;
            }
        }
    } else if (!VEC && row_in) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            hc[j] = h[c0 + j];
            if constexpr (CH) chw |= (unsigned)(all || drainage[c0 + j] >= threshold) << (8 * j);
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

    // ---- receivers at radius 1: NONE for an outlet, for a cell outside the grid and (CH) for a cell that is no channel ----
    RW[((tz + 1) * LP + LC + tx) >> 2] = receiver_codes4(H, tz + 1, tx, sea, [&](int j) {
        return (CH ? !((chw >> (8 * j)) & 1u) : !inside(px + j, pz)) || on_border(px + j, pz);  // (chw: inside, too)
    });
    if (tid < NRING) {
        int lz, lx;
        ring_cell(tid, lz, lx);
        const int qx = x0 + lx - LC, qz = z0 + lz - 1;
        unsigned r = nz_recv::NONE;
        if (inside(qx, qz) && !on_border(qx, qz)) {
            const float *row = &H[(lz + 1) * LP + lx];
            float s, d;
            if (!(row[0] <= sea) && (!CH || all || drainage[base + (size_t)qz * res + qx] >= threshold))
                r = nz_recv::receiver(row[0], row[-1], row[1], row[-LP], row[LP], row[-LP - 1], row[-LP + 1], row[LP - 1],
                                      row[LP + 1], s, d);
        }
        RC[lz * LP + lx] = (unsigned char)r;
    }
    __syncthreads();

    // ---- the donor bytes of the own cells, and (CH) their start state ----
    if (!(WIN ? pz < win.r1 : row_in) || px > hi) return;
    unsigned cw[3][6];  // the receiver codes of the window
    window_bytes(RW, tz, tx, cw);
    unsigned word = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) word |= nz_recv::donor_mask(cw, j) << (8 * j);
    if (WORD && quad) {
        *reinterpret_cast<unsigned *>(donors + c0) = word;
        if constexpr (CH) *reinterpret_cast<unsigned *>(order + c0) = chw;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (px + j > hi) break;
            donors[c0 + j] = (unsigned char)(word >> (8 * j));
            if constexpr (CH) order[c0 + j] = (unsigned char)(chw >> (8 * j));
        }
    }
}

}  // namespace nz_front
