// nz_tile64.hpp -- the workgroup geometry of nz_fluvial.hip, nz_fill.hip, nz_drainage.hip, nz_watershed.hip and
// nz_stream_order.hip (and of nz_donor_front.hpp, the mask launches of the last three), stated once: FT = 256 threads
// own an FX x FZ = 64 x 16 tile of one plane, a thread four consecutive cells of a row (16-byte accesses where planes and
// pitch allow), batch tiles on blockIdx.z.  A plane staged in LDS has LP = 72 cells per row with the tile at column LC = 4:
// a thread's four cells are one aligned float4, and a radius-R plane keeps plane row z0 + i in LDS row R + i.
#pragma once

namespace nz_tile64 {

constexpr int FX = 64, FZ = 16;  // tile of one workgroup
constexpr int FT = 256;          // threads: one per four cells of a row
constexpr int LP = 72;           // LDS row pitch in cells; plane column x0 + i is LDS column LC + i
constexpr int LC = 4;            // keeps a thread's four cells 16-byte aligned in LDS
constexpr int NRING = 2 * (FX + 2) + 2 * FZ;   // cells at radius 1 around the tile
constexpr int NHALO2 = 4 * (FX + 4) + 4 * FZ;  // cells at radius 1 and 2 around the tile

// tiles across `cols` columns and down `rows` rows: the launch grid, and the host's count of per-tile bytes
constexpr int tiles_x(int cols) { return (cols + FX - 1) / FX; }
constexpr int tiles_z(int rows) { return (rows + FZ - 1) / FZ; }

// the ring at radius 1 of the tile, cell i of NRING: its LDS row and column in a radius-1 plane
__device__ __forceinline__ void ring_cell(int i, int &lz, int &lx) {
    if (i < 2 * (FX + 2)) {
        const int rr = i / (FX + 2);
        lz = rr ? FZ + 1 : 0;
        lx = LC - 1 + (i - rr * (FX + 2));
    } else {
        const int j = i - 2 * (FX + 2);
        lz = 1 + (j >> 1);
        lx = (j & 1) ? LC + FX : LC - 1;
    }
}

// the cells at radius 1 and 2 of the tile, cell i of NHALO2: its LDS row and column in a radius-2 plane
__device__ __forceinline__ void halo2_cell(int i, int &lz, int &lx) {
    if (i < 4 * (FX + 4)) {
        const int rr = i / (FX + 4);
        lz = rr < 2 ? rr : FZ + rr;
        lx = LC - 2 + (i - rr * (FX + 4));
    } else {
        const int j = i - 4 * (FX + 4), cc = j & 3;
        lz = 2 + (j >> 2);
        lx = cc < 2 ? LC - 2 + cc : LC + FX - 2 + cc;
    }
}

// a thread's 3 x 6 window (rows pz-1 .. pz+1, columns px-1 .. px+4) of a radius-1 byte plane held as words
__device__ __forceinline__ void window_bytes(const unsigned *words, int tz, int tx, unsigned (&w)[3][6]) {
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(words);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int l = (tz + r) * LP + LC + tx;
        const unsigned q = words[l >> 2];
        w[r][0] = bytes[l - 1], w[r][1] = q & 255u, w[r][2] = (q >> 8) & 255u, w[r][3] = (q >> 16) & 255u, w[r][4] = q >> 24;
        w[r][5] = bytes[l + 4];
    }
}

// the LDS cell of a radius-1 plane that neighbour code k -- W E S N SW SE NW NE -- of a thread's own cell j names; k >= 8
// (no neighbour): the cell itself
__device__ __forceinline__ int neighbour_lds(int tz, int tx, int j, int k) {
    const int dx = k >= 8 || k == 2 || k == 3 ? 0 : (k & 1) ? 1 : -1;
    const int dz = k >= 8 || k < 2 ? 0 : (k == 3 || k >= 6) ? 1 : -1;
    return (tz + 1 + dz) * LP + LC + tx + j + dx;
}

}  // namespace nz_tile64
