// nz_relax_pass.hpp -- the pass protocol of an iterate-to-rest series, stated once: nz_fill.hip relaxes W with it,
// nz_drainage.hip A.  What a cell is relaxed to is theirs; how a series of launches finds out, without the host, that it
// has come to rest is here.
//
// One launch per PASS on the geometry of nz_tile64.hpp.  A pass reads plane_in and writes plane_out, two planes that
// alternate, so no workgroup waits for another and no launch has a race:
//   gate     pass p first reads changed[(p - 1) % 3]; zero means the pass before changed nothing, both planes hold the
//            fixed point, and the whole launch returns at once -- as does every later one (series_gate).
//   skip     when neither this tile nor one of its eight neighbours changed in the pass before -- one byte per tile, two
//            generations alternating with the planes -- the tile is at rest against an unchanged ring: it writes a zero
//            byte and returns (tile_live).  No copy is needed: a tile that did not change has equal cells in both planes.
//   sweeps   on the stage's plane at radius 1 in LDS, the ring frozen: every thread reads its 3 x 6 window and updates its
//            four cells in registers, a workgroup-wide OR of "changed" doubles as the barrier behind the read phase, then
//            the write phase and a second barrier.  The loop ends when a sweep changes nothing, or after `sweeps` of them.
//   store    the own cells to plane_out (the stage), the tile's byte, and one ordinary global atomic on changed[p % 3] when
//            they changed (close_tile).
// Three words in turn are enough: pass p reads word p - 1, bumps word p and (one thread of the grid) zeroes word p + 1,
// which no launch touches before pass p + 1 bumps it.  The first pass changes every tile by decree -- its predecessor is the
// start state, which exists in no plane -- so it consults neither word nor bytes, and pass 1 writes all of the second plane:
// a tile skipped later has been written in both planes, and a series that came to rest holds the fixed point in BOTH.  The
// finalise launch looks at the word of the last pass that ran (series_at_rest): zero is the fixed point, else all or nothing.
//
// The fill's stripe form runs a series per ROUND: status[ST_GO] lets every launch of a round return at once, and pass 0 of
// a round that continues from a caller's plane has neither word nor bytes to go by: all_live, decreed nothing, bumps its word.
#pragma once

namespace nz_relax {

constexpr int ST_PASSES = 0, ST_CONVERGED = 1, ST_CHANGED = 2;  // the status words: changed[3] from ST_CHANGED on
constexpr int ST_GO = 5;                                          // stripe rounds: 0 = every launch returns at once

// Did the pass before change anything at all?  Zero: the series is at rest and the launch returns.  One thread of the
// grid prepares the next pass's word and counts this one.  t0: thread 0 of its workgroup (formed once, by the kernel).
template <bool FIRST>
__device__ __forceinline__ int series_gate(int *status, bool t0, int pass, bool all_live) {
    int *changed = status + ST_CHANGED;
    const int prev = FIRST || all_live ? 1 : changed[(pass + 2) % 3];
    if (t0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
        changed[(pass + 1) % 3] = 0;
        if (FIRST) changed[0] = 1;  // by decree; no workgroup bumps it
        if (prev) status[ST_PASSES] = pass + 1;
    }
    return prev;
}

// Did this tile or one of its eight neighbours change in the pass before?  Thread t < 9 answers for neighbour t; the kernel
// ORs the answers (__syncthreads_or, called there: inside a helper the compiler forms the workgroup size the long way).
// Zero: at rest; a zero byte and return.  tnx x tnz: the tiles of one plane, tile0: the byte of its first.
__device__ __forceinline__ int tile_live(const unsigned char *flags_in, size_t tile0, int tnx, int tnz, int tid) {
    int live = 0;
    if (tid < 9) {
        const int bx = (int)blockIdx.x + tid % 3 - 1, bz = (int)blockIdx.y + tid / 3 - 1;
        if (bx >= 0 && bx < tnx && bz >= 0 && bz < tnz) live = flags_in[tile0 + (size_t)bz * tnx + bx];
    }
    return live;
}

// the end of a tile's pass, one thread of the workgroup: its byte, and its share of the pass's word
template <bool FIRST>
__device__ __forceinline__ void close_tile(int *status, unsigned char *flags_out, size_t me, int pass, bool moved) {
    int *changed = status + ST_CHANGED;
    flags_out[me] = moved ? 1 : 0;
    if (!FIRST && moved) atomicAdd(&changed[pass % 3], 1);
}

// the verdict of a finalise launch: the last pass that ran changed nothing
__device__ __forceinline__ bool series_at_rest(const int *status) {
    const int passes = status[ST_PASSES];
    return status[ST_CHANGED + (passes + 2) % 3] == 0;
}

}  // namespace nz_relax
