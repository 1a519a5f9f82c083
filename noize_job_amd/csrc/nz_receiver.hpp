// nz_receiver.hpp -- the receiver rule of the drainage network, stated once: step 1 of the fluvial model
// (include/noize_hip.h).  nz_fluvial.hip erodes along it, nz_drainage.hip accumulates down it, nz_watershed.hip labels and
// measures along it, nz_stream_order.hip orders the channels among it -- the last three through nz_donor_front.hpp; all
// include this file, so they cannot drift apart.
#pragma once

namespace nz_recv {

constexpr unsigned NONE = 8;            // receiver code of a cell without one
constexpr float DIAG = 0x1.6a09e6p-1f;  // 0.70710678f, bits 0x3F3504F3

// step 1 at one cell: c and its neighbours in the order W E S N SW SE NW NE; a tie keeps the earlier neighbour
__device__ __forceinline__ unsigned receiver(float c, float w, float e, float s, float n, float sw, float se, float nw,
                                             float ne, float &best, float &drop) {
    const float hk[8] = {w, e, s, n, sw, se, nw, ne};
    unsigned r = NONE;
    best = 0.0f;
    drop = 0.0f;
#pragma unroll
    for (unsigned k = 0; k < 8; k++) {
        const float d = c - hk[k];
        const float sl = k < 4 ? d : d * DIAG;
        if (sl > best) {
            best = sl;
            r = k;
            drop = d;
        }
    }
    return r;
}

// The donors of own cell j against the receiver codes cw of the thread's 3 x 6 window: bit k set when neighbour k drains
// here, that is when its receiver is the direction opposite to k -- E W N S NE NW SE SW.  nz_donor_front.hpp stores the mask;
// nz_fluvial.hip's gather keeps the same eight comparisons written out, which leaves its code object as it was.
__device__ __forceinline__ unsigned donor_mask(const unsigned (&cw)[3][6], int j) {
    unsigned m = 0;
    m |= (cw[1][j] == 1u) << 0;
    m |= (cw[1][j + 2] == 0u) << 1;
    m |= (cw[0][j + 1] == 3u) << 2;
    m |= (cw[2][j + 1] == 2u) << 3;
    m |= (cw[0][j] == 7u) << 4;
    m |= (cw[0][j + 2] == 6u) << 5;
    m |= (cw[2][j] == 5u) << 6;
    m |= (cw[2][j + 2] == 4u) << 7;
    return m;
}

}  // namespace nz_recv
