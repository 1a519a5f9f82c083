// nz_mfd_weights.hpp -- the multiple-flow weights of a cell, stated once: nz_drainage_mfd.hip gathers drainage along them,
// nz_fluvial_implicit_mfd.hip erodes along them.  The model is nz_drainage_mfd's (include/noize_hip.h): s_k = h[c] - h[k]
// (times DIAG for k >= 4), k takes flow iff s_k > 0, q_k = s_k / best, g_k = q_k ^ exponent by repeated multiplication, T
// the sum of the g_k > 0 with k ascending, w_k = g_k / T.  Every operation rounded once.
#pragma once

#include "nz_receiver.hpp"
#include "nz_tile64.hpp"

namespace nz_mfd {

// q ^ exponent, left to right: exponent - 1 multiplications
__device__ __forceinline__ float mfd_power(float q, int exponent) {
    float g = q;
    for (int e = 1; e < exponent; e++) g = g * q;
    return g;
}

// `best` and T of the cell at p in a height plane of pitch LP whose eight neighbours all exist
__device__ __forceinline__ void mfd_send_terms(const float *p, int exponent, float &best, float &total) {
    constexpr int LP = nz_tile64::LP;
    const float c = p[0];
    const float hk[8] = {p[-1], p[1], p[-LP], p[LP], p[-LP - 1], p[-LP + 1], p[LP - 1], p[LP + 1]};
    float s[8];
    best = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float d = c - hk[k];
        s[k] = k < 4 ? d : d * nz_recv::DIAG;
        if (s[k] > best) best = s[k];
    }
    total = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (s[k] > 0.0f) {
            const float g = mfd_power(s[k] / best, exponent);
            if (g > 0.0f) total = total + g;  // an infinite s gives a NaN g, an underflow +0: nothing
        }
    }
}

// the eight OUTGOING weights of the cell at p, +0 where nothing goes: the same s, `best`, g and T as above, and the same
// division as the gathering side's (g / T), so a weight is one float whichever side forms it
__device__ __forceinline__ void mfd_out_weights(const float *p, int exponent, float (&w)[8]) {
    constexpr int LP = nz_tile64::LP;
    float best, total;
    mfd_send_terms(p, exponent, best, total);
    const float c = p[0];
    const float hk[8] = {p[-1], p[1], p[-LP], p[LP], p[-LP - 1], p[-LP + 1], p[LP - 1], p[LP + 1]};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float d = c - hk[k];
        const float s = k < 4 ? d : d * nz_recv::DIAG;
        float v = 0.0f;
        if (s > 0.0f) {
            const float g = mfd_power(s / best, exponent);
            if (g > 0.0f) v = g / total;
        }
        w[k] = v;
    }
}

}  // namespace nz_mfd
