// nz_planes.hpp -- row-stripe geometry and plane aliasing checks of the stage entry points.  Pure host C++: no HIP header,
// so that a plain C++ compiler can build it on its own (tests/planes_check.cpp does).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/noize_hip.h"

// ---- error plumbing -------------------------------------------------------------------------
void nz_set_error(const char *fmt, ...);

#define NZ_REQUIRE(cond, ...)        \
    do {                             \
        if (!(cond)) {               \
            nz_set_error(__VA_ARGS__); \
            return NZ_ERR_INVALID;   \
        }                            \
    } while (0)

// ---- row stripes ----------------------------------------------------------------------------
// halo / halo_below: rows needed above / below the owned ones (halo_below < 0: as many as above)
inline int32_t nz_check_stripe(const nz_stripe *st, int halo, int halo_below = -1) {
    if (halo_below < 0) halo_below = halo;  // symmetric stencil
    NZ_REQUIRE(st, "stripe is NULL");
    NZ_REQUIRE(st->cols > 0 && st->rows > 0 && st->grows > 0, "stripe: non-positive extent");
    NZ_REQUIRE(st->pitch == 0 || st->pitch >= st->cols, "stripe: pitch < cols");
    NZ_REQUIRE(st->own0 >= 0 && st->own0 <= st->own1 && st->own1 <= st->rows, "stripe: owned rows outside buffer");
    NZ_REQUIRE(st->own0 + st->grow0 >= 0 && st->own1 + st->grow0 <= st->grows,
               "stripe: owned rows outside the global grid");
    // every row within `halo` of the owned rows must be in the buffer unless it is beyond the border
    int need_lo = st->own0 - halo, need_hi = st->own1 - 1 + halo_below;
    int dom_lo = -st->grow0, dom_hi = st->grows - 1 - st->grow0;
    if (need_lo < dom_lo) need_lo = dom_lo;
    if (need_hi > dom_hi) need_hi = dom_hi;
    NZ_REQUIRE(need_lo >= 0 && need_hi <= st->rows - 1, "stripe: %d ghost rows required above, %d below", halo,
               halo_below);
    return NZ_OK;
}

inline int nz_stripe_pitch(const nz_stripe &st) { return st.pitch > 0 ? st.pitch : st.cols; }  // floats between rows
// the floats a stripe-shaped plane may be touched in: its last row ends with its last cell
inline size_t nz_stripe_span(const nz_stripe &st) { return (size_t)(st.rows - 1) * nz_stripe_pitch(st) + st.cols; }
// rows * pitch, what a plane carved out of a work buffer takes; 0 for a stripe that cannot be sized
inline size_t nz_stripe_plane_floats(const nz_stripe *st) {
    return st && st->rows > 0 && st->cols > 0 && st->pitch >= 0 ? (size_t)st->rows * nz_stripe_pitch(*st) : 0;
}

// The global grid in buffer rows is [nz_stripe_grid_lo, nz_stripe_grid_hi) = [-grow0, grows - grow0); either end may lie
// outside the buffer.  The kernels that take the grid as inclusive rows [zlo, zhi] get (lo, hi - 1).
inline int nz_stripe_grid_lo(const nz_stripe &st) { return -st.grow0; }
inline int nz_stripe_grid_hi(const nz_stripe &st) { return st.grows - st.grow0; }

// The rows [*or0, *or1) a launch produces that has to leave `widen` valid rows on each side of the owned ones for the
// launches behind it: launch j of an n-iteration call of radius r has widen = r * (n - 1 - j).  The widened rows are
// clipped to the grid only, not to the buffer: the stripe has passed nz_check_stripe(st, halo) with halo >= widen, which
// puts every row within `halo` of the owned ones into the buffer unless it lies beyond the grid, so the clip can bite only
// at the grid's own border and 0 <= *or0 <= *or1 <= rows.
inline void nz_stripe_window(const nz_stripe &st, int widen, int *or0, int *or1) {
    const int lo = nz_stripe_grid_lo(st), hi = nz_stripe_grid_hi(st);
    *or0 = st.own0 - widen > lo ? st.own0 - widen : lo;
    *or1 = st.own1 + widen < hi ? st.own1 + widen : hi;
}

// ---- aliasing -------------------------------------------------------------------------------
// Do the byte ranges [a, a + na) and [b, b + nb) share a byte?  A NULL plane overlaps nothing; ranges that merely touch
// do not overlap.
inline bool nz_bytes_overlap(const void *a, size_t na, const void *b, size_t nb) {
    return a && b && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}
// the same for planes of na / nb floats
inline bool nz_planes_overlap(const float *a, size_t na, const float *b, size_t nb) {
    return nz_bytes_overlap(a, na * sizeof(float), b, nb * sizeof(float));
}

struct nz_named_plane { const char *name; const float *p; size_t floats; };  // p NULL: a plane the call does not have
// Every plane a call writes lies apart from every plane it reads and from every other plane it writes; planes that are only
// read may alias.  Write i is checked against every read, then against the writes behind it; the first clash is reported
// as "<write> overlaps <other>".
static inline int32_t nz_require_disjoint(const nz_named_plane *writes, size_t nw, const nz_named_plane *reads, size_t nr) {
    for (size_t i = 0; i < nw; i++) {
        const nz_named_plane &w = writes[i];
        for (size_t j = 0; j < nr; j++)
            NZ_REQUIRE(!nz_planes_overlap(w.p, w.floats, reads[j].p, reads[j].floats), "%s overlaps %s", w.name, reads[j].name);
        for (size_t j = i + 1; j < nw; j++)
            NZ_REQUIRE(!nz_planes_overlap(w.p, w.floats, writes[j].p, writes[j].floats), "%s overlaps %s", w.name,
                       writes[j].name);
    }
    return NZ_OK;
}
