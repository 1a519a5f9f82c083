"""What one fused flow launch must leave behind, from the oracle's per-step pieces (test infrastructure).

A launch of the flow stage (nz_flow_fused_stripe, one launch of nz_flowmap_stage*) runs n iterations of (ComputeFlowStep,
UpdateWaterStep) on a state {water, fN, fS, fE, fW}.  `first`: the state is the implied one (water 1e-4, flux 0).
`last`: the n-th water update is dead; the launch ends in CreateVelocityField + NormalizeMap and leaves one plane.
oracle.flow_step / water_step / velocity / normalize chained exactly as tests/oracle_stripe_ops.py chains them for the
sharding schedule: the oracle clamps at the edge of the plane it is given, so a plane handed to it ends at the grid's border
or 2n rows beyond the rows that are wanted."""
import numpy as np

import oracle as O
from conv_ref import assert_bits_equal  # noqa: F401  (the sign of a zero counts; a NaN matches any NaN)

f32 = np.float32
NORM = (0.0, 0.005)


def terrain(rng, rows, cols):
    """A test input: relief and roughness on the scale of the water column (1e-4), so that water moves in every cell, in all
    four directions, and runs dry in a few."""
    x, z = np.arange(cols), np.arange(rows)
    base = 3e-4 * np.sin(x * 0.05 + rng.random() * 6)[None, :] * np.cos(z * 0.07 + rng.random() * 6)[:, None]
    return (base.astype(f32) + rng.random((rows, cols), dtype=f32) * f32(2e-4)).astype(f32)


def split_iterations(total, cap):
    """nz_split_iterations: fewest launches of at most `cap`, as even as they go, larger first."""
    L = (total + cap - 1) // cap
    return [total // L + (1 if i < total % L else 0) for i in range(L)]


def initial_state(shape):
    return [np.full(shape, 0.0001, f32)] + [np.zeros(shape, f32) for _ in range(4)]


def launch(h, n, first, last, state=None, norm=NORM):
    """One launch on the whole grid `h`: the five state planes [water, fN, fS, fE, fW], or the normalised plane if `last`."""
    h = np.ascontiguousarray(h, f32)
    if first:
        state = initial_state(h.shape)
    w, fl = state[0], list(state[1:])
    for it in range(n):
        fl = O.flow_step(h, w, *fl)
        if not (last and it == n - 1):
            w = O.water_step(w, *fl)
    if last:
        return O.normalize(O.velocity(*fl), *norm)
    return [w] + list(fl)


def chain(h, split, norm=NORM):
    """The stage as launches of split[0], split[1], ... iterations.  Returns (result, states): states[k] is the state
    the k-th launch reads (None for the first), so states[k + 1] is what launch k writes."""
    states, state = [None], None
    for k, n in enumerate(split):
        last = k == len(split) - 1
        out = launch(h, n, k == 0, last, state, norm)
        if last:
            return out, states
        state = out
        states.append(state)
    raise ValueError("empty split")


def stripe_launch(h, g0, g1, n, first, last, state=None, norm=NORM):
    """Rows [g0, g1) of launch(h, ...), computed from those rows and 2n ghost rows of `h` (and of `state`) either side, or
    fewer where the grid ends first."""
    lo, hi = max(0, g0 - 2 * n), min(h.shape[0], g1 + 2 * n)
    sub = None if first else [np.ascontiguousarray(p[lo:hi]) for p in state]
    out = launch(h[lo:hi], n, first, last, sub, norm)
    cut = slice(g0 - lo, g1 - lo)
    return out[cut] if last else [p[cut] for p in out]
