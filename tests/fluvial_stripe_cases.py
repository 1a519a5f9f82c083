"""Cases, buffers and drivers shared by tests/test_fluvial_stripe_ref.py (CPU) and tests/test_gpu_fluvial_stripe.py: the
grids and splits, the parameter sets, one rank's NaN-filled buffers for fluvial_steps, the lockstep run and the comparison."""
import functools

import numpy as np
import torch

import fluvial_ref as F
from test_hydraulic_stripe_ref import copy_rows, terrain

NAMES = ("erodibility", "uplift", "dt", "rain", "seaLevel")
# the stage's defaults; a sea level with fractional rain
PARAMS = [(0.05, 0.002, 1.0, 1.0, float(F.SEA_OFF)), (0.2, 0.0, 0.5, 0.25, 0.3)]


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], np.asarray(want)[bad][0])


f32 = np.float32
ITS = 7  # exchange_every 2 -> blocks 2 2 2 1, exchange_every 4 -> blocks 4 3
MAPS = ("rainMap", "hardness", "upliftMap")
# (grid, world, exchange_every).  70 rows over 8 and 16 ranks are stripes of 8-9 and 4-5 rows, thinner than the kernel's
# 16-row tile; a stripe has to hold the 2 * exchange_every ghost rows its neighbour asks for, which rules out 16 x 4 there
CASES = [((70, 333), w, e) for w in (2, 3, 8, 16) for e in (1, 2, 4) if 2 * e <= 70 // w]
CASES += [((333, 200), 3, 4), ((333, 200), 8, 1), ((333, 200), 16, 2)]
PARAM_SETS = (0, 1)  # the defaults; a sea level with fractional rain


def maps_for(shape, seed=11):
    rng = np.random.default_rng(seed)
    return {"rainMap": (rng.random(shape, dtype=f32) * f32(2.0)).astype(f32), "hardness": rng.random(shape, dtype=f32),
            "upliftMap": (rng.random(shape, dtype=f32) * f32(3.0)).astype(f32)}


def options(with_maps, shape):
    return maps_for(shape) if with_maps else {k: None for k in MAPS}


@functools.lru_cache(maxsize=None)
def reference(rows, cols, its, k, with_maps):
    """fluvial_ref.run on the whole grid, computed once per case and shared (the arrays are not to be modified)."""
    return F.run(terrain(rows, cols), its, **dict(zip(NAMES, PARAMS[k])), **options(with_maps, (rows, cols)))


def sharded_params(its, prm):
    return dict(iterations=its, **dict(zip(NAMES, prm)))


def stripe_bufs(plan, h, opts, exchange_every, device="cpu", pitch=None):
    """One rank's buffers for fluvial_steps, every float NaN except the owned rows of the input planes."""
    cols = plan.cols if pitch is None else pitch
    full = lambda *shape: torch.full(shape, float("nan"), device=device)  # noqa: E731
    own = slice(plan.g0, plan.g0 + plan.nown)

    def plane(a):
        t = full(plan.rows, cols)
        t[plan.own0:plan.own1, :plan.cols] = torch.from_numpy(np.ascontiguousarray(a[own])).to(device)
        return t

    bufs = dict(A=plane(h), B=full(plan.rows, cols), D0=full(plan.rows, cols), D1=full(plan.rows, cols),
                work=full(2, plan.rows, cols) if exchange_every > 1 else None)
    for name in MAPS:
        if opts.get(name) is not None:
            bufs[name] = plane(opts[name])
    return bufs


def gather(plans, results):
    """(heights, drainage) of the whole grid from every rank's owned rows."""
    rows = lambda t, pl: t[pl.own0:pl.own1, :pl.cols].cpu().numpy()  # noqa: E731
    return [np.concatenate([rows(r[i], pl) for r, pl in zip(results, plans)], axis=0) for i in range(2)]


def lockstep(sh, ops, world, exchange_every, h, its, prm, opts, device="cpu"):
    plans = [sh.StripePlan(r, world, h.shape[0], h.shape[1], sh.fluvial_halo_rows(exchange_every)) for r in range(world)]
    bufs = [stripe_bufs(pl, h, opts, exchange_every, device) for pl in plans]
    res = sh.run_fluvial_lockstep([ops] * world, plans, sharded_params(its, prm), bufs, copy_rows,
                                  exchange_every=exchange_every)
    return gather(plans, res)


def assert_run(got, want, what):
    for k, name in enumerate(("heights", "drainage")):
        assert np.isfinite(want[k]).all(), what
        assert_bits(got[k], want[k], "%s: %s" % (what, name))


def count_differing(got, want):
    return sum(int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum()) for k in range(2))
