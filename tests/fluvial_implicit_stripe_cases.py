"""Grids, buffers and drivers shared by tests/test_fluvial_implicit_stripe_ref.py (CPU) and
tests/test_gpu_fluvial_implicit_stripe.py: the filled grids of tests/drainage_stripe_cases.py, their drainage planes from
drainage_ref.accumulate and the planes fluvial_implicit_ref.walk gives for them -- computed once per case and shared, not to
be modified."""
import ctypes as C
import functools

import numpy as np
import torch

import fluvial_implicit_ref as R
from drainage_stripe_cases import OFF, WORLDS, assert_bits, filled, reference as drainage_reference, stripe_ops  # noqa: F401
from test_hydraulic_stripe_ref import copy_rows

f32 = np.float32
HALO = 2  # the drainage area's heights; the solve needs 1 row of the heights and of `out`
DT = 200.0
# A pass is at least one Jacobi step and a round at rest against final ghost rows ends the series, so rounds of 128 passes
# and 128 rounds cover every grid here: a Jacobi restatement of the schedule (tests/fluvial_implicit_stripe_ops.py, ghost
# rows from the heights in round 0 and from the exchanged h' afterwards) needs at most 95 steps in a round (the bowl over
# 2 stripes at dt 200) and 114 rounds (the filled serpentine over 16 stripes at dt 200), the final quiet round included.
PARAMS = dict(maxPasses=128, maxRounds=128)
MOST_ROUNDS, MOST_STEPS = 114, 95
# (grid, world, dt) of the stripes-equal-the-walk tests on both sides
CASES = ([(n, w, DT) for n in ("pitted", "bowl", "serpentine") for w in WORLDS] + [("wide", 16, DT)] +
         [("pitted", w, 1.0) for w in WORLDS])


@functools.lru_cache(maxsize=None)
def area(name, sea=OFF):
    return drainage_reference(name, 1.0, sea)[0]


@functools.lru_cache(maxsize=None)
def hard_map(shape):
    """A hardness map in [0, 0.9]."""
    return (f32(0.45) + f32(0.45) * np.sin(np.arange(shape[0] * shape[1], dtype=np.float64) * 0.37)).astype(f32).reshape(shape)


@functools.lru_cache(maxsize=None)
def uplift_map(shape):
    """An uplift map in [0, 2]."""
    return (f32(1.0) + np.cos(np.arange(shape[0] * shape[1], dtype=np.float64) * 0.11)).astype(f32).reshape(shape)


@functools.lru_cache(maxsize=None)
def reference(name, dt=DT, sea=OFF, mapped=False):
    """fluvial_implicit_ref.walk of the whole filled grid on its exact drainage plane."""
    h = filled(name)
    maps = dict(hardness=hard_map(h.shape), upliftMap=uplift_map(h.shape)) if mapped else {}
    return R.walk(h, area(name, sea), dt=dt, seaLevel=sea, **maps)


def stripe_bufs(plan, h, work_floats, drain_floats=0, device="cpu", pitch=None, A=None, **maps):
    """One rank's buffers for fluvial_implicit_steps, every float NaN except the owned rows of the heights, of A when
    given, and of the maps."""
    cols = plan.cols if pitch is None else pitch
    full = lambda *shape: torch.full(shape, float("nan"), device=device)  # noqa: E731
    own = slice(plan.g0, plan.g0 + plan.nown)

    def plane(a):
        t = full(plan.rows, cols)
        t[plan.own0:plan.own1, :plan.cols] = torch.from_numpy(np.ascontiguousarray(a[own])).to(device)
        return t

    bufs = dict(H=plane(h), out=full(plan.rows, cols), A=full(plan.rows, cols) if A is None else plane(A),
                work=full(max(work_floats, 1)), drainageWork=full(max(drain_floats, 1)),
                words=torch.full((3,), -7, dtype=torch.int32, device=device))
    for k, m in maps.items():
        if m is not None:
            bufs[k] = plane(m)
    return bufs


def lockstep(sh, ops, world, h, params, work_floats=lambda plan: 0, drain_floats=lambda plan: 0, device="cpu", **maps):
    """-> (heights, A, steps, rounds, converged, plans, bufs) of the whole grid through run_fluvial_implicit_lockstep."""
    plans = [sh.StripePlan(r, world, h.shape[0], h.shape[1], HALO) for r in range(world)]
    bufs = [stripe_bufs(pl, h, work_floats(pl), drain_floats(pl), device, **maps) for pl in plans]
    res = sh.run_fluvial_implicit_lockstep([ops] * world, plans, params, bufs, copy_rows)
    assert len({r[2:] for r in res}) == 1, "the ranks disagree about steps / rounds / converged"
    rows = lambda t, pl: t[pl.own0:pl.own1, :pl.cols].cpu().numpy()  # noqa: E731
    return (np.concatenate([rows(r[0], pl) for r, pl in zip(res, plans)]),
            np.concatenate([rows(r[1], pl) for r, pl in zip(res, plans)]), res[0][2], res[0][3], res[0][4], plans, bufs)


@functools.lru_cache(maxsize=None)
def cpu_rounds(name, world, dt):
    """(rounds of the solve, most Jacobi steps in one of its rounds) of the numpy restatement of the schedule."""
    from fluvial_implicit_stripe_ops import FluvialImplicitStripeOps
    from noize_job_amd import sharded as sh
    ops = FluvialImplicitStripeOps()
    got, _, steps, rounds, converged, _, _ = lockstep(sh, ops, world, filled(name), dict(PARAMS, dt=dt))
    assert converged and steps == 1
    assert_bits(got, reference(name, dt), "%s world %d dt %g on the CPU" % (name, world, dt))
    return rounds, max(ops.solve_steps)


def work_floats(nj, pitch=0):
    return lambda plan: nj._native.lib.nz_implicit_fluvial_stripe_work_floats(C.byref(plan.stripe(pitch)))


def drain_floats(nj, pitch=0):
    return lambda plan: nj._native.lib.nz_drainage_stripe_work_floats(C.byref(plan.stripe(pitch)))
