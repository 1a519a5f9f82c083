"""Grids, buffers and drivers shared by tests/test_drainage_stripe_ref.py (CPU) and tests/test_gpu_drainage_stripe.py: the
grids of tests/fill_stripe_cases.py, each filled with fill_ref.flood so that every river reaches the border, and the
drainage planes drainage_ref.accumulate gives for them -- computed once per case and shared, not to be modified."""
import ctypes as C
import functools

import numpy as np
import torch

import drainage_ref as D
import fill_ref as L
from fill_stripe_cases import EPS, WORLDS, assert_bits, grid, stripe_ops  # noqa: F401  (re-exported to the tests)
from test_hydraulic_stripe_ref import copy_rows

f32 = np.float32
OFF = float(D.SEA_OFF)
HALO = 2  # the heights; A and the rain map need 1
# A pass is at least one Jacobi step and a round at rest against final ghost rows ends the series, so rounds of 128
# passes and 128 rounds cover every grid here: a Jacobi restatement of the schedule needs at most 95 steps in a round and
# 114 rounds (the filled serpentine over 16 stripes), the final quiet round included.
PARAMS = dict(maxPasses=128, maxRounds=128)


@functools.lru_cache(maxsize=None)
def filled(name):
    return L.flood(grid(name), EPS)


@functools.lru_cache(maxsize=None)
def signed_rain(shape):
    """A rain map with both signs: sin of the cell index."""
    return np.sin(np.arange(shape[0] * shape[1], dtype=np.float64)).astype(f32).reshape(shape)


@functools.lru_cache(maxsize=None)
def reference(name, rain=1.0, sea=OFF, mapped=False):
    """(A, cells of the longest flow path) of the whole filled grid."""
    h = filled(name)
    return D.accumulate(h, rain, sea, signed_rain(h.shape) if mapped else None)


def stripe_bufs(plan, h, work_floats, device="cpu", pitch=None, rain_map=None):
    """One rank's buffers for drainage_steps, every float NaN except the owned rows of the heights and of the rain map."""
    cols = plan.cols if pitch is None else pitch
    full = lambda *shape: torch.full(shape, float("nan"), device=device)  # noqa: E731
    own = slice(plan.g0, plan.g0 + plan.nown)

    def plane(a):
        t = full(plan.rows, cols)
        t[plan.own0:plan.own1, :plan.cols] = torch.from_numpy(np.ascontiguousarray(a[own])).to(device)
        return t

    bufs = dict(H=plane(h), A=full(plan.rows, cols), work=full(max(work_floats, 1)),
                words=torch.full((3,), -7, dtype=torch.int32, device=device))
    if rain_map is not None:
        bufs["rainMap"] = plane(rain_map)
    return bufs


def lockstep(sh, ops, world, h, params, work_floats=lambda plan: 0, device="cpu", rain_map=None):
    """-> (A, rounds, converged, plans, bufs) of the whole grid through run_drainage_lockstep."""
    plans = [sh.StripePlan(r, world, h.shape[0], h.shape[1], HALO) for r in range(world)]
    bufs = [stripe_bufs(pl, h, work_floats(pl), device, rain_map=rain_map) for pl in plans]
    res = sh.run_drainage_lockstep([ops] * world, plans, params, bufs, copy_rows)
    assert len({(r[1], r[2]) for r in res}) == 1, "the ranks disagree about rounds / converged"
    A = np.concatenate([r[0][pl.own0:pl.own1, :pl.cols].cpu().numpy() for r, pl in zip(res, plans)])
    return A, res[0][1], res[0][2], plans, bufs


def work_floats(nj, pitch=0):
    return lambda plan: nj._native.lib.nz_drainage_stripe_work_floats(C.byref(plan.stripe(pitch)))
