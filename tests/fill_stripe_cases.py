"""Grids, buffers and drivers shared by tests/test_fill_stripe_ref.py (CPU) and tests/test_gpu_fill_stripe.py: a fBm corner
with pits, a bowl that spans three stripes, and a serpentine lake whose spill path crosses every cut many times."""
import contextlib
import ctypes as C
import functools

import numpy as np
import torch

import fill_ref as L
from test_hydraulic_stripe_ref import copy_rows, terrain

f32 = np.float32
WORLDS = (2, 3, 8, 16)
EPS = 1e-4


def pitted(rows, cols):
    rng = np.random.default_rng(3)
    return (terrain(rows, cols) + rng.standard_normal((rows, cols)).astype(f32) * f32(0.01)).astype(f32)


def bowl(rows, cols):
    """A ramp with one hollow from row 8 to row rows - 9: three stripes and more at every world above 2."""
    z, x = np.meshgrid(np.arange(rows, dtype=f32), np.arange(cols, dtype=f32), indexing="ij")
    h = f32(1.0) + x * f32(0.002) + z * f32(0.001)
    rz, rx = (z - f32(rows / 2)) / f32(rows / 2 - 8), (x - f32(cols / 2)) / f32(cols / 2 - 8)
    r2 = rz * rz + rx * rx
    return np.where(r2 < 1, h - (f32(1.0) - r2) * f32(0.8), h).astype(f32)


def serpentine(rows, cols, step=12):
    """A plateau with one channel from the top border that runs down and up the grid in legs `step` columns apart, its floor
    falling away from the mouth: a lake that fills from the mouth inward, along a path that crosses every cut once per leg."""
    h = np.full((rows, cols), f32(10.0), f32)
    path = [(z, 4) for z in range(0, rows - 4)]
    c, down = 4, True
    while c + step < cols - 4:
        zc = rows - 5 if down else 4
        path += [(zc, x) for x in range(c + 1, c + step + 1)]
        c, down = c + step, not down
        path += [(z, c) for z in (range(rows - 6, 3, -1) if not down else range(5, rows - 4))]
    for s, (z, x) in enumerate(path):
        h[z, x] = f32(0.6) - f32(s) * f32(0.0002)
    return h


GRIDS = {"pitted": lambda: pitted(70, 97), "bowl": lambda: bowl(70, 97), "serpentine": lambda: serpentine(70, 97),
         "wide": lambda: pitted(33, 130)}


@functools.lru_cache(maxsize=None)
def grid(name):
    return GRIDS[name]()


@functools.lru_cache(maxsize=None)
def flood(name, sea=float(L.SEA_OFF)):
    """fill_ref.flood on the whole grid, computed once per case and shared (not to be modified)."""
    return L.flood(grid(name), EPS, sea)


def stripe_bufs(plan, h, work_floats, device="cpu", pitch=None, depth=True):
    """One rank's buffers for fill_steps, every float NaN except the owned rows of the heights."""
    cols = plan.cols if pitch is None else pitch
    full = lambda *shape: torch.full(shape, float("nan"), device=device)  # noqa: E731
    H = full(plan.rows, cols)
    H[plan.own0:plan.own1, :plan.cols] = torch.from_numpy(np.ascontiguousarray(h[plan.g0:plan.g0 + plan.nown])).to(device)
    bufs = dict(H=H, W=full(plan.rows, cols), work=full(max(work_floats, 1)),
                words=torch.full((3,), -7, dtype=torch.int32, device=device))
    if depth:
        bufs["depth"] = full(plan.rows, cols)
    return bufs


def lockstep(sh, ops, world, h, params, work_floats=lambda plan: 0, device="cpu"):
    """-> (heights, depth, rounds, converged, plans, bufs) of the whole grid through run_fill_lockstep."""
    plans = [sh.StripePlan(r, world, h.shape[0], h.shape[1], 1) for r in range(world)]
    bufs = [stripe_bufs(pl, h, work_floats(pl), device) for pl in plans]
    res = sh.run_fill_lockstep([ops] * world, plans, params, bufs, copy_rows)
    rows = lambda t, pl: t[pl.own0:pl.own1, :pl.cols].cpu().numpy()  # noqa: E731
    assert len({(r[2], r[3]) for r in res}) == 1, "the ranks disagree about rounds / converged"
    return (np.concatenate([rows(r[0], pl) for r, pl in zip(res, plans)]),
            np.concatenate([rows(r[1], pl) for r, pl in zip(res, plans)]), res[0][2], res[0][3], plans, bufs)


@contextlib.contextmanager
def stripe_ops(nj):
    """(sharded module, HipStripeOps) on a context that shares torch's stream: the buffers are torch CUDA tensors."""
    from noize_job_amd import sharded as sh
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tctx = nj.Context(0, stream=stream.cuda_stream)
        try:
            yield sh, sh.HipStripeOps(tctx)
            stream.synchronize()
        finally:
            tctx.close()


def work_floats(nj, pitch=0):
    return lambda plan: nj._native.lib.nz_fill_stripe_work_floats(C.byref(plan.stripe(pitch)))


def assert_bits(got, want, what):
    bad = got.view(np.uint32) != np.ascontiguousarray(want, f32).view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], np.asarray(want)[bad][0])
