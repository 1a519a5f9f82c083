#!/usr/bin/env python3
"""Grid hydraulic erosion on row stripes (nz_hydraulic_stripe): HIP-event time per iteration, the protocol of
tools/bench_hydraulic.py (each sample times --iters iterations between two events after --warmup such runs; median
[min, max] of --reps samples; simplex fBm heights, the stage's defaults).
  1. the whole 4096^2 grid as one stripe (one call, first and last set) against nz_hydraulic_erosion_stage, the two
     alternating sample by sample in one process;
  2. rank 3 of 8 of a 16384 x 16384 grid on one GPU without the exchange: the iterations in calls of k = 1, 2, 4 (what
     exchange_every = k launches), against the row model -- time proportional to the rows produced, the widened windows
     included: (2048 + 3 (k - 1)) / 2048 of the k = 1 figure on average.
usage: bench_hydraulic_stripe.py [--iters 200] [--reps 7] [--warmup 3] [--skip-rank]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402
from noize_job_amd import sharded as sh  # noqa: E402

N = nj._native
DEFAULTS = (1e-4, 1e-4, 0.01, 1.0, 0.3, 0.3, 0.01)  # initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt


def timed(ctx, call, iters):
    h0 = ctx.record()
    call()
    h1 = ctx.record()
    h1.Complete()
    return ctx.elapsed_ms(h0, h1) / iters


def report(name, ms):
    ms = np.array(ms)
    print("%-44s %.4f ms/iteration  [%.4f, %.4f] over %d samples" % (name, float(np.median(ms)), ms.min(), ms.max(), len(ms)),
          flush=True)
    return float(np.median(ms))


class StripeRun:
    """The planes of one stripe and `iters` iterations on them in calls of at most k (no exchange in between)."""

    def __init__(self, ctx, plan, k):
        self.ctx, self.plan, self.k = ctx, plan, k
        self.st = plan.stripe()
        n = plan.rows * plan.cols
        self.h = [ctx.alloc(n), ctx.alloc(n)]
        self.state = [[ctx.alloc(n) for _ in range(6)] for _ in range(2)]
        work = N.lib.nz_hydraulic_stripe_work_floats(C.byref(self.st), k)
        self.work = ctx.alloc(work) if work else None
        arr = N.dev_ptr * 6
        self.sets = [arr(*[t.ptr for t in s]) for s in self.state]
        # (the ghost rows of the state planes, which nobody exchanges here, hold whatever the allocation held: the kernel's
        # time does not depend on the values)
        whole = plan.widened(plan.halo, plan.halo).stripe()
        ctx.call("nz_fractal_stripe", int(nj.FractalNoise.Simplex), self.h[0].ptr, C.byref(whole), 0.4, 1.0, 2.0, 0.0, 13, 0, 0,
                 1700, handle=False)

    def run(self, iters):
        blocks = sh.split_iterations(iters, self.k)
        cur = 0
        for i, n in enumerate(blocks):
            desc = N.HydraulicDesc(n, *DEFAULTS, 0, None, None, None, None)
            first, last = i == 0, i == len(blocks) - 1
            self.ctx.call("nz_hydraulic_stripe", self.h[cur].ptr, self.h[cur ^ 1].ptr, None if first else self.sets[cur],
                          self.sets[cur ^ 1], self.work.ptr if self.work else None, C.byref(self.st), C.byref(desc), int(first),
                          int(last), handle=False)
            cur ^= 1
        if len(blocks) & 1:  # the next run starts from the plane that holds the heights
            self.h.reverse()

    def close(self):
        for t in self.h + self.state[0] + self.state[1] + ([self.work] if self.work else []):
            t.Dispose()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-rank", action="store_true")
    a = ap.parse_args()
    iters = a.iters + (a.iters & 1)
    with nj.Context(0) as ctx:
        # 1. the whole grid as one stripe against the tile entry
        res = 4096
        d = ctx.alloc(res * res)
        ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700)
        work = ctx.alloc(N.lib.nz_hydraulic_erosion_work_floats(res, 1))
        one = StripeRun(ctx, sh.StripePlan(0, 1, res, res, 0), iters)

        def tile():
            ctx.call("nz_hydraulic_erosion_stage", d.ptr, work.ptr, iters, *DEFAULTS, res, handle=False)

        for _ in range(a.warmup):
            tile()
            one.run(iters)
        ms = {"tile": [], "stripe": []}
        for _ in range(a.reps):
            ms["tile"].append(timed(ctx, tile, iters))
            ms["stripe"].append(timed(ctx, lambda: one.run(iters), iters))
        t = report("4096^2 nz_hydraulic_erosion_stage", ms["tile"])
        s = report("4096^2 as one stripe, one call", ms["stripe"])
        print("   one stripe / tile entry: %.4f" % (s / t), flush=True)
        one.close()
        d.Dispose()
        work.Dispose()
        if a.skip_rank:
            return
        # 2. one rank's stripe of the 16384^2 grid
        base = None
        for k in (1, 2, 4):
            plan = sh.StripePlan(3, 8, 16384, 16384, sh.hydraulic_halo_rows(k))
            r = StripeRun(ctx, plan, k)
            for _ in range(a.warmup):
                r.run(iters)
            med = report("rank 3 of 8 of 16384^2, calls of %d" % k, [timed(ctx, lambda: r.run(iters), iters) for _ in range(a.reps)])
            base = base or med
            print("   against k = 1: %.4f  row model: %.4f" % (med / base, (plan.nown + 3.0 * (k - 1)) / plan.nown), flush=True)
            r.close()


if __name__ == "__main__":
    main()
