#!/usr/bin/env python3
"""The drainage area on row stripes (nz_drainage_stripe_round), tools/bench_fluvial_stripe.py's protocol: torch's HIP events
around every sample, --warmup samples, median [min, max] of --reps samples, the variants alternating in one process.
  1. The filled 13-octave fBm tile of tools/bench_drainage.py at 4096^2 through
       nz_drainage_area with the hosts' default budget                                   -- the yardstick
       one stripe: a single round with that budget plus finalise, nothing read back      -- the window form of the kernels
       one stripe through run_drainage_lockstep (a second round at rest, two votes read back)
       8 stripes rehearsed on one GPU through run_drainage_lockstep, rounds of at most --passes passes, the vote taken in
       process and read back after every round, which the time includes
     with rounds and the passes that did work in every round (the largest over the stripes; from an untimed run that
     reads the status word after every call).  The bar for "one stripe": equal passes, and a median no further above the
     tile entry's than the tile entry's own [min, max] spread in this process.
  2. The chain fill -> drainage -> fluvial(drainageIn), --iters iterations in blocks of --every: the three tile entries
     beside 8 lockstep stripes, bits compared.
usage: bench_drainage_stripe.py [--res 4096] [--reps 7] [--warmup 3] [--passes 64] [--iters 16] [--every 4] [--skip-chain]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402
from noize_job_amd import sharded as sh  # noqa: E402

OFF = nj.FluvialErosionStage.SEA_OFF
EPS = 1e-4
FLUVIAL = (0.05, 0.002, 1.0, 1.0, OFF)  # erodibility, uplift, dt, rain, seaLevel


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=64)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--skip-chain", action="store_true")
    a = ap.parse_args()
    N = nj._native
    res, budget, world = a.res, 64 + a.res // 4, 8
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = nj.Context(0, stream=stream.cuda_stream)
        ops = sh.HipStripeOps(ctx)
        dev = lambda *shape: torch.empty(shape, device="cuda")  # noqa: E731
        words = lambda: torch.zeros(3, dtype=torch.int32, device="cuda")  # noqa: E731
        sized = lambda entry, pl: dev(getattr(N.lib, entry)(C.byref(pl.stripe())))  # noqa: E731
        raw, filled, area = dev(res, res), dev(res, res), dev(res, res)
        ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), raw.data_ptr(), res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700, handle=False)
        work_fill = dev(N.lib.nz_fill_depressions_work_floats(res, 1))
        work_area = dev(N.lib.nz_drainage_area_work_floats(res, 1))
        fill_desc = N.FillDesc(EPS, OFF, budget, None)
        area_desc = N.DrainageDesc(1.0, OFF, budget, None)
        filled.copy_(raw)
        ctx.call("nz_fill_depressions", filled.data_ptr(), work_fill.data_ptr(), C.byref(fill_desc), res, handle=False)

        def copy_rows(dst, d0, src, s0, n):
            dst[d0:d0 + n].copy_(src[s0:s0 + n])

        def sample(reset, fn):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def measure(variants):
            for _ in range(a.warmup):
                for _, reset, fn in variants:
                    sample(reset, fn)
            ms = [[] for _ in variants]
            for _ in range(a.reps):
                for k, (_, reset, fn) in enumerate(variants):
                    ms[k].append(sample(reset, fn))
            return ms

        def line(name, m, base=None):
            md = float(np.median(m))
            return "  %-34s %8.3f ms  [%.3f, %.3f]%s" % (name, md, min(m), max(m), "" if base is None else "  x%.3f" % (md / base))

        class Counting:  # HipStripeOps that reads the status word "passes that did work" after every round
            def __init__(self):
                self.passes = []

            def drainage(self, h, a_, work, plan, *rest, **kw):
                ops.drainage(h, a_, work, plan, *rest, **kw)
                self.passes.append(int(work[0:1].view(torch.int32)[0]))

            def drainage_finalise(self, *args, **kw):
                ops.drainage_finalise(*args, **kw)

        # ---- 1. the drainage area of the filled tile ----
        def make(n, halo, source):
            plans = [sh.StripePlan(r, n, res, res, halo) for r in range(n)]
            bufs = []
            for pl in plans:
                b = dict(H=dev(pl.rows, res), A=dev(pl.rows, res), work=sized("nz_drainage_stripe_work_floats", pl), words=words())
                b["H"][pl.own0:pl.own1].copy_(source[pl.g0:pl.g0 + pl.nown])
                bufs.append(b)
            return plans, bufs

        sets = {1: make(1, 2, filled), world: make(world, 2, filled)}
        results = {}

        def tile_entry():
            ctx.call("nz_drainage_area", filled.data_ptr(), area.data_ptr(), work_area.data_ptr(), C.byref(area_desc), res, handle=False)

        def one_round():
            (pl,), (b,) = sets[1]
            prm = dict(sh.DRAINAGE_DEFAULTS, maxPasses=budget)
            ops.drainage(b["H"], b["A"], b["work"], pl, prm, True, None, b["words"][0:1])
            ops.drainage_finalise(b["A"], pl, prm, b["words"][2:3])

        def stripes(n, passes, the_ops=None):
            plans, bufs = sets[n]
            results[n] = sh.run_drainage_lockstep([the_ops or ops] * n, plans, dict(maxPasses=passes, maxRounds=100000), bufs, copy_rows)

        nothing = lambda: None  # noqa: E731  (the heights are read only: no sample has anything to put back)
        sets[1][1][0]["words"][2:3].fill_(1)
        variants = [("nz_drainage_area", nothing, tile_entry),
                    ("1 stripe, one round + finalise", nothing, one_round),
                    ("1 stripe, run_drainage_lockstep", nothing, lambda: stripes(1, budget)),
                    ("%d stripes, run_drainage_lockstep" % world, nothing, lambda: stripes(world, a.passes))]
        ms = measure(variants)
        status = work_area[0:2].view(torch.int32).tolist()
        base = float(np.median(ms[0]))
        print("drainage area of the filled 13-octave fBm tile, %d^2, %d samples, variants alternating" % (res, a.reps))
        print(line(variants[0][0], ms[0]) + "  passes %d, converged %d" % (status[0], status[1]), flush=True)
        one_round()
        (pl1,), (b1,) = sets[1]
        print(line(variants[1][0], ms[1], base) + "  passes %d, equal to the tile entry's bits %s" %
              (int(b1["work"][0:1].view(torch.int32)[0]), torch.equal(b1["A"][pl1.own0:pl1.own1], area)))
        spread = max(ms[0]) - min(ms[0])
        diff = float(np.median(ms[1])) - base
        print("    bar: one round - tile entry = %+.3f ms against the tile entry's spread %.3f ms: %s" %
              (diff, spread, "met" if diff <= spread else "MISSED"), flush=True)
        for k, (n, passes) in ((2, (1, budget)), (3, (world, a.passes))):
            counting = Counting()
            stripes(n, passes, counting)
            rounds, converged = results[n][0][1], results[n][0][2]
            per_round = [max(counting.passes[r * n:(r + 1) * n]) for r in range(rounds)]
            same = all(torch.equal(b["A"][pl.own0:pl.own1], area[pl.g0:pl.g0 + pl.nown]) for pl, b in zip(*sets[n]))
            print(line(variants[k][0], ms[k], base) + "  rounds %d of at most %d passes, converged %s, equal to the tile entry's bits %s"
                  % (rounds, passes, converged, same))
            print("    passes that did work, per round (largest over the stripes): %s" % per_round, flush=True)
        sets.clear()

        # ---- 2. the chain ----
        if not a.skip_chain:
            its, every = a.iters, a.every
            tile_h, work_flu = dev(res, res), dev(N.lib.nz_fluvial_erosion_work_floats(res, 1))
            flu_desc = N.FluvialDesc(its, *FLUVIAL, None, None, None, area.data_ptr())

            def tile_chain():
                ctx.call("nz_fill_depressions", tile_h.data_ptr(), work_fill.data_ptr(), C.byref(fill_desc), res, handle=False)
                ctx.call("nz_drainage_area", tile_h.data_ptr(), area.data_ptr(), work_area.data_ptr(), C.byref(area_desc), res, handle=False)
                ctx.call("nz_fluvial_erosion", tile_h.data_ptr(), work_flu.data_ptr(), C.byref(flu_desc), res, handle=False)

            plans = [sh.StripePlan(r, world, res, res, sh.fluvial_halo_rows(every)) for r in range(world)]
            plane = lambda pl: dev(pl.rows, res)  # noqa: E731
            H = [plane(pl) for pl in plans]
            fill_bufs = [dict(H=t, W=plane(pl), work=sized("nz_fill_stripe_work_floats", pl), words=words()) for t, pl in zip(H, plans)]
            area_bufs = [dict(H=t, A=plane(pl), work=sized("nz_drainage_stripe_work_floats", pl), words=words()) for t, pl in zip(H, plans)]
            flu_bufs = [dict(A=t, B=plane(pl), D0=plane(pl), D1=plane(pl), work=dev(2, pl.rows, res), drainageIn=b["A"])
                        for t, b, pl in zip(H, area_bufs, plans)]
            out = {}

            def reset_stripes():
                for t, pl in zip(H, plans):
                    t[pl.own0:pl.own1].copy_(raw[pl.g0:pl.g0 + pl.nown])

            def stripe_chain():
                rounds = dict(maxPasses=a.passes, maxRounds=100000)
                out["fill"] = sh.run_fill_lockstep([ops] * world, plans, dict(rounds, epsilon=EPS), fill_bufs, copy_rows)
                out["area"] = sh.run_drainage_lockstep([ops] * world, plans, rounds, area_bufs, copy_rows)
                out["flu"] = sh.run_fluvial_lockstep([ops] * world, plans, dict(iterations=its), flu_bufs, copy_rows, exchange_every=every)

            variants = [("tile chain", lambda: tile_h.copy_(raw), tile_chain), ("%d stripes, lockstep" % world, reset_stripes, stripe_chain)]
            ms = measure(variants)
            base = float(np.median(ms[0]))
            same = all(torch.equal(r[0][pl.own0:pl.own1], tile_h[pl.g0:pl.g0 + pl.nown]) and
                       torch.equal(r[1][pl.own0:pl.own1], work_flu[:res * res].view(res, res)[pl.g0:pl.g0 + pl.nown])
                       for r, pl in zip(out["flu"], plans))
            print("fill -> drainage -> fluvial(drainageIn), %d iterations in blocks of %d, %d^2, %d samples, variants alternating" %
                  (its, every, res, a.reps))
            print(line(variants[0][0], ms[0]))
            print(line(variants[1][0], ms[1], base) + "  fill rounds %d, drainage rounds %d, heights and drainage equal to the tile chain's bits %s"
                  % (out["fill"][0][2], out["area"][0][1], same), flush=True)
        stream.synchronize()
        ctx.close()


if __name__ == "__main__":
    main()
