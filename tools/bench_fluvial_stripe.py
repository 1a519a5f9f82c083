#!/usr/bin/env python3
"""Fluvial erosion and depression filling on row stripes (nz_fluvial_stripe, nz_fill_stripe), tools/bench_fluvial.py's protocol: HIP events, --warmup samples,
median [min, max] of --reps samples, the variants alternating in one process.
  1. The window form against the tile form: one stripe covering a 4096^2 grid beside nz_fluvial_erosion on the same tile,
     per iteration (one call of --iters iterations each).  The bar: the stripe's median lies no further above the tile
     entry's median than the tile entry's own [min, max] spread in this process.
  2. Recomputed ghost rows: rank 3's stripe of an 8-way split of 16384^2 (2048 owned rows; the ghost rows are filled once,
     the exchange itself is not rehearsed) in blocks of exchange_every = 1, 2, 4, 8 iterations, time per iteration beside
     the arithmetic share of recomputed rows per side: 2 * (k - 1) / 2048 in a block's first launch, (k - 1) / 2048 on average.
  3. Depression filling: the 4096^2 tile of tools/bench_fill.py through nz_fill_depressions (default budget), as 1 stripe and
     as 8 stripes rehearsed on one GPU through run_fill_lockstep (rounds of at most --passes passes, the vote taken in
     process and read back after every round, which the time includes): rounds, the passes that did work in every round
     (the largest over the stripes; from an untimed run that reads the status word after every call) and the total time.
usage: bench_fluvial_stripe.py [--iters 16] [--reps 7] [--warmup 3] [--big 16384] [--passes 64] [--skip-fluvial]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402
from noize_job_amd import sharded as sh  # noqa: E402

FLUVIAL = (0.05, 0.002, 1.0, 1.0, nj.FluvialErosionStage.SEA_OFF)  # erodibility, uplift, dt, rain, seaLevel


def measure(ctx, variants, reset, iters, warmup, reps):
    def sample(fn):
        reset()
        h0 = ctx.record()
        fn()
        h1 = ctx.record()
        h1.Complete()
        return ctx.elapsed_ms(h0, h1) / iters

    for _ in range(warmup):
        for _, fn in variants:
            sample(fn)
    ms = [[] for _ in variants]
    for _ in range(reps):
        for k, (_, fn) in enumerate(variants):
            ms[k].append(sample(fn))
    return ms


def fill_section(a):
    """3. the 4096^2 tile: nz_fill_depressions, 1 stripe, 8 lockstep stripes; torch CUDA tensors as plain HBM allocations on
    a context that shares torch's stream, torch's (HIP) events around every sample."""
    import torch
    N = nj._native
    res, eps = 4096, 1e-4
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = nj.Context(0, stream=stream.cuda_stream)
        ops = sh.HipStripeOps(ctx)
        start = torch.empty((res, res), device="cuda")
        ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), start.data_ptr(), res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700, handle=False)
        tile = torch.empty_like(start)
        work_t = torch.empty(N.lib.nz_fill_depressions_work_floats(res, 1), device="cuda")
        desc = N.FillDesc(eps, nj.FluvialErosionStage.SEA_OFF, 64 + res // 4, None)
        prm = dict(epsilon=eps, maxPasses=a.passes, maxRounds=100000)

        def copy_rows(dst, d0, src, s0, n):
            dst[d0:d0 + n].copy_(src[s0:s0 + n])

        def make(world):
            plans = [sh.StripePlan(r, world, res, res, 1) for r in range(world)]
            bufs = []
            for pl in plans:
                st = pl.stripe()
                bufs.append(dict(H=torch.empty((pl.rows, res), device="cuda"), W=torch.empty((pl.rows, res), device="cuda"),
                                 work=torch.empty(N.lib.nz_fill_stripe_work_floats(C.byref(st)), device="cuda"),
                                 words=torch.zeros(3, dtype=torch.int32, device="cuda")))
            return plans, bufs

        def reset_stripes(plans, bufs):
            for pl, b in zip(plans, bufs):
                b["H"][pl.own0:pl.own1].copy_(start[pl.g0:pl.g0 + pl.nown])

        class Counting:  # HipStripeOps that reads the status word "passes that did work" after every round
            def __init__(self):
                self.passes = []

            def fill(self, h, w, work, plan, *rest):
                ops.fill(h, w, work, plan, *rest)
                self.passes.append((plan.rank, int(work[0:1].view(torch.int32)[0])))

            def fill_finalise(self, *args):
                ops.fill_finalise(*args)

        sets = {w: make(w) for w in (1, 8)}
        results = {}

        def tile_entry():
            ctx.call("nz_fill_depressions", tile.data_ptr(), work_t.data_ptr(), C.byref(desc), res, handle=False)

        def stripes(world, the_ops=None):
            plans, bufs = sets[world]
            results[world] = sh.run_fill_lockstep([the_ops or ops] * world, plans, prm, bufs, copy_rows)

        variants = [("nz_fill_depressions", lambda: tile.copy_(start), tile_entry),
                    ("1 stripe", lambda: reset_stripes(*sets[1]), lambda: stripes(1)),
                    ("8 stripes", lambda: reset_stripes(*sets[8]), lambda: stripes(8))]

        def sample(reset, fn):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(a.warmup):
            for _, reset, fn in variants:
                sample(reset, fn)
        ms = [[] for _ in variants]
        for _ in range(a.reps):
            for k, (_, reset, fn) in enumerate(variants):
                ms[k].append(sample(reset, fn))
        status = work_t[0:2].view(torch.int32).tolist()
        print("depression filling, %d^2, %d samples, variants alternating; a round is at most %d passes" % (res, a.reps, a.passes))
        print("  %-20s %.3f ms  [%.3f, %.3f]  passes %d, converged %d" %
              (variants[0][0], float(np.median(ms[0])), min(ms[0]), max(ms[0]), status[0], status[1]), flush=True)
        for k, world in ((1, 1), (2, 8)):
            counting = Counting()
            reset_stripes(*sets[world])
            stripes(world, counting)
            rounds, converged = results[world][0][2], results[world][0][3]
            per_round = [max(p for _, p in counting.passes[r * world:(r + 1) * world]) for r in range(rounds)]
            same = all(torch.equal(b["H"][pl.own0:pl.own1], tile[pl.g0:pl.g0 + pl.nown]) for pl, b in zip(*sets[world]))
            print("  %-20s %.3f ms  [%.3f, %.3f]  x%.2f of the tile entry; rounds %d, converged %s, equal to the tile entry's bits %s"
                  % (variants[k][0], float(np.median(ms[k])), min(ms[k]), max(ms[k]),
                     float(np.median(ms[k])) / float(np.median(ms[0])), rounds, converged, same))
            print("    passes that did work, per round (largest over the stripes): %s" % per_round, flush=True)
        stream.synchronize()
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big", type=int, default=16384)
    ap.add_argument("--passes", type=int, default=64)
    ap.add_argument("--skip-fluvial", action="store_true")
    a = ap.parse_args()
    iters = a.iters + (a.iters & 1)
    N = nj._native
    fill_section(a)
    if a.skip_fluvial:
        return
    with nj.Context(0) as ctx:
        # ---- 1. one stripe over a 4096^2 grid against the tile entry ----
        res = 4096
        n = res * res
        start, d, out_h, out_a = (ctx.alloc(n) for _ in range(4))
        ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), start.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700)
        st = N.Stripe(res, res, 0, res, 0, res, 0)
        work_t = ctx.alloc(N.lib.nz_fluvial_erosion_work_floats(res, 1))
        work_s = ctx.alloc(N.lib.nz_fluvial_stripe_work_floats(C.byref(st), iters))
        desc = N.FluvialDesc(iters, *FLUVIAL, None, None, None, None)

        def reset():  # every sample starts from the same terrain (outside the timed window)
            ctx.call("nz_flush_write_slice", d.ptr, start.ptr, n, handle=False)

        def tile():
            ctx.call("nz_fluvial_erosion", d.ptr, work_t.ptr, C.byref(desc), res, handle=False)

        def stripe():
            ctx.call("nz_fluvial_stripe", d.ptr, out_h.ptr, out_a.ptr, work_s.ptr, C.byref(st), C.byref(desc), handle=False)

        variants = [("tile entry", tile), ("one stripe", stripe)]
        ms = measure(ctx, variants, reset, iters, a.warmup, a.reps)
        med = [float(np.median(m)) for m in ms]
        print("%d^2, %d samples of %d iterations, variants alternating" % (res, a.reps, iters))
        for (name, _), m, md in zip(variants, ms, med):
            print("  %-11s %.4f ms/iteration  [%.4f, %.4f]" % (name, md, min(m), max(m)), flush=True)
        spread = max(ms[0]) - min(ms[0])
        print("  bar: stripe - tile = %+.4f ms against the tile entry's spread %.4f ms: %s" %
              (med[1] - med[0], spread, "met" if med[1] - med[0] <= spread else "MISSED"), flush=True)
        for t in (start, d, out_h, out_a, work_t, work_s):
            t.Dispose()

        # ---- 2. one rank's stripe of an 8-way split, blocks of exchange_every iterations ----
        big, world, rank, top = a.big, 8, 3, 8
        plan = sh.StripePlan(rank, world, big, big, sh.fluvial_halo_rows(top))
        st = plan.stripe()
        cells = plan.rows * big
        h0, hA, hB, d0, d1 = (ctx.alloc(cells) for _ in range(5))
        work = ctx.alloc(N.lib.nz_fluvial_stripe_work_floats(C.byref(st), top))
        ctx.call("nz_fractal_stripe", int(nj.FractalNoise.Simplex), h0.ptr,
                 C.byref(N.Stripe(big, plan.rows, plan.grow0, big, 0, plan.rows, 0)), 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700)

        def reset_big():
            ctx.call("nz_flush_write_slice", hA.ptr, h0.ptr, cells, handle=False)

        def blocks_of(k):
            def run():
                cur, nxt, a_cur, a_nxt = hA, hB, None, d0
                for nb in sh.split_iterations(iters, k):
                    dsc = N.FluvialDesc(nb, *FLUVIAL, None, None, None, a_cur.ptr if a_cur is not None else None)
                    ctx.call("nz_fluvial_stripe", cur.ptr, nxt.ptr, a_nxt.ptr, work.ptr, C.byref(st), C.byref(dsc),
                             handle=False)
                    cur, nxt = nxt, cur
                    a_cur, a_nxt = a_nxt, (d1 if a_nxt is d0 else d0)
            return run

        ks = (1, 2, 4, 8)
        variants = [("every %d" % k, blocks_of(k)) for k in ks]
        ms = measure(ctx, variants, reset_big, iters, a.warmup, a.reps)
        med = [float(np.median(m)) for m in ms]
        print("rank %d of %d of %d^2 (%d owned rows), %d samples of %d iterations, variants alternating" %
              (rank, world, big, plan.nown, a.reps, iters))
        for k, (name, _), m, md in zip(ks, variants, ms, med):
            print("  %-8s %.4f ms/iteration  [%.4f, %.4f]  x%.4f of every 1   recomputed rows per side: first launch %.4f, "
                  "mean over the block %.4f" % (name, md, min(m), max(m), md / med[0], 2.0 * (k - 1) / plan.nown,
                                                (k - 1.0) / plan.nown), flush=True)
        for t in (h0, hA, hB, d0, d1, work):
            t.Dispose()


if __name__ == "__main__":
    main()
