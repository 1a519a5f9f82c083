#!/usr/bin/env python3
"""Depression filling (nz_fill_depressions): HIP-event time of one call to convergence at 1024^2 and 4096^2 on a simplex
fBm tile with the stage's defaults (epsilon 1e-4, no sea, 64 + resolution / 4 passes), beside the only other way to a
pit-free tile, N iterations of the fluvial stage at its defaults, and beside the constant job, all in one process with the
variants alternating.  N is found first: the fluvial stage runs in calls of --probe iterations, each continuing the drainage
of the one before, and the pits (cells that are no outlet and have no strictly lower neighbour) are counted on the host
after every call, until there are none or --limit iterations are reached.  A sample times one call between two events,
after --warmup such samples; reported as median [min, max] of --reps samples.  Also: the passes used, the filled cells, the
cost of an exhausted pass (the default budget against a budget of exactly the passes used), and the fill under other sweep
caps (nz_debug_fill_sweeps), each with a budget of exactly the passes it needs.  The bar, stated per size: the fill to
convergence takes no longer than the N fluvial iterations.
usage: bench_fill.py [--sizes 1024,4096] [--reps 7] [--warmup 3] [--probe 50] [--limit 5000] [--sweeps 4,8,16,32,64]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402

SEA_OFF = nj.FluvialErosionStage.SEA_OFF
FLUVIAL = (0.05, 0.002, 1.0, 1.0, SEA_OFF)  # erodibility, uplift, dt, rain, seaLevel
EPSILON = 1e-4


def pits(h):
    """Inner cells without a strictly lower neighbour (the count of fluvial_ref.pits without a sea)."""
    c = h[1:-1, 1:-1]
    low = np.full(c.shape, np.inf, np.float32)
    for dz in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dz, dx) != (1, 1):
                np.minimum(low, h[dz:dz + c.shape[0], dx:dx + c.shape[1]], out=low)
    return int((low >= c).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--probe", type=int, default=50)
    ap.add_argument("--limit", type=int, default=5000)
    ap.add_argument("--sweeps", default="4,8,16,32,64")
    a = ap.parse_args()
    N = nj._native
    with nj.Context(0) as ctx:
        for res in (int(s) for s in a.sizes.split(",")):
            n = res * res
            start = ctx.alloc(n)
            ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), start.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700)
            d, const, carry, depth = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
            work_f = ctx.alloc(N.lib.nz_fluvial_erosion_work_floats(res, 1))
            work = ctx.alloc(N.lib.nz_fill_depressions_work_floats(res, 1))
            budget = 64 + res // 4

            def reset():  # every sample starts from the same terrain (outside the timed window)
                ctx.call("nz_flush_write_slice", d.ptr, start.ptr, n, handle=False)

            def status():
                ctx.synchronize()
                return [int(v) for v in ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()]

            def fill(passes=budget, dp=None):
                desc = N.FillDesc(EPSILON, SEA_OFF, passes, dp.ptr if dp is not None else None)
                ctx.call("nz_fill_depressions", d.ptr, work.ptr, C.byref(desc), res, handle=False)

            # ---- N: fluvial iterations until no pit is left ----
            before = pits(start.ToArray((res, res)))
            reset()
            done, left = 0, before
            while left and done < a.limit:
                desc = N.FluvialDesc(a.probe, *FLUVIAL, None, None, None, carry.ptr if done else None)
                ctx.call("nz_fluvial_erosion", d.ptr, work_f.ptr, C.byref(desc), res, handle=False)
                ctx.call("nz_flush_write_slice", carry.ptr, work_f.ptr, n, handle=False)
                done += a.probe
                left = pits(d.ToArray((res, res)))
            print("%d^2: %d pits at the start; the fluvial stage at its defaults, probed every %d iterations: %s" %
                  (res, before, a.probe, "none left after N = %d" % done if not left else
                   "%d left after %d iterations, the limit -- N is larger; the bar below uses %d" % (left, done, done)), flush=True)
            n_its = max(done, 1)

            # ---- the fill once, untimed: passes, filled cells, no pits ----
            reset()
            fill(dp=depth)
            used, converged = status()
            dh = depth.ToArray()
            print("  fill: converged %d after %d passes of a budget of %d; %d cells filled (%.2f%%), deepest %.4g; %d pits left" %
                  (converged, used, budget, int((dh > 0).sum()), 100.0 * float((dh > 0).mean()), float(dh.max()),
                   pits(d.ToArray((res, res)))), flush=True)

            fdesc = N.FluvialDesc(n_its, *FLUVIAL, None, None, None, None)
            variants = [("fill, default budget", lambda: fill()),
                        ("fill, budget = passes used", lambda: fill(used)),
                        ("fluvial x N", lambda: ctx.call("nz_fluvial_erosion", d.ptr, work_f.ptr, C.byref(fdesc), res, handle=False)),
                        ("constant job", lambda: ctx.call("nz_constant_job", 0, const.ptr, None, 1.0, res, handle=False))]

            def sample(fn):
                reset()
                h0 = ctx.record()
                fn()
                h1 = ctx.record()
                h1.Complete()
                return ctx.elapsed_ms(h0, h1)

            def measure(vs):
                for _ in range(a.warmup):
                    for _, fn in vs:
                        sample(fn)
                ms = [[] for _ in vs]
                for _ in range(a.reps):
                    for k, (_, fn) in enumerate(vs):
                        ms[k].append(sample(fn))
                return ms

            ms = measure(variants)
            med = [float(np.median(m)) for m in ms]
            print("  %d samples, variants alternating" % a.reps)
            for (name, _), m, md in zip(variants, ms, med):
                print("  %-27s %9.4f ms  [%.4f, %.4f]  x%.1f of the constant job" % (name, md, min(m), max(m), md / med[3]))
            print("  fluvial per iteration       %9.4f ms (N = %d)" % (med[2] / n_its, n_its))
            if budget > used:
                print("  an exhausted pass           %9.4f ms ((default budget - exact budget) / %d launches)" %
                      ((med[0] - med[1]) / (budget - used), budget - used))
            print("  bar: fill to convergence %.4f ms [max %.4f] <= %d fluvial iterations %.4f ms [min %.4f]: %s, x%.1f below" %
                  (med[0], max(ms[0]), n_its, med[2], min(ms[2]), "met" if max(ms[0]) <= min(ms[2]) else
                   ("met at the medians" if med[0] <= med[2] else "MISSED"), med[2] / med[0]), flush=True)

            # ---- the sweep cap: the passes each cap needs first, then timed with exactly that budget ----
            caps = [int(s) for s in a.sweeps.split(",") if s]
            if caps:
                try:
                    need = []
                    for cap in caps:
                        N.lib.nz_debug_fill_sweeps(cap)
                        reset()
                        fill(16 * budget)
                        need.append(status())

                    def capped(cap, passes):
                        def run():
                            N.lib.nz_debug_fill_sweeps(cap)
                            fill(passes)
                        return run
                    cms = measure([("", capped(c, p)) for c, (p, _) in zip(caps, need)])
                    for cap, (p, conv), m in zip(caps, need, cms):
                        print("  sweeps <= %-3d  %9.4f ms  [%.4f, %.4f]  %4d passes, converged %d" %
                              (cap, float(np.median(m)), min(m), max(m), p, conv), flush=True)
                finally:
                    N.lib.nz_debug_fill_sweeps(0)
            for t in (start, d, const, carry, depth, work_f, work):
                t.Dispose()


if __name__ == "__main__":
    main()
