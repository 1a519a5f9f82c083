#!/usr/bin/env python3
"""Multiple-flow drainage (nz_drainage_mfd): HIP-event time of one call to convergence at 1024^2 and 4096^2 on the
project's usual tile -- 13-octave simplex fBm run through nz_fill_depressions at its defaults -- for exponents 1 and 4,
beside (a) nz_drainage_area on the same tile, the yardstick, and (b) the constant job as the byte-bound one; all in one
process with the variants alternating.  Every series is timed with a budget of exactly the passes it needs and, for the
stage's default budget, with the launches that return at once behind it.  Also: the passes used against the default
budget 128 + resolution / 2, the cost of the launches around the passes (a call with a budget of 1 and of 2: setup, one or
two passes, finalise; 2 * t1 - t2 estimates setup + finalise), and the stage under other sweep caps
(nz_debug_drainage_mfd_sweeps).  By bytes a live tile's pass moves 40 B per cell (eight weights, A in and out) against the
tree's 9 (a donor byte, A in and out), a factor of 4.4: the bar for the time ratio is 4.4 x (MFD passes / tree passes) x 1.5.
A sample times one call between two events, after --warmup such samples; reported as median [min, max] of --reps samples.
usage: bench_drainage_mfd.py [--sizes 1024,4096] [--exponents 1,4] [--reps 7] [--warmup 2] [--sweeps 4,8,16,32,64]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402

SEA_OFF = nj.DrainageAreaStage.SEA_OFF
RAIN = 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--exponents", default="1,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweeps", default="4,8,16,32,64")
    a = ap.parse_args()
    N = nj._native
    exponents = [int(s) for s in a.exponents.split(",")]
    with nj.Context(0) as ctx:
        for res in (int(s) for s in a.sizes.split(",")):
            n = res * res
            h = ctx.alloc(n)
            ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), h.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700)
            fwork = ctx.alloc(N.lib.nz_fill_depressions_work_floats(res, 1))
            fdesc = N.FillDesc(1e-4, SEA_OFF, 64 + res // 4, None)
            ctx.call("nz_fill_depressions", h.ptr, fwork.ptr, C.byref(fdesc), res, handle=False)
            ctx.synchronize()
            filled = int(ctx.wrap(fwork.ptr, 2, dtype=np.int32).ToArray()[1])
            fwork.Dispose()
            out, const = ctx.alloc(n), ctx.alloc(n)
            work = ctx.alloc(N.lib.nz_drainage_mfd_work_floats(res, 1))
            work_t = ctx.alloc(N.lib.nz_drainage_area_work_floats(res, 1))
            budget, budget_t = 128 + res // 2, 64 + res // 4  # MfdDrainageStage's and DrainageAreaStage's defaults

            def status(w):
                ctx.synchronize()
                return [int(v) for v in ctx.wrap(w.ptr, 2, dtype=np.int32).ToArray()]

            def mfd(exponent, passes):
                desc = N.DrainageMfdDesc(RAIN, SEA_OFF, passes, exponent, None)
                ctx.call("nz_drainage_mfd", h.ptr, out.ptr, work.ptr, C.byref(desc), res, handle=False)

            def tree(passes):
                desc = N.DrainageDesc(RAIN, SEA_OFF, passes, None)
                ctx.call("nz_drainage_area", h.ptr, out.ptr, work_t.ptr, C.byref(desc), res, handle=False)

            # ---- every series once, untimed, with a budget that cannot run out short of the plane's cell count ----
            tree(16 * budget)
            used_t, conv_t = status(work_t)
            print("%d^2 (fill converged %d): nz_drainage_area converged %d after %d passes (default budget %d)" %
                  (res, filled, conv_t, used_t, budget_t), flush=True)
            used, want = {}, {}
            for e in exponents:
                mfd(e, 16 * budget)
                used[e], conv = status(work)
                want[e] = out.ToArray().view(np.uint32)
                A = out.ToArray()
                print("  nz_drainage_mfd exponent %d: converged %d after %d passes (x%.2f of the tree's); the default budget is "
                      "%d (x%.1f of the passes used); largest area %.6g cells, finite %s" %
                      (e, conv, used[e], used[e] / max(used_t, 1), budget, budget / max(used[e], 1), float(A.max()),
                       bool(np.isfinite(A).all())), flush=True)
                if 2 * used[e] > budget:
                    print("  !! the passes used exceed half the default budget: raise the default to %d" % (2 * used[e]))

            variants = [("(a) nz_drainage_area, exact", lambda: tree(used_t)), ("(a) nz_drainage_area, default", lambda: tree(budget_t)),
                        ("(b) constant job", lambda: ctx.call("nz_constant_job", 0, const.ptr, None, 1.0, res, handle=False)),
                        ("(a) tree, budget 1", lambda: tree(1)), ("(a) tree, budget 2", lambda: tree(2))]
            for e in exponents:
                variants += [("mfd e=%d, exact budget" % e, lambda e=e: mfd(e, used[e])),
                             ("mfd e=%d, default budget" % e, lambda e=e: mfd(e, budget)),
                             ("mfd e=%d, budget 1" % e, lambda e=e: mfd(e, 1)), ("mfd e=%d, budget 2" % e, lambda e=e: mfd(e, 2))]

            def sample(fn):
                ctx.synchronize()
                h0 = ctx.record()
                fn()
                h1 = ctx.record()
                h1.Complete()
                return ctx.elapsed_ms(h0, h1)

            def measure(vs, reps):
                for _ in range(a.warmup):
                    for _, fn in vs:
                        sample(fn)
                ms = [[] for _ in vs]
                for _ in range(reps):
                    for k, (_, fn) in enumerate(vs):
                        ms[k].append(sample(fn))
                return ms

            ms = measure(variants, a.reps)
            med = {name: float(np.median(m)) for (name, _), m in zip(variants, ms)}
            print("  %d samples, variants alternating" % a.reps)
            for (name, _), m in zip(variants, ms):
                print("  %-31s %10.4f ms  [%.4f, %.4f]  x%.1f of the constant job" %
                      (name, med[name], min(m), max(m), med[name] / med["(b) constant job"]))
            t_tree = med["(a) nz_drainage_area, exact"]
            print("  tree: setup + finalise ~ %.4f ms (2 * budget 1 - budget 2); per pass %.4f ms" %
                  (2 * med["(a) tree, budget 1"] - med["(a) tree, budget 2"], t_tree / used_t))
            for e in exponents:
                t = med["mfd e=%d, exact budget" % e]
                around = 2 * med["mfd e=%d, budget 1" % e] - med["mfd e=%d, budget 2" % e]
                bar = 4.4 * used[e] / used_t * 1.5
                print("  mfd e=%d: setup + finalise ~ %.4f ms (2 * budget 1 - budget 2); per pass %.4f ms; x%.2f of the tree's "
                      "time, bar x%.2f (4.4 x %d / %d x 1.5): %s" %
                      (e, around, t / used[e], t / t_tree, bar, used[e], used_t, "within" if t / t_tree <= bar else "BEYOND"),
                      flush=True)

            # ---- the sweep cap: the passes each cap needs first, then timed with exactly that budget ----
            caps = [int(s) for s in a.sweeps.split(",") if s]
            if caps:
                e = exponents[0]
                try:
                    need = []
                    for cap in caps:
                        N.lib.nz_debug_drainage_mfd_sweeps(cap)
                        mfd(e, 64 * budget)
                        need.append(status(work))
                        assert np.array_equal(out.ToArray().view(np.uint32), want[e]) or not need[-1][1], cap

                    def capped(cap, passes):
                        def run():
                            N.lib.nz_debug_drainage_mfd_sweeps(cap)
                            mfd(e, passes)
                        return run
                    cms = measure([("", capped(c, p)) for c, (p, _) in zip(caps, need)], a.reps)
                    for cap, (p, conv), m in zip(caps, need, cms):
                        print("  exponent %d, sweeps <= %-3d  %10.4f ms  [%.4f, %.4f]  %5d passes, converged %d" %
                              (e, cap, float(np.median(m)), min(m), max(m), p, conv), flush=True)
                finally:
                    N.lib.nz_debug_drainage_mfd_sweeps(0)
            for t in (h, out, const, work, work_t):
                t.Dispose()


if __name__ == "__main__":
    main()
