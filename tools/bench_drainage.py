#!/usr/bin/env python3
"""Drainage area (nz_drainage_area): HIP-event time of one call to convergence at 1024^2 and 4096^2 on the project's usual
tile -- 13-octave simplex fBm run through nz_fill_depressions at its defaults -- beside (a) the only other way to the same
plane, nz_fluvial_erosion with erodibility = uplift = 0 for the smallest iteration count N whose drainage is bit-equal to
the stage's, (b) the constant job as the byte-bound yardstick, and (c) the stage under other sweep caps
(nz_debug_drainage_sweeps), each with a budget of exactly the passes it needs; all in one process with the variants
alternating.  N is found first: the fluvial stage runs in calls of --probe iterations, each continuing the drainage of the
one before, compared on the host after every call; the last window is then bisected.  A sample times one call between two
events, after --warmup such samples; reported as median [min, max] of --reps samples.  Also: the passes the default cap
needs against the default budget, and the cost of an exhausted pass.
usage: bench_drainage.py [--sizes 1024,4096] [--reps 7] [--warmup 2] [--probe 256] [--limit 60000] [--sweeps 4,8,16,32,64]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402

SEA_OFF = nj.FluvialErosionStage.SEA_OFF
RAIN = 1.0


def default_budget(res):
    return 64 + res // 4  # DrainageAreaStage's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--probe", type=int, default=256)
    ap.add_argument("--limit", type=int, default=60000)
    ap.add_argument("--sweeps", default="4,8,16,32,64")
    a = ap.parse_args()
    N = nj._native
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
            out, const, carry, keep, hcopy = (ctx.alloc(n) for _ in range(5))
            work = ctx.alloc(N.lib.nz_drainage_area_work_floats(res, 1))
            work_f = ctx.alloc(N.lib.nz_fluvial_erosion_work_floats(res, 1))
            budget = default_budget(res)

            def status():
                ctx.synchronize()
                return [int(v) for v in ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()]

            def drain(passes=budget):
                desc = N.DrainageDesc(RAIN, SEA_OFF, passes, None)
                ctx.call("nz_drainage_area", h.ptr, out.ptr, work.ptr, C.byref(desc), res, handle=False)

            # ---- the stage once, untimed, with a budget that cannot run out short of the plane's cell count ----
            drain(16 * budget)
            used, converged = status()
            want = out.ToArray().view(np.uint32)
            print("%d^2 (fill converged %d): the stage converged %d after %d passes; the default budget is %d (x%.1f); largest "
                  "area %d cells" % (res, filled, converged, used, budget, budget / max(used, 1), int(out.ToArray().max())),
                  flush=True)

            # ---- (a) N: the fewest iterations of the fluvial stage at rest whose drainage equals the stage's ----
            def fluvial(its, start):  # `its` iterations from the drainage in `start` (None: rain), heights from a copy
                ctx.call("nz_flush_write_slice", hcopy.ptr, h.ptr, n, handle=False)
                desc = N.FluvialDesc(its, 0.0, 0.0, 1.0, RAIN, SEA_OFF, None, None, None, start.ptr if start is not None else None)
                ctx.call("nz_fluvial_erosion", hcopy.ptr, work_f.ptr, C.byref(desc), res, handle=False)

            def equal():
                ctx.synchronize()
                return np.array_equal(ctx.wrap(work_f.ptr, n).ToArray().view(np.uint32), want)

            done, hit = 0, False
            while not hit and done < a.limit:
                if done:
                    ctx.call("nz_flush_write_slice", keep.ptr, carry.ptr, n, handle=False)
                fluvial(a.probe, carry if done else None)
                ctx.call("nz_flush_write_slice", carry.ptr, work_f.ptr, n, handle=False)
                hit = equal()
                done += a.probe
            if hit:  # bisect (done - probe, done]: the state after `lo` iterations is in `keep` (lo == 0: the start state)
                lo, hi = done - a.probe, done
                base = lo
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    fluvial(mid - base, keep if base else None)
                    lo, hi = (lo, mid) if equal() else (mid, hi)
                n_its = hi
                print("  (a) nz_fluvial_erosion at rest (erodibility = uplift = 0) is bit-equal to the stage after N = %d "
                      "iterations and not after %d" % (n_its, n_its - 1), flush=True)
            else:
                n_its = done
                print("  (a) nz_fluvial_erosion at rest is NOT bit-equal after %d iterations, the limit; timed with %d" %
                      (done, done), flush=True)
            heights_same = np.array_equal(hcopy.ToArray().view(np.uint32), h.ToArray().view(np.uint32))
            print("      heights untouched by it: %s" % heights_same, flush=True)

            rest = N.FluvialDesc(n_its, 0.0, 0.0, 1.0, RAIN, SEA_OFF, None, None, None, None)
            variants = [("stage, default budget", lambda: drain()),
                        ("stage, budget = passes used", lambda: drain(used)),
                        ("(a) fluvial at rest x N", lambda: ctx.call("nz_fluvial_erosion", hcopy.ptr, work_f.ptr, C.byref(rest), res,
                                                                     handle=False)),
                        ("(b) constant job", lambda: ctx.call("nz_constant_job", 0, const.ptr, None, 1.0, res, handle=False))]

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
            med = [float(np.median(m)) for m in ms]
            print("  %d samples, variants alternating" % a.reps)
            for (name, _), m, md in zip(variants, ms, med):
                print("  %-29s %10.4f ms  [%.4f, %.4f]  x%.1f of the constant job" % (name, md, min(m), max(m), md / med[3]))
            print("  fluvial per iteration         %10.4f ms (N = %d)" % (med[2] / n_its, n_its))
            if budget > used:
                print("  an exhausted pass             %10.4f ms ((default budget - exact budget) / %d launches)" %
                      ((med[0] - med[1]) / (budget - used), budget - used))
            print("  the stage against (a): x%.1f faster at the medians (%.4f ms against %.4f ms)" %
                  (med[2] / med[0], med[0], med[2]), flush=True)

            # ---- (c) the sweep cap: the passes each cap needs first, then timed with exactly that budget ----
            caps = [int(s) for s in a.sweeps.split(",") if s]
            if caps:
                try:
                    need = []
                    for cap in caps:
                        N.lib.nz_debug_drainage_sweeps(cap)
                        drain(64 * budget)
                        need.append(status())
                        assert np.array_equal(out.ToArray().view(np.uint32), want) or not need[-1][1], cap

                    def capped(cap, passes):
                        def run():
                            N.lib.nz_debug_drainage_sweeps(cap)
                            drain(passes)
                        return run
                    cms = measure([("", capped(c, p)) for c, (p, _) in zip(caps, need)], a.reps)
                    for cap, (p, conv), m in zip(caps, need, cms):
                        print("  (c) sweeps <= %-3d  %10.4f ms  [%.4f, %.4f]  %5d passes, converged %d" %
                              (cap, float(np.median(m)), min(m), max(m), p, conv), flush=True)
                finally:
                    N.lib.nz_debug_drainage_sweeps(0)
            for t in (h, out, const, carry, keep, hcopy, work, work_f):
                t.Dispose()


if __name__ == "__main__":
    main()
