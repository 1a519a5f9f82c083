#!/usr/bin/env python3
"""Implicit fluvial erosion (nz_fluvial_implicit): HIP-event time of one solve to convergence at 1024^2 and 4096^2 on the
project's usual tile -- 13-octave simplex fBm run through nz_fill_depressions at its defaults, with the drainage plane of
nz_drainage_area -- for dt in --dts, with the default budget and with a budget of exactly the passes it needs; beside it one
stage iteration (nz_drainage_area, then the solve told to proceed by its converged word), nz_watershed with length and
nz_drainage_area on the same tile (the yardsticks: the same tree and pass scheme), nz_constant_job (the byte-bound one) and
the explicit nz_fluvial_erosion for as many iterations as the same model time (iterations = dt at the explicit dt 1; recorded,
no bar); then the solve under other sweep caps (nz_debug_fluvial_implicit_sweeps), each with a budget of exactly the passes it
needs.  All in one process with the variants alternating.  A sample times one call between two events, after --warmup such
samples; reported as median [min, max] of --reps samples.  Also: the passes the default cap needs against the default
budget.  Last, untimed and unless --no-tiles: the tiles that changed, pass by pass, for the solve and for nz_watershed -- a
call with a budget of p passes leaves the tile bytes of pass p - 1 in `work` (16 status words, then two generations of
(tiles + 15) / 16 * 16 bytes: nz_terrain_stages.cpp) -- summed over the passes.  Writes what it prints to --out as it goes.
usage: bench_fluvial_implicit.py [--sizes 1024,4096] [--dts 1,100] [--reps 7] [--warmup 2] [--sweeps 4,8,16,32,64]
                                 [--no-tiles] [--out profiles/fluvial_implicit.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noize_job_amd as nj  # noqa: E402

SEA_OFF = nj.ImplicitFluvialStage.SEA_OFF
ERODIBILITY, UPLIFT = 0.05, 0.002  # the stage's defaults


def default_budget(res):
    return 64 + res // 4  # ImplicitFluvialStage's, for the drainage series and for the solve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--dts", default="1,100")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweeps", default="4,8,16,32,64")
    ap.add_argument("--no-tiles", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fluvial_implicit.txt"))
    a = ap.parse_args()
    N = nj._native
    sink = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        sink = open(a.out, "w")

    def say(text):
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

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
            out, area, area2, basin, length, const, hx = (ctx.alloc(n) for _ in range(7))
            work = ctx.alloc(N.lib.nz_fluvial_implicit_work_floats(res, 1))
            work_d = ctx.alloc(N.lib.nz_drainage_area_work_floats(res, 1))
            work_w = ctx.alloc(N.lib.nz_watershed_work_floats(res, 1, 1))
            work_x = ctx.alloc(N.lib.nz_fluvial_erosion_work_floats(res, 1))
            budget = default_budget(res)

            def status(w):
                ctx.synchronize()
                return [int(v) for v in ctx.wrap(w.ptr, 2, dtype=np.int32).ToArray()]

            def drain(passes=budget, dst=area):
                desc = N.DrainageDesc(1.0, SEA_OFF, passes, None)
                ctx.call("nz_drainage_area", h.ptr, dst.ptr, work_d.ptr, C.byref(desc), res, handle=False)

            def solve(dt, passes=budget, proceed=None, a_plane=area):
                desc = N.FluvialImplicitDesc(ERODIBILITY, UPLIFT, dt, SEA_OFF, passes, None, None, proceed, None)
                ctx.call("nz_fluvial_implicit", h.ptr, a_plane.ptr, out.ptr, work.ptr, C.byref(desc), res, handle=False)

            def iteration(dt):  # what ImplicitFluvialStage enqueues per iteration
                drain(dst=area2)
                solve(dt, proceed=work_d.ptr + 4, a_plane=area2)

            def shed(passes=budget):
                desc = N.WatershedDesc(SEA_OFF, 1.0, passes)
                ctx.call("nz_watershed", h.ptr, basin.ptr, length.ptr, None, work_w.ptr, C.byref(desc), res, handle=False)

            def explicit(iterations):
                ctx.call("nz_flush_write_slice", hx.ptr, h.ptr, n, handle=False)  # the explicit entry works in place
                desc = N.FluvialDesc(iterations, ERODIBILITY, UPLIFT, 1.0, 1.0, SEA_OFF, None, None, None, None)
                ctx.call("nz_fluvial_erosion", hx.ptr, work_x.ptr, C.byref(desc), res, handle=False)

            drain(16 * budget)
            used_d = status(work_d)
            shed(16 * budget)
            used_w = status(work_w)
            say("%d^2 (fill converged %d): nz_drainage_area %d passes (converged %d), nz_watershed with length %d (converged %d); "
                "the default budget is %d" % (res, filled, used_d[0], used_d[1], used_w[0], used_w[1], budget))

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

            for dt in (float(s) for s in a.dts.split(",")):
                # ---- once, untimed, with a budget that cannot run out short of the plane's cell count ----
                solve(dt, 16 * budget)
                used = status(work)
                want = out.ToArray().view(np.uint32).copy()
                say("  dt %g: the solve comes to rest in %d passes (converged %d), default cap; the default budget %d is x%.1f of that%s"
                    % (dt, used[0], used[1], budget, budget / max(used[0], 1),
                       "" if used[0] + 1 < budget else "  ** TOO SMALL **"))
                steps = max(1, int(round(dt)))
                variants = [("solve, default budget", lambda: solve(dt)),
                            ("solve, budget = passes", lambda: solve(dt, used[0])),
                            ("drainage + solve (one stage iteration)", lambda: iteration(dt)),
                            ("nz_watershed with length, default budget", lambda: shed()),
                            ("nz_drainage_area, default budget", lambda: drain()),
                            ("nz_constant_job", lambda: ctx.call("nz_constant_job", 0, const.ptr, None, 1.0, res, handle=False)),
                            ("explicit nz_fluvial_erosion, %d x dt 1 (with its copy)" % steps, lambda: explicit(steps))]
                ms = measure(variants, a.reps)
                med = [float(np.median(m)) for m in ms]
                say("  dt %g: %d samples, variants alternating" % (dt, a.reps))
                for (name, _), m, md in zip(variants, ms, med):
                    say("    %-52s %10.4f ms  [%.4f, %.4f]  x%.2f of nz_watershed, x%.1f of the constant job" %
                        (name, md, min(m), max(m), md / med[3], md / med[5]))
                say("    the bar: solve / nz_watershed with length = %.2f (expected 1.33 by bytes, bar 1.5): %s" %
                    (med[0] / med[3], "met" if med[0] <= 1.5 * med[3] else "MISSED"))

                # ---- the sweep cap: the passes each cap needs first, then timed with exactly that budget ----
                caps = [int(s) for s in a.sweeps.split(",") if s]
                if caps:
                    try:
                        need = []
                        for cap in caps:
                            N.lib.nz_debug_fluvial_implicit_sweeps(cap)
                            solve(dt, 64 * budget)
                            need.append(status(work))
                            assert np.array_equal(out.ToArray().view(np.uint32), want) or not need[-1][1], cap

                        def capped(cap, passes):
                            def run():
                                N.lib.nz_debug_fluvial_implicit_sweeps(cap)
                                solve(dt, passes)
                            return run
                        cms = measure([("", capped(c, p)) for c, (p, _) in zip(caps, need)], a.reps)
                        for cap, (p, conv), m in zip(caps, need, cms):
                            say("    sweeps <= %-3d  %10.4f ms  [%.4f, %.4f]  %5d passes, converged %d" %
                                (cap, float(np.median(m)), min(m), max(m), p, conv))
                    finally:
                        N.lib.nz_debug_fluvial_implicit_sweeps(0)

                # ---- the tiles that changed in each pass, and the tiles the pass behind it therefore visits ----
                if not a.no_tiles:
                    tnx, tnz = -(-res // 64), -(-res // 16)
                    gen = (tnx * tnz + 15) // 16 * 16  # bytes of one generation

                    def changed_tiles(run, w, rest):
                        moved = visited = 0
                        for p in range(1, rest + 1):
                            run(p)
                            ctx.synchronize()
                            m = ctx.wrap(w.ptr + 64 + gen * ((p - 1) & 1), tnx * tnz, dtype=np.uint8).ToArray().reshape(tnz, tnx) != 0
                            pad = np.pad(m, 1)
                            near = np.zeros_like(m)
                            for dz in range(3):
                                for dx in range(3):
                                    near |= pad[dz:dz + tnz, dx:dx + tnx]
                            moved, visited = moved + int(m.sum()), visited + int(near.sum())
                        return moved, visited
                    for name, run, w, rest in (("the solve", lambda p: solve(dt, p), work, used[0]),
                                               ("nz_watershed", shed, work_w, used_w[0])):
                        moved, visited = changed_tiles(run, w, rest)
                        say("    %-13s tiles that changed, summed over %d passes: %d = %.1f x the plane's %d; tiles visited by the "
                            "pass behind each: %d = %.1f x" % (name, rest, moved, moved / (tnx * tnz), tnx * tnz, visited,
                                                               visited / (tnx * tnz)))
            for t in (h, out, area, area2, basin, length, const, hx, work, work_d, work_w, work_x):
                t.Dispose()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
