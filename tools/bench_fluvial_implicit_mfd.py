#!/usr/bin/env python3
"""Multiple-flow implicit fluvial erosion (nz_fluvial_implicit_mfd): HIP-event time of one solve to convergence at 1024^2
and 4096^2 on the project's usual tile -- 13-octave simplex fBm run through nz_fill_depressions at its defaults -- for dt 1
and 100 and exponents 1 and 4, on the drainage plane nz_drainage_mfd delivers at the same exponent, beside (a)
nz_fluvial_implicit on the same A, the single-flow solve, (b) nz_drainage_mfd on the same tile, whose pass this one's is
modelled on, and (c) the constant job as the byte-bound one; all in one process with the variants alternating.  Every
series is timed with a budget of exactly the passes it needs.  Also: the passes used against MfdFluvialStage's default
budget 128 + resolution / 2 (within a factor of 2 of it the default must be raised), and the cost of the launches around
the passes (a call with a budget of 1 and of 2; 2 * t1 - t2 estimates begin + setup + finalise).
The bar: a live tile's pass of nz_drainage_mfd moves 40 B per cell (eight weights, A in and out), this one's 45 (eight f, b,
the gate byte, h' in and out), so the time per pass may be 45 / 40 x 1.5 = x1.69 of nz_drainage_mfd's in the same run.
A sample times one call between two events, after --warmup such samples; reported as median [min, max] of --reps samples.
Last, untimed and unless --no-tiles: the tiles that changed, pass by pass, and the tiles the pass behind each therefore
visits (a tile is visited when it or one of its eight neighbours changed), summed over the passes, for the solve and for
nz_drainage_mfd -- read from the generation of tile bytes a run of p passes leaves -- and with them the time per visited
tile: "per pass" averages over passes with different numbers of live tiles, this figure does not.
--reps 0 runs every series once at the default budget and times nothing: the form to put under a counter run.
usage: bench_fluvial_implicit_mfd.py [--sizes 1024,4096] [--exponents 1,4] [--dts 1,100] [--reps 7] [--warmup 2]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402

SEA_OFF = nj.DrainageAreaStage.SEA_OFF
BAR = 45.0 / 40.0 * 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--exponents", default="1,4")
    ap.add_argument("--dts", default="1,100")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-tiles", action="store_true")
    a = ap.parse_args()
    N = nj._native
    exponents = [int(s) for s in a.exponents.split(",")]
    dts = [float(s) for s in a.dts.split(",")]
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
            out, const, scratch = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
            areas = {e: ctx.alloc(n) for e in exponents}
            work = ctx.alloc(N.lib.nz_fluvial_implicit_mfd_work_floats(res, 1))
            work_s = ctx.alloc(N.lib.nz_fluvial_implicit_work_floats(res, 1))
            work_d = ctx.alloc(N.lib.nz_drainage_mfd_work_floats(res, 1))
            budget = 128 + res // 2  # MfdFluvialStage's default, for both series

            def status(w):
                ctx.synchronize()
                return [int(v) for v in ctx.wrap(w.ptr, 2, dtype=np.int32).ToArray()]

            def drain(e, passes, to):
                desc = N.DrainageMfdDesc(1.0, SEA_OFF, passes, e, None)
                ctx.call("nz_drainage_mfd", h.ptr, to.ptr, work_d.ptr, C.byref(desc), res, handle=False)

            def solve(e, dt, passes):
                desc = N.FluvialImplicitMfdDesc(0.05, 0.002, dt, SEA_OFF, passes, e, None, None, None, None)
                ctx.call("nz_fluvial_implicit_mfd", h.ptr, areas[e].ptr, out.ptr, work.ptr, C.byref(desc), res, handle=False)

            def single(e, dt, passes):
                desc = N.FluvialImplicitDesc(0.05, 0.002, dt, SEA_OFF, passes, None, None, None, None)
                ctx.call("nz_fluvial_implicit", h.ptr, areas[e].ptr, out.ptr, work_s.ptr, C.byref(desc), res, handle=False)

            # ---- every series once, untimed, with a budget that cannot run out short of the plane's cell count ----
            ample = 16 * budget if a.reps else budget
            print("%d^2 (fill converged %d), default budget %d" % (res, filled, budget), flush=True)
            used_d, used, used_s = {}, {}, {}
            for e in exponents:
                drain(e, ample, areas[e])
                used_d[e], conv = status(work_d)
                print("  nz_drainage_mfd exponent %d: converged %d after %d passes" % (e, conv, used_d[e]), flush=True)
                for dt in dts:
                    single(e, dt, ample)
                    used_s[e, dt], conv_s = status(work_s)
                    solve(e, dt, ample)
                    used[e, dt], conv = status(work)
                    got = out.ToArray()
                    print("  exponent %d dt %g: nz_fluvial_implicit_mfd converged %d after %d passes (the single-flow solve on the "
                          "same A: %d, converged %d); the default budget is x%.1f of the passes used; finite %s" %
                          (e, dt, conv, used[e, dt], used_s[e, dt], conv_s, budget / max(used[e, dt], 1),
                           bool(np.isfinite(got).all())), flush=True)
                    if 2 * used[e, dt] > budget:
                        print("  !! the passes used exceed half the default budget: raise the default to %d" % (2 * used[e, dt]))

            tiles = [h, out, const, scratch, work, work_s, work_d] + list(areas.values())
            if not a.reps:
                for t in tiles:
                    t.Dispose()
                continue
            variants = [("(c) constant job", lambda: ctx.call("nz_constant_job", 0, const.ptr, None, 1.0, res, handle=False))]
            for e in exponents:
                variants += [("(b) drainage_mfd e=%d, exact" % e, lambda e=e: drain(e, used_d[e], scratch)),
                             ("(b) drainage_mfd e=%d, budget 1" % e, lambda e=e: drain(e, 1, scratch)),
                             ("(b) drainage_mfd e=%d, budget 2" % e, lambda e=e: drain(e, 2, scratch))]
                for dt in dts:
                    variants += [("solve e=%d dt=%g, exact" % (e, dt), lambda e=e, dt=dt: solve(e, dt, used[e, dt])),
                                 ("solve e=%d dt=%g, default" % (e, dt), lambda e=e, dt=dt: solve(e, dt, budget)),
                                 ("solve e=%d dt=%g, budget 1" % (e, dt), lambda e=e, dt=dt: solve(e, dt, 1)),
                                 ("solve e=%d dt=%g, budget 2" % (e, dt), lambda e=e, dt=dt: solve(e, dt, 2)),
                                 ("(a) single e=%d dt=%g, exact" % (e, dt), lambda e=e, dt=dt: single(e, dt, used_s[e, dt]))]

            def sample(fn):
                ctx.synchronize()
                h0 = ctx.record()
                fn()
                h1 = ctx.record()
                h1.Complete()
                return ctx.elapsed_ms(h0, h1)

            for _ in range(a.warmup):
                for _, fn in variants:
                    sample(fn)
            ms = [[] for _ in variants]
            for _ in range(a.reps):
                for k, (_, fn) in enumerate(variants):
                    ms[k].append(sample(fn))
            med = {name: float(np.median(m)) for (name, _), m in zip(variants, ms)}
            print("  %d samples, variants alternating" % a.reps)
            for (name, _), m in zip(variants, ms):
                print("  %-34s %10.4f ms  [%.4f, %.4f]  x%.1f of the constant job" %
                      (name, med[name], min(m), max(m), med[name] / med["(c) constant job"]))
            for e in exponents:
                # per pass: the series less the launches around it, over the passes that ran
                around_d = 2 * med["(b) drainage_mfd e=%d, budget 1" % e] - med["(b) drainage_mfd e=%d, budget 2" % e]
                pass_d = (med["(b) drainage_mfd e=%d, exact" % e] - around_d) / used_d[e]
                print("  drainage_mfd e=%d: setup + finalise ~ %.4f ms; per pass %.4f ms over %d passes" %
                      (e, around_d, pass_d, used_d[e]))
                for dt in dts:
                    key = "solve e=%d dt=%g" % (e, dt)
                    around = 2 * med[key + ", budget 1"] - med[key + ", budget 2"]
                    per = (med[key + ", exact"] - around) / used[e, dt]
                    ts = med["(a) single e=%d dt=%g, exact" % (e, dt)]
                    print("  %s: begin + setup + finalise ~ %.4f ms; per pass %.4f ms over %d passes = x%.2f of drainage_mfd's, "
                          "bar x%.2f: %s; the whole solve x%.2f of the single-flow solve's %.4f ms (%d passes)" %
                          (key, around, per, used[e, dt], per / pass_d, BAR, "within" if per / pass_d <= BAR else "BEYOND",
                           med[key + ", exact"] / ts, ts, used_s[e, dt]), flush=True)
            # ---- the tiles that changed in each pass, and the tiles the pass behind it therefore visits ----
            if not a.no_tiles:
                tnx, tnz = -(-res // 64), -(-res // 16)
                gen = (tnx * tnz + 15) // 16 * 16  # bytes of one generation

                def visits(run, w, rest):
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
                    return moved, visited + tnx * tnz  # pass 0 visits every tile by decree
                for e in exponents:
                    rows = [("drainage_mfd e=%d" % e, lambda p, e=e: drain(e, p, scratch), work_d, used_d[e],
                             med["(b) drainage_mfd e=%d, exact" % e])]
                    rows += [("solve e=%d dt=%g" % (e, dt), lambda p, e=e, dt=dt: solve(e, dt, p), work, used[e, dt],
                              med["solve e=%d dt=%g, exact" % (e, dt)]) for dt in dts]
                    base = None
                    for name, run, w, rest, t in rows:
                        moved, visited = visits(run, w, rest)
                        per = t * 1e3 / visited
                        base = base or per
                        print("  %-22s tiles that changed over %d passes: %d = %.1f x the plane's %d; tiles visited: %d = %.1f x; "
                              "%.4f us per visited tile = x%.2f of drainage_mfd's" %
                              (name, rest, moved, moved / (tnx * tnz), tnx * tnz, visited, visited / (tnx * tnz), per, per / base),
                              flush=True)
            for t in tiles:
                t.Dispose()


if __name__ == "__main__":
    main()
