#!/usr/bin/env python3
"""Hillslope diffusion (nz_hillslope_diffusion): HIP-event time of one step on the project's usual tile -- 13-octave simplex
fBm run through nz_fill_depressions at its defaults -- at 1024^2 and 4096^2 and on a batch of 64 x 512^2, for r in --rs, in
place and out of place, on the 16-byte path (the planes as allocated) and on the 4-byte path (the same planes entered one
float further on, so both launch forms run at the same size); beside it nz_constant_job on a plane of the same cell count
(the byte-bound yardstick: 2 plane moves; a step with p kept in `out` moves 8, so its byte floor is 4x that job) and, on the
single tiles, the nz_fluvial_implicit solve at dt 100 on the same tile with the drainage plane of nz_drainage_area (the
comparison that matters to a user: the diffusion step should cost less than the solve it follows).  All in one process with
the variants alternating.  A sample times one call between two events, after --warmup such samples; reported as median
[min, max] of --reps samples.  Writes what it prints to --out as it goes.
usage: bench_hillslope.py [--sizes 1024,4096] [--batch 64x512] [--rs 0.01,1,100] [--reps 9] [--warmup 2]
                          [--out profiles/hillslope.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noize_job_amd as nj  # noqa: E402

SEA_OFF = nj.ImplicitFluvialStage.SEA_OFF
ERODIBILITY, UPLIFT = 0.05, 0.002  # ImplicitFluvialStage's defaults


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--batch", default="64x512")
    ap.add_argument("--rs", default="0.01,1,100")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hillslope.txt"))
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

    cases = [(int(s), 1) for s in a.sizes.split(",") if s]
    if a.batch:
        count, res = (int(v) for v in a.batch.split("x"))
        cases.append((res, count))
    rs = [float(s) for s in a.rs.split(",")]

    with nj.Context(0) as ctx:
        for res, count in cases:
            n = count * res * res
            side = int(round(n ** 0.5))  # the constant job's plane of the same cell count
            assert side * side == n
            # one float of slack behind every plane: the 4-byte path enters the same planes one float further on
            h, plane, out, const = (ctx.alloc(n + 4) for _ in range(4))
            work = ctx.alloc(N.lib.nz_hillslope_diffusion_work_floats(res, count))
            for k in range(count):  # every tile of the batch its own fBm tile
                ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), h.ptr + 4 * k * res * res, res, 0.4, 1.0, 2.0, 0.0, 13,
                         7 * k, 3 * k, 1700, handle=False)
            fwork = ctx.alloc(N.lib.nz_fill_depressions_work_floats(res, count))
            fdesc = N.FillDesc(1e-4, SEA_OFF, 64 + res // 4, None)
            ctx.call("nz_fill_depressions_batch", h.ptr, fwork.ptr, C.byref(fdesc), res, count, handle=False)
            ctx.synchronize()
            filled = int(ctx.wrap(fwork.ptr, 2, dtype=np.int32).ToArray()[1])
            fwork.Dispose()
            ctx.call("nz_flush_write_slice", plane.ptr, h.ptr, n + 4, handle=False)

            def step(r, src, dst, off=0, iterations=1):
                desc = N.HillslopeDesc(r, 1.0, iterations)
                ctx.call("nz_hillslope_diffusion_batch", src.ptr + off, dst.ptr + off, work.ptr, C.byref(desc), res, count,
                         handle=False)

            single = count == 1
            if single:
                area = ctx.alloc(n)
                work_d = ctx.alloc(N.lib.nz_drainage_area_work_floats(res, 1))
                work_f = ctx.alloc(N.lib.nz_fluvial_implicit_work_floats(res, 1))
                budget = 64 + res // 4
                ddesc = N.DrainageDesc(1.0, SEA_OFF, budget, None)
                ctx.call("nz_drainage_area", h.ptr, area.ptr, work_d.ptr, C.byref(ddesc), res, handle=False)
                fdesc2 = N.FluvialImplicitDesc(ERODIBILITY, UPLIFT, 100.0, SEA_OFF, budget, None, None, None, None)

                def solve():
                    ctx.call("nz_fluvial_implicit", h.ptr, area.ptr, out.ptr, work_f.ptr, C.byref(fdesc2), res, handle=False)
                solve()
                ctx.synchronize()
                used = [int(v) for v in ctx.wrap(work_f.ptr, 2, dtype=np.int32).ToArray()]

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

            name = "%d^2" % res if single else "%d x %d^2" % (count, res)
            say("%s (fill converged %d): %d cells, work %d floats%s" % (
                name, filled, n, work.Length,
                "; nz_fluvial_implicit at dt 100 comes to rest in %d passes (converged %d)" % tuple(used) if single else ""))
            variants = [("nz_constant_job, %d^2" % side, lambda: ctx.call("nz_constant_job", 0, const.ptr, None, 1.0, side, handle=False))]
            for r in rs:
                variants += [("r %g: in place, 16-byte path" % r, lambda r=r: step(r, plane, plane)),
                             ("r %g: out of place, 16-byte path" % r, lambda r=r: step(r, h, out)),
                             ("r %g: in place, 4-byte path" % r, lambda r=r: step(r, plane, plane, 4)),
                             ("r %g: out of place, 4-byte path" % r, lambda r=r: step(r, h, out, 4))]
            variants.append(("r 1: 3 iterations in place, 16-byte path", lambda: step(1.0, plane, plane, 0, 3)))
            if single:
                variants.append(("nz_fluvial_implicit, dt 100, default budget", solve))
            ms = measure(variants, a.reps)
            med = [float(np.median(m)) for m in ms]
            say("  %d samples, variants alternating; the byte floor of a step is 4 x the constant job = %.4f ms" %
                (a.reps, 4 * med[0]))
            for (label, _), m, md in zip(variants, ms, med):
                say("    %-46s %10.4f ms  [%.4f, %.4f]  x%.2f of the constant job, x%.2f of the floor" %
                    (label, md, min(m), max(m), md / med[0], md / (4 * med[0])))
            if single:
                worst = max(med[1:1 + 4 * len(rs)])
                fl = ms[-1]
                say("    the bar: the slowest step %.4f ms against the solve beside it %.4f ms [%.4f, %.4f] (spread %.1f %%): "
                    "x%.3f, %s" % (worst, med[-1], min(fl), max(fl), 100.0 * (max(fl) - min(fl)) / med[-1], worst / med[-1],
                                   "met" if worst < min(fl) else "MISSED"))
                for t in (area, work_d, work_f):
                    t.Dispose()
            for t in (h, plane, out, const, work):
                t.Dispose()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
