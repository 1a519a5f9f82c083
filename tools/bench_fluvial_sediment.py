#!/usr/bin/env python3
"""Implicit fluvial erosion with sediment deposition (nz_fluvial_sediment): HIP-event time of one call at the hosts' default
K = 4 at 1024^2 and 4096^2 on the project's usual tile -- 13-octave simplex fBm run through nz_fill_depressions at its
defaults -- for dt 1 and 100 and G 0.5 and 1, on the drainage plane nz_drainage_area delivers, beside the YARDSTICK measured
in the same run: t(nz_fluvial_implicit) + K * (t(nz_drainage_area) + t(nz_fluvial_implicit)) on the same tile, which is what
a host composing the existing entries would pay at the least, its elementwise launches not counted.  All in one process with
the variants alternating; every entry runs with the hosts' default budget 64 + resolution / 4 per series.
The bar: the new entry is not slower than the yardstick beyond the yardstick's own run-to-run spread in this run (it computes
receivers and donors once instead of 2K + 1 times, and adds K + 1 one-plane launches).
Untimed, first: the passes that did work -- solve series 0, and per iteration k the accumulation and the solve together (the
totals of calls with 0, 1, .. K iterations, differenced) -- the launches of a call, and the residual after k = 1 .. K.
A sample times one call between two events, after --warmup such samples; reported as median [min, max] of --reps samples.
usage: bench_fluvial_sediment.py [--sizes 1024,4096] [--dts 1,100] [--gs 0.5,1] [--k 4] [--reps 7] [--warmup 2]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402

SEA_OFF = nj.DrainageAreaStage.SEA_OFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--dts", default="1,100")
    ap.add_argument("--gs", default="0.5,1")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    N = nj._native
    dts = [float(s) for s in a.dts.split(",")]
    gs = [float(s) for s in a.gs.split(",")]
    K = a.k
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
            area, out, scratch = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
            work = ctx.alloc(N.lib.nz_fluvial_sediment_work_floats(res, 1))
            work_i = ctx.alloc(N.lib.nz_fluvial_implicit_work_floats(res, 1))
            work_d = ctx.alloc(N.lib.nz_drainage_area_work_floats(res, 1))
            budget = 64 + res // 4  # the hosts' default, for every series

            def status(w, words=2):
                ctx.synchronize()
                return ctx.wrap(w.ptr, words, dtype=np.int32).ToArray()

            def drain(to):
                desc = N.DrainageDesc(1.0, SEA_OFF, budget, None)
                ctx.call("nz_drainage_area", h.ptr, to.ptr, work_d.ptr, C.byref(desc), res, handle=False)

            def implicit(dt):
                desc = N.FluvialImplicitDesc(0.05, 0.002, dt, SEA_OFF, budget, None, None, None, None)
                ctx.call("nz_fluvial_implicit", h.ptr, area.ptr, out.ptr, work_i.ptr, C.byref(desc), res, handle=False)

            def sediment(dt, G, k):
                desc = N.FluvialSedimentDesc(0.05, 0.002, dt, SEA_OFF, budget, None, None, None, None, G, k, None)
                ctx.call("nz_fluvial_sediment", h.ptr, area.ptr, out.ptr, work.ptr, C.byref(desc), res, handle=False)

            drain(area)
            used_d, conv_d = (int(v) for v in status(work_d))
            print("%d^2 (fill converged %d), budget %d per series; nz_drainage_area converged %d after %d passes" %
                  (res, filled, budget, conv_d, used_d), flush=True)
            launches = 2 + (1 if K else 0) + (2 * K + 1) * budget + 2 * K + 1
            for dt in dts:
                implicit(dt)
                used_i, conv_i = (int(v) for v in status(work_i))
                for G in gs:
                    totals, residuals, conv = [], [], 1
                    for k in range(K + 1):
                        sediment(dt, G, k)
                        st = status(work, 3)
                        totals.append(int(st[0]))
                        conv &= int(st[1])
                        if k:
                            residuals.append(float(st[2:3].view(np.float32)[0]))
                    per = [totals[0]] + [b - c for b, c in zip(totals[1:], totals)]
                    print("  dt %g G %g K %d: converged %d; passes: solve 0 %d (nz_fluvial_implicit alone: %d, converged %d), "
                          "then accumulation + solve per iteration %s, %d in all; %d launches a call; residual after k = 1..%d: %s" %
                          (dt, G, K, conv, per[0], used_i, conv_i, per[1:], totals[-1], launches, K,
                           ", ".join("%.3g" % r for r in residuals)), flush=True)
            tiles = [h, area, out, scratch, work, work_i, work_d]
            if not a.reps:
                for t in tiles:
                    t.Dispose()
                continue
            variants = [("nz_drainage_area", lambda: drain(scratch))]
            for dt in dts:
                variants.append(("nz_fluvial_implicit dt=%g" % dt, lambda dt=dt: implicit(dt)))
                for G in gs:
                    variants.append(("nz_fluvial_sediment dt=%g G=%g" % (dt, G), lambda dt=dt, G=G: sediment(dt, G, K)))

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
            ms = {name: [] for name, _ in variants}
            for _ in range(a.reps):
                for name, fn in variants:
                    ms[name].append(sample(fn))
            print("  %d samples, variants alternating" % a.reps)
            for name, _ in variants:
                m = ms[name]
                print("  %-36s %10.4f ms  [%.4f, %.4f]" % (name, float(np.median(m)), min(m), max(m)))
            td = np.array(ms["nz_drainage_area"])
            for dt in dts:
                ti = np.array(ms["nz_fluvial_implicit dt=%g" % dt])
                yard = ti + K * (td + ti)  # sample by sample: the three calls of a sample ran next to each other
                ym, ylo, yhi = float(np.median(yard)), float(yard.min()), float(yard.max())
                for G in gs:
                    t = float(np.median(ms["nz_fluvial_sediment dt=%g G=%g" % (dt, G)]))
                    print("  dt %g G %g: nz_fluvial_sediment %.4f ms against the yardstick %.4f ms [%.4f, %.4f] = x%.2f: %s" %
                          (dt, G, t, ym, ylo, yhi, t / ym, "within" if t <= yhi else "BEYOND the yardstick's spread"), flush=True)
            for t in tiles:
                t.Dispose()


if __name__ == "__main__":
    main()
