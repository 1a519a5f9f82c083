#!/usr/bin/env python3
"""Stream-power fluvial erosion (nz_fluvial_erosion): HIP-event time per iteration at 1024^2 and 4096^2 on a simplex fBm
tile with the stage's defaults, beside the hydraulic stage and the constant job in the same process, all variants
alternating.  A sample times one call of --iters iterations (an even count: no height copy; the constant job: that many
calls) between two events, after --warmup such samples; reported per iteration as median [min, max] of --reps samples, with
the ratio to the constant job and the byte model's bandwidth (fluvial 16 B per cell and iteration: heights and drainage read
and written; hydraulic 56; constant job 8).  The last line per size states the bar: fluvial <= hydraulic x 16/56.
usage: bench_fluvial.py [--sizes 1024,4096] [--iters 100] [--reps 7] [--warmup 3]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402

HYDRAULIC = (1e-4, 1e-4, 0.01, 1.0, 0.3, 0.3, 0.01)  # initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt
FLUVIAL = (0.05, 0.002, 1.0, 1.0, nj.FluvialErosionStage.SEA_OFF)  # erodibility, uplift, dt, rain, seaLevel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    iters = a.iters + (a.iters & 1)
    N = nj._native
    with nj.Context(0) as ctx:
        for res in (int(s) for s in a.sizes.split(",")):
            n = res * res
            start = ctx.alloc(n)
            ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), start.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700)
            d = ctx.alloc(n)
            const = ctx.alloc(n)
            work_f = ctx.alloc(N.lib.nz_fluvial_erosion_work_floats(res, 1))
            work_h = ctx.alloc(N.lib.nz_hydraulic_erosion_work_floats(res, 1))
            desc = N.FluvialDesc(iters, *FLUVIAL, None, None, None, None)

            def reset():  # every sample starts from the same terrain (outside the timed window)
                ctx.call("nz_flush_write_slice", d.ptr, start.ptr, n, handle=False)

            def fluvial():
                ctx.call("nz_fluvial_erosion", d.ptr, work_f.ptr, C.byref(desc), res, handle=False)

            def hydraulic():
                ctx.call("nz_hydraulic_erosion_stage", d.ptr, work_h.ptr, iters, *HYDRAULIC, res, handle=False)

            def constant():
                for _ in range(iters):
                    ctx.call("nz_constant_job", 0, const.ptr, None, 1.0, res, handle=False)

            variants = [("fluvial", 16.0, fluvial), ("hydraulic", 56.0, hydraulic), ("constant job", 8.0, constant)]

            def sample(fn):
                reset()
                h0 = ctx.record()
                fn()
                h1 = ctx.record()
                h1.Complete()
                return ctx.elapsed_ms(h0, h1) / iters

            for _ in range(a.warmup):
                for _, _, fn in variants:
                    sample(fn)
            ms = [[] for _ in variants]
            for _ in range(a.reps):
                for k, (_, _, fn) in enumerate(variants):
                    ms[k].append(sample(fn))
            med = [float(np.median(m)) for m in ms]
            print("%d^2, %d samples of %d iterations, variants alternating" % (res, a.reps, iters))
            for (name, bytes_per_cell, _), m, md in zip(variants, ms, med):
                print("  %-13s %.4f ms/iteration  [%.4f, %.4f]  x%.3f of the constant job  model %.2f TB/s" %
                      (name, md, min(m), max(m), md / med[2], bytes_per_cell * n / (md * 1e-3) / 1e12), flush=True)
            bar = med[1] * 16.0 / 56.0
            print("  bar: hydraulic x 16/56 = %.4f ms/iteration; fluvial %.4f: %s" %
                  (bar, med[0], "met" if med[0] <= bar else "MISSED"), flush=True)
            for t in (start, d, const, work_f, work_h):
                t.Dispose()


if __name__ == "__main__":
    main()
