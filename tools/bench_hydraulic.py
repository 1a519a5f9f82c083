#!/usr/bin/env python3
"""Grid hydraulic erosion (nz_hydraulic_erosion_stage): HIP-event time per iteration of the stage at 1024^2 and 4096^2 on a
simplex fBm tile with the stage's defaults.  Each sample times one stage call of --iters iterations (an even count: no
height copy) between two events, after --warmup such calls; reported per iteration as median [min, max] of --reps samples,
with the byte model's bandwidth (56 B per cell and iteration: seven state planes read and written).
usage: bench_hydraulic.py [--sizes 1024,4096] [--iters 200] [--reps 7] [--warmup 3]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402

DEFAULTS = (1e-4, 1e-4, 0.01, 1.0, 0.3, 0.3, 0.01)  # initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    iters = a.iters + (a.iters & 1)
    with nj.Context(0) as ctx:
        for res in (int(s) for s in a.sizes.split(",")):
            d = ctx.alloc(res * res)
            ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700)
            work = ctx.alloc(nj._native.lib.nz_hydraulic_erosion_work_floats(res, 1))

            def call():
                ctx.call("nz_hydraulic_erosion_stage", d.ptr, work.ptr, iters, *DEFAULTS, res, handle=False)

            for _ in range(a.warmup):
                call()
            ms = []
            for _ in range(a.reps):
                h0 = ctx.record()
                call()
                h1 = ctx.record()
                h1.Complete()
                ms.append(ctx.elapsed_ms(h0, h1) / iters)
            ms = np.array(ms)
            med = float(np.median(ms))
            print("%5d^2  %.4f ms/iteration  [%.4f, %.4f] over %d samples of %d iterations  model %.2f TB/s" %
                  (res, med, ms.min(), ms.max(), a.reps, iters, 56.0 * res * res / (med * 1e-3) / 1e12), flush=True)
            d.Dispose()
            work.Dispose()


if __name__ == "__main__":
    main()
