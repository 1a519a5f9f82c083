#!/usr/bin/env python3
"""Grid hydraulic erosion, the extended entry against the plain one (nz_hydraulic_erosion_ex / nz_hydraulic_erosion_stage):
HIP-event time per iteration at 1024^2 and 4096^2 on tools/bench_hydraulic.py's tile with the stage's defaults, for six
variants timed in ONE run, alternating (every round of samples visits every variant once, so drift of the machine falls on
all of them alike): the plain entry, _ex with everything off (the same kernels), open border only, both maps only, both
masks only, everything on.  Each sample times one call of --iters iterations (an even count: no height copy) between two
events, after --warmup such calls per variant; reported per iteration as median [min, max] of --reps samples, the ratio to
the plain entry's median, and the byte model's ratio (56 B per cell and iteration; the rain map +4 B x 1.5 for its radius-3
halo, the hardness map +4 B, the two masks +16 B read and written).
usage: bench_hydraulic_ex.py [--sizes 1024,4096] [--iters 200] [--reps 7] [--warmup 3]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402

DEFAULTS = (1e-4, 1e-4, 0.01, 1.0, 0.3, 0.3, 0.01)  # initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt
#            name          open  maps   masks  bytes per cell and iteration
VARIANTS = (("plain entry", None, None, None, 56.0),
            ("ex all off", False, False, False, 56.0),
            ("open only", True, False, False, 56.0),
            ("maps only", False, True, False, 56.0 + 6.0 + 4.0),
            ("masks only", False, False, True, 56.0 + 16.0),
            ("everything on", True, True, True, 56.0 + 6.0 + 4.0 + 16.0))


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
            n = res * res
            d, h0 = ctx.alloc(n), ctx.alloc(n)
            ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), h0.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700)
            work = ctx.alloc(nj._native.lib.nz_hydraulic_erosion_work_floats(res, 1))
            rng = np.random.default_rng(3)
            rain = ctx.from_host((rng.random(n, dtype=np.float32) * np.float32(2.0)).astype(np.float32))
            hard = ctx.from_host((rng.random(n, dtype=np.float32) * np.float32(0.5)).astype(np.float32))
            wear, deposits = ctx.alloc(n), ctx.alloc(n)

            def call(v):
                # every sample starts from the same heights (the copy is outside the timed window)
                ctx.call("nz_flush_write_slice", d.ptr, h0.ptr, n, handle=False)
                _, op, maps, masks, _ = v
                h_a = ctx.record()
                if op is None:
                    ctx.call("nz_hydraulic_erosion_stage", d.ptr, work.ptr, iters, *DEFAULTS, res, handle=False)
                else:
                    desc = nj._native.HydraulicDesc(iters, *DEFAULTS, int(op), rain.ptr if maps else None,
                                                    hard.ptr if maps else None, wear.ptr if masks else None,
                                                    deposits.ptr if masks else None)
                    ctx.call("nz_hydraulic_erosion_ex", d.ptr, work.ptr, C.byref(desc), res, handle=False)
                h_b = ctx.record()
                h_b.Complete()
                return ctx.elapsed_ms(h_a, h_b) / iters

            for _ in range(a.warmup):
                for v in VARIANTS:
                    call(v)
            ms = {v[0]: [] for v in VARIANTS}
            for _ in range(a.reps):
                for v in VARIANTS:
                    ms[v[0]].append(call(v))
            base = float(np.median(ms["plain entry"]))
            for v in VARIANTS:
                t = np.array(ms[v[0]])
                med = float(np.median(t))
                print("%5d^2  %-14s %.4f ms/iteration  [%.4f, %.4f] over %d samples of %d iterations  x%.3f of plain  "
                      "(byte model x%.3f, %.2f TB/s)" % (res, v[0], med, t.min(), t.max(), a.reps, iters, med / base,
                                                        v[4] / 56.0, v[4] * n / (med * 1e-3) / 1e12), flush=True)
            for t in (d, h0, work, rain, hard, wear, deposits):
                t.Dispose()


if __name__ == "__main__":
    main()
