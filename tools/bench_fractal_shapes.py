#!/usr/bin/env python3
"""Octave shapes (nz_fractal_shaped): HIP-event time of one noise launch for fBm, billow and ridged, per basis, at the
metric's size (4096^2, 13 octaves, hurst 0.4, noiseSize 1700), strict and tolerance mode.  Shapes alternate within each
round so that clock drift spreads evenly.
usage: bench_fractal_shapes.py [--res 4096] [--reps 100] [--rounds 3] [--bases Simplex,Perlin,Cellular]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bases", default="Simplex,Perlin,Cellular")
    a = ap.parse_args()
    res = a.res
    with nj.Context(0) as ctx:
        d = ctx.alloc(res * res)

        def timed(basis, shape):
            def launch():
                ctx.call("nz_fractal_shaped", int(basis), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 4096 * 3, 4096 * 5, 1700,
                         int(shape), 1.0, 2.0, handle=False)
            for _ in range(10):
                launch()
            h0 = ctx.record()
            for _ in range(a.reps):
                launch()
            h1 = ctx.record()
            h1.Complete()
            return ctx.elapsed_ms(h0, h1) / a.reps

        for mode, mname in ((0, "strict"), (1, "fast")):
            ctx.float_mode = mode
            for name in a.bases.split(","):
                basis = nj.FractalNoise[name]
                best = {s: float("inf") for s in nj.FractalShape}
                for rnd in range(a.rounds):
                    for s in nj.FractalShape:
                        best[s] = min(best[s], timed(basis, s))
                fbm = best[nj.FractalShape.Fbm]
                print("%-6s %-14s " % (mname, name) + "  ".join("%s %.4f ms (%.3fx)" % (s.name, best[s], best[s] / fbm)
                                                              for s in nj.FractalShape), flush=True)
        d.Dispose()


if __name__ == "__main__":
    main()
