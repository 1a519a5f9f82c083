#!/usr/bin/env python3
"""Domain warp (nz_fractal_warped): HIP-event time of one noise launch for plain fBm and for warped fBm with 2 and 4
displacement octaves, per basis, at the metric's size (4096^2, 13 octaves, hurst 0.4, noiseSize 1700), strict and tolerance
mode.  The forms alternate within each round so that clock drift spreads evenly; best of the rounds.
usage: bench_fractal_warp.py [--res 4096] [--reps 50] [--rounds 3] [--bases Simplex,Perlin,Cellular] [--strength 300]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bases", default="Simplex,Perlin,Cellular")
    ap.add_argument("--strength", type=float, default=300.0)
    a = ap.parse_args()
    res = a.res
    forms = [("fBm", 0), ("warp2", 2), ("warp4", 4)]  # (name, warpOctaves); 0: no warp, the nz_fractal_shaped path
    with nj.Context(0) as ctx:
        d = ctx.alloc(res * res)

        def timed(basis, octaves):
            def launch():
                ctx.call("nz_fractal_warped", int(basis), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 4096 * 3, 4096 * 5, 1700,
                         0, 1.0, 2.0, a.strength, 1.0, octaves, handle=False)
            for _ in range(5):
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
                best = {f: float("inf") for f, _ in forms}
                for _ in range(a.rounds):
                    for f, octaves in forms:
                        best[f] = min(best[f], timed(basis, octaves))
                fbm = best["fBm"]
                print("%-6s %-14s " % (mname, name) + "  ".join("%s %.4f ms (%.3fx)" % (f, best[f], best[f] / fbm)
                                                              for f, _ in forms), flush=True)
        d.Dispose()


if __name__ == "__main__":
    main()
