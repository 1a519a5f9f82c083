#!/usr/bin/env python3
"""Upsample / downsample (nz_upsample, nz_downsample): HIP-event time per call beside nz_constant_job on a 4096^2 plane, the
byte-bound yardstick (8 B per cell), all variants alternating in one process.  Each sample times --calls back-to-back calls
of one variant between two events; every variant gets --warmup untimed samples first, then the variants take turns --reps
times (a write-only fill of the fine plane runs beside them); reported as median [min, max] per call, the ratio to the constant job's median, and the byte model's bandwidth
(4 B per fine cell + 4 B per coarse cell, + 4 B per fine cell with base; `base=dst` is the in-place form, whose
footprint is the constant job's: one fine plane).  --recipe adds the coarse-to-fine total on
bench_hydraulic.py's tile: down + 500 iterations at 1024^2 + subtract + up with base + 20 iterations at 4096^2, against 500
iterations at 4096^2.
usage: bench_resample.py [--fine 4096] [--calls 20] [--reps 7] [--warmup 3] [--recipe]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402

HYDRAULIC = (1e-4, 1e-4, 0.01, 1.0, 0.3, 0.3, 0.01)  # bench_hydraulic.py's defaults
FILTERS = {"nearest": 0, "bilinear": 1, "catmull-rom": 2}


def timed(ctx, fn, calls):
    h0 = ctx.record()
    for _ in range(calls):
        fn()
    h1 = ctx.record()
    h1.Complete()
    return ctx.elapsed_ms(h0, h1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fine", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--recipe", action="store_true")
    a = ap.parse_args()
    fine = a.fine
    with nj.Context(0) as ctx:
        big = ctx.alloc(fine * fine)       # the fine plane: dst of the upsamples, src of the downsamples
        base = ctx.alloc(fine * fine)
        const = ctx.alloc(fine * fine)
        small = {f: ctx.alloc((fine // f) ** 2) for f in (2, 4, 8)}
        ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), base.ptr, fine, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700)
        ctx.call("nz_flush_write_slice", const.ptr, base.ptr, fine * fine)
        for f, t in small.items():
            ctx.call("nz_downsample", base.ptr, fine, t.ptr, f)

        def up(f, filt, with_base, in_place=False):
            b = big.ptr if in_place else base.ptr if with_base else None
            return lambda: ctx.call("nz_upsample", small[f].ptr, fine // f, big.ptr, f, filt, b, handle=False)

        def down(f):
            return lambda: ctx.call("nz_downsample", base.ptr, fine, small[f].ptr, f, handle=False)

        variants = [("constant job %d^2 (yardstick)" % fine, 8.0,
                     lambda: ctx.call("nz_constant_job", 0, const.ptr, None, 1.0, fine, handle=False))]
        # a second yardstick for the forms without base, which write 16 times what they read: a write-only plane
        variants.append(("fill %d^2 (write only)" % fine, 4.0, lambda: ctx.call("nz_fill_array", big.ptr, fine, 0.5, handle=False)))
        for name, filt in FILTERS.items():
            for wb in (False, True):
                variants.append(("up x4 %-11s %s" % (name, "base" if wb else "    "), 4.25 + 4 * wb, up(4, filt, wb)))
        # base = dst: the constant job's footprint (one fine plane read and written where it lies)
        variants.append(("up x4 catmull-rom base=dst", 8.25, up(4, 2, True, True)))
        variants.append(("up x2 catmull-rom base=dst", 9.0, up(2, 2, True, True)))
        variants.append(("down /4", 4.25, down(4)))
        for f in (2, 8):
            variants.append(("up x%d catmull-rom     " % f, 4.0 + 4.0 / (f * f), up(f, 2, False)))
            variants.append(("up x%d catmull-rom base" % f, 8.0 + 4.0 / (f * f), up(f, 2, True)))
            variants.append(("down /%d" % f, 4.0 + 4.0 / (f * f), down(f)))
        for _, _, fn in variants:
            for _ in range(a.warmup):
                timed(ctx, fn, a.calls)
        ms = [[] for _ in variants]
        for _ in range(a.reps):
            for k, (_, _, fn) in enumerate(variants):
                ms[k].append(timed(ctx, fn, a.calls))
        ref = float(np.median(ms[0]))
        print("fine plane %d^2, %d samples of %d calls, variants alternating" % (fine, a.reps, a.calls))
        for (name, bytes_per_cell, _), m in zip(variants, ms):
            m = np.array(m)
            med = float(np.median(m))
            print("%-32s %.4f ms  [%.4f, %.4f]  x%.3f of the constant job  model %.2f TB/s" %
                  (name, med, m.min(), m.max(), med / ref, bytes_per_cell * fine * fine / (med * 1e-3) / 1e12), flush=True)

        if a.recipe:
            cres = fine // 4
            coarse, eroded = small[4], ctx.alloc(cres * cres)
            work_c = ctx.alloc(nj._native.lib.nz_hydraulic_erosion_work_floats(cres, 1))
            work_f = ctx.alloc(nj._native.lib.nz_hydraulic_erosion_work_floats(fine, 1))

            def recipe():
                ctx.call("nz_downsample", base.ptr, fine, coarse.ptr, 4, handle=False)
                ctx.call("nz_flush_write_slice", eroded.ptr, coarse.ptr, cres * cres, handle=False)
                ctx.call("nz_hydraulic_erosion_stage", eroded.ptr, work_c.ptr, 500, *HYDRAULIC, cres, handle=False)
                ctx.call("nz_reduction_job", 0, eroded.ptr, coarse.ptr, None, cres, handle=False)
                ctx.call("nz_upsample", eroded.ptr, cres, big.ptr, 4, 2, base.ptr, handle=False)
                ctx.call("nz_hydraulic_erosion_stage", big.ptr, work_f.ptr, 20, *HYDRAULIC, fine, handle=False)

            def full():
                ctx.call("nz_flush_write_slice", big.ptr, base.ptr, fine * fine, handle=False)
                ctx.call("nz_hydraulic_erosion_stage", big.ptr, work_f.ptr, 500, *HYDRAULIC, fine, handle=False)

            timed(ctx, recipe, 1)
            r = np.array([timed(ctx, recipe, 1) for _ in range(3)])
            timed(ctx, full, 1)
            w = np.array([timed(ctx, full, 1) for _ in range(3)])
            print("coarse-to-fine: down /4 + 500 iterations at %d^2 + subtract + up x4 catmull-rom base + 20 iterations at %d^2: "
                  "%.2f ms [%.2f, %.2f]" % (cres, fine, np.median(r), r.min(), r.max()))
            print("500 iterations at %d^2 (with the copy of the tile): %.2f ms [%.2f, %.2f]  -> x%.1f" %
                  (fine, np.median(w), w.min(), w.max(), np.median(w) / np.median(r)))


if __name__ == "__main__":
    main()
