#!/usr/bin/env python3
"""Watershed (nz_watershed): HIP-event time of one call to convergence at 1024^2 and 4096^2 on the project's usual tile --
13-octave simplex fBm run through nz_fill_depressions at its defaults -- as labels only, labels plus length, and labels plus
length plus receivers, each with the default budget and with a budget of exactly the passes it needs, beside
nz_drainage_area on the same tile (the yardstick: the same tree, the same pass scheme, read the other way) and
nz_constant_job (the byte-bound one); then the stage under other sweep caps (nz_debug_watershed_sweeps), each with a budget
of exactly the passes it needs.  All in one process with the variants alternating.  A sample times one call between two
events, after --warmup such samples; reported as median [min, max] of --reps samples.  Also: the passes the default cap
needs against the default budget, and the number of basins.  Last, untimed and unless --no-tiles: the tiles that changed, pass
by pass, for the stage and for nz_drainage_area -- a call with a budget of p passes leaves the tile bytes of pass p - 1 in
`work` (16 status words, then two generations of (tiles + 15) / 16 * 16 bytes: nz_terrain_stages.cpp) -- summed over the
passes, which is the work the two stages do on the same tree.  Writes what it prints to --out as well.
usage: bench_watershed.py [--sizes 1024,4096] [--reps 7] [--warmup 2] [--sweeps 4,8,16,32,64] [--no-tiles]
                          [--out profiles/watershed.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noize_job_amd as nj  # noqa: E402

SEA_OFF = nj.WatershedStage.SEA_OFF


def default_budget(res):
    return 64 + res // 4  # WatershedStage's, and DrainageAreaStage's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweeps", default="4,8,16,32,64")
    ap.add_argument("--no-tiles", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "watershed.txt"))
    a = ap.parse_args()
    N = nj._native
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

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
            basin, length, area, const = (ctx.alloc(n) for _ in range(4))
            codes = ctx.alloc(n, dtype=np.uint8)
            work = ctx.alloc(N.lib.nz_watershed_work_floats(res, 1, 1))
            work_d = ctx.alloc(N.lib.nz_drainage_area_work_floats(res, 1))
            budget = default_budget(res)

            def status(w=work):
                ctx.synchronize()
                return [int(v) for v in ctx.wrap(w.ptr, 2, dtype=np.int32).ToArray()]

            def shed(passes=budget, with_length=True, with_codes=False):
                desc = N.WatershedDesc(SEA_OFF, 1.0, passes)
                ctx.call("nz_watershed", h.ptr, basin.ptr, length.ptr if with_length else None,
                         codes.ptr if with_codes else None, work.ptr, C.byref(desc), res, handle=False)

            def drain(passes=budget):
                desc = N.DrainageDesc(1.0, SEA_OFF, passes, None)
                ctx.call("nz_drainage_area", h.ptr, area.ptr, work_d.ptr, C.byref(desc), res, handle=False)

            # ---- each form once, untimed, with a budget that cannot run out short of the plane's cell count ----
            forms = [("labels only", dict(with_length=False)), ("labels + length", dict()),
                     ("labels + length + receivers", dict(with_codes=True))]
            used = []
            for name, kw in forms:
                shed(16 * budget, **kw)
                used.append(status())
            labels = ctx.wrap(basin.ptr, n, dtype=np.int32).ToArray()
            want_b, want_l = labels.copy(), length.ToArray().view(np.uint32).copy()
            drain(16 * budget)
            used_d = status(work_d)
            say("%d^2 (fill converged %d): passes to rest, default cap: %s; nz_drainage_area %d (converged %d); the default "
                "budget is %d (x%.1f of the most); %d basins, longest flow path %.1f cells" %
                (res, filled, ", ".join("%s %d (converged %d)" % (nm, p, c) for (nm, _), (p, c) in zip(forms, used)),
                 used_d[0], used_d[1], budget, budget / max(max(p for p, _ in used), 1), len(np.unique(labels)),
                 float(length.ToArray().max())))

            variants = []
            for (name, kw), (p, _) in zip(forms, used):
                variants.append((name + ", default budget", lambda kw=kw: shed(**kw)))
                variants.append((name + ", budget = passes", lambda kw=kw, p=p: shed(p, **kw)))
            variants += [("nz_drainage_area, default budget", lambda: drain()),
                         ("nz_drainage_area, budget = passes", lambda: drain(used_d[0])),
                         ("nz_constant_job", lambda: ctx.call("nz_constant_job", 0, const.ptr, None, 1.0, res, handle=False))]

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

            ms = measure(variants, a.reps)
            med = [float(np.median(m)) for m in ms]
            say("  %d samples, variants alternating" % a.reps)
            for k, ((name, _), m, md) in enumerate(zip(variants, ms, med)):
                say("  %-46s %10.4f ms  [%.4f, %.4f]  x%.2f of nz_drainage_area, x%.1f of the constant job" %
                    (name, md, min(m), max(m), md / med[6 + k % 2 if k < 8 else 6], md / med[8]))

            # ---- the sweep cap: the passes each cap needs first, then timed with exactly that budget (labels + length) ----
            caps = [int(s) for s in a.sweeps.split(",") if s]
            if caps:
                try:
                    need = []
                    for cap in caps:
                        N.lib.nz_debug_watershed_sweeps(cap)
                        shed(64 * budget)
                        need.append(status())
                        same = (np.array_equal(ctx.wrap(basin.ptr, n, dtype=np.int32).ToArray(), want_b) and
                                np.array_equal(length.ToArray().view(np.uint32), want_l))
                        assert same or not need[-1][1], cap

                    def capped(cap, passes):
                        def run():
                            N.lib.nz_debug_watershed_sweeps(cap)
                            shed(passes)
                        return run
                    cms = measure([("", capped(c, p)) for c, (p, _) in zip(caps, need)], a.reps)
                    for cap, (p, conv), m in zip(caps, need, cms):
                        say("  sweeps <= %-3d  %10.4f ms  [%.4f, %.4f]  %5d passes, converged %d" %
                            (cap, float(np.median(m)), min(m), max(m), p, conv))
                finally:
                    N.lib.nz_debug_watershed_sweeps(0)
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
                for name, run, w, rest in (("labels + length", shed, work, used[1][0]), ("nz_drainage_area", drain, work_d, used_d[0])):
                    moved, visited = changed_tiles(run, w, rest)
                    say("  %-17s tiles that changed, summed over %d passes: %d = %.1f x the plane's %d; tiles visited by the "
                        "pass behind each: %d = %.1f x" % (name, rest, moved, moved / (tnx * tnz), tnx * tnz, visited,
                                                           visited / (tnx * tnz)))
            for t in (h, basin, length, area, const, codes, work, work_d):
                t.Dispose()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
