#!/usr/bin/env python3
"""Stream order (nz_stream_order): HIP-event time of one call to convergence at 1024^2 and 4096^2 on the project's usual
tile -- 13-octave simplex fBm run through nz_fill_depressions at its defaults -- as order only without a threshold, order
with the drainage plane of nz_drainage_area and a threshold, and the same plus links, each with the default budget and with
a budget of exactly the passes it needs, beside nz_drainage_area on the same tile (the yardstick: the same tree, the same
donor bits, a float sum in place of max and count) and nz_constant_job (the byte-bound one); then the stage under other
sweep caps (nz_debug_stream_order_sweeps), each with a budget of exactly the passes it needs.  All in one process with the
variants alternating.  A sample times one call between two events, after --warmup such samples; reported as median
[min, max] of --reps samples.  Also: the passes the default cap needs against the default budget, the channel cells, the
links and the highest order.  Writes what it prints to --out as well.
usage: bench_stream_order.py [--sizes 1024,4096] [--reps 7] [--warmup 2] [--sweeps 4,8,16,32,64] [--threshold 100]
                             [--out profiles/stream_order.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noize_job_amd as nj  # noqa: E402

SEA_OFF = nj.StreamOrderStage.SEA_OFF


def default_budget(res):
    return 64 + res // 4  # StreamOrderStage's, and DrainageAreaStage's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweeps", default="4,8,16,32,64")
    ap.add_argument("--threshold", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_order.txt"))
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
            link, area, area2, const = (ctx.alloc(n) for _ in range(4))
            order = ctx.alloc(n, dtype=np.uint8)
            work = ctx.alloc(N.lib.nz_stream_order_work_floats(res, 1, 1))
            work_d = ctx.alloc(N.lib.nz_drainage_area_work_floats(res, 1))
            budget = default_budget(res)

            def status(w=work):
                ctx.synchronize()
                return [int(v) for v in ctx.wrap(w.ptr, 2, dtype=np.int32).ToArray()]

            def stream(passes=budget, with_area=True, with_links=False):
                desc = N.StreamOrderDesc(SEA_OFF, a.threshold, passes, area.ptr if with_area else None)
                ctx.call("nz_stream_order", h.ptr, order.ptr, link.ptr if with_links else None, work.ptr, C.byref(desc), res,
                         handle=False)

            def drain(passes=budget, dst=area2):
                desc = N.DrainageDesc(1.0, SEA_OFF, passes, None)
                ctx.call("nz_drainage_area", h.ptr, dst.ptr, work_d.ptr, C.byref(desc), res, handle=False)

            # ---- the drainage plane the stage reads, then each form once, untimed, with a budget far beyond the default ----
            drain(16 * budget, area)
            used_d = status(work_d)
            forms = [("order, no threshold", dict(with_area=False)), ("order, threshold %g" % a.threshold, dict()),
                     ("order + links, threshold %g" % a.threshold, dict(with_links=True))]
            used = []
            for name, kw in forms:
                stream(16 * budget, **kw)
                used.append(status())
            want_o = order.ToArray().copy()
            want_l = ctx.wrap(link.ptr, n, dtype=np.int32).ToArray().copy()
            say("%d^2 (fill converged %d): passes to rest, default cap: %s; nz_drainage_area %d (converged %d); the default "
                "budget is %d (x%.1f of the most); threshold %g: %d channel cells, %d links, highest order %d" %
                (res, filled, ", ".join("%s %d (converged %d)" % (nm, p, c) for (nm, _), (p, c) in zip(forms, used)),
                 used_d[0], used_d[1], budget, budget / max(max(p for p, _ in used), 1), a.threshold,
                 int((want_o > 0).sum()), len(np.unique(want_l[want_l >= 0])), int(want_o.max())))
            for (name, kw), (p, c) in zip(forms, used):
                if p > budget or not c:
                    say("  NOT INSIDE THE DEFAULT BUDGET: %s needs %d passes, the default allows %d" % (name, p, budget))

            variants = []
            for (name, kw), (p, _) in zip(forms, used):
                variants.append((name + ", default budget", lambda kw=kw: stream(**kw)))
                variants.append((name + ", budget = passes", lambda kw=kw, p=p: stream(p, **kw)))
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

            # ---- the sweep cap: the passes each cap needs first, then timed with exactly that budget (order + links) ----
            caps = [int(s) for s in a.sweeps.split(",") if s]
            if caps:
                try:
                    need = []
                    for cap in caps:
                        N.lib.nz_debug_stream_order_sweeps(cap)
                        stream(64 * budget, with_links=True)
                        need.append(status())
                        same = (np.array_equal(order.ToArray(), want_o) and
                                np.array_equal(ctx.wrap(link.ptr, n, dtype=np.int32).ToArray(), want_l))
                        assert same or not need[-1][1], cap

                    def capped(cap, passes):
                        def run():
                            N.lib.nz_debug_stream_order_sweeps(cap)
                            stream(passes, with_links=True)
                        return run
                    cms = measure([("", capped(c, p)) for c, (p, _) in zip(caps, need)], a.reps)
                    for cap, (p, conv), m in zip(caps, need, cms):
                        say("  sweeps <= %-3d  %10.4f ms  [%.4f, %.4f]  %5d passes, converged %d" %
                            (cap, float(np.median(m)), min(m), max(m), p, conv))
                finally:
                    N.lib.nz_debug_stream_order_sweeps(0)
            for t in (h, link, area, area2, const, order, work, work_d):
                t.Dispose()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
