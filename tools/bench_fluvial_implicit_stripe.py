#!/usr/bin/env python3
"""Implicit fluvial erosion on row stripes (nz_implicit_fluvial_stripe_round), tools/bench_drainage_stripe.py's protocol:
torch's HIP events around every sample, --warmup samples, median [min, max] of --reps samples, the variants alternating in
one process.
  1. The filled 13-octave fBm tile of tools/bench_fluvial_implicit.py at 4096^2 and its exact drainage plane, at dt 1 and 100:
       nz_fluvial_implicit with the hosts' default budget                                  -- the yardstick
       one stripe: a round with `first`, a quiet round, finalise; nothing read back        -- the window form of the kernels
       8 stripes rehearsed on one GPU in lockstep, rounds of at most --passes passes, one row of `out` copied and the vote
       taken in process and read back after every round, which the time includes
     with rounds and the passes that did work in every round (the largest over the stripes; from an untimed run that reads
     the status word after every call).
     The bar for "one stripe": it does the tile entry's passes plus one all-tiles quiet pass and the round launches, so its
     time over the tile entry's is compared with the same ratio of the drainage stage in the same run --
     nz_drainage_stripe_round (a round with `first`, a quiet round, finalise) over nz_drainage_area -- times 1.25: the pass
     carries two more coefficient planes, and the margin covers run-to-run spread.
  2. The chain fill -> drainage -> solve at dt 100: the three tile entries beside 8 lockstep stripes (run_fill_lockstep,
     run_fluvial_implicit_lockstep), bits compared.
usage: bench_fluvial_implicit_stripe.py [--res 4096] [--reps 7] [--warmup 3] [--passes 64] [--skip-chain]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noize_job_amd as nj  # noqa: E402
from noize_job_amd import sharded as sh  # noqa: E402

OFF = nj.FluvialErosionStage.SEA_OFF
EPS = 1e-4
MARGIN = 1.25


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=64)
    ap.add_argument("--skip-chain", action="store_true")
    a = ap.parse_args()
    N = nj._native
    res, budget, world = a.res, 64 + a.res // 4, 8
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = nj.Context(0, stream=stream.cuda_stream)
        ops = sh.HipStripeOps(ctx)
        dev = lambda *shape: torch.empty(shape, device="cuda")  # noqa: E731
        words = lambda: torch.zeros(3, dtype=torch.int32, device="cuda")  # noqa: E731
        sized = lambda entry, pl: dev(getattr(N.lib, entry)(C.byref(pl.stripe())))  # noqa: E731
        raw, filled, area, out = dev(res, res), dev(res, res), dev(res, res), dev(res, res)
        ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), raw.data_ptr(), res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700, handle=False)
        work_fill = dev(N.lib.nz_fill_depressions_work_floats(res, 1))
        work_area = dev(N.lib.nz_drainage_area_work_floats(res, 1))
        work_solve = dev(N.lib.nz_fluvial_implicit_work_floats(res, 1))
        fill_desc = N.FillDesc(EPS, OFF, budget, None)
        area_desc = N.DrainageDesc(1.0, OFF, budget, None)
        solve_desc = lambda dt: N.FluvialImplicitDesc(0.05, 0.002, dt, OFF, budget, None, None, None, None)  # noqa: E731
        filled.copy_(raw)
        ctx.call("nz_fill_depressions", filled.data_ptr(), work_fill.data_ptr(), C.byref(fill_desc), res, handle=False)
        ctx.call("nz_drainage_area", filled.data_ptr(), area.data_ptr(), work_area.data_ptr(), C.byref(area_desc), res, handle=False)

        def copy_rows(dst, d0, src, s0, n):
            dst[d0:d0 + n].copy_(src[s0:s0 + n])

        def sample(reset, fn):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def measure(variants):
            for _ in range(a.warmup):
                for _, reset, fn in variants:
                    sample(reset, fn)
            ms = [[] for _ in variants]
            for _ in range(a.reps):
                for k, (_, reset, fn) in enumerate(variants):
                    ms[k].append(sample(reset, fn))
            return ms

        def line(name, m, base=None):
            md = float(np.median(m))
            return "  %-36s %8.3f ms  [%.3f, %.3f]%s" % (name, md, min(m), max(m), "" if base is None else "  x%.3f" % (md / base))

        status = lambda work: work[0:2].view(torch.int32).tolist()  # noqa: E731
        nothing = lambda: None  # noqa: E731  (the inputs are read only: no sample has anything to put back)

        # ---- 1. the solve on the filled tile ----
        def make(n):
            plans = [sh.StripePlan(r, n, res, res, 1 if n > 1 else 0) for r in range(n)]  # one stripe: no cut, no ghost row
            bufs = []
            for pl in plans:
                b = dict(H=dev(pl.rows, res), A=dev(pl.rows, res), out=dev(pl.rows, res),
                         work=sized("nz_implicit_fluvial_stripe_work_floats", pl), words=words())
                b["H"][pl.own0:pl.own1].copy_(filled[pl.g0:pl.g0 + pl.nown])
                b["A"][pl.own0:pl.own1].copy_(area[pl.g0:pl.g0 + pl.nown])
                bufs.append(b)
            # the heights' ghost rows once: they do not change between samples
            sh._copy_ghost_rows([([b["H"]], 1, 1) for b in bufs], plans, copy_rows)
            return plans, bufs

        sets = {1: make(1), world: make(world)}
        (pl1,), (b1,) = sets[1]
        drain1 = dict(A=dev(pl1.rows, res), work=sized("nz_drainage_stripe_work_floats", pl1), words=words())

        def one_stripe(dt):
            prm = dict(sh.FLUVIAL_IMPLICIT_DEFAULTS, dt=dt, maxPasses=budget)
            w = b1["words"]
            ops.fluvial_implicit(b1["H"], b1["A"], b1["out"], b1["work"], pl1, prm, True, None, w[0:1])
            ops.fluvial_implicit(b1["H"], b1["A"], b1["out"], b1["work"], pl1, prm, False, w[0:1], w[1:2])
            ops.fluvial_implicit_finalise(b1["H"], b1["out"], pl1, w[2:3])

        def drainage_one_stripe():
            prm = dict(sh.DRAINAGE_DEFAULTS, maxPasses=budget)
            w = drain1["words"]
            ops.drainage(b1["H"], drain1["A"], drain1["work"], pl1, prm, True, None, w[0:1])
            ops.drainage(b1["H"], drain1["A"], drain1["work"], pl1, prm, False, w[0:1], w[1:2])
            ops.drainage_finalise(drain1["A"], pl1, prm, w[2:3])

        def lockstep_solve(dt, passes, record=None):
            """The solve's rounds of fluvial_implicit_steps on 8 stripes, the drainage plane given -> rounds"""
            plans, bufs = sets[world]
            prm = dict(sh.FLUVIAL_IMPLICIT_DEFAULTS, dt=dt, maxPasses=passes)
            vote, rounds = 1, 0
            while vote != 0:
                if rounds:
                    sh._copy_ghost_rows([([b["out"]], 1, 1) for b in bufs], plans, copy_rows)
                k, kp = rounds & 1, (rounds - 1) & 1
                for pl, b in zip(plans, bufs):
                    ops.fluvial_implicit(b["H"], b["A"], b["out"], b["work"], pl, prm, rounds == 0,
                                         None if rounds == 0 else b["words"][kp:kp + 1], b["words"][k:k + 1])
                    if record is not None:
                        record.append(status(b["work"])[0])
                vote = max(int(b["words"][k]) for b in bufs)
                for b in bufs:
                    b["words"][k:k + 1].fill_(vote)
                rounds += 1
            for pl, b in zip(plans, bufs):
                b["words"][2:3].fill_(1)
                ops.fluvial_implicit_finalise(b["H"], b["out"], pl, b["words"][2:3])
            return rounds

        def tile_entry(dt):
            d = solve_desc(dt)
            ctx.call("nz_fluvial_implicit", filled.data_ptr(), area.data_ptr(), out.data_ptr(), work_solve.data_ptr(), C.byref(d),
                     res, handle=False)

        def tile_drainage():
            ctx.call("nz_drainage_area", filled.data_ptr(), drain1["A"].data_ptr(), work_area.data_ptr(), C.byref(area_desc), res,
                     handle=False)

        b1["words"][2:3].fill_(1)
        drain1["words"][2:3].fill_(1)
        print("implicit fluvial erosion of the filled 13-octave fBm tile, %d^2, %d samples, variants alternating" % (res, a.reps))
        for dt in (1.0, 100.0):
            variants = [("nz_fluvial_implicit, dt %g" % dt, nothing, lambda: tile_entry(dt)),
                        ("1 stripe: 2 rounds + finalise", nothing, lambda: one_stripe(dt)),
                        ("%d stripes in lockstep" % world, nothing, lambda: lockstep_solve(dt, a.passes)),
                        ("nz_drainage_area", nothing, tile_drainage),
                        ("drainage, 1 stripe: 2 rounds + finalise", nothing, drainage_one_stripe)]
            ms = measure(variants)
            tile_entry(dt)
            st = status(work_solve)
            base = float(np.median(ms[0]))
            print(line(variants[0][0], ms[0]) + "  passes %d, converged %d" % (st[0], st[1]), flush=True)
            one_stripe(dt)
            print(line(variants[1][0], ms[1], base) + "  changed %s, equal to the tile entry's bits %s" %
                  (b1["words"][:2].tolist(), torch.equal(b1["out"][pl1.own0:pl1.own1], out)))
            record = []
            rounds = lockstep_solve(dt, a.passes, record)
            per_round = [max(record[r * world:(r + 1) * world]) for r in range(rounds)]
            same = all(torch.equal(b["out"][pl.own0:pl.own1], out[pl.g0:pl.g0 + pl.nown]) for pl, b in zip(*sets[world]))
            print(line(variants[2][0], ms[2], base) + "  rounds %d of at most %d passes, equal to the tile entry's bits %s" %
                  (rounds, a.passes, same))
            print("    passes that did work, per round (largest over the stripes): %s" % per_round)
            dbase = float(np.median(ms[3]))
            print(line(variants[3][0], ms[3]) + "  passes %d, converged %d" % tuple(status(work_area)))
            print(line(variants[4][0], ms[4], dbase))
            ratio, dratio = float(np.median(ms[1])) / base, float(np.median(ms[4])) / dbase
            print("    bar: one stripe / tile entry = x%.3f against the drainage stage's x%.3f x %.2f = x%.3f: %s" %
                  (ratio, dratio, MARGIN, dratio * MARGIN, "met" if ratio <= dratio * MARGIN else "MISSED"), flush=True)
        sets.clear()

        # ---- 2. the chain ----
        if not a.skip_chain:
            dt = 100.0
            tile_h, tile_out = dev(res, res), dev(res, res)

            def tile_chain():
                d = solve_desc(dt)
                ctx.call("nz_fill_depressions", tile_h.data_ptr(), work_fill.data_ptr(), C.byref(fill_desc), res, handle=False)
                ctx.call("nz_drainage_area", tile_h.data_ptr(), area.data_ptr(), work_area.data_ptr(), C.byref(area_desc), res, handle=False)
                ctx.call("nz_fluvial_implicit", tile_h.data_ptr(), area.data_ptr(), tile_out.data_ptr(), work_solve.data_ptr(),
                         C.byref(d), res, handle=False)

            plans = [sh.StripePlan(r, world, res, res, 2) for r in range(world)]
            plane = lambda pl: dev(pl.rows, res)  # noqa: E731
            H = [plane(pl) for pl in plans]
            fill_bufs = [dict(H=t, W=plane(pl), work=sized("nz_fill_stripe_work_floats", pl), words=words()) for t, pl in zip(H, plans)]
            bufs = [dict(H=t, out=plane(pl), A=plane(pl), work=sized("nz_implicit_fluvial_stripe_work_floats", pl),
                         drainageWork=sized("nz_drainage_stripe_work_floats", pl), words=words()) for t, pl in zip(H, plans)]
            got = {}

            def reset_stripes():
                for t, pl in zip(H, plans):
                    t[pl.own0:pl.own1].copy_(raw[pl.g0:pl.g0 + pl.nown])

            def stripe_chain():
                rounds = dict(maxPasses=a.passes, maxRounds=100000)
                got["fill"] = sh.run_fill_lockstep([ops] * world, plans, dict(rounds, epsilon=EPS), fill_bufs, copy_rows)
                got["solve"] = sh.run_fluvial_implicit_lockstep([ops] * world, plans, dict(rounds, dt=dt), bufs, copy_rows)

            variants = [("tile chain", lambda: tile_h.copy_(raw), tile_chain), ("%d stripes, lockstep" % world, reset_stripes, stripe_chain)]
            ms = measure(variants)
            base = float(np.median(ms[0]))
            same = all(torch.equal(r[0][pl.own0:pl.own1], tile_out[pl.g0:pl.g0 + pl.nown]) and
                       torch.equal(r[1][pl.own0:pl.own1], area[pl.g0:pl.g0 + pl.nown]) for r, pl in zip(got["solve"], plans))
            print("fill -> drainage -> implicit solve at dt %g, %d^2, %d samples, variants alternating" % (dt, res, a.reps))
            print(line(variants[0][0], ms[0]))
            print(line(variants[1][0], ms[1], base) + "  fill rounds %d, solve rounds %d, steps %d, heights and drainage equal to the "
                  "tile chain's bits %s" % (got["fill"][0][2], got["solve"][0][3], got["solve"][0][2], same), flush=True)
        stream.synchronize()
        ctx.close()


if __name__ == "__main__":
    main()
