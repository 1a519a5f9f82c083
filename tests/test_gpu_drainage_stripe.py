"""The drainage area on row stripes on the GPU (nz_drainage_stripe_round, nz_drainage_stripe_finalise, HipStripeOps.drainage,
run_drainage_lockstep, nz_comm_allreduce_max_i32) against tests/drainage_ref.py, bit for bit: one stripe is the topological
walk on a rectangle; a square stripe followed by finalise is nz_drainage_area on the 16-byte and the 4-byte path; the ghost
rows of A are frozen; rows beyond them and the pitch pads are not touched; a proceed word of zero writes nothing; the sweep
cap does not matter; the filled grids over 2 to 16 stripes end at the walk, with a signed rain map and with a sea too; an
exhausted round budget is all or nothing on every stripe; the vote runs through the library's collective with a rank as
its own peer; fill -> drainage -> fluvial on stripes is the tile chain; refusals write nothing; planes carved from a
guarded slab.  Every buffer starts as NaN.  Budgets: drainage_stripe_cases.PARAMS."""
import ctypes as C
import multiprocessing as mp

import numpy as np
import pytest
import torch

import drainage_ref as D
from conftest import ROOT
from drainage_stripe_cases import (EPS, HALO, OFF, PARAMS, WORLDS, assert_bits, filled, lockstep, reference, signed_rain,
                                   stripe_bufs, stripe_ops, work_floats)
from fill_stripe_cases import pitted
from test_gpu_slab import PAIRS, carved
from test_hydraulic_stripe_ref import copy_rows

pytestmark = pytest.mark.gpu
f32 = np.float32
AMPLE = 400  # passes: no grid of the single-stripe tests has a flow path of 400 cells (a pass is at least a Jacobi step)


@pytest.fixture(scope="module")
def hip(nj):
    """fill_stripe_cases.stripe_ops, once for the module."""
    with stripe_ops(nj) as pair:
        yield pair


def one_stripe(hip, nj, h, params=None, pitch=None, rain_map=None, rounds=2, verdict=None):
    """The whole grid as one stripe: a round with `first`, a second round that takes its word as `proceed`, then finalise
    with the verdict "`changed` of the second round == 0" (or `verdict`) -> (A, the rounds' changed words, bufs)"""
    sh, ops = hip
    plan = sh.StripePlan(0, 1, h.shape[0], h.shape[1], 0)
    bufs = stripe_bufs(plan, h, work_floats(nj, pitch or 0)(plan), "cuda", pitch, rain_map)
    prm = dict(sh.DRAINAGE_DEFAULTS, **(params or dict(maxPasses=AMPLE)))
    words, maps = bufs["words"], dict(rainMap=bufs.get("rainMap"), pitch=pitch or 0)
    ops.drainage(bufs["H"], bufs["A"], bufs["work"], plan, prm, True, None, words[0:1], **maps)
    if rounds > 1:
        ops.drainage(bufs["H"], bufs["A"], bufs["work"], plan, prm, False, words[0:1], words[1:2], **maps)
    changed = words[:rounds].tolist()
    words[2:3].fill_(int(changed[-1] == 0) if verdict is None else verdict)
    ops.drainage_finalise(bufs["A"], plan, prm, words[2:3], **maps)
    return bufs["A"][:, :plan.cols].cpu().numpy(), changed, bufs


# 1. one stripe is the walk on a rectangle: the 4-byte path (333 columns) and the 16-byte one, odd and even pass budgets
@pytest.mark.parametrize("shape", [(70, 333), (333, 200), (64, 64)])
def test_one_stripe_is_the_walk_on_a_rectangle(hip, nj, shape):
    h = pitted(*shape)
    want, height = D.accumulate(h)
    assert height + 2 < AMPLE
    for passes in (AMPLE, AMPLE + 1):
        got, changed, _ = one_stripe(hip, nj, h, dict(maxPasses=passes))
        assert changed == [1, 0]
        assert_bits(got, want, "%s, %d passes" % (shape, passes))


# ... and on a square, followed by finalise, it is nz_drainage_area, device against device: 96 is the 16-byte path, 97 the
# 4-byte one; a pass budget that runs out in a single-round series followed by finalise(0) is the tile entry's rain_c
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("res", [96, 97])
def test_a_square_stripe_is_the_tile_entry(hip, nj, ctx, res, mapped):
    from test_gpu_drainage import run_gpu
    h = pitted(res, res)
    rm = signed_rain((res, res)) if mapped else None
    want, passes, converged = run_gpu(nj, ctx, h, 0.75, OFF, AMPLE, rm)
    assert converged == 1
    got, changed, bufs = one_stripe(hip, nj, h, dict(rain=0.75, maxPasses=AMPLE), rain_map=rm)
    assert changed == [1, 0]
    assert_bits(got, want, "drainage")
    assert_bits(got, D.accumulate(h, 0.75, OFF, rm)[0], "reference")
    assert int(bufs["work"][:1].view(torch.int32)[0]) == 1  # the status words of the round at rest: one pass looked
    short, _, tile_converged = run_gpu(nj, ctx, h, 0.75, OFF, 2, rm)
    assert tile_converged == 0
    got, changed, _ = one_stripe(hip, nj, h, dict(rain=0.75, maxPasses=2), rain_map=rm, rounds=1, verdict=0)
    assert changed == [1]
    assert_bits(got, short, "an exhausted budget: rain_c")


# 2. rank 1 of 3 with spare rows beyond the two ghost rows, a pitch on every plane (cols + 5: 4-byte path, cols + 8: 16-byte
# path): rounds against ghost rows put there by hand.  The ghost rows of A keep their bits, the rows beyond them and the
# pads keep their NaN, in A and in the work plane; heights and rain map are not written; a round at rest reports
# changed == 0; proceed == 0 writes nothing.  6 and 7 passes: both parities of the copy back
@pytest.mark.parametrize("pad", [5, 8])
@pytest.mark.parametrize("passes", [6, 7])
def test_ghost_rows_are_frozen_and_the_rest_is_untouched(hip, nj, pad, passes):
    sh, ops = hip
    h = filled("bowl")
    rm = signed_rain(h.shape)
    want = reference("bowl", 0.75, mapped=True)[0]
    rows, cols = h.shape
    pitch = cols + pad
    plan = sh.StripePlan(1, 3, rows, cols, pad)  # 5 and 8 rows on each side: 3 and 6 more than the heights need
    bufs = stripe_bufs(plan, h, work_floats(nj, pitch)(plan), "cuda", pitch, rm)
    lo, hi = plan.own0 - 1, plan.own1 + 1
    put = lambda t, a, n: t[plan.own0 - n:plan.own1 + n, :cols].copy_(  # noqa: E731
        torch.from_numpy(np.ascontiguousarray(a[plan.g0 - n:plan.g0 + plan.nown + n])))
    put(bufs["H"], h, 2)
    put(bufs["rainMap"], rm, 1)
    before = {k: bufs[k].clone() for k in ("H", "rainMap")}
    prm = dict(sh.DRAINAGE_DEFAULTS, rain=0.75, maxPasses=passes)
    words = bufs["words"]
    call = lambda first, proceed, changed: ops.drainage(bufs["H"], bufs["A"], bufs["work"], plan, prm, first, proceed,  # noqa: E731
                                                        changed, rainMap=bufs["rainMap"], pitch=pitch)
    call(True, None, words[0:1])
    assert int(words[0]) == 1
    # later rounds against the walk's own rows as ghost rows: the stripe ends at the walk's floats
    ghost = torch.from_numpy(np.ascontiguousarray(want[[plan.grow0 + lo, plan.grow0 + hi - 1]])).cuda()
    bufs["A"][lo, :cols], bufs["A"][hi - 1, :cols] = ghost[0], ghost[1]
    for r in range(1, 200):
        call(False, words[(r - 1) & 1:((r - 1) & 1) + 1], words[r & 1:(r & 1) + 1])
        if int(words[r & 1]) == 0:
            break
    assert 1 < r < 199, r
    A = bufs["A"].cpu().numpy()
    assert_bits(A[plan.own0:plan.own1, :cols], want[plan.g0:plan.g0 + plan.nown], "the stripe's A")
    assert_bits(A[[lo, hi - 1], :cols], ghost.cpu().numpy(), "ghost rows of a")
    work = bufs["work"].cpu().numpy()
    plane = work[work.size - plan.rows * pitch:].reshape(plan.rows, pitch)
    for what, t in (("a", A), ("work plane", plane)):
        assert np.isnan(t[:, cols:]).all(), "%s: pad floats" % what
        assert np.isnan(t[:lo]).all() and np.isnan(t[hi:]).all(), "%s: rows beyond the ghost row" % what
    assert np.isnan(plane[lo]).all() and np.isnan(plane[hi - 1]).all(), "the work plane's ghost rows"
    # proceed == 0 (the word of the round at rest): nothing is written, changed == 0 -- even with `first`
    kept = bufs["A"].clone()
    words[2:3].fill_(-7)
    call(True, words[r & 1:(r & 1) + 1], words[2:3])
    assert int(words[2]) == 0
    assert_bits(bufs["A"].cpu().numpy(), kept.cpu().numpy(), "a after proceed == 0")
    call(False, None, words[2:3])  # ... and the donor bytes are still those of the first round
    assert int(words[2]) == 0
    assert_bits(bufs["A"].cpu().numpy(), kept.cpu().numpy(), "a after one more round at rest")
    for k in before:
        assert_bits(bufs[k].cpu().numpy(), before[k].cpu().numpy(), k)


# 3. the sweep cap does not change the floats, alone or over stripes
def test_sweep_caps_give_equal_bits(hip, nj):
    sh, ops = hip
    lib = nj._native.lib
    try:
        for sweeps in (1, 2, 16, 200):
            lib.nz_debug_drainage_sweeps(sweeps)
            got, changed, _ = one_stripe(hip, nj, filled("bowl"))
            assert changed == [1, 0]
            assert_bits(got, reference("bowl")[0], "one stripe, %d sweeps" % sweeps)
            got, rounds, converged, _, _ = lockstep(sh, ops, 8, filled("pitted"), PARAMS, work_floats(nj), "cuda")
            assert converged
            assert_bits(got, reference("pitted")[0], "8 stripes, %d sweeps" % sweeps)
    finally:
        lib.nz_debug_drainage_sweeps(0)


# 4. the stripes end at the walk of the whole grid; (33, 130) over 16 ranks are stripes of 2 and 3 rows
@pytest.mark.parametrize("name,world", [(n, w) for n in ("pitted", "bowl", "serpentine") for w in WORLDS] + [("wide", 16)])
def test_stripes_equal_the_walk(hip, nj, name, world):
    sh, ops = hip
    got, rounds, converged, _, _ = lockstep(sh, ops, world, filled(name), PARAMS, work_floats(nj), "cuda")
    print("%s world %d: %d rounds" % (name, world, rounds))
    assert converged and 2 <= rounds <= 128
    assert_bits(got, reference(name)[0], "%s world %d" % (name, world))


def test_a_signed_rain_map_over_stripes(hip, nj):
    sh, ops = hip
    h = filled("pitted")
    got, _, converged, _, _ = lockstep(sh, ops, 8, h, dict(PARAMS, rain=0.75), work_floats(nj), "cuda", signed_rain(h.shape))
    assert converged
    assert_bits(got, reference("pitted", 0.75, mapped=True)[0], "signed rain map")


def test_a_sea_level_over_stripes(hip, nj):
    sh, ops = hip
    h = filled("pitted")
    sea = float(np.quantile(h, 0.3))
    got, _, converged, _, _ = lockstep(sh, ops, 8, h, dict(PARAMS, seaLevel=sea), work_floats(nj), "cuda")
    assert converged
    assert_bits(got, D.accumulate(h, 1.0, sea)[0], "sea level")


# 5. all or nothing: 10 rounds against the 58 the serpentine needs over 8 stripes leave rain_c on every stripe
def test_an_exhausted_round_budget_is_all_or_nothing(hip, nj):
    sh, ops = hip
    h = filled("serpentine")
    rm = signed_rain(h.shape)
    rc = (f32(2.0) * rm).astype(f32)
    got, rounds, converged, plans, bufs = lockstep(sh, ops, 8, h, dict(PARAMS, rain=2.0, maxRounds=10), work_floats(nj),
                                                   "cuda", rm)
    assert (rounds, converged) == (10, False)
    assert_bits(got, rc, "rain_c")
    for pl, b in zip(plans, bufs):
        A = b["A"].cpu().numpy()
        assert_bits(A[pl.own0:pl.own1], rc[pl.g0:pl.g0 + pl.nown], "rank %d" % pl.rank)
        lo, hi = max(pl.own0 - 1, -pl.grow0), min(pl.own1 + 1, pl.grows - pl.grow0)
        assert np.isnan(A[:lo]).all() and np.isnan(A[hi:]).all(), "rank %d: rows beyond the ghost row" % pl.rank


# 6. the vote through nz_comm_allreduce_max_i32, a rank as its own peer, in a child process like every RCCL test
def _rccl_worker(out_path):
    import sys
    sys.path.insert(0, ROOT)
    import noize_job_amd as nj
    from noize_job_amd import sharded as sh
    ctx = nj.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    comm = sh.NativeComm(ctx, sh.NativeComm.unique_id(), 0, 1)
    h = filled("bowl")
    plan = sh.StripePlan(0, 1, h.shape[0], h.shape[1], HALO)
    bufs = stripe_bufs(plan, h, nj._native.lib.nz_drainage_stripe_work_floats(C.byref(plan.stripe())), "cuda")
    A, rounds, converged = sh.run_drainage(sh.HipStripeOps(ctx), comm, plan, PARAMS, bufs)
    np.savez(out_path, rounds=rounds, converged=converged, A=A[plan.own0:plan.own1].cpu().numpy())
    torch.cuda.synchronize()
    comm.close()
    ctx.close()


def test_the_vote_runs_through_the_collective(tmp_path):
    out = str(tmp_path / "vote.npz")
    proc = mp.get_context("spawn").Process(target=_rccl_worker, args=(out,))
    proc.start()
    proc.join(240)
    if proc.is_alive():
        proc.kill()
        proc.join()
        pytest.fail("the RCCL worker did not finish within 240 s")
    assert proc.exitcode == 0
    got = np.load(out)
    assert bool(got["converged"]) and int(got["rounds"]) == 2  # one stripe: a round of work, a round at rest
    assert_bits(got["A"], reference("bowl")[0], "run_drainage through NativeComm")


# 7. the chain the README shows, on stripes: fill -> drainage -> fluvial with the A plane as drainageIn, three ranks, is
# nz_fill_depressions -> nz_drainage_area -> nz_fluvial_erosion(drainageIn) on the tile, heights and drainage
def test_the_chain_on_stripes_is_the_chain_on_the_tile(hip, nj, ctx):
    from test_gpu_drainage import run_gpu as tile_drainage
    from test_gpu_fill import run_gpu as tile_fill
    from test_gpu_fluvial import run_gpu as tile_fluvial
    sh, ops = hip
    N = nj._native
    h = pitted(96, 96)
    its, every, world = 6, 2, 3
    prm = [sh.FLUVIAL_DEFAULTS[k] for k in sh.FLUVIAL_SCALARS]
    hf, _, _, ok = tile_fill(nj, ctx, h, eps=EPS, depth=True)
    A, _, ok2 = tile_drainage(nj, ctx, hf)
    assert ok == 1 and ok2 == 1
    want = tile_fluvial(nj, ctx, hf, its, prm, drainageIn=A)
    plans = [sh.StripePlan(r, world, 96, 96, sh.fluvial_halo_rows(every)) for r in range(world)]
    full = lambda *shape: torch.full(shape, float("nan"), device="cuda")  # noqa: E731
    words = lambda: torch.full((3,), -7, dtype=torch.int32, device="cuda")  # noqa: E731
    sized = lambda entry, pl: full(getattr(N.lib, entry)(C.byref(pl.stripe())))  # noqa: E731
    H = [stripe_bufs(pl, h, 0, "cuda")["H"] for pl in plans]
    fill = sh.run_fill_lockstep([ops] * world, plans, dict(epsilon=EPS, maxPasses=400, maxRounds=400),
                                [dict(H=t, W=full(pl.rows, pl.cols), work=sized("nz_fill_stripe_work_floats", pl), words=words())
                                 for t, pl in zip(H, plans)], copy_rows)
    assert all(r[3] for r in fill)
    area = sh.run_drainage_lockstep([ops] * world, plans, PARAMS,
                                    [dict(H=t, A=full(pl.rows, pl.cols), work=sized("nz_drainage_stripe_work_floats", pl),
                                          words=words()) for t, pl in zip(H, plans)], copy_rows)
    assert all(r[2] for r in area)
    res = sh.run_fluvial_lockstep([ops] * world, plans, dict(iterations=its),
                                  [dict(A=t, B=full(pl.rows, pl.cols), D0=full(pl.rows, pl.cols), D1=full(pl.rows, pl.cols),
                                        work=full(2, pl.rows, pl.cols), drainageIn=a[0]) for t, a, pl in zip(H, area, plans)],
                                  copy_rows, exchange_every=every)
    rows = lambda t, pl: t[pl.own0:pl.own1, :pl.cols].cpu().numpy()  # noqa: E731
    for k, what in enumerate(("heights", "drainage")):
        assert_bits(np.concatenate([rows(r[k], pl) for r, pl in zip(res, plans)]), want[k], what)
    assert_bits(np.concatenate([rows(a[0], pl) for a, pl in zip(area, plans)]), A, "the river map before erosion")


# 8. refusals: NZ_ERR_INVALID, and nothing is written -- one per clause of the contract
def test_refusals_write_nothing(hip, nj):
    sh, ops = hip
    N = nj._native
    h = filled("bowl")
    plan = sh.StripePlan(1, 3, h.shape[0], h.shape[1], HALO)
    bufs = stripe_bufs(plan, h, work_floats(nj)(plan), "cuda", rain_map=signed_rain(h.shape))
    bufs["H"][:] = torch.from_numpy(np.ascontiguousarray(h[plan.grow0:plan.grow0 + plan.rows])).cuda()
    st = plan.stripe()
    Hp, Ap, Kp, Rp = (bufs[k].data_ptr() for k in ("H", "A", "work", "rainMap"))
    w0, w1, w2 = (bufs["words"][i:i + 1].data_ptr() for i in range(3))
    row = 4 * plan.cols

    def desc(rain=1.0, sea=OFF, passes=10, rm=None):
        return N.DrainageDesc(rain, sea, passes, rm)

    def refused(entry, name, *args):
        with pytest.raises(nj.NoizeError) as e:
            ops.ctx.call(entry, *args)
        assert e.value.status == N.NZ_ERR_INVALID and name in str(e.value), (name, str(e.value))

    def rnd(name, hp, ap, kp, stripe, d, first=1, proceed=None, changed=w0):
        refused("nz_drainage_stripe_round", name, hp, ap, kp, C.byref(stripe), d if d is None else C.byref(d), first, proceed, changed)

    rnd("rain", Hp, Ap, Kp, st, desc(rain=float("nan")))
    rnd("rain", Hp, Ap, Kp, st, desc(rain=-1.0))
    rnd("seaLevel", Hp, Ap, Kp, st, desc(sea=float("inf")))
    rnd("maxPasses", Hp, Ap, Kp, st, desc(passes=0))
    rnd("desc", Hp, Ap, Kp, st, None)
    rnd("height", None, Ap, Kp, st, desc())
    rnd("a is NULL", Hp, None, Kp, st, desc())
    rnd("work", Hp, Ap, None, st, desc())
    rnd("changed", Hp, Ap, Kp, st, desc(), changed=None)
    one = sh.StripePlan(1, 3, h.shape[0], h.shape[1], 1).stripe()
    rnd("ghost rows", Hp, Ap, Kp, one, desc())                                        # the heights need 2 with `first`
    rnd("ghost rows", Hp, Ap, Kp, sh.StripePlan(1, 3, h.shape[0], h.shape[1], 0).stripe(), desc(), first=0)  # A needs 1
    rnd("a overlaps height", Hp, Hp + row, Kp, st, desc())
    rnd("a overlaps rainMap", Hp, Ap, Kp, st, desc(rm=Ap + row))
    rnd("a overlaps work", Hp, Ap, Ap + 64, st, desc())
    rnd("work overlaps height", Kp + 64, Ap, Kp, st, desc())
    rnd("work overlaps rainMap", Hp, Ap, Kp, st, desc(rm=Kp + 64))
    rnd("changed overlaps a", Hp, Ap, Kp, st, desc(), changed=Ap + row)
    rnd("changed overlaps work", Hp, Ap, Kp, st, desc(), changed=Kp)
    rnd("proceed overlaps a", Hp, Ap, Kp, st, desc(), proceed=Ap + 8)
    rnd("changed overlaps proceed", Hp, Ap, Kp, st, desc(), proceed=w0)

    def fin(name, ap, d, word):
        refused("nz_drainage_stripe_finalise", name, ap, C.byref(st), d if d is None else C.byref(d), word)

    fin("converged", Ap, desc(), None)
    fin("a is NULL", None, desc(), w2)
    fin("desc", Ap, None, w2)
    fin("rain", Ap, desc(rain=float("inf")), w2)
    fin("a overlaps rainMap", Ap, desc(rm=Ap + row), w2)
    fin("converged overlaps a", Ap, desc(), Ap + row)
    torch.cuda.current_stream().synchronize()
    for name in ("A", "work"):
        assert np.isnan(bufs[name].cpu().numpy()).all(), name
    assert bufs["words"].tolist() == [-7, -7, -7]
    assert_bits(bufs["H"].cpu().numpy(), h[plan.grow0:plan.grow0 + plan.rows], "height")
    # a round without `first` makes do with one ghost row (behind a proceed word of 0 it is accepted and writes `changed`)
    bufs["words"][1:2].fill_(0)
    ops.ctx.call("nz_drainage_stripe_round", Hp, Ap, Kp, C.byref(one), C.byref(desc()), 0, w1, w0).Complete()
    assert bufs["words"].tolist() == [0, 0, -7] and np.isnan(bufs["A"].cpu().numpy()).all()
    assert N.lib.nz_drainage_stripe_halo_rows() == 2 == HALO
    cells = plan.rows * plan.cols
    assert N.lib.nz_drainage_stripe_work_floats(C.byref(st)) > cells + cells // 4  # one plane and the donor bytes


# 9. planes carved from one guarded allocation at four alignments and three mixed pairs: the guards stay silent, the floats
# are the walk's.  70 x 100 takes the 16-byte path where every plane is aligned, 70 x 97 never does
@pytest.mark.parametrize("cols", [100, 97])
def test_on_slab_carved_planes(nj, ctx, cols):
    rows = 70
    h = pitted(rows, cols)
    rm = signed_rain((rows, cols))
    want = D.accumulate(h, 0.75, OFF, rm)[0]
    n = rows * cols
    st = nj._native.Stripe(cols, rows, 0, rows, 0, rows, 0)
    nwork = nj._native.lib.nz_drainage_stripe_work_floats(C.byref(st))
    start = np.array([-7, -7, 1], np.int32)
    for passes in (AMPLE, AMPLE + 1):
        for p, q in PAIRS:
            r = p if p == q else (q + 1) % 4
            with carved(ctx, cols, height=(n, p, h), a=(n, q, None), work=(nwork, r, None), rain=(n, q, rm),
                        words=(3, p, start, np.int32)) as (s, t):
                desc = nj._native.DrainageDesc(0.75, OFF, passes, t.rain.ptr)
                ctx.call("nz_drainage_stripe_round", t.height.ptr, t.a.ptr, t.work.ptr, C.byref(st), C.byref(desc), 1, None, t.words.ptr)
                ctx.call("nz_drainage_stripe_round", t.height.ptr, t.a.ptr, t.work.ptr, C.byref(st), C.byref(desc), 0, t.words.ptr,
                         t.words.ptr + 4)
                ctx.call("nz_drainage_stripe_finalise", t.a.ptr, C.byref(st), C.byref(desc), t.words.ptr + 8).Complete()
                assert t.words.ToArray().tolist() == [1, 0, 1], (p, q)
                assert_bits(t.a.ToArray((rows, cols)), want, (cols, passes, p, q))
                assert_bits(t.height.ToArray((rows, cols)), h, "height")
                s.check()
