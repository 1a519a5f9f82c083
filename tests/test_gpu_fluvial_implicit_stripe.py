"""Implicit fluvial erosion on row stripes on the GPU (nz_implicit_fluvial_stripe_round, nz_implicit_fluvial_stripe_finalise,
HipStripeOps.fluvial_implicit, run_fluvial_implicit_lockstep, nz_comm_allreduce_max_i32) against
tests/fluvial_implicit_ref.py, bit for bit: one stripe is the walk on a rectangle; a square stripe with a quiet second round
and finalise is nz_fluvial_implicit on the 16-byte and the 4-byte path; the ghost rows of `out` are frozen; rows beyond them
and the pitch pads are not touched; a proceed word of zero writes nothing; the sweep cap does not matter; the filled grids
over 2 to 16 stripes end at the walk in no more rounds than the CPU restatement, with a sea and with both maps too; an
exhausted round budget is all or nothing on every stripe; the vote runs through the library's collective with a rank as its
own peer; fill -> drainage -> solve on stripes is the tile chain; refusals write nothing; planes carved from a guarded slab;
the C++ mirror.  Every buffer starts as NaN.  Budgets: fluvial_implicit_stripe_cases.PARAMS."""
import ctypes as C
import multiprocessing as mp
import os
import subprocess

import numpy as np
import pytest
import torch

import drainage_ref as D
import fluvial_implicit_ref as R
from conftest import ROOT
from fill_stripe_cases import EPS, grid, pitted
from fluvial_implicit_stripe_cases import (CASES, DT, HALO, OFF, PARAMS, area, assert_bits, cpu_rounds, drain_floats, filled,
                                           hard_map, lockstep, reference, stripe_bufs, stripe_ops, uplift_map, work_floats)
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


def one_stripe(hip, nj, h, A, params=None, pitch=None, rounds=2, verdict=None, **maps):
    """The whole grid as one stripe: a round with `first`, a second round that takes its word as `proceed`, then finalise
    with the verdict "`changed` of the second round == 0" (or `verdict`) -> (h', the rounds' changed words, bufs)"""
    sh, ops = hip
    plan = sh.StripePlan(0, 1, h.shape[0], h.shape[1], 0)
    bufs = stripe_bufs(plan, h, work_floats(nj, pitch or 0)(plan), 0, "cuda", pitch, A, **maps)
    prm = dict(sh.FLUVIAL_IMPLICIT_DEFAULTS, **(params or dict(maxPasses=AMPLE, dt=DT)))
    words = bufs["words"]
    kw = dict(pitch=pitch or 0, **{k: bufs[k] for k in maps})
    ops.fluvial_implicit(bufs["H"], bufs["A"], bufs["out"], bufs["work"], plan, prm, True, None, words[0:1], **kw)
    if rounds > 1:
        ops.fluvial_implicit(bufs["H"], bufs["A"], bufs["out"], bufs["work"], plan, prm, False, words[0:1], words[1:2], **kw)
    changed = words[:rounds].tolist()
    words[2:3].fill_(int(changed[-1] == 0) if verdict is None else verdict)
    ops.fluvial_implicit_finalise(bufs["H"], bufs["out"], plan, words[2:3], pitch=pitch or 0)
    return bufs["out"][:, :plan.cols].cpu().numpy(), changed, bufs


# 1. one stripe is the walk on a rectangle: the 4-byte path (333 columns) and the 16-byte one, odd and even pass budgets
@pytest.mark.parametrize("shape", [(70, 333), (333, 200), (64, 64)])
def test_one_stripe_is_the_walk_on_a_rectangle(hip, nj, shape):
    h = pitted(*shape)  # pits and all: they rise by du
    A, height = D.accumulate(h)
    assert height + 2 < AMPLE
    want = R.walk(h, A, dt=DT)
    for passes in (AMPLE, AMPLE + 1):
        got, changed, _ = one_stripe(hip, nj, h, A, dict(maxPasses=passes, dt=DT))
        assert changed == [1, 0]
        assert_bits(got, want, "%s, %d passes" % (shape, passes))


# ... and on a square, with a quiet second round and finalise(1), it is nz_fluvial_implicit, device against device: 96 is the
# 16-byte path, 97 the 4-byte one; a pass budget that runs out in a single-round series followed by finalise(0) is the
# tile entry's "nothing", the heights
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("res", [96, 97])
def test_a_square_stripe_is_the_tile_entry(hip, nj, ctx, res, mapped):
    from test_gpu_fluvial_implicit import run_gpu
    h = pitted(res, res)  # pits and all: they rise by du
    A = D.accumulate(h)[0]
    maps = dict(hardness=hard_map((res, res)), upliftMap=uplift_map((res, res))) if mapped else {}
    want, passes, converged = run_gpu(nj, ctx, h, A, AMPLE, dt=DT, erodibility=0.1, **maps)
    assert converged == 1
    got, changed, bufs = one_stripe(hip, nj, h, A, dict(maxPasses=AMPLE, dt=DT, erodibility=0.1), **maps)
    assert changed == [1, 0]
    assert_bits(got, want, "the tile entry")
    assert_bits(got, R.walk(h, A, dt=DT, erodibility=0.1, **maps), "reference")
    assert int(bufs["work"][:1].view(torch.int32)[0]) == 1  # the status words of the round at rest: one pass looked
    short, _, tile_converged = run_gpu(nj, ctx, h, A, 2, dt=DT, erodibility=0.1, **maps)
    assert tile_converged == 0
    got, changed, _ = one_stripe(hip, nj, h, A, dict(maxPasses=2, dt=DT, erodibility=0.1), rounds=1, verdict=0, **maps)
    assert changed == [1]
    assert_bits(got, short, "an exhausted budget: the heights")
    assert_bits(got, h, "the heights")


# 2. rank 1 of 3 with spare rows beyond the ghost row, a pitch on every plane (cols + 5: 4-byte path, cols + 8: 16-byte path):
# rounds against ghost rows put there by hand.  23 owned rows end inside a 64 x 16 tile.  The ghost rows of `out` keep their
# bits, the rows beyond them and the pads keep their NaN, in `out` and in the work planes; heights, drainage and maps are not
# written; a round at rest reports changed == 0; proceed == 0 writes nothing.  6 and 7 passes: both parities of the copy back
@pytest.mark.parametrize("pad", [5, 8])
@pytest.mark.parametrize("passes", [6, 7])
def test_ghost_rows_are_frozen_and_the_rest_is_untouched(hip, nj, pad, passes):
    sh, ops = hip
    h = filled("bowl")
    maps = dict(hardness=hard_map(h.shape), upliftMap=uplift_map(h.shape))
    want = reference("bowl", DT, mapped=True)
    rows, cols = h.shape
    pitch = cols + pad
    plan = sh.StripePlan(1, 3, rows, cols, pad)  # 5 and 8 rows on each side: 4 and 7 more than the solve needs
    assert plan.nown % 16 != 0
    bufs = stripe_bufs(plan, h, work_floats(nj, pitch)(plan), 0, "cuda", pitch, area("bowl"), **maps)
    lo, hi = plan.own0 - 1, plan.own1 + 1
    ghost_h = torch.from_numpy(np.ascontiguousarray(h[[plan.grow0 + lo, plan.grow0 + hi - 1]])).cuda()
    bufs["H"][lo, :cols], bufs["H"][hi - 1, :cols] = ghost_h[0], ghost_h[1]  # ONE ghost row of the heights, none of A or a map
    before = {k: bufs[k].clone() for k in ("H", "A", "hardness", "upliftMap")}
    prm = dict(sh.FLUVIAL_IMPLICIT_DEFAULTS, dt=DT, maxPasses=passes)
    words = bufs["words"]
    call = lambda first, proceed, changed: ops.fluvial_implicit(  # noqa: E731
        bufs["H"], bufs["A"], bufs["out"], bufs["work"], plan, prm, first, proceed, changed, hardness=bufs["hardness"],
        upliftMap=bufs["upliftMap"], pitch=pitch)
    call(True, None, words[0:1])
    assert int(words[0]) == 1
    out = bufs["out"].cpu().numpy()
    assert np.isnan(out[lo]).all() and np.isnan(out[hi - 1]).all(), "a round with `first` does not touch out's ghost rows"
    assert not np.isnan(out[plan.own0:plan.own1, :cols]).any()
    # later rounds against the walk's own rows as ghost rows: the stripe ends at the walk's floats
    ghost = torch.from_numpy(np.ascontiguousarray(want[[plan.grow0 + lo, plan.grow0 + hi - 1]])).cuda()
    bufs["out"][lo, :cols], bufs["out"][hi - 1, :cols] = ghost[0], ghost[1]
    for r in range(1, 200):
        call(False, words[(r - 1) & 1:((r - 1) & 1) + 1], words[r & 1:(r & 1) + 1])
        if int(words[r & 1]) == 0:
            break
    assert 1 < r < 199, r
    out = bufs["out"].cpu().numpy()
    assert_bits(out[plan.own0:plan.own1, :cols], want[plan.g0:plan.g0 + plan.nown], "the stripe's h'")
    assert_bits(out[[lo, hi - 1], :cols], ghost.cpu().numpy(), "ghost rows of out")
    assert np.isnan(out[:, cols:]).all(), "out: pad floats"
    assert np.isnan(out[:lo]).all() and np.isnan(out[hi:]).all(), "out: rows beyond the ghost row"
    work = bufs["work"].cpu().numpy()
    n = plan.rows * pitch
    for k, what in enumerate(("h' work plane", "f", "b")):  # the three float planes at the end of `work`, last first
        plane = work[work.size - (k + 1) * n:work.size - k * n].reshape(plan.rows, pitch)
        assert np.isnan(plane[:, cols:]).all(), "%s: pad floats" % what
        assert np.isnan(plane[:plan.own0]).all() and np.isnan(plane[plan.own1:]).all(), "%s: rows beyond the owned ones" % what
        assert not np.isnan(plane[plan.own0:plan.own1, :cols]).any(), what
    # proceed == 0 (the word of the round at rest): nothing is written, changed == 0 -- even with `first`
    kept = bufs["out"].clone()
    words[2:3].fill_(-7)
    call(True, words[r & 1:(r & 1) + 1], words[2:3])
    assert int(words[2]) == 0
    assert_bits(bufs["out"].cpu().numpy(), kept.cpu().numpy(), "out after proceed == 0")
    call(False, None, words[2:3])  # ... and the coefficients are still those of the first round
    assert int(words[2]) == 0
    assert_bits(bufs["out"].cpu().numpy(), kept.cpu().numpy(), "out after one more round at rest")
    for k in before:
        assert_bits(bufs[k].cpu().numpy(), before[k].cpu().numpy(), k)


# 3. the sweep cap does not change the floats, alone or over stripes
def test_sweep_caps_give_equal_bits(hip, nj):
    sh, ops = hip
    lib = nj._native.lib
    try:
        for sweeps in (1, 3, 16, 200):
            lib.nz_debug_fluvial_implicit_sweeps(sweeps)
            got, changed, _ = one_stripe(hip, nj, filled("bowl"), area("bowl"))
            assert changed == [1, 0]
            assert_bits(got, reference("bowl"), "one stripe, %d sweeps" % sweeps)
            got, _, steps, _, converged, _, _ = lockstep(sh, ops, 8, filled("pitted"), dict(PARAMS, dt=DT), work_floats(nj),
                                                         drain_floats(nj), "cuda")
            assert converged and steps == 1
            assert_bits(got, reference("pitted"), "8 stripes, %d sweeps" % sweeps)
    finally:
        lib.nz_debug_fluvial_implicit_sweeps(0)


# 4. the stripes end at the walk of the whole grid, in the rounds of the CPU restatement or fewer; (33, 130) over 16 ranks are
# stripes of 2 and 3 rows
@pytest.mark.parametrize("name,world,dt", CASES)
def test_stripes_equal_the_walk(hip, nj, name, world, dt):
    sh, ops = hip
    got, A, steps, rounds, converged, _, _ = lockstep(sh, ops, world, filled(name), dict(PARAMS, dt=dt), work_floats(nj),
                                                      drain_floats(nj), "cuda")
    print("%s world %d dt %g: %d rounds (CPU restatement: %d)" % (name, world, dt, rounds, cpu_rounds(name, world, dt)[0]))
    assert converged and steps == 1 and 2 <= rounds <= cpu_rounds(name, world, dt)[0]
    assert_bits(A, area(name), "%s world %d: the drainage area" % (name, world))
    assert_bits(got, reference(name, dt), "%s world %d dt %g" % (name, world, dt))


def test_a_sea_level_over_stripes(hip, nj):
    sh, ops = hip
    h = filled("pitted")
    sea = float(np.quantile(h, 0.3))
    got, _, steps, _, converged, _, _ = lockstep(sh, ops, 8, h, dict(PARAMS, dt=DT, seaLevel=sea), work_floats(nj),
                                                 drain_floats(nj), "cuda")
    assert converged and steps == 1
    assert_bits(got, reference("pitted", DT, sea), "sea level")


def test_hardness_and_uplift_maps_over_stripes(hip, nj):
    sh, ops = hip
    h = filled("bowl")
    got, _, steps, _, converged, _, _ = lockstep(sh, ops, 8, h, dict(PARAMS, dt=DT), work_floats(nj), drain_floats(nj), "cuda",
                                                 hardness=hard_map(h.shape), upliftMap=uplift_map(h.shape))
    assert converged and steps == 1
    assert_bits(got, reference("bowl", DT, mapped=True), "both maps")


# 5. all or nothing: over 3 stripes the drainage area of `pitted` needs 8 rounds and the solve 9 (the CPU restatement, whose
# rounds run to rest like these); a budget of 8 leaves the heights in `out` on every stripe
def test_an_exhausted_round_budget_is_all_or_nothing(hip, nj):
    sh, ops = hip
    h = filled("pitted")
    got, A, steps, rounds, converged, plans, bufs = lockstep(sh, ops, 3, h, dict(PARAMS, dt=DT, maxRounds=8), work_floats(nj),
                                                             drain_floats(nj), "cuda")
    assert (steps, rounds, converged) == (0, 8, False)
    assert_bits(got, h, "the heights")
    assert_bits(A, area("pitted"), "the drainage area")
    for pl, b in zip(plans, bufs):
        out = b["out"].cpu().numpy()
        assert_bits(out[pl.own0:pl.own1], h[pl.g0:pl.g0 + pl.nown], "rank %d" % pl.rank)
        lo, hi = max(pl.own0 - 1, -pl.grow0), min(pl.own1 + 1, pl.grows - pl.grow0)
        assert np.isnan(out[:lo]).all() and np.isnan(out[hi:]).all(), "rank %d: rows beyond the ghost row" % pl.rank


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
    bufs = stripe_bufs(plan, h, work_floats(nj)(plan), drain_floats(nj)(plan), "cuda")
    hn, A, steps, rounds, converged = sh.run_fluvial_implicit(sh.HipStripeOps(ctx), comm, plan, dict(PARAMS, dt=DT), bufs)
    np.savez(out_path, steps=steps, rounds=rounds, converged=converged, h=hn[plan.own0:plan.own1].cpu().numpy())
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
    assert bool(got["converged"]) and int(got["steps"]) == 1 and int(got["rounds"]) == 2  # a round of work, a round at rest
    assert_bits(got["h"], reference("bowl"), "run_fluvial_implicit through NativeComm")


# 7. the chain on stripes is the chain on the tile: fill -> (drainage -> solve) x 2 over three ranks against
# nz_fill_depressions -> ImplicitFluvialStage on the 70 x 70 corner of `pitted`
def test_the_chain_on_stripes_is_the_chain_on_the_tile(hip, nj, ctx):
    sh, ops = hip
    N = nj._native
    res, world, its = 70, 3, 2
    h = np.ascontiguousarray(grid("pitted")[:res, :res])
    stage = nj.ImplicitFluvialStage(ctx, iterations=its, dt=DT, maxPasses=AMPLE)
    pipe = nj.BasePipeline([nj.DepressionFillStage(ctx, epsilon=EPS, maxPasses=AMPLE), stage], "chain")
    d = nj.GeneratorData("h", ctx.from_host(h), res, 0, 0)
    pipe.Enqueue(d)
    pipe.RunToCompletion()
    assert stage.steps == its and stage.converged is True
    want, want_a = d.data.ToArray((res, res)), stage.drainage.ToArray((res, res))
    pipe.Destroy()
    plans = [sh.StripePlan(r, world, res, res, HALO) for r in range(world)]
    full = lambda *shape: torch.full(shape, float("nan"), device="cuda")  # noqa: E731
    words = lambda: torch.full((3,), -7, dtype=torch.int32, device="cuda")  # noqa: E731
    sized = lambda entry, pl: full(getattr(N.lib, entry)(C.byref(pl.stripe())))  # noqa: E731
    bufs = [stripe_bufs(pl, h, work_floats(nj)(pl), drain_floats(nj)(pl), "cuda") for pl in plans]
    fill = sh.run_fill_lockstep([ops] * world, plans, dict(epsilon=EPS, maxPasses=AMPLE, maxRounds=AMPLE),
                                [dict(H=b["H"], W=full(pl.rows, pl.cols), work=sized("nz_fill_stripe_work_floats", pl),
                                      words=words()) for b, pl in zip(bufs, plans)], copy_rows)
    assert all(r[3] for r in fill)
    res_ = sh.run_fluvial_implicit_lockstep([ops] * world, plans, dict(PARAMS, dt=DT, iterations=its), bufs, copy_rows)
    assert all(r[2:] == (its, res_[0][3], True) for r in res_)
    rows = lambda t, pl: t[pl.own0:pl.own1, :pl.cols].cpu().numpy()  # noqa: E731
    assert_bits(np.concatenate([rows(r[0], pl) for r, pl in zip(res_, plans)]), want, "heights")
    assert_bits(np.concatenate([rows(r[1], pl) for r, pl in zip(res_, plans)]), want_a, "the drainage the last step saw")
    assert not R.same(want, h)


# 8. refusals: NZ_ERR_INVALID, and nothing is written -- one per clause of the contract
def test_refusals_write_nothing(hip, nj):
    sh, ops = hip
    N = nj._native
    h = filled("bowl")
    plan = sh.StripePlan(1, 3, h.shape[0], h.shape[1], 1)
    bufs = stripe_bufs(plan, h, work_floats(nj)(plan), 0, "cuda", None, area("bowl"), hardness=hard_map(h.shape),
                       upliftMap=uplift_map(h.shape))
    bufs["H"][:] = torch.from_numpy(np.ascontiguousarray(h[plan.grow0:plan.grow0 + plan.rows])).cuda()
    st = plan.stripe()
    Hp, Ap, Op, Kp, Dp, Up = (bufs[k].data_ptr() for k in ("H", "A", "out", "work", "hardness", "upliftMap"))
    w0, w1, w2 = (bufs["words"][i:i + 1].data_ptr() for i in range(3))
    row = 4 * plan.cols
    before = {k: bufs[k].clone() for k in bufs}

    def desc(erodibility=0.05, uplift=0.002, dt=1.0, sea=OFF, passes=10, hard=None, upl=None, proceed=None, tally=None):
        return N.FluvialImplicitDesc(erodibility, uplift, dt, sea, passes, hard, upl, proceed, tally)

    def refused(entry, name, *args):
        with pytest.raises(nj.NoizeError) as e:
            ops.ctx.call(entry, *args)
        assert e.value.status == N.NZ_ERR_INVALID and name in str(e.value), (name, str(e.value))

    def rnd(name, hp, ap, op, kp, stripe, d, first=1, proceed=None, changed=w0):
        refused("nz_implicit_fluvial_stripe_round", name, hp, ap, op, kp, C.byref(stripe), d if d is None else C.byref(d), first,
                proceed, changed)

    # everything the tile entry refuses
    rnd("desc", Hp, Ap, Op, Kp, st, None)
    rnd("height", None, Ap, Op, Kp, st, desc())
    rnd("drainage", Hp, None, Op, Kp, st, desc())
    rnd("out is NULL", Hp, Ap, None, Kp, st, desc())
    rnd("work", Hp, Ap, Op, None, st, desc())
    rnd("erodibility", Hp, Ap, Op, Kp, st, desc(erodibility=float("nan")))
    rnd("erodibility", Hp, Ap, Op, Kp, st, desc(erodibility=-1.0))
    rnd("uplift", Hp, Ap, Op, Kp, st, desc(uplift=float("inf")))
    rnd("uplift", Hp, Ap, Op, Kp, st, desc(uplift=-1.0))
    rnd("dt", Hp, Ap, Op, Kp, st, desc(dt=float("nan")))
    rnd("dt", Hp, Ap, Op, Kp, st, desc(dt=-1.0))
    rnd("seaLevel", Hp, Ap, Op, Kp, st, desc(sea=float("inf")))
    rnd("maxPasses", Hp, Ap, Op, Kp, st, desc(passes=0))
    # the descriptor's words have no place in a round
    rnd("desc->proceed", Hp, Ap, Op, Kp, st, desc(proceed=w1))
    rnd("desc->tally", Hp, Ap, Op, Kp, st, desc(tally=w1))
    # a NULL word, a missing ghost row (with and without `first`), a NULL stripe
    rnd("changed", Hp, Ap, Op, Kp, st, desc(), changed=None)
    none = sh.StripePlan(1, 3, h.shape[0], h.shape[1], 0).stripe()
    rnd("ghost rows", Hp, Ap, Op, Kp, none, desc())
    rnd("ghost rows", Hp, Ap, Op, Kp, none, desc(), first=0)
    with pytest.raises(nj.NoizeError):
        ops.ctx.call("nz_implicit_fluvial_stripe_round", Hp, Ap, Op, Kp, None, C.byref(desc()), 1, None, w0)
    # overlaps
    rnd("out overlaps height", Hp, Ap, Hp + row, Kp, st, desc())
    rnd("out overlaps drainage", Hp, Ap, Ap + row, Kp, st, desc())
    rnd("out overlaps hardness", Hp, Ap, Op, Kp, st, desc(hard=Op + row))
    rnd("out overlaps upliftMap", Hp, Ap, Op, Kp, st, desc(upl=Op + row))
    rnd("out overlaps work", Hp, Ap, Op, Op + 64, st, desc())
    rnd("work overlaps height", Kp + 64, Ap, Op, Kp, st, desc())
    rnd("work overlaps drainage", Hp, Kp + 64, Op, Kp, st, desc())
    rnd("work overlaps hardness", Hp, Ap, Op, Kp, st, desc(hard=Kp + 64))
    rnd("work overlaps upliftMap", Hp, Ap, Op, Kp, st, desc(upl=Kp + 64))
    rnd("changed overlaps out", Hp, Ap, Op, Kp, st, desc(), changed=Op + row)
    rnd("changed overlaps work", Hp, Ap, Op, Kp, st, desc(), changed=Kp)
    rnd("changed overlaps height", Hp, Ap, Op, Kp, st, desc(), changed=Hp + row)
    rnd("changed overlaps drainage", Hp, Ap, Op, Kp, st, desc(), changed=Ap + row)
    rnd("changed overlaps hardness", Hp, Ap, Op, Kp, st, desc(hard=Dp), changed=Dp + row)
    rnd("proceed overlaps out", Hp, Ap, Op, Kp, st, desc(), proceed=Op + 8)
    rnd("proceed overlaps work", Hp, Ap, Op, Kp, st, desc(), proceed=Kp + 8)
    rnd("changed overlaps proceed", Hp, Ap, Op, Kp, st, desc(), proceed=w0)

    def fin(name, hp, op, word, stripe=st):
        refused("nz_implicit_fluvial_stripe_finalise", name, hp, op, C.byref(stripe), word)

    fin("converged", Hp, Op, None)
    fin("height", None, Op, w2)
    fin("out is NULL", Hp, None, w2)
    fin("out overlaps height", Hp, Hp + row, w2)
    fin("converged overlaps out", Hp, Op, Op + row)
    torch.cuda.current_stream().synchronize()
    for k in bufs:
        a, b = bufs[k].cpu().numpy(), before[k].cpu().numpy()
        assert np.array_equal(a.view(np.uint32) if a.dtype == f32 else a, b.view(np.uint32) if b.dtype == f32 else b), k
    assert np.isnan(bufs["out"].cpu().numpy()).all() and np.isnan(bufs["work"].cpu().numpy()).all()
    assert bufs["words"].tolist() == [-7, -7, -7]
    # behind a proceed word of 0 a round is accepted and writes `changed` alone
    bufs["words"][1:2].fill_(0)
    ops.ctx.call("nz_implicit_fluvial_stripe_round", Hp, Ap, Op, Kp, C.byref(st), C.byref(desc(hard=Dp, upl=Up)), 1, w1, w0).Complete()
    assert bufs["words"].tolist() == [0, 0, -7] and np.isnan(bufs["out"].cpu().numpy()).all()
    assert N.lib.nz_implicit_fluvial_stripe_halo_rows() == 1
    cells = plan.rows * plan.cols
    assert N.lib.nz_implicit_fluvial_stripe_work_floats(C.byref(st)) > 3 * cells + cells // 4  # three planes and the bytes


# 9. planes carved from one guarded allocation at four alignments and three mixed pairs: the guards stay silent, the floats
# are the walk's.  70 x 100 takes the 16-byte path where every plane is aligned, 70 x 97 never does
@pytest.mark.parametrize("cols", [100, 97])
def test_on_slab_carved_planes(nj, ctx, cols):
    import fill_ref as L
    rows = 70
    h = L.flood(pitted(rows, cols), EPS)
    A = D.accumulate(h)[0]
    hard, upl = hard_map((rows, cols)), uplift_map((rows, cols))
    want = R.walk(h, A, dt=DT, hardness=hard, upliftMap=upl)
    n = rows * cols
    st = nj._native.Stripe(cols, rows, 0, rows, 0, rows, 0)
    nwork = nj._native.lib.nz_implicit_fluvial_stripe_work_floats(C.byref(st))
    start = np.array([-7, -7, 1], np.int32)
    for passes in (AMPLE, AMPLE + 1):
        for p, q in PAIRS:
            r = p if p == q else (q + 1) % 4
            with carved(ctx, cols, height=(n, p, h), area=(n, q, A), out=(n, q, None), work=(nwork, r, None), hard=(n, p, hard),
                        upl=(n, q, upl), words=(3, p, start, np.int32)) as (s, t):
                desc = nj._native.FluvialImplicitDesc(0.05, 0.002, DT, OFF, passes, t.hard.ptr, t.upl.ptr, None, None)
                args = (t.height.ptr, t.area.ptr, t.out.ptr, t.work.ptr, C.byref(st), C.byref(desc))
                ctx.call("nz_implicit_fluvial_stripe_round", *args, 1, None, t.words.ptr)
                ctx.call("nz_implicit_fluvial_stripe_round", *args, 0, t.words.ptr, t.words.ptr + 4)
                ctx.call("nz_implicit_fluvial_stripe_finalise", t.height.ptr, t.out.ptr, C.byref(st), t.words.ptr + 8).Complete()
                assert t.words.ToArray().tolist() == [1, 0, 1], (p, q)
                assert_bits(t.out.ToArray((rows, cols)), want, (cols, passes, p, q))
                assert_bits(t.height.ToArray((rows, cols)), h, "height")
                assert_bits(t.area.ToArray((rows, cols)), A, "drainage")
                s.check()


# 10. the C++ mirror: host_demo's fluvial-implicit-stripe mode -- a filled simplex tile as one stripe, its drainage through
# DrainageAreaStage, then ImplicitFluvialStripe's round with `first`, a quiet round and the finalise -- prints 0 for the quiet
# round and equals the Python path on the heights it wrote, and the walk
def test_the_cpp_mirror_runs_the_rounds_and_the_finalise(hip, nj, tmp_path):
    exe = os.path.join(ROOT, "noize_job_amd", "host", "host_demo")
    assert os.path.exists(exe), "host_demo not built (run __graft_entry__.build())"
    res, out = 160, str(tmp_path / "planes.f32")
    changed = subprocess.run([exe, str(res), out, "fluvial-implicit-stripe"], check=True, capture_output=True, text=True).stdout.split()
    assert changed == ["0"]
    h, got = np.fromfile(out, dtype=np.float32).reshape(2, res, res)
    A = D.accumulate(h)[0]
    mine, words, _ = one_stripe(hip, nj, h, A, dict(maxPasses=64 + res // 4, dt=100.0))
    assert words == [1, 0]
    assert_bits(got, mine, "the C++ mirror against the Python path")
    assert_bits(got, R.walk(h, A, dt=100.0), "the walk")
    assert not R.same(got, h)
