"""Depression filling on row stripes on the GPU (nz_fill_stripe, nz_fill_stripe_finalise, HipStripeOps.fill,
run_fill_lockstep, nz_comm_allreduce_max_i32) against tests/fill_ref.py, bit for bit: one stripe is the flood on a
rectangle; a square stripe followed by finalise is nz_fill_depressions, depth included; the ghost rows of W are frozen; rows
beyond them and the pitch pads are not touched; a proceed word of zero writes nothing; the sweep cap does not matter; bowl
and serpentine over 2 to 16 stripes end at the flood; an exhausted round budget is all or nothing on every stripe; the
vote runs through the library's collective with a rank as its own peer; refusals write nothing.  Every buffer starts as NaN."""
import ctypes as C
import multiprocessing as mp

import numpy as np
import pytest
import torch

import fill_ref as L
from conftest import ROOT
from fill_stripe_cases import EPS, WORLDS, assert_bits, bowl, flood, grid, lockstep, pitted, stripe_bufs, stripe_ops, work_floats
from test_gpu_fill import run_gpu

pytestmark = pytest.mark.gpu
f32 = np.float32
PARAMS = dict(epsilon=EPS, maxPasses=400, maxRounds=400)  # 400 passes: the generous budget of tests/test_gpu_fill.py


@pytest.fixture(scope="module")
def hip(nj):
    """fill_stripe_cases.stripe_ops, once for the module."""
    with stripe_ops(nj) as pair:
        yield pair


def one_stripe(hip, nj, h, params=PARAMS, pitch=None):
    """The whole grid as one stripe: one round with `first`, then finalise with a word of 1 -> (heights, depth, changed, bufs)"""
    sh, ops = hip
    plan = sh.StripePlan(0, 1, h.shape[0], h.shape[1], 0)
    bufs = stripe_bufs(plan, h, work_floats(nj, pitch or 0)(plan), "cuda", pitch)
    prm = dict(sh.FILL_DEFAULTS, **params)
    ops.fill(bufs["H"], bufs["W"], bufs["work"], plan, prm, True, None, bufs["words"][0:1], pitch=pitch or 0)
    changed = int(bufs["words"][0])
    bufs["words"][2:3].fill_(1)
    ops.fill_finalise(bufs["H"], bufs["W"], bufs["depth"], plan, bufs["words"][2:3], pitch=pitch or 0)
    cut = lambda t: t[:, :plan.cols].cpu().numpy()  # noqa: E731
    return cut(bufs["H"]), cut(bufs["depth"]), changed, bufs


# 1. one stripe is the flood on a rectangle: the 4-byte path (333 columns) and the 16-byte one, odd and even pass budgets
@pytest.mark.parametrize("shape", [(70, 333), (333, 200), (64, 64)])
def test_one_stripe_is_the_flood_on_a_rectangle(hip, nj, shape):
    h = pitted(*shape)
    want = L.flood(h, EPS)
    for passes in (400, 401):
        got, depth, changed, _ = one_stripe(hip, nj, h, dict(PARAMS, maxPasses=passes))
        assert changed == 1
        assert_bits(got, want, "%s, %d passes" % (shape, passes))
        assert_bits(depth, (want - h).astype(f32), "%s: depth" % (shape,))


# ... and on a square, followed by finalise, it is nz_fill_depressions, device against device
def test_a_square_stripe_is_the_tile_entry(hip, nj, ctx):
    h = bowl(160, 160)
    want, want_depth, _, converged = run_gpu(nj, ctx, h, eps=EPS, depth=True)
    assert converged == 1
    got, depth, _, _ = one_stripe(hip, nj, h)
    assert_bits(got, want, "heights")
    assert_bits(depth, want_depth, "depth")
    assert_bits(got, L.flood(h, EPS), "reference")


# 2. rank 1 of 3 with two rows more than the one ghost row, a pitch on every plane (cols + 5: 4-byte path, cols + 8:
# 16-byte path): rounds against ghost rows put there by hand.  The ghost rows of W keep their bits, the rows beyond them and
# the pads keep their NaN, in W and in the work plane; a second round at rest reports changed == 0; proceed == 0 writes nothing
@pytest.mark.parametrize("pad", [5, 8])
@pytest.mark.parametrize("passes", [6, 7])
def test_ghost_rows_are_frozen_and_the_rest_is_untouched(hip, nj, pad, passes):
    sh, ops = hip
    name = "bowl"
    h, want = grid(name), flood(name)
    rows, cols = h.shape
    pitch = cols + pad
    plan = sh.StripePlan(1, 3, rows, cols, 3)
    bufs = stripe_bufs(plan, h, work_floats(nj, pitch)(plan), "cuda", pitch)
    lo, hi = plan.own0 - 1, plan.own1 + 1
    bufs["H"][lo:hi, :cols] = torch.from_numpy(np.ascontiguousarray(h[plan.grow0 + lo:plan.grow0 + hi])).cuda()
    prm = dict(sh.FILL_DEFAULTS, epsilon=EPS, maxPasses=passes)
    words = bufs["words"]
    ops.fill(bufs["H"], bufs["W"], bufs["work"], plan, prm, True, None, words[0:1], pitch=pitch)
    assert int(words[0]) == 1
    # later rounds against the flood's own rows as ghost rows: the stripe goes down to the flood's floats
    ghost = torch.from_numpy(np.ascontiguousarray(want[[plan.grow0 + lo, plan.grow0 + hi - 1]])).cuda()
    bufs["W"][lo, :cols], bufs["W"][hi - 1, :cols] = ghost[0], ghost[1]
    for r in range(1, 200):
        ops.fill(bufs["H"], bufs["W"], bufs["work"], plan, prm, False, words[(r - 1) & 1:((r - 1) & 1) + 1],
                 words[r & 1:(r & 1) + 1], pitch=pitch)
        if int(words[r & 1]) == 0:
            break
    assert r < 199, r
    W = bufs["W"].cpu().numpy()
    assert_bits(W[plan.own0:plan.own1, :cols], want[plan.g0:plan.g0 + plan.nown], "the stripe's W")
    assert_bits(W[[lo, hi - 1], :cols], ghost.cpu().numpy(), "ghost rows of w")
    work = bufs["work"].cpu().numpy()
    plane = work[work.size - plan.rows * pitch:].reshape(plan.rows, pitch)
    for what, t in (("w", W), ("work plane", plane)):
        assert np.isnan(t[:, cols:]).all(), "%s: pad floats" % what
        assert np.isnan(t[:lo]).all() and np.isnan(t[hi:]).all(), "%s: rows beyond the ghost row" % what
    assert np.isnan(plane[lo]).all() and np.isnan(plane[hi - 1]).all(), "the work plane's ghost rows"
    # proceed == 0 (the word of the round at rest): nothing is written, changed == 0 -- even with `first`
    before = bufs["W"].clone()
    zero = words[r & 1:(r & 1) + 1]
    words[2:3].fill_(-7)
    ops.fill(bufs["H"], bufs["W"], bufs["work"], plan, prm, True, zero, words[2:3], pitch=pitch)
    assert int(words[2]) == 0
    assert_bits(bufs["W"].cpu().numpy(), before.cpu().numpy(), "w after proceed == 0")
    # the heights were never written
    assert_bits(bufs["H"].cpu().numpy()[lo:hi, :cols], h[plan.grow0 + lo:plan.grow0 + hi], "height")


# 3. the sweep cap does not change the floats, alone or over stripes
def test_sweep_caps_give_equal_bits(hip, nj):
    sh, ops = hip
    lib = nj._native.lib
    try:
        for sweeps in (1, 4, 200):
            lib.nz_debug_fill_sweeps(sweeps)
            got, _, _, _ = one_stripe(hip, nj, grid("bowl"), dict(PARAMS, maxPasses=2000))
            assert_bits(got, flood("bowl"), "one stripe, %d sweeps" % sweeps)
            got, _, rounds, converged, _, _ = lockstep(sh, ops, 8, grid("pitted"), PARAMS, work_floats(nj), "cuda")
            assert converged
            assert_bits(got, flood("pitted"), "8 stripes, %d sweeps" % sweeps)
    finally:
        lib.nz_debug_fill_sweeps(0)


# 4. the stripes end at the flood of the whole grid; the serpentine needs a round per crossing of a cut
@pytest.mark.parametrize("name,world", [(n, w) for n in ("pitted", "bowl", "serpentine") for w in WORLDS] + [("wide", 16)])
def test_stripes_equal_the_flood(hip, nj, name, world):
    sh, ops = hip
    h, want = grid(name), flood(name)
    got, depth, rounds, converged, _, _ = lockstep(sh, ops, world, h, PARAMS, work_floats(nj), "cuda")
    print("%s world %d: %d rounds" % (name, world, rounds))
    assert converged and rounds >= 2
    assert rounds >= 8 or name != "serpentine"
    assert_bits(got, want, "%s world %d" % (name, world))
    assert_bits(depth, (want - h).astype(f32), "%s world %d: depth" % (name, world))


def test_a_sea_level_over_stripes(hip, nj):
    sh, ops = hip
    got, _, _, converged, _, _ = lockstep(sh, ops, 8, grid("pitted"), dict(PARAMS, seaLevel=0.45), work_floats(nj), "cuda")
    assert converged
    assert_bits(got, L.flood(grid("pitted"), EPS, 0.45), "sea level")


# 5. all or nothing: one round short, or passes that run out in every round, leave every stripe's heights and a zero depth
@pytest.mark.parametrize("name,world", [("bowl", 3), ("serpentine", 8)])
def test_an_exhausted_round_budget_is_all_or_nothing(hip, nj, name, world):
    sh, ops = hip
    h = grid(name)
    need = lockstep(sh, ops, world, h, PARAMS, work_floats(nj), "cuda")[2]
    for prm in (dict(PARAMS, maxRounds=need - 1), dict(PARAMS, maxPasses=1, maxRounds=2)):
        got, depth, rounds, converged, plans, bufs = lockstep(sh, ops, world, h, prm, work_floats(nj), "cuda")
        assert (rounds, converged) == (prm["maxRounds"], False)
        assert_bits(got, h, "heights stay")
        assert not depth.any()
        for pl, b in zip(plans, bufs):
            assert_bits(b["H"][pl.own0:pl.own1].cpu().numpy(), h[pl.g0:pl.g0 + pl.nown], "rank %d" % pl.rank)


# 6. the vote through nz_comm_allreduce_max_i32, a rank as its own peer, in a child process like every RCCL test
def _rccl_worker(out_path):
    import sys
    sys.path.insert(0, ROOT)
    import noize_job_amd as nj
    from noize_job_amd import sharded as sh
    ctx = nj.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    comm = sh.NativeComm(ctx, sh.NativeComm.unique_id(), 0, 1)
    words = torch.tensor([5, -3, 0], dtype=torch.int32, device="cuda")
    first = comm.allreduce_max(words)
    h = grid("bowl")
    plan = sh.StripePlan(0, 1, h.shape[0], h.shape[1], 1)
    bufs = stripe_bufs(plan, h, nj._native.lib.nz_fill_stripe_work_floats(C.byref(plan.stripe())), "cuda")
    H, depth, rounds, converged = sh.run_fill(sh.HipStripeOps(ctx), comm, plan, PARAMS, bufs)
    np.savez(out_path, words=words.cpu().numpy(), first=first, rounds=rounds, converged=converged,
             heights=H[plan.own0:plan.own1].cpu().numpy(), depth=depth[plan.own0:plan.own1].cpu().numpy())
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
    assert got["words"].tolist() == [5, -3, 0] and int(got["first"]) == 5
    assert bool(got["converged"]) and int(got["rounds"]) == 2  # one stripe: a round of work, a round at rest
    assert_bits(got["heights"], flood("bowl"), "run_fill through NativeComm")
    assert_bits(got["depth"], (flood("bowl") - grid("bowl")).astype(f32), "depth")


# 7. refusals: NZ_ERR_INVALID, and nothing is written
def test_refusals_write_nothing(hip, nj):
    sh, ops = hip
    N = nj._native
    h = grid("bowl")
    plan = sh.StripePlan(1, 3, h.shape[0], h.shape[1], 1)
    bufs = stripe_bufs(plan, h, work_floats(nj)(plan), "cuda")
    bufs["H"][:] = torch.from_numpy(np.ascontiguousarray(h[plan.grow0:plan.grow0 + plan.rows])).cuda()
    st = plan.stripe()
    Hp, Wp, Kp, Dp = (bufs[k].data_ptr() for k in ("H", "W", "work", "depth"))
    w0, w2 = bufs["words"][0:1].data_ptr(), bufs["words"][2:3].data_ptr()

    def desc(eps=EPS, sea=float(L.SEA_OFF), passes=10):
        return N.FillDesc(eps, sea, passes, None)

    def refused(entry, name, *args):
        with pytest.raises(nj.NoizeError) as e:
            ops.ctx.call(entry, *args)
        assert e.value.status == N.NZ_ERR_INVALID and name in str(e.value), (name, str(e.value))

    def fill(name, hp, wp, kp, stripe, d, changed=w0):
        refused("nz_fill_stripe", name, hp, wp, kp, C.byref(stripe), d if d is None else C.byref(d), 1, None, changed)

    fill("epsilon", Hp, Wp, Kp, st, desc(eps=-1.0))
    fill("epsilon", Hp, Wp, Kp, st, desc(eps=float("nan")))
    fill("seaLevel", Hp, Wp, Kp, st, desc(sea=float("inf")))
    fill("maxPasses", Hp, Wp, Kp, st, desc(passes=0))
    fill("desc", Hp, Wp, Kp, st, None)
    fill("work", Hp, Wp, None, st, desc())
    fill("changed", Hp, Wp, Kp, st, desc(), changed=None)
    fill("w overlaps height", Hp, Hp + 4 * plan.cols, Kp, st, desc())
    fill("work overlaps w", Hp, Wp, Wp + 64, st, desc())
    short = sh.StripePlan(1, 3, h.shape[0], h.shape[1], 0).stripe()
    fill("ghost rows", Hp, Wp, Kp, short, desc())
    fin = lambda name, hp, wp, dp, word: refused("nz_fill_stripe_finalise", name, hp, wp, dp, C.byref(st), word)  # noqa: E731
    fin("converged", Hp, Wp, Dp, None)
    fin("height/w", Hp, None, Dp, w2)
    fin("depth overlaps w", Hp, Wp, Wp + 4 * plan.cols, w2)
    torch.cuda.current_stream().synchronize()
    for name in ("W", "work", "depth"):
        assert np.isnan(bufs[name].cpu().numpy()).all(), name
    assert bufs["words"].tolist() == [-7, -7, -7]
    assert_bits(bufs["H"].cpu().numpy(), h[plan.grow0:plan.grow0 + plan.rows], "height")
    assert N.lib.nz_fill_stripe_halo_rows() == 1
    assert N.lib.nz_fill_stripe_work_floats(C.byref(st)) > plan.rows * plan.cols
