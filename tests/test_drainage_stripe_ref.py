"""The drainage area on row stripes, the schedule on the CPU: drainage_steps / run_drainage / run_drainage_lockstep of
noize_job_amd.sharded driven with the numpy reference as compute back end (tests/drainage_stripe_ops.py) end at
drainage_ref.accumulate's floats on the whole grid bit for bit -- in one process and over `gloo`, with a signed rain map
and with a sea; a pass budget too short for a round only adds rounds; an exhausted round budget is all or nothing on every
rank.  The budgets (drainage_stripe_cases.PARAMS) rest on "a pass is at least one Jacobi step"."""
import os

import numpy as np
import pytest

import drainage_ref as D
from conftest import ROOT
from drainage_stripe_cases import HALO, PARAMS, WORLDS, assert_bits, filled, lockstep, reference, signed_rain, stripe_bufs

f32 = np.float32


def run(h, world, rain_map=None, ops=None, **kw):
    from drainage_stripe_ops import DrainageStripeOps
    from noize_job_amd import sharded as sh
    return lockstep(sh, ops or DrainageStripeOps(), world, h, dict(PARAMS, **kw), rain_map=rain_map)


# 1. the stripes end at the topological walk of the whole grid; (33, 130) over 16 ranks are stripes of 2 and 3 rows
@pytest.mark.parametrize("name,world", [(n, w) for n in ("pitted", "bowl", "serpentine", "wide") for w in WORLDS])
def test_lockstep_equals_the_walk(name, world):
    got, rounds, converged, _, _ = run(filled(name), world)
    print("%s world %d: %d rounds" % (name, world, rounds))
    assert converged and 2 <= rounds <= 128
    assert_bits(got, reference(name)[0], "%s world %d" % (name, world))


# ... and so does the long chain of drainage_ref.serpentine, unfilled: 1037 cells, a few crossings of every cut
@pytest.mark.parametrize("world", WORLDS)
def test_the_long_chain(world):
    h = D.serpentine(48)
    want, height = D.accumulate(h)
    got, rounds, converged, _, _ = run(h, world, maxPasses=height + 2)
    print("serpentine(48) world %d: %d rounds" % (world, rounds))
    assert converged and rounds <= 128
    assert_bits(got, want, "world %d" % world)


# 2. a rain map with both signs: values move both ways, the fixed point is the same
def test_a_signed_rain_map():
    h = filled("pitted")
    got, _, converged, _, _ = run(h, 8, rain_map=signed_rain(h.shape), rain=0.75)
    assert converged
    want = reference("pitted", 0.75, mapped=True)[0]
    assert (want < 0).any() and (want > 0).any()
    assert_bits(got, want, "signed rain map")


# 3. a sea level above the lowest heights: the outlets follow the global grid
def test_a_sea_level():
    h = filled("pitted")
    sea = float(np.quantile(h, 0.3))
    got, _, converged, _, _ = run(h, 8, seaLevel=sea)
    assert converged
    assert_bits(got, D.accumulate(h, 1.0, sea)[0], "sea level")


# 4. a pass budget too short for a round: every round short of rest says so, the next one carries on.  A round short of
# rest makes maxPasses > 0 Jacobi steps, a cell's value is final after as many steps as its path has cells, so "longest
# path + 2" rounds suffice
def test_a_short_pass_budget_only_adds_rounds():
    from drainage_stripe_ops import DrainageStripeOps
    from noize_job_amd import sharded as sh
    h = D.serpentine(32)
    want, height = D.accumulate(h)
    ops = DrainageStripeOps()
    votes = []

    class Watch:  # the ops, with every rank's `changed` word written down
        def drainage(self, *args, **kw):
            ops.drainage(*args, **kw)
            votes.append(int(args[7][0]))

        drainage_finalise = ops.drainage_finalise

    got, rounds, converged, _, _ = lockstep(sh, Watch(), 2, h, dict(maxPasses=8, maxRounds=height + 2))
    assert converged and rounds > run(h, 2, maxPasses=height + 2)[1]
    assert len(ops.steps) == len(votes) == 2 * rounds
    assert votes[:2] == [1, 1]  # `first`
    for steps, vote in list(zip(ops.steps, votes))[2:]:
        assert vote == (1 if steps > 0 else 0), (steps, vote)
    assert max(ops.steps) == 8 and ops.steps.count(8) > 2  # rounds that ran out of passes, and went on
    assert_bits(got, want, "8 passes a round")


# 5. all or nothing: a round budget far too short leaves rain_c in every owned cell on EVERY rank and nothing else written
def test_an_exhausted_round_budget_is_all_or_nothing():
    h = filled("serpentine")
    rm = signed_rain(h.shape)
    got, rounds, converged, plans, bufs = run(h, 8, rain_map=rm, rain=2.0, maxRounds=10)
    assert (rounds, converged) == (10, False)
    assert_bits(got, (f32(2.0) * rm).astype(f32), "rain_c")
    for pl, b in zip(plans, bufs):
        A = b["A"].numpy()
        assert_bits(A[pl.own0:pl.own1], (f32(2.0) * rm[pl.g0:pl.g0 + pl.nown]).astype(f32), "rank %d" % pl.rank)
        lo, hi = max(pl.own0 - 1, -pl.grow0), min(pl.own1 + 1, pl.grows - pl.grow0)
        assert np.isnan(A[:lo]).all() and np.isnan(A[hi:]).all(), "rank %d: rows beyond the ghost row" % pl.rank
        assert_bits(b["H"][pl.own0:pl.own1].numpy(), h[pl.g0:pl.g0 + pl.nown], "rank %d: heights" % pl.rank)


# 6. the same over gloo: run_drainage with TorchComm, one process per rank
def _worker(rank, world, port, name, out_path):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    from drainage_stripe_ops import DrainageStripeOps
    from noize_job_amd import sharded as sh
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    h = filled(name)
    plan = sh.StripePlan(rank, world, h.shape[0], h.shape[1], HALO)
    bufs = stripe_bufs(plan, h, 0, rain_map=signed_rain(h.shape))
    A, rounds, converged = sh.run_drainage(DrainageStripeOps(), sh.TorchComm(dist), plan, PARAMS, bufs)
    parts = [None] * world
    dist.all_gather_object(parts, (plan.g0, A[plan.own0:plan.own1].numpy(), rounds, converged))
    if rank == 0:
        parts.sort(key=lambda t: t[0])
        assert len({(p[2], p[3]) for p in parts}) == 1
        np.savez(out_path, A=np.concatenate([p[1] for p in parts]), rounds=parts[0][2], converged=parts[0][3])
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_ranks_equal_the_walk(tmp_path):
    from test_sharded_cpu import _spawn
    out = str(tmp_path / "drainage.npz")
    _spawn(_worker, 3, lambda port: (3, port, "bowl", out))
    got = np.load(out)
    assert bool(got["converged"]) and int(got["rounds"]) >= 2
    assert_bits(got["A"], reference("bowl", mapped=True)[0], "gloo world 3")


# 7. the protocol: 2 rows of the heights (and of the rain map) before round 0, 1 row of A before every later round, a vote
# after every round; round 0 says `first` and has no proceed word, every later round is handed the word the vote before it
# reduced; the A plane comes back as it serves fluvial_steps
def test_steps_ask_for_the_documented_exchanges_and_votes():
    import torch
    from noize_job_amd import sharded as sh
    calls = []

    class Rec:
        def drainage(self, h, a, work, plan, prm, first, proceed, changed, rainMap=None):
            calls.append(("round", first, None if proceed is None else proceed.data_ptr(), changed.data_ptr(), rainMap))

        def drainage_finalise(self, a, plan, prm, converged, rainMap=None):
            calls.append(("finalise", int(converged[0]), rainMap))

    words = torch.zeros(3, dtype=torch.int32)
    bufs = dict(H="H", A="A", work="work", words=words, rainMap="R")
    gen = sh.drainage_steps(Rec(), sh.StripePlan(1, 3, 90, 8, 2), dict(maxRounds=5), bufs)
    reqs, votes, answer = [], iter([1, 1, 0]), None
    try:
        while True:
            req = gen.send(answer)
            reqs.append(req[0] if req[0] == sh.VOTE else (req[0], req[1], req[2]))
            answer = next(votes) if req[0] == sh.VOTE else None
    except StopIteration as done:
        result = done.value
    assert reqs == [(["H", "R"], 2, 2), sh.VOTE, (["A"], 1, 1), sh.VOTE, (["A"], 1, 1), sh.VOTE]
    p = [words[i:i + 1].data_ptr() for i in range(2)]
    assert calls == [("round", True, None, p[0], "R"), ("round", False, p[0], p[1], "R"), ("round", False, p[1], p[0], "R"),
                     ("finalise", 1, "R")]
    assert result == ("A", 3, True)
    with pytest.raises(AssertionError):
        next(sh.drainage_steps(Rec(), sh.StripePlan(1, 3, 90, 8, 1), None, bufs))
    assert sh.DRAINAGE_DEFAULTS == dict(rain=1.0, seaLevel=float(D.SEA_OFF), maxPasses=64, maxRounds=64)
