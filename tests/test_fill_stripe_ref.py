"""Depression filling on row stripes, the schedule on the CPU: fill_steps / run_fill / run_fill_lockstep of
noize_job_amd.sharded driven with the numpy reference as compute back end (tests/fill_stripe_ops.py) end at
fill_ref.flood's floats on the whole grid bit for bit, depth included -- in one process and over `gloo`; a bowl over three
stripes and a serpentine lake need more than one round; a round budget one short is all or nothing on every rank."""
import os

import numpy as np
import pytest

import fill_ref as L
from conftest import ROOT
from fill_stripe_cases import EPS, WORLDS, assert_bits, flood, grid, lockstep, stripe_bufs

f32 = np.float32
PARAMS = dict(epsilon=EPS, maxPasses=100000, maxRounds=1000)


def run(name, world, **kw):
    from fill_stripe_ops import FillStripeOps
    from noize_job_amd import sharded as sh
    return lockstep(sh, FillStripeOps(), world, grid(name), dict(PARAMS, **kw))


# 1. the stripes end at the priority flood of the whole grid; (33, 130) over 16 ranks are stripes of 2 and 3 rows
@pytest.mark.parametrize("name,world", [(n, w) for n in ("pitted", "bowl", "serpentine") for w in WORLDS] + [("wide", 16)])
def test_lockstep_equals_the_flood(name, world):
    h, want = grid(name), flood(name)
    got, depth, rounds, converged, _, _ = run(name, world)
    print("%s world %d: %d rounds" % (name, world, rounds))
    assert converged and rounds >= 2
    assert_bits(got, want, "%s world %d" % (name, world))
    assert_bits(depth, (want - h).astype(f32), "%s world %d: depth" % (name, world))


# 2. the serpentine's spill path crosses the one cut of world 2 once per leg: more rounds than the bowl's plain crossing
def test_the_serpentine_needs_a_round_per_crossing():
    assert run("serpentine", 2)[2] > run("bowl", 2)[2] >= 2
    assert run("serpentine", 2)[2] >= 8


# 3. a short pass budget per round only adds rounds
def test_a_small_pass_budget_ends_at_the_same_floats():
    got, _, rounds, converged, _, _ = run("bowl", 3, maxPasses=7)
    assert converged and rounds > run("bowl", 3)[2]
    assert_bits(got, flood("bowl"), "bowl, 7 passes a round")


# 4. a sea level: the outlets follow the global grid
def test_a_sea_level():
    sea = 0.45
    from fill_stripe_ops import FillStripeOps
    from noize_job_amd import sharded as sh
    got, _, _, converged, _, _ = lockstep(sh, FillStripeOps(), 8, grid("pitted"), dict(PARAMS, seaLevel=sea))
    assert converged
    assert_bits(got, L.flood(grid("pitted"), EPS, sea), "sea level")


# 5. all or nothing: one round short leaves the heights untouched on EVERY rank, and the depth zero
@pytest.mark.parametrize("name,world", [("bowl", 3), ("serpentine", 8)])
def test_a_round_budget_one_short_is_all_or_nothing(name, world):
    h = grid(name)
    need = run(name, world)[2]
    got, depth, rounds, converged, plans, bufs = run(name, world, maxRounds=need - 1)
    assert (rounds, converged) == (need - 1, False)
    assert_bits(got, h, "heights stay")
    assert not depth.any()
    for pl, b in zip(plans, bufs):  # rank by rank
        assert_bits(b["H"][pl.own0:pl.own1].numpy(), h[pl.g0:pl.g0 + pl.nown], "rank %d" % pl.rank)


# 6. the same over gloo: run_fill with TorchComm, one process per rank
def _worker(rank, world, port, name, out_path):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    from fill_stripe_ops import FillStripeOps
    from noize_job_amd import sharded as sh
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    h = grid(name)
    plan = sh.StripePlan(rank, world, h.shape[0], h.shape[1], 1)
    bufs = stripe_bufs(plan, h, 0)
    H, depth, rounds, converged = sh.run_fill(FillStripeOps(), sh.TorchComm(dist), plan, PARAMS, bufs)
    parts = [None] * world
    dist.all_gather_object(parts, (plan.g0, H[plan.own0:plan.own1].numpy(), depth[plan.own0:plan.own1].numpy(), rounds, converged))
    if rank == 0:
        parts.sort(key=lambda t: t[0])
        assert len({(p[3], p[4]) for p in parts}) == 1
        np.savez(out_path, heights=np.concatenate([p[1] for p in parts]), depth=np.concatenate([p[2] for p in parts]),
                 rounds=parts[0][3], converged=parts[0][4])
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_ranks_equal_the_flood(tmp_path):
    from test_sharded_cpu import _spawn
    out = str(tmp_path / "fill.npz")
    _spawn(_worker, 3, lambda port: (3, port, "bowl", out))
    got = np.load(out)
    assert bool(got["converged"]) and int(got["rounds"]) >= 2
    assert_bits(got["heights"], flood("bowl"), "gloo world 3")
    assert_bits(got["depth"], (flood("bowl") - grid("bowl")).astype(f32), "gloo world 3: depth")


# 7. the protocol: an exchange request is (planes, 1, 1), a vote request (VOTE, word); round 0 says `first` and has no
# proceed word, every later round is handed the word the vote before it reduced
def test_steps_ask_for_the_documented_exchanges_and_votes():
    import torch
    from noize_job_amd import sharded as sh
    calls = []

    class Rec:
        def fill(self, h, w, work, plan, prm, first, proceed, changed):
            calls.append(("fill", first, None if proceed is None else proceed.data_ptr(), changed.data_ptr()))

        def fill_finalise(self, h, w, depth, plan, converged):
            calls.append(("finalise", int(converged[0])))

    words = torch.zeros(3, dtype=torch.int32)
    bufs = dict(H="H", W="W", work="work", words=words)
    gen = sh.fill_steps(Rec(), sh.StripePlan(1, 3, 90, 8, 1), dict(maxRounds=5), bufs)
    reqs, votes, answer = [], iter([1, 1, 0]), None
    try:
        while True:
            req = gen.send(answer)
            reqs.append(req[0] if req[0] == sh.VOTE else (req[0], req[1], req[2]))
            answer = next(votes) if req[0] == sh.VOTE else None
    except StopIteration as done:
        result = done.value
    assert reqs == [(["H"], 1, 1), sh.VOTE, (["W"], 1, 1), sh.VOTE, (["W"], 1, 1), sh.VOTE]
    p = [words[i:i + 1].data_ptr() for i in range(2)]
    assert calls == [("fill", True, None, p[0]), ("fill", False, p[0], p[1]), ("fill", False, p[1], p[0]), ("finalise", 1)]
    assert result == ("H", None, 3, True)
    assert sh.NoComm().allreduce_max(torch.tensor([3], dtype=torch.int32)) == 3
