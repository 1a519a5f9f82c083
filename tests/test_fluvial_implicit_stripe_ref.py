"""Implicit fluvial erosion on row stripes, the schedule on the CPU: fluvial_implicit_steps / run_fluvial_implicit /
run_fluvial_implicit_lockstep of noize_job_amd.sharded driven with the numpy reference as compute back end
(tests/fluvial_implicit_stripe_ops.py) end at fluvial_implicit_ref.walk's floats on the whole grid bit for bit -- in one
process and over `gloo`, with a sea and with both maps; the chain of several iterations equals fluvial_implicit_ref.chain;
an exhausted round budget is all or nothing on every rank; a drainage that does not converge applies no step.  The budgets
(fluvial_implicit_stripe_cases.PARAMS) rest on "a pass is at least one Jacobi step" and are held here to the numbers they
were derived from."""
import os

import numpy as np
import pytest

import fluvial_implicit_ref as R
from conftest import ROOT
from fluvial_implicit_stripe_cases import (CASES, DT, HALO, MOST_ROUNDS, MOST_STEPS, PARAMS, area, assert_bits, cpu_rounds,
                                           filled, hard_map, lockstep, reference, stripe_bufs, uplift_map)

f32 = np.float32


def run(h, world, ops=None, **kw):
    from fluvial_implicit_stripe_ops import FluvialImplicitStripeOps
    from noize_job_amd import sharded as sh
    maps = {k: kw.pop(k) for k in ("hardness", "upliftMap", "rainMap") if k in kw}
    return lockstep(sh, ops or FluvialImplicitStripeOps(), world, h, dict(PARAMS, **kw), **maps)


# 1. the stripes end at the walk of the whole grid (cpu_rounds compares the bits), within the rounds and the steps per round
# the budgets were derived from; (33, 130) over 16 ranks are stripes of 2 and 3 rows
@pytest.mark.parametrize("name,world,dt", CASES)
def test_lockstep_equals_the_walk(name, world, dt):
    rounds, steps = cpu_rounds(name, world, dt)
    print("%s world %d dt %g: %d rounds, at most %d steps in one" % (name, world, dt, rounds, steps))
    assert 2 <= rounds <= MOST_ROUNDS and steps <= MOST_STEPS
    assert MOST_ROUNDS < PARAMS["maxRounds"] and MOST_STEPS < PARAMS["maxPasses"]


def test_the_worst_cases_are_the_ones_named():
    assert cpu_rounds("serpentine", 16, DT)[0] == MOST_ROUNDS
    assert cpu_rounds("bowl", 2, DT)[1] == MOST_STEPS


# 2. all or nothing: a round budget far too short leaves the heights in every owned cell of `out` on EVERY rank, nothing
# else written, converged False and no step counted
def test_an_exhausted_round_budget_is_all_or_nothing():
    h = filled("pitted")  # over 3 stripes the drainage area needs 8 rounds (maxRounds is its budget too), the solve 9
    assert cpu_rounds("pitted", 3, DT)[0] == 9
    got, A, steps, rounds, converged, plans, bufs = run(h, 3, dt=DT, maxRounds=8)
    assert (steps, rounds, converged) == (0, 8, False)
    assert_bits(got, h, "the heights")
    assert_bits(A, area("pitted"), "the drainage area")
    for pl, b in zip(plans, bufs):
        own = slice(pl.g0, pl.g0 + pl.nown)
        for k in ("H", "out"):
            assert_bits(b[k][pl.own0:pl.own1].numpy(), h[own], "rank %d: %s" % (pl.rank, k))
        out = b["out"].numpy()
        lo, hi = max(pl.own0 - 1, -pl.grow0), min(pl.own1 + 1, pl.grows - pl.grow0)
        assert np.isnan(out[:lo]).all() and np.isnan(out[hi:]).all(), "rank %d: rows beyond the ghost row" % pl.rank


# 3. a drainage that does not converge applies no step: the solve is not called at all
def test_a_drainage_short_of_rest_applies_no_step():
    from fluvial_implicit_stripe_ops import FluvialImplicitStripeOps
    h = filled("serpentine")
    ops = FluvialImplicitStripeOps()
    got, _, steps, rounds, converged, plans, bufs = run(h, 8, ops=ops, dt=DT, maxRounds=3, iterations=2)
    assert (steps, rounds, converged) == (0, 0, False) and ops.solve_steps == []
    assert_bits(got, h, "the heights")
    for b in bufs:
        assert np.isnan(b["out"].numpy()).all()


# 4. iterations: drainage area and solve per iteration, the planes swapping, against the hosts' chain
def test_three_iterations_equal_the_chain():
    h = filled("pitted")
    got, A, steps, _, converged, _, _ = run(h, 3, dt=50.0, iterations=3, rain=0.5)
    want_h, want_a = R.chain(h, 3, dt=50.0, rain=0.5)
    assert converged and steps == 3
    assert_bits(got, want_h, "heights after 3 iterations")
    assert_bits(A, want_a, "the drainage area the last iteration saw")


# 5. a sea level above the lowest heights: the outlets follow the global grid
def test_a_sea_level():
    h = filled("pitted")
    sea = float(np.quantile(h, 0.3))
    got, _, steps, _, converged, _, _ = run(h, 8, dt=DT, seaLevel=sea)
    assert converged and steps == 1
    want = reference("pitted", DT, sea)
    assert_bits(want[h <= sea], h[h <= sea], "cells below the sea keep their bits")
    assert_bits(got, want, "sea level")


# 6. a hardness map and an uplift map
def test_hardness_and_uplift_maps():
    h = filled("bowl")
    got, _, steps, _, converged, _, _ = run(h, 8, dt=DT, hardness=hard_map(h.shape), upliftMap=uplift_map(h.shape))
    assert converged and steps == 1
    want = reference("bowl", DT, mapped=True)
    assert not R.same(want, reference("bowl", DT))
    assert_bits(got, want, "both maps")


# 7. the same over gloo: run_fluvial_implicit with TorchComm, one process per rank
def _worker(rank, world, port, name, out_path):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    from fluvial_implicit_stripe_ops import FluvialImplicitStripeOps
    from noize_job_amd import sharded as sh
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    h = filled(name)
    plan = sh.StripePlan(rank, world, h.shape[0], h.shape[1], HALO)
    bufs = stripe_bufs(plan, h, 0, hardness=hard_map(h.shape), upliftMap=uplift_map(h.shape))
    hn, _, steps, rounds, converged = sh.run_fluvial_implicit(FluvialImplicitStripeOps(), sh.TorchComm(dist), plan,
                                                              dict(PARAMS, dt=DT), bufs)
    parts = [None] * world
    dist.all_gather_object(parts, (plan.g0, hn[plan.own0:plan.own1].numpy(), steps, rounds, converged))
    if rank == 0:
        parts.sort(key=lambda t: t[0])
        assert len({p[2:] for p in parts}) == 1
        np.savez(out_path, h=np.concatenate([p[1] for p in parts]), steps=parts[0][2], rounds=parts[0][3],
                 converged=parts[0][4])
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_ranks_equal_the_walk(tmp_path):
    from test_sharded_cpu import _spawn
    out = str(tmp_path / "fluvial_implicit.npz")
    _spawn(_worker, 3, lambda port: (3, port, "bowl", out))
    got = np.load(out)
    assert bool(got["converged"]) and int(got["steps"]) == 1 and int(got["rounds"]) >= 2
    assert_bits(got["h"], reference("bowl", DT, mapped=True), "gloo world 3")


# 8. the protocol: the drainage's requests first; then 1 row of the heights before round 0 of the solve, 1 row of `out` before
# every later round, a vote after every round; round 0 says `first` and has no proceed word, every later round is handed the
# word the vote before it reduced; finalise with the verdict; the planes swap
def test_steps_ask_for_the_documented_exchanges_and_votes():
    import torch
    from noize_job_amd import sharded as sh
    calls = []

    class Rec:
        def drainage(self, h, a, work, plan, prm, first, proceed, changed, rainMap=None):
            calls.append(("drainage", h, a, work, first, prm["rain"], prm["maxPasses"], rainMap))

        def drainage_finalise(self, a, plan, prm, converged, rainMap=None):
            calls.append(("drainage_finalise", int(converged[0])))

        def fluvial_implicit(self, h, a, out, work, plan, prm, first, proceed, changed, **maps):
            calls.append(("round", h, a, out, work, first, None if proceed is None else proceed.data_ptr(),
                          changed.data_ptr(), prm["dt"], maps))

        def fluvial_implicit_finalise(self, h, out, plan, converged):
            calls.append(("finalise", h, out, int(converged[0])))

    words = torch.zeros(3, dtype=torch.int32)
    bufs = dict(H="H", out="O", A="A", work="work", drainageWork="dwork", words=words, rainMap="R", hardness="K")
    gen = sh.fluvial_implicit_steps(Rec(), sh.StripePlan(1, 3, 90, 8, 2), dict(maxRounds=5, dt=7.0, rain=2.0, maxPasses=9), bufs)
    reqs, votes, answer = [], iter([1, 0, 1, 1, 0]), None  # the drainage: 2 rounds; the solve: 3
    try:
        while True:
            req = gen.send(answer)
            reqs.append(req[0] if req[0] == sh.VOTE else (req[0], req[1], req[2]))
            answer = next(votes) if req[0] == sh.VOTE else None
    except StopIteration as done:
        result = done.value
    assert reqs == [(["H", "R"], 2, 2), sh.VOTE, (["A"], 1, 1), sh.VOTE,
                    (["H"], 1, 1), sh.VOTE, (["O"], 1, 1), sh.VOTE, (["O"], 1, 1), sh.VOTE]
    p = [words[i:i + 1].data_ptr() for i in range(2)]
    maps = dict(hardness="K")
    assert calls == [("drainage", "H", "A", "dwork", True, 2.0, 9, "R"), ("drainage", "H", "A", "dwork", False, 2.0, 9, "R"),
                     ("drainage_finalise", 1),
                     ("round", "H", "A", "O", "work", True, None, p[0], 7.0, maps),
                     ("round", "H", "A", "O", "work", False, p[0], p[1], 7.0, maps),
                     ("round", "H", "A", "O", "work", False, p[1], p[0], 7.0, maps), ("finalise", "H", "O", 1)]
    assert result == ("O", "A", 1, 3, True)
    with pytest.raises(AssertionError):
        next(sh.fluvial_implicit_steps(Rec(), sh.StripePlan(1, 3, 90, 8, 1), None, bufs))
    assert sh.FLUVIAL_IMPLICIT_DEFAULTS == dict(R.DEFAULTS, maxPasses=64, maxRounds=64)
