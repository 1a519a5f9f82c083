"""The stripe sweep on the CPU: every case of tests/sweep_stripe_cases.py -- the tie tiles, `zeros` and `tiny` cut into row
stripes at (65, 3), (65, 8) and (130, 3) -- through run_hydraulic_lockstep, run_fluvial_lockstep, run_fill_lockstep,
run_drainage_lockstep and run_fluvial_implicit_lockstep of noize_job_amd.sharded with the numpy stripe ops as compute back
end, against the whole tile's model bit for bit.  It shows that the schedules (which rows are exchanged, which are
recomputed, who votes) are safe on heights that tie across the cuts, and that the fill's, the drainage's and the implicit
step's budgets hold every case -- the implicit step's rounds and the most Jacobi steps of one of its solve rounds are printed
and held to the figures of tests/sweep_stripe_cases.py, far inside 128 and 128 -- before tests/test_gpu_sweep_stripes.py asks
the kernels the same."""
import pytest

import sweep_stripe_cases as SC

MOST_IMPLICIT_ROUNDS, MOST_IMPLICIT_STEPS = 7, 66  # tiny 65^2 over 8, set 1; manh_pit 130^2 over 3, set 2

@pytest.fixture(scope="module")
def be():
    return SC.cpu_backend()


@pytest.mark.parametrize("name,res,world", SC.CASES)
def test_hydraulic_stripes_on_ties(be, oracle, name, res, world):
    assert SC.every_for(res, world) == (1, 2)
    SC.hydraulic(be, name, res, world)


@pytest.mark.parametrize("name,res,world", SC.CASES)
def test_fluvial_stripes_on_ties(be, name, res, world):
    SC.fluvial(be, name, res, world)


@pytest.mark.parametrize("name,res,world", SC.CASES)
def test_fill_stripes_on_ties(be, name, res, world):
    print("%s %d over %d: rounds %s" % (name, res, world, SC.fill(be, name, res, world)))


@pytest.mark.parametrize("name,res,world", SC.CASES)
def test_drainage_stripes_on_ties(be, name, res, world):
    print("%s %d over %d: rounds %s" % (name, res, world, SC.drainage(be, name, res, world)))


def implicit_rounds_and_steps(be, name, res, world):
    """SC.fluvial_implicit, its rounds and the most Jacobi steps one solve round of it took, held to the budget."""
    ops = be.ops["fluvial_implicit"]
    del ops.solve_steps[:]
    rounds = SC.fluvial_implicit(be, name, res, world)
    steps = max(ops.solve_steps)
    print("%s %d over %d: rounds %s, at most %d steps in a round" % (name, res, world, rounds, steps))
    # a round that used its last pass may not have been at rest: the budget holds a case that stays below it
    assert max(rounds) < SC.FLUVIAL_IMPLICIT_BUDGET["maxRounds"] and steps < SC.FLUVIAL_IMPLICIT_BUDGET["maxPasses"]
    return max(rounds), steps


@pytest.mark.parametrize("name,res,world", SC.CASES)
def test_fluvial_implicit_stripes_on_ties(be, name, res, world):
    rounds, steps = implicit_rounds_and_steps(be, name, res, world)
    assert rounds <= MOST_IMPLICIT_ROUNDS and steps <= MOST_IMPLICIT_STEPS  # the figures of the module docstring


@pytest.mark.parametrize("family", list(SC.FAMILIES))
def test_the_pitched_case_dense(be, oracle, family):
    """The numpy ops know no pitch: the tile, size and split of the GPU's padded-pitch case, dense."""
    name, res, world, _ = SC.PITCHED
    assert SC.every_for(res, world) == (1, 2)
    if family == "fluvial_implicit":
        implicit_rounds_and_steps(be, name, res, world)
    else:
        SC.FAMILIES[family](be, name, res, world)
