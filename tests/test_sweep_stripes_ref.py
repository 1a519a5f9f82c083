"""The stripe sweep on the CPU: every case of tests/sweep_stripe_cases.py -- the tie tiles, `zeros` and `tiny` cut into row
stripes at (65, 3), (65, 8) and (130, 3) -- through run_hydraulic_lockstep, run_fluvial_lockstep, run_fill_lockstep and
run_drainage_lockstep of noize_job_amd.sharded with the numpy stripe ops as compute back end, against the whole tile's
model bit for bit.  It shows that the schedules (which rows are exchanged, which are recomputed, who votes) are safe on
heights that tie across the cuts, and that the fill's and the drainage's budgets hold every case, before
tests/test_gpu_sweep_stripes.py asks the kernels the same."""
import pytest

import sweep_stripe_cases as SC


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


@pytest.mark.parametrize("family", list(SC.FAMILIES))
def test_the_pitched_case_dense(be, oracle, family):
    """The numpy ops know no pitch: the tile, size and split of the GPU's padded-pitch case, dense."""
    name, res, world, _ = SC.PITCHED
    assert SC.every_for(res, world) == (1, 2)
    SC.FAMILIES[family](be, name, res, world)
