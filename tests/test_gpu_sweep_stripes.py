"""Five stripe entries on the GPU -- nz_hydraulic_stripe, nz_fluvial_stripe, nz_fill_stripe(_finalise),
nz_drainage_stripe_round(_finalise), nz_implicit_fluvial_stripe_round(_finalise) through HipStripeOps and the run_*_lockstep
drivers -- on the stripe sweep of
tests/sweep_stripe_cases.py: the tie tiles, `zeros` and `tiny` cut into row stripes at (65, 3), (65, 8) and (130, 3), and
terraces16 at 67 over 3 ranks with a pitch of 72 floats on every plane, against the whole tile's model bit for bit in every
plane the family returns.  Heights tie across every cut (tests/test_terrain_tiles.py), so the first-lowest-wins order of a
receiver chosen among ghost-row cells, a `<=` against a sea level in a ghost row and a flat without a receiver that spans
a cut have to agree with the whole grid's.  The implicit entry runs its driver's whole iteration on each stripe -- the
drainage rounds, then the solve rounds against one frozen ghost row of h' -- on the tiles as they are, twice over in its
second parameter set: a ghost-row receiver that the two kinds of round chose differently would show in the drainage area or
in the heights.  tests/test_sweep_stripes_ref.py runs the same cases through the numpy stripe ops
and shows that the budgets hold them: a stripe run that does not converge here is a finding."""
import pytest

import sweep_stripe_cases as SC
from fill_stripe_cases import stripe_ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(nj):
    """fill_stripe_cases.stripe_ops, once for the module, behind the sweep's back end."""
    with stripe_ops(nj) as (sh, ops):
        yield SC.gpu_backend(nj, sh, ops)


@pytest.mark.parametrize("name,res,world", SC.CASES)
def test_hydraulic_stripes_on_ties(be, oracle, name, res, world):
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


@pytest.mark.parametrize("name,res,world", SC.CASES)
def test_fluvial_implicit_stripes_on_ties(be, name, res, world):
    print("%s %d over %d: rounds %s" % (name, res, world, SC.fluvial_implicit(be, name, res, world)))


@pytest.mark.parametrize("family", list(SC.FAMILIES))
def test_a_padded_pitch(be, oracle, family):
    """Every plane of every rank at 72 floats a row for 67 columns; the pad floats keep their NaN."""
    name, res, world, pitch = SC.PITCHED
    assert pitch > res and be.pitch(pitch) == pitch
    SC.FAMILIES[family](be, name, res, world, pitch)
