"""The implicit fluvial model (tests/fluvial_implicit_ref.py) without a GPU: a tile worked by hand, the schedules that must
agree, what follows from the model, batch independence and a control that the model really divides.  Bit for bit throughout."""
import numpy as np
import pytest

import drainage_ref as D
import fluvial_implicit_ref as R
import fluvial_ref as F
import terrain_tiles as T
from test_hydraulic_ref import relief

f32 = np.float32
_memo = {}


def tile(name, res):
    """(heights, exact drainage area) of a terrain_tiles family or of the relief tile, computed once, read only."""
    if (name, res) not in _memo:
        h = (np.ascontiguousarray(relief(res), f32) if name == "relief33" else
             np.ascontiguousarray(T.GENERATORS[name](res, np.random.default_rng(res + 7)), f32))
        A = D.accumulate(h)[0]
        h.setflags(write=False), A.setflags(write=False)
        _memo[(name, res)] = (h, A)
    return _memo[(name, res)]


def assert_same(got, want, what):
    assert got.dtype == want.dtype == f32 and got.shape == want.shape, what
    bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


HAND = np.array([[9, 9, 9, 9, 9],
                 [9, 5, 4, 3, 0],
                 [9, 6, 7, 2, 9],
                 [9, 8, 1, 8, 9],
                 [9, 9, 9, 9, 9]], f32)


def test_a_tile_worked_by_hand():
    # The tile of tests/test_watershed_ref.py: rows are z, columns x.  The receivers of the inner cells:
    #   (x1,z1)=5 -> E;  (2,1)=4 -> NE;  (3,1)=3 -> E, the low border cell (4,1);  (1,2)=6 -> NE;  (2,2)=7 -> N;
    #   (3,2)=2 -> SE, the low border cell;  (1,3)=8 -> E;  (2,3)=1: a pit;  (3,3)=8 -> W
    # A = 4 everywhere, erodibility 1/4, dt 2, uplift 1/4: du = 1/2, f = (1/4 * 2) * 1 * 2 = 1 along a cardinal move and
    # (1/2 * DIAG) * 2 = DIAG along a diagonal one, so a cardinal cell is the mean of h + 1/2 and its receiver.
    A = np.full((5, 5), 4, f32)
    kw = dict(erodibility=0.25, uplift=0.25, dt=2.0)
    has, q, b, f = R.coefficients(HAND, A, **kw)
    d, o = F.DIAG, f32(0.0)
    assert d == f32(0.70710677)
    assert_same(f, np.array([[o, o, o, o, o], [o, 1, d, 1, o], [o, d, 1, d, o], [o, 1, o, 1, o], [o, o, o, o, o]], f32), "f")
    assert_same(b, np.array([[9, 9, 9, 9, 9], [9, 5.5, 4.5, 3.5, 0], [9, 6.5, 7.5, 2.5, 9], [9, 8.5, 1.5, 8.5, 9],
                             [9, 9, 9, 9, 9]], f32), "b")
    one = f32(1.0)
    e32 = f32(f32(2.5) / f32(one + d))                        # (3,2) -> the border cell at 0
    e21 = f32(f32(f32(4.5) + f32(d * e32)) / f32(one + d))    # (2,1) -> (3,2)
    e11 = f32(f32(f32(5.5) + e21) / f32(2.0))                 # (1,1) -> (2,1)
    e12 = f32(f32(f32(6.5) + f32(d * f32(1.5))) / f32(one + d))  # (1,2) -> the pit at 1 + 1/2
    want = np.array([[9, 9, 9, 9, 9], [9, e11, e21, 1.75, 0], [9, e12, 4.5, e32, 9], [9, 5, 1.5, 5, 9], [9, 9, 9, 9, 9]], f32)
    # the same four written out
    assert [float(v).hex() for v in (e11, e21, e12, e32)] == ["0x1.17c3b60000000p+2", "0x1.9f0ed80000000p+1",
                                                              "0x1.1b73a00000000p+2", "0x1.76e7400000000p+0"]
    assert_same(R.walk(HAND, A, **kw), want, "walk by hand")
    for start in ("b", "h"):
        got, steps = R.jacobi(HAND, A, start=start, **kw)
        assert steps == 3  # the longest path has three moves
        assert_same(got, want, "jacobi from " + start)
    assert_same(R.tiled(HAND, A, tile=(2, 2), sweeps=1, **kw)[0], want, "2 x 2 tiles")
    # one more Jacobi step over the fixed point changes no bit
    assert_same(R.step(want, has, q, b, f), want, "fixed point")


@pytest.mark.parametrize("res", (33, 65))
@pytest.mark.parametrize("name", ["relief33"] + sorted(T.GENERATORS))
def test_walk_jacobi_and_tile_sweeps_end_in_the_same_bits(name, res):
    h, A = tile(name, res)
    for dt in (1.0, 200.0):
        kw = dict(dt=dt)
        want = R.walk(h, A, **kw)
        assert_same(R.jacobi(h, A, **kw)[0], want, "jacobi dt %g" % dt)
        assert_same(R.jacobi(h, A, start="h", **kw)[0], want, "jacobi from h dt %g" % dt)
        for cap in (1, 3, 16):
            assert_same(R.tiled(h, A, sweeps=cap, **kw)[0], want, "tiled cap %d dt %g" % (cap, dt))
        has, q, b, f = R.coefficients(h, A, **kw)
        assert_same(R.step(want, has, q, b, f), want, "fixed point dt %g" % dt)


def test_maps_and_a_sea_through_every_schedule():
    h, A = tile("relief33", 65)
    rng = np.random.default_rng(3)
    kw = dict(dt=50.0, seaLevel=T.sea_at(h), hardness=rng.random(h.shape, dtype=f32),
              upliftMap=rng.random(h.shape, dtype=f32) * f32(2.0))
    A = D.accumulate(h, seaLevel=kw["seaLevel"])[0]
    want = R.walk(h, A, **kw)
    assert_same(R.jacobi(h, A, **kw)[0], want, "jacobi")
    assert_same(R.tiled(h, A, sweeps=3, **kw)[0], want, "tiled")
    sea = F.outlets(h, kw["seaLevel"])
    assert sea[1:-1, 1:-1].any()
    assert_same(want[sea], h[sea], "outlets keep their bits")
    assert not R.same(want, R.walk(h, A, dt=50.0, seaLevel=kw["seaLevel"]))  # the maps do something


@pytest.mark.parametrize("name", ["relief33"] + sorted(T.GENERATORS))
def test_without_erodibility_only_the_uplift_is_left_and_outlets_keep_their_bits(name):
    h, A = tile(name, 33)
    out = F.outlets(h)
    for dt in (1.0, 200.0):
        got = R.walk(h, A, erodibility=0.0, dt=dt)
        du = f32(dt) * f32(0.002)
        # f = +0: (b + 0 * q) / 1 = b; array_equal, as b = -0 comes back as +0 when 0 * q is +0
        assert np.array_equal(got[~out], (h + du)[~out])
        assert_same(got[out], h[out], "outlets")
        assert_same(R.walk(h, A, dt=dt)[out], h[out], "outlets, eroding")


BOUNDED = ("relief33", "relief", "noisy", "metres", "negative", "wide", "uniform", "cheb_cone", "manh_cone", "cheb_pit",
           "manh_pit")


@pytest.mark.parametrize("res", (33, 65))
@pytest.mark.parametrize("name", BOUNDED)
def test_a_cell_ends_between_its_receiver_and_its_uplifted_height(name, res):
    """h'[q] <= h'[c] <= h[c] + du holds in exact arithmetic without an upliftMap: h' is a mean of b and h'[q] with weights
    1 / (1 + f) and f / (1 + f), and by induction from the roots h'[q] <= h[q] + du < h[c] + du.  In float32 it is asserted
    on the families whose neighbouring heights differ by far more than an ulp of the result; it is NOT asserted on `tiny`
    (subnormal differences: the quotient's rounding is larger than the gap between a cell and its receiver) and `zeros`
    (+-0 and +-1e-45: b and q are equal or one ulp apart and rounding decides the order), nor on terraces and checker,
    which the statement was not checked on."""
    h, A = tile(name, res)
    for dt in (1.0, 200.0):
        has, q, b, f = R.coefficients(h, A, dt=dt)
        got = R.walk(h, A, dt=dt)
        recv = got.reshape(-1)[q]
        assert (recv[has] <= got[has]).all(), dt
        assert (got[has] <= b[has]).all(), dt


def test_a_batch_is_its_tiles_one_by_one():
    tiles = [tile(n, 33) for n in ("relief", "noisy", "terraces4")]
    single = [R.walk(h, A, dt=20.0) for h, A in tiles]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        hs = np.stack([tiles[i][0] for i in order])
        As = np.stack([tiles[i][1] for i in order])
        got = np.stack([R.walk(hs[i], As[i], dt=20.0) for i in range(3)])
        for pos, i in enumerate(order):
            assert_same(got[pos], single[i], "position %d of %s" % (pos, order))
    # ... and not a plane of three tiles on top of each other: that one has no border between them
    h3, A3 = np.concatenate([t[0] for t in tiles]), np.concatenate([t[1] for t in tiles])
    assert not R.same(R.walk(h3, A3, dt=20.0)[:33], single[0])


def test_the_model_divides_twice_the_step_is_not_twice_the_change():
    h, A = tile("relief33", 33)
    one, two = R.walk(h, A, uplift=0.0, dt=100.0), R.walk(h, A, uplift=0.0, dt=200.0)
    assert not np.array_equal(two - h, f32(2.0) * (one - h))
    # and a very large step stays bounded where the explicit scheme's limiter would have taken over: nothing below an outlet
    big = R.walk(h, A, uplift=0.0, dt=1e6)
    assert np.isfinite(big).all() and big.min() >= h[F.outlets(h)].min()


def test_the_long_chain():
    """drainage_ref.serpentine(): one channel of 12 403 moves.  Jacobi comes to rest long before the chain's length: far from
    the mouth the recurrence has forgotten the outlet to the last bit."""
    h = D.serpentine()
    A = D.accumulate(h)[0]
    want = R.walk(h, A)
    got, steps = R.jacobi(h, A, start="h")
    assert_same(got, want, "jacobi")
    assert 40 < steps <= 12405
    has, q, b, f = R.coefficients(h, A)
    assert_same(R.step(want, has, q, b, f), want, "fixed point")
