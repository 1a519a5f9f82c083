"""The multiple-flow implicit fluvial model (tests/fluvial_implicit_mfd_ref.py) without a GPU: 3^2 and 4^2 tiles worked by
hand as rationals, the schedules that must agree bit for bit, the single-weight closure against the single-flow model, and
what follows from the model (zero erodibility, outlets, the exact-arithmetic bounds, NaN, Jacobi steps <= DAG height)."""
from fractions import Fraction

import numpy as np
import pytest

import drainage_mfd_ref as M
import fill_stripe_cases as S
import fluvial_implicit_mfd_ref as R
import fluvial_implicit_ref as R1
import fluvial_ref as F

f32 = np.float32
DIAGQ = Fraction(float(F.DIAG))  # the float32 constant as the rational it is
_memo = {}


def assert_same(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def filled(name, exponent):
    """(filled heights, multiple-flow drainage, DAG height of the drainage) of a fill_stripe_cases grid, computed once."""
    if (name, exponent) not in _memo:
        h = np.ascontiguousarray(S.flood(name), f32)
        A, height = M.walk(h, exponent=exponent)
        h.setflags(write=False), A.setflags(write=False)
        _memo[(name, exponent)] = (h, A, height)
    return _memo[(name, exponent)]


def rational_model(h, A, erodibility, uplift, dt, exponent):
    """The model's text over the rationals (small integer heights, square A, DIAG the float32 constant), cells lowest first."""
    rows, cols = h.shape
    hq = [[Fraction(int(v)) for v in row] for row in h]
    du, kc, dtq = Fraction(dt) * Fraction(uplift), Fraction(erodibility), Fraction(dt)
    out = [row[:] for row in hq]
    for _, x, z in sorted((hq[z][x], x, z) for z in range(1, rows - 1) for x in range(1, cols - 1)):
        s = {}
        for k, (dx, dz) in enumerate(F.NEIGHBOURS):
            d = hq[z][x] - hq[z + dz][x + dx]
            if d > 0:
                s[k] = d if k < 4 else d * DIAGQ
        b = hq[z][x] + du
        if not s:
            out[z][x] = b
            continue
        best = max(s.values())
        g = {k: (v / best) ** exponent for k, v in s.items()}
        total = sum(g.values())
        e = kc * Fraction(int(round(float(A[z, x]) ** 0.5)))
        N, D = b, Fraction(1)
        for k in sorted(g):
            f = e * (1 if k < 4 else DIAGQ) * dtq * (g[k] / total)
            N += f * out[z + F.NEIGHBOURS[k][1]][x + F.NEIGHBOURS[k][0]]
            D += f
        out[z][x] = N / D
    return np.array([[float(v) for v in row] for row in out], np.float64)


KW = dict(erodibility=0.25, uplift=0.25, dt=2.0)  # with A = 4: du = 1/2, e = 1/2, f = w along a cardinal move


def test_three_by_three_tiles_worked_by_hand():
    A = np.full((3, 3), 4, f32)
    # one lower neighbour, E: w = 1, f = 1, h' = (4.5 + 1 * 2) / 2
    one = np.array([[9, 9, 9], [9, 4, 2], [9, 9, 9]], f32)
    # two lower neighbours, W and E, equal slopes: w = 1/2 each, h' = (4.5 + 1/2 * 2 + 1/2 * 2) / 2
    two = np.array([[9, 9, 9], [2, 4, 2], [9, 9, 9]], f32)
    # three: W at slope 2 and S, N at slope 1: q = 1, 1/2, 1/2, T = 2, w = 1/2, 1/4, 1/4;
    # N = 4.5 + 1/2 * 2 + 1/4 * 3 + 1/4 * 3 = 7, D = 2
    three = np.array([[9, 3, 9], [2, 4, 9], [9, 3, 9]], f32)
    # the same at exponent 2: g = 1, 1/4, 1/4, T = 3/2: not dyadic, so against the rationals below only
    for h, centre, gates in ((one, 3.25, [1]), (two, 3.25, [0, 1]), (three, 3.5, [0, 2, 3])):
        G, b, Fk = R.coefficients(h, A, **KW)
        assert np.flatnonzero(G[:, 1, 1]).tolist() == gates and G.sum() == len(gates)
        assert b[1, 1] == f32(4.5) and Fk[:, 1, 1].sum() == f32(1.0)
        want = h.copy()
        want[1, 1] = centre
        got, height = R.walk(h, A, **KW)
        assert height == 2
        assert_same(got, want, "walk")
        for start in ("b", "h"):
            got, steps = R.jacobi(h, A, start=start, **KW)
            assert steps <= 1
            assert_same(got, want, "jacobi from " + start)
        assert_same(R.step(want, G, b, Fk), want, "fixed point")
    # a diagonal among three, at exponents 1 and 2, against the rationals: SW at 1, E at 2, N at 3 under a centre of 4
    diag = np.array([[1, 9, 9], [9, 4, 2], [9, 3, 9]], f32)
    for exponent in (1, 2, 4):
        got = R.walk(diag, A, exponent=exponent, **KW)[0]
        want = rational_model(diag, A, exponent=exponent, **KW)
        assert np.flatnonzero(R.coefficients(diag, A, exponent=exponent, **KW)[0][:, 1, 1]).tolist() == [1, 3, 4]
        np.testing.assert_allclose(got, want, rtol=4e-7, atol=0)
        assert want[1, 1] < 4.5 and want[1, 1] > 1


HAND4 = np.array([[9, 9, 9, 9],
                  [9, 5, 4, 0],
                  [9, 6, 3, 9],
                  [9, 9, 9, 9]], f32)


def test_a_four_by_four_tile_worked_by_hand():
    # rows are z, columns x; S is z - 1, N is z + 1.  The gates of the inner cells:
    #   (2,2)=3: SE, the low border cell (3,1): one;      (2,1)=4: E, the border cell, and N, (2,2): two;
    #   (1,1)=5: E, (2,1), and NE, (2,2): two, a diagonal;  (1,2)=6: E, (2,2), S, (1,1), SE, (2,1): three, a diagonal
    A = np.full((4, 4), 4, f32)
    for exponent in (1, 2, 4):
        kw = dict(KW, exponent=exponent)
        G, b, Fk = R.coefficients(HAND4, A, **kw)
        gates = {(x, z): np.flatnonzero(G[:, z, x]).tolist() for z in (1, 2) for x in (1, 2)}
        assert gates == {(2, 2): [5], (2, 1): [1, 3], (1, 1): [1, 7], (1, 2): [1, 2, 5]}
        assert G[:, 0].sum() == G[:, -1].sum() == G[:, :, 0].sum() == G[:, :, -1].sum() == 0  # a border cell sends nothing
        got, height = R.walk(HAND4, A, **kw)
        assert height == 5  # border, (2,2), (2,1), (1,1), (1,2)
        np.testing.assert_allclose(got, rational_model(HAND4, A, exponent=exponent, **KW), rtol=1e-6, atol=0)
        for start in ("b", "h"):
            j, steps = R.jacobi(HAND4, A, start=start, **kw)
            assert steps <= height
            assert_same(j, got, "jacobi from " + start)
        assert_same(R.tiled(HAND4, A, tile=(2, 2), sweeps=1, **kw)[0], got, "2 x 2 tiles")
        assert_same(R.step(got, G, b, Fk), got, "fixed point")
    # (2,2) has one positive weight: w == 1 and the single-flow recurrence, written out
    d = F.DIAG
    got = R.walk(HAND4, A, **KW)[0]
    assert_same(got[2, 2], f32(f32(f32(3.5) + f32(d * f32(0.0))) / f32(f32(1.0) + d)), "(2,2)")


@pytest.mark.parametrize("exponent", (1, 4))
@pytest.mark.parametrize("name", ("pitted", "bowl", "serpentine"))
def test_walk_jacobi_and_tile_sweeps_end_in_the_same_bits(name, exponent):
    h, A, _ = filled(name, exponent)
    for dt in (1.0, 200.0):
        kw = dict(dt=dt, exponent=exponent)
        want, height = R.walk(h, A, **kw)
        for start in ("b", "h"):
            got, steps = R.jacobi(h, A, start=start, **kw)
            assert steps <= height, (start, dt, steps, height)  # a Jacobi step settles one more level of the DAG
            assert_same(got, want, "jacobi from %s dt %g" % (start, dt))
        for cap in (1, 3, 16):
            assert_same(R.tiled(h, A, sweeps=cap, **kw)[0], want, "tiled cap %d dt %g" % (cap, dt))
        G, b, Fk = R.coefficients(h, A, **kw)
        assert_same(R.step(want, G, b, Fk), want, "fixed point dt %g" % dt)
        assert np.isfinite(want).all()


@pytest.mark.parametrize("exponent", (1, 4))
@pytest.mark.parametrize("name", ("pitted", "bowl", "serpentine"))
def test_on_the_single_weight_closure_the_model_is_the_single_flow_one(name, exponent):
    h, A, _ = filled(name, exponent)
    closed = R.single_closure(h, exponent=exponent)
    single = (M.weights(h, exponent=exponent) > 0).sum(axis=0) == 1
    assert not (closed & ~single).any()
    if name == "serpentine":
        # the channel and the plateau's rim: every single-weight cell lies on a path of single-weight cells
        assert closed.sum() == single.sum() >= 600
    for dt in (1.0, 200.0):
        got = R.walk(h, A, dt=dt, exponent=exponent)[0]
        want = R1.walk(h, A, dt=dt)  # the same A: only the routing of the solve differs
        assert_same(got[closed], want[closed], "%s closure dt %g" % (name, dt))
        if name != "serpentine":
            assert not R.same(got, want)  # ... and off the closure the two models differ


def test_without_erodibility_only_the_uplift_is_left_and_outlets_keep_their_bits():
    for name in ("pitted", "bowl"):
        h, A, _ = filled(name, 1)
        sea = f32(np.median(h))
        for s in (F.SEA_OFF, sea):
            out = F.outlets(h, s)
            for dt in (1.0, 200.0):
                got = R.walk(h, A, erodibility=0.0, dt=dt, seaLevel=s)[0]
                du = f32(dt) * f32(0.002)
                assert np.array_equal(got[~out], (h + du)[~out])
                assert_same(got[out], h[out], "outlets")
                assert_same(R.walk(h, A, dt=dt, seaLevel=s, exponent=4)[0][out], h[out], "outlets, eroding")
        assert F.outlets(h, sea)[1:-1, 1:-1].any()


def test_maps_and_a_sea_through_every_schedule():
    h, _, _ = filled("pitted", 1)
    rng = np.random.default_rng(3)
    sea = f32(np.quantile(h, 0.3))
    kw = dict(dt=50.0, seaLevel=sea, exponent=2, hardness=rng.random(h.shape, dtype=f32),
              upliftMap=rng.random(h.shape, dtype=f32) * f32(2.0))
    A = M.walk(h, seaLevel=sea, exponent=2)[0]
    want = R.walk(h, A, **kw)[0]
    assert_same(R.jacobi(h, A, **kw)[0], want, "jacobi")
    assert_same(R.tiled(h, A, sweeps=3, **kw)[0], want, "tiled")
    assert not R.same(want, R.walk(h, A, dt=50.0, seaLevel=sea, exponent=2)[0])  # the maps do something


def walk64(h, A, **kw):
    """The model in float64 on the float32 coefficients' gates: what "exact arithmetic" means for the bounds."""
    G, _, _ = R.coefficients(h, A, **kw)
    W = M._weights(h, kw.get("seaLevel", F.SEA_OFF), kw.get("exponent", 1), np.float64, float(np.sqrt(0.5)))
    dt, du = float(kw.get("dt", 1.0)), float(kw.get("dt", 1.0)) * 0.002
    e = 0.05 * np.sqrt(np.asarray(A, np.float64))
    h64 = np.asarray(h, np.float64)
    b = np.where(F.outlets(np.asarray(h, f32)), h64, h64 + du)
    hn = b.reshape(-1).copy()
    cols = h.shape[1]
    low = np.full(h.size, np.inf)
    for c in np.argsort(h64.reshape(-1), kind="stable").tolist():
        z, x = divmod(c, cols)
        if not G[:, z, x].any():
            continue
        n, d = hn[c], 1.0
        for k, (dx, dz) in enumerate(F.NEIGHBOURS):
            if G[k, z, x]:
                q = c + dz * cols + dx
                f = e[z, x] * (1.0 if k < 4 else float(np.sqrt(0.5))) * dt * W[k, z, x]
                n, d = n + f * hn[q], d + f
                low[c] = min(low[c], hn[q])
        hn[c] = n / d
    return hn.reshape(h.shape), low.reshape(h.shape), b, G.any(axis=0)


@pytest.mark.parametrize("name", ("pitted", "bowl", "serpentine"))
def test_in_exact_arithmetic_a_cell_ends_between_its_lowest_target_and_its_uplifted_height(name):
    """min_k h'[k] <= h'[c] <= h[c] + du without an upliftMap: h' is a mean of b and the h'[k] with positive weights
    1 / D and f_k / D, and by induction from the leaves h'[k] <= h[k] + du < h[c] + du.  Asserted in float64, where the
    rounding of a mean is far below the gaps of these grids (the fill's epsilon, 1e-4); a relative 1e-12 allows for it."""
    for exponent in (1, 4):
        h, A, _ = filled(name, exponent)
        for dt in (1.0, 200.0):
            got, low, b, opens = walk64(h, A, dt=dt, exponent=exponent)
            slack = 1e-12 * np.abs(b)
            assert (low[opens] <= got[opens] + slack[opens]).all(), (exponent, dt)
            assert (got[opens] <= b[opens] + slack[opens]).all(), (exponent, dt)
            np.testing.assert_allclose(R.walk(h, A, dt=dt, exponent=exponent)[0], got, rtol=2e-5)


def test_nan_heights_send_and_receive_nothing_and_a_nan_area_travels_upstream():
    h, A, _ = filled("pitted", 1)
    h = h.copy()
    z, x = 30, 40
    h[z, x] = np.nan
    A2 = M.walk(h)[0]
    G, b, Fk = R.coefficients(h, A2, dt=20.0)
    assert not G[:, z, x].any()  # it sends nothing ...
    for k, (dx, dz) in enumerate(F.NEIGHBOURS):
        assert not G[F.OPPOSITE[k], z + dz, x + dx]  # ... and no neighbour sends to it
    got = R.walk(h, A2, dt=20.0)[0]
    assert np.isnan(got[z, x]) and np.isnan(got).sum() == 1
    assert_same(R.jacobi(h, A2, dt=20.0)[0], got, "jacobi with a NaN height")
    assert_same(R.tiled(h, A2, sweeps=3, dt=20.0)[0], got, "tiled with a NaN height")
    # a NaN (or negative) A: that cell and every cell that drains through it
    h, A, _ = filled("pitted", 1)
    for bad in (np.nan, -1.0):
        A3 = A.copy()
        A3[z, x] = bad
        got = R.walk(h, A3, dt=20.0)[0]
        G, b, Fk = R.coefficients(h, A3, dt=20.0)
        assert G[:, z, x].any() and np.isnan(got[z, x])
        up = np.zeros(h.shape, bool)
        up[z, x] = True
        for c in np.argsort(h.reshape(-1), kind="stable").tolist():  # upstream closure, lowest first
            cz, cx = divmod(c, h.shape[1])
            for k, (dx, dz) in enumerate(F.NEIGHBOURS):
                if G[k, cz, cx] and up[cz + dz, cx + dx]:
                    up[cz, cx] = True
        assert up.sum() > 1 and np.array_equal(np.isnan(got), up)
        assert_same(R.jacobi(h, A3, dt=20.0)[0], got, "jacobi with a bad A")
    # an f that overflows gives NaN
    big = R.walk(h, A, erodibility=3e38, dt=3e38)[0]
    assert np.isnan(big[R.coefficients(h, A)[0].any(axis=0)]).all()


def test_a_batch_is_its_tiles_one_by_one_and_the_chain_iterates():
    h, _, _ = filled("bowl", 1)
    got, A = R.chain(h, 2, dt=50.0, exponent=4)
    A1 = M.walk(h, exponent=4)[0]
    h1 = R.walk(h, A1, dt=50.0, exponent=4)[0]
    A2 = M.walk(h1, exponent=4)[0]
    assert_same(A, A2, "the chain's drainage is the last iteration's")
    assert_same(got, R.walk(h1, A2, dt=50.0, exponent=4)[0], "two iterations")
    assert not R.same(got, h1)
