"""The sediment model (tests/fluvial_sediment_ref.py) without a GPU: two tiles worked by hand as rationals, the schedules that
must agree, the closure on the implicit model, and what follows from the model.  Bit for bit throughout."""
from fractions import Fraction as Q

import numpy as np
import pytest

import drainage_ref as D
import fill_ref
import fluvial_implicit_ref as R
import fluvial_ref as F
import fluvial_sediment_ref as S
import terrain_tiles as T
from test_hydraulic_ref import relief

f32 = np.float32
_memo = {}


def tile(name, res):
    """(heights, exact drainage area) of a terrain_tiles family, of `faint` or of the relief tile, computed once, read only."""
    if (name, res) not in _memo:
        if name == "relief33":
            h = np.ascontiguousarray(relief(res), f32)
        elif name == "faint":  # relief so faint that most differences are a few ulps of the heights
            h = (f32(1000.0) + np.ascontiguousarray(relief(res), f32) * f32(1e-4)).astype(f32)
        else:
            h = np.ascontiguousarray(T.GENERATORS[name](res, np.random.default_rng(res + 7)), f32)
        A = D.accumulate(h)[0]
        h.setflags(write=False), A.setflags(write=False)
        _memo[(name, res)] = (h, A)
    return _memo[(name, res)]


def filled(res=65):
    if ("filled", res) not in _memo:
        h = fill_ref.flood(np.ascontiguousarray(relief(res), f32))
        _memo[("filled", res)] = (h, D.accumulate(h)[0])
    return _memo[("filled", res)]


def assert_same(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def exact(plane):
    return [[Q(float(v)) for v in row] for row in plane]


# ---- two tiles by hand ---------------------------------------------------------------------------------------------------
# A = 4 everywhere, erodibility 1/4, dt 2: f = ((1/4 * 2) * 1) * 2 = 1 along a cardinal move, so a cell with a receiver is the
# mean of its b and its receiver; uplift 1/4: du = 1/2.  Every number below is a dyadic rational that float32 holds exactly.
HAND4 = np.array([[9, 9, 9, 9],
                  [9, 4, 2, 0],
                  [9, 16, 8, 9],
                  [9, 9, 9, 9]], f32)


def test_a_confluence_worked_by_hand():
    # rows are z, columns x.  a = (1,1) = 4 -> E; b = (2,1) = 2 -> E, the low border cell (3,1); c = (1,2) = 16 -> S, to a
    # (drop 12 against 14 * DIAG to b); d = (2,2) = 8 -> S, to b (drop 6 against 8 * DIAG to the border cell).  b is a
    # confluence: its donors are a, neighbour 0 (W), and d, neighbour 3 (N), added in that order.
    A = np.full((4, 4), 4, f32)
    kw = dict(erodibility=0.25, uplift=0.25, dt=2.0)
    r = F.receivers(HAND4)[0]
    assert (r[1, 1], r[1, 2], r[2, 1], r[2, 2]) == (1, 1, 2, 2)
    half = Q(1, 2)
    b0 = dict(a=Q(4) + half, b=Q(2) + half, c=Q(16) + half, d=Q(8) + half)
    h0 = {}
    h0["b"] = (b0["b"] + 0) / 2
    h0["a"] = (b0["a"] + h0["b"]) / 2
    h0["d"] = (b0["d"] + h0["b"]) / 2
    h0["c"] = (b0["c"] + h0["a"]) / 2
    assert h0 == dict(b=Q(5, 4), a=Q(23, 8), d=Q(39, 8), c=Q(155, 16))
    e = {k: b0[k] - h0[k] for k in b0}
    flux = dict(c=e["c"], d=e["d"])
    flux["a"] = e["a"] + flux["c"]
    flux["b"] = (e["b"] + flux["a"]) + flux["d"]  # W first, then N
    flux["out"] = Q(0) + flux["b"]
    assert flux == dict(c=Q(109, 16), d=Q(29, 8), a=Q(135, 16), b=Q(213, 16), out=Q(213, 16))
    qin = dict(c=Q(0), d=Q(0), a=flux["c"], b=(Q(0) + flux["a"]) + flux["d"])
    G = half
    b1 = {k: b0[k] + (G * qin[k]) / 4 for k in b0}
    h1 = {}
    h1["b"] = (b1["b"] + 0) / 2
    h1["a"] = (b1["a"] + h1["b"]) / 2
    h1["d"] = (b1["d"] + h1["b"]) / 2
    h1["c"] = (b1["c"] + h1["a"]) / 2
    assert h1["b"] == Q(513, 256) and h1["a"] == Q(3766, 1024)
    got, gflux, residual, series = S.walk(HAND4, A, deposition=0.5, sedimentIterations=1, **kw)
    where = dict(a=(1, 1), b=(1, 2), c=(2, 1), d=(2, 2))
    for k, (z, x) in where.items():
        assert Q(float(got[z, x])) == h1[k], k
        assert Q(float(gflux[z, x])) == flux[k], k
    assert Q(float(gflux[1, 3])) == flux["out"]  # the flux of an outlet is the sum entering it
    out = F.outlets(HAND4)
    assert_same(got[out], HAND4[out], "outlets untouched")
    assert np.count_nonzero(gflux[out]) == 1
    assert Q(float(residual)) == max(h1[k] - h0[k] for k in h1) == h1["a"] - h0["a"] and series == [residual]
    # the donor order matters to the model: with N before W the sum differs when it is not exact -- here it is exact, so the
    # order is pinned through the receivers' codes instead
    for name, run in (("jacobi", S.jacobi), ("tiled", lambda *a, **k: S.tiled(*a, tile=(2, 2), sweeps=1, **k))):
        j = run(HAND4, A, deposition=0.5, sedimentIterations=1, **kw)
        assert_same(j[0], got, name), assert_same(j[1], gflux, name + ": flux")
        assert j[2] == residual


# a channel along row 1 to the low border cell (4,1), a row of 16 above it and a row of 32 above that: every cell of rows 2
# and 3 drains S (16 - 3 = 13 against 14 * DIAG, and so on), so every channel cell is a confluence of its W and its N donor
HAND5 = np.array([[64, 64, 64, 64, 64],
                  [64, 3, 2, 1, 0],
                  [64, 16, 16, 16, 64],
                  [64, 32, 32, 32, 64],
                  [64, 64, 64, 64, 64]], f32)


def test_a_tree_worked_by_hand_over_two_iterations():
    A = np.full((5, 5), 4, f32)
    A[3, 2] = 0  # a cell without area takes no deposit
    kw = dict(erodibility=0.25, uplift=0.0, dt=2.0)
    r = F.receivers(HAND5)[0]
    assert r[1, 1:4].tolist() == [1, 1, 1] and (r[2:4, 1:4] == 2).all()
    # (3,2) has A = 0: f = +0 there, the cell keeps its b
    b0 = exact(HAND5)

    def solve(b):
        h = [row[:] for row in b]
        for x in (3, 2, 1):
            h[1][x] = (b[1][x] + h[1][x + 1]) / 2
        for x in (1, 2, 3):
            h[2][x] = (b[2][x] + h[1][x]) / 2
            h[3][x] = (b[3][x] + h[2][x]) / 2 if x != 2 else b[3][x]
        return h

    hk = solve(b0)
    first = None
    for k in range(2):
        e = [[b0[z][x] - hk[z][x] for x in range(5)] for z in range(5)]
        flux = [row[:] for row in e]
        for x in (1, 2, 3):
            flux[2][x] = e[2][x] + flux[3][x]
        for x in (1, 2, 3):
            flux[1][x] = (e[1][x] + flux[1][x - 1] if x > 1 else e[1][x]) + flux[2][x]  # W (neighbour 0), then N (3)
        flux[1][4] = e[1][4] + flux[1][3]
        qin = [[Q(0)] * 5 for _ in range(5)]
        for x in (1, 2, 3):
            qin[2][x] = flux[3][x]
            qin[1][x] = (flux[1][x - 1] if x > 1 else Q(0)) + flux[2][x]
        bk = [[b0[z][x] + (1 * qin[z][x]) / 4 if 1 <= z <= 3 and 1 <= x <= 3 and (z, x) != (3, 2) else b0[z][x]
               for x in range(5)] for z in range(5)]
        nxt = solve(bk)
        residual = max(abs(nxt[z][x] - hk[z][x]) for z in range(5) for x in range(5))
        hk = nxt
        first = first or residual
    got, gflux, gres, series = S.walk(HAND5, A, deposition=1.0, sedimentIterations=2, **kw)
    assert exact(got) == hk and exact(gflux) == flux
    assert [Q(float(v)) for v in series] == [first, residual] and Q(float(gres)) == residual and residual < first
    assert got[3, 2] == HAND5[3, 2] and gflux[3, 2] == 0 and qin[2][2] == 0
    assert flux[1][4] == sum(sum(row) for row in e)  # everything given up leaves through the one outlet that is fed
    j = S.jacobi(HAND5, A, deposition=1.0, sedimentIterations=2, **kw)
    assert_same(j[0], got, "jacobi"), assert_same(j[1], gflux, "jacobi: flux")


# ---- the schedules ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["relief33", "faint"] + sorted(T.GENERATORS))
def test_walk_jacobi_and_tile_sweeps_end_in_the_same_bits(name):
    h, A = tile(name, 33)
    for dt, G in ((1.0, 0.5), (200.0, 1.0)):
        kw = dict(dt=dt, deposition=G, sedimentIterations=2)
        want = S.walk(h, A, **kw)
        j = S.jacobi(h, A, **kw)
        assert_same(j[0], want[0], "jacobi dt %g" % dt), assert_same(j[1], want[1], "jacobi dt %g: flux" % dt)
        assert j[3] == want[3]
        for cap in (1, 3, 16):
            t = S.tiled(h, A, tile=(16, 8), sweeps=cap, **kw)  # 33^2 in 3 x 5 tiles
            assert_same(t[0], want[0], "tiled cap %d dt %g" % (cap, dt))
            assert_same(t[1], want[1], "tiled cap %d dt %g: flux" % (cap, dt))
            assert t[3] == want[3]


def test_the_kernel_s_tiles_on_relief():
    h, A = tile("relief33", 97)
    kw = dict(dt=50.0, deposition=1.0, sedimentIterations=1)
    want = S.walk(h, A, **kw)
    t = S.tiled(h, A, sweeps=16, **kw)
    assert_same(t[0], want[0], "64 x 16 tiles"), assert_same(t[1], want[1], "64 x 16 tiles: flux")


@pytest.mark.parametrize("name", ["relief33", "faint"] + sorted(T.GENERATORS))
def test_no_deposition_or_no_iterations_is_the_implicit_model(name):
    h, A = tile(name, 33)
    for dt in (1.0, 200.0):
        plain = R.walk(h, A, dt=dt)
        got = S.walk(h, A, dt=dt, sedimentIterations=0, deposition=1.0)
        assert_same(got[0], plain, "K = 0"), assert_same(got[1], np.zeros_like(h), "K = 0: flux")
        assert got[2] == 0 and got[3] == []
        got = S.walk(h, A, dt=dt, sedimentIterations=3, deposition=0.0)
        assert_same(got[0], plain, "G = 0")
        assert got[2] == 0


# ---- what follows from the model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["relief33", "noisy", "metres", "negative", "terraces16", "cheb_pit"])
def test_deposition_only_lifts_and_outlets_keep_their_bits(name):
    h, A = tile(name, 33)
    sea = T.sea_at(h)
    A = D.accumulate(h, seaLevel=sea)[0]
    for dt, G in ((1.0, 0.5), (200.0, 1.0), (200.0, 2.0)):
        hist = S.history(h, A, dt=dt, deposition=G, sedimentIterations=3, seaLevel=sea)
        h0 = hist[0][0]
        assert_same(h0, R.walk(h, A, dt=dt, seaLevel=sea), "h0")
        out = F.outlets(h, sea)
        for hk, flux, _ in hist[1:]:
            assert (hk >= h0).all(), (dt, G)  # every operation of the solve is monotone in b, and bk >= b0
            assert_same(hk[out], h[out], "outlets")
        # the flux of an outlet is the sum entering it: its own e is +0
        qin = F.drainage(hist[-1][1], F.receivers(h, sea)[0], np.zeros_like(h))
        assert_same(hist[-1][1][out], qin[out], "outlet flux")


def test_a_pit_gains_exactly_its_deposit_term():
    h, A = tile("noisy", 33)
    r = F.receivers(h)[0]
    pit = (r == F.NONE) & ~F.outlets(h)
    assert pit.any()
    s = S.series(h, A, dt=20.0, deposition=1.0, sedimentIterations=2)
    has, q, b0, f = R.coefficients(h, A, dt=20.0)
    qin = S.deposit(s["Q"], r, b0, A, F.outlets(h), 1.0)[0]
    fed = pit & (qin > 0)
    assert fed.any()
    assert_same(s["h"][pit], (b0[pit] + ((f32(1.0) * qin[pit]) / A[pit]).astype(f32)).astype(f32), "pits")
    assert (s["h"][fed] > b0[fed]).all()


def test_the_residual_does_not_grow_on_the_filled_tile():
    h, A = filled()
    assert F.pits(h) == 0
    for G in (0.5, 1.0):
        series = S.walk(h, A, dt=1.0, deposition=G, sedimentIterations=6)[3]
        assert all(b <= a for a, b in zip(series, series[1:])) and series[-1] < series[0] / 8, (G, series)


def test_the_default_iterations_are_the_measured_ones():
    # the smallest K with residual <= 1 % of max |b0 - h0| on the filled 97^2 tile at dt 100, G 0.5
    h = fill_ref.flood(np.ascontiguousarray(relief(97, 300), f32))
    A = D.accumulate(h)[0]
    b0 = R.coefficients(h, A, dt=100.0)[2]
    bar = f32(0.01) * np.abs(b0 - R.walk(h, A, dt=100.0)).max()
    series = S.walk(h, A, dt=100.0, deposition=S.DEFAULT_G, sedimentIterations=6)[3]
    assert min(k + 1 for k, v in enumerate(series) if v <= bar) == S.DEFAULT_K == 4 and S.DEFAULT_G == 0.5


def test_cells_without_area_take_no_deposit():
    h, A = tile("relief33", 33)
    A = A.copy()
    rng = np.random.default_rng(2)
    off = rng.random(h.shape) < 0.2
    A[off] = rng.choice(np.array([0.0, -0.0, -3.0], f32), int(off.sum()))
    s = S.series(h, A, dt=5.0, deposition=1.0, sedimentIterations=1)
    b0 = R.coefficients(h, A, dt=5.0)[2]
    assert_same(s["b"][off], b0[off], "bk where A <= 0")
    live = ~off & ~F.outlets(h)
    assert (s["b"][live] > b0[live]).any()


def test_a_nan_height_travels_as_in_the_implicit_model():
    h, A = tile("relief33", 33)
    h = h.copy()
    h[16, 16] = np.nan
    A = D.accumulate(h)[0]
    plain = R.walk(h, A, dt=20.0)
    got, flux, residual, _ = S.walk(h, A, dt=20.0, sedimentIterations=2)
    assert np.isnan(got[16, 16]) and np.array_equal(np.isnan(got), np.isnan(plain))
    assert np.isfinite(residual)  # a NaN cell does not enter the residual
    j = S.jacobi(h, A, dt=20.0, sedimentIterations=2)
    assert_same(j[0], got, "jacobi with a NaN"), assert_same(j[1], flux, "jacobi with a NaN: flux")
    assert (got[~np.isnan(got)] >= plain[~np.isnan(got)]).all()


def test_the_chain_is_the_stage():
    h, _ = filled()
    wh, wA, wQ, wr = S.chain(h, 2, dt=50.0)
    A1 = D.accumulate(h)[0]
    h1 = S.walk(h, A1, dt=50.0)[0]
    A2 = D.accumulate(h1)[0]
    h2, Q2, r2, _ = S.walk(h1, A2, dt=50.0)
    assert_same(wh, h2, "chain"), assert_same(wA, A2, "chain: drainage"), assert_same(wQ, Q2, "chain: flux")
    assert wr == r2
    assert not R.same(wh, R.chain(h, 2, dt=50.0)[0])
