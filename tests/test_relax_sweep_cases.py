"""The cases and models of tests/relax_sweep_cases.py, on the CPU: what tests/test_gpu_sweep_relax.py takes for granted.

    the stream      relax_sweep_cases(seed), seeds 0 to 7, is pinned -- describe(c), the tile's name, the bytes of the heights
                    and of the maps -- and reaches every one of its five families, every form, the faint tile, exponent 16 and a
                    signed rain map; mfd_sweep_cases(seed), the multiple-flow implicit step's own stream, is pinned the same way
                    and reaches both forms, a faint tile and an exponent-16 case that erode, both maps and a rain map, on
                    drainage planes that are positive everywhere
    the models      walk, jacobi and tiled (the kernels' schedule, at sweep caps 1, 3 and 16) agree bit for bit on every tile of
                    TILES at 65^2, and every plane is finite -- the multiple-flow implicit step with a sea on a cell value, both
                    maps, exponent 16 and a positive rain map
    the tiles       `faint` is subnormal in a quarter to a half of its cells; the hillslope model keeps the -0 of the held border
                    of `zeros`, leaves none inside and leaves subnormal cells, as it does on `faint`; so does the implicit fluvial
                    model on `faint`; exponent 16 gives subnormal and vanished weights where exponent 3 gives none; on every tie
                    tile receivers are chosen among equal drops, on all but the cones among equal slopes, and there the first in
                    the order W E S N SW SE NW NE wins; erodibility 0 with uplift 0 returns the heights, from both implicit
                    models, bit for bit on every tile but `zeros`; at exponent 16 the multiple-flow implicit model has cells
                    with a lower neighbour and no open edge -- outlets, all of them: the steepest neighbour's quotient is 1.0
                    and its gate never shuts -- and cells inside with single gates shut, and both come back as the text says
    the invariants  of the GPU test's chain: the cells that carry a basin label are the unit-rain drainage area of that outlet

The figures (printed with -s), seed 3, at 66^2 / 97^2 (65^2 for the ties and basins):
    faint           0.478 / 0.249 of the cells subnormal
    hillslope       zeros: 131 / 202 cells of -0, all on the border; 42 / 100 subnormal cells at r 0.01, 4 at the other r;
                    faint: 1941 to 2743 / 1159 to 2300 subnormal cells over the four r
    implicit        faint, uplift 0: 1948 / 2334 subnormal cells at dt 1, 3269 / 5825 at dt 200
    exponent 16     uniform 31 / 96 subnormal and 21 / 49 vanished weights, metres 47 / 77 and 18 / 53; none on terraces16, none
                    at exponent 3
    exponent 16,    uniform 219 / 324 cells with a drop > 0 and no open edge, metres 249 / 375, every one an outlet of the
    implicit        border, none inside; uniform 21 / 49 cells inside with a gate shut on a drop > 0, metres 18 / 53
    tied receivers  among equal slopes, sea off: terraces4 220, terraces16 604, cheb_pit 125, manh_pit 125, checker 1984, the
                    cones 0 (among equal drops 3840 and 3844)
    basins          terraces4 3436, checker 2241: nearly every cell a flat without a receiver"""
import hashlib

import numpy as np
import pytest

import drainage_mfd_ref as M
import drainage_ref as D
import fluvial_implicit_mfd_ref as R2
import fluvial_implicit_ref as R
import fluvial_ref as F
import hillslope_ref as HS
import relax_sweep_cases as C
import stream_order_ref as S
import terrain_tiles as T
import watershed_ref as W

f32 = np.float32
OFF = C.OFF
SWEEP_DIGESTS = {0: "c30593638ecd412f", 1: "27158f9a7d8292bc", 2: "b073a7dcb36d7682", 3: "331d255d50068171",
                 4: "28a3929e70d833be", 5: "b4ffdb1bb452dfc0", 6: "d311f4fa5942a708", 7: "43eea763de7ff492"}


MFD_SWEEP_DIGESTS = {0: "23e49ed551127135", 1: "c9d459cfd1ab3975", 2: "e7741748861c55de", 3: "55bd92938868d3ca",
                     4: "cb674fb710fd852e", 5: "3929ccfafecdf62a", 6: "61ee8738a17a4ce9", 7: "c182a9731f2dbcc8"}


def make(name, res):
    return C.tile(name, res)


# ---- the stream ----------------------------------------------------------------------------------------------------------------
def digest(cases):
    m = hashlib.sha256()
    for c in cases:
        m.update(C.describe(c).encode())
        m.update(c["name"].encode())
        m.update(np.ascontiguousarray(c["hh"]).tobytes())
        for name in ("drainage", "hardness", "upliftMap", "rainMap"):
            if c[name] is not None:
                m.update(np.ascontiguousarray(c[name]).tobytes())
    return m.hexdigest()[:16]


@pytest.mark.parametrize("seed", range(8))
def test_the_seeded_sweep_is_pinned(seed):
    cases = C.relax_sweep_cases(seed)
    print("%d: %r" % (seed, digest(cases)))
    assert len(cases) == 5 and all(c["hh"].shape[-1] in C.SWEEP_SIZES for c in cases)
    assert digest(cases) == SWEEP_DIGESTS[seed], [C.describe(c) for c in cases]


@pytest.mark.parametrize("seed", range(8))
def test_the_seeded_multiple_flow_sweep_is_pinned(seed):
    cases = C.mfd_sweep_cases(seed)
    print("%d: %r" % (seed, digest(cases)))
    assert len(cases) == 3 and all(c["hh"].shape[-1] in C.SWEEP_SIZES for c in cases)
    assert digest(cases) == MFD_SWEEP_DIGESTS[seed], [C.describe(c) for c in cases]


def test_the_seeded_multiple_flow_sweep_reaches_every_form_and_edge():
    cases = [c for seed in range(8) for c in C.mfd_sweep_cases(seed)]
    assert len(cases) == 24 and len({C.describe(c) + c["name"] for c in cases}) == 24
    assert {c["family"] for c in cases} == {"fluvial_implicit_mfd"}
    assert {c["form"] for c in cases} == {"tile", "batch"}
    assert any(c["name"] == "faint" for c in cases) and any(c["exponent"] == 16 for c in cases)
    assert any(c["name"] == "faint" and c["erodibility"] > 0 for c in cases)
    assert any(c["exponent"] == 16 and c["erodibility"] > 0 and c["name"] not in ("zeros", "checker") for c in cases)
    assert max(c["hh"].shape[-1] for c in cases) <= 131
    assert any(c["rainmap"] == "positive" and c["rainMap"] is not None for c in cases) and any(c["maps"] for c in cases)
    assert {c["rainmap"] for c in cases} == {None, "positive"}
    for c in cases:
        assert (c["drainage"] > 0).all(), C.describe(c)  # sqrt(A) stays among the finite numbers
        planes, bound = C.model(c)
        assert all(np.isfinite(p).all() for p in planes) and bound >= 2, C.describe(c)


def test_the_seeded_sweep_reaches_every_family_form_and_edge():
    cases = [c for seed in range(8) for c in C.relax_sweep_cases(seed)]
    assert len(cases) == 40 and len({C.describe(c) + c["name"] for c in cases}) == 40
    assert {c["family"] for c in cases} == set(C.SWEEP_FAMILIES) == set(C.FAMILIES) - {"fluvial_implicit_mfd"}
    assert {c["form"] for c in cases} == {"tile", "batch", "inplace"}
    for fam in C.SWEEP_FAMILIES:
        assert {c["form"] for c in cases if c["family"] == fam} >= {"tile", "batch"}, fam
    assert any(c["name"] == "faint" for c in cases)
    mfd = [c for c in cases if c["family"] == "drainage_mfd"]
    assert any(c["exponent"] == 16 for c in mfd) and any(c["rainmap"] == "signed" and (c["rainMap"] < 0).any() for c in mfd)
    for c in cases:
        planes, bound = C.model(c)
        assert all(np.isfinite(p).all() for p in planes), C.describe(c)
        assert (bound is None) == (c["family"] == "hillslope")


# ---- the models agree with themselves ------------------------------------------------------------------------------------------
def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("name", sorted(C.TILES))
def test_walk_jacobi_and_tiled_agree(name, family):
    res = 65
    h = make(name, res)
    sea = T.sea_at(h, 0.3)
    if family == "watershed":
        walk = W.walk(h, sea, 0.3)[:2]
        others = [W.jacobi(h, sea, 0.3)[:2]] + [W.tiled(h, sea, 0.3, sweeps=s)[:2] for s in (1, 3, 16)]
    elif family == "stream_order":
        A = D.accumulate(h, 1.0, sea)[0]
        walk = S.walk(h, sea, A, 2.0)[:2]
        others = [S.jacobi(h, sea, A, 2.0)[:2]] + [S.tiled(h, sea, A, 2.0, sweeps=s)[:2] for s in (1, 3, 16)]
    elif family == "fluvial_implicit":
        A = D.accumulate(h, 1.0, sea)[0]
        hard, upl = C.implicit_maps(h.shape, 11)
        kw = dict(dt=200.0, seaLevel=sea, hardness=hard, upliftMap=upl)
        walk = (R.walk(h, A, **kw),)
        others = [R.jacobi(h, A, **kw)[:1]] + [R.tiled(h, A, sweeps=s, **kw)[:1] for s in (1, 3, 16)]
    elif family == "drainage_mfd":
        rm = C.drainage_rain_map(h.shape, 11, signed=True)
        walk = M.walk(h, 0.3, sea, rm, 16)[:1]
        others = [M.jacobi(h, 0.3, sea, rm, 16)[:1]] + [M.tiled(h, 0.3, sea, rm, 16, sweeps=s)[:1] for s in (1, 3, 16)]
    elif family == "fluvial_implicit_mfd":
        A = M.walk(h, 0.75, sea, C.drainage_rain_map(h.shape, 11), 16)[0]
        assert (A > 0).all()
        hard, upl = C.implicit_maps(h.shape, 11)
        kw = dict(dt=200.0, seaLevel=sea, exponent=16, hardness=hard, upliftMap=upl)
        walk = R2.walk(h, A, **kw)[:1]
        others = [R2.jacobi(h, A, **kw)[:1]] + [R2.tiled(h, A, sweeps=s, **kw)[:1] for s in (1, 3, 16)]
    else:  # no relaxation: three iterations are one iteration three times, the border is held
        walk = (HS.diffuse(h, 100.0, 1.0, 3),)
        once = h
        for _ in range(3):
            once = HS.diffuse(once, 100.0, 1.0, 1)
        others = [(once,)]
        edge = np.ones(h.shape, bool)
        edge[1:-1, 1:-1] = False
        assert same(walk[0][edge], h[edge])
    assert all(np.isfinite(p).all() for p in walk), (name, family)
    for k, other in enumerate(others):
        for p, q in zip(walk, other):
            assert same(p, q), (name, family, k)


# ---- the tiles do what the GPU test takes them for -----------------------------------------------------------------------------
# what the GPU test needs is subnormal cells by the hundred next to normal ones, not a share to the percent: a fifth of the
# tile itself, a tenth of a result (a large r smooths a result towards the tile's mean, which is a normal number)
FIFTH, TENTH = 0.2, 0.1


@pytest.mark.parametrize("res", [66, 97])
def test_faint_is_subnormal(res):
    h = make("faint", res)
    share = float(C.subnormal(h).mean())
    print("faint %d: %.3f of the cells subnormal" % (res, share))
    assert h.dtype == f32 and h.flags.c_contiguous and (h != 0).all() and FIFTH < share < 1 - FIFTH
    assert res != 66 or share > 0.25


@pytest.mark.parametrize("res", [66, 97])
def test_hillslope_keeps_negative_zeros_on_the_border_only_and_leaves_subnormals(res):
    z, faint = make("zeros", res), make("faint", res)
    inner = np.zeros(z.shape, bool)
    inner[1:-1, 1:-1] = True
    minus = lambda a: (a == 0) & np.signbit(a)  # noqa: E731
    assert (minus(z) & inner).sum() > 0.25 * z.size and (minus(z) & ~inner).sum() > res
    counts = []
    for r in C.RS:
        out = HS.diffuse(z, r)
        # the held border keeps its -0; inside p_i = (v_i + r * p_{i-1}) * inv_i adds a +0 sooner or later: no -0 survives
        assert np.array_equal(minus(out) & ~inner, minus(z) & ~inner) and not (minus(out) & inner).any(), r
        counts.append((int(minus(out).sum()), int(C.subnormal(out).sum())))
    print("hillslope on zeros %d: (-0 cells, subnormal cells) per r %s" % (res, counts))
    assert max(s for _, s in counts) > 0
    counts = [int((C.subnormal(HS.diffuse(faint, r)) & inner).sum()) for r in C.RS]
    print("hillslope on faint %d: subnormal cells inside the border per r %s" % (res, counts))
    assert min(counts) > TENTH * res * res


@pytest.mark.parametrize("res", [66, 97])
def test_the_implicit_step_leaves_subnormals_on_faint(res):
    h = make("faint", res)
    A = D.accumulate(h)[0]
    counts = []
    for dt in (1.0, 200.0):
        out = R.walk(h, A, uplift=0.0, dt=dt)
        moved = out.view(np.uint32) != h.view(np.uint32)
        counts.append(int((C.subnormal(out) & moved).sum()))
    print("implicit fluvial on faint %d, uplift 0: subnormal cells that moved %s" % (res, counts))
    assert min(counts) > FIFTH * res * res


def weight_counts(h, exponent):
    """(subnormal weights, edges that take flow and whose weight vanished)."""
    Wt = M.weights(h, OFF, exponent)
    s = np.zeros_like(Wt)
    for k, (dx, dz) in enumerate(F.NEIGHBOURS):
        c, n = F._window(h.shape, dx, dz)
        s[k][c] = h[c] - h[n]
    live = (s > 0) & ~F.outlets(h, OFF)[None]
    return int(C.subnormal(Wt).sum()), int((live & (Wt == 0)).sum())


@pytest.mark.parametrize("res", [66, 97])
def test_exponent_16_underflows_where_exponent_3_does_not(res):
    for name in ("uniform", "metres", "terraces16"):
        h = make(name, res)
        three, sixteen = weight_counts(h, 3), weight_counts(h, 16)
        print("%s %d: (subnormal, vanished) weights at exponent 3 %s, at 16 %s" % (name, res, three, sixteen))
        assert three == (0, 0), name
        if name == "terraces16":
            assert sixteen == (0, 0)
        else:
            assert sixteen[0] > 0 and sixteen[1] > three[1], name


def tied(h, sea=OFF):
    """(the cells with a receiver whose best slope two or more neighbours share; the first such neighbour of every cell; the
    receivers; the cells with a receiver that have one drop > 0 at two or more neighbours)."""
    r, best, _ = F.receivers(h, sea)
    s = np.full((8,) + h.shape, -np.inf, f32)
    d = np.zeros((8,) + h.shape, f32)
    for k, (dx, dz) in enumerate(F.NEIGHBOURS):
        c, n = F._window(h.shape, dx, dz)
        d[k][c] = h[c] - h[n]
        s[k][c] = d[k][c] if k < 4 else d[k][c] * F.DIAG
    share = s == best[None]
    d = np.sort(d, axis=0)
    equal = ((d[1:] == d[:-1]) & (d[1:] > 0)).any(axis=0)
    has = r != F.NONE
    return has & (share.sum(axis=0) >= 2), np.argmax(share, axis=0).astype(np.uint8), r, has & equal


# where two or more SLOPES tie for the best: plateau edges of the terraces, a checker peak's four cardinals, the two cardinals
# of a cheb_pit's diagonal cells, the two diagonals of a manh_pit's axis cells (odd sizes have axis cells).  On the cones the
# best slope is alone, but equal DROPS are everywhere: a cardinal and two diagonals (cheb), two cardinals under a diagonal (manh)
SLOPE_TIES = {"terraces4": (65, 130), "terraces16": (65, 130), "checker": (65, 130), "cheb_pit": (65, 130), "manh_pit": (65,),
              "cheb_cone": (), "manh_cone": ()}


@pytest.mark.parametrize("res", [65, 130])
@pytest.mark.parametrize("name", list(T.TIES))
def test_the_receiver_of_a_tie_is_the_first_of_the_equal_slopes(name, res):
    """include/noize_hip.h: the neighbours are tried in the order W E S N SW SE NW NE and a later one has to be strictly
    steeper, so among equal slopes the first wins."""
    h = make(name, res)
    for sea in (OFF, T.sea_at(h, 0.3)):
        ties, first, r, equal = tied(h, sea)
        print("%s %d sea %g: %d receivers chosen among equal slopes, %d among equal drops" % (
            name, res, sea, int(ties.sum()), int(equal.sum())))
        assert equal.sum() >= res, (name, res, sea)
        assert (r[ties] == first[ties]).all()
        if res in SLOPE_TIES[name]:
            assert ties.sum() >= res, (name, res, sea)
            later = np.zeros(h.shape, bool)  # ... and the first is not the last: `>=` for `>` would name another neighbour
            for k, (dx, dz) in enumerate(F.NEIGHBOURS):
                c, n = F._window(h.shape, dx, dz)
                later[c] |= (h[c] - h[n]) * (f32(1.0) if k < 4 else F.DIAG) == F.receivers(h, sea)[1][c]
            assert (ties & later).any()


@pytest.mark.parametrize("name", sorted(C.TILES))
def test_without_erosion_and_uplift_the_implicit_step_returns_the_heights(name):
    h = make(name, 65)
    (out,), _ = C.model(C.identity_case(h))
    if name == "zeros":  # (-0 + +0) / 1 is +0: a -0 with a receiver changes its sign
        changed = out[0].view(np.uint32) != h.view(np.uint32)
        assert np.array_equal(out[0], h) and changed.any() and (np.signbit(h[changed]) & (h[changed] == 0)).all()
    else:
        assert same(out[0], h), name


@pytest.mark.parametrize("name", sorted(C.TILES))
def test_without_erosion_and_uplift_the_multiple_flow_step_returns_the_heights(name):
    h = make(name, 65)
    (out,), _ = C.model(C.identity_case(h, family="fluvial_implicit_mfd"))
    if name == "zeros":  # no cell of it has a lower neighbour: b = -0 + +0 is +0 on every cell that is no outlet
        changed = out[0].view(np.uint32) != h.view(np.uint32)
        assert np.array_equal(out[0], h) and changed.any() and (np.signbit(h[changed]) & (h[changed] == 0)).all()
        assert not F.outlets(h, OFF)[changed].any()
    else:
        assert same(out[0], h), name


def drops_and_gates(h, exponent):
    """(the cells with a drop > 0 to some neighbour, the drops > 0 per direction, the gates of the multiple-flow model)."""
    drop = np.zeros((8,) + h.shape, bool)
    for k, (dx, dz) in enumerate(F.NEIGHBOURS):
        c, n = F._window(h.shape, dx, dz)
        drop[k][c] = h[c] - h[n] > 0
    return drop.any(axis=0), drop, M.weights(h, OFF, exponent) > 0


@pytest.mark.parametrize("res", [66, 97])
@pytest.mark.parametrize("name", ["uniform", "metres"])
def test_at_exponent_16_a_cell_without_an_open_edge_comes_back_as_b(name, res):
    """Exponent 16, uplift 0, the sea off.  The cells with a drop > 0 to some neighbour and no open edge exist, and every one
    of them is an outlet of the border: the steepest neighbour's quotient s / best is 1.0 exactly and so are its powers, so a
    cell inside keeps that gate whatever underflows around it.  What underflow does shut is single gates (the vanished
    weights of the test above): cells inside with a lower neighbour the step does not look at.  Both come back as the model
    says: the first as b, the second from their open gates alone."""
    h = make(name, res)
    lower, drop, G = drops_and_gates(h, 16)
    opens = G.any(axis=0)
    shut = lower & ~opens
    inside = ~F.outlets(h, OFF)
    some_shut = inside & (drop & ~G).any(axis=0)
    print("%s %d exponent 16: %d cells with a drop > 0 and no open edge, %d of them inside; %d cells inside with a gate shut "
          "on a drop > 0" % (name, res, int(shut.sum()), int((shut & inside).sum()), int(some_shut.sum())))
    assert shut.sum() > 0 and not (shut & inside).any() and (opens[inside] == lower[inside]).all()
    assert some_shut.sum() > 0 and opens[some_shut].all()
    A = M.walk(h, exponent=16)[0]
    assert (A > 0).all()
    for dt in (1.0, 200.0):
        kw = dict(uplift=0.0, dt=dt, exponent=16)
        out = R2.walk(h, A, **kw)[0]
        _, b, Fk = R2.coefficients(h, A, **kw)
        assert np.isfinite(out).all() and same(out[~opens], b[~opens]) and same(b, h)  # uplift 0: b is the heights
        assert not Fk[~G].any() and same(R2.step(out, G, b, Fk), out)
        assert (out[some_shut] < h[some_shut]).all()  # they erode along the gates that stayed open


# ---- the invariants of the GPU test's chain ------------------------------------------------------------------------------------
def assert_labels_count_the_drainage(basin, r, A):
    """Per outlet or pit L (a cell without a receiver): its label is its own index, and the cells that carry L are the
    unit-rain drainage area at L; no other cell is a label."""
    own = np.arange(basin.size, dtype=np.int32).reshape(basin.shape)
    root = r == F.NONE
    assert (basin[root] == own[root]).all() and (basin[~root] != own[~root]).all()
    count = np.bincount(basin.reshape(-1), minlength=basin.size).reshape(basin.shape)
    assert (count[root] == A[root]).all() and not count[~root].any()


def assert_labels_follow_the_receivers(basin, r):
    has = r != F.NONE
    assert (basin[has] == basin.reshape(-1)[W.targets(r)][has]).all()


@pytest.mark.parametrize("name", list(T.TIES))
def test_basin_sizes_are_drainage_areas(name):
    h = make(name, 65)
    for sea in (OFF, T.sea_at(h, 0.3)):
        basin = W.walk(h, sea)[0]
        r = F.receivers(h, sea)[0]
        assert_labels_count_the_drainage(basin, r, D.accumulate(h, 1.0, sea)[0])
        assert_labels_follow_the_receivers(basin, r)
    print("%s: %d basins" % (name, len(np.unique(W.walk(h)[0]))))
