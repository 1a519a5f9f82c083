"""The generators of tests/terrain_tiles.py earn their names: checked with the numpy models alone (fluvial_ref, fill_ref), at
the sizes tests/test_gpu_sweep_terrain.py runs them at, so that what the GPU tests assume about their inputs is a fact.

Two measures of "ties", both over the inner cells and both recomputed from the eight drops d = h[c] - h[k]:
    tie share         two or more of the eight slopes (d, or d * DIAG for a diagonal) equal the best slope the model holds at
                      the end, zero included: a `>=` for the `>` of the receiver rule changes exactly these cells (on a
                      plateau it invents a receiver)
    equal-drop share  some drop > 0 occurs at two or more neighbours
On the cones no two SLOPES ever tie off the axes -- with a cardinal and a diagonal neighbour equally lower the slopes are d and
d * DIAG -- so for them the bar of 20 % is on the equal-drop share, and the receiver codes are pinned quadrant by quadrant:
that is what a wrong DIAG, or a DIAG on a cardinal, turns over.  The figures (printed with -s):
    res 65 / 130   terraces4 0.86 / 0.86, terraces16 0.45 / 0.46, checker 1.00 / 1.00 tie share;
                   cheb_cone 0.97 / 0.98, manh_cone 0.97 / 1.00, cheb_pit 1.00 / 1.00, manh_pit 1.00 / 1.00 equal-drop share
    tiny           0.78 / 0.77 of the non-zero drops are subnormal at 66 / 97
    metres         66: 3 pits, 106 after a fill with epsilon 1e-4, 0 with 1e-2;  97: 10, 2074 and 0
    serpentine     97 cells, pitch 6: 96 passes with 16 sweeps, 505 with 3, 1506 with 1; one tile wakes up 7 times
    cuts           the splits of the stripe sweep (65 rows over 3 and 8 ranks, 130 over 3, and 2 / 8 ranks beside them): every
                   tie tile and `zeros` have at least 18 pairs of equal heights across every cut, straight or diagonal, and
                   `tiny` at least 129 pairs a subnormal amount apart"""
import numpy as np
import pytest

import fill_ref as L
import fluvial_ref as F
import terrain_tiles as T

f32 = np.float32
INNER = (slice(1, -1), slice(1, -1))
CARDINAL, DIAGONAL = {0, 1, 2, 3}, {4, 5, 6, 7}


def drops(h):
    """The eight drops of every cell, [k, z, x]; 0 where the neighbour does not exist."""
    d = np.zeros((8,) + h.shape, f32)
    for k, (dx, dz) in enumerate(F.NEIGHBOURS):
        c, n = F._window(h.shape, dx, dz)
        d[k][c] = h[c] - h[n]
    return d


def tie_share(h):
    d = drops(h)
    s = np.concatenate([d[:4], d[4:] * F.DIAG])
    best = F.receivers(h)[1]
    return float(((s == best[None]).sum(axis=0) >= 2)[INNER].mean())


def equal_drop_share(h):
    d = np.sort(drops(h), axis=0)
    return float(((d[1:] == d[:-1]) & (d[1:] > 0)).any(axis=0)[INNER].mean())


def make(name, res):
    return T.GENERATORS[name](res, np.random.default_rng(3))


@pytest.mark.parametrize("res", [65, 130])
@pytest.mark.parametrize("name", list(T.TIES))
def test_the_tie_tiles_tie(name, res):
    h = make(name, res)
    assert h.dtype == f32 and h.shape == (res, res) and h.flags.c_contiguous
    ties, equal = tie_share(h), equal_drop_share(h)
    print("%s %d: tie share %.3f, equal-drop share %.3f" % (name, res, ties, equal))
    if "cone" in name or "pit" in name:
        assert equal >= 0.2, (name, res, equal)
    else:
        assert ties >= 0.2, (name, res, ties)
    # exact arithmetic: every height is a multiple of 1/16 below 2^7, so every difference is exact
    assert np.array_equal(h * f32(16.0), np.round(h * f32(16.0))) and np.abs(h).max() < 128


@pytest.mark.parametrize("res", [65, 130])
def test_the_cones_choose_cardinals_and_diagonals(res):
    z, x = np.mgrid[0:res, 0:res]
    c = (res - 1) / 2
    east, north = x - c, z - c
    inner = np.zeros((res, res), bool)
    inner[INNER] = True
    # cheb_cone: off the diagonals the one cardinal towards the middle; W E S N are 0 1 2 3
    r = F.receivers(T.cheb_cone(res))[0]
    for code, where in ((0, east > np.abs(north)), (1, -east > np.abs(north)), (2, north > np.abs(east)),
                        (3, -north > np.abs(east))):
        assert where[inner].any() and (r[where & inner] == code).all(), ("cheb_cone", code)
    assert set(np.unique(r[inner & (np.abs(east) != np.abs(north))])) <= CARDINAL
    # cheb_pit: the cardinal away from the middle
    r = F.receivers(T.cheb_pit(res))[0]
    for code, where in ((1, east > np.abs(north)), (0, -east > np.abs(north)), (3, north > np.abs(east)),
                        (2, -north > np.abs(east))):
        assert (r[where & inner] == code).all(), ("cheb_pit", code)
    # manh_cone: inside a quadrant the diagonal towards the middle; SW SE NW NE are 4 5 6 7.  At an even size no cell lies on
    # an axis, but the rows and columns either side of it do not count: their diagonal crosses the axis and drops by d only
    off = (np.abs(east) >= 1) & (np.abs(north) >= 1)
    r = F.receivers(T.manh_cone(res))[0]
    for code, where in ((4, (east > 0) & (north > 0)), (5, (east < 0) & (north > 0)), (6, (east > 0) & (north < 0)),
                        (7, (east < 0) & (north < 0))):
        assert (where & off & inner).any() and (r[where & off & inner] == code).all(), ("manh_cone", code)
    # manh_pit: the diagonal away from the middle, and on the axes (odd sizes) two diagonals tie: the earlier one wins
    r = F.receivers(T.manh_pit(res))[0]
    for code, where in ((7, (east > 0) & (north > 0)), (6, (east < 0) & (north > 0)), (5, (east > 0) & (north < 0)),
                        (4, (east < 0) & (north < 0))):
        assert (r[where & inner] == code).all(), ("manh_pit", code)
    assert set(np.unique(r[inner & (east != 0) & (north != 0)])) <= DIAGONAL
    if res & 1:
        for code, where in ((5, (north == 0) & (east > 0)), (4, (north == 0) & (east < 0)), (6, (east == 0) & (north > 0)),
                            (4, (east == 0) & (north < 0))):
            assert (r[where & inner] == code).all(), ("manh_pit axis", code)


@pytest.mark.parametrize("res", [66, 97])
def test_tiny_drops_are_subnormal_and_still_erode(res):
    h = make("tiny", res)
    d = np.abs(drops(h))
    d = d[d != 0]
    share = float((d < f32(2.0 ** -126)).mean())
    print("tiny %d: %.3f of the non-zero drops are subnormal" % (res, share))
    assert share >= 0.5
    got, _ = F.run(h, 3)
    assert np.isfinite(got).all() and not np.array_equal(got.view(np.uint32), h.view(np.uint32))


@pytest.mark.parametrize("res", [66, 97])
def test_zeros_have_both_signs_and_specks(res):
    h = make("zeros", res)
    zero = h == 0
    assert (np.signbit(h) & zero).any() and (~np.signbit(h) & zero).any()
    specks = h[~zero]
    assert 0 < specks.size < 0.03 * h.size and (np.abs(specks) == f32(1e-45)).all() and (specks > 0).any() and (specks < 0).any()


@pytest.mark.parametrize("res", [66, 97])
def test_metres_round_the_default_epsilon_away(res):
    """include/noize_hip.h: the epsilon can be "absorbed by rounding at the tile's magnitudes".  From 2048 up half an ulp is
    more than 1e-4, so a filled lake stays a flat without receivers; 1e-2 is ten ulps at 13000."""
    h = make("metres", res)
    assert h.min() >= 2048 and h.max() < 16384
    before, absorbed, kept = F.pits(h), F.pits(L.flood(h, 1e-4)), F.pits(L.flood(h, 1e-2))
    print("metres %d: %d pits, %d after a fill with 1e-4, %d with 1e-2" % (res, before, absorbed, kept))
    assert absorbed > before > 0 and kept == 0


def wake_ups(record):
    """Per tile: how often it changed again after two or more passes of rest."""
    rec = np.stack(record).reshape(len(record), -1)
    counts = []
    for col in rec.T:
        n, rest, seen = 0, 0, False
        for v in col:
            if v:
                n += seen and rest >= 2
                seen, rest = True, 0
            else:
                rest += 1
        counts.append(n)
    return counts


def test_the_serpentine_winds_through_its_tiles():
    h, eps = T.serpentine_tile(), T.SERPENTINE["eps"]
    want = L.flood(h, eps)
    record = []
    W, passes = L.tiled(h, eps, tile=(64, 16), sweeps=16, record=record)
    assert L.same(W, want)
    assert len(record) == passes + 1 and not record[-1].any() and all(r.any() for r in record[:-1])
    woken = max(wake_ups(record))
    print("serpentine: %d passes, the busiest tile wakes up %d times" % (passes, woken))
    assert woken >= 3
    assert passes == T.SERPENTINE_PASSES[16] <= 150
    for sweeps in (3, 1):
        W, passes = L.tiled(h, eps, tile=(64, 16), sweeps=sweeps)
        assert L.same(W, want) and passes == T.SERPENTINE_PASSES[sweeps], (sweeps, passes)
    # the walls stand; the floor is a lake that rises by epsilon a cell along the one way out, dry only next to the mouth
    floor = h < 1
    floor[0, 1] = False
    assert (W[~floor] == h[~floor]).all() and (W[floor] > h[floor]).mean() > 0.95 and W[floor].max() < 1


def test_the_record_leaves_the_tiled_model_alone():
    h = make("noisy", 40)
    record = []
    a, b = L.tiled(h, 1e-4, tile=(16, 8), sweeps=4), L.tiled(h, 1e-4, tile=(16, 8), sweeps=4, record=record)
    assert L.same(a[0], b[0]) and a[1] == b[1] == len(record) - 1 and record[0].shape == (5, 3)


# the stripe sweep (tests/sweep_stripe_cases.py) takes its tiles to tie across every cut of its splits
def test_cut_rows_are_the_stripe_plans():
    from noize_job_amd import sharded as sh
    for rows, world in ((65, 3), (65, 8), (130, 3), (67, 3), (70, 16), (8, 8)):
        assert T.cut_rows(rows, world) == [sh.StripePlan(r, world, rows, 4, 0).g0 for r in range(1, world)]
    h = np.arange(36, dtype=f32).reshape(6, 6)
    assert T.cut_ties(h, 2) == [0] and T.cut_subnormal(h, 3) == [0, 0]
    h[3, 2] = h[2, 3]   # a diagonal pair across the cut at row 3
    h[3, 5] = h[2, 5]   # and a straight one
    assert T.cut_ties(h, 2) == [2] and T.cut_ties(h, 3) == [0, 0]
    h[3, 0], h[4, 0] = f32(2e-38), f32(2e-38) + f32(1e-40)  # normal numbers a subnormal amount apart, across the cut at row 4
    assert T.cut_subnormal(h, 3) == [0, 1] and T.cut_subnormal(h, 2) == [0]


@pytest.mark.parametrize("res,world", [(65, 3), (65, 8), (130, 3), (65, 2), (130, 2), (130, 8)])
@pytest.mark.parametrize("name", list(T.TIES) + ["zeros", "tiny"])
def test_the_stripe_tiles_tie_across_every_cut(name, res, world):
    """(65, 3), (65, 8) and (130, 3) are the splits of the stripe sweep; every tile of it has equal heights across every cut,
    straight or diagonal -- `tiny` instead heights that differ by a subnormal amount."""
    h = make(name, res)
    assert len(T.cut_rows(res, world)) == world - 1
    if name == "tiny":
        counts = T.cut_subnormal(h, world)
        print("tiny %d over %d: subnormal differences across the cuts %s" % (res, world, counts))
        assert max(counts) >= 1
    else:
        counts = T.cut_ties(h, world)
        print("%s %d over %d: equal pairs across the cuts %s" % (name, res, world, counts))
        assert min(counts) >= 1


def test_the_pitched_stripe_tile_ties_across_its_cuts():
    assert min(T.cut_ties(make("terraces16", 67), 3)) >= 1
