"""The multiple-flow drainage model (tests/drainage_mfd_ref.py) without a GPU: a tile worked by hand as rationals, the
schedules that must agree bit for bit, what follows from the model (one lower neighbour sends 1, weights sum to 1, rain is
conserved), float32 against float64, and the long chain."""
from fractions import Fraction

import numpy as np
import pytest

import drainage_mfd_ref as M
import drainage_ref as D
import fill_ref
import fluvial_ref as F
import terrain_tiles as T
from test_hydraulic_ref import relief

f32 = np.float32
OFF = float(F.SEA_OFF)
DIAGQ = Fraction(float(F.DIAG))  # the float32 constant as the rational it is


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def rain_map(shape, seed=3, signed=False):
    m = np.random.default_rng(seed).random(shape, dtype=f32) * f32(1.5) + f32(0.25)
    return (m - f32(1.0)).astype(f32) if signed else m.astype(f32)


HAND = np.array([[9, 9, 9, 9, 9],
                 [9, 6, 4, 9, 9],
                 [9, 4, 2, 9, 9],
                 [9, 9, 1, 9, 9],
                 [9, 9, 0, 9, 9]], f32)


def rational_model(h, exponent):
    """The model's text over the rationals (small integer heights, DIAG the float32 constant): outgoing weights and A."""
    rows, cols = h.shape
    hq = [[Fraction(int(v)) for v in row] for row in h]
    W = {}
    for z in range(1, rows - 1):
        for x in range(1, cols - 1):
            s = {}
            for k, (dx, dz) in enumerate(F.NEIGHBOURS):
                d = hq[z][x] - hq[z + dz][x + dx]
                if d > 0:
                    s[k] = d if k < 4 else d * DIAGQ
            if s:
                best = max(s.values())
                g = {k: (v / best) ** exponent for k, v in s.items()}
                total = sum(g.values())
                for k, v in g.items():
                    W[(x, z, k)] = v / total
    A = {}
    for _, x, z in sorted(((-hq[z][x], x, z) for z in range(rows) for x in range(cols))):
        a = Fraction(1)
        for k, (dx, dz) in enumerate(F.NEIGHBOURS):
            a += W.get((x + dx, z + dz, F.OPPOSITE[k]), 0) * A.get((x + dx, z + dz), 0)
        A[(x, z)] = a
    return W, A


@pytest.mark.parametrize("exponent", [1, 2, 4])
def test_a_tile_worked_by_hand(exponent):
    # rows are z, columns x; S is the row above on the page (z - 1), N the row below.  The inner cells and their lower
    # neighbours:  (1,1)=6 -> E (2), N (2), NE (4 DIAG);  (2,1)=4 -> N alone;  (1,2)=4 -> E (2), NE (3 DIAG, the steepest);
    # (2,2)=2 -> N alone;  (2,3)=1 -> N alone, the outlet (2,4);  (3,1)=9 -> W (5), NW (7 DIAG);  (3,2)=9 -> W (7), SW (5 DIAG),
    # NW (8 DIAG);  (3,3)=9 -> W (8), SW (7 DIAG), NW (9 DIAG);  (1,3)=9 -> E (8), S (5), SE (7 DIAG), NE (9 DIAG)
    Wq, Aq = rational_model(HAND, exponent)
    p, D_ = exponent, DIAGQ
    assert Wq[(1, 1, 1)] == Wq[(1, 1, 3)] == Fraction(2) ** p / (2 * Fraction(2) ** p + (4 * D_) ** p)
    assert Wq[(1, 2, 7)] == (3 * D_) ** p / (Fraction(2) ** p + (3 * D_) ** p)
    assert Wq[(2, 1, 3)] == Wq[(2, 2, 3)] == Wq[(2, 3, 3)] == 1
    assert sorted(k for (x, z, k) in Wq if (x, z) == (1, 3)) == [1, 2, 5, 7]
    assert Aq[(1, 1)] == 1  # its higher neighbours are border cells: outlets send nothing
    assert Aq[(2, 1)] == 1 + Wq[(1, 1, 1)] * 1 + Wq[(3, 1, 0)] * 1 + Wq[(3, 2, 4)] * 1  # W = (1,1), E = (3,1), NE = (3,2)
    assert sum(Aq[c] for c in Aq if not any((c[0], c[1], k) in Wq for k in range(8))) == 25  # rain is conserved
    W = M.weights(HAND, exponent=exponent)
    for (x, z, k), w in Wq.items():
        assert abs(Fraction(float(W[k][z, x])) - w) <= w * Fraction(6 * exponent + 6, 2 ** 24), (x, z, k)  # roundings: s, q, the powers, T, w
    assert np.count_nonzero(W) == len(Wq)
    assert W[3][1, 2] == W[3][2, 2] == W[3][3, 2] == 1  # one lower neighbour: exactly 1
    A, height = M.walk(HAND, exponent=exponent)
    for (x, z), a in Aq.items():
        assert abs(Fraction(float(A[z, x])) - a) <= a * Fraction(5 * (6 * exponent + 8), 2 ** 24), (x, z)  # a path of five cells
    # the path (1,1) -> (1,2) -> (2,2) -> (2,3) -> (2,4), and nothing longer ((3,1) -> (2,2) is as long)
    assert height == 5
    # the order of the gather, as float32: (2,1) takes W = (1,1), then E = (3,1), then NE = (3,2)
    one = f32(1)
    assert A[1, 2] == f32(f32(f32(one + f32(W[1][1, 1] * one)) + f32(W[0][1, 3] * one)) + f32(W[4][2, 3] * one))
    assert_bits(M.jacobi(HAND, exponent=exponent)[0], A, "Jacobi")


def tiles():
    out = [("relief97", np.ascontiguousarray(relief(97, 300), f32), (64, 16))]
    for name, gen in sorted(T.GENERATORS.items()):
        out.append((name, np.ascontiguousarray(gen(33, np.random.default_rng(5)), f32), (16, 8)))
    return out


TILES = tiles()
# The largest relative difference between the float32 plane and its float64 restatement on TILES, raw and filled, at
# exponents 1 and 4, measured: 0.0952, on `zeros` raw -- its slopes are the smallest subnormal, where d * DIAG has no bit to
# round into, so float32 sends a diagonal as much as a cardinal neighbour and float64 does not.  `tiny` raw, subnormal
# slopes with a few bits, measures 1.75e-6.  On every other tile the slopes are normal numbers and the largest difference
# is 1.04e-6 (terraces16 filled).  The test allows four times the measured value, overall and on the normal tiles.
MEASURED_F32_VS_F64 = 0.0952
MEASURED_F32_VS_F64_NORMAL = 1.04e-6
SUBNORMAL_SLOPES = ("zeros", "tiny")


@pytest.mark.parametrize("name,h,tile", TILES, ids=[t[0] for t in TILES])
@pytest.mark.parametrize("filled", [False, True], ids=["raw", "filled"])
def test_schedules_agree_and_the_model_holds(name, h, tile, filled, capsys):
    if filled:
        h = fill_ref.flood(h)
    rm = rain_map(h.shape, signed=True)
    worst = 0.0
    for exponent in (1, 4):
        want, height = M.walk(h, exponent=exponent)
        assert np.isfinite(want).all(), name  # the precondition of every comparison below
        A, steps = M.jacobi(h, exponent=exponent)
        assert_bits(A, want, "%s: Jacobi" % name)
        assert steps <= height - 1
        # what follows from the model
        W = M.weights(h, exponent=exponent)
        sends = (W > 0).sum(axis=0)
        lower = np.zeros(h.shape, int)
        for k, (dx, dz) in enumerate(F.NEIGHBOURS):
            c, n = F._window(h.shape, dx, dz)
            lower[c] += h[c] > h[n]
        inner = ~F.outlets(h)
        one = inner & (lower == 1)
        assert (W.max(axis=0)[one] == 1).all() and (sends[one] == 1).all(), name
        assert (sends[~inner] == 0).all() and (sends[inner] <= lower[inner]).all(), name
        total = W.astype(np.float64).sum(axis=0)
        assert (np.abs(total[sends > 0] - 1) <= 2.0 ** -20).all(), (name, np.abs(total[sends > 0] - 1).max())
        assert (want >= 1).all()  # rain >= 0 and no map: A >= rain
        # float64: rain is conserved over the cells that send nothing, and float32 stays close
        A64 = M.walk64(h, exponent=exponent)
        assert abs(A64[sends == 0].sum() - h.size) <= 1e-9 * h.size, name
        assert abs(float(want[sends == 0].astype(np.float64).sum()) - h.size) <= 1.6e-6 * h.size, name
        worst = max(worst, float(np.abs(want / A64 - 1).max()))
        # the kernel's schedule, with a signed rain map: values move both ways
        signed, _ = M.walk(h, 0.75, OFF, rm, exponent)
        assert np.isfinite(signed).all(), name
        passes = []
        for cap in (1, 3, 16):
            A, p = M.tiled(h, 0.75, OFF, rm, exponent, tile=tile, sweeps=cap)
            assert_bits(A, signed, "%s: tiles, cap %d" % (name, cap))
            passes.append(p)
        assert max(passes) <= height - 1  # a pass is at least one Jacobi step
    with capsys.disabled():
        print("\n%s %s: float32 against float64 %.3g" % (name, "filled" if filled else "raw", worst))
    assert worst <= 4 * (MEASURED_F32_VS_F64 if name in SUBNORMAL_SLOPES else MEASURED_F32_VS_F64_NORMAL), (name, worst)


def test_a_sea_and_nan_heights():
    h = np.ascontiguousarray(relief(48, 300), f32)
    sea = float(np.median(h))
    W = M.weights(h, sea, 2)
    assert not W[:, F.outlets(h, sea)].any()
    want, _ = M.walk(h, 0.5, sea, rain_map(h.shape), 2)
    assert_bits(M.jacobi(h, 0.5, sea, rain_map(h.shape), 2)[0], want, "sea: Jacobi")
    assert_bits(M.tiled(h, 0.5, sea, rain_map(h.shape), 2, tile=(16, 8), sweeps=3)[0], want, "sea: tiles")
    h = h.copy()
    h[20, 20] = np.nan
    h[30, 7] = np.inf  # an infinite difference: NaN weights, and the gate drops them
    A, _ = M.walk(h)
    assert np.isfinite(A).all() and A[20, 20] == 1 and A[30, 7] == 1
    I = M.incoming(M.weights(h))
    assert not (I[:, 20, 20] > 0).any() and not (M.weights(h)[:, 20, 20] > 0).any()
    assert_bits(M.jacobi(h)[0], A, "NaN: Jacobi")


def test_the_serpentine(capsys):
    h = D.serpentine()
    A, height = M.walk(h)
    tree = D.accumulate(h)[1]
    with capsys.disabled():
        print("\nserpentine 160^2: DAG height %d (the single-direction tree: %d)" % (height, tree))
    assert np.isfinite(A).all() and height >= tree >= 4000
    assert_bits(M.step(A, M.incoming(M.weights(h)), F.rain_plane(h.shape, 1.0)), A, "serpentine: fixed point")
