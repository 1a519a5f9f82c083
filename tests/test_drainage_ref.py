"""The drainage-area model (tests/drainage_ref.py) without a GPU: a tile worked by hand, the schedules that must agree, the
fluvial model at rest, the fixed point, the integer sums, tie-rich tiles and the long chain.  Bit for bit throughout."""
import numpy as np
import pytest

import drainage_ref as D
import fluvial_ref as F
import terrain_tiles as T
from test_hydraulic_ref import relief

f32 = np.float32
OFF = float(F.SEA_OFF)


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def rain_map(shape, seed=3):
    return (np.random.default_rng(seed).random(shape, dtype=f32) * f32(1.5) + f32(0.25)).astype(f32)


HAND = np.array([[9, 9, 9, 9, 9],
                 [9, 5, 4, 3, 0],
                 [9, 6, 7, 2, 9],
                 [9, 8, 7, 6, 9],
                 [9, 9, 9, 9, 9]], f32)


def test_a_tile_worked_by_hand():
    # rows are z, columns x; S is the row above on the page (z - 1), N the row below.  The receivers of the inner cells:
    #   (x1,z1)=5 -> E;  (2,1)=4 -> NE (drop 2 * 0.7071 beats E's 1);  (3,1)=3 -> E, the low border cell
    #   (1,2)=6 -> SE (2 * 0.7071 beats S's 1);  (2,2)=7 -> E (5);  (3,2)=2 -> SE, the low border cell
    #   (1,3)=8 -> S (2);  (2,3)=7 -> SE (5 * 0.7071);  (3,3)=6 -> S (4)
    r, _, _ = F.receivers(HAND)
    N = F.NONE
    assert r.tolist() == [[N, N, N, N, N], [N, 1, 7, 1, N], [N, 5, 1, 5, N], [N, 2, 5, 2, N], [N, N, N, N, N]]
    # so (1,3) -> (1,2) -> (2,1) -> (3,2) -> (4,1), and (1,1) -> (2,1); (2,2), (2,3), (3,3) -> (3,2); (3,1) -> (4,1)
    A, height = D.accumulate(HAND)
    assert A.tolist() == [[1, 1, 1, 1, 1], [1, 1, 4, 1, 10], [1, 2, 1, 8, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1]]
    assert height == 5
    # the order of the gather shows with a rain that is no power of two: k ascending is W, N, SW, NW at (3,2)
    q = f32(0.1)
    A, _ = D.accumulate(HAND, rain=0.1)
    a12 = f32(q + q)                    # (1,2): N = (1,3)
    a21 = f32(f32(q + q) + a12)         # (2,1): W = (1,1), then NW = (1,2)
    a32 = f32(f32(f32(f32(q + q) + q) + a21) + q)  # (3,2): W = (2,2), N = (3,3), SW = (2,1), NW = (2,3)
    a41 = f32(f32(q + q) + a32)         # (4,1): W = (3,1), NW = (3,2)
    assert (A[2, 1], A[1, 2], A[2, 3], A[1, 4]) == (a12, a21, a32, a41)
    assert_bits(A[0], np.full(5, q), "the top border")


CASES = [("relief70", OFF, False), ("relief70", 0.45, True), ("terraces", OFF, True), ("rand", 0.5, False)]


def make(name):
    rng = np.random.default_rng(11)
    if name == "relief70":
        return relief(80)[:70, :80].copy()  # 70 rows x 80 columns: partial tiles both ways, no square
    if name == "terraces":
        return T.terraces(72, rng, K=16)
    return rng.random((40, 70), dtype=f32)


@pytest.mark.parametrize("name,sea,mapped", CASES)
def test_three_schedules_one_result(name, sea, mapped):
    h = make(name)
    rm = rain_map(h.shape) if mapped else None
    want, height = D.accumulate(h, 0.75, sea, rm)
    A, steps = D.jacobi(h, 0.75, sea, rm)
    assert_bits(A, want, name + ": Jacobi")
    assert steps <= height - 1  # a cell is final one step after its donors
    passes = []
    for cap in (1, 3, 16):
        A, p = D.tiled(h, 0.75, sea, rm, sweeps=cap)
        assert_bits(A, want, "%s: tiles, cap %d" % (name, cap))
        passes.append(p)
    assert passes[0] >= passes[1] >= passes[2] >= 1
    # the fixed point: one more step of the fluvial model's accumulation returns the plane
    r = F.receivers(h, sea)[0]
    assert_bits(F.drainage(want, r, F.rain_plane(h.shape, 0.75, rm)), want, name + ": fixed point")


@pytest.mark.parametrize("res,sea,mapped", [(48, OFF, False), (48, 0.45, True), (33, 0.45, False), (17, OFF, True)])
def test_equals_the_fluvial_model_at_rest(res, sea, mapped):
    h = relief(res) if res != 33 else np.random.default_rng(res).random((res, res), dtype=f32)
    rm = rain_map(h.shape, res) if mapped else None
    want, height = D.accumulate(h, 1.25, sea, rm)
    hh, A = F.run(h, height + 1, erodibility=0.0, uplift=0.0, rain=1.25, seaLevel=sea, rainMap=rm)
    assert_bits(hh, h, "heights at rest")
    assert_bits(A, want, "drainage at rest")
    # ... and it is a drainageIn the model keeps
    _, again = F.run(h, 2, erodibility=0.0, uplift=0.0, rain=1.25, seaLevel=sea, rainMap=rm, drainageIn=want)
    assert_bits(again, want, "warm start")


@pytest.mark.parametrize("kind", sorted(T.TIES) + ["relief", "zeros"])
def test_rain_one_counts_cells(kind):
    res = 45
    h = np.ascontiguousarray(T.GENERATORS[kind](res, np.random.default_rng(5)), f32)
    A, height = D.accumulate(h)
    r = F.receivers(h)[0]
    assert (A == np.floor(A)).all() and A.min() == 1
    assert float(A[r == F.NONE].astype(np.float64).sum()) == res * res
    assert_bits(F.drainage(A, r, F.rain_plane(h.shape, 1.0)), A, kind + ": fixed point")
    assert_bits(D.tiled(h, tile=(16, 8), sweeps=2)[0], A, kind + ": small tiles")
    assert 1 <= height <= res * res


def test_the_serpentine_is_a_long_chain():
    h = D.serpentine()
    assert h.shape == (160, 160) and h.max() == f32(1e4)
    A, height = D.accumulate(h)
    assert height >= 4000, height  # the fixture must go on exercising long chains
    r = F.receivers(h)[0]
    assert_bits(F.drainage(A, r, F.rain_plane(h.shape, 1.0)), A, "serpentine: fixed point")
    assert (A == np.floor(A)).all()
    assert float(A[r == F.NONE].astype(np.float64).sum()) == 160 * 160
    out = np.argwhere((h == 0) & F.outlets(h))
    assert len(out) == 1 and A[tuple(out[0])] >= height  # the one outlet collects the whole channel
