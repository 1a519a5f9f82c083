"""The watershed model (tests/watershed_ref.py) without a GPU: a tile worked by hand, the schedules that must agree, labels
that are outlets and pits, the tie to the drainage area, filled tiles, a sea, the scaling of the length and the long chain.
Bit for bit throughout."""
import numpy as np
import pytest

import drainage_ref as D
import fill_ref
import fluvial_ref as F
import watershed_ref as W
from test_hydraulic_ref import relief

f32 = np.float32
OFF = float(F.SEA_OFF)
_memo = {}


def tile(res):
    if res not in _memo:
        _memo[res] = (np.random.default_rng(res).random((res, res), dtype=f32) if res <= 5
                      else np.ascontiguousarray(relief(res), f32))
        _memo[res].setflags(write=False)
    return _memo[res]


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


HAND = np.array([[9, 9, 9, 9, 9],
                 [9, 5, 4, 3, 0],
                 [9, 6, 7, 2, 9],
                 [9, 8, 1, 8, 9],
                 [9, 9, 9, 9, 9]], f32)


def test_a_tile_worked_by_hand():
    # rows are z, columns x; S is the row above on the page (z - 1), N the row below.  The receivers of the inner cells:
    #   (x1,z1)=5 -> E;  (2,1)=4 -> NE (drop 2 * 0.7071 beats E's 1);  (3,1)=3 -> E, the low border cell (4,1) = cell 9
    #   (1,2)=6 -> NE (5 * 0.7071);  (2,2)=7 -> N (6);  (3,2)=2 -> SE, the low border cell
    #   (1,3)=8 -> E (7);  (2,3)=1: a pit, cell 17;  (3,3)=8 -> W (7)
    N = F.NONE
    assert F.receivers(HAND)[0].tolist() == [[N, N, N, N, N], [N, 1, 7, 1, N], [N, 7, 3, 5, N], [N, 1, N, 0, N],
                                             [N, N, N, N, N]]
    basin, length, hops = W.walk(HAND)
    # so (1,1) -> (2,1) -> (3,2) -> (4,1) and (3,1) -> (4,1): basin 9; everything else inside drains to the pit
    assert basin.dtype == np.int32 and basin.tolist() == [[0, 1, 2, 3, 4], [5, 9, 9, 9, 9], [10, 17, 17, 9, 14],
                                                          [15, 17, 17, 17, 19], [20, 21, 22, 23, 24]]
    assert hops.tolist() == [[0, 0, 0, 0, 0], [0, 3, 2, 1, 0], [0, 1, 1, 1, 0], [0, 1, 0, 1, 0], [0, 0, 0, 0, 0]]
    d, one, o = W.SQRT2, f32(1.0), f32(0.0)
    assert d == f32(1.41421354)
    want = np.array([[o, o, o, o, o], [o, f32(f32(d + d) + one), f32(d + d), one, o], [o, d, one, d, o],
                     [o, one, o, one, o], [o, o, o, o, o]], f32)
    assert_same(length, want, "length by hand")
    # a cell size that is no power of two: the diagonal step is ONE product, rounded once
    cs = f32(0.3)
    dd = f32(cs * W.SQRT2)
    _, length, _ = W.walk(HAND, cellSize=0.3)
    assert (length[1, 1], length[1, 2], length[2, 1]) == (f32(f32(dd + dd) + cs), f32(dd + dd), dd)
    assert not np.signbit(length[F.receivers(HAND)[0] == N]).any()  # +0


@pytest.mark.parametrize("res", [5, 65, 97])
def test_three_schedules_one_result(res):
    h = tile(res)
    for sea, cs in ((OFF, 1.0), (float(np.median(h)), 0.3)):
        b, l, hops = W.walk(h, sea, cs)
        jb, jl, steps = W.jacobi(h, sea, cs)
        assert_same(jb, b, "Jacobi labels")
        assert_same(jl, l, "Jacobi length")
        assert steps == hops.max()  # a cell is final one step after its receiver
        passes = []
        for cap in (1, 4, None):
            tb, tl, p = W.tiled(h, sea, cs, sweeps=cap)
            assert_same(tb, b, "tiles, cap %s: labels" % cap)
            assert_same(tl, l, "tiles, cap %s: length" % cap)
            passes.append(p)
        assert passes[0] >= passes[1] >= passes[2] and passes[0] <= hops.max()


@pytest.mark.parametrize("res", [5, 65, 160])
def test_labels_are_cells_without_a_receiver_and_count_the_drainage_area(res):
    h = tile(res)
    b, l, hops = W.walk(h)
    r = F.receivers(h)[0]
    flat = b.reshape(-1)
    assert (r.reshape(-1)[flat] == F.NONE).all()      # every label is an outlet or a pit
    assert np.array_equal(flat[flat], flat)           # basin[basin] == basin
    assert np.array_equal(b[r == F.NONE], np.arange(h.size, dtype=np.int32).reshape(h.shape)[r == F.NONE])
    # with rain 1 the cells that carry label o are what the drainage stage accumulates at o
    A = D.accumulate(h)[0]
    counts = np.bincount(flat, minlength=h.size).reshape(h.shape)
    assert np.array_equal(counts[r == F.NONE], A[r == F.NONE].astype(np.int64))
    assert counts[r != F.NONE].sum() == 0
    # the fixed point, one step of the model
    has, q, st, _, _ = W._start(h, OFF, 1.0)
    nb, nl = W._step(b, l, has, q, st)
    assert_same(nb, b, "fixed point: labels")
    assert_same(nl, l, "fixed point: length")
    assert (l[r == F.NONE] == 0).all() and (l[r != F.NONE] > 0).all() and ((hops == 0) == (r == F.NONE)).all()


def test_behind_the_fill_every_label_lies_on_the_border():
    h = tile(160)
    before = np.unique(W.walk(h)[0])
    filled = fill_ref.flood(h)
    assert F.pits(filled) == 0
    after = np.unique(W.walk(filled)[0])
    z, x = np.divmod(after, 160)
    assert ((z == 0) | (z == 159) | (x == 0) | (x == 159)).all()
    zb, xb = np.divmod(before, 160)
    assert not ((zb == 0) | (zb == 159) | (xb == 0) | (xb == 159)).all()  # the bed has pits
    assert (len(before), len(after)) == (718, 636)


def test_sea_cells_label_themselves():
    h = tile(97)
    sea = float(np.median(h))
    b, l, hops = W.walk(h, sea)
    wet = h <= f32(sea)
    own = np.arange(h.size, dtype=np.int32).reshape(h.shape)
    assert wet.sum() > 1000 and np.array_equal(b[wet], own[wet]) and not l[wet].any() and not hops[wet].any()
    assert not np.array_equal(b, W.walk(h)[0])  # the sea matters


def test_the_length_scales_with_the_cell_size_bit_for_bit():
    h = tile(97)
    b1, l1, _ = W.walk(h, cellSize=1.0)
    b2, l2, _ = W.walk(h, cellSize=2.0)
    assert_same(b2, b1, "labels do not depend on the cell size")
    assert_same(l2, (l1 * f32(2.0)).astype(f32), "twice the length")
    assert l1.max() > 30


def test_the_serpentine_is_a_long_chain():
    h = D.serpentine()
    b, l, hops = W.walk(h)
    assert hops.max() == 12404 and hops[1, 1] == 12404  # the channel head
    assert l.max() == l[1, 1] and l.max().view(np.uint32) == f32(12468.604).view(np.uint32)
    out = np.argwhere((h == 0) & F.outlets(h))
    assert len(out) == 1 and b[1, 1] == out[0][0] * 160 + out[0][1]
