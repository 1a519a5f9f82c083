"""The stream-order model (tests/stream_order_ref.py) without a GPU: a tile worked by hand, the schedules that must agree,
the properties the header states, the tie to the drainage area, filled tiles and the two long chains.  Byte for byte
throughout."""
import numpy as np
import pytest

import drainage_ref as D
import fill_ref
import fluvial_ref as F
import stream_order_ref as S
import terrain_tiles as T
from test_hydraulic_ref import relief

f32 = np.float32
OFF = float(F.SEA_OFF)
_memo = {}


def tile(res):
    if res not in _memo:
        _memo[res] = (np.random.default_rng(res).random((res, res), dtype=f32) if res <= 5
                      else np.ascontiguousarray(relief(res, 500 if res == 160 else 300), f32))  # the GPU suite's tiles
        _memo[res].setflags(write=False)
    return _memo[res]


def area(res):
    key = ("area", res)
    if key not in _memo:
        _memo[key] = D.accumulate(tile(res))[0]
        _memo[key].setflags(write=False)
    return _memo[key]


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


# Rows are z, columns x, c = z * 7 + x; S is the row above on the page (z - 1), N the row below.  The 9s are slopes that
# are no river (their drainage is 0); the river cells, with their receivers:
#   a (1,1)=5 -> NE (2,2);  b (1,2)=5 -> N (2,2) (drop 1);  (2,2)=4 -> NE (3,3)
#   (4,2)=4 -> SE (3,3) (its NE neighbour (5,3) is as high as itself)
#   (3,3)=3 -> E (3,4) (1 beats the diagonal drops of 1 * 0.7071 to (2,4) and (4,4));  (3,4)=2 -> E (3,5)
#   (2,4)=2 -> NE (3,5);  (5,3)=4 -> SE (4,4) and (5,5)=4 -> SW (4,4) (drop 2 * 0.7071);  (4,4)=2 -> SE (3,5)
#   (3,5)=1 -> E, the low border cell (3,6)=0, which has no receiver and is a channel cell: the mouth
HAND = np.array([[9, 9, 9, 9, 9, 9, 9],
                 [9, 5, 5, 9, 9, 9, 9],
                 [9, 9, 4, 9, 2, 9, 9],
                 [9, 9, 9, 3, 2, 1, 0],
                 [9, 9, 4, 9, 2, 9, 9],
                 [9, 9, 9, 4, 9, 4, 9],
                 [9, 9, 9, 9, 9, 9, 9]], f32)
RIVER = (HAND < 9).astype(f32)


def test_a_tile_worked_by_hand():
    N = F.NONE
    r = F.receivers(HAND)[0]
    river = {(1, 1): 7, (1, 2): 3, (2, 2): 7, (4, 2): 5, (3, 3): 1, (3, 4): 1, (2, 4): 7, (5, 3): 5, (5, 5): 4, (4, 4): 5,
             (3, 5): 1, (3, 6): N}
    assert {zx: int(r[zx]) for zx in river} == river and int((RIVER > 0).sum()) == len(river)
    order, link, chain = S.walk(HAND, OFF, RIVER, 0.5)
    # heads a, b, (4,2), (2,4), (5,3), (5,5): order 1, each its own link (8, 9, 30, 18, 38, 40)
    # (2,2): a and b, two of order 1 -> 2, a confluence: link 16.  (4,4): (5,3) and (5,5) likewise -> 2, link 32
    # (3,3): (2,2) of order 2 and (4,2) of order 1: the maximum once -> stays 2; two donors, so a link starts: 24
    # (3,4): one donor -> its order 2 and its link 24, a one-donor reach
    # (3,5): (3,4) and (4,4) of order 2 and (2,4) of order 1: three donors of which the two largest tie -> 3, link 26
    # (3,6): the mouth, one donor -> 3 and link 26.  Everything else: no channel, 0 and -1
    want_o = [[0, 0, 0, 0, 0, 0, 0],
              [0, 1, 1, 0, 0, 0, 0],
              [0, 0, 2, 0, 1, 0, 0],
              [0, 0, 0, 2, 2, 3, 3],
              [0, 0, 1, 0, 2, 0, 0],
              [0, 0, 0, 1, 0, 1, 0],
              [0, 0, 0, 0, 0, 0, 0]]
    want_l = [[-1, -1, -1, -1, -1, -1, -1],
              [-1, 8, 9, -1, -1, -1, -1],
              [-1, -1, 16, -1, 18, -1, -1],
              [-1, -1, -1, 24, 24, 26, 26],
              [-1, -1, 30, -1, 32, -1, -1],
              [-1, -1, -1, 38, -1, 40, -1],
              [-1, -1, -1, -1, -1, -1, -1]]
    assert order.dtype == np.uint8 and order.tolist() == want_o
    assert link.dtype == np.int32 and link.tolist() == want_l
    assert chain == 6  # a, (2,2), (3,3), (3,4), (3,5), the mouth
    # the threshold cuts b off: (2,2) is no confluence any more -- order 1 and a's link; (3,3) now joins two of order 1,
    # which gives the 2 it had, and is a confluence as before: nothing changes below it
    cut = RIVER.copy()
    cut[1, 2] = f32(0.25)
    order, link, chain = S.walk(HAND, OFF, cut, 0.5)
    want_o[1][2], want_o[2][2] = 0, 1
    want_l[1][2], want_l[2][2] = -1, 8
    assert order.tolist() == want_o and link.tolist() == want_l and chain == 6
    # three donors of which the two SMALLER tie: without (5,5), (4,4) has order 1, and (3,5) gathers 2, 1, 1 -> 2
    cut = RIVER.copy()
    cut[5, 5] = f32(np.nan)  # a NaN is no channel
    order, link, _ = S.walk(HAND, OFF, cut, 0.5)
    assert (order[4, 4], link[4, 4], order[3, 5], link[3, 5], order[3, 6], order[5, 5], link[5, 5]) == (1, 38, 2, 26, 2, 0, -1)
    # a sea up to (3,5) takes that cell's receiver away, not its channel: it keeps its 3 as a mouth, and the border cell
    # behind it has lost its donor and is a head
    so, sl, _ = S.walk(HAND, 1.0, RIVER, 0.5)
    o, l, _ = S.walk(HAND, OFF, RIVER, 0.5)
    assert (so[3, 5], sl[3, 5], so[3, 6], sl[3, 6]) == (3, 26, 1, 27)
    so[3, 6], sl[3, 6] = 3, 26
    assert_same(so, o, "a sea at the mouth: order")
    assert_same(sl, l, "a sea at the mouth: link")
    # ... and without a drainage plane every cell is a channel cell: the slopes count, and 1 + log2(area) still bounds
    o, l, _ = S.walk(HAND)
    assert (o > 0).all() and (l >= 0).all() and o[3, 6] >= 3


def cases(h, A):
    yield OFF, None, 0.0
    yield float(np.median(h)), None, 0.0
    yield OFF, A, 8.0
    yield float(np.median(h)), A, 3.0


@pytest.mark.parametrize("res", [5, 16, 65, 97])
def test_three_schedules_one_result(res):
    h = tile(res)
    for sea, A, thr in cases(h, area(res)):
        o, l, chain = S.walk(h, sea, A, thr)
        jo, jl, steps = S.jacobi(h, sea, A, thr)
        assert_same(jo, o, "Jacobi order")
        assert_same(jl, l, "Jacobi link")
        # a head is final at the start, every other cell at the latest one step after its donors
        assert steps <= max(chain - 1, 0)
        passes = []
        for cap in (1, 2, None):
            to, tl, p = S.tiled(h, sea, A, thr, sweeps=cap)
            assert_same(to, o, "tiles, cap %s: order" % cap)
            assert_same(tl, l, "tiles, cap %s: link" % cap)
            passes.append(p)
        assert passes[0] >= passes[1] >= passes[2] and passes[0] <= max(chain - 1, 0)


def test_the_figures_of_the_relief_tiles():
    assert [int(S.walk(tile(res))[0].max()) for res in (16, 65, 97, 160)] == [3, 5, 5, 5]
    got = []
    for res in (16, 65, 97, 160):
        o, l, _ = S.walk(tile(res), OFF, area(res), 8.0)
        got.append((int((o > 0).sum()), len(np.unique(l[l >= 0]))))
    assert got == [(57, 16), (867, 331), (2028, 777), (5798, 2253)]


@pytest.mark.parametrize("name", sorted(T.TIES))
def test_the_schedules_agree_on_tie_rich_tiles(name):
    h = T.GENERATORS[name](33, np.random.default_rng(7))
    A = D.accumulate(h)[0]
    for sea, dr, thr in ((OFF, None, 0.0), (T.sea_at(h), A, 2.0)):
        o, l, chain = S.walk(h, sea, dr, thr)
        jo, jl, _ = S.jacobi(h, sea, dr, thr)
        assert_same(jo, o, name + ": Jacobi order")
        assert_same(jl, l, name + ": Jacobi link")
        for cap in (1, 2, None):
            to, tl, _ = S.tiled(h, sea, dr, thr, tile=(16, 8), sweeps=cap)
            assert_same(to, o, "%s, tiles cap %s: order" % (name, cap))
            assert_same(tl, l, "%s, tiles cap %s: link" % (name, cap))


def donors_of(h, sea, dr, thr):
    ch, bits = S.donor_bits(h, sea, dr, thr)
    return ch, bits, np.unpackbits(bits.reshape(-1, 1), axis=1).sum(axis=1).reshape(h.shape)


@pytest.mark.parametrize("res", [5, 65, 160])
def test_the_properties(res):
    h = tile(res)
    A = area(res)
    for sea, dr, thr in cases(h, A):
        o, l, _ = S.walk(h, sea, dr, thr)
        ch, bits, nd = donors_of(h, sea, dr, thr)
        assert np.array_equal(o > 0, ch) and np.array_equal(l >= 0, ch)          # order > 0 <=> ch <=> link >= 0
        # order never falls along a receiver step between channel cells
        r = F.receivers(h, sea)[0]
        off = np.array([dz * res + dx for dx, dz in F.NEIGHBOURS] + [0], np.int64)
        q = (np.arange(h.size) + off[r.reshape(-1)]).reshape(h.shape)
        both = ch & (r != F.NONE) & ch.reshape(-1)[q]
        assert (o.reshape(-1)[q][both] >= o[both]).all() and (both.sum() > 0 or res == 5)
        # link[link[c]] == link[c]; the distinct links are exactly the channel cells with |D| != 1
        lf = l.reshape(-1)
        assert np.array_equal(lf[lf[lf >= 0]], lf[lf >= 0])
        own = np.arange(h.size, dtype=np.int32).reshape(h.shape)
        assert np.array_equal(np.unique(lf[lf >= 0]), own[ch & (nd != 1)])
        # the fixed point, one step of the model
        no, nl = S.step(o, l, ch, bits)
        assert_same(no, o, "fixed point: order")
        assert_same(nl, l, "fixed point: link")
    # without `drainage`: order <= 1 + floor(log2(A)), A the rain-1 drainage area
    o, l, _ = S.walk(h)
    assert (o <= 1 + np.floor(np.log2(A.astype(np.float64)))).all() and o.max() >= 2
    # drainage = A with a threshold <= 1 selects every cell: the drainage == NULL result
    for thr in (1.0, 0.5, -3.0):
        to, tl, _ = S.walk(h, OFF, A, thr)
        assert_same(to, o, "threshold %g: order" % thr)
        assert_same(tl, l, "threshold %g: link" % thr)


def test_behind_the_fill_a_channel_never_ends_inland():
    h = fill_ref.flood(tile(97))
    assert F.pits(h) == 0
    A = D.accumulate(h)[0]
    r = F.receivers(h)[0]
    off = np.array([dz * 97 + dx for dx, dz in F.NEIGHBOURS] + [0], np.int64)
    q = (np.arange(h.size) + off[r.reshape(-1)]).reshape(h.shape)
    for thr in (2.0, 8.0, 50.0):
        o, l, _ = S.walk(h, OFF, A, thr)
        ch = o > 0
        assert ch.sum() > 50 and ch.reshape(-1)[q][ch].all()  # a channel cell's receiver is a channel cell (or it is an outlet: q == c)
        # and every link ends at a confluence or on the border
        assert (r[ch & ~ch.reshape(-1)[q]] == F.NONE).all()


def test_the_serpentine_is_one_link_of_order_one():
    h = D.serpentine()
    dr = S.channel_of(h)
    o, l, chain = S.walk(h, OFF, dr, 0.5)
    ch = dr > 0
    assert chain == int(ch.sum()) == 12405 and ch[1, 1]  # the flow path: it cuts two cells off at each of the 78 turns
    assert (o[ch] == 1).all() and not o[~ch].any()
    assert (l[ch] == 1 * 160 + 1).all() and (l[~ch] == -1).all()  # the head's index
    # without the channel plane the walls are slopes that drain into the channel: it is no chain of single donors
    assert S.walk(h)[0].max() > 1


def test_a_second_head_sends_its_order_down_the_whole_chain():
    h = S.two_heads()
    res = 160
    r = F.receivers(h)[0]
    base = S.channel_of(D.serpentine()) > 0
    assert r[2, res - 3] == 3 and np.array_equal(r[base], F.receivers(D.serpentine())[0][base])  # N; the chain is as it was
    dr = S.channel_of(h, ((1, 1), (2, res - 3)))
    o, l, chain = S.walk(h, OFF, dr, 0.5)
    ch = dr > 0
    assert ch.sum() == 12406 and chain == 12405 and np.array_equal(ch & base, base)
    # row 1 up to the corner it cuts and the connector: order 1, the first head's link; the second head: its own
    first = np.zeros_like(ch)
    first[1, 1:res - 2] = first[2, res - 2] = True
    assert (first & base).sum() == 158 and (o[first] == 1).all() and (l[first] == res + 1).all()
    assert o[2, res - 3] == 1 and l[2, res - 3] == 2 * res + res - 3
    rest = base & ~first
    assert rest.sum() == 12405 - 158 and (o[rest] == 2).all() and (l[rest] == 3 * res + res - 3).all()
    assert len(np.unique(l[ch])) == 3
