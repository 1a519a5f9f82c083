"""The numpy model of depression filling (tests/fill_ref.py) against itself: a hand-worked tile, the three schedules bit
for bit, every property the model states, and the pits of the fluvial stage gone."""
import numpy as np
import pytest

import fill_ref as L
import fluvial_ref as F
from test_hydraulic_ref import relief

f32 = np.float32
OFF = float(F.SEA_OFF)
_memo = {}


def tile(name):
    if name not in _memo:
        rng = np.random.default_rng(7)
        make = {"fbm64": lambda: relief(64), "fbm128": lambda: relief(128), "fbm160": lambda: relief(160, 500),
                "noisy97": lambda: (relief(97, 97) + rng.standard_normal((97, 97)).astype(f32) * f32(0.01)).astype(f32),
                "rand130": lambda: np.random.default_rng(3).random((130, 130), dtype=f32)}
        _memo[name] = np.ascontiguousarray(make[name](), f32)
        _memo[name].setflags(write=False)
    return _memo[name]


def flood(name, eps, sea=OFF):
    key = (name, eps, sea)
    if key not in _memo:
        _memo[key] = L.flood(tile(name), eps, sea)
        _memo[key].setflags(write=False)
    return _memo[key]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# a 7 x 7 tile, rows z = 0..6: inside a border of 9 whose one low cell, (z 3, x 0) = 2, is the way out, a wall of 8 and
# slopes of 7 around row 3.  Along row 3 lie an outer hollow (3 behind the sill 4, the side cell 5 above it), the saddle 6,
# and behind it an inner hollow of two levels (1 and, diagonally below the saddle, 2) that spills over the saddle into the
# outer one.  Every 7 and 8 has a lower neighbour before and after, so only the hollows move.
HAND = np.array([[9, 9, 9, 9, 9, 9, 9],
                 [9, 8, 8, 8, 8, 8, 9],
                 [9, 7, 5, 7, 7, 7, 9],
                 [2, 4, 3, 6, 1, 7, 9],
                 [9, 7, 7, 7, 2, 7, 9],
                 [9, 8, 8, 8, 8, 8, 9],
                 [9, 9, 9, 9, 9, 9, 9]], f32)


def test_the_hand_worked_tile():
    # epsilon 0: the spill elevations.  The sill 4 keeps its height (its way out is the 2 on the border), the outer hollow
    # rises to it, the saddle stays, both levels of the inner hollow rise to the saddle: flats remain
    want0 = HAND.copy()
    want0[3, 2] = 4
    want0[3, 4] = want0[4, 4] = 6
    # epsilon 1/4 (exact in binary): every filled cell lies 1/4 above the neighbour it drains to.  3 -> 4 + 1/4; the inner
    # hollow's two cells both touch the saddle (one of them diagonally): 6 + 1/4 each; 5 and 7 stand above their lakes
    want25 = HAND.copy()
    want25[3, 2] = 4.25
    want25[3, 4] = want25[4, 4] = 6.25
    for eps, want in ((0.0, want0), (0.25, want25)):
        for got in (L.flood(HAND, eps), L.jacobi(HAND, eps)[0], L.tiled(HAND, eps, tile=(4, 2), sweeps=1)[0],
                    L.tiled(HAND, eps, tile=(3, 3))[0]):
            assert np.array_equal(bits(got), bits(want)), (eps, got)
    assert F.pits(HAND) == 2 and F.pits(want0) == 3 and F.pits(want25) == 0  # a flat has no receiver either
    # the lake depths
    depth = want0 - HAND
    assert depth.sum() == 1 + 5 + 4 and depth[3, 2] == 1 and depth[3, 4] == 5 and depth[4, 4] == 4
    # a sea at 2.5 makes both levels of the inner hollow outlets: they stay, the outer hollow fills as before
    sea = L.flood(HAND, 0.25, 2.5)
    want = want25.copy()
    want[3, 4], want[4, 4] = 1, 2
    assert np.array_equal(bits(sea), bits(want))


@pytest.mark.parametrize("name", ["fbm64", "fbm160", "noisy97", "rand130"])
@pytest.mark.parametrize("eps", [0.0, 1e-4])
def test_the_schedules_agree_bit_for_bit(name, eps):
    h = tile(name)
    want = flood(name, eps)
    jac, jp = L.jacobi(h, eps)
    free, fp = L.tiled(h, eps)
    capped, cp = L.tiled(h, eps, sweeps=4)
    for what, got in (("jacobi", jac), ("tiled", free), ("tiled, 4 sweeps", capped)):
        assert np.array_equal(bits(got), bits(want)), (name, eps, what)
    assert fp <= cp <= jp, (fp, cp, jp)  # sweeping on chip saves passes, which is the kernel's point


@pytest.mark.parametrize("name", ["fbm64", "noisy97", "rand130"])
@pytest.mark.parametrize("eps", [0.0, 1e-4])
def test_the_properties_of_the_model(name, eps):
    h = tile(name)
    W = flood(name, eps)
    out = F.outlets(h)
    assert np.isfinite(W).all() and (W >= h).all()
    assert np.array_equal(bits(W[out]), bits(h[out]))
    assert W.min() >= h.min()
    assert (W > h).any()  # these tiles do have hollows
    # a fixed point of the operator, and filling a filled tile changes nothing
    assert np.array_equal(bits(L.step(W, h, out, f32(eps))), bits(W))
    assert np.array_equal(bits(L.flood(W, eps)), bits(W))
    # where nothing was filled the input is returned bit for bit; a tile without pits comes back whole
    assert np.array_equal(bits(W[W == h]), bits(h[W == h]))
    ramp = (np.arange(40, dtype=f32)[None, :] * f32(0.01) + np.arange(40, dtype=f32)[:, None] * f32(0.003)).astype(f32)
    assert F.pits(ramp) == 0 and np.array_equal(bits(L.flood(ramp, eps)), bits(ramp))
    if eps == 0.0:  # the spill elevation: no cell above the highest of its way out, so none above the border's maximum
        assert W.max() <= max(h.max(), h[out].max())


@pytest.mark.parametrize("name,before", [("fbm64", 10), ("fbm128", 52), ("fbm160", 77)])
def test_filling_leaves_the_fluvial_stage_no_pits(name, before):
    h = tile(name)
    assert F.pits(h) == before
    assert F.pits(flood(name, 1e-4)) == 0


def test_a_sea_inside_the_range_stays_and_leaves_no_pits():
    h = tile("fbm128")
    sea = float(np.median(h))
    W = L.flood(h, 1e-4, sea)
    low = h <= f32(sea)
    assert low.any() and not low.all()
    assert np.array_equal(bits(W[low]), bits(h[low]))
    assert (W >= h).all() and F.pits(W, sea) == 0
    assert np.array_equal(bits(L.jacobi(h, 1e-4, sea)[0]), bits(W))
