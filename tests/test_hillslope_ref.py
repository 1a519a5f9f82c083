"""The hillslope diffusion model (tests/hillslope_ref.py, the restatement of nz_hillslope_diffusion) checked on the CPU:
hand-worked tiles, the stated properties, the float32 error against the same recurrences in float64 and against a dense
float64 solve, the smoothing of an fBm tile, and iterations against repeated calls."""
from fractions import Fraction as Q

import numpy as np
import pytest

import hillslope_ref as R
from test_hydraulic_ref import relief

f32 = np.float32
SIZES = (3, 5, 64, 130)
RS = (0.01, 1.0, 100.0, 1e4)
_memo = {}


def tile(res, seed=1):
    """rng.random * 100 of the seed, computed once, read only."""
    if (res, seed) not in _memo:
        t = (np.random.default_rng(seed).random((res, res), dtype=f32) * f32(100.0)).astype(f32)
        t.setflags(write=False)
        _memo[(res, seed)] = t
    return _memo[(res, seed)]


def assert_same(got, want, what):
    assert got.dtype == want.dtype == f32 and got.shape == want.shape, what
    bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def border(res):
    b = np.zeros((res, res), bool)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = True
    return b


# By hand, r = 1: B = 3.  A line of 3 has one unknown, x_1 = (v_0 + v_1 + v_2) / 3.  A line of 4 has two: den_1 = 3, inv_1 =
# cp_1 = 1/3, den_2 = 3 - 1/3 = 8/3, inv_2 = cp_2 = 3/8; with a = v_0 + v_1 and b = v_2 + v_3 the recurrences give
# p_1 = a/3, p_2 = (v_2 + a/3) 3/8, x_2 = p_2 + 3 v_3 / 8 = (a + 3 b) / 8, x_1 = a/3 + x_2 / 3 = (3 a + b) / 8.
# The operations are float32, 1/3 is rounded and a cell is the end of at most 10 of them on values up to 24: 10 * 24 * 2^-24
# = 1.4e-5 bounds the error.
HAND_TOL = 2e-5


def test_a_hand_worked_3x3():
    h = np.array([[1, 2, 3], [4, 14, 6], [7, 8, 9]], f32)
    # half-step X, row 1: (4 + 14 + 6) / 3 = 8;  half-step Z, column 1: (2 + 8 + 8) / 3 = 6
    want = [[Q(1), Q(2), Q(3)], [Q(4), Q(6), Q(6)], [Q(7), Q(8), Q(9)]]
    got = R.diffuse_r(h, 1.0)
    assert got.dtype == f32
    for z in range(3):
        for x in range(3):
            assert abs(Q(float(got[z, x])) - want[z][x]) <= Q(HAND_TOL), (z, x, got[z, x])
    assert_same(got[border(3)], h[border(3)], "3x3: the border")


def test_a_hand_worked_4x4():
    h = np.array([[0, 8, 16, 0], [8, 16, 0, 8], [0, 0, 8, 16], [8, 0, 8, 0]], f32)
    # half-step X: row 1, a = 24, b = 8 -> (10, 6); row 2, a = 0, b = 24 -> (3, 9)
    # half-step Z: column 1 = (8, 10, 3, 0), a = 18, b = 3 -> (57/8, 27/8); column 2 = (16, 6, 9, 8), a = 22, b = 17 ->
    # (83/8, 73/8)
    want = [[Q(0), Q(8), Q(16), Q(0)], [Q(8), Q(57, 8), Q(83, 8), Q(8)], [Q(0), Q(27, 8), Q(73, 8), Q(16)],
            [Q(8), Q(0), Q(8), Q(0)]]
    got = R.diffuse_r(h, 1.0)
    for z in range(4):
        for x in range(4):
            assert abs(Q(float(got[z, x])) - want[z][x]) <= Q(HAND_TOL), (z, x, got[z, x])
    assert_same(got[border(4)], h[border(4)], "4x4: the border")
    inv, cp = R.tables(1.0, 4)
    assert abs(Q(float(inv[1])) - Q(1, 3)) < Q(1e-7) and abs(Q(float(inv[2])) - Q(3, 8)) < Q(1e-7)
    assert abs(Q(float(cp[1])) - Q(1, 3)) < Q(1e-7) and abs(Q(float(cp[2])) - Q(3, 8)) < Q(1e-7)


def test_r_zero_and_tiny_tiles_return_the_heights_bit_for_bit():
    h = np.array(tile(5))
    h[1, 1], h[2, 2], h[0, 3] = f32(-0.0), f32(np.nan), f32(np.inf)
    for kw in (dict(diffusivity=0.0, dt=5.0), dict(diffusivity=3.0, dt=0.0), dict(diffusivity=-0.0, dt=1.0)):
        assert_same(R.diffuse(h, iterations=3, **kw), h, kw)
    for res in (1, 2):
        t = np.full((res, res), f32(-0.0))
        for r in RS:
            assert_same(R.diffuse_r(t, r, 2), t, (res, r))
    # the recurrence itself would not keep the sign of a -0.0: that is why r == 0 is a definition
    z = np.ones((3, 3), f32)
    z[1, 1] = f32(-0.0)
    inv, cp = R.tables(0.0, 3)
    assert not R.same(R.step(z, f32(0.0), inv, cp), z)


@pytest.mark.parametrize("res", SIZES)
def test_borders_keep_their_bits_and_the_range_holds(res):
    h = tile(res)
    lo, hi = h.min(), h.max()
    b = border(res)
    for r in RS:
        for its in (1, 2):
            got = R.diffuse_r(h, r, its)
            assert_same(got[b], h[b], ("border", res, r, its))
            assert lo <= got.min() and got.max() <= hi, (res, r, its, got.min(), got.max())
            if res >= 3:
                assert not R.same(got, h)


# Measured here on the seed-1 tiles (3^2, 5^2, 64^2, 130^2; r = 0.01, 1, 100, 1e4): the float32 result is within 8.3e-4 of
# the same recurrences in float64 (the largest at 130^2, r = 100) on heights up to 100; the bound is that with a margin of 4
# for other seeds.  At 16^2 the float32 result is within 3.8e-5 of the dense float64 solve (measured, seeds 1 and 2; bound
# 4x).  The dense solve and the float64 recurrences solve the same linear system, so between them only the dense solve's own
# error shows: the 14 x 14 matrix has a condition number of at most 91 (r = 1e4: eigenvalues 1 + 2 r (1 - cos(k pi / 15))),
# so two solves on heights up to 100 err by about 2 * 91 * 2^-53 * 100 = 2e-12 at the most (measured 5.7e-14).
F32_VS_F64 = 4 * 8.3e-4
DENSE_VS_F64 = 2e-12
DENSE_VS_F32 = 4 * 3.8e-5


def test_agrees_with_float64_and_with_a_dense_solve(capsys):
    worst = 0.0
    for res in SIZES:
        for r in RS:
            for seed in (1, 2):
                err = float(np.abs(R.diffuse_r(tile(res, seed), r) - R.diffuse_r(tile(res, seed), r, dtype=np.float64)).max())
                if seed == 1:
                    worst = max(worst, err)
                assert err <= F32_VS_F64, (res, r, seed, err)
    d64 = d32 = 0.0
    for r in RS:
        for seed in (1, 2):
            h = tile(16, seed)
            dense = R.dense(h, r)
            d64 = max(d64, float(np.abs(dense - R.diffuse_r(h, r, dtype=np.float64)).max()))
            d32 = max(d32, float(np.abs(dense - R.diffuse_r(h, r)).max()))
    with capsys.disabled():
        print("\nhillslope: float32 vs float64 %.3g (seed 1), dense vs float64 %.3g, dense vs float32 %.3g" % (worst, d64, d32))
    assert d64 <= DENSE_VS_F64 and d32 <= DENSE_VS_F32, (d64, d32)


def laplacian_energy(h):
    h = h.astype(np.float64)
    lap = h[1:-1, :-2] + h[1:-1, 2:] + h[:-2, 1:-1] + h[2:, 1:-1] - 4.0 * h[1:-1, 1:-1]
    return float((lap * lap).sum())


def test_every_iteration_smooths_an_fbm_tile():
    h = np.ascontiguousarray(relief(97), f32)
    for r in (0.25, 10.0):
        energy = [laplacian_energy(h)]
        cur = h
        for _ in range(5):
            cur = R.diffuse_r(cur, r)
            energy.append(laplacian_energy(cur))
        assert all(b < a for a, b in zip(energy, energy[1:])), (r, energy)


def test_iterations_are_repeated_calls():
    for res, r in ((5, 1.0), (64, 100.0), (130, 0.01)):
        h = tile(res)
        three = R.diffuse_r(h, r, 3)
        cur = h
        for _ in range(3):
            cur = R.diffuse_r(cur, r)
        assert_same(three, cur, (res, r))
    assert_same(R.diffuse(tile(64), 0.5, 4.0, 2), R.diffuse_r(tile(64), 2.0, 2), "r is the one product")
    assert R.DEFAULTS == dict(diffusivity=0.01, dt=1.0, iterations=1)


def test_a_nan_spreads_along_its_line_and_then_across():
    h = np.array(tile(64))
    h[20, 30] = f32(np.nan)
    got = R.diffuse_r(h, 1.0)
    nan = np.isnan(got)
    b = border(64)
    assert not nan[b].any()                           # the held cells never take part
    assert nan[1:-1, 1:-1].all()                      # row 20 by half-step X, then every column by half-step Z
    h[20, 30] = f32(np.inf)
    got = R.diffuse_r(h, 1.0)
    assert not np.isfinite(got[1:-1, 1:-1]).any() and np.isfinite(got[b]).all()
