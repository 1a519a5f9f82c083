"""The numpy convolution restatement (tests/conv_ref.py) on the CPU: its fmaf against libm's, its strict sequence against
the C oracle bit for bit, both fp32 sequences against the float64 operation's a-priori bound, and the comparison helper
itself.  No GPU."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import conv_ref as R
from conftest import adversarial_tiles

f32 = np.float32


@pytest.fixture(scope="module")
def libm_fmaf():
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return lambda a, b, c: np.array([m.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], f32)


def _fma_cases(rng, n):
    e = rng.integers(-30, 30, (3, n))
    a, b, c = ((rng.random((3, n)) - 0.5) * 2.0 ** e).astype(f32)
    cases = [(a, b, c)]
    # exact cancellation: c = -fl(a*b), the result is the product's rounding error (or an exact zero)
    cases.append((a, b, -(a * b)))
    cases.append((a, b, (a * b)))
    # ties: (1 + i 2^-12)(1 + j 2^-12) = 1 + (i + j) 2^-12 + ij 2^-24 sits halfway between two floats when ij is odd
    i, j = rng.integers(1, 4096, (2, n))
    a2, b2 = (1 + i * 2.0 ** -12).astype(f32), (1 + j * 2.0 ** -12).astype(f32)
    cases.append((a2, b2, np.zeros(n, f32)))
    cases.append((a2, -b2, rng.choice(np.array([0, 1, -1, 2.0 ** -23, -(2.0 ** -24), 3.0], f32), n)))
    # underflow into and below the denormals: products near 2^-126 .. 2^-160, addends 0, +-0 and tiny
    ea, eb = rng.integers(-80, -60, (2, n))
    a3 = ((rng.random(n) + 0.5) * 2.0 ** ea * rng.choice([-1, 1], n)).astype(f32)
    b3 = ((rng.random(n) + 0.5) * 2.0 ** eb * rng.choice([-1, 1], n)).astype(f32)
    c3 = rng.choice(np.array([0.0, -0.0, 1e-45, -1e-45, 2.0 ** -126, -(2.0 ** -140), 3e-39], f32), n)
    cases.append((a3, b3, c3))
    return [tuple(np.asarray(x, f32) for x in cs) for cs in cases]


def test_fmaf_matches_libm(libm_fmaf):
    rng = np.random.default_rng(7)
    for a, b, c in _fma_cases(rng, 4000):
        R.assert_bits_equal(R.fmaf(a, b, c), libm_fmaf(a, b, c), "fmaf")


def test_fmaf_special_values(libm_fmaf):
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38, -3.4e38, 0.5], f32)
    a, b, c = (x.ravel() for x in np.meshgrid(sp, sp, sp, indexing="ij"))
    with np.errstate(invalid="ignore", over="ignore"):
        R.assert_bits_equal(R.fmaf(a, b, c), libm_fmaf(a, b, c), "fmaf special")
    # the cases the strict / FAST difference of the seeds rests on
    assert R.fmaf(f32(-1e-45), f32(0.25), f32(0.0)).view(np.uint32) == np.float32(-0.0).view(np.uint32)
    assert R.fmaf(f32(-0.0), f32(0.25), f32(0.0)).view(np.uint32) == 0
    assert (f32(0.0) + f32(-1e-45) * f32(0.25)).view(np.uint32) == 0


def test_assert_bits_equal_sees_the_sign_of_zero_and_accepts_any_nan():
    with pytest.raises(AssertionError, match="0x80000000"):
        R.assert_bits_equal(np.zeros(3, f32), np.array([0, -0.0, 0], f32), "zeros")
    nan2 = np.array([0x7fc00001], np.uint32).view(f32)
    R.assert_bits_equal(np.array([np.nan], f32), nan2, "nan payloads")
    with pytest.raises(AssertionError):
        R.assert_bits_equal(np.array([1.0], f32), np.array([np.nextafter(f32(1), f32(2))], f32))


@pytest.mark.parametrize("ft", range(14))
def test_filter_tables_match_the_oracle(oracle, ft):
    if ft == R.SOBEL3_2D:
        return
    kx, kz, fac, ks = oracle.kernel_filter_table(ft)
    mx, mz, mf = R.filter_taps(ft)
    R.assert_bits_equal(mx, kx, "kx")
    R.assert_bits_equal(mz, kz, "kz")
    assert f32(mf) == f32(fac) and len(mx) == ks


def test_blur_tables_match_the_oracle(oracle):
    for sigma in range(16):
        for width in range(1, 26):
            R.assert_bits_equal(R.blur_taps("gauss", width, sigma)[0], oracle.gauss_kernel(sigma, width), (sigma, width))


def _tiles(res):
    t = dict(adversarial_tiles(res))
    t.update(R.signed_zero_tiles(res))
    rng = np.random.default_rng(res)
    t["signed"] = ((rng.random((res, res), dtype=f32) - f32(0.5)) * f32(100)).astype(f32)
    return t


@pytest.mark.parametrize("ft", range(14))
def test_strict_restatement_equals_the_oracle_filters(oracle, ft):
    for res in (9, 37):
        for name, t in _tiles(res).items():
            got, rec = R.filter_apply(t, ft, 3, record=(1, 2, 3))
            for it in (1, 2, 3):
                R.assert_bits_equal(rec[it], oracle.kernel_filter(t, ft, it), "ft=%d it=%d %d^2 %s" % (ft, it, res, name))


@pytest.mark.parametrize("width", range(1, 26))
def test_strict_restatement_equals_the_oracle_blurs(oracle, width):
    res = 31
    for name, t in _tiles(res).items():
        sigma = width % 16
        kx, kz, fac = R.blur_taps("gauss", width, sigma)
        R.assert_bits_equal(R.separable(t, kx, kz, fac, 2, ksize=width), oracle.gauss(t, width, sigma, 2),
                            "gauss %d %s" % (width, name))
        kx, kz, fac = R.blur_taps("smooth", width)
        R.assert_bits_equal(R.separable(t, kx, kz, fac, 1, ksize=width), oracle.smooth(t, width, 1),
                            "smooth %d %s" % (width, name))


@pytest.mark.parametrize("ksize", [1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 17, 25])
def test_strict_restatement_equals_the_oracle_custom_kernels(oracle, ksize):
    rng = np.random.default_rng(ksize)
    res = 23
    kx = (rng.random(ksize) * 2 - 0.6).astype(f32)
    kz = (rng.random(ksize) * 2 - 0.6).astype(f32)
    for factor in (0.37, -1.7, 1.0):
        for name, t in _tiles(res).items():
            R.assert_bits_equal(R.separable(t, kx, kz, factor, ksize=ksize), oracle.separable(t, ksize, kx, kz, factor),
                                "k=%d f=%g %s" % (ksize, factor, name))
    # all-negative taps: every product of a zero plane is -0
    neg = -np.abs(kx) - f32(0.01)
    for factor in (1.0, -2.0):
        for name, t in R.signed_zero_tiles(res).items():
            want = oracle.separable(t, ksize, neg, neg, factor)
            R.assert_bits_equal(R.separable(t, neg, neg, factor, ksize=ksize), want, "neg k=%d f=%g %s" % (ksize, factor, name))


def test_signed_zero_planes_give_plus_zero_in_strict_mode(oracle):
    """The reference seeds every tap sum with +0: a sum whose products are all -0 is +0.  The FAST sequence
    (fmaf(v, k, t) from t = +0) gives +0 for exact -0 products and -0 for products that underflow."""
    res = 12
    z = R.signed_zero_tiles(res)
    for name, t in z.items():
        for ft in (2, 3, 8) if name != "neg_denormal" else (2, 3):  # (Smooth3's taps are 1: -1e-45 survives)
            got = R.filter_apply(t, ft)
            R.assert_bits_equal(got, np.zeros_like(t), "strict %s ft=%d" % (name, ft))
            R.assert_bits_equal(oracle.kernel_filter(t, ft), np.zeros_like(t), "oracle %s ft=%d" % (name, ft))
    R.assert_bits_equal(R.filter_apply(z["neg_zero"], 2, fast=True), np.zeros((res, res), f32), "fast -0")
    # FAST: the X pass of -1e-45 underflows to -0 (fmaf rounds the exact negative product), the Z pass of -0 gives +0
    k = R.filter_taps(2)[0]
    R.assert_bits_equal(R.pass_x(z["neg_denormal"], k, 1.0, fast=True), np.full((res, res), -0.0, f32), "fast X -1e-45")
    R.assert_bits_equal(R.pass_x(z["neg_denormal"], k, 1.0), np.zeros((res, res), f32), "strict X -1e-45")
    R.assert_bits_equal(R.filter_apply(z["neg_denormal"], 2, fast=True), np.zeros((res, res), f32), "fast -1e-45")
    neg = R.NEG_TAPS[5]
    R.assert_bits_equal(R.separable(z["zero"], neg, neg, 1.0, fast=True), np.zeros((res, res), f32), "fast 0 x neg")
    R.assert_bits_equal(R.separable(z["zero"], neg, neg, -1.0), np.full((res, res), -0.0, f32), "strict 0 x neg x -1")


@pytest.mark.parametrize("ft", [0, 2, 3, 6, 8, 9, 12])
def test_both_fp32_sequences_stay_inside_the_float64_bound(ft):
    rng = np.random.default_rng(ft)
    res = 40
    kx, kz, fac = R.filter_taps(ft)
    for t in (rng.random((res, res), dtype=f32), ((rng.random((res, res), dtype=f32) - f32(0.5)) * f32(1e3)).astype(f32),
              adversarial_tiles(res)["impulse_corner"]):
        exact, bound = R.separable64(t, kx, kz, fac, 5)
        for fast in (False, True):
            got = R.separable(t, kx, kz, fac, 5, fast=fast).astype(np.float64)
            assert (np.abs(got - exact) <= bound).all(), (ft, fast, float(np.max(np.abs(got - exact) - bound)))
        # the bound is not vacuous: far below the plane's magnitude
        assert bound.max() < 1e-5 * np.abs(exact).max()


def test_custom_kernels_stay_inside_the_float64_bound():
    rng = np.random.default_rng(3)
    t = ((rng.random((33, 33), dtype=f32) - f32(0.5)) * f32(20)).astype(f32)
    for ksize in (4, 11, 25):
        kx, kz = (rng.random((2, ksize)) - 0.4).astype(f32)
        exact, bound = R.separable64(t, kx, kz, -1.3, 2, ksize=ksize)
        for fast in (False, True):
            got = R.separable(t, kx, kz, -1.3, 2, ksize=ksize, fast=fast).astype(np.float64)
            assert (np.abs(got - exact) <= bound).all(), (ksize, fast)


def test_banded_restatement_equals_the_whole_plane():
    rng = np.random.default_rng(11)
    t = rng.random((2, 150, 70), dtype=f32)
    kx, kz, fac = R.filter_taps(2)
    whole = R.separable(t, kx, kz, fac, 6, fast=True)
    for r0, r1, band in R.banded(lambda a: R.separable(a, kx, kz, fac, 6, fast=True), t, 6 * 2, [(0, 10), (70, 90), (140, 150)]):
        R.assert_bits_equal(band, whole[..., r0:r1, :], "band %d" % r0)


def test_stripe_rows_clamp_to_the_grid_rows():
    rng = np.random.default_rng(12)
    t = rng.random((30, 17), dtype=f32)
    k = R.filter_taps(0)[0]
    # rows 5 .. 24 of a buffer are grid rows 0 .. 19 (ghost rows above and below): clamping there is clamping the grid
    want = R.pass_z(t[5:25], k, 1.0)
    R.assert_bits_equal(R.pass_z(t, k, 1.0, zc0=5, zc1=24)[5:25], want, "stripe clamp")
