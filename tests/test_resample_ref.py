"""The resampling model (tests/resample_ref.py, include/noize_hip.h) on the CPU: the weights are the exact rationals, known
answers that need no second implementation, and the reference's own stripe form equals its monolithic form.  The last test
holds the three hosts to the feature's surface."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import resample_ref as R
from conftest import ROOT

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("f", R.FACTORS)
def test_weights_are_the_exact_rationals_and_sum_to_one(f):
    for filt in R.FILTERS:
        for p in range(f):
            first, exact = R.taps_exact(f, filt, p)
            first32, w32 = R.taps(f, filt, p)
            assert first == first32 and len(exact) == len(w32) == (1, 2, 4)[filt]
            for e, w in zip(exact, w32):
                assert w.dtype == f32 and Fraction(float(w)) == e, (f, filt, p, e, w)  # exact after rounding to float32
            assert sum(exact) == 1
            d, t = R.phase(f, p)
            assert 0 < t < 1 and d == (-1 if p < f // 2 else 0)
            # the cell-centred position: i0 + t = i + (2p+1)/(2f) - 1/2
            assert d + t == Fraction(2 * p + 1, 2 * f) - Fraction(1, 2)
    assert R.taps_exact(2, R.CATMULL_ROM, 0)[1] == [Fraction(-3, 128), Fraction(29, 128), Fraction(111, 128), Fraction(-9, 128)]


@pytest.mark.parametrize("f", R.FACTORS)
def test_a_constant_plane_stays_constant(f):
    src = np.full((9, 9), f32(0.5))
    for filt in R.FILTERS:
        got = R.upsample(src, f, filt)
        assert got.shape == (9 * f, 9 * f) and got.dtype == f32
        assert (bits(got) == bits(f32(0.5))).all(), (f, filt)


@pytest.mark.parametrize("f", R.FACTORS)
def test_a_ramp_is_reproduced_at_the_cell_centres(f):
    # 0.25 x + 0.5 z + 3 on 16^2: linear, so bilinear and Catmull-Rom reproduce it exactly wherever no tap is clamped --
    # every fine cell at least 2 f cells from the border; all values are small dyadic rationals, so nothing rounds
    n = 16
    x = np.arange(n, dtype=f32)
    src = (f32(0.25) * x[None, :] + f32(0.5) * x[:, None] + f32(3)).astype(f32)
    j = np.arange(n * f)
    pos = ((2 * j + 1) / (2.0 * f) - 0.5)  # coarse coordinate of fine cell j: exact in double
    want = (0.25 * pos[None, :] + 0.5 * pos[:, None] + 3).astype(f32)
    assert (want.astype(np.float64) == 0.25 * pos[None, :] + 0.5 * pos[:, None] + 3).all()
    inner = slice(2 * f, n * f - 2 * f)
    for filt in (R.BILINEAR, R.CATMULL_ROM):
        got = R.upsample(src, f, filt)
        assert (bits(got[inner, inner]) == bits(want[inner, inner])).all(), (f, filt)
    near = R.upsample(src, f, R.NEAREST)
    assert (bits(near) == bits(np.repeat(np.repeat(src, f, 0), f, 1))).all()


@pytest.mark.parametrize("f", R.FACTORS)
def test_the_mean_of_small_integers_is_exact(f):
    rng = np.random.default_rng(f)
    src = rng.integers(-100, 100, (6 * f, 5 * f)).astype(f32)
    want = src.astype(np.float64).reshape(6, f, 5, f).sum(axis=(1, 3)) / (f * f)
    got = R.downsample(src, f)
    assert got.shape == (6, 5) and (got.astype(np.float64) == want).all()


@pytest.mark.parametrize("f", R.FACTORS)
def test_nearest_then_mean_is_the_identity_on_dyadic_inputs(f):
    rng = np.random.default_rng(10 + f)
    src = (rng.integers(-4096, 4096, (7, 7)) / 64.0).astype(f32)
    src[0, 0] = f32(-0.0)
    got = R.downsample(R.upsample(src, f, R.NEAREST), f)
    assert (bits(got) == bits(src)).all()


def test_signed_zero_nan_and_inf_follow_the_model():
    mz = np.full((4, 4), f32(-0.0))
    assert (bits(R.upsample(mz, 2, R.NEAREST)) == 0x80000000).all()      # nearest copies bits
    for filt in (R.BILINEAR, R.CATMULL_ROM):
        assert (bits(R.upsample(mz, 2, filt)) == 0).all()                  # a sum seeded with +0 never returns -0
    assert (bits(R.downsample(mz, 2)) == 0x80000000).all()               # the mean has no seed
    odd = np.zeros((4, 4), f32)
    odd.view(np.uint32)[1, 1] = 0xFFC12345
    assert bits(R.upsample(odd, 2, R.NEAREST))[2, 2] == 0xFFC12345
    assert bits(R.upsample(odd, 2, R.BILINEAR))[2, 2] == R.CANONICAL_NAN
    assert bits(R.upsample(odd, 2, R.NEAREST, base=np.zeros((8, 8), f32)))[2, 2] == R.CANONICAL_NAN
    inf = np.full((4, 4), f32(np.inf))
    assert (bits(R.upsample(inf, 4, R.CATMULL_ROM)) == R.CANONICAL_NAN).all()  # inf * negative weight + inf
    assert (R.upsample(inf, 4, R.BILINEAR) == np.inf).all()


@pytest.mark.parametrize("f", (2, 4))
def test_the_stripe_form_equals_the_monolithic_form(f):
    rng = np.random.default_rng(3)
    rows, cols = 40, 24
    src = rng.standard_normal((rows, cols)).astype(f32)
    base = rng.standard_normal((rows * f, cols * f)).astype(f32)
    for filt in R.FILTERS:
        halo = R.HALO[filt]
        for with_base in (False, True):
            mono = R.upsample_stripe(src, 0, rows, 0, rows * f, f, filt, base if with_base else None)
            for world in (1, 2, 3, 5):
                cuts = [rows * f * r // world for r in range(world + 1)]
                parts = []
                for g0, g1 in zip(cuts, cuts[1:]):
                    lo, hi = max(g0 // f - halo, 0), min((g1 - 1) // f + halo, rows - 1)
                    parts.append(R.upsample_stripe(src[lo:hi + 1], lo, rows, g0, g1, f, filt, base[g0:g1] if with_base else None))
                    if lo > 0 and filt != R.NEAREST:  # one ghost row too few is an error, not a clamp
                        with pytest.raises(ValueError):
                            R.upsample_stripe(src[lo + 1:hi + 1], lo + 1, rows, g0, g1, f, filt)
                assert (bits(np.concatenate(parts)) == bits(mono)).all(), (f, filt, world, with_base)
    fine = rng.standard_normal((rows * f, cols * f)).astype(f32)
    mono = R.downsample(fine, f)
    for world in (1, 2, 3, 5):
        cuts = [rows * r // world for r in range(world + 1)]
        parts = [R.downsample_stripe(fine[f * g0:f * g1], f * g0, g0, g1, f) for g0, g1 in zip(cuts, cuts[1:])]
        assert (bits(np.concatenate(parts)) == bits(mono)).all(), (f, world)
    with pytest.raises(ValueError):
        R.downsample_stripe(fine[1:], 1, 0, 2, f)


def test_the_hosts_carry_the_feature(nj):
    # the binding, the enum and the stages exist in all three hosts with the C ABI's values
    N = nj._native
    for name in ("nz_upsample", "nz_upsample_batch", "nz_downsample", "nz_downsample_batch", "nz_upsample_stripe",
                 "nz_downsample_stripe", "nz_upsample_stripe_halo_rows"):
        assert name in N.SIGNATURES, name
    assert [int(v) for v in nj.ResampleFilter] == [N.NZ_RESAMPLE_NEAREST, N.NZ_RESAMPLE_BILINEAR, N.NZ_RESAMPLE_CATMULL_ROM] == [0, 1, 2]
    assert [N.lib.nz_upsample_stripe_halo_rows(k) for k in (0, 1, 2)] == [R.HALO[k] for k in R.FILTERS]
    up, down = nj.UpsampleStage(None), nj.DownsampleStage(None)
    assert (up.factor, up.filter, up.base, down.factor) == (2, nj.ResampleFilter.CatmullRom, None, 2)
    assert nj.UpsampleStage(None, 4)._out_position(-3) == -12 and nj.DownsampleStage(None, 4)._out_position(-3) == -1
    header = open(os.path.join(ROOT, "include", "noize_hip.h")).read()
    assert re.search(r"enum nz_resample_filter \{ NZ_RESAMPLE_NEAREST = 0, NZ_RESAMPLE_BILINEAR = 1, NZ_RESAMPLE_CATMULL_ROM = 2 \}",
                     header)
    hpp = open(os.path.join(ROOT, "noize_job_amd", "host", "noize_pipeline.hpp")).read()
    cs = open(os.path.join(ROOT, "host-cs", "Stages", "Stages.cs")).read()
    for text in (hpp, cs):
        for cls in ("UpsampleStage", "DownsampleStage"):
            assert re.search(r"class %s\s*:" % cls, text), cls
        for entry in ("nz_upsample(", "nz_upsample_batch(", "nz_downsample(", "nz_downsample_batch("):
            assert entry in text, entry
    assert "enum class ResampleFilter { Nearest, Bilinear, CatmullRom }" in hpp
    assert "enum ResampleFilter { Nearest = 0, Bilinear = 1, CatmullRom = 2 }" in cs
    from noize_job_amd.sharded import HipStripeOps
    assert callable(HipStripeOps.upsample) and callable(HipStripeOps.downsample)
