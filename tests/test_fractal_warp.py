"""CPU side of the domain warp (nz_fractal_warped*, WarpedNoiseStage): the reference driver reduces to the shaped driver
without a warp, its displacement is the oracle's fBm, its coordinate step is pinned to hand-worked values, and the three
hosts carry the new entries and classes."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fractal_shapes_ref import BILLOW, FBM, RIDGED, _libm, fractal_shaped
from fractal_warp_ref import displacement, fractal_warped, warp_coordinate

f32 = np.float32
ENTRIES = ("nz_fractal_warped", "nz_fractal_warped_batch", "nz_fractal_warped_stripe")
ARGS = (0.4, 1.0, 2.0, 0.0173, 5, -1234, -567, 97)  # hurst, amp, stepdown, detune, octaves, xpos, zpos, noiseSize


@pytest.mark.parametrize("basis", range(8))
def test_no_warp_is_the_shaped_driver(oracle, basis):
    for shape in (FBM, BILLOW, RIDGED):
        want = fractal_shaped(basis, 9, 13, *ARGS, shape=shape)
        for strength, octv in ((0.0, 3), (37.5, 0)):
            got = fractal_warped(basis, 9, 13, *ARGS, shape=shape, warp_strength=strength, warp_scale=0.25,
                                 warp_octaves=octv)
            assert got.dtype == f32 and np.array_equal(got, want), (basis, shape, strength, octv)


@pytest.mark.parametrize("basis", range(8))
def test_displacement_is_the_oracle_fractal(oracle, basis):
    hurst, amp, step, det, _, xp, zp, ns = ARGS
    want = oracle.fractal(basis, 11, 17, hurst, amp, step, det, 3, xp, zp, ns)
    qx, _ = displacement(basis, 11, 17, hurst, amp, step, det, xp, zp, ns, warp_scale=1.0, warp_octaves=3)
    assert qx.dtype == f32 and np.array_equal(qx, want)
    rows, _ = displacement(basis, 11, 17, hurst, amp, step, det, xp, zp, ns, warp_scale=1.0, warp_octaves=3,
                           row_ids=[0, 6, 10])
    assert np.array_equal(rows, want[[0, 6, 10]])


def test_warp_coordinate_known_answers():
    X = f32(1234.0)
    assert warp_coordinate(X, 0.75, 8.0) == X + f32(4.0)  # (2 * 0.75 - 1) * 8 = 4
    assert warp_coordinate(X, 0.5, 8.0) == X  # the midpoint does not move
    assert warp_coordinate(X, 0.5, -200.0) == X
    assert warp_coordinate(X, 0.0, 8.0) == X - f32(8.0) and warp_coordinate(X, 1.0, 8.0) == X + f32(8.0)
    assert warp_coordinate(X, 0.25, -200.0) == X + f32(100.0)  # a negative strength moves the other way
    assert warp_coordinate(f32(-3.0), 0.75, 2.0) == f32(-2.0)


def test_warp_moves_the_plane():
    got = fractal_warped(3, 7, 9, *ARGS, warp_strength=37.5, warp_scale=0.25, warp_octaves=2)
    plain = fractal_shaped(3, 7, 9, *ARGS)
    assert np.isfinite(got).all() and not np.array_equal(got, plain)


def test_second_displacement_uses_the_offsets(oracle):
    # qz is D at (u + 5.2, v + 1.3): at warpScale 1 and noiseSize 1 that is the oracle fBm of the tile shifted by (5.2, 1.3)
    hurst, amp, step, det = 0.5, 1.0, 2.0, 0.0
    _, qz = displacement(3, 1, 1, hurst, amp, step, det, 10, 20, 1, warp_scale=1.0, warp_octaves=2)
    want = oracle.fractal_norm(hurst, 2)
    v = [oracle.noise_value(3, float(f32(10.0) + f32(5.2)), float(f32(20.0) + f32(1.3))),
         oracle.noise_value(3, float(f32(2.0) * (f32(10.0) + f32(5.2))), float(f32(2.0) * (f32(20.0) + f32(1.3))))]
    t = f32(0.0) + f32(1.0) * f32(v[0])
    t = t + f32(_libm.exp2f(f32(-0.5))) * f32(v[1])
    assert qz[0, 0] == t / f32(want)


def test_library_exports_the_warped_entries(nj):
    lib = ctypes.CDLL(nj._native.LIB_PATH)
    sig = nj._native.SIGNATURES
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in sig, name
    # each takes its shaped counterpart's arguments with (warpStrength, warpScale, warpOctaves) before `dep`
    for name, base in zip(ENTRIES, ("nz_fractal_shaped", "nz_fractal_shaped_batch", "nz_fractal_shaped_stripe")):
        got, want = sig[name][1], sig[base][1]
        assert got[:-2] == want[:-2] + [ctypes.c_float, ctypes.c_float, ctypes.c_int32] and got[-2:] == want[-2:], name


def test_header_declares_the_warped_entries():
    text = open(os.path.join(ROOT, "include", "noize_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"int32_t %s\(([^;]*)\);" % name, text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert params[-6:] == ["float ridgeGain", "float warpStrength", "float warpScale", "int32_t warpOctaves",
                               "nz_handle dep", "nz_handle *out"], (name, params)


def test_python_host_has_the_warped_stage(nj):
    assert issubclass(nj.WarpedNoiseStage, nj.ShapedNoiseStage) and issubclass(nj.WarpedNoiseStage, nj.NoiseStage)
    st = nj.WarpedNoiseStage(None, nj.FractalNoise.Simplex, 0.4, 1.0, 13, 2.0, 0.0, 1700)
    assert st.shape == nj.FractalShape.Fbm
    assert (st.warpStrength, st.warpScale, st.warpOctaves) == (0.0, 1.0, 4)
    st = nj.WarpedNoiseStage(None, nj.FractalNoise.Perlin, shape=nj.FractalShape.Ridged, warpStrength=-200.0,
                             warpScale=0.25, warpOctaves=2)
    assert (st.noiseType, st.shape, st.warpStrength, st.warpScale, st.warpOctaves) == (
        nj.FractalNoise.Perlin, nj.FractalShape.Ridged, -200.0, 0.25, 2)


def test_cpp_and_cs_hosts_have_the_warped_stage():
    hpp = open(os.path.join(ROOT, "noize_job_amd", "host", "noize_pipeline.hpp")).read()
    cs = open(os.path.join(ROOT, "host-cs", "Stages", "Stages.cs")).read()
    native = open(os.path.join(ROOT, "host-cs", "Native.cs")).read()
    assert re.search(r"class WarpedNoiseStage\s*:\s*public ShapedNoiseStage", hpp)
    assert "nz_fractal_warped_batch(" in hpp and "nz_fractal_warped(" in hpp
    assert re.search(r"class WarpedNoiseStage\s*:\s*ShapedNoiseStage", cs)
    assert "Native.nz_fractal_warped(" in cs and "Native.nz_fractal_warped_batch(" in cs
    for name in ENTRIES:
        assert "static extern int %s(" % name in native, name
    # the stock-list fast paths still compare the exact type and the retry rule still takes any NoiseStage
    assert "typeid(*n) != typeid(NoiseStage)" in hpp
    assert "dynamic_cast<NoiseStage *>(stage_instances[0]) != nullptr" in hpp
    pipe_cs = open(os.path.join(ROOT, "host-cs", "Pipeline", "Pipeline.cs")).read()
    assert "stages[0].GetType() != typeof(NoiseStage)" in pipe_cs and "stage_instances[0] is NoiseStage" in pipe_cs
