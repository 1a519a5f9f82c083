"""CPU side of the octave shapes (billow, ridged multifractal; nz_fractal_shaped*): the reference driver is pinned to the
oracle's fBm, its per-octave arithmetic to hand-worked values, and the three hosts carry the new entries and classes."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fractal_shapes_ref import BILLOW, FBM, RIDGED, fractal_shaped, shape_octave

f32 = np.float32
ENTRIES = ("nz_fractal_shaped", "nz_fractal_shaped_batch", "nz_fractal_shaped_stripe")


@pytest.mark.parametrize("basis", range(8))
def test_driver_fbm_is_the_oracle_fractal(oracle, basis):
    args = (0.4, 1.0, 2.0, 0.0173, 6, -1234, -567, 97)  # hurst, amp, stepdown, detune, octaves, xpos, zpos, noiseSize
    want = oracle.fractal(basis, 33, 47, *args)
    got = fractal_shaped(basis, 33, 47, *args, shape=FBM)
    assert got.dtype == f32 and np.array_equal(got, want)
    rows = fractal_shaped(basis, 33, 47, *args, shape=FBM, row_ids=[0, 17, 32])
    assert np.array_equal(rows, want[[0, 17, 32]])


def test_billow_known_answers():
    one, a = f32(1.0), f32(0.5)
    t, w = shape_octave(BILLOW, f32(0.25), one, a, f32(0.5))  # |2 * 0.5 - 1| = 0
    assert t == f32(0.25) and w == one
    for v in (f32(0.0), f32(1.0)):  # |2v - 1| = 1
        t, w = shape_octave(BILLOW, f32(0.25), one, a, v)
        assert t == f32(0.75) and w == one
    t, _ = shape_octave(BILLOW, f32(0.0), one, one, f32(0.75))  # |1.5 - 1| = 0.5
    assert t == f32(0.5)


def test_ridged_known_answers():
    one, a = f32(1.0), f32(0.5)
    # v = 0.5: e = 0, r = (1 - 0)^2 * w = w; the weight becomes clamp(2 w)
    t, w = shape_octave(RIDGED, f32(0.0), one, a, f32(0.5))
    assert t == f32(0.5) and w == one  # 2 clamps to 1
    t, w = shape_octave(RIDGED, f32(0.0), f32(0.25), a, f32(0.5))
    assert t == f32(0.125) and w == f32(0.5)
    # v = 0 or 1: e = 1, r = 0, nothing added and the next octave's weight is 0
    for v in (f32(0.0), f32(1.0)):
        t, w = shape_octave(RIDGED, f32(0.3), one, a, v)
        assert t == f32(0.3) and w == f32(0.0)
    # a weight of 0 silences the next octave whatever its value
    t, w = shape_octave(RIDGED, f32(0.3), f32(0.0), a, f32(0.5))
    assert t == f32(0.3) and w == f32(0.0)
    # the clamp at 0: a negative gain
    t, w = shape_octave(RIDGED, f32(0.0), one, one, f32(0.5), offset=f32(1.0), gain=f32(-3.0))
    assert t == one and w == f32(0.0)
    # offset and gain: v = 0.75 -> e = 0.5, r = (1.5 - 0.5)^2 = 1, w = clamp(0.25) = 0.25
    t, w = shape_octave(RIDGED, f32(0.0), one, one, f32(0.75), offset=f32(1.5), gain=f32(0.25))
    assert t == one and w == f32(0.25)


def test_fbm_octave_is_the_plain_sum():
    t, w = shape_octave(FBM, f32(0.25), f32(0.125), f32(0.5), f32(0.75))
    assert t == f32(0.25) + f32(0.5) * f32(0.75) and w == f32(0.125)


def test_library_exports_the_shaped_entries(nj):
    lib = ctypes.CDLL(nj._native.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in nj._native.SIGNATURES, name
    # each takes its counterpart's arguments with (shape, ridgeOffset, ridgeGain) before `dep`
    sig = nj._native.SIGNATURES
    for name, base in zip(ENTRIES, ("nz_fractal", "nz_fractal_batch", "nz_fractal_stripe")):
        got, want = sig[name][1], sig[base][1]
        assert got[:-2] == want[:-2] + [ctypes.c_int32, ctypes.c_float, ctypes.c_float] and got[-2:] == want[-2:], name


def test_header_declares_the_shape_enum_and_entries():
    text = open(os.path.join(ROOT, "include", "noize_hip.h")).read()
    m = re.search(r"enum nz_fractal_shape\s*\{([^}]*)\}", text)
    assert m and [s.strip() for s in m.group(1).split(",")] == ["NZ_SHAPE_FBM = 0", "NZ_SHAPE_BILLOW = 1",
                                                                 "NZ_SHAPE_RIDGED = 2"]
    for name in ENTRIES:
        assert re.search(r"int32_t %s\(" % name, text), name


def test_python_host_has_the_shaped_stage(nj):
    assert [(s.name, int(s)) for s in nj.FractalShape] == [("Fbm", 0), ("Billow", 1), ("Ridged", 2)]
    assert issubclass(nj.ShapedNoiseStage, nj.NoiseStage) and nj.ShapedNoiseStage is not nj.NoiseStage
    st = nj.ShapedNoiseStage(None, nj.FractalNoise.Simplex, 0.4, 1.0, 13, 2.0, 0.0, 1700)
    assert (st.shape, st.ridgeOffset, st.ridgeGain) == (nj.FractalShape.Ridged, 1.0, 2.0)
    st = nj.ShapedNoiseStage(None, nj.FractalNoise.Perlin, shape=nj.FractalShape.Billow, ridgeOffset=0.9, ridgeGain=3.0)
    assert (st.noiseType, st.shape, st.ridgeOffset, st.ridgeGain) == (nj.FractalNoise.Perlin, nj.FractalShape.Billow, 0.9, 3.0)


def test_cpp_and_cs_hosts_have_the_shaped_stage():
    hpp = open(os.path.join(ROOT, "noize_job_amd", "host", "noize_pipeline.hpp")).read()
    cs = open(os.path.join(ROOT, "host-cs", "Stages", "Stages.cs")).read()
    assert "enum class FractalShape { Fbm, Billow, Ridged };" in hpp
    assert re.search(r"class ShapedNoiseStage\s*:\s*public NoiseStage", hpp)
    assert "nz_fractal_shaped_batch(" in hpp and "nz_fractal_shaped(" in hpp
    assert "public enum FractalShape { Fbm, Billow, Ridged }" in cs
    assert re.search(r"class ShapedNoiseStage\s*:\s*NoiseStage", cs)
    assert "Native.nz_fractal_shaped_batch(" in cs and "Native.nz_fractal_shaped(" in cs
    # the stock-list fast paths keep comparing the exact type (a ridged stage must never run there as fBm) ...
    assert "typeid(*n) != typeid(NoiseStage)" in hpp
    pipe_cs = open(os.path.join(ROOT, "host-cs", "Pipeline", "Pipeline.cs")).read()
    assert "stages[0].GetType() != typeof(NoiseStage)" in pipe_cs
    # ... while the retry rule (the first stage regenerates the tile) takes the subclass in all three hosts
    assert "dynamic_cast<NoiseStage *>(stage_instances[0]) != nullptr" in hpp
    assert "stage_instances[0] is NoiseStage" in pipe_cs
    py = open(os.path.join(ROOT, "noize_job_amd", "pipeline.py")).read()
    assert "isinstance(self.stage_instances[0], NoiseStage)" in py
