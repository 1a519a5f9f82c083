"""CPU checks of grid hydraulic erosion: the reference driver of tests/hydraulic_ref.py (capacity 0 is the flow map's
state, the sum of the heights is conserved, the defaults stay finite) and the C ABI of the stage (exported, bound in
Python, and declared in the generated C# binding)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hydraulic_ref as H
import oracle as O
from conftest import ROOT

f32 = np.float32
ENTRIES = ("nz_hydraulic_erosion_work_floats", "nz_hydraulic_erosion_stage", "nz_hydraulic_erosion_stage_rw",
           "nz_hydraulic_erosion_stage_batch")
# (initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt)
PARAMS = [(1e-4, 1e-4, 0.01, 1.0, 0.3, 0.3, 0.01),
          (1e-3, 5e-4, 0.05, 4.0, 0.5, 0.1, 0.0),
          (0.0, 2e-4, 0.0, 0.5, 1.0, 1.0, 0.05)]
NAMES = ("initialWater", "rain", "evaporation", "capacity", "dissolve", "deposit", "minTilt")


def relief(res, noise_size=300):
    """A smoothed simplex fBm tile (the quickstart's kind of terrain)."""
    h = O.fractal(O.SIMPLEX, res, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, noise_size)
    return O.kernel_filter(h, O.GAUSS5_S1, 4)


def test_capacity_zero_is_the_flow_map():
    h = relief(48)
    its = 12
    b, d, s, flux = H.run(h, its, initialWater=1e-4, rain=0.0, evaporation=0.0, capacity=0.0, state=True)
    assert np.array_equal(b, h) and not s.any()
    w = np.full(h.shape, f32(1e-4), f32)
    fl = tuple(np.zeros(h.shape, f32) for _ in range(4))
    for _ in range(its):
        fl = O.flow_step(h, w, *fl)
        w = O.water_step(w, *fl)
    assert np.array_equal(d, w)
    for got, want in zip(flux, fl):
        assert np.array_equal(got, want)
    res, water = H.run(h, its, initialWater=1e-4, rain=0.0, evaporation=0.0, capacity=0.0)
    assert np.array_equal(res, h) and np.array_equal(water, w)


@pytest.mark.parametrize("prm", PARAMS, ids=["defaults", "strong", "dry-start"])
def test_sum_is_conserved(prm):
    h = relief(64)
    kw = dict(zip(NAMES, prm))
    res, water = H.run(h, 150, **kw)
    assert np.isfinite(res).all() and (water >= 0).all()
    assert not np.array_equal(res, h)  # it does erode
    s0, s1 = h.astype(np.float64).sum(), res.astype(np.float64).sum()
    assert abs(s1 - s0) <= 1e-6 * np.abs(h.astype(np.float64)).sum(), (s0, s1)


def test_defaults_stay_finite():
    h = relief(64)
    res, water = H.run(h, 2000)
    assert np.isfinite(res).all() and np.isfinite(water).all()
    assert np.abs(res - h).max() < 1.0


def test_zero_iterations_is_the_input():
    h = relief(16)
    res, water = H.run(h, 0)
    assert np.array_equal(res, h) and (water == f32(1e-4)).all()


def test_the_abi_exports_and_binds_the_stage(nj):
    lib = ctypes.CDLL(nj._native.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in nj._native.SIGNATURES, name
    assert nj._native.lib.nz_hydraulic_erosion_work_floats(64, 3) == 14 * 64 * 64 * 3
    assert nj._native.lib.nz_hydraulic_erosion_work_floats(0, 1) == 0
    cs = open(os.path.join(ROOT, "host-cs", "Native.cs")).read()
    for name in ENTRIES:
        assert " %s(" % name in cs, name
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, gen.stdout + gen.stderr


def test_every_host_has_the_stage(nj):
    assert "HydraulicErosionStage" in nj.__all__
    hpp = open(os.path.join(ROOT, "noize_job_amd", "host", "noize_pipeline.hpp")).read()
    cs = open(os.path.join(ROOT, "host-cs", "Stages", "Stages.cs")).read()
    assert "class HydraulicErosionStage : public PipelineStage" in hpp
    assert "class HydraulicErosionStage : PipelineStage" in cs
    for entry in ("nz_hydraulic_erosion_stage(", "nz_hydraulic_erosion_stage_rw(", "nz_hydraulic_erosion_stage_batch("):
        assert entry in hpp and "Native." + entry in cs, entry
