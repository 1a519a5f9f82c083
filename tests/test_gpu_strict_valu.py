"""Strict mode's instruction savings leave every bit where it was.

Three kernels drop VALU work their results do not need, in NZ_FLOAT_STRICT only:

  * the 5-tap register-tile filter forms each product of a mirror-symmetric table once (conv_tile<SYM>, nz_filter.hip) and
    multiplies the neighbour lanes' values through DPP; NZ_CONV_SYM=0 forces the generic form;
  * the flow map no longer adds +0 to its fluxes (flux_sum / update_water_m, nz_flow_common.hpp);
  * the simplex fBm reads the octaves' frequencies and amplitudes from a host-built table of up to 16 octaves
    (nz_octave_table) instead of running the wave-uniform recurrence.

Everything is compared with the CPU oracle on bit patterns (`view(uint32)`): zero signs are the point.  The knobs are read
once per process, so the filter and flow cases run in fresh child processes (tests/strict_valu_child.py); the inputs and
the oracle's planes are computed once per module and handed to every child in one file.

Filter grids are the smallest that select each launch form: 300^2 is TINY (1024 x 2 rows), 776^2 SMALL (512 x 4, > 600 K
cells), 352^2 with NZ_CONV_SMALL=0 the metric's BIG tile (512 x 8: one interior tile, edge tiles on all sides).  1, 4 and 5
applications are one launch everywhere; 9 and 17 are several launches -- chained by default on the small grids and from three
launches on BIG, separate under NZ_CONV_CHAIN=0, chained from two under NZ_CONV_CHAIN=2."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_ref as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
KNOBS = ("NZ_CONV_SYM", "NZ_CONV_SMALL", "NZ_CONV_CHAIN", "NZ_CONV_STREAM", "NZ_FLOW_STREAM", "NZ_FLOW_TINY", "NZ_FLOW_NMAX")
GAUSS5_S1, GAUSS5_S2 = 2, 6
APPLICATIONS = (1, 4, 5, 9, 17)


def child(*args, **knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    run = subprocess.run([sys.executable, "-s", os.path.join(HERE, "strict_valu_child.py"), *args], env=env,
                         capture_output=True, text=True, timeout=240)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), (run.stdout + run.stderr)[-3000:]


def signed(rng, shape):
    return ((rng.random(shape, dtype=f32) - f32(0.3)) * f32(8)).astype(f32)


def neg_zero_with_denormals(rng, res):
    """-0 everywhere, one cell in ~200 a denormal of either sign: products that underflow to +-0 beside true zeros"""
    t = np.full((res, res), -0.0, f32)
    n = res * res // 200
    idx = rng.choice(res * res, n, replace=False)
    t.reshape(-1)[idx] = (rng.integers(1, 1 << 20, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(f32)
    return t


# ---- filter ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conv_cases(oracle, tmp_path_factory):
    rng = np.random.default_rng(5005)
    arrays, meta = {}, []
    for group, res, wcols in (("small", 300, 131), ("small", 776, 779), ("big", 352, 131)):
        planes = {"slab": signed(rng, (res, res)),           # carved 4 bytes past a 16-byte boundary: the 4-byte accesses
                  "window": signed(rng, (res, wcols)),       # odd width at an aligned pitch: rows that are no whole groups
                  "stage": neg_zero_with_denormals(rng, res)}
        for kind, t in planes.items():
            key = "%s%d" % (kind, res)
            arrays[key] = t
            meta.append({"group": group, "key": key, "kind": kind, "filters": [GAUSS5_S1, GAUSS5_S2],
                         "iterations": list(APPLICATIONS)})
            for ft in (GAUSS5_S1, GAUSS5_S2):
                for it in APPLICATIONS:
                    arrays["%s_%d_%d" % (key, ft, it)] = oracle.kernel_filter(t, ft, it)
    path = str(tmp_path_factory.mktemp("strict_valu") / "conv.npz")
    np.savez(path, meta=json.dumps(meta), **arrays)
    return path


CONV_ENVS = {"small-default": ("small", {}),
             "small-separate": ("small", {"NZ_CONV_CHAIN": "0"}),
             "big-default": ("big", {"NZ_CONV_SMALL": "0"}),
             "big-chain2": ("big", {"NZ_CONV_SMALL": "0", "NZ_CONV_CHAIN": "2"})}


@pytest.mark.parametrize("sym", ["sym", "generic"])
@pytest.mark.parametrize("env", list(CONV_ENVS))
def test_gauss5_launch_forms_equal_the_oracle(nj, conv_cases, env, sym):
    group, knobs = CONV_ENVS[env]
    if sym == "generic":
        knobs = dict(knobs, NZ_CONV_SYM="0")
    child("conv", conv_cases, group, **knobs)


# ---- flow -----------------------------------------------------------------------------------------------------------
def flow_planes(rng, rows, cols):
    """terrain with a flat block (every flux sum 0 inside it), a block of -0, +-inf and NaN cells; and a plane of -0 alone"""
    h = F.terrain(rng, rows, cols)
    h[8:24, cols // 5:cols // 2] = f32(2e-4)
    h[30:44, cols // 2:cols - 3] = f32(-0.0)
    h[3, 2], h[rows // 2, cols - 1], h[rows - 2, cols // 3] = np.inf, -np.inf, np.nan
    h[rows - 1, 0], h[0, cols - 2], h[50, cols // 2] = np.nan, np.inf, -np.inf
    return {"mixed": h, "negzero": np.full((rows, cols), -0.0, f32)}


@pytest.fixture(scope="module")
def flow_cases(oracle, tmp_path_factory):
    rng = np.random.default_rng(7007)
    arrays, meta = {}, []
    for cols in (100, 254):   # one strip of the streaming kernel; three strips
        for name, h in flow_planes(rng, 70, cols).items():
            key = "%s%d" % (name, cols)
            arrays[key] = h
            meta.append({"key": key, "iterations": [1, 2, 3, 4, 5]})
            for n in range(1, 6):
                arrays["%s_%d" % (key, n)] = oracle.flowmap(h, n, *F.NORM)
    path = str(tmp_path_factory.mktemp("strict_valu") / "flow.npz")
    np.savez(path, meta=json.dumps(meta), **arrays)
    return path


@pytest.mark.parametrize("kernel", ["tile", "stream"])
def test_flow_kernels_equal_the_oracle(nj, flow_cases, kernel):
    child("flow", flow_cases, **({"NZ_FLOW_STREAM": "2"} if kernel == "stream" else {}))


# ---- fBm ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("detune", [0.0, 0.013])
@pytest.mark.parametrize("octaves", [13, 16, 17])   # 13, 16: the octave table; 17: the in-kernel recurrence
def test_simplex_fbm_octave_table(nj, ctx, oracle, octaves, detune):
    import ctypes as C
    simplex = int(nj.FractalNoise.Simplex)
    for rows, cols in ((70, 64), (5, 513)):
        args = (0.4, 1.0, 2.0, detune, octaves, 37, -11, 1700)
        want = oracle.fractal(oracle.SIMPLEX, rows, cols, *args)
        d = ctx.from_host(np.full(rows * cols, np.nan, f32))
        st = nj.Stripe(cols, rows, 0, rows, 0, rows, cols)
        ctx.call("nz_fractal_stripe", simplex, d.ptr, C.byref(st), *args).Complete()
        got = d.ToArray((rows, cols))
        d.Dispose()
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), "%d octaves detune %g %dx%d: %d cells differ, first at %s" % (
            octaves, detune, rows, cols, int(bad.sum()), tuple(np.argwhere(bad)[0]))
