"""Edge tiles of the register-tile filter kernels form their row-clamp masks in every application (conv_tile, nz_filter.hip:
the comparisons run against copies of the clamp rows the compiler cannot hoist out of the application loop).  The masks decide
which window rows of a thread are replaced by the grid's first / last row, so grids SHORTER than the windows are where a wrong
mask shows: 5 rows (both clamps inside every thread's Z window, whatever the rows per thread), 12 rows (both inside one 8-row
block's window), 40 rows (one tile row, the clamps in different blocks), each 300 columns wide as a window of two NaN planes
with rows one float past a 16-byte multiple apart.  Every tap count (3, 5, 7, 9) and every tile shape: the small grids' shapes by
default, the 128-row tiles under NZ_CONV_SMALL=0, the generic 5-tap form under NZ_CONV_SYM=0.  1 and 4 applications are one
launch; 9 are several, chained on small grids.

All comparisons are bit for bit against the CPU oracle.  The knobs are read once per process: each environment is one child
process (tests/strict_valu_child.py) reading the same file of inputs and expected planes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
KNOBS = ("NZ_CONV_SYM", "NZ_CONV_SMALL", "NZ_CONV_CHAIN", "NZ_CONV_STREAM")
FILTERS = (0, 1, 2, 3)  # Gauss9_S1, Gauss7_S1, Gauss5_S1, Gauss3_S1
APPLICATIONS = (1, 4, 9)


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    rng = np.random.default_rng(4242)
    arrays, meta = {}, []
    for rows in (5, 12, 40):
        t = ((rng.random((rows, 300), dtype=f32) - f32(0.3)) * f32(8)).astype(f32)
        t[0], t[-1] = t[0] * f32(1e4), t[-1] * f32(-1e-4)  # the rows the clamps repeat: unlike their neighbours in scale and sign
        key = "rows%d" % rows
        arrays[key] = t
        meta.append({"group": "short", "key": key, "kind": "window", "filters": list(FILTERS), "iterations": list(APPLICATIONS)})
        for ft in FILTERS:
            for it in APPLICATIONS:
                arrays["%s_%d_%d" % (key, ft, it)] = oracle.kernel_filter(t, ft, it)
    path = str(tmp_path_factory.mktemp("conv_row_clamps") / "cases.npz")
    np.savez(path, meta=json.dumps(meta), **arrays)
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"NZ_CONV_SMALL": "0"}, {"NZ_CONV_SMALL": "0", "NZ_CONV_SYM": "0"},
                                 {"NZ_CONV_SMALL": "0", "NZ_CONV_CHAIN": "2"}],
                         ids=["small-shapes", "big-tiles", "big-tiles-generic", "big-tiles-chained"])
def test_short_grids_equal_the_oracle(nj, cases, env):
    knobs = {k: v for k, v in os.environ.items() if k not in KNOBS}
    knobs.update(env)
    run = subprocess.run([sys.executable, "-s", os.path.join(HERE, "strict_valu_child.py"), "conv", cases, "short"], env=knobs,
                         capture_output=True, text=True, timeout=240)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), (run.stdout + run.stderr)[-3000:]
