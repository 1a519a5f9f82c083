"""The chained filter grid behind its host-built tile plan (nz_chain_plan.hpp, the plan cache of the context, the 16-byte
accesses of edge tiles): bit for bit against the CPU oracle.

Every environment runs tests/chain_plan_child.py in a fresh process with its own time limit, because the knobs are read
once per process.  The grids are the smallest that take each path of the 512 x 8 tile: 352 x 352 has one fully interior
tile and edge tiles on all four sides, 360 rows x 1000 columns has 36 tiles per launch and uneven class counts, 263 x 301
is unaligned (4-byte accesses), 352 rows x 350 columns at pitch 352 is aligned without whole column groups (4-byte again),
350 x 352 at pitch 356 takes the 16-byte edge path with a pitch beyond the row.  Every window lies in planes that are NaN
elsewhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("NZ_CONV_SMALL", "NZ_CONV_CHAIN", "NZ_CONV_STREAM")


def child(case, *args, **knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    run = subprocess.run([sys.executable, "-s", os.path.join(HERE, "chain_plan_child.py"), case, *args], env=env,
                         capture_output=True, text=True, timeout=180)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), (run.stdout + run.stderr)[-3000:]


def test_metric_tile_on_edge_shapes(nj):
    child("metric", NZ_CONV_SMALL="0", NZ_CONV_CHAIN="2")


def test_small_tiles_with_default_knobs(nj):
    child("default")


def test_fast_mode_chained_equals_separate_launches(nj, tmp_path):
    a, b = str(tmp_path / "chained.npy"), str(tmp_path / "separate.npy")
    child("fast", a, NZ_CONV_SMALL="0", NZ_CONV_CHAIN="2")
    child("fast", b, NZ_CONV_SMALL="0", NZ_CONV_CHAIN="0")
    a, b = np.load(a), np.load(b)
    assert a.shape == b.shape and np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%d cells differ" % int((a.view(np.uint32) != b.view(np.uint32)).sum())


def test_plan_cache(nj):
    child("cache")


def test_nan_framed_window(nj):
    child("nan_window", NZ_CONV_SMALL="0", NZ_CONV_CHAIN="2")
