"""Strict flow map with shared height differences and a one-sided K clamp: still the oracle's bits.

The streaming kernel (nz_flow_stream.hip) forms each difference of two adjacent totals once, in x through DPP and in z through
a register a stage keeps from one row to the next, and both fused kernels compute K = fminf(1, water / (sum * dt)) without the
reference's fmaxf(0, .) (nz_flow_common.hpp has the argument, tests/test_flow_shared_differences.py the float32 identities).

Every case runs in the tile kernel (the default at these sizes) and, with NZ_FLOW_STREAM=2, in the streaming kernel, each in a
fresh child process (tests/strict_valu_child.py, mode `flow`), and is compared with the CPU oracle on bit patterns.

Rows 70, 71, 72 with the streaming kernel's 16-row segments: a top segment (COND fill), interior segments with the phased fill
(rows 16 - 48), a last segment of 6, 7 and 8 rows, and a steady loop followed by one or two left-over steps.  Columns 100: one
strip with both borders in one wave; 131: two border strips; 254: three strips, the smallest grid with an interior strip --
the path that shares the west difference across lanes.  1 .. 5 iterations: the first runs the FIRST form only (its own
subtractions), the others mix both.

Planes: terraces (the terrain quantised to eight levels: ties everywhere, so every shared difference is +-0); the mixed plane
of test_gpu_strict_valu.py (flat block, -0 block, +-inf and NaN cells, on the borders too) with non-finite cells on both sides
of the strip seam at columns 107 / 108; -0 alone; the terrain times 1e30 (huge flux sums, K -> +0) and times 1e-30 with a flat
block (next to a water column of 1e-4 such heights vanish from the totals: every sum is 0 / 0), and times 1e-2 with the same
block (differences of ~1e-6: the water exceeds every sum and K clamps to 1, with 0 / 0 inside the block)."""
import json

import numpy as np
import pytest

import flow_ref as F
from test_gpu_strict_valu import child, flow_planes

pytestmark = pytest.mark.gpu
f32 = np.float32
ROWS, COLS = (70, 71, 72), (100, 131, 254)


def planes(rng, rows, cols):
    t = F.terrain(rng, rows, cols)
    lo, hi = float(t.min()), float(t.max())
    terraces = (np.floor((t - f32(lo)) / f32((hi - lo) / 8)).clip(0, 7) * f32((hi - lo) / 8) + f32(lo)).astype(f32)
    out = dict(flow_planes(rng, rows, cols))
    mixed = out["mixed"]
    if cols > 108:  # the seam between the first two strips of a five-iteration launch (108 stored columns per strip)
        mixed[12, 107], mixed[12, 108] = np.nan, np.inf
        mixed[40, 107], mixed[41, 108] = -np.inf, np.nan
        mixed[60, 107], mixed[60, 108] = f32(5e-4), f32(5e-4)
    out.update(terraces=terraces, huge=(t * f32(1e30)).astype(f32))
    for name, scale in (("tiny", 1e-30), ("small", 1e-2)):
        p = (t * f32(scale)).astype(f32)
        p[20:36, cols // 4:cols // 2] = p[20, cols // 4]
        out[name] = p
    return out


@pytest.fixture(scope="module")
def flow2_cases(oracle, tmp_path_factory):
    rng = np.random.default_rng(9009)
    arrays, meta = {}, []
    for rows, cols in zip(ROWS * 3, sorted(COLS * 3)):  # all nine pairs
        for name, h in planes(rng, rows, cols).items():
            key = "%s_%dx%d" % (name, rows, cols)
            arrays[key] = h
            meta.append({"key": key, "iterations": [1, 2, 3, 4, 5]})
            for n in range(1, 6):
                arrays["%s_%d" % (key, n)] = oracle.flowmap(h, n, *F.NORM)
    assert len({(arrays[m["key"]].shape) for m in meta}) == 9
    path = str(tmp_path_factory.mktemp("strict_valu_flow2") / "flow.npz")
    np.savez(path, meta=json.dumps(meta), **arrays)
    return path


@pytest.mark.parametrize("kernel", ["tile", "stream"])
def test_flow_kernels_equal_the_oracle_on_shared_difference_planes(nj, flow2_cases, kernel):
    child("flow", flow2_cases, **({"NZ_FLOW_STREAM": "2"} if kernel == "stream" else {}))
