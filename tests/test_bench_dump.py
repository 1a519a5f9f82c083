"""bench.py --dump-outputs: which rows of a plane are written (no GPU needed)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_a_small_plane_is_written_whole():
    assert np.array_equal(bench.dump_rows(512, 512), np.arange(512))
    assert np.array_equal(bench.dump_rows(1024, 1024), np.arange(1024))


def test_a_large_plane_is_a_fixed_sample_within_the_budget():
    for rows, cols in ((4096, 4096), (16384, 16384), (8192, 16384)):
        r = bench.dump_rows(rows, cols)
        assert len(r) * cols * 4 <= bench.DUMP_MAX_BYTES < 64 * 10 ** 6
        assert np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < rows   # sorted, distinct, inside the plane
        assert np.array_equal(r, bench.dump_rows(rows, cols))           # the same rows on every run


def test_the_dump_files(tmp_path):
    rows = bench.dump_rows(4096, 4096)
    bench.write_dump(np, str(tmp_path / "d"), rows, np.ones((len(rows), 4096), np.float64))
    h, r = np.load(tmp_path / "d" / "height.npy"), np.load(tmp_path / "d" / "height_rows.npy")
    assert h.dtype == np.float32 and h.shape == (len(rows), 4096)
    assert r.dtype == np.float64 and np.array_equal(r, rows)
