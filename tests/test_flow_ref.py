"""tests/flow_ref.py against the oracle's whole stage (CPU): launches chained over any split of the iterations, and a
stripe's owned rows from 2n ghost rows, reproduce oracle.flowmap bit for bit."""
import numpy as np
import pytest

import flow_ref as F
import terrain_tiles as T

f32 = np.float32
ROWS, COLS = 67, 45


def _grid():
    """A relief with everything below the 0.3 quantile raised to it: sea-level plateaus, equal neighbours, zero slopes."""
    h = T.relief(ROWS, np.random.default_rng(67))[:, :COLS]
    return np.ascontiguousarray(np.maximum(h, f32(T.sea_at(h))), f32)


def _splits(total, rng):
    out = {tuple(F.split_iterations(total, cap)) for cap in range(1, 6)}
    for _ in range(6):  # random compositions of `total`
        cuts = np.flatnonzero(rng.random(total - 1) < 0.4) + 1 if total > 1 else np.array([], int)
        out.add(tuple(int(v) for v in np.diff(np.concatenate([[0], cuts, [total]]))))
    return sorted(out)


def test_split_iterations_is_the_librarys_rule():
    assert F.split_iterations(5, 5) == [5] and F.split_iterations(6, 5) == [3, 3] and F.split_iterations(7, 5) == [4, 3]
    assert F.split_iterations(11, 5) == [4, 4, 3] and F.split_iterations(12, 5) == [4, 4, 4] and F.split_iterations(12, 1) == [1] * 12


@pytest.mark.parametrize("total", range(1, 13))
def test_chained_launches_reproduce_the_stage(oracle, total):
    h = _grid()
    assert (h == h.min()).mean() > 0.2  # the plateaus are there
    want = oracle.flowmap(h, total, *F.NORM)
    for split in _splits(total, np.random.default_rng(total)):
        assert sum(split) == total
        got, states = F.chain(h, split)
        F.assert_bits_equal(got, want, "split %s" % (split,))
        assert states[0] is None and len(states) == len(split)


@pytest.mark.parametrize("n", range(1, 6))
def test_a_stripe_from_its_ghost_rows_equals_the_whole_grid(oracle, n):
    h = _grid()
    mid = F.launch(h, 3, True, False)  # a state for the launches that read one
    for first, last in ((1, 1), (1, 0), (0, 1), (0, 0)):
        whole = F.launch(h, n, first, last, None if first else mid)
        for g0, g1 in ((0, 9), (0, 30), (21, 40), (25, 26), (50, ROWS), (0, ROWS)):
            part = F.stripe_launch(h, g0, g1, n, first, last, None if first else mid)
            if last:
                F.assert_bits_equal(part, whole[g0:g1], "n=%d last rows %d..%d" % (n, g0, g1))
            else:
                for k in range(5):
                    F.assert_bits_equal(part[k], whole[k][g0:g1], "n=%d plane %d rows %d..%d" % (n, k, g0, g1))
    # one ghost row fewer is not enough.  Only n = 1 shows it on this relief: a wrong row reaches the owned rows through one
    # further step per row, each scaled by the water's share of the total height (1e-4), and is rounded away after two
    if n == 1:
        short = F.launch(h[20:41], 1, True, True)[1:20]
        assert not np.array_equal(short, F.launch(h, 1, True, True)[21:40])
