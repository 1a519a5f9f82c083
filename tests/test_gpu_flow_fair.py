"""The fair share of a SIMD between the two waves of the row-streaming flow kernel (fs_fair_prio, nz_flow_stream.hip): at
the top of every step of the fill and drain loops and of every three-step trip a wave reads the 100 MHz clock and its wave
slot and sets its priority from them, which must change no value.

NZ_FLOW_STREAM and NZ_FLOW_FAIR are read once per process, so tests/flow_fair_child.py runs in a fresh process with its own
time limit, once with NZ_FLOW_STREAM=2 NZ_FLOW_FAIR=2 (the code runs wherever the kernel has it: n = 4 and 5) and once with
NZ_FLOW_FAIR=0, one after the other.  Each child runs flow_fair_child.CASES -- the smallest shapes that take the clock read
and the s_setprio through every loop they sit in: the pipeline fill, the three-step trips, the leftover steps and the drain,
in segments on and away from the grid's first and last rows and in border and inner strips; none has more than 217 x 97
cells -- in all three float modes and writes its planes.  Here:

  * NZ_FLOAT_STRICT and NZ_FLOAT_FAST: both children's planes have the bit patterns of the oracle (tests/flow_ref.py's
    comparison: the sign of a zero counts, a NaN matches a NaN);
  * NZ_FLOAT_RELAXED: the two children's planes are bit-equal to each other;
  * nothing outside a plane's cells was written: the pads and the rows around a slab-carved plane are still NaN.

One more case runs the default rule (NZ_FLOW_FAIR unset) in this process: the smallest launch of 4096 columns that streams
by the form query at n = 5, one round of waves, against the oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_fair_child as K
import flow_ref as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
KNOBS = ("NZ_FLOW_STREAM", "NZ_FLOW_FAIR", "NZ_FLOW_TINY", "NZ_FLOW_NMAX")
STREAM_CELLS = 8 * 1024 * 1024


def child(out, **knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    run = subprocess.run([sys.executable, "-s", os.path.join(HERE, "flow_fair_child.py"), out], env=env,
                         capture_output=True, text=True, timeout=180)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), (run.stdout + run.stderr)[-3000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def children(nj, tmp_path_factory):
    d = tmp_path_factory.mktemp("flow_fair")
    fair = child(str(d / "fair.npz"), NZ_FLOW_STREAM="2", NZ_FLOW_FAIR="2")
    plain = child(str(d / "plain.npz"), NZ_FLOW_STREAM="2", NZ_FLOW_FAIR="0")
    return {"fair": fair, "plain": plain}


@pytest.fixture(scope="module")
def wants(oracle):
    """case id -> the oracle's planes (count, rows, cols), computed once"""
    out = {}
    for case in K.CASES:
        kind, n, rows, cols, count, pad = case
        h = K.inputs(case)
        w = np.stack([oracle.flowmap(t, n, *F.NORM) for t in h])
        out[K.case_id(case)] = w[:, 2 * n:2 * n + rows] if kind == "slab" else w
    return out


def cells(case, buf):
    """The planes' cells (count, rows, cols) of what a child wrote; everything around them must still be NaN."""
    kind, n, rows, cols, count, pad = case
    if kind == "batch":
        return buf
    own0 = K.ABOVE + 2 * n if kind == "slab" else 0
    assert np.isnan(buf[:own0]).all() and np.isnan(buf[own0 + rows:]).all() and np.isnan(buf[:, cols:]).all(), \
        "%s: written outside the owned rows x cols" % K.case_id(case)
    return buf[None, own0:own0 + rows, :cols]


def test_the_cases_are_small():
    ids = [K.case_id(c) for c in K.CASES]
    assert len(set(ids)) == len(ids)
    assert all(rows * cols <= 217 * 97 for _, _, rows, cols, _, _ in K.CASES)
    assert {c[1] for c in K.CASES} == {4, 5} and {c[4] for c in K.CASES} == {1, 2} and any(c[5] == 3 for c in K.CASES)


@pytest.mark.parametrize("which", ["fair", "plain"])
@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_oracle_bits(children, wants, which, mode):
    got = children[which]
    assert len(got) == 3 * len(K.CASES)
    for case in K.CASES:
        cid = K.case_id(case)
        g = cells(case, got["%s/%s" % (mode, cid)])
        assert np.isfinite(g).all(), "%s %s [%s]: non-finite cells" % (which, cid, mode)
        F.assert_bits_equal(g, wants[cid], "%s %s [%s]" % (which, cid, mode))


def test_relaxed_bits_do_not_depend_on_the_priority(children, wants):
    for case in K.CASES:
        cid = K.case_id(case)
        a, b = (cells(case, children[w]["relaxed/" + cid]) for w in ("fair", "plain"))
        assert np.isfinite(a).all(), cid
        F.assert_bits_equal(a, b, "%s [relaxed] fair against plain" % cid)
        # ... and these are the mode's values: the band tests/test_gpu_fast.py grants it against the strict oracle
        w = wants[cid].astype(np.float64)
        d = np.abs(a.astype(np.float64) - w)
        bad = int((d > 1e-5 * np.abs(w) + 1e-6).sum())
        assert bad <= max(8, 0.02 * w.size) and d.max() < 1e-3, "%s [relaxed]: %d of %d cells outside the band" % (cid, bad, w.size)


def test_default_rule_one_round_of_4096_columns(nj, oracle):
    """NZ_FLOW_FAIR as the environment has it (unset: the rule): 4096 columns x the fewest rows that stream at n = 5 is one
    round of resident waves, so the launch runs with the fair share on."""
    cols, lib = 4096, nj._native.lib
    n = min(5, lib.nz_flow_fused_max_iterations())   # NZ_FLOW_NMAX: the entry fuses no more
    knobs = any(os.environ.get(k) for k in KNOBS)
    with nj.Context(0) as ctx:
        def form(rows):
            return lib.nz_flow_launch_form(ctx._h, cols, rows, 1, n, 1, 1)
        lo, hi = 1, (1 << 24) // cols + 1
        if form(hi) == K.STREAM:
            while lo < hi:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if form(mid) == K.STREAM else (mid + 1, hi)
        else:   # a knob rules the streaming kernel out: the same grid, whatever form it takes
            lo = STREAM_CELLS // cols
        rows = lo
        if not knobs:
            assert rows == STREAM_CELLS // cols and form(rows) == K.STREAM and form(rows - 1) != K.STREAM
    h = F.terrain(np.random.default_rng(4096), rows, cols)
    want = oracle.flowmap(h, n, *F.NORM)
    nan = np.full(h.shape, np.nan, f32)
    for mode, name in K.MODES.items():
        with nj.Context(0) as ctx:
            ctx.float_mode = mode
            src, dst = ctx.from_host(h), ctx.from_host(nan)
            st = nj.Stripe(cols, rows, 0, rows, 0, rows, cols)
            ctx.call("nz_flow_fused_stripe", src.ptr, None, None, dst.ptr, C.byref(st), n, 1, 1, *F.NORM, handle=False)
            ctx.synchronize()
            got = dst.ToArray(h.shape)
            src.Dispose()
            dst.Dispose()
        if mode < 2:
            F.assert_bits_equal(got, want, "4096 x %d x%d [%s]" % (rows, n, name))
        else:
            d = np.abs(got.astype(np.float64) - want.astype(np.float64))
            bad = int((d > 1e-5 * np.abs(want) + 1e-6).sum())
            assert bad <= max(8, 0.02 * want.size) and d.max() < 1e-3, "[relaxed]: %d of %d cells outside the band" % (bad, want.size)
