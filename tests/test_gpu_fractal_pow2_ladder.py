"""The strict simplex fBm kernel's power-of-two octave ladder on the GPU (fractal_simplex_tab_kernel: with every octave
frequency a power of two the skewed coordinates of octave i are octave 0's times f[i]) against the CPU oracle, bit for bit,
at the smallest grids that reach every path of the launch:

    5 x 130     one workgroup per row, a partial last thread pair, more rows than rows_per_wg after the small-grid reduction
    9 x 1027    three workgroups per row, an odd last column
    512 x 512   a batch of two tiles with different positions (the batch entry takes square tiles; every row is compared)

Ladder tables (stepdown 2, 4, 0.5 without detune), tables that are none (detune 0.01, stepdown 3: the loop the kernel
always had), rows partly beyond the tables' range (the guarded loop; a wave with one such lane leaves the ladder as a
whole), coordinates that are exactly zero, and the three octave shapes.  The tolerance mode keeps its own contract."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_parity
from fractal_shapes_ref import BILLOW, FBM, RIDGED, fractal_shaped

pytestmark = pytest.mark.gpu
SIMPLEX = 3
GRIDS = [(5, 130), (9, 1027)]  # rows, cols
# (hurst, amp, stepdown, detune, octaves, xpos, zpos, noiseSize)
DEFAULT = [(0.4, 1.0, 2.0, 0.0, 1, -2100, -777, 97),
           (0.4, 1.0, 2.0, 0.0, 13, 4096, -8192, 1700),
           (0.4, 1.0, 2.0, 0.0, 16, 7, 3, 90000)]       # the table's maximum: fmax 2^15, coordinates below 32
LADDER = [(0.5938, 1.3, 4.0, 0.0, 8, -300, 41, 300),    # fmax 2^14
          (0.4, 1.0, 0.5, 0.0, 13, -2100, -777, 97)]    # descending: the smallest frequency is 2^-12
NO_LADDER = [(0.4, 1.0, 2.0, 0.01, 13, 4096, -8192, 1700),
             (0.4, 1.0, 3.0, 0.0, 9, -300, 41, 300)]
# 13 octaves reach 2^12: |coordinate| >= 256 is beyond the tables.  noiseSize 4: columns from 1024 on (9 x 1027), columns
# from 124 on and every row (5 x 130, xpos 900) -- and column 0 / row 0 of the first are exactly zero
BEYOND = [(0.4, 1.0, 2.0, 0.0, 13, 0, 0, 4),
          (0.4, 1.0, 2.0, 0.0, 13, 900, 1021, 4)]
# a column and a row that are exactly zero inside the grid, positive and negative zero (noiseSize < 0: -0)
ZEROS = [(0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700),
         (0.4, 1.0, 2.0, 0.0, 13, -64, -2, 1700),
         (0.4, 1.0, 0.5, 0.0, 13, -129, -4, -97)]


def stripe(ctx, nj, rows, cols, args, shape=None):
    """nz_fractal_stripe / nz_fractal_shaped_stripe on a rows x cols buffer that owns every row."""
    d = ctx.alloc(rows * cols)
    st = nj.Stripe(cols, rows, 0, rows, 0, rows, cols)
    hurst, amp, step, det, octv, xp, zp, ns = args
    if shape is None:
        ctx.call("nz_fractal_stripe", SIMPLEX, d.ptr, C.byref(st), hurst, amp, step, det, octv, xp, zp, ns)
    else:
        ctx.call("nz_fractal_shaped_stripe", SIMPLEX, d.ptr, C.byref(st), hurst, amp, step, det, octv, xp, zp, ns, *shape)
    out = d.ToArray((rows, cols))
    d.Dispose()
    return out


def check_bits(got, want, what):
    assert np.array_equal(got, want), "%s: %d cells differ" % (what, int((got != want).sum()))


@pytest.mark.parametrize("rows,cols", GRIDS, ids=["5x130", "9x1027"])
@pytest.mark.parametrize("family", ["default", "ladder", "no_ladder", "beyond", "zeros"])
def test_fbm_matches_oracle(nj, ctx, oracle, rows, cols, family):
    for args in {"default": DEFAULT, "ladder": LADDER, "no_ladder": NO_LADDER, "beyond": BEYOND, "zeros": ZEROS}[family]:
        got = stripe(ctx, nj, rows, cols, args)
        check_bits(got, oracle.fractal(SIMPLEX, rows, cols, *args), "%dx%d %s" % (rows, cols, args))


@pytest.mark.parametrize("rows,cols", GRIDS, ids=["5x130", "9x1027"])
@pytest.mark.parametrize("shape", [(FBM, 1.0, 2.0), (BILLOW, 1.0, 2.0), (RIDGED, 0.9, 3.5)], ids=["fbm", "billow", "ridged"])
def test_shapes_match_the_driver(nj, ctx, rows, cols, shape):
    for args in (DEFAULT[1], LADDER[1], NO_LADDER[0], BEYOND[0]):
        got = stripe(ctx, nj, rows, cols, args, shape)
        want = fractal_shaped(SIMPLEX, rows, cols, *args, shape=shape[0], offset=shape[1], gain=shape[2])
        check_bits(got, want, "%dx%d shape=%s %s" % (rows, cols, shape, args))


@pytest.mark.parametrize("args", [DEFAULT[1], LADDER[0], NO_LADDER[0], DEFAULT[2]], ids=["x2", "x4", "detune", "16oct"])
def test_batch_of_two(nj, ctx, oracle, args):
    res, pos = 512, [(0, 0), (-4096, 1536)]
    hurst, amp, step, det, octv, _, _, ns = args
    b = nj.GeneratorDataBatch.create(ctx, "b", res, pos)
    ctx.call("nz_fractal_batch", SIMPLEX, b.data.ptr, res, len(pos), b.positions.ptr, hurst, amp, step, det, octv, ns)
    got = b.data.ToArray((len(pos), res, res))
    b.data.Dispose(); b.positions.Dispose()
    for k, (xp, zp) in enumerate(pos):
        check_bits(got[k], oracle.fractal(SIMPLEX, res, res, hurst, amp, step, det, octv, xp, zp, ns), "tile %d %s" % (k, args))


def test_tolerance_mode_keeps_its_contract(nj, oracle):
    # FAST has no ladder: the parent's contract, 1e-5 relative / 1e-6 absolute against the oracle
    c = nj.Context(0)
    c.float_mode = 1
    try:
        for rows, cols in GRIDS:
            got = stripe(c, nj, rows, cols, DEFAULT[1])
            assert_parity(got, oracle.fractal(SIMPLEX, rows, cols, *DEFAULT[1]), "fast %dx%d" % (rows, cols))
    finally:
        c.close()
