"""The strict simplex table kernels after the ladder's FMA fold (snoise2_tab_ladder: the unskew's first difference as
fmaf(f, x, -floor)) and the masked corner-1 step (corner1_step: x12.xy -= i1 as two adds under an exec mask), on the GPU
against the CPU oracle: bit for bit through nz_fractal_stripe / nz_fractal_shaped_stripe / nz_fractal_warped_stripe, at the
smallest grids that reach what changed.

    ladder   8 x 130 (one full wave and a wave of one lane), 5 x 129 (odd width: the scalar store) and 9 x 2 (a two-column
             plane: one lane), stepdown 2, no detune, 13 octaves and 1, each at noiseSize 1700 and 1, at (0, 0), (-4096, -37)
             and (-1, -2): column 1 has x = 0 and row 2 has z = 0, the coordinates that scale without a bound.  (At
             noiseSize 1 the tile at (-4096, -37) passes the tables' range in its 13 octaves, 4096 * 4096 > 2^20, and takes
             the guarded loop with its direct evaluation; the two others stay in the ladder with integer coordinates.)
    masks    1 octave at noiseSize 4096, 8 x 130: at (2048, 0) every cell has the corner-1 select true, at (0, 2048) every
             cell has it false -- a wave runs one of the two adds with no lane enabled -- and at (0, 0) both values sit in
             one wave.  A float32 numpy restatement of the skew / floor / unskew asserts that the tiles hold those masks.
    loops    8 x 130, one tile per other octave loop the masked step reaches: the host table (stepdown 2.5), the
             recurrence in the kernel, the guarded loop with its direct evaluation
    shapes   billow and ridged through the shaped entry, fBm through the warped entry, 8 x 130
    fast     tolerance mode on one ladder tile: 1e-5 relative / 1e-6 absolute, the mode's contract (its code is unchanged)"""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_parity
from fractal_shapes_ref import BILLOW, FBM, RIDGED, fractal_shaped
from fractal_warp_ref import fractal_warped

gpu = pytest.mark.gpu  # (the mask test is numpy alone)
f32 = np.float32
SIMPLEX = 3
SHAPES = {"8x130": (8, 130), "5x129": (5, 129), "9x2": (9, 2)}
POSITIONS = {"origin": (0, 0), "negative": (-4096, -37), "zero_row_col": (-1, -2)}
# 1 octave, noiseSize 4096, 8 x 130: (xpos, zpos)
MASK_TILES = {"all_true": (2048, 0), "all_false": (0, 2048), "mixed": (0, 0)}
MASK_ROWS, MASK_COLS, MASK_NS = 8, 130, 4096
# (hurst, amp, stepdown, detune, octaves, xpos, zpos, noiseSize), the families of test_gpu_fractal_octave_trim.py
LOOPS = {"host_table": (0.4, 1.0, 2.5, 0.0, 13, 4096, -8192, 1700),
         "device_recurrence": (0.4, 1.0, 2.0, 0.0, 17, 7, 3, 90000),
         "guarded_and_direct": (0.4, 1.0, 2.0, 0.0, 13, 900, 1021, 4)}
LADDER = (0.4, 1.0, 2.0, 0.0, 13, 4096, -8192, 1700)


def ladder_args(pos, octaves, noise_size):
    return (0.4, 1.0, 2.0, 0.0, octaves) + POSITIONS[pos] + (noise_size,)


def mask_args(tile):
    return (0.4, 1.0, 2.0, 0.0, 1) + MASK_TILES[tile] + (MASK_NS,)


def corner1_select(tile):
    """The corner-1 select of the tile's one octave per cell, operation by operation in float32 (snoise2_tab)."""
    xpos, zpos = MASK_TILES[tile]
    Cx, Cy = f32(0.211324865405187), f32(0.366025403784439)
    x = ((np.arange(MASK_COLS, dtype=f32) + f32(xpos)) / f32(MASK_NS))[None, :]
    z = ((np.arange(MASK_ROWS, dtype=f32) + f32(zpos)) / f32(MASK_NS))[:, None]
    vx, vy = np.broadcast_arrays(f32(1) * x, f32(1) * z)
    s = vx * Cy + vy * Cy
    fx, fy = np.floor(vx + s), np.floor(vy + s)
    t = fx * Cx + fy * Cx
    x0x, x0y = vx - fx + t, vy - fy + t
    assert all(a.dtype == f32 for a in (s, fx, x0x, x0y))
    return x0x > x0y


def test_mask_tiles_hold_their_masks():
    assert corner1_select("all_true").all()
    assert not corner1_select("all_false").any()
    gt = corner1_select("mixed")
    # a wave holds columns 0 .. 127 of a row, two cells per lane: the step runs once over the even and once over the odd ones
    halves = [gt[r, c:128:2] for r in range(MASK_ROWS) for c in (0, 1)]
    both = [h.any() and not h.all() for h in halves]
    print("mixed: %d of %d half-waves hold both values" % (sum(both), len(both)))
    assert sum(both) >= 8


def stripe(ctx, nj, rows, cols, args, shape=None, warp=None):
    """nz_fractal_stripe / nz_fractal_shaped_stripe / nz_fractal_warped_stripe on a rows x cols buffer that owns every row."""
    d = ctx.alloc(rows * cols)
    st = nj.Stripe(cols, rows, 0, rows, 0, rows, cols)
    try:
        if warp is not None:
            ctx.call("nz_fractal_warped_stripe", SIMPLEX, d.ptr, C.byref(st), *args, *shape, *warp)
        elif shape is not None:
            ctx.call("nz_fractal_shaped_stripe", SIMPLEX, d.ptr, C.byref(st), *args, *shape)
        else:
            ctx.call("nz_fractal_stripe", SIMPLEX, d.ptr, C.byref(st), *args)
        return d.ToArray((rows, cols))
    finally:
        d.Dispose()


def check_bits(got, want, what):
    assert np.array_equal(got, want), "%s: %d cells differ" % (what, int((got != want).sum()))


@gpu
@pytest.mark.parametrize("noise_size", (1700, 1))
@pytest.mark.parametrize("octaves", (13, 1))
@pytest.mark.parametrize("pos", sorted(POSITIONS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_ladder_tiles_match_oracle(nj, ctx, oracle, shape, pos, octaves, noise_size):
    rows, cols = SHAPES[shape]
    args = ladder_args(pos, octaves, noise_size)
    check_bits(stripe(ctx, nj, rows, cols, args), oracle.fractal(SIMPLEX, rows, cols, *args), "%s %s" % (shape, args))


@gpu
@pytest.mark.parametrize("tile", sorted(MASK_TILES))
def test_mask_tiles_match_oracle(nj, ctx, oracle, tile):
    args = mask_args(tile)
    check_bits(stripe(ctx, nj, MASK_ROWS, MASK_COLS, args), oracle.fractal(SIMPLEX, MASK_ROWS, MASK_COLS, *args), tile)


@gpu
@pytest.mark.parametrize("loop", sorted(LOOPS))
def test_other_octave_loops_match_oracle(nj, ctx, oracle, loop):
    check_bits(stripe(ctx, nj, 8, 130, LOOPS[loop]), oracle.fractal(SIMPLEX, 8, 130, *LOOPS[loop]), loop)


@gpu
@pytest.mark.parametrize("shape", [(BILLOW, 1.0, 2.0), (RIDGED, 0.9, 3.5)], ids=["billow", "ridged"])
def test_shaped_entry_matches_the_driver(nj, ctx, shape):
    for args in (LADDER, LOOPS["host_table"], mask_args("mixed")):
        want = fractal_shaped(SIMPLEX, 8, 130, *args, shape=shape[0], offset=shape[1], gain=shape[2])
        check_bits(stripe(ctx, nj, 8, 130, args, shape), want, "shape=%s %s" % (shape, args))


@gpu
def test_warped_entry_matches_the_driver(nj, ctx):
    warp = (37.5, 1.0, 3)
    for args in ((0.4, 1.0, 2.0, 0.0, 8, -2100, -777, 97), mask_args("mixed")):
        want = fractal_warped(SIMPLEX, 8, 130, *args, shape=FBM, warp_strength=warp[0], warp_scale=warp[1],
                              warp_octaves=warp[2])
        check_bits(stripe(ctx, nj, 8, 130, args, (FBM, 1.0, 2.0), warp), want, "warped %s" % (args,))


@gpu
def test_tolerance_mode_keeps_its_contract(nj, oracle):
    c = nj.Context(0)
    c.float_mode = 1
    try:
        assert_parity(stripe(c, nj, 8, 130, LADDER), oracle.fractal(SIMPLEX, 8, 130, *LADDER), "fast, ladder tile")
    finally:
        c.close()
