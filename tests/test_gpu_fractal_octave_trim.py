"""The simplex table kernels after the octave trim (clamp-folded corner falloffs; T1 staged as pairs {k(i), k(i) - step} so
that the three corner addresses are a0, (gt ? a0 : a2m) + step and a2m + 2 step), on the GPU against the CPU oracle: strict
mode bit for bit through nz_fractal_stripe / nz_fractal_shaped_stripe, at the smallest grids that reach what changed.

    a  8 x 130, xpos -6600, zpos 80, noiseSize 1     lattice x index 289 (fp32 mod289 of -8959)
    b  8 x 130, xpos 80, zpos -6590, noiseSize 1     lattice y index 289: T1 entry iy + 1 = 290 is read; iy spans 1 .. 289
    a2, b2  the same places at noiseSize 2 (xpos -13200, zpos 160 / xpos 160, zpos -13180): half-cell coordinates, so that
       the corner-1 select takes both values in those cells (at noiseSize 1 it is false in every cell of a and b)
    g  8 x 130, xpos -3, zpos -4, noiseSize 2        ix = 0 with iy = 288: k(289) = 0, so a2m = -step, the one negative base
    c  5 x 130, one tile per octave loop of the kernel (ladder, host table, device recurrence, guarded table / direct)
    d  5 x 130, the three octave shapes
    e  9 x 130, warped simplex against tests/fractal_warp_ref.py (the warped kernels stage the tables themselves)
    f  tolerance mode on a, a2, b, b2, g: 1e-5 relative / 1e-6 absolute against the oracle, the mode's contract

For a, b and g a float32 numpy restatement of the kernel's skew / floor / mod289 shows first that the tiles hold the cells
they are there for (a: 5, b: 22 in octave 0), with both values of the corner-1 select among them (a with a2, b with b2), and
corner falloffs that are clamped to exactly 0 as well as positive ones."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_parity
from fractal_shapes_ref import BILLOW, FBM, RIDGED, fractal_shaped
from fractal_warp_ref import fractal_warped

gpu = pytest.mark.gpu  # (the lattice test is numpy alone)
f32 = np.float32
SIMPLEX = 3
ROWS, COLS = 8, 130
# (xpos, zpos, noiseSize); hurst 0.4, amp 1, stepdown 2, no detune; 1 and 3 octaves
EDGE_TILES = {"a": (-6600, 80, 1), "a2": (-13200, 160, 2), "b": (80, -6590, 1), "b2": (160, -13180, 2), "g": (-3, -4, 2)}
OCTAVES = (1, 3)
# (hurst, amp, stepdown, detune, octaves, xpos, zpos, noiseSize) on 5 x 130: the families of test_gpu_fractal_pow2_ladder.py
LOOPS = {"ladder": (0.4, 1.0, 2.0, 0.0, 13, 4096, -8192, 1700),
         "host_table": (0.4, 1.0, 2.0, 0.01, 13, 4096, -8192, 1700),
         # 17 octaves: more than the host's octave table holds (16), so f and a come from the recurrence in the kernel; the
         # entries accept it.  fmax 2^16, coordinates below 16
         "device_recurrence": (0.4, 1.0, 2.0, 0.0, 17, 7, 3, 90000),
         # noiseSize 4, 13 octaves reach 2^12: columns from 124 on and rows from 3 on pass 2^20 in the upper octaves (the
         # direct evaluation) and stay inside it in the lower ones (the guarded table evaluation)
         "guarded_and_direct": (0.4, 1.0, 2.0, 0.0, 13, 900, 1021, 4)}


def edge_args(tile, octaves):
    xpos, zpos, ns = EDGE_TILES[tile]
    return (0.4, 1.0, 2.0, 0.0, octaves, xpos, zpos, ns)


def lattice(tile, octaves):
    """The kernel's lattice indices, corner-1 select and the three corner falloffs before the clamp, per octave and cell,
    operation by operation in float32 (snoise2_tab of nz_fractal.hip)."""
    xpos, zpos, ns = EDGE_TILES[tile]
    Cx, Cy, Cz = f32(0.211324865405187), f32(0.366025403784439), f32(-0.577350269189626)
    x = ((np.arange(COLS, dtype=f32) + f32(xpos)) / f32(ns))[None, :]
    z = ((np.arange(ROWS, dtype=f32) + f32(zpos)) / f32(ns))[:, None]
    out = []
    for i in range(octaves):
        f = f32(2.0 ** i)
        vx, vy = np.broadcast_arrays(f * x, f * z)
        s = vx * Cy + vy * Cy
        fx, fy = np.floor(vx + s), np.floor(vy + s)
        t = fx * Cx + fy * Cx
        x0x, x0y = vx - fx + t, vy - fy + t
        gt = x0x > x0y
        x12x = x0x + Cx - np.where(gt, f32(1), f32(0))
        x12y = x0y + Cx - np.where(gt, f32(0), f32(1))
        x12z, x12w = x0x + Cz, x0y + Cz
        mod289 = lambda v: v - np.floor(v * f32(1.0 / 289.0)) * f32(289.0)  # every product is an exact integer
        m = np.stack([f32(0.5) - (x0x * x0x + x0y * x0y), f32(0.5) - (x12x * x12x + x12y * x12y),
                      f32(0.5) - (x12z * x12z + x12w * x12w)])
        assert all(a.dtype == f32 for a in (fx, fy, x0x, x12x, m))
        out.append((mod289(fx).astype(np.int64), mod289(fy).astype(np.int64), gt, m))
    return out


def reaches(tile, ix, iy):
    """the cells of one octave that this tile is there for"""
    if tile[0] == "a":
        return ix == 289
    if tile[0] == "b":
        return iy == 289
    return (ix == 0) & (iy == 288)


@pytest.mark.parametrize("group", ["a", "b", "g"])
def test_edge_tiles_hold_their_cells(group):
    gts = []
    for tile in sorted(t for t in EDGE_TILES if t[0] == group):
        counts, seen_iy, ms = [], set(), []
        for ix, iy, gt, m in lattice(tile, max(OCTAVES)):
            assert 0 <= ix.min() and ix.max() <= 289 and 0 <= iy.min() and iy.max() <= 289
            sel = reaches(tile, ix, iy)
            counts.append(int(sel.sum()))
            gts.append(gt[sel])
            ms.append(m[:, sel].ravel())
            seen_iy.update(np.unique(iy).tolist())
        print("tile %s: cells per octave %s" % (tile, counts))
        assert counts[0] > 0  # already in the octave a single-octave call runs
        assert counts[0] == {"a": 5, "b": 22}.get(tile, counts[0])
        ms = np.concatenate(ms)
        assert (ms <= 0).any() and (ms > 0).any(), "a corner falloff clamped to exactly 0 and a positive one, in these cells"
        if tile == "b":
            assert min(seen_iy) == 1 and max(seen_iy) == 289
    gts = np.concatenate(gts)
    if group == "g":
        assert not gts.all()  # corner 1 takes the negative base as well
    else:
        # (with noiseSize 1 every coordinate is an integer, x0.x == x0.y and the select is false in all of a and b: a2 and
        # b2, the same lattice cells at half-cell coordinates, bring the cells with the select true)
        assert gts.any() and not gts.all(), "both values of the corner-1 select among these cells"


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


_WANT = {}


def want_edge(oracle, tile, octaves):
    """the oracle's plane of an edge tile, computed once for the strict and the tolerance test"""
    key = (tile, octaves)
    if key not in _WANT:
        _WANT[key] = oracle.fractal(SIMPLEX, ROWS, COLS, *edge_args(tile, octaves))
        _WANT[key].setflags(write=False)
    return _WANT[key]


def check_bits(got, want, what):
    assert np.array_equal(got, want), "%s: %d cells differ" % (what, int((got != want).sum()))


@gpu
@pytest.mark.parametrize("octaves", OCTAVES)
@pytest.mark.parametrize("tile", sorted(EDGE_TILES))
def test_edge_tiles_match_oracle(nj, ctx, oracle, tile, octaves):
    got = stripe(ctx, nj, ROWS, COLS, edge_args(tile, octaves))
    check_bits(got, want_edge(oracle, tile, octaves), "tile %s, %d octaves" % (tile, octaves))


@gpu
@pytest.mark.parametrize("loop", sorted(LOOPS))
def test_every_octave_loop_matches_oracle(nj, ctx, oracle, loop):
    got = stripe(ctx, nj, 5, 130, LOOPS[loop])
    check_bits(got, oracle.fractal(SIMPLEX, 5, 130, *LOOPS[loop]), loop)


@gpu
@pytest.mark.parametrize("shape", [(FBM, 1.0, 2.0), (BILLOW, 1.0, 2.0), (RIDGED, 0.9, 3.5)], ids=["fbm", "billow", "ridged"])
def test_shaped_entry_matches_the_driver(nj, ctx, shape):
    for args in (LOOPS["ladder"], edge_args("b", 3)):
        got = stripe(ctx, nj, 5, 130, args, shape)
        want = fractal_shaped(SIMPLEX, 5, 130, *args, shape=shape[0], offset=shape[1], gain=shape[2])
        check_bits(got, want, "shape=%s %s" % (shape, args))


def warped_stripe(ctx, nj, rows, cols, args, shape, warp):
    d = ctx.alloc(rows * cols)
    st = nj.Stripe(cols, rows, 0, rows, 0, rows, cols)
    ctx.call("nz_fractal_warped_stripe", SIMPLEX, d.ptr, C.byref(st), *args, shape, 1.0, 2.0, *warp)
    out = d.ToArray((rows, cols))
    d.Dispose()
    return out


@gpu
def test_warped_staging_matches_the_driver(nj, ctx):
    rows, cols, warp = 9, 130, (37.5, 1.0, 3)
    # a plain tile, and tile b's position: the displacement and the octave loop both read T1 entry 290 there
    tiles = [(0.4, 1.0, 2.0, 0.0, 8, -2100, -777, 97), (0.4, 1.0, 2.0, 0.0, 3, 80, -6590, 1)]
    fast = nj.Context(0)
    fast.float_mode = 1
    try:
        for args in tiles:
            want = fractal_warped(SIMPLEX, rows, cols, *args, shape=FBM, warp_strength=warp[0], warp_scale=warp[1],
                                  warp_octaves=warp[2])
            check_bits(warped_stripe(ctx, nj, rows, cols, args, FBM, warp), want, "warped %s" % (args,))
            # the tolerance form (its own halved pair table) stays inside its band of the strict result
            assert_parity(warped_stripe(fast, nj, rows, cols, args, FBM, warp), want, "warped, fast %s" % (args,))
    finally:
        fast.close()


@gpu
def test_tolerance_mode_keeps_its_contract(nj, oracle):
    c = nj.Context(0)
    c.float_mode = 1
    try:
        for tile in sorted(EDGE_TILES):
            for octaves in OCTAVES:
                got = stripe(c, nj, ROWS, COLS, edge_args(tile, octaves))
                assert_parity(got, want_edge(oracle, tile, octaves), "fast, tile %s, %d octaves" % (tile, octaves))
    finally:
        c.close()
