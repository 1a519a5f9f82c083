"""Upsample / downsample on the GPU (nz_upsample*, nz_downsample*, UpsampleStage, DownsampleStage) against the numpy model of
tests/resample_ref.py, bit for bit: every output is prefilled with NaN and compared as bit patterns.  Tiles at sizes that
cover single cells, partial workgroup tiles in both directions and more than one workgroup per axis at every factor; batches
at odd float offsets; planes carved from a guarded slab at the four 4-byte phases; stripes of a non-square grid; special
values; the float modes; every refusal; handles; the coarse-to-fine recipe through the C ABI; the stages in a pipeline."""
import ctypes as C
import functools

import numpy as np
import pytest

import hydraulic_ref as H
import resample_ref as R
from slab import Slab
from test_gpu_hydraulic import assert_bits
from test_hydraulic_ref import NAMES, PARAMS

pytestmark = pytest.mark.gpu
f32 = np.float32
# 131 joins the issue's list: the upsample tile is 256 fine columns wide, so at factor 2 it takes more than 128 coarse
# columns to put two workgroups side by side
RESOLUTIONS = (1, 2, 3, 5, 37, 67, 131)
NAN = f32(np.nan)


@functools.lru_cache(maxsize=None)
def plane(rows, cols=None, seed=0):
    """A reproducible plane with structure at every scale and both signs (read-only: shared between tests)."""
    cols = cols or rows
    rng = np.random.default_rng(1000 * rows + cols + seed)
    z, x = np.mgrid[0:rows, 0:cols].astype(f32)
    a = (np.sin(x * f32(0.37)) * np.cos(z * f32(0.23)) + rng.standard_normal((rows, cols)).astype(f32) * f32(0.25)).astype(f32)
    a.setflags(write=False)
    return a


def nan_tile(ctx, n):
    return ctx.from_host(np.full(n, NAN, f32))


def gpu_upsample(ctx, src, f, filt, base=None, inplace=False, count=1):
    """src: (R, R) or (count, R, R).  -> the fine plane(s).  base with inplace: dst starts as the base plane."""
    src = np.ascontiguousarray(src, f32)
    res = src.shape[-1]
    shape = src.shape[:-2] + (res * f, res * f)
    s = ctx.from_host(src)
    d = ctx.from_host(base) if inplace else nan_tile(ctx, int(np.prod(shape)))
    b = None if base is None else (d if inplace else ctx.from_host(base))
    bp = b.ptr if b is not None else None
    if count > 1:
        ctx.call("nz_upsample_batch", s.ptr, res, d.ptr, f, filt, bp, count)
    else:
        ctx.call("nz_upsample", s.ptr, res, d.ptr, f, filt, bp)
    got = d.ToArray(shape)
    if b is not None and not inplace:
        assert_bits(b.ToArray(shape), np.ascontiguousarray(base, f32), "base is only read")
        b.Dispose()
    assert_bits(s.ToArray(src.shape), src, "src is only read")
    s.Dispose(); d.Dispose()
    return got


def gpu_downsample(ctx, src, f, count=1):
    src = np.ascontiguousarray(src, f32)
    res = src.shape[-1]
    shape = src.shape[:-2] + (res // f, res // f)
    s, d = ctx.from_host(src), nan_tile(ctx, int(np.prod(shape)))
    if count > 1:
        ctx.call("nz_downsample_batch", s.ptr, res, d.ptr, f, count)
    else:
        ctx.call("nz_downsample", s.ptr, res, d.ptr, f)
    got = d.ToArray(shape)
    s.Dispose(); d.Dispose()
    return got


# 1. upsample: resolutions x factors x filters x base absent / separate / in place
@pytest.mark.parametrize("filt", R.FILTERS)
@pytest.mark.parametrize("f", R.FACTORS)
def test_upsample_matches_the_model(ctx, f, filt):
    for res in RESOLUTIONS:
        src, base = plane(res), plane(res * f, seed=5)
        assert_bits(gpu_upsample(ctx, src, f, filt), R.upsample(src, f, filt), "res %d no base" % res)
        want = R.upsample(src, f, filt, base)
        assert_bits(gpu_upsample(ctx, src, f, filt, base), want, "res %d base apart" % res)
        assert_bits(gpu_upsample(ctx, src, f, filt, base, inplace=True), want, "res %d base in place" % res)


# 2. downsample
@pytest.mark.parametrize("f", R.FACTORS)
def test_downsample_matches_the_model(ctx, f):
    for k in (1, 3, 37, 67, 131):
        src = plane(k * f, seed=2)
        assert_bits(gpu_downsample(ctx, src, f), R.downsample(src, f), "res %d" % (k * f))


# 3. batches of 3 at resolution 37: tiles 1 and 2 sit at odd float offsets; tile k equals the single-tile call and the model
@pytest.mark.parametrize("f", R.FACTORS)
def test_batches_equal_single_tiles(ctx, f):
    tiles = np.stack([plane(37, seed=k) for k in range(3)])
    bases = np.stack([plane(37 * f, seed=10 + k) for k in range(3)])
    for filt in R.FILTERS:
        for base, inplace in ((None, False), (bases, False), (bases, True)):
            got = gpu_upsample(ctx, tiles, f, filt, base, inplace, count=3)
            for k in range(3):
                b = None if base is None else base[k]
                assert_bits(got[k], gpu_upsample(ctx, tiles[k], f, filt, b, inplace), "up tile %d filter %d" % (k, filt))
                assert_bits(got[k], R.upsample(tiles[k], f, filt, b), "up tile %d filter %d: model" % (k, filt))
    fine = np.stack([plane(37 * f, seed=20 + k) for k in range(3)])
    got = gpu_downsample(ctx, fine, f, count=3)
    for k in range(3):
        assert_bits(got[k], gpu_downsample(ctx, fine[k], f), "down tile %d" % k)
        assert_bits(got[k], R.downsample(fine[k], f), "down tile %d: model" % k)


# 4. planes carved from a guarded slab at the four 4-byte phases
@pytest.mark.parametrize("phase", range(4))
def test_slab_carved_planes_at_every_phase(ctx, phase):
    res = 37
    for f in R.FACTORS:
        src, base, fine = plane(res), plane(res * f, seed=5), plane(res * f, seed=2)
        n = (res * f) ** 2
        for filt in R.FILTERS:
            for mode in ("none", "apart", "inplace"):
                with Slab(ctx, guard=2048) as slab:
                    s = slab.carve(res * res, (phase + 1) % 4, fill=src, name="src")
                    d = slab.carve(n, phase, fill=base if mode == "inplace" else NAN, name="dst")
                    b = slab.carve(n, (phase + 2) % 4, fill=base, name="base") if mode == "apart" else None
                    slab.upload()
                    bp = None if mode == "none" else d.ptr if mode == "inplace" else b.ptr
                    ctx.call("nz_upsample", s.ptr, res, d.ptr, f, filt, bp).Complete()
                    want = R.upsample(src, f, filt, None if mode == "none" else base)
                    assert_bits(d.ToArray((res * f, res * f)), want, "up f %d filter %d base %s" % (f, filt, mode))
                    slab.check()
        with Slab(ctx, guard=2048) as slab:
            s = slab.carve(n, phase, fill=fine, name="src")
            d = slab.carve(res * res, (phase + 3) % 4, fill=NAN, name="dst")
            slab.upload()
            ctx.call("nz_downsample", s.ptr, res * f, d.ptr, f).Complete()
            assert_bits(d.ToArray((res, res)), R.downsample(fine, f), "down f %d" % f)
            slab.check()


# 5. stripes of a non-square grid: gathered owned rows equal the monolithic call and the model; pad floats and non-owned
#    rows still hold NaN; one ghost row too few is refused
def stripe_buffer(ctx, content, pitch):
    """A device buffer of len(content) rows `pitch` floats apart: `content` in the first columns, NaN in the pad."""
    rows, cols = content.shape
    host = np.full((rows, pitch), NAN, f32)
    host[:, :cols] = content
    return ctx.from_host(host[:rows].reshape(-1)[:(rows - 1) * pitch + cols] if rows else host.reshape(-1))


def read_stripe(tile, rows, cols, pitch):
    flat = tile.ToArray()
    full = np.full(rows * pitch, NAN, f32)
    full[:flat.size] = flat
    return full.reshape(rows, pitch)[:, :cols], full.reshape(rows, pitch)[:, cols:]


@pytest.mark.parametrize("padded", (False, True))
@pytest.mark.parametrize("f", (2, 4))
def test_stripes_equal_the_monolithic_grid(nj, ctx, f, padded):
    crows, ccols = 40, 96
    frows, fcols = crows * f, ccols * f
    coarse, base, fine = plane(crows, ccols), plane(frows, fcols, seed=5), plane(frows, fcols, seed=2)
    cpitch, fpitch = (ccols + 1, fcols + 3) if padded else (ccols, fcols)
    S = nj.Stripe
    whole_c = S(ccols, crows, 0, crows, 0, crows, 0)
    whole_f = S(fcols, frows, 0, frows, 0, frows, 0)
    for filt in R.FILTERS:
        halo = nj._native.lib.nz_upsample_stripe_halo_rows(filt)
        assert halo == R.HALO[filt]
        for with_base in (False, True):
            want = R.upsample_stripe(coarse, 0, crows, 0, frows, f, filt, base if with_base else None)
            s, d = ctx.from_host(coarse), nan_tile(ctx, frows * fcols)
            b = ctx.from_host(base) if with_base else None
            ctx.call("nz_upsample_stripe", s.ptr, C.byref(whole_c), d.ptr, C.byref(whole_f), f, filt, b.ptr if b else None)
            assert_bits(d.ToArray((frows, fcols)), want, "monolithic stripe call, filter %d" % filt)
            for world in (1, 2, 3, 5):
                cuts = [frows * r // world for r in range(world + 1)]
                parts = []
                for g0, g1 in zip(cuts, cuts[1:]):
                    lo, hi = max(g0 // f - halo, 0), min((g1 - 1) // f + halo, crows - 1)
                    b0, b1 = max(g0 - 1, 0), min(g1 + 1, frows)  # the fine buffer holds a row more on either side
                    cst = S(ccols, hi + 1 - lo, lo, crows, max(g0 // f - lo, 0), min((g1 - 1) // f - lo + 1, hi + 1 - lo), cpitch if padded else 0)
                    fst = S(fcols, b1 - b0, b0, frows, g0 - b0, g1 - b0, fpitch if padded else 0)
                    sb = stripe_buffer(ctx, coarse[lo:hi + 1], cpitch)
                    db = stripe_buffer(ctx, np.full((b1 - b0, fcols), NAN, f32), fpitch)
                    bb = stripe_buffer(ctx, base[b0:b1], fpitch) if with_base else None
                    ctx.call("nz_upsample_stripe", sb.ptr, C.byref(cst), db.ptr, C.byref(fst), f, filt, bb.ptr if bb else None)
                    cells, pad = read_stripe(db, b1 - b0, fcols, fpitch)
                    parts.append(cells[g0 - b0:g1 - b0])
                    assert np.isnan(pad).all() and np.isnan(cells[:g0 - b0]).all() and np.isnan(cells[g1 - b0:]).all(), \
                        "pad floats and non-owned rows are not written"
                    if lo > 0 and halo:  # one ghost row too few above
                        short = S(ccols, hi - lo, lo + 1, crows, cst.own0 - 1, cst.own1 - 1, cst.pitch)
                        with pytest.raises(nj.NoizeError) as e:
                            ctx.call("nz_upsample_stripe", sb.ptr + 4 * cpitch, C.byref(short), db.ptr, C.byref(fst), f, filt, None)
                        assert e.value.status == nj._native.NZ_ERR_INVALID and "srcSt" in str(e.value)
                        assert_bits(read_stripe(db, b1 - b0, fcols, fpitch)[0], cells, "a refused call writes nothing")
                    for t in (sb, db, bb):
                        if t is not None:
                            t.Dispose()
                assert_bits(np.concatenate(parts), want, "up filter %d base %s world %d" % (filt, with_base, world))
            for t in (s, d, b):
                if t is not None:
                    t.Dispose()
    want = R.downsample(fine, f)
    for world in (1, 2, 3, 5):
        cuts = [crows * r // world for r in range(world + 1)]
        parts = []
        for g0, g1 in zip(cuts, cuts[1:]):
            b0, b1 = max(g0 - 1, 0), min(g1 + 1, crows)
            fst = S(fcols, f * (g1 - g0), f * g0, frows, 0, f * (g1 - g0), fpitch if padded else 0)
            cst = S(ccols, b1 - b0, b0, crows, g0 - b0, g1 - b0, cpitch if padded else 0)
            sb = stripe_buffer(ctx, fine[f * g0:f * g1], fpitch)
            db = stripe_buffer(ctx, np.full((b1 - b0, ccols), NAN, f32), cpitch)
            ctx.call("nz_downsample_stripe", sb.ptr, C.byref(fst), db.ptr, C.byref(cst), f)
            cells, pad = read_stripe(db, b1 - b0, ccols, cpitch)
            parts.append(cells[g0 - b0:g1 - b0])
            assert np.isnan(pad).all() and np.isnan(cells[:g0 - b0]).all() and np.isnan(cells[g1 - b0:]).all()
            if g1 - g0 > 1:  # a fine row too few below
                short = S(fcols, fst.rows - 1, fst.grow0, frows, 0, fst.rows - 1, fst.pitch)
                with pytest.raises(nj.NoizeError) as e:
                    ctx.call("nz_downsample_stripe", sb.ptr, C.byref(short), db.ptr, C.byref(cst), f)
                assert e.value.status == nj._native.NZ_ERR_INVALID and "srcSt" in str(e.value)
            sb.Dispose(); db.Dispose()
        assert_bits(np.concatenate(parts), want, "down world %d" % world)
    # the sharded driver's thin wrappers are the same entries
    from noize_job_amd.sharded import HipStripeOps

    class Buf:
        def __init__(self, tile):
            self.tile = tile

        def data_ptr(self):
            return self.tile.ptr

    ops = HipStripeOps(ctx)
    s, d, c = ctx.from_host(coarse), nan_tile(ctx, frows * fcols), nan_tile(ctx, crows * ccols)
    ops.upsample(Buf(s), whole_c, Buf(d), whole_f, f, R.CATMULL_ROM)
    assert_bits(d.ToArray((frows, fcols)), R.upsample_stripe(coarse, 0, crows, 0, frows, f, R.CATMULL_ROM), "ops.upsample")
    ops.downsample(Buf(d), whole_f, Buf(c), whole_c, f)
    assert_bits(c.ToArray((crows, ccols)), R.downsample(d.ToArray((frows, fcols)), f), "ops.downsample")
    assert ops.upsample_halo_rows(R.CATMULL_ROM) == 2
    s.Dispose(); d.Dispose(); c.Dispose()


# 6. NaN, +-Inf and -0 planes and cells: the model's bits (sums are seeded with +0, so only nearest returns -0)
def test_special_values(ctx):
    res = 37
    specials = {"nan": f32(np.nan), "+inf": f32(np.inf), "-inf": f32(-np.inf), "-0": f32(-0.0)}
    sprinkled = plane(res).copy()
    sprinkled[3, 4], sprinkled[20, 36], sprinkled[36, 0], sprinkled[11, 11] = np.nan, np.inf, -np.inf, -0.0
    sprinkled.view(np.uint32)[30, 30] = 0xFFC12345  # a NaN with a sign and a payload
    for f in R.FACTORS:
        base = plane(res * f, seed=5)
        inputs = [("sprinkled", sprinkled)] + [(k, np.full((res, res), v)) for k, v in specials.items()]
        for name, src in inputs:
            for filt in R.FILTERS:
                got = gpu_upsample(ctx, src, f, filt)
                assert_bits(got, R.upsample(src, f, filt), "%s f %d filter %d" % (name, f, filt))
                if name == "-0":
                    assert (got.view(np.uint32) == (0x80000000 if filt == R.NEAREST else 0)).all()
                assert_bits(gpu_upsample(ctx, src, f, filt, base), R.upsample(src, f, filt, base), "%s with base" % name)
        for name, v in specials.items():
            fine = np.full((res * f, res * f), v)
            assert_bits(gpu_downsample(ctx, fine, f), R.downsample(fine, f), "down %s f %d" % (name, f))
        fine = plane(res * f, seed=2).copy()
        fine[5, 7], fine[40, 3], fine[41, 3] = np.nan, np.inf, -np.inf
        assert_bits(gpu_downsample(ctx, fine, f), R.downsample(fine, f), "down sprinkled f %d" % f)


# 7. the three float modes give identical bits
def test_float_modes_are_identical(nj, ctx):
    src, base, fine = plane(67), plane(67 * 4, seed=5), plane(67 * 4, seed=2)
    want = [gpu_upsample(ctx, src, 4, filt, base) for filt in R.FILTERS] + [gpu_downsample(ctx, fine, 4)]
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got = [gpu_upsample(mctx, src, 4, filt, base) for filt in R.FILTERS] + [gpu_downsample(mctx, fine, 4)]
        finally:
            mctx.close()
        for k, (g, w) in enumerate(zip(got, want)):
            assert_bits(g, w, "float mode %d, case %d" % (mode, k))


# 8. every refusal is NZ_ERR_INVALID, names the argument and leaves dst untouched; the context stays usable
def test_refusals_write_nothing(nj, ctx):
    res, f = 16, 2
    n = (res * f) ** 2
    sentinel = np.full(2 * n, f32(7.25))
    big = ctx.from_host(sentinel)             # dst at its start; the overlap cases take src / base from inside it
    src = ctx.from_host(plane(res))
    fine = ctx.from_host(plane(res * f))
    S = nj.Stripe
    cst, fst = S(res, res, 0, res, 0, res, 0), S(res * f, res * f, 0, res * f, 0, res * f, 0)
    CR = R.CATMULL_ROM
    bad = [
        ("factor", "nz_upsample", (src.ptr, res, big.ptr, 3, CR, None)),
        ("factor", "nz_upsample", (src.ptr, res, big.ptr, 16, CR, None)),
        ("factor", "nz_upsample", (src.ptr, res, big.ptr, 0, CR, None)),
        ("factor", "nz_downsample", (fine.ptr, res * f, big.ptr, 3)),
        ("factor", "nz_upsample_batch", (src.ptr, res, big.ptr, 1, CR, None, 1)),
        ("factor", "nz_downsample_batch", (fine.ptr, res * f, big.ptr, -2, 1)),
        ("factor", "nz_upsample_stripe", (src.ptr, C.byref(cst), big.ptr, C.byref(fst), 5, CR, None)),
        ("factor", "nz_downsample_stripe", (fine.ptr, C.byref(fst), big.ptr, C.byref(cst), 6)),
        ("filter", "nz_upsample", (src.ptr, res, big.ptr, f, 3, None)),
        ("filter", "nz_upsample", (src.ptr, res, big.ptr, f, -1, None)),
        ("filter", "nz_upsample_stripe", (src.ptr, C.byref(cst), big.ptr, C.byref(fst), f, 9, None)),
        ("srcResolution", "nz_upsample", (src.ptr, 0, big.ptr, f, CR, None)),
        ("srcResolution", "nz_upsample", (src.ptr, -4, big.ptr, f, CR, None)),
        ("srcResolution", "nz_downsample", (fine.ptr, 0, big.ptr, f)),
        ("srcResolution", "nz_downsample", (fine.ptr, 30, big.ptr, 4)),          # 4 does not divide 30
        ("srcResolution", "nz_downsample", (fine.ptr, 31, big.ptr, f)),
        ("dst", "nz_upsample", (src.ptr, 8192, big.ptr, 8, CR, None)),           # 2^32 cells
        ("dst", "nz_upsample", (src.ptr, 23171, big.ptr, 2, CR, None)),          # 46342^2 > 2^31
        ("dst", "nz_upsample_batch", (src.ptr, 4096, big.ptr, 4, CR, None, 8)),  # 8 x 2^28
        ("dst", "nz_upsample", (src.ptr, 1 << 29, big.ptr, 8, CR, None)),        # (2^32)^2 wraps to 0 in 64 bits
        ("dst", "nz_upsample", (src.ptr, 1 << 30, big.ptr, 4, CR, None)),
        ("dst", "nz_upsample_batch", (src.ptr, 1 << 24, big.ptr, 2, CR, None, 1 << 14)),  # 2^14 x 2^50 wraps
        ("src", "nz_downsample", (fine.ptr, 1 << 30, big.ptr, 4)),
        ("src", "nz_downsample_batch", (fine.ptr, 1 << 24, big.ptr, 2, 1 << 14)),
        ("src", "nz_upsample", (None, res, big.ptr, f, CR, None)),
        ("dst", "nz_upsample", (src.ptr, res, None, f, CR, None)),
        ("src", "nz_downsample", (None, res * f, big.ptr, f)),
        ("dst", "nz_downsample", (fine.ptr, res * f, None, f)),
        ("src", "nz_upsample_stripe", (None, C.byref(cst), big.ptr, C.byref(fst), f, CR, None)),
        ("dst", "nz_downsample_stripe", (fine.ptr, C.byref(fst), None, C.byref(cst), f)),
        ("srcSt", "nz_upsample_stripe", (src.ptr, None, big.ptr, C.byref(fst), f, CR, None)),
        ("dstSt", "nz_downsample_stripe", (fine.ptr, C.byref(fst), big.ptr, None, f)),
        ("dst overlaps src", "nz_upsample", (big.ptr + 4 * (n - 1), res, big.ptr, f, CR, None)),
        ("dst overlaps src", "nz_upsample", (big.ptr, res, big.ptr, f, CR, None)),
        ("dst overlaps src", "nz_downsample", (big.ptr + 4 * (res * res - 1), res * f, big.ptr, f)),
        ("base", "nz_upsample", (src.ptr, res, big.ptr, f, CR, big.ptr + 16)),
        ("base", "nz_upsample", (src.ptr, res, big.ptr, f, CR, big.ptr + 4 * (n - 1))),
        ("base", "nz_upsample_stripe", (src.ptr, C.byref(cst), big.ptr, C.byref(fst), f, CR, big.ptr + 4)),
        # mismatched stripe geometry: cols, grows, and the same the other way round
        ("srcSt", "nz_upsample_stripe", (src.ptr, C.byref(S(res - 1, res, 0, res, 0, res, 0)), big.ptr, C.byref(fst), f, CR, None)),
        ("srcSt", "nz_upsample_stripe", (src.ptr, C.byref(S(res, res, 0, res + 1, 0, res, 0)), big.ptr, C.byref(fst), f, CR, None)),
        ("dstSt", "nz_upsample_stripe", (src.ptr, C.byref(cst), big.ptr, C.byref(fst), 4, CR, None)),
        ("dstSt", "nz_downsample_stripe", (fine.ptr, C.byref(fst), big.ptr, C.byref(S(res, res, 0, res - 1, 0, res - 1, 0)), f)),
        ("pitch", "nz_upsample_stripe", (src.ptr, C.byref(cst), big.ptr, C.byref(S(res * f, res * f, 0, res * f, 0, res * f, res)), f, CR, None)),
    ]
    for name, entry, args in bad:
        with pytest.raises(nj.NoizeError) as e:
            ctx.call(entry, *args)
        assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))
    ctx.synchronize()
    assert_bits(big.ToArray(), sentinel, "dst after the refusals")
    ctx.call("nz_upsample", src.ptr, res, big.ptr, f, CR, None)
    assert_bits(big.ToArray()[:n].reshape(res * f, res * f), R.upsample(plane(res), f, CR), "after the refusals")
    assert_bits(big.ToArray()[n:], sentinel[n:], "beyond dst")
    big.Dispose(); src.Dispose(); fine.Dispose()


# 9. dep / out handles chain with a following stage
def test_handles_chain(nj, ctx):
    res, f = 67, 4
    src = plane(res * f, seed=2)
    s, c, d = ctx.from_host(src), nan_tile(ctx, res * res), nan_tile(ctx, (res * f) ** 2)
    other = nj.Context(0)
    try:
        h1 = ctx.call("nz_downsample", s.ptr, res * f, c.ptr, f)
        assert h1.id != 0
        h2 = other.call("nz_constant_job", 0, c.ptr, None, 2.0, res, dep=h1)       # another context waits on the device
        h3 = ctx.call("nz_upsample", c.ptr, res, d.ptr, f, R.BILINEAR, None, dep=h2)
        h3.Complete()
        assert h1.IsCompleted and h2.IsCompleted and h3.IsCompleted
        coarse = (R.downsample(src, f) * f32(2.0)).astype(f32)
        assert_bits(c.ToArray((res, res)), coarse, "downsample, then the constant stage")
        assert_bits(d.ToArray((res * f, res * f)), R.upsample(coarse, f, R.BILINEAR), "then upsample")
        assert ctx.call("nz_upsample", c.ptr, res, d.ptr, f, R.NEAREST, None, handle=False).id == 0
        ctx.synchronize()
        assert_bits(d.ToArray((res * f, res * f)), R.upsample(coarse, f, R.NEAREST), "no handle: stream order")
    finally:
        other.close()
    s.Dispose(); c.Dispose(); d.Dispose()


# 10. coarse-to-fine, end to end, every step through the C ABI
def test_coarse_to_fine_recipe(nj, ctx):
    res, f, its = 128, 4, 10
    cres = res // f
    prm = PARAMS[1]
    fine = ctx.alloc(res * res)
    ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), fine.ptr, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300)
    tile = fine.ToArray((res, res))
    assert np.isfinite(tile).all() and tile.std() > 0
    coarse, eroded, out = nan_tile(ctx, cres * cres), ctx.alloc(cres * cres), nan_tile(ctx, res * res)
    work = ctx.alloc(nj._native.lib.nz_hydraulic_erosion_work_floats(cres, 1))
    h = ctx.call("nz_downsample", fine.ptr, res, coarse.ptr, f)
    h = ctx.call("nz_flush_write_slice", eroded.ptr, coarse.ptr, cres * cres, dep=h)               # eroded = coarse
    h = ctx.call("nz_hydraulic_erosion_stage", eroded.ptr, work.ptr, its, *prm, cres, dep=h)
    h = ctx.call("nz_reduction_job", int(nj.ReductionType.SUBTRACT), eroded.ptr, coarse.ptr, None, cres, dep=h)
    h = ctx.call("nz_upsample", eroded.ptr, cres, out.ptr, f, R.CATMULL_ROM, fine.ptr, dep=h)
    h.Complete()
    c = R.downsample(tile, f)
    e, _ = H.run(c, its, **dict(zip(NAMES, prm)))
    delta = (e - c).astype(f32)
    assert np.abs(delta).max() > 0, "the erosion changed the coarse tile"
    assert_bits(coarse.ToArray((cres, cres)), c, "downsample")
    assert_bits(eroded.ToArray((cres, cres)), delta, "eroded - coarse")
    assert_bits(out.ToArray((res, res)), R.upsample(delta, f, R.CATMULL_ROM, tile), "the recipe")
    assert_bits(fine.ToArray((res, res)), tile, "the fine tile is only read")
    for t in (fine, coarse, eroded, out, work):
        t.Dispose()


# 11. NoiseStage -> DownsampleStage(2) -> UpsampleStage(2) in a BasePipeline, single tile and batch of 3
def test_stages_in_a_pipeline(nj, ctx):
    res = 64
    noise_args = (nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300)

    def run(payload):
        down, up = nj.DownsampleStage(ctx, 2), nj.UpsampleStage(ctx, 2)
        pipe = nj.BasePipeline([nj.NoiseStage(ctx, *noise_args), down, up], "resample")
        seen, done = [], []
        down.OnStageScheduledAction.insert(0, lambda req, h: seen.append(req.data))  # before the hand-over to `up`
        pipe.Enqueue(payload, completeAction=done.append)
        pipe.RunToCompletion()
        assert len(done) == 1 and len(seen) == 1
        return down, up, pipe, seen[0], done[0]

    d = nj.GeneratorData("t", ctx.alloc(res * res), res, 6, -5)
    down, up, pipe, mid, end = run(d)
    assert type(mid) is nj.GeneratorData and (mid.uuid, mid.resolution, mid.xpos, mid.zpos) == ("t", 32, 3, -3)
    assert mid.data is down.out and mid.data.Length == 32 * 32
    assert type(end) is nj.GeneratorData and (end.uuid, end.resolution, end.xpos, end.zpos) == ("t", 64, 6, -6)
    assert end.data is up.out and end.data.Length == res * res
    noise = d.data.ToArray((res, res))
    c, o = nan_tile(ctx, 32 * 32), nan_tile(ctx, res * res)
    ctx.call("nz_downsample", d.data.ptr, res, c.ptr, 2)
    ctx.call("nz_upsample", c.ptr, 32, o.ptr, 2, R.CATMULL_ROM, None)
    assert_bits(mid.data.ToArray((32, 32)), c.ToArray((32, 32)), "the plane handed downstream")
    assert_bits(end.data.ToArray((res, res)), o.ToArray((res, res)), "the pipeline's result")
    assert_bits(end.data.ToArray((res, res)), R.upsample(R.downsample(noise, 2), 2, R.CATMULL_ROM), "the model")
    pipe.Destroy()
    assert up.out is None and down.out is None
    c.Dispose(); o.Dispose(); d.data.Dispose()

    positions = [(0, 0), (64, -64), (-130, 7)]
    b = nj.GeneratorDataBatch.create(ctx, "b", res, positions)
    down, up, pipe, mid, end = run(b)
    assert type(mid) is nj.GeneratorDataBatch and (mid.resolution, mid.count) == (32, 3) and mid.data is down.out
    assert mid.positions.ToArray().reshape(-1, 2).tolist() == [[0, 0], [32, -32], [-65, 3]]
    assert type(end) is nj.GeneratorDataBatch and (end.resolution, end.count) == (64, 3) and end.data is up.out
    assert end.positions.ToArray().reshape(-1, 2).tolist() == [[0, 0], [64, -64], [-130, 6]]
    got = end.data.ToArray((3, res, res))
    noise = b.data.ToArray((3, res, res))
    for k in range(3):
        single = nj.GeneratorData("s", ctx.alloc(res * res), res, *positions[k])
        _, up1, pipe1, _, end1 = run(single)
        assert_bits(noise[k], single.data.ToArray((res, res)), "noise tile %d" % k)
        assert_bits(got[k], end1.data.ToArray((res, res)), "batch tile %d equals the single tile" % k)
        assert_bits(got[k], R.upsample(R.downsample(noise[k], 2), 2, R.CATMULL_ROM), "batch tile %d: the model" % k)
        pipe1.Destroy()
        single.data.Dispose()
    pipe.Destroy()
    b.data.Dispose(); b.positions.Dispose()


# 12. the quick start's coarse-to-fine recipe through the stages: the erosion works in place, so it runs on a copy of
#     DownsampleStage's plane and the un-eroded plane is still there to subtract
def test_quick_start_recipe_through_the_stages(nj, ctx):
    res, f, its = 128, 4, 10
    cres = res // f
    full = ctx.alloc(res * res)
    ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), full.ptr, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300)
    host = full.ToArray((res, res))
    tile = nj.GeneratorData("t", full, res, 8, -8)
    down = nj.DownsampleStage(ctx, f)
    nj.BasePipeline([down]).Schedule(tile)
    ctx.synchronize()
    assert tile.data is full and tile.resolution == res, "the caller's payload is left as it was"
    eroded = ctx.alloc(down.out.Length)
    ctx.call("nz_flush_write_slice", eroded.ptr, down.out.ptr, eroded.Length)
    coarse = nj.GeneratorData("c", eroded, cres)
    hyd = nj.HydraulicErosionStage(ctx, iterations=its)
    nj.BasePipeline([hyd]).Schedule(coarse)
    ctx.synchronize()
    ctx.call("nz_reduction_job", int(nj.ReductionType.SUBTRACT), eroded.ptr, down.out.ptr, None, cres)
    up = nj.UpsampleStage(ctx, f, nj.ResampleFilter.CatmullRom, base=tile.data)
    nj.BasePipeline([up]).Schedule(coarse)
    ctx.synchronize()
    c = R.downsample(host, f)
    e, _ = H.run(c, its)
    delta = (e - c).astype(f32)
    assert np.abs(delta).max() > 0
    assert_bits(down.out.ToArray((cres, cres)), c, "the un-eroded coarse plane is still there")
    assert_bits(up.out.ToArray((res, res)), R.upsample(delta, f, R.CATMULL_ROM, host), "the recipe through the stages")
    for st in (down, hyd, up):
        st.Destroy()
    full.Dispose(); eroded.Dispose()
