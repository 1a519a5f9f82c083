"""Every convolution launch form, in every float mode, bit for bit against the numpy restatement of its mode.

tests/conv_ref.py restates the reference's tap sums twice: STRICT (`t = +0; t = t + v * k` per tap, then `* factor`) and
FAST (each `t + v * k` contracted to `fmaf(v, k, t)`).  A context in NZ_FLOAT_STRICT must give the first, NZ_FLOAT_FAST and
NZ_FLOAT_RELAXED the second -- whatever launch form runs: the register tiles (BIG 512 x 8 / 256 x 8, SMALL 512 x 4, TINY
1024 x 2), chained or separate, the row-streaming kernel, the wide kernels of 11..25 taps, the generic X / Z passes of even
sizes, their UNIT (factor 1) and scaled forms, batched, stripe and READ / WRITE geometries.  Comparisons are on the bit
patterns (assert_bits_equal): the sign of a zero counts.  FAST and RELAXED results must also stay within 1e-5 relative
(1e-6 absolute) of STRICT.

Sizes select the forms by the default rules of nz_filter.hip / nz_stages.cpp: 300^2 = TINY for 5 taps, SMALL for 7 and 9,
BIG for 3; 1030^2 SMALL for 5; 2712^2 BIG (>= 7 M cells, 3+ launches chained, 2 separate); a grid of 40 M cells or more
streams (3 and 5 taps).  Planes above 2048^2 are restated in row bands (conv_ref.banded)."""
import ctypes as C

import numpy as np
import pytest

import conv_ref as R
from conftest import adversarial_tiles

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = {"strict": 0, "fast": 1, "relaxed": 2}
CAP = {3: 6, 5: 5, 7: 3, 9: 3}  # fusion depth per launch (conv_tcap); 5 taps: 6 on SMALL grids, 9 on TINY ones
KSIZE = {0: 9, 1: 7, 2: 5, 3: 3, 4: 9, 5: 7, 6: 5, 7: 3, 8: 3, 9: 3, 10: 3, 11: 3, 12: 3, 13: 3}

_memo = {}


def restated(key, fast, fn):
    """fn(fast), memoised per module: FAST and RELAXED share one restatement, and the strict one serves as their bar."""
    if (key, fast) not in _memo:
        _memo[(key, fast)] = fn(fast)
    return _memo[(key, fast)]


def check(mode, got, key, fn, what):
    fast = mode > 0
    R.assert_bits_equal(got, restated(key, fast, fn), "%s [mode %d]" % (what, mode))
    if fast:
        R.assert_within(got, restated(key, False, fn), "%s [mode %d] against strict" % (what, mode))


@pytest.fixture(scope="module", params=list(MODES.values()), ids=list(MODES))
def mctx(nj, request):
    c = nj.Context(0)
    c.float_mode = request.param
    assert c.float_mode == request.param
    yield c
    c.close()


def _run(ctx, name, plane, *args):
    """An in-place entry (src, tmp, *args) on a copy of `plane`; returns the result."""
    src, tmp = ctx.from_host(plane), ctx.alloc(plane.size)
    try:
        ctx.call(name, src.ptr, tmp.ptr, *args).Complete()
        return src.ToArray(plane.shape)
    finally:
        src.Dispose()
        tmp.Dispose()


def _bands(rows, mid=64):
    """top border, an interior band (64 rows: it crosses a tile seam of every launch depth), bottom border"""
    return [(0, 16), (rows // 2 - mid // 2, rows // 2 + mid // 2), (rows - 16, rows)]


def _signed(rng, shape, scale=8.0):
    return ((rng.random(shape, dtype=f32) - f32(0.3)) * f32(scale)).astype(f32)


def _counts(ft, res):
    ks = KSIZE[ft]
    if ft == R.SOBEL3_2D:
        return (1, 2, 3)
    cap = CAP[ks]
    if ks == 5 and res * res < 7 * 1024 * 1024:
        cap = 9 if res * res <= 600 * 1024 else 6
    return tuple(sorted({1, cap, cap + 1, 17, 32}))


# ---- KernelFilterStage: every filter type, iteration counts across the fusion caps, every tile shape ------------------
@pytest.mark.parametrize("ft", range(14))
def test_filter_stage_small_grids(nj, mctx, ft):
    mode = mctx.float_mode
    for res in (300, 301):
        t = _signed(np.random.default_rng(100 + ft), (res, res))
        counts = _counts(ft, res) if res == 300 else _counts(ft, res)[1:3]
        fn = lambda fast, t=t, counts=counts: R.filter_apply(t, ft, max(counts), fast=fast, record=counts)[1]  # noqa: E731
        for it in counts:
            got = _run(mctx, "nz_kernel_filter_stage", t, ft, it, res)
            R.assert_bits_equal(got, restated(("filter", ft, res), mode > 0, fn)[it], "ft=%d x%d %d^2 [mode %d]" % (ft, it, res, mode))
            if mode:
                R.assert_within(got, restated(("filter", ft, res), False, fn)[it], "ft=%d x%d %d^2 against strict" % (ft, it, res))


@pytest.mark.parametrize("ft,res,counts", [(2, 1030, (1, 6, 7, 17)),        # 5 taps, SMALL: chained from 2 launches
                                           (2, 2712, (1, 6, 17)),           # BIG: one launch, two separate, chained
                                           (1, 2712, (1, 4, 10)),
                                           (4, 2712, (3, 4, 10)),
                                           (3, 2712, (6, 7, 17))],          # 3 taps: separate launches only
                         ids=["g5-1030", "g5-2712", "g7-2712", "g9s2-2712", "g3-2712"])
def test_filter_stage_large_grids(nj, mctx, ft, res, counts):
    mode = mctx.float_mode
    t = _signed(np.random.default_rng(ft * 7 + res), (res, res))
    reach = max(counts) * ((KSIZE[ft] - 1) // 2)
    bands = _bands(res)

    def fn(fast):
        kx, kz, fac = R.filter_taps(ft)
        out = {c: [] for c in counts}
        for _, _, b in R.banded(lambda a: np.stack([v for _, v in sorted(
                R.separable(a, kx, kz, fac, max(counts), fast=fast, record=counts)[1].items())]), t, reach, bands):
            for i, c in enumerate(sorted(counts)):
                out[c].append(b[i])
        return out

    for it in counts:
        got = _run(mctx, "nz_kernel_filter_stage", t, ft, it, res)
        for (r0, r1), want, strict in zip(bands, restated(("large", ft, res), mode > 0, fn)[it],
                                          restated(("large", ft, res), False, fn)[it]):
            R.assert_bits_equal(got[r0:r1], want, "ft=%d x%d %d^2 rows %d..%d [mode %d]" % (ft, it, res, r0, r1, mode))
            if mode:
                R.assert_within(got[r0:r1], strict, "ft=%d x%d %d^2 rows %d..%d against strict" % (ft, it, res, r0, r1))


def test_single_grid_streaming(nj, mctx):
    # 6656^2 = 44 M cells: Gauss5 x17 runs the row-streaming kernel (launches of 5 + 4 + 4 + 4)
    mode, res, it = mctx.float_mode, 6656, 17
    t = _signed(np.random.default_rng(6656), (res, res))
    kx, kz, fac = R.filter_taps(2)
    bands = _bands(res)
    fn = lambda fast: [b for _, _, b in R.banded(  # noqa: E731
        lambda a: R.separable(a, kx, kz, fac, it, fast=fast), t, it * 2, bands)]
    got = _run(mctx, "nz_kernel_filter_stage", t, 2, it, res)
    for (r0, r1), want, strict in zip(bands, restated("stream", mode > 0, fn), restated("stream", False, fn)):
        R.assert_bits_equal(got[r0:r1], want, "stream rows %d..%d [mode %d]" % (r0, r1, mode))
        if mode:
            R.assert_within(got[r0:r1], strict, "stream rows %d..%d against strict" % (r0, r1))
    # the signed-zero planes through the same form: every cell is the constant the restatement gives a small plane
    for name in ("neg_zero", "neg_denormal"):
        z = R.signed_zero_tiles(res)[name]
        got = _run(mctx, "nz_kernel_filter_stage", z, 2, it, res)
        want = R.separable(R.signed_zero_tiles(8)[name], kx, kz, fac, it, fast=mode > 0)[0, 0]
        R.assert_bits_equal(got, np.full_like(got, want), "stream %s [mode %d]" % (name, mode))


# ---- blur stages: every width, the wide kernels, the generic passes of even sizes -------------------------------------
@pytest.mark.parametrize("width", range(1, 26))
def test_blur_stages_every_width(nj, mctx, width):
    mode = mctx.float_mode
    sigma = width % 16
    for res, it in ((300, 2), (301, 1)):
        t = _signed(np.random.default_rng(width * 1000 + res), (res, res))
        for kind in ("gauss", "smooth"):
            kx, kz, fac = R.blur_taps(kind, width, sigma)
            fn = lambda fast, t=t, kx=kx, kz=kz, fac=fac, it=it: R.separable(t, kx, kz, fac, it, ksize=width, fast=fast)  # noqa: E731
            if kind == "gauss":
                got = _run(mctx, "nz_gauss_blur_stage", t, width, sigma, it, res)
            else:
                got = _run(mctx, "nz_smooth_blur_stage", t, width, it, res)
            check(mode, got, ("blur", kind, width, res), fn, "%s width %d x%d %d^2" % (kind, width, it, res))


# ---- custom kernels: asymmetric taps, negative factor, one application per kernel family -------------------------------
@pytest.mark.parametrize("ksize", [3, 4, 5, 7, 9, 11, 12, 17, 25])
def test_separable_series_asymmetric_kernels(nj, mctx, ksize):
    mode = mctx.float_mode
    rng = np.random.default_rng(ksize)
    kx = (rng.random(ksize) * 2 - 0.6).astype(f32)
    kz = (rng.random(ksize) * 1.5 - 0.2).astype(f32)
    assert not np.array_equal(kx, kx[::-1]) and not np.array_equal(kz, kz[::-1])
    for res in (300, 301):
        t = _signed(rng, (res, res))
        for factor in (0.37, -1.7):
            src, tmp = mctx.from_host(t), mctx.alloc(res * res)
            mctx.call("nz_separable_series", src.ptr, tmp.ptr, res, ksize, kx.ctypes.data_as(nj._native.f32p),
                      kz.ctypes.data_as(nj._native.f32p), factor).Complete()
            got = src.ToArray((res, res))
            src.Dispose()
            tmp.Dispose()
            fn = lambda fast, t=t, factor=factor: R.separable(t, kx, kz, factor, ksize=ksize, fast=fast)  # noqa: E731
            what = "series k=%d f=%g %d^2 [mode %d]" % (ksize, factor, res, mode)
            R.assert_bits_equal(got, restated(("series", ksize, res, factor), mode > 0, fn), what)
            # mixed-sign taps on a mixed-sign plane cancel: 1e-5 of strict is not a bar either fp32 sequence meets (a few cells
            # of every size miss it, in both directions).  Both are held to the float64 operation's a-priori bound instead.
            exact, bound = restated(("series64", ksize, res, factor), None,
                                    lambda _, t=t, factor=factor: R.separable64(t, kx, kz, factor, ksize=ksize))
            err = np.abs(got.astype(np.float64) - exact)
            assert (err <= bound).all(), "%s: %d cells outside the float64 bound" % (what, int((err > bound).sum()))


# ---- batched entries ------------------------------------------------------------------------------------------------
def _batch(ctx, name, planes, *args):
    count, res = planes.shape[0], planes.shape[1]
    src, tmp = ctx.from_host(planes), ctx.alloc(planes.size)
    try:
        ctx.call(name, src.ptr, tmp.ptr, *args, res, count).Complete()
        return src.ToArray(planes.shape)
    finally:
        src.Dispose()
        tmp.Dispose()


def test_batched_big_tiles(nj, mctx):
    # the README's batch: 64 x 512^2 = 16.8 M cells, so the batch runs the BIG shape; each tile alone runs TINY
    mode, res, count, it = mctx.float_mode, 512, 64, 2
    planes = _signed(np.random.default_rng(64), (count, res, res))
    kx, kz, fac = R.filter_taps(2)
    fn = lambda fast: R.separable(planes, kx, kz, fac, it, fast=fast)  # noqa: E731
    got = _batch(mctx, "nz_kernel_filter_stage_batch", planes, 2, it)
    check(mode, got, "batch64", fn, "64 x 512^2 Gauss5 x2")
    for k in (0, 1, 31, 62, 63):
        R.assert_bits_equal(got[k], _run(mctx, "nz_kernel_filter_stage", planes[k], 2, it, res), "tile %d alone" % k)


@pytest.mark.parametrize("ft", [2, 3])
def test_batched_streaming(nj, mctx, ft):
    # 4 x 3300^2 = 43.6 M cells: the batch streams (conv_stream_kernel with blockIdx.y > 0); each tile alone runs BIG tiles
    mode, res, count, it = mctx.float_mode, 3300, 4, 7
    planes = _signed(np.random.default_rng(3300 + ft), (count, res, res))
    kx, kz, fac = R.filter_taps(ft)
    bands = _bands(res)
    fn = lambda fast: [b for _, _, b in R.banded(  # noqa: E731
        lambda a: R.separable(a, kx, kz, fac, it, fast=fast), planes, it * ((KSIZE[ft] - 1) // 2), bands)]
    got = _batch(mctx, "nz_kernel_filter_stage_batch", planes, ft, it)
    for (r0, r1), want, strict in zip(bands, restated(("bstream", ft), mode > 0, fn), restated(("bstream", ft), False, fn)):
        R.assert_bits_equal(got[:, r0:r1], want, "batch stream ft=%d rows %d..%d [mode %d]" % (ft, r0, r1, mode))
        if mode:
            R.assert_within(got[:, r0:r1], strict, "batch stream ft=%d rows %d..%d against strict" % (ft, r0, r1))
    for k in (0, count - 1):
        R.assert_bits_equal(got[k], _run(mctx, "nz_kernel_filter_stage", planes[k], ft, it, res), "tile %d alone" % k)


def test_batched_small_odd_counts(nj, mctx):
    mode, res = mctx.float_mode, 301
    rng = np.random.default_rng(301)
    cases = [("nz_kernel_filter_stage_batch", (0, 4), ("filter", 0), 4, 3),      # 9 taps SMALL, chained
             ("nz_kernel_filter_stage_batch", (8, 7), ("filter", 8), 7, 5),      # Smooth3: 3 taps, factor 1/3
             ("nz_kernel_filter_stage_batch", (6, 10), ("filter", 6), 10, 3),   # 5 taps, batch of 0.27 M cells: TINY
             ("nz_gauss_blur_stage_batch", (13, 5, 2), ("gauss", 13, 5), 2, 3),  # wide kernel
             ("nz_smooth_blur_stage_batch", (4, 1), ("smooth", 4), 1, 5)]        # even size: generic passes grid by grid
    for name, args, what, it, count in cases:
        planes = _signed(rng, (count, res, res))
        if what[0] == "filter":
            fn = lambda fast, p=planes, ft=what[1], it=it: R.filter_apply(p, ft, it, fast=fast)  # noqa: E731
            single = ("nz_kernel_filter_stage", args + (res,))
        else:
            kx, kz, fac = R.blur_taps(what[0], what[1], what[2] if what[0] == "gauss" else 0)
            fn = lambda fast, p=planes, kx=kx, kz=kz, it=it, w=what[1]: R.separable(p, kx, kz, 1.0, it, ksize=w, fast=fast)  # noqa: E731
            single = (name.replace("_batch", ""), args + (res,))
        got = _batch(mctx, name, planes, *args)
        check(mode, got, ("small-batch",) + what, fn, "%s %s x%d" % (name, what, count))
        for k in range(count):
            R.assert_bits_equal(got[k], _run(mctx, single[0], planes[k], *single[1]), "%s tile %d alone" % (what, k))


# ---- stripes and READ / WRITE pairs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ft,T", [(2, 5), (3, 6), (0, 3), (8, 4), (9, 2)])
def test_stripes_with_ghost_rows(nj, mctx, ft, T):
    mode, grows, cols, pitch = mctx.float_mode, 203, 130, 137
    grid = _signed(np.random.default_rng(ft + 17 * T), (grows, cols))
    want = restated(("stripe", ft, T), mode > 0, lambda fast: R.filter_apply(grid, ft, T, fast=fast))
    halo = nj._native.lib.nz_kernel_filter_halo_rows(ft, T)
    # a stripe at each border and one inside; each buffer carries ghost rows beyond its own rows where the grid has them
    for g0, g1 in ((0, 70), (70, 140), (140, grows)):
        b0, b1 = max(0, g0 - halo - 2), min(grows, g1 + halo + 3)
        buf = np.full((b1 - b0, pitch), np.nan, f32)
        buf[:, :cols] = grid[b0:b1]
        src, dst = mctx.from_host(buf), mctx.from_host(np.full(buf.shape, np.nan, f32))
        st = nj.Stripe(cols, b1 - b0, b0, grows, g0 - b0, g1 - b0, pitch)
        mctx.call("nz_kernel_filter_stripe", src.ptr, dst.ptr, C.byref(st), ft, T).Complete()
        out = dst.ToArray(buf.shape)
        src.Dispose()
        dst.Dispose()
        R.assert_bits_equal(out[g0 - b0:g1 - b0, :cols], want[g0:g1], "stripe ft=%d T=%d rows %d..%d [mode %d]" % (ft, T, g0, g1, mode))
        assert np.isnan(out[:g0 - b0]).all() and np.isnan(out[g1 - b0:]).all() and np.isnan(out[:, cols:]).all()


def test_read_write_pair_entries(nj, mctx):
    mode, res = mctx.float_mode, 300
    t = _signed(np.random.default_rng(77), (res, res))
    g13 = R.blur_taps("gauss", 13, 4)
    s4 = R.blur_taps("smooth", 4)
    cases = [(nj.KernelFilterStage(mctx, nj.KernelFilterType.Gauss5_S1, 17), ("rw", 2, 17),
              lambda fast: R.filter_apply(t, 2, 17, fast=fast)),
             (nj.KernelFilterStage(mctx, nj.KernelFilterType.Smooth3, 3), ("rw", 8, 3),
              lambda fast: R.filter_apply(t, 8, 3, fast=fast)),
             (nj.StageGaussianBlur(mctx, 3, nj.GaussSigma(4), 13), ("rw-g13",),
              lambda fast: R.separable(t, g13[0], g13[1], 1.0, 3, fast=fast)),
             (nj.StageSmoothBlur(mctx, 2, 3), ("rw-s3",), lambda fast: R.separable(t, *R.blur_taps("smooth", 3), 2, fast=fast))]
    for stage, key, fn in cases:
        data, write = mctx.from_host(t), mctx.alloc(res * res)
        gd = nj.GeneratorData("rw", data, res, 0, 0, write=write)
        stage.ReceiveHandledInput(nj.PipelineWorkItem(gd), nj.JobHandle())
        stage.jobHandle.Complete()
        check(mode, gd.data.ToArray((res, res)), key, fn, "READ / WRITE %s" % (key,))
        data.Dispose()
        write.Dispose()
    # even kernelSize through the pair: the generic passes
    data, write = mctx.from_host(t), mctx.alloc(res * res)
    tile = nj._native.RWTile(data.ptr, write.ptr, res, 1)
    mctx.call("nz_smooth_blur_stage_rw", C.byref(tile), 4, 2).Complete()
    out = mctx.wrap(tile.read, res * res).ToArray((res, res))
    check(mode, out, ("rw-s4",), lambda fast: R.separable(t, s4[0], s4[1], 1.0, 2, ksize=4, fast=fast), "READ / WRITE smooth 4")
    data.Dispose()
    write.Dispose()


# ---- edge tiles: adversarial planes, signed zeros, non-finite cells -------------------------------------------------
def _edge_tiles(res):
    tiles = dict(adversarial_tiles(res))
    tiles.update(R.signed_zero_tiles(res))
    t = np.random.default_rng(res).random((res, res), dtype=f32)
    t[3, 5], t[res // 2, 0], t[-1, -1], t[0, res // 3] = np.nan, np.inf, -np.inf, np.nan
    tiles["non_finite"] = t
    return tiles


@pytest.mark.parametrize("res", [64, 301])
def test_edge_tiles(nj, mctx, res):
    mode = mctx.float_mode
    # (entry, args, restatement) per launch form: TINY 5 taps, 3 taps, Smooth3 (factor 1/3), SMALL 9 taps, wide, generic
    forms = [("nz_kernel_filter_stage", (2, 3), lambda t, fast: R.filter_apply(t, 2, 3, fast=fast)),
             ("nz_kernel_filter_stage", (7, 2), lambda t, fast: R.filter_apply(t, 7, 2, fast=fast)),
             ("nz_kernel_filter_stage", (8, 1), lambda t, fast: R.filter_apply(t, 8, 1, fast=fast)),
             ("nz_kernel_filter_stage", (0, 4), lambda t, fast: R.filter_apply(t, 0, 4, fast=fast)),
             ("nz_kernel_filter_stage", (11, 1), lambda t, fast: R.filter_apply(t, 11, 1, fast=fast)),
             ("nz_gauss_blur_stage", (13, 3, 1), lambda t, fast: R.separable(t, *R.blur_taps("gauss", 13, 3), fast=fast)),
             ("nz_smooth_blur_stage", (4, 1), lambda t, fast: R.separable(t, *R.blur_taps("smooth", 4), ksize=4, fast=fast))]
    for name, t in _edge_tiles(res).items():
        for entry, args, fn in forms:
            got = _run(mctx, entry, t, *args, res)
            check(mode, got, ("edge", res, name, entry, args), lambda fast, t=t, fn=fn: fn(t, fast),
                  "%s%s %s %d^2" % (entry, args, name, res))


@pytest.mark.parametrize("ksize", [3, 5, 12, 13])
def test_zeros_under_all_negative_taps(nj, mctx, ksize):
    # every product of a +0 plane under negative taps is -0: the sum is +0, and a negative factor makes it -0
    mode, res = mctx.float_mode, 300
    k = -(np.arange(ksize, dtype=f32) + f32(1)) / f32(ksize * ksize)
    for name, t in R.signed_zero_tiles(res).items():
        for factor in (1.0, -1.0, 0.5):
            src, tmp = mctx.from_host(t), mctx.alloc(res * res)
            mctx.call("nz_separable_series", src.ptr, tmp.ptr, res, ksize, k.ctypes.data_as(nj._native.f32p),
                      k.ctypes.data_as(nj._native.f32p), factor).Complete()
            got = src.ToArray((res, res))
            src.Dispose()
            tmp.Dispose()
            check(mode, got, ("negtaps", ksize, name, factor),
                  lambda fast, t=t, factor=factor: R.separable(t, k, k, factor, ksize=ksize, fast=fast),
                  "negative taps k=%d f=%g %s" % (ksize, factor, name))
