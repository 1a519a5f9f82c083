"""Octave shapes on the GPU (nz_fractal_shaped*, ShapedNoiseStage) against the reference driver of
tests/fractal_shapes_ref.py: shape 0 is nz_fractal bit for bit in every float mode, billow and ridged are the driver bit for
bit in strict mode (Sin: 1e-5, its device sinf), the tolerance modes stay inside the 1e-5 / 1e-6 band, batch and stripe
forms are the single-tile form, and a ridged tile goes through the metric pipeline as the oracle's stages say."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_parity
from fractal_shapes_ref import BILLOW, FBM, RIDGED, fractal_shaped

pytestmark = pytest.mark.gpu
f32 = np.float32
BASES = ["Sin", "Perlin", "PeriodicPerlin", "Simplex", "RotatedSimplex", "Cellular", "DomainRotatedPerlin",
         "DomainRotatedSimplex"]
# (hurst, amp, stepdown, detune, octaves, xpos, zpos, noiseSize): a plain tile, negative coordinates with detune, and a tile
# whose top octaves pass NZ_TAB_LIMIT (2^20: 300 * 4096 > 1.2e6) -- the direct fallback and the guarded octave loop
TILES = [(0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300),
         (0.5938, 1.3, 1.9168, 0.0317, 6, -2100, -777, 97),
         (0.4, 1.0, 2.0, 0.0, 13, 300000, 2000, 1000)]
SHAPES = [(BILLOW, 1.0, 2.0), (RIDGED, 1.0, 2.0), (RIDGED, 0.9, 3.5)]


@pytest.fixture(scope="module", params=[0, 1, 2], ids=["strict", "fast", "relaxed"])
def mctx(nj, request):
    c = nj.Context(0)
    c.float_mode = request.param
    yield c
    c.close()


def plane(ctx, name, basis, res, args, shape=None):
    d = ctx.alloc(res * res)
    hurst, amp, step, det, octv, xp, zp, ns = args
    extra = () if shape is None else shape
    ctx.call(name, basis, d.ptr, res, hurst, amp, step, det, octv, xp, zp, ns, *extra)
    out = d.ToArray((res, res))
    d.Dispose()
    return out


def stripe_rows(ctx, basis, cols, rows, grow0, grows, args, shape, pitch=0):
    """nz_fractal_shaped_stripe on a buffer of `rows` rows, every row owned: world rows grow0 .. grow0 + rows - 1."""
    import noize_job_amd as nj
    pitch = pitch or cols
    d = ctx.alloc(rows * pitch)
    st = nj.Stripe(cols, rows, grow0, grows, 0, rows, pitch)
    hurst, amp, step, det, octv, xp, zp, ns = args
    ctx.call("nz_fractal_shaped_stripe", basis, d.ptr, C.byref(st), hurst, amp, step, det, octv, xp, zp, ns, *shape)
    out = d.ToArray((rows, pitch))[:, :cols]
    d.Dispose()
    return out


def check_strict(got, want, basis, what):
    if basis == 0:  # Sin: device sinf, as in the fBm tests
        assert_parity(got, want, what)
    else:
        assert np.array_equal(got, want), "%s: %d cells differ" % (what, int((got != want).sum()))


# 1. shape 0 through the new entry is nz_fractal, in every float mode
@pytest.mark.parametrize("basis", range(8), ids=BASES)
def test_shape_fbm_is_nz_fractal(mctx, basis):
    for args in TILES:
        want = plane(mctx, "nz_fractal", basis, 61, args)
        got = plane(mctx, "nz_fractal_shaped", basis, 61, args, (FBM, 1.0, 2.0))
        assert np.array_equal(got, want), (BASES[basis], args)


# 2. billow and ridged against the driver, strict
@pytest.mark.parametrize("basis", range(8), ids=BASES)
def test_shapes_match_the_driver(nj, ctx, basis):
    for args in TILES:
        for shape in SHAPES:
            got = plane(ctx, "nz_fractal_shaped", basis, 61, args, shape)
            want = fractal_shaped(basis, 61, 61, *args, shape=shape[0], offset=shape[1], gain=shape[2])
            check_strict(got, want, basis, "%s shape=%s %s" % (BASES[basis], shape, args))


@pytest.mark.parametrize("basis", range(8), ids=BASES)
def test_shapes_odd_rectangle(nj, ctx, basis):
    # 257 x 129 through the stripe entry (one stripe owning the whole grid): partial vectors at the row end
    args = (0.4, 1.0, 2.0, 0.0, 5, -300, 41, 150)
    for shape in SHAPES[:2]:
        got = stripe_rows(ctx, basis, 257, 129, 0, 129, args, shape, pitch=260)
        want = fractal_shaped(basis, 129, 257, *args, shape=shape[0], offset=shape[1], gain=shape[2])
        check_strict(got, want, basis, "%s shape=%s 257x129" % (BASES[basis], shape))


# 3. batch == single calls; stripes == rows of the monolithic plane
@pytest.mark.parametrize("basis", [1, 3, 4, 5, 7], ids=[BASES[b] for b in (1, 3, 4, 5, 7)])
def test_batch_and_stripes_equal_single_tiles(nj, ctx, basis):
    res, pos = 64, [(0, 0), (-4096, 512), (300000, -70000)]
    hurst, amp, step, det, octv, ns = 0.45, 1.0, 2.0, 0.01, 9, 700
    for shape in SHAPES:
        b = nj.GeneratorDataBatch.create(ctx, "b", res, pos)
        ctx.call("nz_fractal_shaped_batch", basis, b.data.ptr, res, len(pos), b.positions.ptr, hurst, amp, step, det, octv,
                 ns, *shape)
        got = b.data.ToArray((len(pos), res, res))
        for k, (xp, zp) in enumerate(pos):
            want = plane(ctx, "nz_fractal_shaped", basis, res, (hurst, amp, step, det, octv, xp, zp, ns), shape)
            assert np.array_equal(got[k], want), (BASES[basis], shape, k)
        # the same batch through the stage
        st = nj.ShapedNoiseStage(ctx, nj.FractalNoise(basis), hurst, amp, octv, step, det, ns, nj.FractalShape(shape[0]),
                                 shape[1], shape[2])
        b2 = nj.GeneratorDataBatch.create(ctx, "b2", res, pos)
        st.ReceiveHandledInput(nj.PipelineWorkItem(b2), nj.JobHandle())
        st.jobHandle.Complete()
        assert np.array_equal(b2.data.ToArray((len(pos), res, res)), got)
        b.data.Dispose(); b2.data.Dispose(); b.positions.Dispose(); b2.positions.Dispose()
        # stripes
        args = (hurst, amp, step, det, octv, pos[1][0], pos[1][1], ns)
        mono = plane(ctx, "nz_fractal_shaped", basis, res, args, shape)
        for g0, g1 in ((0, 23), (23, 64)):
            rows = stripe_rows(ctx, basis, res, g1 - g0, g0, res, args, shape)
            assert np.array_equal(rows, mono[g0:g1]), (BASES[basis], shape, g0)


# 4. the tolerance modes stay inside the band; bases without a tolerance form are exactly strict
@pytest.mark.parametrize("mode", [1, 2], ids=["fast", "relaxed"])
def test_tolerance_modes_stay_in_band(nj, ctx, mode):
    c = nj.Context(0)
    c.float_mode = mode
    try:
        worst = 0.0
        for basis in range(8):
            for args in TILES:
                for shape in SHAPES:
                    strict = plane(ctx, "nz_fractal_shaped", basis, 61, args, shape)
                    got = plane(c, "nz_fractal_shaped", basis, 61, args, shape)
                    assert_parity(got, strict, "%s mode=%d shape=%s %s" % (BASES[basis], mode, shape, args))
                    if basis != 3:  # only the simplex kernel has a tolerance form
                        assert np.array_equal(got, strict), (BASES[basis], shape, args)
                    worst = max(worst, float(np.abs(got.astype(np.float64) - strict).max()))
        print("mode %d: largest difference from strict %.3g" % (mode, worst))
    finally:
        c.close()


# 5. the metric's size: 4096^2, simplex, 13 octaves, ridged; sampled rows against the driver
def test_ridged_4096_sampled_rows(nj, ctx):
    R, args = 4096, (0.4, 1.0, 2.0, 0.0, 13, 4096 * 3, 4096 * 5, 1700)
    got = plane(ctx, "nz_fractal_shaped", 3, R, args, (RIDGED, 1.0, 2.0))
    rows = [0, 1, 1777, 2048, 4095]
    want = fractal_shaped(3, R, R, *args, shape=RIDGED, row_ids=rows)
    assert np.array_equal(got[rows], want)
    assert np.isfinite(got).all() and got.min() >= 0.0


# 6. ShapedNoiseStage(Ridged) -> Gauss5 x17 -> FlowMap x5 -> erosion x5 == the oracle's stages on the driver's plane; on a
#    single plane and on a READ / WRITE pair
def test_ridged_pipeline_matches_oracle_stages(nj, ctx, oracle):
    res, xp, zp = 160, 4096, -2048
    args = (0.4, 1.0, 2.0, 0.0, 13, xp, zp, 1700)
    noise = fractal_shaped(3, res, res, *args, shape=RIDGED)
    want = oracle.erosion_min(oracle.flowmap(oracle.kernel_filter(noise, oracle.GAUSS5_S1, 17), 5, 0.0, 0.005), 5)
    for rw in (False, True):
        stages = [nj.ShapedNoiseStage(ctx, nj.FractalNoise.Simplex, 0.4, 1.0, 13, 2.0, 0.0, 1700, nj.FractalShape.Ridged),
                  nj.KernelFilterStage(ctx, nj.KernelFilterType.Gauss5_S1, 17),
                  nj.FlowMapStage(ctx, 5, 0.0, 0.005),
                  nj.ErosionStage(ctx, 5)]
        pipe = nj.BasePipeline(stages, "ridged")
        d = nj.GeneratorData("r", ctx.alloc(res * res), res, xp, zp, write=ctx.alloc(res * res) if rw else None)
        done = []
        pipe.Enqueue(d, completeAction=done.append)
        pipe.RunToCompletion()
        assert len(done) == 1
        got = d.data.ToArray((res, res))
        assert np.array_equal(got, want), "rw=%s: %d cells differ" % (rw, int((got != want).sum()))
        pipe.Destroy()


# 7. an unknown shape is NZ_ERR_INVALID and writes nothing
def test_invalid_shape_writes_nothing(nj, ctx):
    res = 32
    sentinel = np.full((res, res), 7.25, f32)
    d = ctx.from_host(sentinel)
    pos = ctx.from_host(np.zeros(2, np.int32))
    st = nj.Stripe(res, res, 0, res, 0, res, 0)
    for shape in (-1, 3, 1 << 20):
        calls = [("nz_fractal_shaped", (3, d.ptr, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300)),
                 ("nz_fractal_shaped_batch", (3, d.ptr, res, 1, pos.ptr, 0.4, 1.0, 2.0, 0.0, 8, 300)),
                 ("nz_fractal_shaped_stripe", (3, d.ptr, C.byref(st), 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300))]
        for name, a in calls:
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(name, *a, shape, 1.0, 2.0)
            assert e.value.status == nj._native.NZ_ERR_INVALID and "shape" in str(e.value), (name, shape)
    ctx.synchronize()
    assert np.array_equal(d.ToArray((res, res)), sentinel)
    # the context is still usable
    ctx.call("nz_fractal_shaped", 3, d.ptr, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300, RIDGED, 1.0, 2.0)
    assert np.array_equal(d.ToArray((res, res)), fractal_shaped(3, res, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300, shape=RIDGED))
    d.Dispose(); pos.Dispose()
