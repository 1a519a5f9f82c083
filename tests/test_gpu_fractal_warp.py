"""Domain warp on the GPU (nz_fractal_warped*, WarpedNoiseStage) against the reference driver of tests/fractal_warp_ref.py:
no warp is nz_fractal_shaped bit for bit in every float mode, a warped tile is the driver bit for bit in strict mode (Sin:
1e-5, its device sinf), the tolerance modes stay inside the 1e-5 band of strict, batch / stripe / stage forms are the
single-tile form, adjacent tiles agree on their shared cells, and a warped tile goes through the metric pipeline as the
oracle's stages say."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import assert_parity
from fractal_shapes_ref import BILLOW, FBM, RIDGED
from fractal_warp_ref import fractal_warped

pytestmark = pytest.mark.gpu
f32 = np.float32
BASES = ["Sin", "Perlin", "PeriodicPerlin", "Simplex", "RotatedSimplex", "Cellular", "DomainRotatedPerlin",
         "DomainRotatedSimplex"]
# (hurst, amp, stepdown, detune, octaves, xpos, zpos, noiseSize): a plain tile, negative coordinates with detune, and a tile
# whose top octaves pass NZ_TAB_LIMIT (2^20: 300 * 4096 > 1.2e6) -- the guarded octave loop
TILES = [(0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300),
         (0.5938, 1.3, 1.9168, 0.0317, 6, -2100, -777, 97),
         (0.4, 1.0, 2.0, 0.0, 13, 300000, 2000, 1000)]
WARPS = [(37.5, 1.0, 3), (-200.0, 0.25, 2)]  # (warpStrength, warpScale, warpOctaves)
RES = 40


@pytest.fixture(scope="module", params=[0, 1, 2], ids=["strict", "fast", "relaxed"])
def mctx(nj, request):
    c = nj.Context(0)
    c.float_mode = request.param
    yield c
    c.close()


def plane(ctx, name, basis, res, args, extra=()):
    d = ctx.alloc(res * res)
    ctx.call(name, basis, d.ptr, res, *args, *extra)
    out = d.ToArray((res, res))
    d.Dispose()
    return out


def warped(ctx, basis, res, args, shape, warp):
    return plane(ctx, "nz_fractal_warped", basis, res, args, (shape, 1.0, 2.0) + tuple(warp))


def driver(basis, rows, cols, args, shape, warp, row_ids=None):
    return fractal_warped(basis, rows, cols, *args, shape=shape, warp_strength=warp[0], warp_scale=warp[1],
                          warp_octaves=warp[2], row_ids=row_ids)


def stripe_rows(ctx, basis, cols, rows, grow0, grows, args, shape, warp, pitch=0):
    """nz_fractal_warped_stripe on a buffer of `rows` rows, every row owned: world rows grow0 .. grow0 + rows - 1."""
    import noize_job_amd as nj
    pitch = pitch or cols
    d = ctx.alloc(rows * pitch)
    st = nj.Stripe(cols, rows, grow0, grows, 0, rows, pitch)
    ctx.call("nz_fractal_warped_stripe", basis, d.ptr, C.byref(st), *args, shape, 1.0, 2.0, *warp)
    out = d.ToArray((rows, pitch))[:, :cols]
    d.Dispose()
    return out


def check_strict(got, want, basis, what):
    if basis == 0:  # Sin: device sinf
        assert_parity(got, want, what)
    else:
        assert np.array_equal(got, want), "%s: %d cells differ" % (what, int((got != want).sum()))


# 1. no warp (strength 0 or no displacement octaves) is nz_fractal_shaped, in every float mode
@pytest.mark.parametrize("basis", range(8), ids=BASES)
def test_no_warp_is_nz_fractal_shaped(mctx, basis):
    for args in TILES:
        for shape in (FBM, BILLOW, RIDGED):
            want = plane(mctx, "nz_fractal_shaped", basis, RES, args, (shape, 1.0, 2.0))
            for warp in ((0.0, 1.0, 4), (37.5, 0.25, 0), (-0.0, 2.0, 3)):
                got = warped(mctx, basis, RES, args, shape, warp)
                assert np.array_equal(got, want), (BASES[basis], args, shape, warp)


# 2. warped tiles against the driver, strict; Sin held to the 1e-5 band at a small strength
@pytest.mark.parametrize("basis", range(1, 8), ids=BASES[1:])
def test_warp_matches_the_driver(nj, ctx, basis):
    for args in TILES:
        for shape in (FBM, RIDGED):
            for warp in WARPS:
                got = warped(ctx, basis, RES, args, shape, warp)
                want = driver(basis, RES, RES, args, shape, warp)
                check_strict(got, want, basis, "%s shape=%d warp=%s %s" % (BASES[basis], shape, warp, args))
    # the displacement's own octaves past NZ_TAB_LIMIT (its guarded loop): 13 octaves at warpScale 1 on the far tile
    warp = (37.5, 1.0, 13)
    got = warped(ctx, basis, RES, TILES[2], FBM, warp)
    check_strict(got, driver(basis, RES, RES, TILES[2], FBM, warp), basis, "%s far displacement" % BASES[basis])


def test_sin_warp_within_band(nj, ctx):
    worst = 0.0
    for args in TILES:
        for shape in (FBM, RIDGED):
            for warp in ((8.0, 1.0, 3), (-6.0, 0.25, 2)):
                got = warped(ctx, 0, RES, args, shape, warp)
                want = driver(0, RES, RES, args, shape, warp)
                assert_parity(got, want, "Sin shape=%d warp=%s %s" % (shape, warp, args))
                worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    print("Sin: largest difference from the driver %.3g" % worst)


# 3. an odd rectangle through the stripe entry, row pitch 260
@pytest.mark.parametrize("basis", [1, 2, 3, 5, 7], ids=[BASES[b] for b in (1, 2, 3, 5, 7)])
def test_warp_odd_rectangle(nj, ctx, basis):
    args = (0.4, 1.0, 2.0, 0.0, 5, -300, 41, 150)
    warp = (37.5, 0.25, 2)
    got = stripe_rows(ctx, basis, 257, 129, 0, 129, args, RIDGED, warp, pitch=260)
    want = driver(basis, 129, 257, args, RIDGED, warp)
    check_strict(got, want, basis, "%s 257x129" % BASES[basis])


# 4. batch == single calls == the stage; stripes == rows of the monolithic plane
@pytest.mark.parametrize("basis", [1, 3, 5, 7], ids=[BASES[b] for b in (1, 3, 5, 7)])
def test_batch_stage_and_stripes_equal_single_tiles(nj, ctx, basis):
    res, pos = 64, [(0, 0), (-4096, 512), (300000, -70000)]
    hurst, amp, step, det, octv, ns = 0.45, 1.0, 2.0, 0.01, 9, 700
    for shape, warp in ((FBM, (37.5, 1.0, 3)), (RIDGED, (-200.0, 0.25, 2))):
        b = nj.GeneratorDataBatch.create(ctx, "b", res, pos)
        ctx.call("nz_fractal_warped_batch", basis, b.data.ptr, res, len(pos), b.positions.ptr, hurst, amp, step, det, octv,
                 ns, shape, 1.0, 2.0, *warp)
        got = b.data.ToArray((len(pos), res, res))
        for k, (xp, zp) in enumerate(pos):
            want = warped(ctx, basis, res, (hurst, amp, step, det, octv, xp, zp, ns), shape, warp)
            assert np.array_equal(got[k], want), (BASES[basis], shape, k)
        st = nj.WarpedNoiseStage(ctx, nj.FractalNoise(basis), hurst, amp, octv, step, det, ns, nj.FractalShape(shape),
                                 warpStrength=warp[0], warpScale=warp[1], warpOctaves=warp[2])
        b2 = nj.GeneratorDataBatch.create(ctx, "b2", res, pos)
        st.ReceiveHandledInput(nj.PipelineWorkItem(b2), nj.JobHandle())
        st.jobHandle.Complete()
        assert np.array_equal(b2.data.ToArray((len(pos), res, res)), got)
        b.data.Dispose(); b2.data.Dispose(); b.positions.Dispose(); b2.positions.Dispose()
        args = (hurst, amp, step, det, octv, pos[1][0], pos[1][1], ns)
        mono = warped(ctx, basis, res, args, shape, warp)
        for g0, g1 in ((0, 23), (23, 64)):
            rows = stripe_rows(ctx, basis, res, g1 - g0, g0, res, args, shape, warp)
            assert np.array_equal(rows, mono[g0:g1]), (BASES[basis], shape, g0)


# 5. world coordinates: adjacent tiles agree on their shared column and row
@pytest.mark.parametrize("basis", [1, 3, 5, 6], ids=[BASES[b] for b in (1, 3, 5, 6)])
def test_tile_seams(nj, ctx, basis):
    res, warp = 64, (-200.0, 0.25, 4)
    base = (0.4, 1.0, 2.0, 0.0, 8)
    t00 = warped(ctx, basis, res, base + (0, 0, 300), RIDGED, warp)
    t10 = warped(ctx, basis, res, base + (63, 0, 300), RIDGED, warp)
    t01 = warped(ctx, basis, res, base + (0, 63, 300), RIDGED, warp)
    assert np.array_equal(t00[:, 63], t10[:, 0])
    assert np.array_equal(t00[63, :], t01[0, :])


# 6. the tolerance modes stay inside the band; bases without a tolerance form are exactly strict
@pytest.mark.parametrize("mode", [1, 2], ids=["fast", "relaxed"])
def test_tolerance_modes_stay_in_band(nj, ctx, mode):
    c = nj.Context(0)
    c.float_mode = mode
    try:
        worst = 0.0
        for basis in range(8):
            for args in TILES:
                for shape in (FBM, BILLOW, RIDGED):
                    for warp in WARPS:
                        strict = warped(ctx, basis, RES, args, shape, warp)
                        got = warped(c, basis, RES, args, shape, warp)
                        what = "%s mode=%d shape=%d warp=%s %s" % (BASES[basis], mode, shape, warp, args)
                        assert_parity(got, strict, what)
                        if basis != 3:  # only simplex has a tolerance form
                            assert np.array_equal(got, strict), what
                        worst = max(worst, float(np.abs(got.astype(np.float64) - strict).max()))
        print("mode %d: largest difference from strict %.3g" % (mode, worst))
    finally:
        c.close()


# 7. the metric's size: 4096^2, simplex, 13 octaves, 4 displacement octaves; sampled rows against the driver
@pytest.mark.parametrize("shape", [FBM, RIDGED], ids=["fbm", "ridged"])
def test_warp_4096_sampled_rows(nj, ctx, shape):
    R, args, warp = 4096, (0.4, 1.0, 2.0, 0.0, 13, 4096 * 3, 4096 * 5, 1700), (300.0, 1.0, 4)
    got = warped(ctx, 3, R, args, shape, warp)
    rows = [0, 1, 1777, 2048, 4095]
    assert np.array_equal(got[rows], driver(3, R, R, args, shape, warp, row_ids=rows))
    assert np.isfinite(got).all()


# 8. WarpedNoiseStage -> Gauss5 x17 -> FlowMap x5 -> erosion x5 == the oracle's stages on the driver's plane; on a single
#    plane and on a READ / WRITE pair
def test_warped_pipeline_matches_oracle_stages(nj, ctx, oracle):
    res, xp, zp = 160, 4096, -2048
    args, warp = (0.4, 1.0, 2.0, 0.0, 13, xp, zp, 1700), (300.0, 1.0, 4)
    noise = driver(3, res, res, args, FBM, warp)
    want = oracle.erosion_min(oracle.flowmap(oracle.kernel_filter(noise, oracle.GAUSS5_S1, 17), 5, 0.0, 0.005), 5)
    for rw in (False, True):
        stages = [nj.WarpedNoiseStage(ctx, nj.FractalNoise.Simplex, 0.4, 1.0, 13, 2.0, 0.0, 1700, warpStrength=300.0,
                                      warpScale=1.0, warpOctaves=4),
                  nj.KernelFilterStage(ctx, nj.KernelFilterType.Gauss5_S1, 17),
                  nj.FlowMapStage(ctx, 5, 0.0, 0.005),
                  nj.ErosionStage(ctx, 5)]
        pipe = nj.BasePipeline(stages, "warped")
        d = nj.GeneratorData("w", ctx.alloc(res * res), res, xp, zp, write=ctx.alloc(res * res) if rw else None)
        done = []
        pipe.Enqueue(d, completeAction=done.append)
        pipe.RunToCompletion()
        assert len(done) == 1
        got = d.data.ToArray((res, res))
        assert np.array_equal(got, want), "rw=%s: %d cells differ" % (rw, int((got != want).sum()))
        pipe.Destroy()


# 9. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    sentinel = np.full((res, res), 7.25, f32)
    d = ctx.from_host(sentinel)
    pos = ctx.from_host(np.zeros(2, np.int32))
    st = nj.Stripe(res, res, 0, res, 0, res, 0)
    heads = {"nz_fractal_warped": (3, d.ptr, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300),
             "nz_fractal_warped_batch": (3, d.ptr, res, 1, pos.ptr, 0.4, 1.0, 2.0, 0.0, 8, 300),
             "nz_fractal_warped_stripe": (3, d.ptr, C.byref(st), 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300)}
    bad = [((-1, 1.0, 2.0, 37.5, 1.0, 4), "shape"), ((3, 1.0, 2.0, 37.5, 1.0, 4), "shape"),
           ((0, 1.0, 2.0, 37.5, 1.0, -1), "warpOctaves"),
           ((0, 1.0, 2.0, math.nan, 1.0, 4), "warpStrength"), ((0, 1.0, 2.0, math.inf, 1.0, 4), "warpStrength"),
           ((0, 1.0, 2.0, 37.5, math.nan, 4), "warpScale"), ((0, 1.0, 2.0, 37.5, -math.inf, 4), "warpScale")]
    for name, head in heads.items():
        for tail, word in bad:
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(name, *head, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and word in str(e.value), (name, tail)
    # what the shaped entries reject: a resolution out of range, an unknown basis
    with pytest.raises(nj.NoizeError) as e:
        ctx.call("nz_fractal_warped", 3, d.ptr, 0, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300, 0, 1.0, 2.0, 37.5, 1.0, 4)
    assert e.value.status == nj._native.NZ_ERR_INVALID
    with pytest.raises(nj.NoizeError) as e:
        ctx.call("nz_fractal_warped", 8, d.ptr, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300, 0, 1.0, 2.0, 37.5, 1.0, 4)
    assert e.value.status == nj._native.NZ_ERR_INVALID
    ctx.synchronize()
    assert np.array_equal(d.ToArray((res, res)), sentinel)
    ctx.call("nz_fractal_warped", 3, d.ptr, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300, RIDGED, 1.0, 2.0, 37.5, 1.0, 4)
    want = driver(3, res, res, (0.4, 1.0, 2.0, 0.0, 8, 0, 0, 300), RIDGED, (37.5, 1.0, 4))
    assert np.array_equal(d.ToArray((res, res)), want)
    d.Dispose(); pos.Dispose()
