"""The hillslope diffusion stage on the GPU (nz_hillslope_diffusion*, HillslopeDiffusionStage) against the numpy restatement
of tests/hillslope_ref.py, bit for bit throughout: sizes on and across the 64-row and 64-column block edges at four values of
r, in place and out of place, one and three iterations, the batch form, planes carved from a guarded slab, a reused work
buffer, the three float modes, r = 0, NaN cells, bad arguments, the stage in a pipeline, and one 1024^2 run."""
import ctypes as C
import math

import numpy as np
import pytest

import fill_ref as L
import fluvial_implicit_ref as RI
import hillslope_ref as R
from test_gpu_slab import PAIRS, carved, memo
from test_hydraulic_ref import relief

pytestmark = pytest.mark.gpu
f32 = np.float32
# on and across the block edges (63, 64, 65), a line longer than two blocks (130, 160), 16-byte widths (4, 16, 64, 68, 128,
# 160) and 4-byte widths; 1 and 2 have no interior
RES = [1, 2, 3, 4, 5, 16, 63, 64, 65, 68, 97, 128, 130, 160]
RS = [0.01, 1.0, 100.0, 1e4]
SENTINEL = f32(-123.5)


def tile(res, seed=1):
    """rng.random * 100 of the seed: rough, so every cell moves."""
    return memo(("hillslope tile", res, seed),
                lambda: (np.random.default_rng(seed).random((res, res), dtype=f32) * f32(100.0)).astype(f32))


def ref(key, h, diffusivity, dt=1.0, iterations=1):
    return memo(("hillslope ref", key, float(diffusivity), float(dt), iterations),
                lambda: R.diffuse(h, diffusivity, dt, iterations))


def assert_same(got, want, what):
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def run_gpu(nj, ctx, h, diffusivity, dt=1.0, iterations=1, in_place=False, work=None):
    """One run on the host plane h (res x res, or count x res x res) -> out; out of place the heights are checked to come
    back untouched."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    src = ctx.from_host(h)
    out = src if in_place else ctx.from_host(np.full(h.size, SENTINEL, f32))
    own = work is None
    if own:
        work = ctx.alloc(max(1, nj._native.lib.nz_hillslope_diffusion_work_floats(res, count)))
    desc = nj._native.HillslopeDesc(diffusivity, dt, iterations)
    if h.ndim == 3:
        ctx.call("nz_hillslope_diffusion_batch", src.ptr, out.ptr, work.ptr, C.byref(desc), res, count).Complete()
    else:
        ctx.call("nz_hillslope_diffusion", src.ptr, out.ptr, work.ptr, C.byref(desc), res).Complete()
    got = out.ToArray(h.shape)
    if not in_place:
        assert_same(src.ToArray(h.shape), h, "the heights are read only")
        out.Dispose()
    src.Dispose()
    if own:
        work.Dispose()
    return got


def border(res):
    b = np.zeros((res, res), bool)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = True
    return b


# 1. every size at every r, one and three iterations, out of place and in place
@pytest.mark.parametrize("res", RES)
def test_matches_the_reference(nj, ctx, res):
    h = tile(res)
    assert nj._native.lib.nz_hillslope_diffusion_work_floats(res, 1) >= 2 * res
    for r in RS:
        for its in (1, 3):
            want = ref(res, h, r, 1.0, its)
            what = "%d^2 r %g x%d" % (res, r, its)
            got = run_gpu(nj, ctx, h, r, 1.0, its)
            assert_same(got, want, what)
            assert_same(got[border(res)], h[border(res)], what + ": the border keeps its bits")
            assert_same(run_gpu(nj, ctx, h, r, 1.0, its, in_place=True), want, what + ", in place")
    # r is the one product diffusivity * dt
    assert_same(run_gpu(nj, ctx, h, 0.375, 24.0, 2), ref(res, h, 0.375, 24.0, 2), "%d^2 0.375 x 24" % res)


# 2. every position of a batch is the tile alone: 5 tiles of 65^2 (4-byte path), 3 tiles of 64^2 (16-byte path)
@pytest.mark.parametrize("res,count", [(65, 5), (64, 3)])
def test_a_batch(nj, ctx, res, count):
    a = tile(res)
    tiles = [a, a[::-1], a.T, tile(res, 2), a[:, ::-1]][:count]
    tiles = [np.ascontiguousarray(t) for t in tiles]
    for r, its in ((1.0, 1), (100.0, 3)):
        single = [run_gpu(nj, ctx, t, r, 1.0, its) for t in tiles]
        for k, (t, got) in enumerate(zip(tiles, single)):
            assert_same(got, ref(("batch", res, k), t, r, 1.0, its), "single %d" % k)
        for in_place in (False, True):
            got = run_gpu(nj, ctx, np.stack(tiles), r, 1.0, its, in_place=in_place)
            for k in range(count):
                assert_same(got[k], single[k], "position %d of %d x %d^2, in place %s" % (k, count, res, in_place))


# 3. planes carved from one guarded allocation at four alignments and three mixed pairs: the guards stay silent
@pytest.mark.parametrize("res", [64, 68, 97])
def test_on_slab_carved_planes(nj, ctx, res):
    h, n = tile(res), res * res
    want = ref(res, h, 100.0, 1.0, 2)
    desc = nj._native.HillslopeDesc(100.0, 1.0, 2)
    nwork = nj._native.lib.nz_hillslope_diffusion_work_floats(res, 1)
    for p, q in PAIRS:
        r = p if p == q else (q + 1) % 4
        with carved(ctx, res, height=(n, p, h), out=(n, q, None), work=(nwork, r, None)) as (s, t):
            ctx.call("nz_hillslope_diffusion", t.height.ptr, t.out.ptr, t.work.ptr, C.byref(desc), res).Complete()
            assert_same(t.out.ToArray((res, res)), want, ("out", res, p, q))
            assert_same(t.height.ToArray((res, res)), h, ("heights", res, p, q))
            s.check()
        with carved(ctx, res, plane=(n, p, h), work=(nwork, q, None)) as (s, t):
            ctx.call("nz_hillslope_diffusion", t.plane.ptr, t.plane.ptr, t.work.ptr, C.byref(desc), res).Complete()
            assert_same(t.plane.ToArray((res, res)), want, ("in place", res, p, q))
            s.check()
    count = 3
    hh = np.stack([h, h[::-1].copy(), h.T.copy()])
    wants = np.stack([ref(("slab", res, k), hh[k], 100.0, 1.0, 2) for k in range(count)])
    nwork = nj._native.lib.nz_hillslope_diffusion_work_floats(res, count)
    for p, q in PAIRS:
        with carved(ctx, res, height=(count * n, p, hh), out=(count * n, q, None), work=(nwork, (q + 2) % 4, None)) as (s, t):
            ctx.call("nz_hillslope_diffusion_batch", t.height.ptr, t.out.ptr, t.work.ptr, C.byref(desc), res, count).Complete()
            assert_same(t.out.ToArray((count, res, res)), wants, ("batch out", res, p, q))
            s.check()


# 4. one work buffer, uncleared, across 160^2 at r 100 -> 65^2 at r 0.01 -> 160^2 at r 1: no table entry of a run survives
def test_a_reused_work_buffer(nj, ctx):
    work = ctx.alloc(nj._native.lib.nz_hillslope_diffusion_work_floats(160, 1))
    for res, r in ((160, 100.0), (65, 0.01), (160, 1.0), (68, 1e4)):
        got = run_gpu(nj, ctx, tile(res), r, 1.0, 2, work=work)
        assert_same(got, ref(res, tile(res), r, 1.0, 2), "reused work %d r %g" % (res, r))
    work.Dispose()


# 5. all three float modes give the same bits
def test_float_modes_agree(nj, ctx):
    for res in (97, 128):
        h = tile(res)
        want = ref(res, h, 100.0, 1.0, 3)
        assert_same(run_gpu(nj, ctx, h, 100.0, 1.0, 3), want, "strict")
        for mode in (1, 2):
            mctx = nj.Context(0)
            try:
                mctx.float_mode = mode
                got = run_gpu(nj, mctx, h, 100.0, 1.0, 3)
            finally:
                mctx.close()
            assert_same(got, want, "%d^2 float mode %d" % (res, mode))


# 6. r == 0 is out = h bit for bit, whatever the cells hold
def test_r_zero_returns_the_heights(nj, ctx):
    h = np.array(tile(65))
    h[1, 1], h[2, 2], h[0, 3], h[30, 30] = f32(-0.0), f32(np.nan), f32(np.inf), f32(-0.0)
    for diffusivity, dt in ((0.0, 5.0), (3.0, 0.0), (-0.0, 1.0), (0.0, 0.0)):
        for in_place in (False, True):
            assert_same(run_gpu(nj, ctx, h, diffusivity, dt, 3, in_place=in_place), h, ("r == 0", diffusivity, dt, in_place))
    hh = np.stack([h, h.T.copy()])
    assert_same(run_gpu(nj, ctx, hh, 0.0, 1.0), hh, "r == 0, a batch")


# 7. NaN: a cell in the interior spreads along its row and then down every column; a cell on the top border spreads down
# its own column only.  The pattern is the reference's; every other cell has the reference's bits
def test_nan_cells_spread_as_in_the_reference(nj, ctx):
    for res in (65, 128):
        for at in ((20, 30), (0, 10), (res - 1, res - 2), (17, 0)):
            h = np.array(tile(res))
            h[at] = f32(np.nan)
            want = R.diffuse_r(h, 1.0)
            got = run_gpu(nj, ctx, h, 1.0)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (res, at)
            assert_same(got[~nan], want[~nan], ("beside the NaN cells", res, at))
            assert nan.sum() >= res - 2


# 8. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    n = res * res
    sentinel = np.full((res, res), 7.25, f32)
    h, out = ctx.from_host(sentinel), ctx.from_host(sentinel)
    work = ctx.alloc(nj._native.lib.nz_hillslope_diffusion_work_floats(res, 1) + n)  # room for a plane inside it
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731

    def refused(name, desc, height=h, o=out, wk=work, res=res, count=1):
        p = C.byref(desc) if desc is not None else None
        for entry, tail in (("nz_hillslope_diffusion", (res,)), ("nz_hillslope_diffusion_batch", (res, count))):
            if count != 1 and entry == "nz_hillslope_diffusion":
                continue
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, ptr(height), ptr(o), ptr(wk), p, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))

    good = lambda diffusivity=0.5, dt=2.0, iterations=2: nj._native.HillslopeDesc(diffusivity, dt, iterations)  # noqa: E731
    for v in (math.nan, math.inf, -math.inf, -1e-6):
        refused("diffusivity", good(diffusivity=v))
        refused("dt", good(dt=v))
    refused("r is not finite", good(diffusivity=3e38, dt=3e38))
    refused("1 + 2 r is not finite", good(diffusivity=2e38, dt=1.0))
    refused("iterations", good(iterations=0))
    refused("iterations", good(iterations=-3))
    refused("desc", None)
    refused("height", good(), height=None)
    refused("out", good(), o=None)
    refused("work", good(), wk=None)
    refused("int32", good(), res=46340, count=2)  # 2 x 46340^2 cells: checked before any plane is touched
    half_h = ctx.wrap(h.ptr + 4 * (n // 2), n)      # a plane that begins inside the heights
    one_on = ctx.wrap(h.ptr + 4, n)                 # ... one cell behind their start
    inside = ctx.wrap(work.ptr + 4 * 8, n)          # ... inside `work`
    refused("out overlaps height", good(), o=half_h)
    refused("out overlaps height", good(), o=one_on)
    refused("out overlaps height", good(), height=half_h, o=h)
    refused("work overlaps out", good(), o=inside)
    refused("work overlaps height", good(), height=inside)
    refused("work overlaps out", good(), height=inside, o=inside)   # in place inside work
    refused("work overlaps out", good(), wk=out)
    refused("work overlaps height", good(), wk=h)
    refused("work overlaps out", good(), height=h, o=h, wk=ctx.wrap(h.ptr + 4 * (n - 2), work.Length))
    ctx.synchronize()
    for t in (h, out):
        assert_same(t.ToArray((res, res)), sentinel, "a plane of a refused call")
    assert (work.ToArray() == f32(7.25)).all()
    # an empty payload is no error and touches nothing
    ctx.call("nz_hillslope_diffusion", h.ptr, out.ptr, work.ptr, C.byref(good()), 0).Complete()
    ctx.call("nz_hillslope_diffusion_batch", h.ptr, out.ptr, work.ptr, C.byref(good()), res, 0).Complete()
    assert_same(out.ToArray((res, res)), sentinel, "an empty payload")
    assert (work.ToArray() == f32(7.25)).all()
    w = nj._native.lib.nz_hillslope_diffusion_work_floats
    assert w(0, 1) == 0 and w(64, 0) == 0 and w(-3, 2) == 0 and w(8, -1) == 0
    # the context still works, and zero scalars are in range
    hh = tile(res)
    h.CopyFrom(hh)
    ctx.call("nz_hillslope_diffusion", h.ptr, out.ptr, work.ptr, C.byref(good()), res).Complete()
    assert_same(out.ToArray((res, res)), R.diffuse(hh, 0.5, 2.0, 2), "after the refusals")
    ctx.call("nz_hillslope_diffusion", h.ptr, out.ptr, work.ptr, C.byref(good(diffusivity=-0.0)), res).Complete()
    assert_same(out.ToArray((res, res)), hh, "diffusivity -0.0 is r == 0")
    for t in (h, out, work):
        t.Dispose()


def evolve(key, h, rounds, T, diffusivity, iterations=1):
    """The numpy chain [fill, implicit fluvial (dt T), hillslope (dt T)] x rounds."""
    def make():
        cur = np.array(h, f32)
        for _ in range(rounds):
            cur = L.flood(cur)
            cur = RI.chain(cur, 1, dt=T)[0]
            cur = R.diffuse(cur, diffusivity, T, iterations)
        return cur
    return memo(("hillslope evolve", key, rounds, T, diffusivity, iterations), make)


# 9. the evolution loop [DepressionFillStage, ImplicitFluvialStage(dt=T), HillslopeDiffusionStage(dt=T)], two rounds at 97^2,
# against the numpy chain: a single tile, a batch, and a payload of another size through the same stages
def test_stage_in_a_pipeline(nj, ctx):
    T, kappa = 50.0, 0.01
    st = nj.HillslopeDiffusionStage(ctx, kappa, T, 2)  # the positional order
    assert (st.diffusivity, st.dt, st.iterations, st.work) == (kappa, T, 2, None)
    fill, rivers = nj.DepressionFillStage(ctx), nj.ImplicitFluvialStage(ctx, dt=T)
    pipe = nj.BasePipeline([fill, rivers, st], "evolve")

    def rounds(d, n=2):
        for _ in range(n):
            done = []
            pipe.Enqueue(d, completeAction=done.append)
            pipe.RunToCompletion()
            assert len(done) == 1

    h97 = np.ascontiguousarray(relief(97, 300), f32)
    d = nj.GeneratorData("h", ctx.from_host(h97), 97, 0, 0)
    rounds(d)
    want = evolve("relief 97", h97, 2, T, kappa, 2)
    assert_same(d.data.ToArray((97, 97)), want, "two rounds at 97^2")
    assert not R.same(want, evolve("relief 97", h97, 1, T, kappa, 2))
    assert st.work.Length == nj._native.lib.nz_hillslope_diffusion_work_floats(97, 1)
    # a resize to 65^2: the work buffer follows the payload
    h65 = np.ascontiguousarray(h97[:65, 30:95])
    d65 = nj.GeneratorData("h", ctx.from_host(h65), 65, 0, 0)
    rounds(d65)
    assert_same(d65.data.ToArray((65, 65)), evolve("relief 65", h65, 2, T, kappa, 2), "65^2 behind 97^2")
    assert st.work.Length == nj._native.lib.nz_hillslope_diffusion_work_floats(65, 1)
    # a batch of two at 97^2
    hh = np.stack([h97, np.ascontiguousarray(h97.T)])
    bt = nj.GeneratorDataBatch("h", ctx.from_host(hh), 97, None, 2)
    rounds(bt)
    got = bt.data.ToArray((2, 97, 97))
    assert_same(got[0], want, "batch tile 0")
    assert_same(got[1], evolve("relief 97 T", hh[1], 2, T, kappa, 2), "batch tile 1")
    # any other payload is refused, like its siblings
    with pytest.raises(Exception, match="Unhandled stageio"):
        st.Schedule(nj.PipelineWorkItem(object()), nj.JobHandle())
    for stage in (fill, rivers, st):
        stage.OnDestroy()
    assert st.work is None


# 10. 1024^2: 16 blocks along a line, 16 x 16 waves a sweep, on the 13-octave fBm tile
def test_1024_matches_the_reference(nj, ctx):
    res = 1024
    d = ctx.alloc(res * res)
    ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700).Complete()
    h = d.ToArray((res, res))
    d.Dispose()
    want = R.diffuse(h, 0.5, 200.0, 1)
    got = run_gpu(nj, ctx, h, 0.5, 200.0, 1, in_place=True)
    assert_same(got, want, "1024^2, r = 100")
    assert not R.same(got, h)
