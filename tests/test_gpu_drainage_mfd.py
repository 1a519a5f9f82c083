"""The multiple-flow drainage stage on the GPU (nz_drainage_mfd*, MfdDrainageStage, ImplicitFluvialStage(routing=Multiple))
against the walk of tests/drainage_mfd_ref.py, bit for bit throughout: sizes on and across the 64-column / 16-row tile edges
with and without a rain map and a sea at exponents 1 and 4, the batch form, the long chain with an ample and with an
exhausted budget (all or nothing), the sweep hook, a reused work buffer, the three float modes, planes carved from a guarded
slab, a signed rain map, the terrain families, bad arguments, the stages in a pipeline, and a 1024^2 filled tile checked as
a fixed point."""
import ctypes as C
import math

import numpy as np
import pytest

import drainage_mfd_ref as M
import drainage_ref as D
import fill_ref
import fluvial_implicit_ref as R
import fluvial_ref as F
import terrain_tiles as T
from test_gpu_slab import PAIRS, carved, memo
from test_hydraulic_ref import relief

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
RES = [1, 2, 3, 5, 16, 63, 64, 65, 68, 97, 130, 160]
EXPONENTS = [1, 4]
# a pass is at least one Jacobi step, so "cells of the longest path of the flow graph" + 2 launches always suffice; the
# tests that know the height ask for exactly that, the others for a budget no tile here but the serpentine comes near
GENEROUS = 600


def tile(res):
    def make():
        if res <= 5:
            return np.random.default_rng(res).random((res, res), dtype=f32)
        return np.ascontiguousarray(relief(res, 500 if res == 160 else 300), f32)
    return memo(("drainage tile", res), make)  # test_gpu_drainage's tiles, shared with it


def rain_map(res, seed=0):
    return memo(("drainage rain map", res, seed),
                lambda: (np.random.default_rng(100 + res + seed).random((res, res), dtype=f32) * f32(1.5) + f32(0.25)).astype(f32))


def walk(key, h, rain=1.0, sea=OFF, rm=None, exponent=1):
    """(A, DAG height) of the model, computed once per key and shared; nothing writes to it."""
    return memo(("mfd walk", key, rain, sea, rm is not None, exponent), lambda: M.walk(h, rain, sea, rm, exponent))


def serpentine():
    return memo("mfd serpentine", lambda: (D.serpentine(),) + M.walk(D.serpentine()))  # h, A, DAG height


def assert_bits(got, want, what):
    want = np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def desc_of(nj, rain, sea, budget, exponent=1, rm=None):
    return nj._native.DrainageMfdDesc(rain, sea, budget, exponent, rm.ptr if rm is not None else None)


def run_gpu(nj, ctx, h, rain=1.0, sea=OFF, budget=GENEROUS, rm=None, exponent=1, work=None):
    """One run on the host plane h (res x res, or count x res x res) -> (drainage, passes, converged); the heights are
    checked to come back untouched."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    src, out = ctx.from_host(h), ctx.from_host(np.full(h.shape, np.nan, f32))
    own = work is None
    if own:
        work = ctx.alloc(nj._native.lib.nz_drainage_mfd_work_floats(res, count))
    m = ctx.from_host(np.ascontiguousarray(rm, f32)) if rm is not None else None
    desc = desc_of(nj, rain, sea, budget, exponent, m)
    if h.ndim == 3:
        ctx.call("nz_drainage_mfd_batch", src.ptr, out.ptr, work.ptr, C.byref(desc), res, count).Complete()
    else:
        ctx.call("nz_drainage_mfd", src.ptr, out.ptr, work.ptr, C.byref(desc), res).Complete()
    got = out.ToArray(h.shape)
    assert_bits(src.ToArray(h.shape), h, "the heights are read only")
    status = ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()
    for t in (src, out, m) + ((work,) if own else ()):
        if t is not None:
            t.Dispose()
    return got, int(status[0]), int(status[1])


# 1. sizes on and across the tile edges (the 16-byte and the 4-byte path, partial tiles both ways, one tile and many), each
# with and without a rain map and a sea, at exponents 1 and 4; the budget is the DAG height + 2
@pytest.mark.parametrize("exponent", EXPONENTS)
@pytest.mark.parametrize("res", RES)
def test_matches_the_walk(nj, ctx, res, exponent):
    h = tile(res)
    sea = float(np.median(h))
    for rain, s, mapped in ((1.0, OFF, False), (0.75, OFF, True), (1.0, sea, False), (0.3, sea, True)):
        rm = rain_map(res) if mapped else None
        want, height = walk(res, h, rain, s, rm, exponent)
        assert np.isfinite(want).all()
        got, passes, conv = run_gpu(nj, ctx, h, rain, s, height + 2, rm, exponent)
        assert conv == 1 and 2 <= passes <= height + 1, (res, rain, s, mapped, passes, height)
        assert_bits(got, want, "%d^2 exponent %d rain %g sea %g map %s" % (res, exponent, rain, s, mapped))
        if not mapped:
            assert (got >= f32(rain)).all()


# 2. every position of a batch is the tile alone
def test_a_batch_of_three(nj, ctx):
    res = 97
    a = tile(res)
    tiles = [a, np.ascontiguousarray(a[::-1]), np.ascontiguousarray(a.T)]
    maps = [rain_map(res, k) for k in range(3)]
    single = [run_gpu(nj, ctx, t, 0.75, 0.4, rm=m, exponent=2) for t, m in zip(tiles, maps)]
    for k, (t, m, (got, _, conv)) in enumerate(zip(tiles, maps, single)):
        assert conv == 1
        assert_bits(got, walk(("batch", k), t, 0.75, 0.4, m, 2)[0], "single")
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        got, passes, conv = run_gpu(nj, ctx, np.stack([tiles[j] for j in order]), 0.75, 0.4,
                                    rm=np.stack([maps[j] for j in order]), exponent=2)
        assert conv == 1 and passes == max(s[1] for s in single)  # the status words cover the whole batch
        for k, j in enumerate(order):
            assert_bits(got[k], single[j][0], "position %d tile %d" % (k, j))


# 3. the long chain: a budget that needs no measurement, and all or nothing when it runs out
def test_the_serpentine_converges_and_an_exhausted_budget_returns_the_start_state(nj, ctx, capsys):
    h, want, height = serpentine()
    got, passes, conv = run_gpu(nj, ctx, h, budget=height + 2)
    with capsys.disabled():
        print("\nserpentine 160^2: DAG height %d, converged after %d passes" % (height, passes))
    assert conv == 1
    assert_bits(got, want, "serpentine")
    rm = rain_map(160)
    for budget in (1, 2, 7):
        got, passes, conv = run_gpu(nj, ctx, h, budget=budget)
        assert (passes, conv) == (budget, 0)
        assert_bits(got, np.ones_like(h), "serpentine, budget %d: rain everywhere" % budget)
        got, passes, conv = run_gpu(nj, ctx, h, 0.3, budget=budget, rm=rm, exponent=4)
        assert (passes, conv) == (budget, 0)
        assert_bits(got, F.rain_plane(h.shape, 0.3, rm), "serpentine, budget %d: rain_c everywhere" % budget)


# 4. the schedule is free: every sweep cap gives the same plane; the default comes back afterwards
def test_the_sweep_cap_does_not_matter(nj, ctx):
    lib = nj._native.lib
    s, sw, sheight = serpentine()
    f = tile(130)
    fw, fheight = walk(130, f, 0.75, OFF, rain_map(130), 4)
    default = lib.nz_debug_drainage_mfd_sweeps(0)
    try:
        for cap in (1, 2, 7, 16, 200):
            lib.nz_debug_drainage_mfd_sweeps(cap)
            got, passes, conv = run_gpu(nj, ctx, s, budget=sheight + 2)
            assert conv == 1, (cap, passes)
            assert_bits(got, sw, "serpentine, cap %d" % cap)
            got, passes, conv = run_gpu(nj, ctx, f, 0.75, budget=fheight + 2, rm=rain_map(130), exponent=4)
            assert conv == 1, (cap, passes)
            assert_bits(got, fw, "relief 130^2, cap %d" % cap)
    finally:
        assert lib.nz_debug_drainage_mfd_sweeps(0) == 200
    assert lib.nz_debug_drainage_mfd_sweeps(0) == default >= 1
    assert lib.nz_debug_drainage_sweeps(0) == default  # the tree's cap is another word


# 5. the same work buffer, uncleared, with another tile: no tile byte, weight or verdict of the first run survives
def test_a_reused_work_buffer(nj, ctx):
    res = 130
    work = ctx.alloc(nj._native.lib.nz_drainage_mfd_work_floats(res, 1))
    a, b = tile(res), np.ascontiguousarray(tile(res).T[::-1])
    for k, h in ((0, a), (1, b), (0, a)):
        got, _, conv = run_gpu(nj, ctx, h, work=work)
        assert conv == 1
        assert_bits(got, walk(("reused", k), h)[0], "reused work")
    got, passes, conv = run_gpu(nj, ctx, b, budget=1, work=work)  # ... nor a verdict
    assert (passes, conv) == (1, 0)
    assert_bits(got, np.ones_like(b), "reused work, one pass")
    work.Dispose()


# 6. all three float modes give the same bits
def test_float_modes_agree(nj, ctx):
    h, rm = tile(97), rain_map(97)
    want = run_gpu(nj, ctx, h, 0.3, 0.4, rm=rm, exponent=4)
    assert_bits(want[0], walk(97, h, 0.3, 0.4, rm, 4)[0], "strict")
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got = run_gpu(nj, mctx, h, 0.3, 0.4, rm=rm, exponent=4)
        finally:
            mctx.close()
        assert_bits(got[0], want[0], "float mode %d" % mode)
        assert got[1:] == want[1:]


# 7. planes carved from one guarded allocation at four alignments and three mixed pairs: the guards stay silent
@pytest.mark.parametrize("res", [64, 97])
def test_on_slab_carved_planes(nj, ctx, res):
    h, rm, n = tile(res), rain_map(res), res * res
    want = walk(res, h, 0.75, OFF, rm, 1)[0]
    nwork = nj._native.lib.nz_drainage_mfd_work_floats(res, 1)
    for p, q in PAIRS:
        r = p if p == q else (q + 1) % 4
        with carved(ctx, res, height=(n, p, h), drainage=(n, q, None), work=(nwork, r, None), rain=(n, q, rm)) as (s, t):
            ctx.call("nz_drainage_mfd", t.height.ptr, t.drainage.ptr, t.work.ptr,
                     C.byref(desc_of(nj, 0.75, OFF, GENEROUS, 1, t.rain)), res).Complete()
            assert_bits(t.drainage.ToArray((res, res)), want, (res, p, q))
            assert_bits(t.height.ToArray((res, res)), h, ("heights", res, p, q))
            assert ctx.wrap(t.work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
            s.check()
    count = 3
    hh = np.stack([h, h[::-1].copy(), h.T.copy()])
    want = np.stack([walk(("carved", res, k), hh[k], exponent=4)[0] for k in range(count)])
    nwork = nj._native.lib.nz_drainage_mfd_work_floats(res, count)
    for p, q in PAIRS:
        with carved(ctx, res, height=(count * n, p, hh), drainage=(count * n, q, None), work=(nwork, (q + 2) % 4, None)) as (s, t):
            ctx.call("nz_drainage_mfd_batch", t.height.ptr, t.drainage.ptr, t.work.ptr,
                     C.byref(desc_of(nj, 1.0, OFF, GENEROUS, 4)), res, count).Complete()
            assert_bits(t.drainage.ToArray((count, res, res)), want, ("batch", res, p, q))
            s.check()


# 8. a signed rain map: values move both ways, and "changed" must look at every single update
def test_a_signed_rain_map(nj, ctx):
    for res in (97, 130):
        h = tile(res)
        rm = (rain_map(res) - f32(1.0)).astype(f32)
        assert (rm < 0).any() and (rm > 0).any()
        for exponent in EXPONENTS:
            want, height = walk(("signed", res), h, 0.75, OFF, rm, exponent)
            got, passes, conv = run_gpu(nj, ctx, h, 0.75, OFF, height + 2, rm, exponent)
            assert conv == 1 and passes <= height + 1
            assert_bits(got, want, "signed map, %d^2 exponent %d" % (res, exponent))


# 9. the terrain families at 97^2: ties, plateaus, extreme scales, subnormal slopes
@pytest.mark.parametrize("exponent", EXPONENTS)
@pytest.mark.parametrize("kind", sorted(T.GENERATORS))
def test_the_terrain_families(nj, ctx, kind, exponent):
    h = memo(("mfd family", kind), lambda: np.ascontiguousarray(T.GENERATORS[kind](97, np.random.default_rng(5)), f32))
    want, height = walk(("family", kind), h, exponent=exponent)
    assert np.isfinite(want).all()
    got, passes, conv = run_gpu(nj, ctx, h, budget=height + 2, exponent=exponent)
    assert conv == 1 and 2 <= passes <= height + 1, (kind, passes, height)
    assert_bits(got, want, "%s exponent %d" % (kind, exponent))


# 10. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    n = res * res
    sentinel = np.full((res, res), 7.25, f32)
    h, out, rm = ctx.from_host(sentinel), ctx.from_host(sentinel), ctx.from_host(sentinel)
    work = ctx.alloc(nj._native.lib.nz_drainage_mfd_work_floats(res, 1))
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731

    def refused(name, desc, height=h, drainage=out, wk=work):
        p = C.byref(desc) if desc is not None else None
        for entry, tail in (("nz_drainage_mfd", (res,)), ("nz_drainage_mfd_batch", (res, 1))):
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, ptr(height), ptr(drainage), ptr(wk), p, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))

    for v in (math.nan, math.inf, -math.inf):
        refused("rain", desc_of(nj, v, OFF, 10))
        refused("seaLevel", desc_of(nj, 1.0, v, 10))
    refused("rain", desc_of(nj, -1e-6, OFF, 10))
    refused("maxPasses", desc_of(nj, 1.0, OFF, 0))
    refused("maxPasses", desc_of(nj, 1.0, OFF, -3))
    for e in (0, 17, -1, 1 << 20):
        refused("exponent", desc_of(nj, 1.0, OFF, 10, e))
    refused("desc", None)
    good = desc_of(nj, 1.0, OFF, 10)
    refused("height", good, height=None)
    refused("drainage", good, drainage=None)
    refused("work", good, wk=None)
    inside = ctx.wrap(work.ptr + 4 * (work.Length - n // 2), n)  # a plane that begins inside `work`
    half_h = ctx.wrap(h.ptr + 4 * (n // 2), n)                    # ... inside the heights
    half_m = ctx.wrap(rm.ptr + 4 * (n // 2), n)                   # ... inside the rain map
    for plane in (h, half_h, inside, work):
        refused("drainage overlaps", good, drainage=plane)
    for plane in (rm, half_m):
        refused("drainage overlaps rainMap", desc_of(nj, 1.0, OFF, 10, 1, rm), drainage=plane)
    refused("work overlaps height", good, height=inside)
    refused("work overlaps rainMap", desc_of(nj, 1.0, OFF, 10, 1, inside))
    ctx.synchronize()
    for t in (h, out, rm):
        assert_bits(t.ToArray((res, res)), sentinel, "a plane of a refused call")
    assert (work.ToArray() == f32(7.25)).all()
    # an empty payload is no error and touches nothing
    ctx.call("nz_drainage_mfd", h.ptr, out.ptr, work.ptr, C.byref(good), 0).Complete()
    ctx.call("nz_drainage_mfd_batch", h.ptr, out.ptr, work.ptr, C.byref(good), res, 0).Complete()
    assert_bits(out.ToArray((res, res)), sentinel, "an empty payload")
    assert nj._native.lib.nz_drainage_mfd_work_floats(0, 1) == 0 == nj._native.lib.nz_drainage_mfd_work_floats(res, 0)
    # a sea level of -FLT_MAX, a rain of 0 and the exponents 1 and 16 are in range, and the context still works
    hh = tile(97)[:res, :res].copy()
    h.CopyFrom(hh)
    ctx.call("nz_drainage_mfd", h.ptr, out.ptr, work.ptr, C.byref(desc_of(nj, 0.0, OFF, 200)), res).Complete()
    assert not out.ToArray().any() and ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
    for e in (1, 16):
        ctx.call("nz_drainage_mfd", h.ptr, out.ptr, work.ptr, C.byref(desc_of(nj, 1.0, OFF, 200, e)), res).Complete()
        assert_bits(out.ToArray((res, res)), M.walk(hh, exponent=e)[0], "after the refusals, exponent %d" % e)
    for t in (h, out, rm, work):
        t.Dispose()


# 11. the stage behind NoiseStage and DepressionFillStage; a caller's plane, a rain map and a batch; a resized payload; a
# budget that runs out
def test_stage_in_a_pipeline(nj, ctx):
    res = 128
    st = nj.MfdDrainageStage(ctx)
    assert (st.drainage, st.passes, st.converged) == (None, None, None)
    noise = nj.NoiseStage(ctx, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300)
    pipe = nj.BasePipeline([noise, nj.DepressionFillStage(ctx), st], "spread rivers")
    d = nj.GeneratorData("h", ctx.alloc(res * res), res, 0, 0)
    done = []
    pipe.Enqueue(d, completeAction=done.append)
    pipe.RunToCompletion()
    assert len(done) == 1
    h = d.data.ToArray((res, res))
    assert F.pits(h) == 0  # filled
    want, height = M.walk(h)
    assert st.converged is True and 2 <= st.passes <= min(height + 1, 128 + res // 2)
    A = st.drainage.ToArray((res, res))
    assert_bits(A, want, "the stage's drainage")
    assert (A >= 1).all()  # rain 1 and no map: A >= rain
    # a resize: the same stage with a 65^2 payload, then 128^2 again
    h65 = np.ascontiguousarray(h[:65, 40:105])
    d65 = nj.GeneratorData("h", ctx.from_host(h65), 65, 0, 0)
    st.ReceiveHandledInput(nj.PipelineWorkItem(d65), nj.JobHandle())
    assert st.converged is True and st.drainage.Length == 65 * 65
    assert_bits(st.drainage.ToArray((65, 65)), M.walk(h65)[0], "65^2 behind 128^2")
    st.ReceiveHandledInput(nj.PipelineWorkItem(d), nj.JobHandle())
    assert st.converged is True
    assert_bits(st.drainage.ToArray((res, res)), want, "128^2 behind 65^2")
    # a caller's plane, a rain map, an exponent, a batch
    hh = np.stack([h, np.ascontiguousarray(h.T)])
    rm = np.stack([rain_map(res), rain_map(res, 1)])
    out, m = ctx.alloc(2 * res * res), ctx.from_host(rm)
    sea = float(np.median(h))
    st2 = nj.MfdDrainageStage(ctx, rain=0.5, seaLevel=sea, exponent=4, maxPasses=GENEROUS, rainMap=m, out=out)
    b = nj.GeneratorDataBatch("h", ctx.from_host(hh), res, None, 2)
    st2.ReceiveHandledInput(nj.PipelineWorkItem(b), nj.JobHandle())
    assert st2.converged is True and st2.drainage is out
    got = out.ToArray((2, res, res))
    for k in range(2):
        assert_bits(got[k], M.walk(hh[k], 0.5, sea, rm[k], 4)[0], "batch tile %d" % k)
    assert_bits(b.data.ToArray((2, res, res)), hh, "the heights pass through")
    # a budget that runs out: the start state, converged False
    st3 = nj.MfdDrainageStage(ctx, maxPasses=2)
    d3 = nj.GeneratorData("h", ctx.from_host(h), res, 0, 0)
    st3.ReceiveHandledInput(nj.PipelineWorkItem(d3), nj.JobHandle())
    assert st3.converged is False and st3.passes == 2
    assert_bits(st3.drainage.ToArray((res, res)), np.ones_like(h), "budget of 2")
    with pytest.raises(ValueError):
        nj.MfdDrainageStage(ctx, out=ctx.alloc(5)).ReceiveHandledInput(nj.PipelineWorkItem(d3), nj.JobHandle())
    for s in (st, st2, st3):
        s.OnDestroy()
    assert st.drainage is None and st.passes is None


def mfd_chain(h, iterations, exponent, **kw):
    """flood -> (walk of the multiple-flow model -> the implicit solve's walk) per iteration, in numpy."""
    h = fill_ref.flood(np.ascontiguousarray(h, f32))
    A = None
    for _ in range(iterations):
        A = M.walk(h, exponent=exponent)[0]
        h = R.walk(h, A, **kw)
    return h, A


# 12. ImplicitFluvialStage: routing=Multiple for 2 iterations against the numpy chain; routing=Steepest is today's stage
def test_implicit_fluvial_routing(nj, ctx):
    res = 97
    h = tile(res)

    def run(**kw):
        st = nj.ImplicitFluvialStage(ctx, iterations=2, dt=50.0, **kw)
        pipe = nj.BasePipeline([nj.DepressionFillStage(ctx), st], "valleys")
        d = nj.GeneratorData("h", ctx.from_host(h), res, 0, 0)
        done = []
        pipe.Enqueue(d, completeAction=done.append)
        pipe.RunToCompletion()
        assert len(done) == 1 and st.steps == 2 and st.converged is True
        out = d.data.ToArray((res, res)), st.drainage.ToArray((res, res))
        st.OnDestroy()
        return out

    for exponent in (1, 4):
        wh, wA = mfd_chain(h, 2, exponent, dt=50.0)
        gh, gA = run(routing=nj.FlowRouting.Multiple, flowExponent=exponent)
        assert_bits(gh, wh, "Multiple, exponent %d: heights" % exponent)
        assert_bits(gA, wA, "Multiple, exponent %d: drainage" % exponent)
    today = run()
    steepest = run(routing=nj.FlowRouting.Steepest, flowExponent=4)  # the exponent belongs to Multiple alone
    wh, wA = R.chain(fill_ref.flood(h), 2, dt=50.0)
    for got in (today, steepest):
        assert_bits(got[0], wh, "Steepest: heights")
        assert_bits(got[1], wA, "Steepest: drainage")
    assert not M.same(gh, wh)  # the routing matters


# 13. 1024^2, filled, rain 1, the hosts' default budget: the many-tile skip logic.  No walk is needed: the fixed point is
# unique, so "one Jacobi step of the model returns the plane" is a complete check
@pytest.mark.parametrize("exponent", EXPONENTS)
def test_1024_filled_is_the_fixed_point(nj, ctx, capsys, exponent):
    res = 1024
    n = res * res

    def filled():
        d = ctx.alloc(n)
        ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700).Complete()
        fwork = ctx.alloc(nj._native.lib.nz_fill_depressions_work_floats(res, 1))
        fdesc = nj._native.FillDesc(1e-4, OFF, 64 + res // 4, None)
        ctx.call("nz_fill_depressions", d.ptr, fwork.ptr, C.byref(fdesc), res).Complete()
        assert ctx.wrap(fwork.ptr, 2, dtype=np.int32).ToArray()[1] == 1
        fwork.Dispose()
        h = d.ToArray((res, res))
        d.Dispose()
        return h

    h = memo("mfd 1024 filled", filled)
    d = ctx.from_host(h)
    st = nj.MfdDrainageStage(ctx, exponent=exponent)  # every other default
    g = nj.GeneratorData("h", d, res, 0, 0)
    st.ReceiveHandledInput(nj.PipelineWorkItem(g), nj.JobHandle())
    passes, conv = st.passes, st.converged
    with capsys.disabled():
        print("\n1024^2 filled fBm, exponent %d: converged %s after %d passes (default budget %d)"
              % (exponent, conv, passes, 128 + res // 2))
    assert conv is True
    A = st.drainage.ToArray((res, res))
    assert_bits(d.ToArray((res, res)), h, "1024: the heights")
    st.OnDestroy()
    d.Dispose()
    assert np.isfinite(A).all() and (A >= 1).all()
    assert_bits(M.step(A, M.incoming(M.weights(h, exponent=exponent)), F.rain_plane(h.shape, 1.0)), A, "1024: a fixed point")
