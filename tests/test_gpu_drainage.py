"""The drainage-area stage on the GPU (nz_drainage_area*, DrainageAreaStage) against the topological walk of
tests/drainage_ref.py, bit for bit throughout: sizes on and across the 64-column / 16-row tile edges with and without a
rain map and a sea, the batch form, the long chain with an ample and with an exhausted budget (all or nothing), the sweep
hook, reused work planes, the three float modes, the plane as the fluvial stage's warm start, planes carved from a guarded
slab, bad arguments, the stage in a pipeline, and a 4096^2 filled tile checked as a fixed point."""
import ctypes as C
import math

import numpy as np
import pytest

import drainage_ref as D
import fluvial_ref as F
from test_gpu_slab import PAIRS, carved, memo
from test_hydraulic_ref import relief

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
RES = [1, 2, 3, 5, 16, 63, 64, 65, 68, 97, 130, 160]
# a pass is at least one Jacobi step, so "cells of the longest flow path" + 2 launches always suffice; no tile here has a
# path of 400 cells but the serpentine, which states its own budget
GENEROUS = 400


def tile(res):
    def make():
        if res <= 5:
            return np.random.default_rng(res).random((res, res), dtype=f32)
        return np.ascontiguousarray(relief(res, 500 if res == 160 else 300), f32)
    return memo(("drainage tile", res), make)


def rain_map(res, seed=0):
    return memo(("drainage rain map", res, seed),
                lambda: (np.random.default_rng(100 + res + seed).random((res, res), dtype=f32) * f32(1.5) + f32(0.25)).astype(f32))


def serpentine():
    return memo("drainage serpentine", lambda: (D.serpentine(),) + D.accumulate(D.serpentine()))  # h, A, tree height


def ref(res, rain, sea, mapped):
    return memo(("drainage ref", res, rain, sea, mapped),
                lambda: D.accumulate(tile(res), rain, sea, rain_map(res) if mapped else None))


def assert_bits(got, want, what):
    want = np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def desc_of(nj, rain, sea, budget, rm=None):
    return nj._native.DrainageDesc(rain, sea, budget, rm.ptr if rm is not None else None)


def run_gpu(nj, ctx, h, rain=1.0, sea=OFF, budget=GENEROUS, rm=None, work=None):
    """One run on the host plane h (res x res, or count x res x res) -> (drainage, passes, converged); the heights are
    checked to come back untouched."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    src, out = ctx.from_host(h), ctx.from_host(np.full(h.shape, np.nan, f32))
    own = work is None
    if own:
        work = ctx.alloc(nj._native.lib.nz_drainage_area_work_floats(res, count))
    m = ctx.from_host(np.ascontiguousarray(rm, f32)) if rm is not None else None
    desc = desc_of(nj, rain, sea, budget, m)
    if h.ndim == 3:
        ctx.call("nz_drainage_area_batch", src.ptr, out.ptr, work.ptr, C.byref(desc), res, count).Complete()
    else:
        ctx.call("nz_drainage_area", src.ptr, out.ptr, work.ptr, C.byref(desc), res).Complete()
    got = out.ToArray(h.shape)
    assert_bits(src.ToArray(h.shape), h, "the heights are read only")
    status = ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()
    for t in (src, out, m) + ((work,) if own else ()):
        if t is not None:
            t.Dispose()
    return got, int(status[0]), int(status[1])


# 1. sizes on and across the tile edges (the 16-byte and the 4-byte path, partial tiles both ways, one tile and many), each
# with and without a rain map and a sea
@pytest.mark.parametrize("res", RES)
def test_matches_the_topological_walk(nj, ctx, res):
    h = tile(res)
    sea = float(np.median(h))
    for rain, s, mapped in ((1.0, OFF, False), (0.75, OFF, True), (1.0, sea, False), (0.3, sea, True)):
        want, height = ref(res, rain, s, mapped)
        got, passes, conv = run_gpu(nj, ctx, h, rain, s, rm=rain_map(res) if mapped else None)
        assert conv == 1 and 2 <= passes <= height + 1, (res, rain, s, mapped, passes, height)
        assert_bits(got, want, "%d^2 rain %g sea %g map %s" % (res, rain, s, mapped))
    got, _, _ = run_gpu(nj, ctx, h)
    r = F.receivers(h)[0]
    assert (got == np.floor(got)).all() and float(got[r == F.NONE].astype(np.float64).sum()) == res * res


# 2. every position of a batch is the tile alone
def test_a_batch_of_three(nj, ctx):
    res = 97
    a = tile(res)
    tiles = [a, np.ascontiguousarray(a[::-1]), np.ascontiguousarray(a.T)]
    maps = [rain_map(res, k) for k in range(3)]
    single = [run_gpu(nj, ctx, t, 0.75, 0.4, rm=m) for t, m in zip(tiles, maps)]
    for t, m, (got, _, conv) in zip(tiles, maps, single):
        assert conv == 1
        assert_bits(got, D.accumulate(t, 0.75, 0.4, m)[0], "single")
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        got, passes, conv = run_gpu(nj, ctx, np.stack([tiles[j] for j in order]), 0.75, 0.4, rm=np.stack([maps[j] for j in order]))
        assert conv == 1 and passes == max(s[1] for s in single)  # the status words cover the whole batch
        for k, j in enumerate(order):
            assert_bits(got[k], single[j][0], "position %d tile %d" % (k, j))


# 3. the long chain: a budget that needs no measurement, and all or nothing when it runs out
def test_the_serpentine_converges_and_an_exhausted_budget_returns_the_start_state(nj, ctx, capsys):
    h, want, height = serpentine()
    got, passes, conv = run_gpu(nj, ctx, h, budget=height + 2)
    with capsys.disabled():
        print("\nserpentine 160^2: tree height %d, converged after %d passes" % (height, passes))
    assert conv == 1
    assert_bits(got, want, "serpentine")
    got, passes, conv = run_gpu(nj, ctx, h, budget=1)
    assert (passes, conv) == (1, 0)
    assert_bits(got, np.ones_like(h), "serpentine, one pass: rain everywhere")
    rm = rain_map(160)
    for budget in (1, 2, 7):
        got, passes, conv = run_gpu(nj, ctx, h, 0.3, budget=budget, rm=rm)
        assert (passes, conv) == (budget, 0)
        assert_bits(got, F.rain_plane(h.shape, 0.3, rm), "serpentine, budget %d: rain_c everywhere" % budget)


# 4. the schedule is free: every sweep cap gives the same plane; the default comes back afterwards
def test_the_sweep_cap_does_not_matter(nj, ctx):
    lib = nj._native.lib
    s, sw, sheight = serpentine()
    f = tile(130)
    fw, fheight = ref(130, 0.75, OFF, True)
    default = lib.nz_debug_drainage_sweeps(0)
    try:
        for cap in (1, 2, 7, 16, 200):
            lib.nz_debug_drainage_sweeps(cap)
            got, passes, conv = run_gpu(nj, ctx, s, budget=sheight + 2)
            assert conv == 1, (cap, passes)
            assert_bits(got, sw, "serpentine, cap %d" % cap)
            got, passes, conv = run_gpu(nj, ctx, f, 0.75, budget=fheight + 2, rm=rain_map(130))
            assert conv == 1, (cap, passes)
            assert_bits(got, fw, "fBm 130^2, cap %d" % cap)
    finally:
        assert lib.nz_debug_drainage_sweeps(0) == 200
    assert lib.nz_debug_drainage_sweeps(0) == default >= 1


# 5. the same work planes twice, uncleared, with another tile: no tile byte or donor byte of the first run survives
def test_reused_work_planes(nj, ctx):
    res = 130
    work = ctx.alloc(nj._native.lib.nz_drainage_area_work_floats(res, 1))
    a, b = tile(res), np.ascontiguousarray(tile(res).T[::-1])
    for h in (a, b, a):
        got, _, conv = run_gpu(nj, ctx, h, work=work)
        assert conv == 1
        assert_bits(got, D.accumulate(h)[0], "reused work")
    got, passes, conv = run_gpu(nj, ctx, b, budget=1, work=work)  # ... nor a verdict
    assert (passes, conv) == (1, 0)
    assert_bits(got, np.ones_like(b), "reused work, one pass")
    work.Dispose()


# 6. all three float modes give the same bits
def test_float_modes_agree(nj, ctx):
    h, rm = tile(97), rain_map(97)
    want = run_gpu(nj, ctx, h, 0.3, 0.4, rm=rm)
    assert_bits(want[0], D.accumulate(h, 0.3, 0.4, rm)[0], "strict")
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got = run_gpu(nj, mctx, h, 0.3, 0.4, rm=rm)
        finally:
            mctx.close()
        assert_bits(got[0], want[0], "float mode %d" % mode)
        assert got[1:] == want[1:]


# 7. the plane is a drainageIn: the fluvial stage continues from it as the model does
def test_warm_start_of_the_fluvial_stage(nj, ctx):
    res = 97
    h = tile(res)
    A, _, conv = run_gpu(nj, ctx, h)
    assert conv == 1
    assert_bits(A, D.accumulate(h)[0], "the drainage")
    src, din = ctx.from_host(h), ctx.from_host(A)
    work = ctx.alloc(nj._native.lib.nz_fluvial_erosion_work_floats(res, 1))
    desc = nj._native.FluvialDesc(3, 0.05, 0.002, 1.0, 1.0, OFF, None, None, None, din.ptr)
    ctx.call("nz_fluvial_erosion", src.ptr, work.ptr, C.byref(desc), res).Complete()
    hw, aw = F.run(h, 3, drainageIn=A)
    assert_bits(src.ToArray((res, res)), hw, "fluvial heights from the warm start")
    assert_bits(ctx.wrap(work.ptr, res * res).ToArray((res, res)), aw, "fluvial drainage from the warm start")
    assert not D.same(hw, F.run(h, 3)[0])  # the warm start matters
    for t in (src, din, work):
        t.Dispose()


# 8. planes carved from one guarded allocation at four alignments and three mixed pairs: the guards stay silent
@pytest.mark.parametrize("res", [64, 97])
def test_on_slab_carved_planes(nj, ctx, res):
    h, rm, n = tile(res), rain_map(res), res * res
    want = D.accumulate(h, 0.75, OFF, rm)[0]
    nwork = nj._native.lib.nz_drainage_area_work_floats(res, 1)
    for p, q in PAIRS:
        r = p if p == q else (q + 1) % 4
        with carved(ctx, res, height=(n, p, h), drainage=(n, q, None), work=(nwork, r, None), rain=(n, q, rm)) as (s, t):
            ctx.call("nz_drainage_area", t.height.ptr, t.drainage.ptr, t.work.ptr, C.byref(desc_of(nj, 0.75, OFF, GENEROUS, t.rain)),
                     res).Complete()
            assert_bits(t.drainage.ToArray((res, res)), want, (res, p, q))
            assert_bits(t.height.ToArray((res, res)), h, ("heights", res, p, q))
            assert ctx.wrap(t.work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
            s.check()
    count = 3
    hh = np.stack([h, h[::-1].copy(), h.T.copy()])
    want = np.stack([D.accumulate(hh[k])[0] for k in range(count)])
    nwork = nj._native.lib.nz_drainage_area_work_floats(res, count)
    for p, q in PAIRS:
        with carved(ctx, res, height=(count * n, p, hh), drainage=(count * n, q, None), work=(nwork, (q + 2) % 4, None)) as (s, t):
            ctx.call("nz_drainage_area_batch", t.height.ptr, t.drainage.ptr, t.work.ptr, C.byref(desc_of(nj, 1.0, OFF, GENEROUS)),
                     res, count).Complete()
            assert_bits(t.drainage.ToArray((count, res, res)), want, ("batch", res, p, q))
            s.check()


# 9. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    n = res * res
    sentinel = np.full((res, res), 7.25, f32)
    h, out, rm = ctx.from_host(sentinel), ctx.from_host(sentinel), ctx.from_host(sentinel)
    work = ctx.alloc(nj._native.lib.nz_drainage_area_work_floats(res, 1))
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731

    def refused(name, desc, height=h, drainage=out, wk=work):
        p = C.byref(desc) if desc is not None else None
        for entry, tail in (("nz_drainage_area", (res,)), ("nz_drainage_area_batch", (res, 1))):
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, ptr(height), ptr(drainage), ptr(wk), p, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))

    for v in (math.nan, math.inf, -math.inf):
        refused("rain", desc_of(nj, v, OFF, 10))
        refused("seaLevel", desc_of(nj, 1.0, v, 10))
    refused("rain", desc_of(nj, -1e-6, OFF, 10))
    refused("maxPasses", desc_of(nj, 1.0, OFF, 0))
    refused("maxPasses", desc_of(nj, 1.0, OFF, -3))
    refused("desc", None)
    good = desc_of(nj, 1.0, OFF, 10)
    refused("height", good, height=None)
    refused("drainage", good, drainage=None)
    inside = ctx.wrap(work.ptr + 4 * (work.Length - n // 2), n)  # a plane that begins inside `work`
    half_h = ctx.wrap(h.ptr + 4 * (n // 2), n)                    # ... inside the heights
    half_m = ctx.wrap(rm.ptr + 4 * (n // 2), n)                   # ... inside the rain map
    for plane in (h, half_h, inside, work):
        refused("drainage overlaps", good, drainage=plane)
    for plane in (rm, half_m):
        refused("drainage overlaps rainMap", desc_of(nj, 1.0, OFF, 10, rm), drainage=plane)
    refused("work overlaps height", good, height=inside)
    refused("work overlaps rainMap", desc_of(nj, 1.0, OFF, 10, inside))
    ctx.synchronize()
    for t in (h, out, rm):
        assert_bits(t.ToArray((res, res)), sentinel, "a plane of a refused call")
    assert (work.ToArray() == f32(7.25)).all()
    # an empty payload is no error and touches nothing
    ctx.call("nz_drainage_area", h.ptr, out.ptr, work.ptr, C.byref(good), 0).Complete()
    ctx.call("nz_drainage_area_batch", h.ptr, out.ptr, work.ptr, C.byref(good), res, 0).Complete()
    assert_bits(out.ToArray((res, res)), sentinel, "an empty payload")
    # a sea level of -FLT_MAX and a rain of 0 are in range, and the context still works
    hh = tile(97)[:res, :res].copy()
    h.CopyFrom(hh)
    ctx.call("nz_drainage_area", h.ptr, out.ptr, work.ptr, C.byref(desc_of(nj, 0.0, OFF, 200)), res).Complete()
    assert not out.ToArray().any() and ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
    ctx.call("nz_drainage_area", h.ptr, out.ptr, work.ptr, C.byref(desc_of(nj, 1.0, OFF, 200)), res).Complete()
    assert_bits(out.ToArray((res, res)), D.accumulate(hh)[0], "after the refusals")
    for t in (h, out, rm, work):
        t.Dispose()


# 10. the stage behind NoiseStage and DepressionFillStage, one tile and a batch; the plane as the fluvial stage's warm start
def test_stage_in_a_pipeline(nj, ctx):
    res = 128
    st = nj.DrainageAreaStage(ctx)
    assert (st.drainage, st.passes, st.converged) == (None, None, None)
    noise = nj.NoiseStage(ctx, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300)
    pipe = nj.BasePipeline([noise, nj.DepressionFillStage(ctx), st], "rivers")
    d = nj.GeneratorData("h", ctx.alloc(res * res), res, 0, 0)
    done = []
    pipe.Enqueue(d, completeAction=done.append)
    pipe.RunToCompletion()
    assert len(done) == 1
    h = d.data.ToArray((res, res))
    assert F.pits(h) == 0  # filled
    want, height = D.accumulate(h)
    assert st.converged is True and 2 <= st.passes <= min(height + 1, 64 + res // 4)
    A = st.drainage.ToArray((res, res))
    assert_bits(A, want, "the stage's drainage")
    assert float(A[F.outlets(h)].astype(np.float64).sum()) == res * res  # every river reaches the border
    # a caller's plane, a rain map, a batch -- and the plane handed on to the fluvial stage
    hh = np.stack([h, np.ascontiguousarray(h.T)])
    rm = np.stack([rain_map(res), rain_map(res, 1)])
    out, m = ctx.alloc(2 * res * res), ctx.from_host(rm)
    st2 = nj.DrainageAreaStage(ctx, rain=0.5, seaLevel=float(np.median(h)), maxPasses=GENEROUS, rainMap=m, out=out)
    b = nj.GeneratorDataBatch("h", ctx.from_host(hh), res, None, 2)
    st2.ReceiveHandledInput(nj.PipelineWorkItem(b), nj.JobHandle())
    assert st2.converged is True and st2.drainage is out
    got = out.ToArray((2, res, res))
    for k in range(2):
        assert_bits(got[k], D.accumulate(hh[k], 0.5, float(np.median(h)), rm[k])[0], "batch tile %d" % k)
    assert_bits(b.data.ToArray((2, res, res)), hh, "the heights pass through")
    fl = nj.FluvialErosionStage(ctx, iterations=2, rain=0.5, seaLevel=float(np.median(h)), rainMap=m, drainageIn=out)
    fl.ReceiveHandledInput(nj.PipelineWorkItem(b), nj.JobHandle())
    fl.jobHandle.Complete()
    hw, aw = F.run(hh[1], 2, rain=0.5, seaLevel=float(np.median(h)), rainMap=rm[1], drainageIn=got[1])
    assert_bits(b.data.ToArray((2, res, res))[1], hw, "fluvial behind the stage")
    assert_bits(fl.drainage.ToArray((2, res, res))[1], aw, "fluvial drainage behind the stage")
    # a budget that runs out: the start state, converged False
    st3 = nj.DrainageAreaStage(ctx, maxPasses=2)
    d3 = nj.GeneratorData("h", ctx.from_host(h), res, 0, 0)
    st3.ReceiveHandledInput(nj.PipelineWorkItem(d3), nj.JobHandle())
    assert st3.converged is False and st3.passes == 2
    assert_bits(st3.drainage.ToArray((res, res)), np.ones_like(h), "budget of 2")
    with pytest.raises(ValueError):
        nj.DrainageAreaStage(ctx, out=ctx.alloc(5)).ReceiveHandledInput(nj.PipelineWorkItem(d3), nj.JobHandle())
    for s in (st, st2, st3, fl):
        s.OnDestroy()
    assert st.drainage is None and st.passes is None


# 11. 4096^2, filled, rain 1, the hosts' default budget.  No oracle is needed: the fixed point is unique, so "one step of the
# model's accumulation returns the plane" is a complete check
def test_4096_filled_is_the_fixed_point(nj, ctx, capsys):
    res = 4096
    n = res * res
    d = ctx.alloc(n)
    ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700).Complete()
    fwork = ctx.alloc(nj._native.lib.nz_fill_depressions_work_floats(res, 1))
    fdesc = nj._native.FillDesc(1e-4, OFF, 64 + res // 4, None)
    ctx.call("nz_fill_depressions", d.ptr, fwork.ptr, C.byref(fdesc), res).Complete()
    assert ctx.wrap(fwork.ptr, 2, dtype=np.int32).ToArray()[1] == 1
    fwork.Dispose()
    h = d.ToArray((res, res))
    st = nj.DrainageAreaStage(ctx)  # every default
    g = nj.GeneratorData("h", d, res, 0, 0)
    st.ReceiveHandledInput(nj.PipelineWorkItem(g), nj.JobHandle())
    passes, conv = st.passes, st.converged
    with capsys.disabled():
        print("\n4096^2 filled fBm: converged %s after %d passes (default budget %d)" % (conv, passes, 64 + res // 4))
    assert conv is True
    A = st.drainage.ToArray((res, res))
    assert_bits(d.ToArray((res, res)), h, "4096: the heights")
    st.OnDestroy()
    d.Dispose()
    r = F.receivers(h)[0]
    assert_bits(F.drainage(A, r, F.rain_plane(h.shape, 1.0)), A, "4096: a fixed point")
    assert (A == np.floor(A)).all()
    assert float(A[r == F.NONE].astype(np.float64).sum()) == n
