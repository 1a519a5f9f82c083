"""The implicit fluvial stage on the GPU (nz_fluvial_implicit*, ImplicitFluvialStage) against the walk of
tests/fluvial_implicit_ref.py, bit for bit throughout: sizes on and across the 64-column / 16-row tile edges with and without
a sea and the two maps at a small and a large time step, the batch form, the long chain with an ample and with an exhausted
budget (all or nothing), the sweep hook, a reused work buffer, the three float modes, planes carved from a guarded slab, the
proceed word and the tally, bad arguments, the stage in a pipeline, and a 1024^2 filled tile checked as a fixed point."""
import ctypes as C
import math

import numpy as np
import pytest

import drainage_ref as D
import fluvial_implicit_ref as R
import fluvial_ref as F
import terrain_tiles as T
from test_gpu_slab import PAIRS, carved, memo
from test_gpu_watershed import tile

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
RES = [1, 2, 3, 5, 16, 63, 64, 65, 68, 97, 130, 160]
# a pass is at least one Jacobi step and the recurrence has the watershed's dependency graph, so "moves of the longest flow
# path" + 2 launches always suffice; no tile here has a path of 400 moves but the serpentine, which states its own budget
GENEROUS = 400
# the serpentine runs: at this step the reference Jacobi needs more than 11 000 steps (test below), the chain has 12 403 moves
SERP_DT = 200.0
SERP_AMPLE = 12407


def area(key, h, sea=OFF):
    return memo(("implicit area", key, sea), lambda: D.accumulate(h, 1.0, sea)[0])


def maps(res):
    """(hardness in [0, 1), upliftMap in [0, 2)) of a tile size."""
    def make():
        rng = np.random.default_rng(100 + res)
        return rng.random((res, res), dtype=f32), (rng.random((res, res), dtype=f32) * f32(2.0)).astype(f32)
    return memo(("implicit maps", res), make)


def ref(key, h, A, **kw):
    k = tuple(sorted((n, v if not isinstance(v, np.ndarray) else id(v)) for n, v in kw.items()))
    return memo(("implicit ref", key, k), lambda: R.walk(h, A, **kw))


def serpentine():
    def make():
        h = D.serpentine()
        A = D.accumulate(h)[0]
        return h, A, R.walk(h, A, dt=SERP_DT)
    return memo("implicit serpentine", make)


def assert_same(got, want, what):
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def desc_of(nj, erodibility=0.05, uplift=0.002, dt=1.0, seaLevel=OFF, budget=GENEROUS, hardness=None, upliftMap=None,
            proceed=None, tally=None):
    return nj._native.FluvialImplicitDesc(erodibility, uplift, dt, seaLevel, budget, hardness, upliftMap, proceed, tally)


SENTINEL = f32(-123.5)


def run_gpu(nj, ctx, h, A, budget=GENEROUS, work=None, hardness=None, upliftMap=None, proceed=None, tally=None, **kw):
    """One run on the host planes h, A (res x res, or count x res x res) -> (out, passes, converged); the inputs are checked
    to come back untouched.  proceed: None or the value of the device word; tally: None or a device tile of two int32."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    src, drain = ctx.from_host(h), ctx.from_host(np.ascontiguousarray(A, f32))
    out = ctx.from_host(np.full(h.size, SENTINEL, f32))
    hard = ctx.from_host(hardness) if hardness is not None else None
    upl = ctx.from_host(upliftMap) if upliftMap is not None else None
    word = ctx.from_host(np.array([proceed], np.int32)) if proceed is not None else None
    own = work is None
    if own:
        work = ctx.alloc(nj._native.lib.nz_fluvial_implicit_work_floats(res, count))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731
    desc = desc_of(nj, budget=budget, hardness=ptr(hard), upliftMap=ptr(upl), proceed=ptr(word), tally=ptr(tally), **kw)
    if h.ndim == 3:
        ctx.call("nz_fluvial_implicit_batch", src.ptr, drain.ptr, out.ptr, work.ptr, C.byref(desc), res, count).Complete()
    else:
        ctx.call("nz_fluvial_implicit", src.ptr, drain.ptr, out.ptr, work.ptr, C.byref(desc), res).Complete()
    got = out.ToArray(h.shape)
    assert_same(src.ToArray(h.shape), h, "the heights are read only")
    assert_same(drain.ToArray(h.shape), np.ascontiguousarray(A, f32), "the drainage is read only")
    status = ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()
    for t in (src, drain, out, hard, upl, word) + ((work,) if own else ()):
        if t is not None:
            t.Dispose()
    return got, int(status[0]), int(status[1])


# 1. sizes on and across the tile edges (the 16-byte and the 4-byte path, partial tiles both ways, one tile and many), each
# with and without a sea and the two maps, at a small and a large step
@pytest.mark.parametrize("res", RES)
def test_matches_the_walk(nj, ctx, res):
    h = tile(res)
    hard, upl = maps(res)
    for sea in (OFF, T.sea_at(h)):
        A = area(res, h, sea)
        for with_maps in (False, True):
            m = dict(hardness=hard, upliftMap=upl) if with_maps else {}
            for dt in (1.0, 200.0):
                what = "%d^2 sea %g maps %s dt %g" % (res, sea, with_maps, dt)
                want = ref(res, h, A, dt=dt, seaLevel=sea, **m)
                got, passes, conv = run_gpu(nj, ctx, h, A, dt=dt, seaLevel=sea, **m)
                assert conv == 1 and 2 <= passes <= GENEROUS, (what, passes)
                assert_same(got, want, what)
                out = F.outlets(h, sea)
                assert_same(got[out], h[out], what + ": outlets keep their bits")


# 2. every position of a batch is the tile alone
def test_a_batch_of_three(nj, ctx):
    res = 97
    a = tile(res)
    tiles = [a, np.ascontiguousarray(a[::-1]), np.ascontiguousarray(a.T)]
    areas = [area(("batch", k), t, 0.4) for k, t in enumerate(tiles)]
    kw = dict(dt=50.0, seaLevel=0.4)
    single = [run_gpu(nj, ctx, t, A, **kw) for t, A in zip(tiles, areas)]
    for k, (t, A, got) in enumerate(zip(tiles, areas, single)):
        assert got[2] == 1
        assert_same(got[0], ref(("batch", k), t, A, **kw), "single %d" % k)
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        got, passes, conv = run_gpu(nj, ctx, np.stack([tiles[j] for j in order]), np.stack([areas[j] for j in order]), **kw)
        assert conv == 1 and passes == max(s[1] for s in single)  # the status words cover the whole batch
        for k, j in enumerate(order):
            assert_same(got[k], single[j][0], "position %d tile %d" % (k, j))


# 3. the long chain: a budget that needs no measurement, and all or nothing when it runs out.  A value moves up the chain by
# at most four cells per sweep (a thread's own four) and 16 sweeps per pass, so 40 passes reach 2560 cells up; the reference
# Jacobi from the same start needs more than 11 000 steps for the last bit to settle, so 40 passes cannot suffice.  A pass
# is at least one Jacobi step, so the chain's 12 403 moves + 2 always do.
def test_the_serpentine_converges_and_an_exhausted_budget_returns_the_heights(nj, ctx, capsys):
    h, A, want = serpentine()
    steps = memo("implicit serpentine jacobi", lambda: R.jacobi(h, A, dt=SERP_DT)[1])
    assert 40 * 16 * 4 < steps <= SERP_AMPLE - 2
    tally = ctx.from_host(np.array([5, 70], np.int32))
    got, passes, conv = run_gpu(nj, ctx, h, A, budget=SERP_AMPLE, dt=SERP_DT, tally=tally)
    with capsys.disabled():
        print("\nserpentine 160^2 dt %g: reference Jacobi %d steps, converged after %d passes" % (SERP_DT, steps, passes))
    assert conv == 1 and 40 < passes <= steps + 2
    assert_same(got, want, "serpentine")
    counted = [6, 70 + passes]
    assert tally.ToArray().tolist() == counted
    for budget in (1, 2, 40):
        got, passes, conv = run_gpu(nj, ctx, h, A, budget=budget, dt=SERP_DT, tally=tally)
        assert (passes, conv) == (budget, 0)
        assert_same(got, h, "serpentine, budget %d: the heights bit for bit" % budget)
        assert tally.ToArray().tolist() == counted  # untouched
    tally.Dispose()


# 4. the schedule is free: every sweep cap gives the same plane; the default comes back afterwards
def test_the_sweep_cap_does_not_matter(nj, ctx):
    lib = nj._native.lib
    s, sA, swant = serpentine()
    f = tile(130)
    fA = area(130, f)
    fwant = ref(130, f, fA, dt=200.0)
    default = lib.nz_debug_fluvial_implicit_sweeps(0)
    try:
        for cap in (1, 2, 7, 200):
            lib.nz_debug_fluvial_implicit_sweeps(cap)
            got, passes, conv = run_gpu(nj, ctx, s, sA, budget=SERP_AMPLE, dt=SERP_DT)
            assert conv == 1, (cap, passes)
            assert_same(got, swant, "serpentine, cap %d" % cap)
            got, passes, conv = run_gpu(nj, ctx, f, fA, dt=200.0)
            assert conv == 1, (cap, passes)
            assert_same(got, fwant, "130^2, cap %d" % cap)
    finally:
        assert lib.nz_debug_fluvial_implicit_sweeps(0) == 200
    assert lib.nz_debug_fluvial_implicit_sweeps(0) == default == 16


# 5. one work buffer, uncleared, across 160^2 -> 65^2 -> 160^2: no tile byte, coefficient or verdict of a run survives
def test_a_reused_work_buffer(nj, ctx):
    work = ctx.alloc(nj._native.lib.nz_fluvial_implicit_work_floats(160, 1))
    for res in (160, 65, 160):
        h = tile(res) if res == 160 else np.ascontiguousarray(tile(97)[:65, 30:95])
        A = area(("reuse", res), h)
        got, _, conv = run_gpu(nj, ctx, h, A, dt=20.0, work=work)
        assert conv == 1
        assert_same(got, ref(("reuse", res), h, A, dt=20.0), "reused work %d" % res)
    h = tile(160)
    got, passes, conv = run_gpu(nj, ctx, h, area(("reuse", 160), h), budget=1, dt=20.0, work=work)  # ... nor a verdict
    assert (passes, conv) == (1, 0)
    assert_same(got, h, "reused work, one pass")
    work.Dispose()


# 6. all three float modes give the same bits
def test_float_modes_agree(nj, ctx):
    h = tile(97)
    hard, upl = maps(97)
    A = area(97, h, 0.4)
    kw = dict(dt=30.0, seaLevel=0.4, hardness=hard, upliftMap=upl)
    want = ref(97, h, A, **kw)
    assert_same(run_gpu(nj, ctx, h, A, **kw)[0], want, "strict")
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got = run_gpu(nj, mctx, h, A, **kw)
        finally:
            mctx.close()
        assert got[2] == 1
        assert_same(got[0], want, "float mode %d" % mode)


# 7. planes carved from one guarded allocation at four alignments and three mixed pairs: the guards stay silent
@pytest.mark.parametrize("res", [64, 97])
def test_on_slab_carved_planes(nj, ctx, res):
    h, n = tile(res), res * res
    hard, upl = maps(res)
    A = area(res, h)
    want = ref(res, h, A, dt=30.0, hardness=hard, upliftMap=upl)
    nwork = nj._native.lib.nz_fluvial_implicit_work_floats(res, 1)
    for p, q in PAIRS:
        r = p if p == q else (q + 1) % 4
        with carved(ctx, res, height=(n, p, h), drainage=(n, q, A), out=(n, q, None), work=(nwork, r, None),
                    hardness=(n, r, hard), upliftMap=(n, p, upl), tally=(2, q, np.zeros(2, np.int32), np.int32)) as (s, t):
            desc = desc_of(nj, dt=30.0, hardness=t.hardness.ptr, upliftMap=t.upliftMap.ptr, tally=t.tally.ptr)
            ctx.call("nz_fluvial_implicit", t.height.ptr, t.drainage.ptr, t.out.ptr, t.work.ptr, C.byref(desc), res).Complete()
            assert_same(t.out.ToArray((res, res)), want, ("out", res, p, q))
            assert_same(t.height.ToArray((res, res)), h, ("heights", res, p, q))
            status = ctx.wrap(t.work.ptr, 2, dtype=np.int32).ToArray()
            assert status[1] == 1 and t.tally.ToArray().tolist() == [1, int(status[0])]
            s.check()
    count = 3
    hh = np.stack([h, h[::-1].copy(), h.T.copy()])
    AA = np.stack([area(("slab", res, k), hh[k]) for k in range(count)])
    wants = np.stack([ref(("slab", res, k), hh[k], AA[k], dt=30.0) for k in range(count)])
    nwork = nj._native.lib.nz_fluvial_implicit_work_floats(res, count)
    for p, q in PAIRS:
        with carved(ctx, res, height=(count * n, p, hh), drainage=(count * n, p, AA), out=(count * n, q, None),
                    work=(nwork, (q + 2) % 4, None)) as (s, t):
            ctx.call("nz_fluvial_implicit_batch", t.height.ptr, t.drainage.ptr, t.out.ptr, t.work.ptr,
                     C.byref(desc_of(nj, dt=30.0)), res, count).Complete()
            assert_same(t.out.ToArray((count, res, res)), wants, ("batch out", res, p, q))
            s.check()


# 8. the proceed word: zero, the step is not applied and nothing is counted; one, it is; the tally sums two calls
def test_proceed_and_tally(nj, ctx):
    h = tile(97)
    A = area(97, h)
    want = ref(97, h, A, dt=30.0)
    tally = ctx.from_host(np.zeros(2, np.int32))
    got, passes, conv = run_gpu(nj, ctx, h, A, dt=30.0, proceed=0, tally=tally)
    assert (passes, conv) == (0, 0) and tally.ToArray().tolist() == [0, 0]
    assert_same(got, h, "proceed 0: out == h")
    got, p1, conv = run_gpu(nj, ctx, h, A, dt=30.0, proceed=1, tally=tally)
    assert conv == 1 and tally.ToArray().tolist() == [1, p1]
    assert_same(got, want, "proceed 1")
    got, p2, conv = run_gpu(nj, ctx, h, A, dt=30.0, proceed=-7, tally=tally)  # any word but zero
    assert conv == 1 and tally.ToArray().tolist() == [2, p1 + p2]
    assert_same(got, want, "proceed -7")
    # a work buffer that held a converged run, then a zero word: the status is {0, 0} again
    work = ctx.alloc(nj._native.lib.nz_fluvial_implicit_work_floats(97, 1))
    assert run_gpu(nj, ctx, h, A, dt=30.0, work=work)[1:] == (p1, 1)
    got, passes, conv = run_gpu(nj, ctx, h, A, dt=30.0, proceed=0, work=work, tally=tally)
    assert (passes, conv) == (0, 0) and tally.ToArray().tolist() == [2, p1 + p2]
    assert_same(got, h, "proceed 0 behind a converged run")
    # the chain the hosts use: the drainage call's converged word is the proceed word, on the device
    dwork = ctx.alloc(nj._native.lib.nz_drainage_area_work_floats(97, 1))
    src, dr, out = ctx.from_host(h), ctx.alloc(97 * 97), ctx.from_host(np.full(97 * 97, SENTINEL, f32))
    for dbudget, applied in ((GENEROUS, True), (2, False)):
        ddesc = nj._native.DrainageDesc(1.0, OFF, dbudget, None)
        ctx.call("nz_drainage_area", src.ptr, dr.ptr, dwork.ptr, C.byref(ddesc), 97, handle=False)
        desc = desc_of(nj, dt=30.0, proceed=dwork.ptr + 4)
        ctx.call("nz_fluvial_implicit", src.ptr, dr.ptr, out.ptr, work.ptr, C.byref(desc), 97).Complete()
        assert_same(out.ToArray((97, 97)), want if applied else h, "chained, drainage budget %d" % dbudget)
        assert ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray().tolist() == ([p1, 1] if applied else [0, 0])
    for t in (tally, work, dwork, src, dr, out):
        t.Dispose()


# 9. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    n = res * res
    sentinel = np.full((res, res), 7.25, f32)
    h, dr, out, hard, upl = (ctx.from_host(sentinel) for _ in range(5))
    work = ctx.alloc(nj._native.lib.nz_fluvial_implicit_work_floats(res, 1))
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    tally = ctx.from_host(np.array([4, 9], np.int32))
    word = ctx.from_host(np.array([1, 0, 0, 0], np.int32))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731

    def refused(name, desc, height=h, d=dr, o=out, wk=work, res=res, count=1):
        p = C.byref(desc) if desc is not None else None
        for entry, tail in (("nz_fluvial_implicit", (res,)), ("nz_fluvial_implicit_batch", (res, count))):
            if count != 1 and entry == "nz_fluvial_implicit":
                continue
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, ptr(height), ptr(d), ptr(o), ptr(wk), p, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))

    def good(**kw):
        kw = dict(dict(budget=10, hardness=hard.ptr, upliftMap=upl.ptr, proceed=word.ptr, tally=tally.ptr), **kw)
        return desc_of(nj, **kw)

    for field in ("erodibility", "uplift", "dt"):
        for v in (math.nan, math.inf, -math.inf, -1e-6):
            refused(field, good(**{field: v}))
    for v in (math.nan, math.inf, -math.inf):
        refused("seaLevel", good(seaLevel=v))
    refused("maxPasses", good(budget=0))
    refused("maxPasses", good(budget=-3))
    refused("desc", None)
    refused("height", good(), height=None)
    refused("drainage", good(), d=None)
    refused("out", good(), o=None)
    refused("work", good(), wk=None)
    refused("int32", good(), res=46340, count=2)  # 2 x 46340^2 cells: checked before any plane is touched
    inside = ctx.wrap(work.ptr + 4 * (work.Length - n // 2), n)  # a plane that begins inside `work`
    half_h = ctx.wrap(h.ptr + 4 * (n // 2), n)                    # ... inside the heights
    half_o = ctx.wrap(out.ptr + 4 * (n // 2), n)                  # ... inside out
    for plane, name in ((h, "height"), (half_h, "height"), (dr, "drainage"), (hard, "hardness"), (upl, "upliftMap"),
                        (inside, "work"), (work, "work")):
        refused("out overlaps " + name, good(), o=plane)
    refused("out overlaps hardness", good(hardness=half_o.ptr))
    refused("out overlaps upliftMap", good(upliftMap=half_o.ptr))
    refused("work overlaps height", good(), height=inside)
    refused("work overlaps drainage", good(), d=inside)
    refused("work overlaps hardness", good(hardness=inside.ptr))
    for plane, name in ((h, "height"), (dr, "drainage"), (out, "out"), (hard, "hardness"), (upl, "upliftMap"), (work, "work")):
        refused("tally overlaps " + name, good(tally=plane.ptr + 4 * (plane.Length - 2)))  # the plane's last two words
        refused("tally overlaps " + name, good(tally=plane.ptr))                          # ... and its first two
    refused("tally overlaps proceed", good(tally=word.ptr + 4, proceed=word.ptr + 8))  # its second word
    refused("proceed overlaps out", good(proceed=out.ptr + 8))
    refused("proceed overlaps work", good(proceed=work.ptr + 4))
    ctx.synchronize()
    for t in (h, dr, out, hard, upl):
        assert_same(t.ToArray((res, res)), sentinel, "a plane of a refused call")
    assert (work.ToArray() == f32(7.25)).all() and tally.ToArray().tolist() == [4, 9]
    # an empty payload is no error and touches nothing
    ctx.call("nz_fluvial_implicit", h.ptr, dr.ptr, out.ptr, work.ptr, C.byref(good()), 0).Complete()
    ctx.call("nz_fluvial_implicit_batch", h.ptr, dr.ptr, out.ptr, work.ptr, C.byref(good()), res, 0).Complete()
    assert_same(out.ToArray((res, res)), sentinel, "an empty payload")
    assert tally.ToArray().tolist() == [4, 9]
    # zero scalars and a sea of -FLT_MAX are in range, and the context still works
    hh = tile(97)[:res, :res].copy()
    A = D.accumulate(hh)[0]
    h.CopyFrom(hh), dr.CopyFrom(A)
    ctx.call("nz_fluvial_implicit", h.ptr, dr.ptr, out.ptr, work.ptr, C.byref(desc_of(nj, dt=30.0, tally=tally.ptr)), res).Complete()
    assert_same(out.ToArray((res, res)), R.walk(hh, A, dt=30.0), "after the refusals")
    assert tally.ToArray()[0] == 5
    for kw in (dict(erodibility=0.0), dict(uplift=0.0), dict(dt=0.0), dict(erodibility=-0.0, uplift=-0.0, dt=-0.0)):
        ctx.call("nz_fluvial_implicit", h.ptr, dr.ptr, out.ptr, work.ptr, C.byref(desc_of(nj, **kw)), res).Complete()
        assert_same(out.ToArray((res, res)), R.walk(hh, A, **kw), "in range: %s" % kw)
    for t in (h, dr, out, hard, upl, work, tally, word):
        t.Dispose()


def chain(key, h, iterations, **kw):
    return memo(("implicit chain", key, iterations, tuple(sorted(kw.items()))), lambda: R.chain(h, iterations, **kw))


# 10. the stage behind DepressionFillStage, 3 iterations at 97^2: heights and drainage equal the numpy chain; then a WRITE
# plane with an even and an odd count, a resized payload, a batch, and a budget that runs out
def test_stage_in_a_pipeline(nj, ctx):
    res = 97
    st = nj.ImplicitFluvialStage(ctx, iterations=3, dt=50.0)
    assert (st.drainage, st.steps, st.passes, st.converged) == (None, None, None, None)
    pipe = nj.BasePipeline([nj.DepressionFillStage(ctx), st], "valleys")
    fill = nj.DepressionFillStage(ctx)  # the filled heights the stage starts from, by a run of their own
    f = nj.GeneratorData("h", ctx.from_host(tile(res)), res, 0, 0)
    fill.ReceiveHandledInput(nj.PipelineWorkItem(f), nj.JobHandle())
    fill.jobHandle.Complete()
    filled = f.data.ToArray((res, res))
    assert F.pits(filled) == 0
    d = nj.GeneratorData("h", ctx.from_host(tile(res)), res, 0, 0)
    done = []
    pipe.Enqueue(d, completeAction=done.append)
    pipe.RunToCompletion()
    assert len(done) == 1
    wh, wA = chain("stage 97", filled, 3, dt=50.0)
    assert st.steps == 3 and st.converged is True and 6 <= st.passes <= 3 * (64 + res // 4)
    assert_same(d.data.ToArray((res, res)), wh, "the stage's heights")
    assert_same(st.drainage.ToArray((res, res)), wA, "the stage's drainage")
    assert not R.same(wh, filled)
    # a WRITE plane: the pair is used and swapped, `data` holds the result for an even and for an odd count
    for iterations in (2, 3):
        st.iterations = iterations
        first, second = ctx.from_host(filled), ctx.from_host(np.full(res * res, SENTINEL, f32))
        rw = nj.GeneratorData("h", first, res, 0, 0, write=second)
        st.ReceiveHandledInput(nj.PipelineWorkItem(rw), nj.JobHandle())
        st.jobHandle.Complete()
        wh, wA = chain("stage 97", filled, iterations, dt=50.0)
        assert st.steps == iterations and st.converged is True
        assert (rw.data is first) == (iterations % 2 == 0) and {id(rw.data), id(rw.write)} == {id(first), id(second)}
        assert_same(rw.data.ToArray((res, res)), wh, "WRITE plane, %d iterations" % iterations)
        assert_same(st.drainage.ToArray((res, res)), wA, "WRITE plane, %d iterations: drainage" % iterations)
        first.Dispose(), second.Dispose()
    # a resize to 65^2 without a WRITE plane, an even count: the planes and the work buffers follow the payload
    h65 = np.ascontiguousarray(filled[:65, 30:95])
    st.iterations = 2
    d65 = nj.GeneratorData("h", ctx.from_host(h65), 65, 0, 0)
    st.ReceiveHandledInput(nj.PipelineWorkItem(d65), nj.JobHandle())
    wh, wA = chain("stage 65", h65, 2, dt=50.0)
    assert st.steps == 2 and st.drainage.Length == 65 * 65
    assert_same(d65.data.ToArray((65, 65)), wh, "65^2 behind 97^2")
    assert_same(st.drainage.ToArray((65, 65)), wA, "65^2 behind 97^2: drainage")
    # a batch, a sea and the maps
    hh = np.stack([h65, np.ascontiguousarray(h65.T)])
    hard, upl = maps(65)
    m2 = [np.stack([m, np.ascontiguousarray(m.T)]) for m in (hard, upl)]
    dev = [ctx.from_host(m) for m in m2]
    sea = T.sea_at(h65)
    st2 = nj.ImplicitFluvialStage(ctx, 1, 0.1, 0.01, 20.0, 2.0, sea, GENEROUS, None, dev[0], dev[1])  # the positional order
    bt = nj.GeneratorDataBatch("h", ctx.from_host(hh), 65, None, 2)
    st2.ReceiveHandledInput(nj.PipelineWorkItem(bt), nj.JobHandle())
    assert st2.converged is True and st2.steps == 1
    got = bt.data.ToArray((2, 65, 65))
    for k in range(2):
        wh, wA = R.chain(hh[k], 1, 0.1, 0.01, 20.0, 2.0, sea, None, m2[0][k], m2[1][k])
        assert_same(got[k], wh, "batch tile %d" % k)
        assert_same(st2.drainage.ToArray((2, 65, 65))[k], wA, "batch tile %d: drainage" % k)
    # a budget that runs out on the long chain: no step is applied, the heights are unchanged
    s = D.serpentine()
    st3 = nj.ImplicitFluvialStage(ctx, iterations=2, dt=SERP_DT, maxPasses=2)
    ds = nj.GeneratorData("h", ctx.from_host(s), 160, 0, 0)
    st3.ReceiveHandledInput(nj.PipelineWorkItem(ds), nj.JobHandle())
    assert st3.steps == 0 and st3.converged is False and st3.passes == 0
    assert_same(ds.data.ToArray((160, 160)), s, "maxPasses 2 on the serpentine")
    for x in (st, st2, st3, fill):
        x.OnDestroy()
    assert st.drainage is None and st.steps is None


# 11. 1024^2, filled, the hosts' default budget: the many-tile skip logic.  No walk is needed: the fixed point is unique, so
# "one Jacobi step of the model over the result changes no bit" is a complete check
def test_1024_filled_is_the_fixed_point(nj, ctx, capsys):
    res = 1024
    n = res * res
    d = ctx.alloc(n)
    ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700).Complete()
    fwork = ctx.alloc(nj._native.lib.nz_fill_depressions_work_floats(res, 1))
    fdesc = nj._native.FillDesc(1e-4, OFF, 64 + res // 4, None)
    ctx.call("nz_fill_depressions", d.ptr, fwork.ptr, C.byref(fdesc), res).Complete()
    assert ctx.wrap(fwork.ptr, 2, dtype=np.int32).ToArray()[1] == 1
    fwork.Dispose()
    h = d.ToArray((res, res))
    st = nj.ImplicitFluvialStage(ctx, dt=100.0)  # every other default
    g = nj.GeneratorData("h", d, res, 0, 0)
    st.ReceiveHandledInput(nj.PipelineWorkItem(g), nj.JobHandle())
    steps, passes = st.steps, st.passes
    with capsys.disabled():
        print("\n1024^2 filled fBm, dt 100: %d step after %d passes (default budget %d)" % (steps, passes, 64 + res // 4))
    assert steps == 1 and st.converged is True
    got, A = g.data.ToArray((res, res)), st.drainage.ToArray((res, res))
    st.OnDestroy()
    d.Dispose()
    has, q, b, f = R.coefficients(h, A, dt=100.0)
    assert_same(R.step(got, has, q, b, f), got, "1024: one Jacobi step over the result")
    assert_same(got[~has], b[~has], "1024: outlets and pits")
    assert not R.same(got, h)
