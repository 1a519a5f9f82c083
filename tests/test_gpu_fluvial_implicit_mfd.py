"""The multiple-flow implicit fluvial stage on the GPU (nz_fluvial_implicit_mfd*, MfdFluvialStage) against the walk of
tests/fluvial_implicit_mfd_ref.py, bit for bit throughout: sizes on and across the 64-column / 16-row tile edges with and
without a sea and the two maps at exponents 1 and 4 and a small and a large time step, the batch form, the filled serpentine
with an ample and with exhausted budgets (all or nothing), the sweep hook, a reused work buffer, the three float modes, planes
carved from a guarded slab, the proceed word and the tally, bad arguments, the terrain families, NaN cells, the single-weight
closure against nz_fluvial_implicit on the device, the stage in a pipeline, and a 1024^2 filled tile checked as a fixed
point."""
import ctypes as C
import math

import numpy as np
import pytest

import drainage_mfd_ref as M
import fill_ref
import fill_stripe_cases as S
import fluvial_implicit_mfd_ref as R
import fluvial_implicit_ref as R1
import fluvial_ref as F
import relax_sweep_cases as RS
from test_gpu_drainage_mfd import tile
from test_gpu_slab import PAIRS, carved, memo

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
RES = [1, 2, 3, 5, 16, 63, 64, 65, 68, 97, 130, 160]
EXPONENTS = [1, 4]
# a pass is at least one Jacobi step and a Jacobi step settles one more level of the flow DAG, so "cells of the longest path
# of the DAG" + 2 launches always suffice; the tests that know the height ask for exactly that, the others for a budget no
# tile here comes near
GENEROUS = 600
SERP_DT = 200.0
SENTINEL = f32(-123.5)


def area(key, h, sea=OFF, exponent=1):
    """(multiple-flow drainage, DAG height) of a tile, computed once per key and shared; nothing writes to it."""
    return memo(("fmfd area", key, sea, exponent), lambda: M.walk(h, 1.0, sea, None, exponent))


def maps(res):
    """(hardness in [0, 1), upliftMap in [0, 2)) of a tile size."""
    def make():
        rng = np.random.default_rng(100 + res)
        return rng.random((res, res), dtype=f32), (rng.random((res, res), dtype=f32) * f32(2.0)).astype(f32)
    return memo(("fmfd maps", res), make)


def ref(key, h, A, **kw):
    """(h', DAG height) of the model, computed once per key and parameters."""
    k = tuple(sorted((n, v if not isinstance(v, np.ndarray) else id(v)) for n, v in kw.items()))
    return memo(("fmfd ref", key, k), lambda: R.walk(h, A, **kw))


def serpentine():
    """fill_stripe_cases.serpentine at 97^2, filled: h, A, h' at SERP_DT, DAG height."""
    def make():
        h = fill_ref.flood(S.serpentine(97, 97), S.EPS)
        A = M.walk(h)[0]
        return (h, A) + R.walk(h, A, dt=SERP_DT)
    return memo("fmfd serpentine", make)


def assert_same(got, want, what):
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def desc_of(nj, erodibility=0.05, uplift=0.002, dt=1.0, seaLevel=OFF, budget=GENEROUS, exponent=1, hardness=None,
            upliftMap=None, proceed=None, tally=None):
    return nj._native.FluvialImplicitMfdDesc(erodibility, uplift, dt, seaLevel, budget, exponent, hardness, upliftMap, proceed,
                                             tally)


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
        work = ctx.alloc(nj._native.lib.nz_fluvial_implicit_mfd_work_floats(res, count))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731
    desc = desc_of(nj, budget=budget, hardness=ptr(hard), upliftMap=ptr(upl), proceed=ptr(word), tally=ptr(tally), **kw)
    if h.ndim == 3:
        ctx.call("nz_fluvial_implicit_mfd_batch", src.ptr, drain.ptr, out.ptr, work.ptr, C.byref(desc), res, count).Complete()
    else:
        ctx.call("nz_fluvial_implicit_mfd", src.ptr, drain.ptr, out.ptr, work.ptr, C.byref(desc), res).Complete()
    got = out.ToArray(h.shape)
    assert_same(src.ToArray(h.shape), h, "the heights are read only")
    assert_same(drain.ToArray(h.shape), np.ascontiguousarray(A, f32), "the drainage is read only")
    status = ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()
    for t in (src, drain, out, hard, upl, word) + ((work,) if own else ()):
        if t is not None:
            t.Dispose()
    return got, int(status[0]), int(status[1])


# 1. sizes on and across the tile edges (the 16-byte and the 4-byte path, partial tiles both ways, one tile and many), plain
# and with a sea and the two maps, at a small and a large step; the budget is the DAG height + 2
@pytest.mark.parametrize("exponent", EXPONENTS)
@pytest.mark.parametrize("res", RES)
def test_matches_the_walk(nj, ctx, res, exponent):
    h = tile(res)
    hard, upl = maps(res)
    for sea, m in ((OFF, {}), (float(np.median(h)), dict(hardness=hard, upliftMap=upl))):
        A, _ = area(res, h, sea, exponent)
        for dt in (1.0, 200.0):
            what = "%d^2 exponent %d sea %g maps %s dt %g" % (res, exponent, sea, bool(m), dt)
            want, height = ref(res, h, A, dt=dt, seaLevel=sea, exponent=exponent, **m)
            got, passes, conv = run_gpu(nj, ctx, h, A, budget=height + 2, dt=dt, seaLevel=sea, exponent=exponent, **m)
            assert conv == 1 and 2 <= passes <= height + 1, (what, passes, height)
            assert_same(got, want, what)
            out = F.outlets(h, sea)
            assert_same(got[out], h[out], what + ": outlets keep their bits")


# 2. every position of a batch is the tile alone
def test_a_batch_of_three(nj, ctx):
    res = 97
    a = tile(res)
    tiles = [a, np.ascontiguousarray(a[::-1]), np.ascontiguousarray(a.T)]
    areas = [area(("batch", k), t, 0.4, 2)[0] for k, t in enumerate(tiles)]
    kw = dict(dt=50.0, seaLevel=0.4, exponent=2)
    single = [run_gpu(nj, ctx, t, A, **kw) for t, A in zip(tiles, areas)]
    for k, (t, A, got) in enumerate(zip(tiles, areas, single)):
        assert got[2] == 1
        assert_same(got[0], ref(("batch", k), t, A, **kw)[0], "single %d" % k)
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        got, passes, conv = run_gpu(nj, ctx, np.stack([tiles[j] for j in order]), np.stack([areas[j] for j in order]), **kw)
        assert conv == 1 and passes == max(s[1] for s in single)  # the status words cover the whole batch
        for k, j in enumerate(order):
            assert_same(got[k], single[j][0], "position %d tile %d" % (k, j))


# 3. the filled serpentine: a budget that needs no measurement, and all or nothing when it runs out.  One pass can never do:
# pass 0 changes every tile by decree.  For height // 2 the sweep cap is 1, where the kernel's schedule is
# fluvial_implicit_mfd_ref.one_sweep_passes exactly -- a value climbs a leg of the channel by one row per pass -- and that
# count, taken here from the reference and not from the device, lies above height // 2.
def test_the_serpentine_converges_and_an_exhausted_budget_returns_the_heights(nj, ctx, capsys):
    h, A, want, height = serpentine()
    lib = nj._native.lib
    needs = memo("fmfd serpentine one sweep", lambda: R.one_sweep_passes(h, A, height + 2, dt=SERP_DT))
    assert needs is not None and height // 2 < needs <= height + 2
    tally = ctx.from_host(np.array([5, 70], np.int32))
    got, passes, conv = run_gpu(nj, ctx, h, A, budget=height + 2, dt=SERP_DT, tally=tally)
    with capsys.disabled():
        print("\nfilled serpentine 97^2 dt %g: DAG height %d, %d passes at a cap of 1 by the reference, converged after %d"
              % (SERP_DT, height, needs, passes))
    assert conv == 1 and 2 <= passes <= height + 1
    assert_same(got, want, "serpentine")
    counted = [6, 70 + passes]
    assert tally.ToArray().tolist() == counted
    got, passes, conv = run_gpu(nj, ctx, h, A, budget=1, dt=SERP_DT, tally=tally)
    assert (passes, conv) == (1, 0)
    assert_same(got, h, "serpentine, budget 1: the heights bit for bit")
    assert lib.nz_debug_fluvial_implicit_mfd_sweeps(1) == 16
    try:
        got, passes, conv = run_gpu(nj, ctx, h, A, budget=height // 2, dt=SERP_DT, tally=tally)
        assert (passes, conv) == (height // 2, 0)
        assert_same(got, h, "serpentine, budget height // 2 at a cap of 1: the heights bit for bit")
        got, passes, conv = run_gpu(nj, ctx, h, A, budget=height + 2, dt=SERP_DT)
        assert conv == 1 and height // 2 < passes <= height + 1, (passes, needs)
        assert_same(got, want, "serpentine at a cap of 1")
    finally:
        assert lib.nz_debug_fluvial_implicit_mfd_sweeps(0) == 1
    assert tally.ToArray().tolist() == counted  # untouched by the two that ran out
    tally.Dispose()


# 4. the schedule is free: every sweep cap gives the same plane; the default comes back afterwards
def test_the_sweep_cap_does_not_matter(nj, ctx):
    lib = nj._native.lib
    s, sA, swant, sheight = serpentine()
    f = tile(130)
    fA, _ = area(130, f, OFF, 4)
    fwant, fheight = ref(130, f, fA, dt=200.0, exponent=4)
    default = lib.nz_debug_fluvial_implicit_mfd_sweeps(0)
    others = [lib.nz_debug_fluvial_implicit_sweeps(0), lib.nz_debug_drainage_mfd_sweeps(0)]
    try:
        for cap in (1, 2, 3, 5, 16, 200):
            lib.nz_debug_fluvial_implicit_mfd_sweeps(cap)
            got, passes, conv = run_gpu(nj, ctx, s, sA, budget=sheight + 2, dt=SERP_DT)
            assert conv == 1, (cap, passes)
            assert_same(got, swant, "serpentine, cap %d" % cap)
            got, passes, conv = run_gpu(nj, ctx, f, fA, budget=fheight + 2, dt=200.0, exponent=4)
            assert conv == 1, (cap, passes)
            assert_same(got, fwant, "130^2, cap %d" % cap)
    finally:
        assert lib.nz_debug_fluvial_implicit_mfd_sweeps(0) == 200
    assert lib.nz_debug_fluvial_implicit_mfd_sweeps(0) == default == 16
    assert [lib.nz_debug_fluvial_implicit_sweeps(0), lib.nz_debug_drainage_mfd_sweeps(0)] == others  # its own cap


# 5. one work buffer, uncleared, across 160^2 -> 65^2 -> 160^2: no tile byte, coefficient or verdict of a run survives
def test_a_reused_work_buffer(nj, ctx):
    work = ctx.alloc(nj._native.lib.nz_fluvial_implicit_mfd_work_floats(160, 1))
    for res in (160, 65, 160):
        h = tile(res) if res == 160 else np.ascontiguousarray(tile(97)[:65, 30:95])
        A, _ = area(("reuse", res), h)
        got, _, conv = run_gpu(nj, ctx, h, A, dt=20.0, work=work)
        assert conv == 1
        assert_same(got, ref(("reuse", res), h, A, dt=20.0)[0], "reused work %d" % res)
    h = tile(160)
    got, passes, conv = run_gpu(nj, ctx, h, area(("reuse", 160), h)[0], budget=1, dt=20.0, work=work)  # ... nor a verdict
    assert (passes, conv) == (1, 0)
    assert_same(got, h, "reused work, one pass")
    work.Dispose()


# 6. all three float modes give the same bits
def test_float_modes_agree(nj, ctx):
    h = tile(97)
    hard, upl = maps(97)
    A, _ = area(97, h, 0.4, 4)
    kw = dict(dt=30.0, seaLevel=0.4, exponent=4, hardness=hard, upliftMap=upl)
    want = ref(97, h, A, **kw)[0]
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
    A, _ = area(res, h, OFF, 2)
    want = ref(res, h, A, dt=30.0, exponent=2, hardness=hard, upliftMap=upl)[0]
    nwork = nj._native.lib.nz_fluvial_implicit_mfd_work_floats(res, 1)
    for p, q in PAIRS:
        r = p if p == q else (q + 1) % 4
        with carved(ctx, res, height=(n, p, h), drainage=(n, q, A), out=(n, q, None), work=(nwork, r, None),
                    hardness=(n, r, hard), upliftMap=(n, p, upl), tally=(2, q, np.zeros(2, np.int32), np.int32)) as (s, t):
            desc = desc_of(nj, dt=30.0, exponent=2, hardness=t.hardness.ptr, upliftMap=t.upliftMap.ptr, tally=t.tally.ptr)
            ctx.call("nz_fluvial_implicit_mfd", t.height.ptr, t.drainage.ptr, t.out.ptr, t.work.ptr, C.byref(desc), res).Complete()
            assert_same(t.out.ToArray((res, res)), want, ("out", res, p, q))
            assert_same(t.height.ToArray((res, res)), h, ("heights", res, p, q))
            status = ctx.wrap(t.work.ptr, 2, dtype=np.int32).ToArray()
            assert status[1] == 1 and t.tally.ToArray().tolist() == [1, int(status[0])]
            s.check()
    count = 3
    hh = np.stack([h, h[::-1].copy(), h.T.copy()])
    AA = np.stack([area(("slab", res, k), hh[k])[0] for k in range(count)])
    wants = np.stack([ref(("slab", res, k), hh[k], AA[k], dt=30.0)[0] for k in range(count)])
    nwork = nj._native.lib.nz_fluvial_implicit_mfd_work_floats(res, count)
    for p, q in PAIRS:
        with carved(ctx, res, height=(count * n, p, hh), drainage=(count * n, p, AA), out=(count * n, q, None),
                    work=(nwork, (q + 2) % 4, None)) as (s, t):
            ctx.call("nz_fluvial_implicit_mfd_batch", t.height.ptr, t.drainage.ptr, t.out.ptr, t.work.ptr,
                     C.byref(desc_of(nj, dt=30.0)), res, count).Complete()
            assert_same(t.out.ToArray((count, res, res)), wants, ("batch out", res, p, q))
            s.check()


# 8. the proceed word: zero, the step is not applied and nothing is counted; one, it is; the tally sums two calls
def test_proceed_and_tally(nj, ctx):
    h = tile(97)
    A, _ = area(97, h)
    want = ref(97, h, A, dt=30.0)[0]
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
    work = ctx.alloc(nj._native.lib.nz_fluvial_implicit_mfd_work_floats(97, 1))
    assert run_gpu(nj, ctx, h, A, dt=30.0, work=work)[1:] == (p1, 1)
    got, passes, conv = run_gpu(nj, ctx, h, A, dt=30.0, proceed=0, work=work, tally=tally)
    assert (passes, conv) == (0, 0) and tally.ToArray().tolist() == [2, p1 + p2]
    assert_same(got, h, "proceed 0 behind a converged run")
    # the chain the hosts use: the drainage call's converged word is the proceed word, on the device
    dwork = ctx.alloc(nj._native.lib.nz_drainage_mfd_work_floats(97, 1))
    src, dr, out = ctx.from_host(h), ctx.alloc(97 * 97), ctx.from_host(np.full(97 * 97, SENTINEL, f32))
    for dbudget, applied in ((GENEROUS, True), (2, False)):
        ddesc = nj._native.DrainageMfdDesc(1.0, OFF, dbudget, 1, None)
        ctx.call("nz_drainage_mfd", src.ptr, dr.ptr, dwork.ptr, C.byref(ddesc), 97, handle=False)
        desc = desc_of(nj, dt=30.0, proceed=dwork.ptr + 4)
        ctx.call("nz_fluvial_implicit_mfd", src.ptr, dr.ptr, out.ptr, work.ptr, C.byref(desc), 97).Complete()
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
    work = ctx.alloc(nj._native.lib.nz_fluvial_implicit_mfd_work_floats(res, 1))
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    tally = ctx.from_host(np.array([4, 9], np.int32))
    word = ctx.from_host(np.array([1, 0, 0, 0], np.int32))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731

    def refused(name, desc, height=h, d=dr, o=out, wk=work, res=res, count=1):
        p = C.byref(desc) if desc is not None else None
        for entry, tail in (("nz_fluvial_implicit_mfd", (res,)), ("nz_fluvial_implicit_mfd_batch", (res, count))):
            if count != 1 and entry == "nz_fluvial_implicit_mfd":
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
    for e in (0, 17, -1, 1 << 20):
        refused("exponent", good(exponent=e))
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
    ctx.call("nz_fluvial_implicit_mfd", h.ptr, dr.ptr, out.ptr, work.ptr, C.byref(good()), 0).Complete()
    ctx.call("nz_fluvial_implicit_mfd_batch", h.ptr, dr.ptr, out.ptr, work.ptr, C.byref(good()), res, 0).Complete()
    assert_same(out.ToArray((res, res)), sentinel, "an empty payload")
    assert tally.ToArray().tolist() == [4, 9]
    # zero scalars, the exponents at both ends and a sea of -FLT_MAX are in range, and the context still works
    hh = tile(97)[:res, :res].copy()
    h.CopyFrom(hh)
    for kw in (dict(dt=30.0), dict(erodibility=0.0), dict(uplift=0.0), dict(dt=0.0), dict(erodibility=-0.0, uplift=-0.0, dt=-0.0),
               dict(dt=30.0, exponent=16)):
        A = M.walk(hh, exponent=kw.get("exponent", 1))[0]
        dr.CopyFrom(A)
        ctx.call("nz_fluvial_implicit_mfd", h.ptr, dr.ptr, out.ptr, work.ptr, C.byref(desc_of(nj, tally=tally.ptr, **kw)), res).Complete()
        assert_same(out.ToArray((res, res)), R.walk(hh, A, **kw)[0], "in range: %s" % kw)
    assert tally.ToArray()[0] == 10
    for t in (h, dr, out, hard, upl, work, tally, word):
        t.Dispose()


# 10. the terrain families and the faint tile at 97^2: ties, plateaus, extreme scales, subnormal slopes
@pytest.mark.parametrize("exponent", EXPONENTS)
@pytest.mark.parametrize("kind", sorted(RS.TILES))
def test_the_terrain_families(nj, ctx, kind, exponent):
    h = memo(("fmfd family", kind), lambda: np.ascontiguousarray(RS.TILES[kind](97, np.random.default_rng(5)), f32))
    A, _ = area(("family", kind), h, OFF, exponent)
    for dt in (1.0, 200.0):
        want, height = ref(("family", kind), h, A, dt=dt, exponent=exponent)
        got, passes, conv = run_gpu(nj, ctx, h, A, budget=height + 2, dt=dt, exponent=exponent)
        assert conv == 1 and 2 <= passes <= height + 1, (kind, passes, height)
        assert_same(got, want, "%s exponent %d dt %g" % (kind, exponent, dt))


# 11. a NaN height sends and receives nothing; a NaN drainage cell travels upstream and nowhere else
def test_nan_cells(nj, ctx):
    res = 97
    z, x = 40, 50
    h = tile(res).copy()
    h[z, x] = np.nan
    A = M.walk(h)[0]
    want, height = R.walk(h, A, dt=20.0)
    got, passes, conv = run_gpu(nj, ctx, h, A, budget=height + 2, dt=20.0)
    assert conv == 1 and np.isnan(want).sum() == 1
    assert_same(got, want, "a NaN height")
    h = tile(res)
    A = area(res, h)[0].copy()
    A[z, x] = np.nan
    want, height = R.walk(h, A, dt=20.0)
    got, passes, conv = run_gpu(nj, ctx, h, A, budget=height + 2, dt=20.0)
    assert conv == 1 and 1 < np.isnan(want).sum() < res * res // 2
    assert_same(got, want, "a NaN drainage cell")


# 12. on the single-weight closure the entry and nz_fluvial_implicit give the same bits from the same A, on the device
def test_the_closure_equals_the_single_flow_entry(nj, ctx):
    h, A, _, height = serpentine()
    closed = memo("fmfd serpentine closure", lambda: R.single_closure(h))
    assert closed.sum() >= 600  # the test cannot pass empty
    res = h.shape[0]
    for dt in (1.0, SERP_DT):
        got, _, conv = run_gpu(nj, ctx, h, A, budget=height + 2, dt=dt)
        assert conv == 1
        src, dr, out = ctx.from_host(h), ctx.from_host(A), ctx.from_host(np.full(res * res, SENTINEL, f32))
        work = ctx.alloc(nj._native.lib.nz_fluvial_implicit_work_floats(res, 1))
        desc = nj._native.FluvialImplicitDesc(0.05, 0.002, dt, OFF, height + 2, None, None, None, None)
        ctx.call("nz_fluvial_implicit", src.ptr, dr.ptr, out.ptr, work.ptr, C.byref(desc), res).Complete()
        assert ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
        single = out.ToArray((res, res))
        assert_same(got[closed], single[closed], "the closure, dt %g" % dt)
        for t in (src, dr, out, work):
            t.Dispose()
    h2 = tile(97)  # ... and off a closure the two entries differ: this one erodes along the fan
    A2, _ = area(97, h2)
    got2 = run_gpu(nj, ctx, h2, A2, dt=50.0)[0]
    assert not R.same(got2, R1.walk(h2, A2, dt=50.0))


def chain(key, h, iterations, **kw):
    return memo(("fmfd chain", key, iterations, tuple(sorted(kw.items()))), lambda: R.chain(h, iterations, **kw))


# 13. the stage behind DepressionFillStage, 3 iterations at 97^2: heights and drainage equal the numpy chain; then a WRITE
# plane with an even and an odd count, a resized payload, a batch, and a budget that runs out
def test_stage_in_a_pipeline(nj, ctx):
    res = 97
    st = nj.MfdFluvialStage(ctx, iterations=3, dt=50.0, exponent=2)
    assert (st.drainage, st.steps, st.passes, st.converged) == (None, None, None, None)
    pipe = nj.BasePipeline([nj.DepressionFillStage(ctx), st], "fans")
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
    wh, wA = chain("stage 97", filled, 3, dt=50.0, exponent=2)
    assert st.steps == 3 and st.converged is True and 6 <= st.passes <= 3 * (128 + res // 2)
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
        wh, wA = chain("stage 97", filled, iterations, dt=50.0, exponent=2)
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
    wh, wA = chain("stage 65", h65, 2, dt=50.0, exponent=2)
    assert st.steps == 2 and st.drainage.Length == 65 * 65
    assert_same(d65.data.ToArray((65, 65)), wh, "65^2 behind 97^2")
    assert_same(st.drainage.ToArray((65, 65)), wA, "65^2 behind 97^2: drainage")
    # a batch, a sea and the maps
    hh = np.stack([h65, np.ascontiguousarray(h65.T)])
    hard, upl = maps(65)
    m2 = [np.stack([m, np.ascontiguousarray(m.T)]) for m in (hard, upl)]
    dev = [ctx.from_host(m) for m in m2]
    sea = float(np.median(h65))
    st2 = nj.MfdFluvialStage(ctx, 1, 0.1, 0.01, 20.0, 2.0, sea, 4, GENEROUS, None, dev[0], dev[1])  # the positional order
    bt = nj.GeneratorDataBatch("h", ctx.from_host(hh), 65, None, 2)
    st2.ReceiveHandledInput(nj.PipelineWorkItem(bt), nj.JobHandle())
    assert st2.converged is True and st2.steps == 1
    got = bt.data.ToArray((2, 65, 65))
    for k in range(2):
        wh, wA = R.chain(hh[k], 1, 0.1, 0.01, 20.0, 2.0, sea, 4, None, m2[0][k], m2[1][k])
        assert_same(got[k], wh, "batch tile %d" % k)
        assert_same(st2.drainage.ToArray((2, 65, 65))[k], wA, "batch tile %d: drainage" % k)
    # a budget that runs out: no step is applied, the heights are unchanged
    s = serpentine()[0]
    st3 = nj.MfdFluvialStage(ctx, iterations=2, dt=SERP_DT, maxPasses=1)
    ds = nj.GeneratorData("h", ctx.from_host(s), 97, 0, 0)
    st3.ReceiveHandledInput(nj.PipelineWorkItem(ds), nj.JobHandle())
    assert st3.steps == 0 and st3.converged is False and st3.passes == 0
    assert_same(ds.data.ToArray((97, 97)), s, "maxPasses 1 on the serpentine")
    for x in (st, st2, st3, fill):
        x.OnDestroy()
    assert st.drainage is None and st.steps is None


# 14. 1024^2, filled, the hosts' default budget: the many-tile skip logic.  No walk is needed: the fixed point is unique, so
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
    st = nj.MfdFluvialStage(ctx, dt=100.0, exponent=4)  # every other default
    g = nj.GeneratorData("h", d, res, 0, 0)
    st.ReceiveHandledInput(nj.PipelineWorkItem(g), nj.JobHandle())
    steps, passes = st.steps, st.passes
    with capsys.disabled():
        print("\n1024^2 filled fBm, dt 100, exponent 4: %d step after %d passes (default budget %d)" % (steps, passes, 128 + res // 2))
    assert steps == 1 and st.converged is True
    got, A = g.data.ToArray((res, res)), st.drainage.ToArray((res, res))
    st.OnDestroy()
    d.Dispose()
    G, b, Fk = R.coefficients(h, A, dt=100.0, exponent=4)
    assert_same(R.step(got, G, b, Fk), got, "1024: one Jacobi step over the result")
    opens = G.any(axis=0)
    assert_same(got[~opens], b[~opens], "1024: outlets, pits and flats")
    assert not R.same(got, h)
