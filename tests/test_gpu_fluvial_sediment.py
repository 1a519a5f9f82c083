"""The sediment stage on the GPU (nz_fluvial_sediment*, SedimentFluvialStage, host_demo's sediment mode) against the walk of
tests/fluvial_sediment_ref.py, bit for bit throughout: sizes on and across the 64-column / 16-row tile edges with and
without a sea and the two maps at a small and a large time step, two deposition coefficients and three iteration counts,
the closure on nz_fluvial_implicit, the batch form, the long chain with an ample budget and with budgets that run out in
each kind of series (all or nothing), the sweep hook, a reused work buffer, the three float modes, planes carved from a
guarded slab, the proceed word and the tally, bad arguments, the stage in a pipeline, the compiled C++ host, and a 1024^2
filled tile checked as a fixed point."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import drainage_mfd_ref as M
import drainage_ref as D
import fluvial_implicit_ref as R
import fluvial_ref as F
import fluvial_sediment_ref as S
import terrain_tiles as T
from test_gpu_slab import PAIRS, carved, memo
from test_gpu_watershed import tile
from watershed_ref import targets

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "noize_job_amd", "host", "host_demo")
RES = [1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 97, 160]
KS = (0, 1, 3)
SENTINEL = f32(-123.5)
SERP_DT = 200.0


def area(key, h, sea=OFF):
    """(A, cells of the longest flow path) of a tile: the path + 2 is a budget that always suffices, for each series."""
    return memo(("sediment area", key, sea), lambda: D.accumulate(h, 1.0, sea))


def maps(res):
    def make():
        rng = np.random.default_rng(100 + res)
        return rng.random((res, res), dtype=f32), (rng.random((res, res), dtype=f32) * f32(2.0)).astype(f32)
    return memo(("sediment maps", res), make)


def history(key, h, A, K, **kw):
    """[(h', flux, residual)] at 0 .. K iterations, computed once per key and argument set; nothing writes to it."""
    k = tuple(sorted((n, v if not isinstance(v, np.ndarray) else id(v)) for n, v in kw.items()))
    return memo(("sediment history", key, K, k), lambda: S.history(h, A, sedimentIterations=K, **kw))


def assert_same(got, want, what):
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def bits(x):
    return int(np.asarray(x, f32).reshape(1).view(np.uint32)[0])


def desc_of(nj, erodibility=0.05, uplift=0.002, dt=1.0, seaLevel=OFF, budget=400, hardness=None, upliftMap=None, proceed=None,
            tally=None, deposition=0.5, iterations=4, flux=None):
    return nj._native.FluvialSedimentDesc(erodibility, uplift, dt, seaLevel, budget, hardness, upliftMap, proceed, tally,
                                          deposition, iterations, flux)


class Run:
    pass


def run_gpu(nj, ctx, h, A, budget=400, work=None, hardness=None, upliftMap=None, proceed=None, tally=None, **kw):
    """One run on the host planes h, A (res x res, or count x res x res); the inputs are checked to come back untouched.
    -> out, flux (started as SENTINEL), passes, conv, residual (float32)."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    src, drain = ctx.from_host(h), ctx.from_host(np.ascontiguousarray(A, f32))
    out, flux = ctx.from_host(np.full(h.size, SENTINEL, f32)), ctx.from_host(np.full(h.size, SENTINEL, f32))
    hard = ctx.from_host(hardness) if hardness is not None else None
    upl = ctx.from_host(upliftMap) if upliftMap is not None else None
    word = ctx.from_host(np.array([proceed], np.int32)) if proceed is not None else None
    own = work is None
    if own:
        work = ctx.alloc(nj._native.lib.nz_fluvial_sediment_work_floats(res, count))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731
    desc = desc_of(nj, budget=budget, hardness=ptr(hard), upliftMap=ptr(upl), proceed=ptr(word), tally=ptr(tally),
                   flux=flux.ptr, **kw)
    if h.ndim == 3:
        ctx.call("nz_fluvial_sediment_batch", src.ptr, drain.ptr, out.ptr, work.ptr, C.byref(desc), res, count).Complete()
    else:
        ctx.call("nz_fluvial_sediment", src.ptr, drain.ptr, out.ptr, work.ptr, C.byref(desc), res).Complete()
    r = Run()
    r.out, r.flux = out.ToArray(h.shape), flux.ToArray(h.shape)
    assert_same(src.ToArray(h.shape), h, "the heights are read only")
    assert_same(drain.ToArray(h.shape), np.ascontiguousarray(A, f32), "the drainage is read only")
    status = ctx.wrap(work.ptr, 3, dtype=np.int32).ToArray()
    r.passes, r.conv, r.residual = int(status[0]), int(status[1]), status[2:3].view(f32)[0]
    for t in (src, drain, out, flux, hard, upl, word) + ((work,) if own else ()):
        if t is not None:
            t.Dispose()
    return r


def run_implicit(nj, ctx, h, A, budget=400, hardness=None, upliftMap=None, **kw):
    """nz_fluvial_implicit on the same planes -> (out, passes)."""
    res = h.shape[-1]
    src, drain, out = ctx.from_host(h), ctx.from_host(np.ascontiguousarray(A, f32)), ctx.alloc(h.size)
    hard = ctx.from_host(hardness) if hardness is not None else None
    upl = ctx.from_host(upliftMap) if upliftMap is not None else None
    work = ctx.alloc(nj._native.lib.nz_fluvial_implicit_work_floats(res, 1))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731
    desc = nj._native.FluvialImplicitDesc(kw.get("erodibility", 0.05), kw.get("uplift", 0.002), kw.get("dt", 1.0),
                                          kw.get("seaLevel", OFF), budget, ptr(hard), ptr(upl), None, None)
    ctx.call("nz_fluvial_implicit", src.ptr, drain.ptr, out.ptr, work.ptr, C.byref(desc), res).Complete()
    got, status = out.ToArray(h.shape), ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()
    assert status[1] == 1
    for t in (src, drain, out, hard, upl, work):
        if t is not None:
            t.Dispose()
    return got, int(status[0])


def check(r, want, what, budget, K):
    """A converged run against (h', flux, residual) of the walk."""
    assert r.conv == 1 and 2 * (2 * K + 1) <= r.passes <= budget * (2 * K + 1), (what, r.passes)
    assert_same(r.out, want[0], what + ": out")
    assert_same(r.flux, want[1], what + ": flux")
    assert bits(r.residual) == bits(want[2]), (what, r.residual, want[2])


# 1. sizes on and across the tile edges (the 16-byte and the 4-byte path, partial tiles both ways, one tile and many), each
# with and without a sea and the two maps, at a small and a large step, two coefficients and three iteration counts; the
# budget of every series is the tree height + 2
@pytest.mark.parametrize("res", RES)
def test_matches_the_walk(nj, ctx, res):
    h = tile(res)
    hard, upl = maps(res)
    for sea in (OFF, T.sea_at(h)):
        A, height = area(res, h, sea)
        budget = height + 2
        for with_maps in (False, True):
            m = dict(hardness=hard, upliftMap=upl) if with_maps else {}
            for dt in (1.0, 200.0):
                for G in (0.5, 1.0):
                    hist = history(res, h, A, max(KS), dt=dt, seaLevel=sea, deposition=G, **m)
                    for K in KS:
                        what = "%d^2 sea %g maps %s dt %g G %g K %d" % (res, sea, with_maps, dt, G, K)
                        r = run_gpu(nj, ctx, h, A, budget=budget, dt=dt, seaLevel=sea, deposition=G, iterations=K, **m)
                        check(r, hist[K], what, budget, K)
                        out = F.outlets(h, sea)
                        assert_same(r.out[out], h[out], what + ": outlets keep their bits")


# 2. the closure on the device: no iterations, or no deposition, is nz_fluvial_implicit's plane
@pytest.mark.parametrize("res", [64, 97])
def test_no_iterations_or_no_deposition_is_the_implicit_entry(nj, ctx, res):
    h = tile(res)
    hard, upl = maps(res)
    A, height = area(res, h, 0.4)
    kw = dict(dt=50.0, seaLevel=0.4)
    plain, p0 = run_implicit(nj, ctx, h, A, height + 2, hard, upl, **kw)
    assert_same(plain, R.walk(h, A, hardness=hard, upliftMap=upl, **kw), "nz_fluvial_implicit")
    r = run_gpu(nj, ctx, h, A, budget=height + 2, hardness=hard, upliftMap=upl, iterations=0, deposition=1.0, **kw)
    assert (r.conv, r.passes, bits(r.residual)) == (1, p0, 0)
    assert_same(r.out, plain, "K = 0")
    assert_same(r.flux, np.zeros_like(h), "K = 0: the flux is +0")
    for G in (0.0, -0.0):
        r = run_gpu(nj, ctx, h, A, budget=height + 2, hardness=hard, upliftMap=upl, iterations=3, deposition=G, **kw)
        assert r.conv == 1 and bits(r.residual) == 0
        assert_same(r.out, plain, "G = %r" % G)
        assert not (r.flux == 0).all()  # the flux is computed all the same


# 3. every position of a batch is the tile alone; the residual is the batch's
def test_a_batch_of_three(nj, ctx):
    res = 97
    a = tile(res)
    tiles = [a, np.ascontiguousarray(a[::-1]), np.ascontiguousarray(a.T)]
    areas = [area(("batch", k), t, 0.4)[0] for k, t in enumerate(tiles)]
    kw = dict(dt=50.0, seaLevel=0.4, deposition=1.0, iterations=2)
    single = [run_gpu(nj, ctx, t, A, **kw) for t, A in zip(tiles, areas)]
    for k, (t, A, got) in enumerate(zip(tiles, areas, single)):
        check(got, history(("batch", k), t, A, 2, dt=50.0, seaLevel=0.4, deposition=1.0)[2], "single %d" % k, 400, 2)
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        r = run_gpu(nj, ctx, np.stack([tiles[j] for j in order]), np.stack([areas[j] for j in order]), **kw)
        assert r.conv == 1 and bits(r.residual) == max(bits(s.residual) for s in single)
        for k, j in enumerate(order):
            assert_same(r.out[k], single[j].out, "position %d tile %d" % (k, j))
            assert_same(r.flux[k], single[j].flux, "position %d tile %d: flux" % (k, j))


# 4. the long chain.  A budget of the tree height + 2 needs no measurement.  Then the three ways a budget runs out, each all
# or nothing; `passes` tells which series ran out, because a series that did not come to rest stops every launch behind it.
#   a. 2 launches per series: solve 0 needs more.
#   b. dt 1e-3: f <= 0.006, a solve's changes die within a few cells and it rests after a few passes, while every cell of the
#      chain gives up something and Q has to travel all 12 560 cells, at most 64 per pass: 40 passes end in the accumulation.
#   c. An uplift map that makes b0 = +0 on every interior cell but one wall cell beside the channel's last cells (du = 1,
#      map = -h): solve 0 changes that one cell, Q is non-zero on the few cells below it, and the deposit there lifts the whole
#      chain upstream -- the model says so below -- at most 64 cells per pass: 40 passes end in the last solve.
def serpentine():
    def make():
        h = D.serpentine()
        A, height = D.accumulate(h)
        return h, A, height
    return memo("sediment serpentine", make)


def lifted_serpentine():
    def make():
        h, A, _ = serpentine()
        r = F.receivers(h)[0]
        q = targets(r)
        wall = [(z, x) for z in range(1, 159) for x in range(1, 159)
                if h[z, x] == f32(1e4) and r[z, x] != F.NONE and h.reshape(-1)[q[z, x]] <= f32(1.5)]
        um = (-h).astype(f32)
        um[wall[0]] = f32(-9999.0)
        kw = dict(dt=128.0, uplift=0.0078125, deposition=1.0)
        s = S.series(h, A, sedimentIterations=1, upliftMap=um, **kw)
        inner = np.zeros(h.shape, bool)
        inner[1:-1, 1:-1] = True
        assert np.count_nonzero(R.coefficients(h, A, upliftMap=um, dt=128.0, uplift=0.0078125)[2][inner]) == 1
        assert np.count_nonzero(s["Q"]) < 64                                           # the accumulation stays in one tile or two
        moved = (s["h"].view(np.uint32) != s["b"].view(np.uint32)) & (h < f32(1e4))   # chain cells the last solve moves
        assert (h[moved] / f32(0.25)).max() > 3 * 40 * 64                              # ... far beyond 40 passes' reach
        return um, kw
    return memo("sediment lifted serpentine", make)


def test_the_serpentine_converges_and_an_exhausted_budget_returns_the_heights(nj, ctx, capsys):
    h, A, height = serpentine()
    ample = height + 2
    tally = ctx.from_host(np.array([5, 70], np.int32))
    want = history("serpentine", h, A, 1, dt=SERP_DT)[1]
    r = run_gpu(nj, ctx, h, A, budget=ample, dt=SERP_DT, iterations=1, tally=tally)
    with capsys.disabled():
        print("\nserpentine 160^2 dt %g, K 1: converged after %d passes over 3 series" % (SERP_DT, r.passes))
    check(r, want, "serpentine", ample, 1)
    counted = [6, 70 + r.passes]
    assert tally.ToArray().tolist() == counted

    def nothing(r, what):
        assert r.conv == 0 and bits(r.residual) == 0, what
        assert_same(r.out, h, what + ": the heights bit for bit")
        assert (r.flux == SENTINEL).all(), what + ": the flux is untouched"
        assert tally.ToArray().tolist() == counted, what

    r = run_gpu(nj, ctx, h, A, budget=2, dt=SERP_DT, iterations=1, tally=tally)  # a.
    nothing(r, "budget 2")
    assert r.passes == 2
    small = dict(dt=1e-3, iterations=1)  # b.
    p0 = run_gpu(nj, ctx, h, A, budget=40, iterations=0, dt=1e-3)
    assert p0.conv == 1 and p0.passes < 40
    r = run_gpu(nj, ctx, h, A, budget=40, tally=tally, **small)
    nothing(r, "budget 40, dt 1e-3")
    assert r.passes == p0.passes + 40, (r.passes, p0.passes)
    um, kw = lifted_serpentine()  # c.
    p0 = run_gpu(nj, ctx, h, A, budget=40, upliftMap=um, **dict(kw, iterations=0))
    assert p0.conv == 1 and p0.passes < 40
    r = run_gpu(nj, ctx, h, A, budget=40, upliftMap=um, tally=tally, **dict(kw, iterations=1))
    nothing(r, "budget 40, the lifted chain")
    assert p0.passes + 40 < r.passes <= p0.passes + 80, (r.passes, p0.passes)
    r = run_gpu(nj, ctx, h, A, budget=ample, upliftMap=um, **dict(kw, iterations=1))
    check(r, history("lifted serpentine", h, A, 1, upliftMap=um, **kw)[1], "the lifted chain, ample", ample, 1)
    tally.Dispose()


# 5. the schedule is free: every sweep cap, one for both kinds of series, gives the same planes; the default comes back
def test_the_sweep_cap_does_not_matter(nj, ctx):
    lib = nj._native.lib
    s, sA, height = serpentine()
    swant = history("serpentine", s, sA, 1, dt=SERP_DT)[1]
    f = tile(130)
    fA, fheight = area(130, f)
    fwant = history(130, f, fA, 2, dt=200.0, deposition=1.0)[2]
    default = lib.nz_debug_fluvial_sediment_sweeps(0)
    others = [lib.nz_debug_fluvial_implicit_sweeps(0), lib.nz_debug_drainage_sweeps(0)]
    try:
        for cap in (1, 2, 7, 200):
            lib.nz_debug_fluvial_sediment_sweeps(cap)
            r = run_gpu(nj, ctx, s, sA, budget=height + 2, dt=SERP_DT, iterations=1)
            check(r, swant, "serpentine, cap %d" % cap, height + 2, 1)
            r = run_gpu(nj, ctx, f, fA, budget=fheight + 2, dt=200.0, deposition=1.0, iterations=2)
            check(r, fwant, "130^2, cap %d" % cap, fheight + 2, 2)
    finally:
        assert lib.nz_debug_fluvial_sediment_sweeps(0) == 200
    assert lib.nz_debug_fluvial_sediment_sweeps(0) == default == 16
    assert [lib.nz_debug_fluvial_implicit_sweeps(0), lib.nz_debug_drainage_sweeps(0)] == others  # a cap of its own


# 6. one work buffer, uncleared, across 160^2 -> 65^2 -> 160^2: no tile byte, coefficient, flux or verdict of a run survives
def test_a_reused_work_buffer(nj, ctx):
    work = ctx.alloc(nj._native.lib.nz_fluvial_sediment_work_floats(160, 1))
    for res in (160, 65, 160):
        h = tile(res) if res == 160 else np.ascontiguousarray(tile(97)[:65, 30:95])
        A = area(("reuse", res), h)[0]
        r = run_gpu(nj, ctx, h, A, dt=20.0, iterations=2, work=work)
        check(r, history(("reuse", res), h, A, 2, dt=20.0)[2], "reused work %d" % res, 400, 2)
    h = tile(160)
    r = run_gpu(nj, ctx, h, area(("reuse", 160), h)[0], budget=1, dt=20.0, iterations=2, work=work)  # ... nor a verdict
    assert (r.passes, r.conv, bits(r.residual)) == (1, 0, 0)
    assert_same(r.out, h, "reused work, one pass")
    work.Dispose()


# 7. all three float modes give the same bits
def test_float_modes_agree(nj, ctx):
    h = tile(97)
    hard, upl = maps(97)
    A = area(97, h, 0.4)[0]
    kw = dict(dt=30.0, seaLevel=0.4, hardness=hard, upliftMap=upl)
    want = history(97, h, A, 2, **kw)[2]
    check(run_gpu(nj, ctx, h, A, iterations=2, **kw), want, "strict", 400, 2)
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got = run_gpu(nj, mctx, h, A, iterations=2, **kw)
        finally:
            mctx.close()
        check(got, want, "float mode %d" % mode, 400, 2)


# 8. planes carved from one guarded allocation at four alignments and three mixed pairs: the guards stay silent
@pytest.mark.parametrize("res", [64, 97])
def test_on_slab_carved_planes(nj, ctx, res):
    h, n = tile(res), res * res
    hard, upl = maps(res)
    A = area(res, h)[0]
    want = history(res, h, A, 2, dt=30.0, hardness=hard, upliftMap=upl)[2]
    nwork = nj._native.lib.nz_fluvial_sediment_work_floats(res, 1)
    for p, q in PAIRS:
        r = p if p == q else (q + 1) % 4
        with carved(ctx, res, height=(n, p, h), drainage=(n, q, A), out=(n, q, None), work=(nwork, r, None),
                    hardness=(n, r, hard), upliftMap=(n, p, upl), flux=(n, r, None),
                    tally=(2, q, np.zeros(2, np.int32), np.int32)) as (s, t):
            desc = desc_of(nj, dt=30.0, hardness=t.hardness.ptr, upliftMap=t.upliftMap.ptr, tally=t.tally.ptr, iterations=2,
                           flux=t.flux.ptr)
            ctx.call("nz_fluvial_sediment", t.height.ptr, t.drainage.ptr, t.out.ptr, t.work.ptr, C.byref(desc), res).Complete()
            assert_same(t.out.ToArray((res, res)), want[0], ("out", res, p, q))
            assert_same(t.flux.ToArray((res, res)), want[1], ("flux", res, p, q))
            assert_same(t.height.ToArray((res, res)), h, ("heights", res, p, q))
            status = ctx.wrap(t.work.ptr, 3, dtype=np.int32).ToArray()
            assert status[1] == 1 and t.tally.ToArray().tolist() == [1, int(status[0])] and int(status[2]) == bits(want[2])
            s.check()
    count = 3
    hh = np.stack([h, h[::-1].copy(), h.T.copy()])
    AA = np.stack([area(("slab", res, k), hh[k])[0] for k in range(count)])
    wants = [history(("slab", res, k), hh[k], AA[k], 2, dt=30.0)[2] for k in range(count)]
    nwork = nj._native.lib.nz_fluvial_sediment_work_floats(res, count)
    for p, q in PAIRS:
        with carved(ctx, res, height=(count * n, p, hh), drainage=(count * n, p, AA), out=(count * n, q, None),
                    work=(nwork, (q + 2) % 4, None), flux=(count * n, (p + 1) % 4, None)) as (s, t):
            ctx.call("nz_fluvial_sediment_batch", t.height.ptr, t.drainage.ptr, t.out.ptr, t.work.ptr,
                     C.byref(desc_of(nj, dt=30.0, iterations=2, flux=t.flux.ptr)), res, count).Complete()
            assert_same(t.out.ToArray((count, res, res)), np.stack([w[0] for w in wants]), ("batch out", res, p, q))
            assert_same(t.flux.ToArray((count, res, res)), np.stack([w[1] for w in wants]), ("batch flux", res, p, q))
            s.check()


# 9. the proceed word: zero, the step is not applied and nothing is counted; one, it is; the tally sums two calls
def test_proceed_and_tally(nj, ctx):
    h = tile(97)
    A = area(97, h)[0]
    want = history(97, h, A, 2, dt=30.0)[2]
    tally = ctx.from_host(np.zeros(2, np.int32))
    kw = dict(dt=30.0, iterations=2)
    r = run_gpu(nj, ctx, h, A, proceed=0, tally=tally, **kw)
    assert (r.passes, r.conv, bits(r.residual)) == (0, 0, 0) and tally.ToArray().tolist() == [0, 0]
    assert_same(r.out, h, "proceed 0: out == h")
    assert (r.flux == SENTINEL).all()
    r = run_gpu(nj, ctx, h, A, proceed=1, tally=tally, **kw)
    p1 = r.passes
    check(r, want, "proceed 1", 400, 2)
    assert tally.ToArray().tolist() == [1, p1]
    r = run_gpu(nj, ctx, h, A, proceed=-7, tally=tally, **kw)  # any word but zero
    check(r, want, "proceed -7", 400, 2)
    assert tally.ToArray().tolist() == [2, p1 + r.passes]
    # a work buffer that held a converged run, then a zero word: the status is {0, 0, +0} again
    work = ctx.alloc(nj._native.lib.nz_fluvial_sediment_work_floats(97, 1))
    assert run_gpu(nj, ctx, h, A, work=work, **kw).passes == p1
    r = run_gpu(nj, ctx, h, A, proceed=0, work=work, **kw)
    assert (r.passes, r.conv, bits(r.residual)) == (0, 0, 0)
    assert_same(r.out, h, "proceed 0 behind a converged run")
    # the chain the hosts use: the drainage call's converged word is the proceed word, on the device
    dwork = ctx.alloc(nj._native.lib.nz_drainage_area_work_floats(97, 1))
    src, dr, out = ctx.from_host(h), ctx.alloc(97 * 97), ctx.from_host(np.full(97 * 97, SENTINEL, f32))
    for dbudget, applied in ((400, True), (2, False)):
        ddesc = nj._native.DrainageDesc(1.0, OFF, dbudget, None)
        ctx.call("nz_drainage_area", src.ptr, dr.ptr, dwork.ptr, C.byref(ddesc), 97, handle=False)
        desc = desc_of(nj, dt=30.0, iterations=2, proceed=dwork.ptr + 4)
        ctx.call("nz_fluvial_sediment", src.ptr, dr.ptr, out.ptr, work.ptr, C.byref(desc), 97).Complete()
        assert_same(out.ToArray((97, 97)), want[0] if applied else h, "chained, drainage budget %d" % dbudget)
        assert ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray().tolist() == ([p1, 1] if applied else [0, 0])
    for t in (tally, work, dwork, src, dr, out):
        t.Dispose()


# 10. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    n = res * res
    sentinel = np.full((res, res), 7.25, f32)
    h, dr, out, hard, upl, flux = (ctx.from_host(sentinel) for _ in range(6))
    work = ctx.alloc(nj._native.lib.nz_fluvial_sediment_work_floats(res, 1))
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    tally = ctx.from_host(np.array([4, 9], np.int32))
    word = ctx.from_host(np.array([1, 0, 0, 0], np.int32))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731

    def refused(name, desc, height=h, d=dr, o=out, wk=work, res=res, count=1):
        p = C.byref(desc) if desc is not None else None
        for entry, tail in (("nz_fluvial_sediment", (res,)), ("nz_fluvial_sediment_batch", (res, count))):
            if count != 1 and entry == "nz_fluvial_sediment":
                continue
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, ptr(height), ptr(d), ptr(o), ptr(wk), p, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))

    def good(**kw):
        kw = dict(dict(budget=10, hardness=hard.ptr, upliftMap=upl.ptr, proceed=word.ptr, tally=tally.ptr, flux=flux.ptr), **kw)
        return desc_of(nj, **kw)

    # everything the implicit entry refuses
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
    refused("int32", good(), res=46340, count=2)
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
        refused("tally overlaps " + name, good(tally=plane.ptr + 4 * (plane.Length - 2)))
        refused("tally overlaps " + name, good(tally=plane.ptr))
    refused("tally overlaps proceed", good(tally=word.ptr + 4, proceed=word.ptr + 8))
    refused("proceed overlaps out", good(proceed=out.ptr + 8))
    refused("proceed overlaps work", good(proceed=work.ptr + 4))
    # this entry's own
    for v in (math.nan, math.inf, -math.inf, -1e-6):
        refused("deposition", good(deposition=v))
    refused("iterations", good(iterations=-1))
    for plane, name in ((h, "height"), (half_h, "height"), (dr, "drainage"), (out, "out"), (half_o, "out"), (hard, "hardness"),
                        (upl, "upliftMap"), (work, "work"), (inside, "work")):
        refused("flux overlaps " + name, good(flux=plane.ptr))
    refused("flux overlaps tally", good(tally=flux.ptr + 4 * (n - 2)))
    refused("flux overlaps proceed", good(proceed=flux.ptr + 8))
    ctx.synchronize()
    for t in (h, dr, out, hard, upl, flux):
        assert_same(t.ToArray((res, res)), sentinel, "a plane of a refused call")
    assert (work.ToArray() == f32(7.25)).all() and tally.ToArray().tolist() == [4, 9]
    # an empty payload is no error and touches nothing
    ctx.call("nz_fluvial_sediment", h.ptr, dr.ptr, out.ptr, work.ptr, C.byref(good()), 0).Complete()
    ctx.call("nz_fluvial_sediment_batch", h.ptr, dr.ptr, out.ptr, work.ptr, C.byref(good()), res, 0).Complete()
    assert_same(out.ToArray((res, res)), sentinel, "an empty payload")
    assert_same(flux.ToArray((res, res)), sentinel, "an empty payload: flux")
    assert tally.ToArray().tolist() == [4, 9]
    # zero scalars, no flux plane and a sea of -FLT_MAX are in range, and the context still works
    hh = tile(97)[:res, :res].copy()
    A = D.accumulate(hh)[0]
    h.CopyFrom(hh), dr.CopyFrom(A)
    for kw in (dict(dt=30.0), dict(erodibility=0.0), dict(uplift=0.0), dict(dt=0.0), dict(deposition=0.0), dict(iterations=0)):
        ctx.call("nz_fluvial_sediment", h.ptr, dr.ptr, out.ptr, work.ptr, C.byref(desc_of(nj, **kw)), res).Complete()
        ref_kw = dict(kw)
        K = ref_kw.pop("iterations", 4)
        assert_same(out.ToArray((res, res)), S.walk(hh, A, sedimentIterations=K, **ref_kw)[0], "in range: %s" % kw)
    for t in (h, dr, out, hard, upl, flux, work, tally, word):
        t.Dispose()


# 11. the stage behind DepressionFillStage, 3 iterations at 97^2, against the numpy chain: heights, drainage, flux and
# residual; then a WRITE plane with an even and an odd count, a resized payload, a batch with the options, multiple-flow
# routing, and a budget that runs out
def filled97(nj, ctx):
    res = 97
    fill = nj.DepressionFillStage(ctx)
    f = nj.GeneratorData("h", ctx.from_host(tile(res)), res, 0, 0)
    fill.ReceiveHandledInput(nj.PipelineWorkItem(f), nj.JobHandle())
    fill.jobHandle.Complete()
    filled = f.data.ToArray((res, res))
    fill.OnDestroy()
    assert F.pits(filled) == 0
    return filled


def chain(key, h, iterations, **kw):
    return memo(("sediment chain", key, iterations, tuple(sorted(kw.items()))), lambda: S.chain(h, iterations, **kw))


def test_stage_in_a_pipeline(nj, ctx):
    res = 97
    filled = filled97(nj, ctx)
    st = nj.SedimentFluvialStage(ctx, iterations=3, dt=50.0, recordFlux=True)
    assert isinstance(st, nj.ImplicitFluvialStage)
    assert (st.drainage, st.steps, st.passes, st.converged, st.flux, st.residual) == (None,) * 6
    assert (st.deposition, st.sedimentIterations) == (0.5, 4)
    pipe = nj.BasePipeline([nj.DepressionFillStage(ctx), st], "plains")
    d = nj.GeneratorData("h", ctx.from_host(tile(res)), res, 0, 0)
    done = []
    pipe.Enqueue(d, completeAction=done.append)
    pipe.RunToCompletion()
    assert len(done) == 1
    wh, wA, wQ, wr = chain("stage 97", filled, 3, dt=50.0)
    assert st.steps == 3 and st.converged is True and 3 * 18 <= st.passes <= 3 * 9 * (64 + res // 4)
    assert_same(d.data.ToArray((res, res)), wh, "the stage's heights")
    assert_same(st.drainage.ToArray((res, res)), wA, "the stage's drainage")
    assert_same(st.flux.ToArray((res, res)), wQ, "the stage's flux")
    assert bits(st.residual) == bits(wr)
    plain = R.chain(filled, 3, dt=50.0)[0]
    assert not R.same(wh, plain) and (wh >= plain).mean() > 0.9  # it deposits
    # a WRITE plane: the pair is used and swapped, `data` holds the result for an even and for an odd count
    for iterations in (2, 3):
        st.iterations = iterations
        first, second = ctx.from_host(filled), ctx.from_host(np.full(res * res, SENTINEL, f32))
        rw = nj.GeneratorData("h", first, res, 0, 0, write=second)
        st.ReceiveHandledInput(nj.PipelineWorkItem(rw), nj.JobHandle())
        st.jobHandle.Complete()
        wh, wA, wQ, wr = chain("stage 97", filled, iterations, dt=50.0)
        assert st.steps == iterations and st.converged is True
        assert (rw.data is first) == (iterations % 2 == 0) and {id(rw.data), id(rw.write)} == {id(first), id(second)}
        assert_same(rw.data.ToArray((res, res)), wh, "WRITE plane, %d iterations" % iterations)
        assert_same(st.flux.ToArray((res, res)), wQ, "WRITE plane, %d iterations: flux" % iterations)
        first.Dispose(), second.Dispose()
    # a resize to 65^2 without a WRITE plane, an even count: the planes and the work buffers follow the payload
    h65 = np.ascontiguousarray(filled[:65, 30:95])
    st.iterations = 2
    d65 = nj.GeneratorData("h", ctx.from_host(h65), 65, 0, 0)
    st.ReceiveHandledInput(nj.PipelineWorkItem(d65), nj.JobHandle())
    wh, wA, wQ, wr = chain("stage 65", h65, 2, dt=50.0)
    assert st.steps == 2 and st.drainage.Length == 65 * 65 and st.flux.Length == 65 * 65
    assert_same(d65.data.ToArray((65, 65)), wh, "65^2 behind 97^2")
    assert_same(st.flux.ToArray((65, 65)), wQ, "65^2 behind 97^2: flux")
    assert bits(st.residual) == bits(wr)
    # a batch, a sea and the maps, every parameter by position, no flux plane
    hh = np.stack([h65, np.ascontiguousarray(h65.T)])
    hard, upl = maps(65)
    m2 = [np.stack([m, np.ascontiguousarray(m.T)]) for m in (hard, upl)]
    dev = [ctx.from_host(m) for m in m2]
    sea = T.sea_at(h65)
    st2 = nj.SedimentFluvialStage(ctx, 1, 0.1, 0.01, 20.0, 2.0, sea, 400, None, dev[0], dev[1], nj.FlowRouting.Steepest, 1,
                                  1.0, 2, False)
    bt = nj.GeneratorDataBatch("h", ctx.from_host(hh), 65, None, 2)
    st2.ReceiveHandledInput(nj.PipelineWorkItem(bt), nj.JobHandle())
    assert st2.converged is True and st2.steps == 1 and st2.flux is None
    got = bt.data.ToArray((2, 65, 65))
    worst = 0
    for k in range(2):
        wh, wA, wQ, wr = S.chain(hh[k], 1, 0.1, 0.01, 20.0, 2.0, sea, None, m2[0][k], m2[1][k], 1.0, 2)
        assert_same(got[k], wh, "batch tile %d" % k)
        assert_same(st2.drainage.ToArray((2, 65, 65))[k], wA, "batch tile %d: drainage" % k)
        worst = max(worst, bits(wr))
    assert bits(st2.residual) == worst
    # multiple-flow routing: only the area changes
    st4 = nj.SedimentFluvialStage(ctx, iterations=2, dt=50.0, routing=nj.FlowRouting.Multiple, flowExponent=2, recordFlux=True)
    dm = nj.GeneratorData("h", ctx.from_host(h65), 65, 0, 0)
    st4.ReceiveHandledInput(nj.PipelineWorkItem(dm), nj.JobHandle())
    wh, wA, wQ, wr = S.chain(h65, 2, dt=50.0, area=lambda h, rain, sea, rm: M.walk(h, rain, sea, rm, 2))
    assert st4.steps == 2
    assert_same(dm.data.ToArray((65, 65)), wh, "multiple-flow routing")
    assert_same(st4.drainage.ToArray((65, 65)), wA, "multiple-flow routing: drainage")
    assert_same(st4.flux.ToArray((65, 65)), wQ, "multiple-flow routing: flux")
    # a budget that runs out on the long chain: no step is applied, the heights are unchanged
    s = D.serpentine()
    st3 = nj.SedimentFluvialStage(ctx, iterations=2, dt=SERP_DT, maxPasses=2)
    ds = nj.GeneratorData("h", ctx.from_host(s), 160, 0, 0)
    st3.ReceiveHandledInput(nj.PipelineWorkItem(ds), nj.JobHandle())
    assert st3.steps == 0 and st3.converged is False and st3.passes == 0 and st3.residual == 0.0
    assert_same(ds.data.ToArray((160, 160)), s, "maxPasses 2 on the serpentine")
    for x in (st, st2, st3, st4):
        x.OnDestroy()
    assert st.drainage is None and st.steps is None and st.flux is None and st.residual is None


# 12. 1024^2, filled, the hosts' default budget and defaults: the many-tile skip logic.  No walk is needed: both fixed
# points are unique, so "one Jacobi step of each series of the last iteration changes no bit" is a complete check of the
# last iteration given the one before, and the residual ties the two together
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
    K = 2
    runs = []
    for k in (K - 1, K):  # the same tile at K - 1 and at K iterations
        st = nj.SedimentFluvialStage(ctx, dt=100.0, sedimentIterations=k, recordFlux=True)
        g = nj.GeneratorData("h", ctx.from_host(h), res, 0, 0)
        st.ReceiveHandledInput(nj.PipelineWorkItem(g), nj.JobHandle())
        assert st.steps == 1 and st.converged is True
        runs.append((g.data.ToArray((res, res)), st.flux.ToArray((res, res)), st.residual, st.passes,
                     st.drainage.ToArray((res, res))))
        st.OnDestroy()
        g.data.Dispose()
    d.Dispose()
    (hp, _, _, _, A), (hk, Q, residual, passes, _) = runs
    with capsys.disabled():
        print("\n1024^2 filled fBm, dt 100, K %d: %d passes over %d series, residual %g" % (K, passes, 2 * K + 1, residual))
    has, q, b0, f = R.coefficients(h, A, dt=100.0)
    r = F.receivers(h)[0]
    e = (b0 - hp).astype(f32)
    assert_same(F.drainage(Q, r, e), Q, "1024: one Jacobi step of the accumulation over the flux")
    bk = S.deposit(Q, r, b0, A, F.outlets(h), 0.5)[1]
    assert_same(R.step(hk, has, q, bk, f), hk, "1024: one Jacobi step of the solve over the result")
    assert_same(hk[~has], bk[~has], "1024: outlets and pits")
    dd = np.abs(hk - hp)
    assert bits(residual) == bits(dd[dd > 0].max()) and not R.same(hk, hp)


# 13. the compiled C++ host: host_demo's sediment mode drives SedimentFluvialStage through its defaults, every option, a
# WRITE plane, a batch of a single tile's length, an exhausted budget and OnDestroy, and dumps every plane and counter
def run_host_demo(res, planes, tmp_path):
    assert os.path.exists(EXE), "host_demo not built (run __graft_entry__.build())"
    src, out = str(tmp_path / "in.f32"), str(tmp_path / "out.bin")
    np.concatenate([np.ascontiguousarray(p, f32).ravel() for p in planes]).tofile(src)
    p = subprocess.run([EXE, str(res), out, "sediment", src], timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    raw = np.fromfile(out, np.uint8)
    got, values, at = {}, {}, 0
    for line in p.stdout.splitlines():
        w = line.split()
        if w[0] == "plane":
            assert w[1] not in got and w[2] == "f32", line
            got[w[1]] = raw[at:at + 4 * int(w[3])].view(f32)
            at += 4 * int(w[3])
        else:
            assert w[0] == "value" and w[1] not in values, line
            values[w[1]] = int(w[2])
    assert at == raw.size
    return got, values


def test_the_cpp_host_runs_the_stage(nj, ctx, tmp_path):
    res, m = 97, 32
    filled = filled97(nj, ctx)
    rain = (np.random.default_rng(7).random((res, res), dtype=f32) * f32(1.5) + f32(0.25)).astype(f32)
    hard, upl = maps(res)
    corner = np.ascontiguousarray(filled[:96, :96])
    blocks = np.stack([corner[m * z:m * z + m, m * x:m * x + m] for z in range(3) for x in range(3)])
    got, val = run_host_demo(res, [filled, rain, hard, upl, corner, blocks], tmp_path)
    plane = lambda name, shape=(res, res): got[name].reshape(shape)  # noqa: E731
    # a: defaults at dt 50, 3 iterations; no flux plane
    wh, wA, wQ, wr = chain("stage 97", filled, 3, dt=50.0)
    assert_same(plane("a.height"), wh, "a: heights")
    assert_same(plane("a.drainage"), wA, "a: drainage")
    assert (val["a.steps"], val["a.converged"], val["a.flux_null"], val["a.residual_bits"]) == (3, 1, 1, bits(wr))
    assert val["a.work_floats"] == nj._native.lib.nz_fluvial_sediment_work_floats(res, 1) and val["a.passes"] >= 3 * 18
    # b: every option
    wh, wA, wQ, wr = S.chain(filled, 2, 0.1, 0.01, 20.0, 2.0, 0.4, rain, hard, upl, 1.0, 2,
                             area=lambda h, rn, sea, rm: M.walk(h, rn, sea, rm, 2))
    assert_same(plane("b.height"), wh, "b: heights")
    assert_same(plane("b.drainage"), wA, "b: drainage")
    assert_same(plane("b.flux"), wQ, "b: flux")
    assert (val["b.steps"], val["b.converged"], val["b.flux_null"], val["b.residual_bits"]) == (2, 1, 0, bits(wr))
    # c: a WRITE plane and an odd count: the pair comes back swapped, `data` holds the result
    wh, wA, wQ, wr = chain("stage 97", filled, 3, dt=50.0)
    assert_same(plane("c.height"), wh, "c: heights")
    assert_same(plane("c.flux"), wQ, "c: flux")
    assert (val["c.swapped"], val["c.steps"], val["c.residual_bits"]) == (1, 3, bits(wr))
    # d1, d: the 96^2 corner, then nine 32^2 blocks -- the same length, more borders
    assert_same(plane("d1.height", (96, 96)), chain("corner 96", corner, 1, dt=50.0)[0], "d1: heights")
    db = plane("d.height", (9, m, m))
    worst = 0
    for k in range(9):
        wh, wA, wQ, wr = S.chain(blocks[k], 1, dt=50.0)
        assert_same(db[k], wh, "d: block %d" % k)
        assert_same(plane("d.drainage", (9, m, m))[k], wA, "d: block %d, drainage" % k)
        worst = max(worst, bits(wr))
    assert (val["d.steps"], val["d.converged"], val["d.residual_bits"]) == (1, 1, worst)
    assert val["d.work_floats"] == nj._native.lib.nz_fluvial_sediment_work_floats(m, 9) != val["d1.work_floats"]
    # e: a budget of 2: nothing is applied
    assert_same(plane("e.height"), filled, "e: heights")
    assert (val["e.steps"], val["e.converged"], val["e.passes"], val["e.residual_bits"]) == (0, 0, 0, 0)
    # f: OnDestroy
    assert (val["f.drainage_null"], val["f.flux_null"], val["f.steps"], val["f.work_floats"]) == (1, 1, -1, 0)
    assert val["f.residual_bits"] == bits(f32(-1.0))
