"""The stream-order stage on the GPU (nz_stream_order*, StreamOrderStage) against the walk of tests/stream_order_ref.py,
byte for byte throughout: sizes on and across the 64-column / 16-row tile edges with and without a sea, a drainage plane
and a link plane, the batch form, the two long chains with an ample and with an exhausted budget (all or nothing), the
sweep hook, a reused work buffer, the three float modes, planes carved from a guarded slab, bad arguments, the stage in a
pipeline, the tie-rich tiles, and a 1024^2 filled tile checked as a fixed point."""
import ctypes as C
import math

import numpy as np
import pytest

import drainage_ref as D
import fluvial_ref as F
import stream_order_ref as S
import terrain_tiles as T
from test_gpu_slab import PAIRS, carved, memo
from test_hydraulic_ref import relief

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
RES = [1, 2, 3, 5, 16, 63, 64, 65, 68, 97, 130, 160]
GUARD = 0xEE
# a pass is at least one Jacobi step, so "cells of the longest chain of channel donors" + 2 launches always suffice; no
# tile here has a chain of 400 cells but the two serpentines, which state their own budget
GENEROUS = 400


def tile(res):
    def make():
        if res <= 5:
            return np.random.default_rng(res).random((res, res), dtype=f32)
        return np.ascontiguousarray(relief(res, 500 if res == 160 else 300), f32)
    return memo(("watershed tile", res), make)  # the watershed tests' tiles, shared


def area(key, h):
    return memo(("stream order area", key), lambda: D.accumulate(h)[0])


def threshold_of(res):
    """A threshold that leaves a proper sub-network: 8 on the relief tiles (the figures of test_stream_order_ref), lower on
    the tiles too small to gather that much."""
    return 8.0 if res >= 16 else 2.0


def ref(key, h, sea=OFF, dr=None, thr=0.0):
    """(order, link, chain) of the walk, computed once per tile and argument set.  `dr` is identified by the key."""
    return memo(("stream order ref", key, sea, dr is not None, thr), lambda: S.walk(h, sea, dr, thr))


def long_tiles():
    def make():
        a, b = D.serpentine(), S.two_heads()
        da, db = S.channel_of(a), S.channel_of(b, ((1, 1), (2, 157)))
        return ((a, da) + S.walk(a, OFF, da, 0.5), (b, db) + S.walk(b, OFF, db, 0.5))  # h, drainage, order, link, chain
    return memo("stream order long tiles", make)


def assert_same(got, want, what):
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    g, w = (got, want) if got.dtype.itemsize == 1 else (got.view(np.uint32), want.view(np.uint32))
    bad = g != w
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def desc_of(nj, sea=OFF, thr=0.0, budget=GENEROUS, drainage=None):
    return nj._native.StreamOrderDesc(sea, thr, budget, drainage.ptr if drainage is not None else None)


def run_gpu(nj, ctx, h, sea=OFF, dr=None, thr=0.0, budget=GENEROUS, links=True, work=None):
    """One run on the host plane h (res x res, or count x res x res) -> (order, link, passes, converged), link None when
    not asked for; the planes start as sentinels, guard bytes stand behind the order plane, and the heights and the
    drainage are checked to come back untouched."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    n = h.size
    src = ctx.from_host(h)
    drain = ctx.from_host(np.ascontiguousarray(dr, f32)) if dr is not None else None
    order = ctx.from_host(np.full((n + 3) // 4 * 4 + 16, GUARD, np.uint8))
    link = ctx.from_host(np.full(n, -7, np.int32)) if links else None
    own = work is None
    if own:
        work = ctx.alloc(nj._native.lib.nz_stream_order_work_floats(res, count, 1 if links else 0))
    desc = desc_of(nj, sea, thr, budget, drain)
    planes = (src.ptr, order.ptr, link.ptr if links else None, work.ptr)
    if h.ndim == 3:
        ctx.call("nz_stream_order_batch", *planes, C.byref(desc), res, count).Complete()
    else:
        ctx.call("nz_stream_order", *planes, C.byref(desc), res).Complete()
    raw = order.ToArray()
    assert (raw[n:] == GUARD).all(), "bytes behind the order plane"
    got = (raw[:n].reshape(h.shape), link.ToArray(h.shape) if links else None)
    assert_same(src.ToArray(h.shape), h, "the heights are read only")
    if dr is not None:
        assert_same(drain.ToArray(h.shape), np.ascontiguousarray(dr, f32), "the drainage is read only")
    status = ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()
    for t in (src, drain, order, link) + ((work,) if own else ()):
        if t is not None:
            t.Dispose()
    return got + (int(status[0]), int(status[1]))


# 1. sizes on and across the tile edges (the wide and the narrow path, partial tiles both ways, one tile and many), each
# with and without a sea, a drainage plane and a link plane
@pytest.mark.parametrize("res", RES)
def test_matches_the_walk(nj, ctx, res):
    h = tile(res)
    A = area(res, h)
    thr = threshold_of(res)
    for sea in (OFF, float(np.median(h))):
        for dr, t in ((None, 0.0), (A, thr)):
            wo, wl, chain = ref(res, h, sea, dr, t)
            if dr is not None and res >= 16:
                assert 0 < (wo > 0).sum() < h.size  # a proper sub-network
            for links in (True, False):
                what = "%d^2 sea %g drainage %s links %s" % (res, sea, dr is not None, links)
                o, l, passes, conv = run_gpu(nj, ctx, h, sea, dr, t, links=links)
                assert conv == 1 and 2 <= passes <= chain + 2, (what, passes, chain)
                assert_same(o, wo, what + ": order")
                if links:
                    assert_same(l, wl, what + ": link")


# 2. every position of a batch is the tile alone, and the links are tile-local
def test_a_batch_of_three(nj, ctx):
    res = 97
    a = tile(res)
    tiles = [a, np.ascontiguousarray(a[::-1]), np.ascontiguousarray(a.T)]
    areas = [area(("batch", k), t) for k, t in enumerate(tiles)]
    single = [run_gpu(nj, ctx, t, 0.4, A, 8.0) for t, A in zip(tiles, areas)]
    for k, (t, A, got) in enumerate(zip(tiles, areas, single)):
        wo, wl, chain = ref(("batch", k), t, 0.4, A, 8.0)
        assert got[3] == 1
        assert_same(got[0], wo, "single: order")
        assert_same(got[1], wl, "single: link")
        assert -1 <= got[1].min() and 0 < got[1].max() < res * res
    for seq in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        o, l, passes, conv = run_gpu(nj, ctx, np.stack([tiles[j] for j in seq]), 0.4, np.stack([areas[j] for j in seq]), 8.0)
        assert conv == 1 and passes == max(s[2] for s in single)  # the status words cover the whole batch
        for k, j in enumerate(seq):
            assert_same(o[k], single[j][0], "position %d tile %d: order" % (k, j))
            assert_same(l[k], single[j][1], "position %d tile %d: link" % (k, j))


# 3. the long chains: a budget that needs no measurement, and all or nothing when it runs out
@pytest.mark.parametrize("which", [0, 1])
def test_a_long_chain_converges_and_an_exhausted_budget_returns_the_start_state(nj, ctx, capsys, which):
    h, dr, wo, wl, chain = long_tiles()[which]
    assert chain == 12405 and int(wo.max()) == 1 + which
    o, l, passes, conv = run_gpu(nj, ctx, h, OFF, dr, 0.5, budget=chain + 2)
    with capsys.disabled():
        print("\nlong chain %d, 160^2: %d cells, converged after %d passes" % (which, chain, passes))
    assert conv == 1 and 2 <= passes <= chain + 2
    assert_same(o, wo, "long chain: order")
    assert_same(l, wl, "long chain: link")
    so, sl = S.start(dr >= f32(0.5))
    for budget, links in ((3, True), (3, False), (1, True)):
        o, l, passes, conv = run_gpu(nj, ctx, h, OFF, dr, 0.5, budget=budget, links=links)
        if which == 0 and not links:  # one reach of order 1: without links the start state IS the fixed point
            assert (passes, conv) == (2, 1)
        else:
            assert (passes, conv) == (budget, 0)
        assert_same(o, so, "long chain, budget %d: 1 on the channel, 0 elsewhere" % budget)
        if links:
            assert_same(l, sl, "long chain, budget %d: own index on the channel, -1 elsewhere" % budget)


# 4. the schedule is free: every sweep cap gives the same planes, and a larger cap never takes more passes
def test_the_sweep_cap_does_not_matter(nj, ctx):
    lib = nj._native.lib
    s, sdr, so, sl, schain = long_tiles()[1]
    f = tile(130)
    A = area(130, f)
    fo, fl, fchain = ref(130, f, OFF, A, 8.0)
    default = lib.nz_debug_stream_order_sweeps(0)
    try:
        before = None
        for cap in (1, 2, 5, 200):
            lib.nz_debug_stream_order_sweeps(cap)
            o, l, p1, conv = run_gpu(nj, ctx, s, OFF, sdr, 0.5, budget=schain + 2)
            assert conv == 1, (cap, p1)
            assert_same(o, so, "two heads, cap %d: order" % cap)
            assert_same(l, sl, "two heads, cap %d: link" % cap)
            o, l, p2, conv = run_gpu(nj, ctx, f, OFF, A, 8.0, budget=fchain + 2)
            assert conv == 1, (cap, p2)
            assert_same(o, fo, "130^2, cap %d: order" % cap)
            assert_same(l, fl, "130^2, cap %d: link" % cap)
            assert before is None or (p1 <= before[0] and p2 <= before[1]), (cap, p1, p2, before)
            before = (p1, p2)
    finally:
        assert lib.nz_debug_stream_order_sweeps(0) == 200
    assert lib.nz_debug_stream_order_sweeps(0) == default >= 1


# 5. one work buffer, uncleared, across 160^2 -> 65^2 -> 160^2: no tile byte, donor byte or verdict of a run survives
def test_a_reused_work_buffer(nj, ctx):
    work = ctx.alloc(nj._native.lib.nz_stream_order_work_floats(160, 1, 1))
    for res in (160, 65, 160):
        h = tile(res) if res == 160 else np.ascontiguousarray(tile(97)[:65, 30:95])
        A = area(("reuse", res), h)
        wo, wl, chain = ref(("reuse", res), h, OFF, A, 8.0)
        o, l, _, conv = run_gpu(nj, ctx, h, OFF, A, 8.0, work=work)
        assert conv == 1
        assert_same(o, wo, "reused work %d: order" % res)
        assert_same(l, wl, "reused work %d: link" % res)
    o, l, passes, conv = run_gpu(nj, ctx, tile(160), budget=1, work=work)  # ... nor a verdict
    assert (passes, conv) == (1, 0)
    assert_same(o, np.ones((160, 160), np.uint8), "reused work, one pass: order")
    assert_same(l, np.arange(160 * 160, dtype=np.int32).reshape(160, 160), "reused work, one pass: link")
    work.Dispose()


# 6. all three float modes give the same bytes
def test_float_modes_agree(nj, ctx):
    h = tile(97)
    A = area(97, h)
    wo, wl, chain = ref(97, h, 0.4, A, 8.0)
    want = run_gpu(nj, ctx, h, 0.4, A, 8.0)
    assert_same(want[0], wo, "strict: order")
    assert_same(want[1], wl, "strict: link")
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got = run_gpu(nj, mctx, h, 0.4, A, 8.0)
        finally:
            mctx.close()
        for k, name in enumerate(("order", "link")):
            assert_same(got[k], want[k], "float mode %d: %s" % (mode, name))
        assert got[2:] == want[2:]


# 7. planes carved from one guarded allocation at four alignments and three mixed pairs, the order bytes at every byte
# phase in turn: the guards stay silent
@pytest.mark.parametrize("res", [64, 97])
def test_on_slab_carved_planes(nj, ctx, res):
    h, n = tile(res), res * res
    A = area(res, h)
    wo, wl, chain = ref(res, h, OFF, A, 8.0)
    for links in (1, 0):
        nwork = nj._native.lib.nz_stream_order_work_floats(res, 1, links)
        for i, (p, q) in enumerate(PAIRS):
            r = p if p == q else (q + 1) % 4
            # the order bytes: with the planes where these share a phase -- but once, all planes on 16 bytes, one byte off
            # -- and at odd bytes in the mixed pairs
            odd = i % 4 if p != q else 1 - links if p == 0 else 0
            spec = dict(height=(n, p, h), drainage=(n, q, A), work=(nwork, r, None),
                        order=(n, None, None, np.uint8, (4 * q + odd) % 16))
            if links:
                spec["link"] = (n, r, None, np.int32)
            with carved(ctx, res, **spec) as (s, t):
                ctx.call("nz_stream_order", t.height.ptr, t.order.ptr, t.link.ptr if links else None, t.work.ptr,
                         C.byref(desc_of(nj, OFF, 8.0, drainage=t.drainage)), res).Complete()
                assert_same(t.order.ToArray((res, res)), wo, ("order", res, p, q))
                if links:
                    assert_same(t.link.ToArray((res, res)), wl, ("link", res, p, q))
                assert_same(t.height.ToArray((res, res)), h, ("heights", res, p, q))
                assert_same(t.drainage.ToArray((res, res)), A, ("drainage", res, p, q))
                assert ctx.wrap(t.work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
                s.check()
    count = 3
    hh = np.stack([h, h[::-1].copy(), h.T.copy()])
    want = [ref(("slab", res, k), hh[k]) for k in range(count)]
    nwork = nj._native.lib.nz_stream_order_work_floats(res, count, 1)
    for i, (p, q) in enumerate(PAIRS):
        with carved(ctx, res, height=(count * n, p, hh), link=(count * n, q, None, np.int32),
                    order=(count * n, None, None, np.uint8, (4 * p + i) % 16), work=(nwork, (q + 2) % 4, None)) as (s, t):
            ctx.call("nz_stream_order_batch", t.height.ptr, t.order.ptr, t.link.ptr, t.work.ptr, C.byref(desc_of(nj)),
                     res, count).Complete()
            assert_same(t.order.ToArray((count, res, res)), np.stack([w[0] for w in want]), ("batch order", res, p, q))
            assert_same(t.link.ToArray((count, res, res)), np.stack([w[1] for w in want]), ("batch link", res, p, q))
            s.check()


# 8. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    n = res * res
    sentinel = np.full((res, res), 7.25, f32)
    h, dr, order, link = (ctx.from_host(sentinel) for _ in range(4))  # order: n floats hold the n bytes with room to spare
    work = ctx.alloc(nj._native.lib.nz_stream_order_work_floats(res, 1, 1))
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731

    def refused(name, desc, height=h, o=order, l=link, wk=work, res=res, count=1):
        p = C.byref(desc) if desc is not None else None
        for entry, tail in (("nz_stream_order", (res,)), ("nz_stream_order_batch", (res, count))):
            if count != 1 and entry == "nz_stream_order":
                continue
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, ptr(height), ptr(o), ptr(l), ptr(wk), p, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))

    for v in (math.nan, math.inf, -math.inf):
        refused("threshold", desc_of(nj, OFF, v, 10, dr))
        refused("threshold", desc_of(nj, OFF, v, 10))
    refused("seaLevel", desc_of(nj, math.nan, 1.0, 10, dr))
    refused("maxPasses", desc_of(nj, OFF, 1.0, 0, dr))
    refused("maxPasses", desc_of(nj, OFF, 1.0, -3))
    refused("desc", None)
    good = desc_of(nj, OFF, 1.0, 10, dr)
    refused("height", good, height=None)
    refused("order", good, o=None)
    refused("work", good, wk=None)
    refused("int32", good, res=46340, count=2)  # 2 x 46340^2 cells: checked before any plane is touched
    inside = ctx.wrap(work.ptr + 4 * (work.Length - n // 2), n)  # a plane that begins inside `work`
    half_h = ctx.wrap(h.ptr + 4 * (n // 2), n)                    # ... inside the heights
    half_d = ctx.wrap(dr.ptr + 4 * (n // 2), n)                   # ... inside the drainage
    half_l = ctx.wrap(link.ptr + 4 * (n // 2), n)                 # ... inside the links
    last_l = ctx.wrap(link.ptr + 3 * n, n)                        # the last n bytes of the links
    for plane in (h, half_h, dr, half_d, inside, work):
        refused("order overlaps", good, o=plane)
        refused("link overlaps", good, l=plane)
    refused("order overlaps link", good, o=half_l)
    refused("order overlaps link", good, o=last_l)
    refused("work overlaps height", good, height=inside)
    refused("work overlaps drainage", desc_of(nj, OFF, 1.0, 10, inside))
    ctx.synchronize()
    for t in (h, dr, order, link):
        assert_same(t.ToArray((res, res)), sentinel, "a plane of a refused call")
    assert (work.ToArray() == f32(7.25)).all()
    # an empty payload is no error and touches nothing
    ctx.call("nz_stream_order", h.ptr, order.ptr, link.ptr, work.ptr, C.byref(good), 0).Complete()
    ctx.call("nz_stream_order_batch", h.ptr, order.ptr, link.ptr, work.ptr, C.byref(good), res, 0).Complete()
    assert_same(order.ToArray((res, res)), sentinel, "an empty payload")
    # a sea of -FLT_MAX or +-inf is in range, a drainage plane with NaNs is no error -- those cells are no channel --
    # and the context still works
    hh = tile(97)[:res, :res].copy()
    A = area("after the refusals", hh).copy()
    A[::3, 1::4] = np.nan
    assert np.isnan(A).sum() > 50
    h.CopyFrom(hh)
    dr.CopyFrom(A)
    for sea in (OFF, -math.inf, 0.45, math.inf):
        wo, wl, chain = ref("after the refusals", hh, sea, A, 2.0)
        assert not wo[np.isnan(A)].any() and (wl[np.isnan(A)] == -1).all() and (wo > 0).sum() > 50
        ctx.call("nz_stream_order", h.ptr, order.ptr, link.ptr, work.ptr, C.byref(desc_of(nj, sea, 2.0, 200, dr)), res).Complete()
        assert_same(ctx.wrap(order.ptr, n, dtype=np.uint8).ToArray((res, res)), wo, "after the refusals: order")
        assert_same(ctx.wrap(link.ptr, n, dtype=np.int32).ToArray((res, res)), wl, "after the refusals: link")
        assert ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
    # everything lies under an infinite sea: no receivers, every channel cell a head of order 1
    assert_same(wo, (A >= f32(2.0)).astype(np.uint8), "an infinite sea")
    for t in (h, dr, order, link, work):
        t.Dispose()


# 9. the stage behind the fill and the drainage stage, then a resize, and what is not a device tile
def test_stage_in_a_pipeline(nj, ctx):
    def through(res, area_plane, st):
        pipe = nj.BasePipeline([nj.NoiseStage(ctx, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300),
                                nj.DepressionFillStage(ctx), nj.DrainageAreaStage(ctx, out=area_plane), st], "rivers")
        d = nj.GeneratorData("h", ctx.alloc(res * res), res, 0, 0)
        done = []
        pipe.Enqueue(d, completeAction=done.append)
        pipe.RunToCompletion()
        assert len(done) == 1
        h, A = d.data.ToArray((res, res)), area_plane.ToArray((res, res))
        assert F.pits(h) == 0  # filled
        wo, wl, chain = S.walk(h, OFF, A, 6.0)
        assert st.converged is True and 2 <= st.passes <= min(chain + 2, 64 + res // 4)
        assert st.order.dtype == np.uint8 and st.order.Length == st.links.Length == res * res
        got = st.links.ToArray((res, res))
        assert got.dtype == np.int32
        assert_same(st.order.ToArray((res, res)), wo, "%d^2: the stage's order" % res)
        assert_same(got, wl, "%d^2: the stage's links" % res)
        assert 0 < (wo > 0).sum() < res * res and wo.max() >= 2
        assert_same(d.data.ToArray((res, res)), h, "the heights pass through")
        d.data.Dispose()

    st = nj.StreamOrderStage(ctx, threshold=6.0, recordLinks=True)
    assert (st.order, st.links, st.passes, st.converged) == (None, None, None, None)
    a130, a65 = ctx.alloc(130 * 130), ctx.alloc(65 * 65)
    st.drainage = a130
    through(130, a130, st)
    st.drainage = a65  # a resize to 65^2: the planes and the work buffer follow the payload
    through(65, a65, st)
    # a drainage plane of another size, or something that is no device tile, raises before any launch
    d65 = nj.GeneratorData("h", ctx.from_host(tile(65)), 65, 0, 0)
    for bad in (a130, np.zeros(65 * 65, f32), 3.0):
        st.drainage = bad
        with pytest.raises((ValueError, TypeError)):
            st.ReceiveHandledInput(nj.PipelineWorkItem(d65), nj.JobHandle())
    # order only, every default: a batch, no link plane
    h65 = tile(65)
    hh = np.stack([h65, np.ascontiguousarray(h65.T)])
    st2 = nj.StreamOrderStage(ctx)
    bt = nj.GeneratorDataBatch("h", ctx.from_host(hh), 65, None, 2)
    st2.ReceiveHandledInput(nj.PipelineWorkItem(bt), nj.JobHandle())
    assert st2.converged is True and st2.links is None
    got = st2.order.ToArray((2, 65, 65))
    for k in range(2):
        assert_same(got[k], ref(("stage batch", k), hh[k])[0], "batch tile %d" % k)
    # a budget that runs out: the start state, converged False
    st3 = nj.StreamOrderStage(ctx, maxPasses=2, recordLinks=True)
    st3.ReceiveHandledInput(nj.PipelineWorkItem(d65), nj.JobHandle())
    assert st3.converged is False and st3.passes == 2
    assert_same(st3.order.ToArray((65, 65)), np.ones((65, 65), np.uint8), "budget of 2: order")
    assert_same(st3.links.ToArray((65, 65)), np.arange(65 * 65, dtype=np.int32).reshape(65, 65), "budget of 2: links")
    for s in (st, st2, st3):
        s.OnDestroy()
    assert st.order is None and st.passes is None
    for t in (a130, a65, d65.data, bt.data):
        t.Dispose()


# 10. one tile of each tie-rich family, at the sizes of the terrain sweep's tie pass
@pytest.mark.parametrize("res", [65, 130])
@pytest.mark.parametrize("name", sorted(T.TIES))
def test_tie_rich_tiles(nj, ctx, name, res):
    h = memo(("stream order ties", name, res), lambda: T.GENERATORS[name](res, np.random.default_rng(11)))
    A = area(("ties", name, res), h)
    for sea, dr, thr in ((OFF, None, 0.0), (T.sea_at(h), A, 2.0)):
        wo, wl, chain = ref(("ties", name, res), h, sea, dr, thr)
        o, l, passes, conv = run_gpu(nj, ctx, h, sea, dr, thr)
        assert conv == 1 and passes <= chain + 2, (name, passes, chain)
        assert_same(o, wo, name + ": order")
        assert_same(l, wl, name + ": link")


# 11. 1024^2, filled, the hosts' default budget: the many-tile skip logic.  No walk is needed: the fixed point is unique, so
# "one step of the model returns the planes" is a complete check
def test_1024_filled_is_the_fixed_point(nj, ctx, capsys):
    res = 1024
    n = res * res
    lib = nj._native.lib
    d = ctx.alloc(n)
    ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700).Complete()
    fwork = ctx.alloc(lib.nz_fill_depressions_work_floats(res, 1))
    fdesc = nj._native.FillDesc(1e-4, OFF, 64 + res // 4, None)
    ctx.call("nz_fill_depressions", d.ptr, fwork.ptr, C.byref(fdesc), res).Complete()
    assert ctx.wrap(fwork.ptr, 2, dtype=np.int32).ToArray()[1] == 1
    fwork.Dispose()
    h = d.ToArray((res, res))
    g = nj.GeneratorData("h", d, res, 0, 0)
    drain = nj.DrainageAreaStage(ctx)
    drain.ReceiveHandledInput(nj.PipelineWorkItem(g), nj.JobHandle())
    assert drain.converged is True
    shed = nj.WatershedStage(ctx, length=False, recordReceivers=True)
    shed.ReceiveHandledInput(nj.PipelineWorkItem(g), nj.JobHandle())
    assert shed.converged is True
    A, r = drain.drainage.ToArray((res, res)), shed.receivers.ToArray((res, res))
    thr = 100.0
    st = nj.StreamOrderStage(ctx, threshold=thr, drainage=drain.drainage, recordLinks=True)  # every other default
    st.ReceiveHandledInput(nj.PipelineWorkItem(g), nj.JobHandle())
    passes, conv = st.passes, st.converged
    with capsys.disabled():
        print("\n1024^2 filled fBm: converged %s after %d passes (default budget %d)" % (conv, passes, 64 + res // 4))
    assert conv is True
    o, l = st.order.ToArray((res, res)), st.links.ToArray((res, res))
    assert_same(d.ToArray((res, res)), h, "1024: the heights")
    assert_same(drain.drainage.ToArray((res, res)), A, "1024: the drainage")
    for s in (st, shed, drain):
        s.OnDestroy()
    d.Dispose()
    # the model's equations, cell by cell: the donor bits from the downloaded receivers and area, then one step
    ch = A >= f32(thr)
    bits = np.zeros((res, res), np.uint8)
    for k, (dx, dz) in enumerate(F.NEIGHBOURS):
        c, nb = F._window((res, res), dx, dz)
        bits[c] |= (((r[nb] == F.OPPOSITE[k]) & ch[nb]).astype(np.uint8) << k).astype(np.uint8)
    assert 1000 < ch.sum() < n // 4 and o.max() >= 4
    no, nl = S.step(o, l, ch, bits)
    assert_same(o, no, "1024: order is the model's function of its donors' orders")
    assert_same(l, nl, "1024: link is the one donor's, or the own index")
    assert np.array_equal(o > 0, ch) and np.array_equal(l >= 0, ch)
