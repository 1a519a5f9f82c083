"""The watershed stage on the GPU (nz_watershed*, WatershedStage) against the walk of tests/watershed_ref.py, bit for bit
throughout: sizes on and across the 64-column / 16-row tile edges with and without a sea, a length plane and a receiver
plane, the batch form, the long chain with an ample and with an exhausted budget (all or nothing), the sweep hook, a reused
work buffer, the three float modes, planes carved from a guarded slab, bad arguments, the stage in a pipeline, and a 1024^2
filled tile checked as a fixed point."""
import ctypes as C
import math

import numpy as np
import pytest

import drainage_ref as D
import fluvial_ref as F
import watershed_ref as W
from test_gpu_slab import PAIRS, carved, memo
from test_hydraulic_ref import relief

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
RES = [1, 2, 3, 5, 16, 63, 64, 65, 68, 97, 130, 160]
# a pass is at least one Jacobi step, so "moves of the longest flow path" + 2 launches always suffice; no tile here has a
# path of 400 moves but the serpentine, which states its own budget
GENEROUS = 400


def tile(res):
    def make():
        if res <= 5:
            return np.random.default_rng(res).random((res, res), dtype=f32)
        return np.ascontiguousarray(relief(res, 500 if res == 160 else 300), f32)
    return memo(("watershed tile", res), make)


def ref(h_key, h, sea=OFF, cs=1.0):
    """(basin, length, hops, receivers) of the walk, computed once per tile and argument set."""
    return memo(("watershed ref", h_key, sea, cs), lambda: W.walk(h, sea, cs) + (F.receivers(h, sea)[0],))


def serpentine():
    return memo("watershed serpentine", lambda: (D.serpentine(),) + W.walk(D.serpentine()))  # h, basin, length, hops


def assert_same(got, want, what):
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    g, w = (got, want) if got.dtype.itemsize == 1 else (got.view(np.uint32), want.view(np.uint32))
    bad = g != w
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def desc_of(nj, sea=OFF, cs=1.0, budget=GENEROUS):
    return nj._native.WatershedDesc(sea, cs, budget)


def run_gpu(nj, ctx, h, sea=OFF, cs=1.0, budget=GENEROUS, length=True, receivers=True, work=None):
    """One run on the host plane h (res x res, or count x res x res) -> (basin, length, receivers, passes, converged), a
    plane that was not asked for None; the heights are checked to come back untouched."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    n = h.size
    src = ctx.from_host(h)
    basin = ctx.from_host(np.full(n, -7, np.int32))
    ln = ctx.from_host(np.full(n, np.nan, f32)) if length else None
    rc = ctx.from_host(np.full((n + 3) // 4 * 4, 0xEE, np.uint8)) if receivers else None
    own = work is None
    if own:
        work = ctx.alloc(nj._native.lib.nz_watershed_work_floats(res, count, 1 if length else 0))
    desc = desc_of(nj, sea, cs, budget)
    planes = (src.ptr, basin.ptr, ln.ptr if length else None, rc.ptr if receivers else None, work.ptr)
    if h.ndim == 3:
        ctx.call("nz_watershed_batch", *planes, C.byref(desc), res, count).Complete()
    else:
        ctx.call("nz_watershed", *planes, C.byref(desc), res).Complete()
    got = (basin.ToArray(h.shape), ln.ToArray(h.shape) if length else None)
    codes = None
    if receivers:
        raw = rc.ToArray()
        assert (raw[n:] == 0xEE).all(), "bytes behind the receiver plane"
        codes = raw[:n].reshape(h.shape)
    assert_same(src.ToArray(h.shape), h, "the heights are read only")
    status = ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()
    for t in (src, basin, ln, rc) + ((work,) if own else ()):
        if t is not None:
            t.Dispose()
    return got + (codes, int(status[0]), int(status[1]))


# 1. sizes on and across the tile edges (the 16-byte and the 4-byte path, partial tiles both ways, one tile and many), each
# with and without a sea, a length plane and a receiver plane
@pytest.mark.parametrize("res", RES)
def test_matches_the_walk(nj, ctx, res):
    h = tile(res)
    for sea, cs in ((OFF, 1.0), (float(np.median(h)), 0.3)):
        wb, wl, hops, wr = ref(res, h, sea, cs)
        for length in (True, False):
            for receivers in (True, False):
                what = "%d^2 sea %g length %s receivers %s" % (res, sea, length, receivers)
                b, l, r, passes, conv = run_gpu(nj, ctx, h, sea, cs, length=length, receivers=receivers)
                assert conv == 1 and 2 <= passes <= int(hops.max()) + 2, (what, passes, int(hops.max()))
                assert_same(b, wb, what + ": basin")
                if length:
                    assert_same(l, wl, what + ": length")
                if receivers:
                    assert_same(r, wr, what + ": receivers")


# 2. every position of a batch is the tile alone, and the labels are tile-local
def test_a_batch_of_three(nj, ctx):
    res = 97
    a = tile(res)
    tiles = [a, np.ascontiguousarray(a[::-1]), np.ascontiguousarray(a.T)]
    single = [run_gpu(nj, ctx, t, 0.4, 0.3) for t in tiles]
    for k, (t, got) in enumerate(zip(tiles, single)):
        wb, wl, hops, wr = ref(("batch", k), t, 0.4, 0.3)
        assert got[4] == 1
        assert_same(got[0], wb, "single: basin")
        assert_same(got[1], wl, "single: length")
        assert_same(got[2], wr, "single: receivers")
        assert 0 <= got[0].min() and got[0].max() < res * res
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        b, l, r, passes, conv = run_gpu(nj, ctx, np.stack([tiles[j] for j in order]), 0.4, 0.3)
        assert conv == 1 and passes == max(s[3] for s in single)  # the status words cover the whole batch
        for k, j in enumerate(order):
            assert_same(b[k], single[j][0], "position %d tile %d: basin" % (k, j))
            assert_same(l[k], single[j][1], "position %d tile %d: length" % (k, j))
            assert_same(r[k], single[j][2], "position %d tile %d: receivers" % (k, j))


# 3. the long chain: a budget that needs no measurement, and all or nothing when it runs out
def test_the_serpentine_converges_and_an_exhausted_budget_returns_the_start_state(nj, ctx, capsys):
    h, wb, wl, hops = serpentine()
    height = int(hops.max())
    b, l, r, passes, conv = run_gpu(nj, ctx, h, budget=height + 2)
    with capsys.disabled():
        print("\nserpentine 160^2: %d moves, converged after %d passes" % (height, passes))
    assert conv == 1 and 2 <= passes <= height + 2
    assert_same(b, wb, "serpentine: basin")
    assert_same(l, wl, "serpentine: length")
    own = np.arange(h.size, dtype=np.int32).reshape(h.shape)
    for budget, length in ((1, True), (2, True), (7, True), (7, False)):
        b, l, r, passes, conv = run_gpu(nj, ctx, h, budget=budget, length=length)
        assert (passes, conv) == (budget, 0)
        assert_same(b, own, "serpentine, budget %d: own index everywhere" % budget)
        if length:
            assert_same(l, np.zeros_like(h), "serpentine, budget %d: +0 everywhere" % budget)
        assert_same(r, F.receivers(h)[0], "serpentine, budget %d: the receivers are complete" % budget)


# 4. the schedule is free: every sweep cap gives the same planes; the default comes back afterwards
def test_the_sweep_cap_does_not_matter(nj, ctx):
    lib = nj._native.lib
    s, sb, sl, shops = serpentine()
    f = tile(130)
    fb, fl, fhops, _ = ref(130, f, OFF, 0.3)
    default = lib.nz_debug_watershed_sweeps(0)
    try:
        for cap in (1, 2, 7, 16, 200):
            lib.nz_debug_watershed_sweeps(cap)
            b, l, _, passes, conv = run_gpu(nj, ctx, s, budget=int(shops.max()) + 2, receivers=False)
            assert conv == 1, (cap, passes)
            assert_same(b, sb, "serpentine, cap %d: basin" % cap)
            assert_same(l, sl, "serpentine, cap %d: length" % cap)
            b, l, _, passes, conv = run_gpu(nj, ctx, f, cs=0.3, budget=int(fhops.max()) + 2, receivers=False)
            assert conv == 1, (cap, passes)
            assert_same(b, fb, "fBm 130^2, cap %d: basin" % cap)
            assert_same(l, fl, "fBm 130^2, cap %d: length" % cap)
    finally:
        assert lib.nz_debug_watershed_sweeps(0) == 200
    assert lib.nz_debug_watershed_sweeps(0) == default >= 1


# 5. one work buffer, uncleared, across 160^2 -> 65^2 -> 160^2: no tile byte, receiver byte or verdict of a run survives
def test_a_reused_work_buffer(nj, ctx):
    work = ctx.alloc(nj._native.lib.nz_watershed_work_floats(160, 1, 1))
    for res in (160, 65, 160):
        h = tile(res) if res == 160 else np.ascontiguousarray(tile(97)[:65, 30:95])
        wb, wl, hops, wr = ref(("reuse", res), h)
        b, l, r, _, conv = run_gpu(nj, ctx, h, receivers=False, work=work)  # the receiver bytes live in `work`
        assert conv == 1
        assert_same(b, wb, "reused work %d: basin" % res)
        assert_same(l, wl, "reused work %d: length" % res)
    b, l, r, passes, conv = run_gpu(nj, ctx, tile(160), budget=1, work=work)  # ... nor a verdict
    assert (passes, conv) == (1, 0)
    assert_same(b, np.arange(160 * 160, dtype=np.int32).reshape(160, 160), "reused work, one pass")
    work.Dispose()


# 6. all three float modes give the same bits
def test_float_modes_agree(nj, ctx):
    h = tile(97)
    wb, wl, hops, wr = ref(97, h, 0.4, 0.3)
    want = run_gpu(nj, ctx, h, 0.4, 0.3)
    assert_same(want[0], wb, "strict: basin")
    assert_same(want[1], wl, "strict: length")
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got = run_gpu(nj, mctx, h, 0.4, 0.3)
        finally:
            mctx.close()
        for k, name in enumerate(("basin", "length", "receivers")):
            assert_same(got[k], want[k], "float mode %d: %s" % (mode, name))
        assert got[3:] == want[3:]


# 7. planes carved from one guarded allocation at four alignments and three mixed pairs, the receiver bytes at every byte
# phase in turn: the guards stay silent
@pytest.mark.parametrize("res", [64, 97])
def test_on_slab_carved_planes(nj, ctx, res):
    h, n = tile(res), res * res
    wb, wl, hops, wr = ref(res, h, OFF, 0.3)
    for length in (1, 0):
        nwork = nj._native.lib.nz_watershed_work_floats(res, 1, length)
        for i, (p, q) in enumerate(PAIRS):
            r = p if p == q else (q + 1) % 4
            # the receiver bytes: with the planes where these share a phase -- but once, all planes on 16 bytes, one byte
            # off -- and at odd bytes in the mixed pairs
            odd = i % 4 if p != q else 1 - length if p == 0 else 0
            spec = dict(height=(n, p, h), basin=(n, q, None, np.int32), work=(nwork, r, None),
                        receivers=(n, None, None, np.uint8, (4 * q + odd) % 16))
            if length:
                spec["length"] = (n, r, None)
            with carved(ctx, res, **spec) as (s, t):
                ctx.call("nz_watershed", t.height.ptr, t.basin.ptr, t.length.ptr if length else None, t.receivers.ptr,
                         t.work.ptr, C.byref(desc_of(nj, cs=0.3)), res).Complete()
                assert_same(t.basin.ToArray((res, res)), wb, ("basin", res, p, q))
                if length:
                    assert_same(t.length.ToArray((res, res)), wl, ("length", res, p, q))
                assert_same(t.receivers.ToArray((res, res)), wr, ("receivers", res, p, q))
                assert_same(t.height.ToArray((res, res)), h, ("heights", res, p, q))
                assert ctx.wrap(t.work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
                s.check()
    count = 3
    hh = np.stack([h, h[::-1].copy(), h.T.copy()])
    want = [ref(("slab", res, k), hh[k]) for k in range(count)]
    nwork = nj._native.lib.nz_watershed_work_floats(res, count, 1)
    for p, q in PAIRS:
        with carved(ctx, res, height=(count * n, p, hh), basin=(count * n, q, None, np.int32), length=(count * n, p, None),
                    work=(nwork, (q + 2) % 4, None)) as (s, t):
            ctx.call("nz_watershed_batch", t.height.ptr, t.basin.ptr, t.length.ptr, None, t.work.ptr, C.byref(desc_of(nj)),
                     res, count).Complete()
            assert_same(t.basin.ToArray((count, res, res)), np.stack([w[0] for w in want]), ("batch basin", res, p, q))
            assert_same(t.length.ToArray((count, res, res)), np.stack([w[1] for w in want]), ("batch length", res, p, q))
            s.check()


# 8. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    n = res * res
    sentinel = np.full((res, res), 7.25, f32)
    h, basin, ln, rc = (ctx.from_host(sentinel) for _ in range(4))  # rc: n floats hold the n receiver bytes with room to spare
    work = ctx.alloc(nj._native.lib.nz_watershed_work_floats(res, 1, 1))
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731

    def refused(name, desc, height=h, b=basin, l=ln, r=rc, wk=work, res=res, count=1):
        p = C.byref(desc) if desc is not None else None
        for entry, tail in (("nz_watershed", (res,)), ("nz_watershed_batch", (res, count))):
            if count != 1 and entry == "nz_watershed":
                continue
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, ptr(height), ptr(b), ptr(l), ptr(r), ptr(wk), p, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))

    for v in (math.nan, math.inf, -math.inf, 0.0, -0.0, -1e-6):
        refused("cellSize", desc_of(nj, OFF, v, 10))
    refused("seaLevel", desc_of(nj, math.nan, 1.0, 10))
    refused("maxPasses", desc_of(nj, OFF, 1.0, 0))
    refused("maxPasses", desc_of(nj, OFF, 1.0, -3))
    refused("desc", None)
    good = desc_of(nj, OFF, 1.0, 10)
    refused("height", good, height=None)
    refused("basin", good, b=None)
    refused("work", good, wk=None)
    refused("int32", good, res=46340, count=2)  # 2 x 46340^2 cells: checked before any plane is touched
    inside = ctx.wrap(work.ptr + 4 * (work.Length - n // 2), n)  # a plane that begins inside `work`
    half_h = ctx.wrap(h.ptr + 4 * (n // 2), n)                    # ... inside the heights
    half_b = ctx.wrap(basin.ptr + 4 * (n // 2), n)                # ... inside the labels
    quarter_l = ctx.wrap(ln.ptr + 3 * n, n)                       # the last n bytes of the length
    for plane in (h, half_h, inside, work):
        refused("basin overlaps", good, b=plane)
        refused("length overlaps", good, l=plane)
        refused("receivers overlaps", good, r=plane)
    refused("basin overlaps length", good, l=half_b)
    refused("receivers overlaps basin", good, r=half_b)
    refused("receivers overlaps length", good, r=quarter_l)
    refused("work overlaps height", good, height=inside)
    ctx.synchronize()
    for t in (h, basin, ln, rc):
        assert_same(t.ToArray((res, res)), sentinel, "a plane of a refused call")
    assert (work.ToArray() == f32(7.25)).all()
    # an empty payload is no error and touches nothing
    ctx.call("nz_watershed", h.ptr, basin.ptr, ln.ptr, rc.ptr, work.ptr, C.byref(good), 0).Complete()
    ctx.call("nz_watershed_batch", h.ptr, basin.ptr, ln.ptr, rc.ptr, work.ptr, C.byref(good), res, 0).Complete()
    assert_same(basin.ToArray((res, res)), sentinel, "an empty payload")
    # a sea of -FLT_MAX or +-inf is in range, and the context still works
    hh = tile(97)[:res, :res].copy()
    h.CopyFrom(hh)
    wb, wl, hops, wr = ref("after the refusals", hh)
    for sea in (OFF, -math.inf):
        ctx.call("nz_watershed", h.ptr, basin.ptr, ln.ptr, rc.ptr, work.ptr, C.byref(desc_of(nj, sea, 1.0, 200)), res).Complete()
        assert_same(ctx.wrap(basin.ptr, n, dtype=np.int32).ToArray((res, res)), wb, "after the refusals: basin")
        assert_same(ln.ToArray((res, res)), wl, "after the refusals: length")
        assert_same(ctx.wrap(rc.ptr, n, dtype=np.uint8).ToArray((res, res)), wr, "after the refusals: receivers")
    ctx.call("nz_watershed", h.ptr, basin.ptr, ln.ptr, rc.ptr, work.ptr, C.byref(desc_of(nj, math.inf, 1.0, 200)), res).Complete()
    assert (ctx.wrap(rc.ptr, n, dtype=np.uint8).ToArray() == F.NONE).all()  # everything lies under an infinite sea
    assert not ln.ToArray().any() and ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray().tolist() == [2, 1]
    for t in (h, basin, ln, rc, work):
        t.Dispose()


# 9. the stage behind DepressionFillStage: every label on the border; then a resize, a batch and the options
def test_stage_in_a_pipeline(nj, ctx):
    res = 160
    st = nj.WatershedStage(ctx, recordReceivers=True)
    assert (st.basin, st.length, st.receivers, st.passes, st.converged) == (None, None, None, None, None)
    pipe = nj.BasePipeline([nj.DepressionFillStage(ctx), st], "basins")
    d = nj.GeneratorData("h", ctx.from_host(tile(res)), res, 0, 0)
    done = []
    pipe.Enqueue(d, completeAction=done.append)
    pipe.RunToCompletion()
    assert len(done) == 1
    h = d.data.ToArray((res, res))
    assert F.pits(h) == 0  # filled
    wb, wl, hops, wr = ref("stage 160", h)
    assert st.converged is True and 2 <= st.passes <= min(int(hops.max()) + 2, 64 + res // 4)
    b = st.basin.ToArray((res, res))
    assert b.dtype == np.int32
    assert_same(b, wb, "the stage's labels")
    assert_same(st.length.ToArray((res, res)), wl, "the stage's length")
    assert st.receivers.dtype == np.uint8
    assert_same(st.receivers.ToArray((res, res)), wr, "the stage's receivers")
    z, x = np.divmod(np.unique(b), res)
    assert ((z == 0) | (z == res - 1) | (x == 0) | (x == res - 1)).all()  # every label lies on the border
    # a resize to 97^2: the planes and the work buffer follow the payload
    h97 = tile(97)
    d97 = nj.GeneratorData("h", ctx.from_host(h97), 97, 0, 0)
    st.ReceiveHandledInput(nj.PipelineWorkItem(d97), nj.JobHandle())
    wb, wl, hops, wr = ref(97, h97)
    assert st.converged is True and st.basin.Length == st.length.Length == st.receivers.Length == 97 * 97
    assert_same(st.basin.ToArray((97, 97)), wb, "97^2 behind 160^2: labels")
    assert_same(st.length.ToArray((97, 97)), wl, "97^2 behind 160^2: length")
    assert_same(st.receivers.ToArray((97, 97)), wr, "97^2 behind 160^2: receivers")
    assert_same(d97.data.ToArray((97, 97)), h97, "the heights pass through")
    # a batch, a sea and a cell size, labels only
    hh = np.stack([h97, np.ascontiguousarray(h97.T)])
    st2 = nj.WatershedStage(ctx, seaLevel=0.4, cellSize=0.3, maxPasses=GENEROUS, length=False)
    bt = nj.GeneratorDataBatch("h", ctx.from_host(hh), 97, None, 2)
    st2.ReceiveHandledInput(nj.PipelineWorkItem(bt), nj.JobHandle())
    assert st2.converged is True and st2.length is None and st2.receivers is None
    got = st2.basin.ToArray((2, 97, 97))
    for k in range(2):
        assert_same(got[k], ref(("stage batch", k), hh[k], 0.4, 0.3)[0], "batch tile %d" % k)
    # a budget that runs out: the start state, converged False
    st3 = nj.WatershedStage(ctx, maxPasses=2)
    st3.ReceiveHandledInput(nj.PipelineWorkItem(d97), nj.JobHandle())
    assert st3.converged is False and st3.passes == 2
    assert_same(st3.basin.ToArray((97, 97)), np.arange(97 * 97, dtype=np.int32).reshape(97, 97), "budget of 2")
    assert not st3.length.ToArray().any()
    for s in (st, st2, st3):
        s.OnDestroy()
    assert st.basin is None and st.passes is None


# 10. 1024^2, filled, the hosts' default budget: the many-tile skip logic.  No walk is needed: the fixed point is unique, so
# "one step of the model returns the planes" is a complete check
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
    st = nj.WatershedStage(ctx, recordReceivers=True)  # every default
    g = nj.GeneratorData("h", d, res, 0, 0)
    st.ReceiveHandledInput(nj.PipelineWorkItem(g), nj.JobHandle())
    passes, conv = st.passes, st.converged
    with capsys.disabled():
        print("\n1024^2 filled fBm: converged %s after %d passes (default budget %d)" % (conv, passes, 64 + res // 4))
    assert conv is True
    b, l, r = st.basin.ToArray((res, res)), st.length.ToArray((res, res)), st.receivers.ToArray((res, res))
    assert_same(d.ToArray((res, res)), h, "1024: the heights")
    st.OnDestroy()
    d.Dispose()
    wr = F.receivers(h)[0]
    assert_same(r, wr, "1024: receivers")
    has, q, step = wr != F.NONE, W.targets(wr), W.steps_of(1.0)[wr]
    own = np.arange(n, dtype=np.int32).reshape(res, res)
    assert_same(b, np.where(has, b.reshape(-1)[q], own).astype(np.int32), "1024: basin == basin[q], own index without a receiver")
    assert_same(l, np.where(has, (l.reshape(-1)[q] + step).astype(f32), f32(0.0)).astype(f32), "1024: length == length[q] + step")
    z, x = np.divmod(np.unique(b), res)
    assert ((z == 0) | (z == res - 1) | (x == 0) | (x == res - 1)).all()  # filled: every label on the border
