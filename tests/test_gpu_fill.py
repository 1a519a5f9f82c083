"""Depression filling on the GPU (nz_fill_depressions*, DepressionFillStage) against the heap priority-flood of
tests/fill_ref.py, bit for bit throughout: sizes on and across the 64-column / 16-row tile edges, assorted tiles with a
tile-spanning bowl among them, the in-place / _rw / _batch forms and the three float modes, the depth plane, the pass
budget (all or nothing), tile skipping and the schedule hook, planes carved from a guarded slab, the stage in front of the
fluvial stage and on payloads of equal length and different tile counts, the compiled C++ host, bad arguments, and a
4096^2 plane checked on a band around a seam of the launch grid."""
import ctypes as C
import math

import numpy as np
import pytest

import fill_ref as L
import fluvial_ref as F
from test_gpu_slab import PAIRS, carved, memo
from test_hydraulic_ref import relief

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
EPS = (0.0, 1e-4, 1e-2)
GENEROUS = 400  # passes: the bowl, the longest front here, needs a few dozen


def ramp(res):
    return (np.arange(res, dtype=f32)[None, :] * f32(0.01) + np.arange(res, dtype=f32)[:, None] * f32(0.003)).astype(f32)


def bowl(res=160):
    """A cone pit over the whole tile behind a high border; the one low border cell is the corner (0, 0), so the only way
    out is the cone's highest inner cell, (1, 1): one front from that corner across every tile."""
    z, x = np.mgrid[0:res, 0:res].astype(f32)
    c = f32((res - 1) / 2)
    h = (np.sqrt((x - c) ** 2 + (z - c) ** 2) * f32(0.01)).astype(f32)
    h[0, :] = h[-1, :] = h[:, 0] = h[:, -1] = f32(100.0)
    h[0, 0] = f32(-1.0)
    return h


def make(name):
    rng = np.random.default_rng(7)
    kind, res = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
    if kind == "fbm":
        return relief(res, 500 if res == 160 else 300)
    if kind == "noisy":
        return (relief(res, res) + rng.standard_normal((res, res)).astype(f32) * f32(0.01)).astype(f32)
    if kind == "rand":
        return rng.random((res, res), dtype=f32)
    if kind == "const":
        return np.full((res, res), f32(0.375))
    if kind == "ramp":
        return ramp(res)
    assert kind == "bowl"
    return bowl(res)


def tile(name):
    return memo(("fill tile", name), lambda: np.ascontiguousarray(make(name), f32))


def flood(name, eps, sea=OFF):
    return memo(("fill flood", name, eps, sea), lambda: L.flood(tile(name), eps, sea))


def desc_of(nj, eps, sea, budget, depth=None):
    return nj._native.FillDesc(eps, sea, budget, depth.ptr if depth is not None else None)


def run_gpu(nj, ctx, h, eps=1e-4, sea=OFF, budget=GENEROUS, form="inplace", depth=False):
    """One run on the host plane h (res x res, or count x res x res) -> (result, depth or None, passes, converged)."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    src = ctx.from_host(h)
    work = ctx.alloc(nj._native.lib.nz_fill_depressions_work_floats(res, count))
    dp = ctx.from_host(np.full(h.shape, np.nan, f32)) if depth else None
    desc = desc_of(nj, eps, sea, budget, dp)
    other = None
    if form == "rw":
        other = ctx.from_host(np.full(h.shape, 7.25, f32))
        t = nj._native.RWTile(src.ptr, other.ptr, res, count)
        ctx.call("nz_fill_depressions_rw", C.byref(t), work.ptr, C.byref(desc)).Complete()
        assert t.read == src.ptr and t.write == other.ptr  # the result lands in tile->read
        assert (other.ToArray() == f32(7.25)).all()
    elif form == "batch":
        ctx.call("nz_fill_depressions_batch", src.ptr, work.ptr, C.byref(desc), res, count).Complete()
    else:
        assert count == 1
        ctx.call("nz_fill_depressions", src.ptr, work.ptr, C.byref(desc), res).Complete()
    got = src.ToArray(h.shape)
    status = ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()
    d = dp.ToArray(h.shape) if depth else None
    for t in (src, work, other, dp):
        if t is not None:
            t.Dispose()
    return got, d, int(status[0]), int(status[1])


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != np.ascontiguousarray(want, f32).view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], np.asarray(want)[bad][0])


# 1. sizes on and across the tile edges, assorted tiles, three epsilons
@pytest.mark.parametrize("name", ["rand1", "rand2", "rand3", "fbm17", "fbm63", "fbm64", "fbm65", "fbm97", "fbm130", "fbm160",
                                  "noisy97", "rand130", "const65", "ramp17", "ramp97", "bowl160"])
def test_matches_the_priority_flood(nj, ctx, name):
    h = tile(name)
    for eps in EPS:
        got, _, passes, converged = run_gpu(nj, ctx, h, eps)
        assert converged == 1 and 1 <= passes < GENEROUS, (name, eps, passes)
        assert_bits(got, flood(name, eps), "%s eps %g" % (name, eps))
        if name.startswith("ramp"):  # no pits: the input comes back bit for bit, after a front or two across the tile
            assert_bits(got, h, name)
            assert passes <= 4 + h.shape[0] // 16, (name, passes)
        if name == "const65" and eps > 0:  # one flat: a cone of epsilon steps towards the middle
            assert got[32, 32] == got.max() > h[32, 32]


# 2. in-place, _rw and _batch agree; every tile of a batch is the tile alone; all float modes give the same bits
def test_forms_batch_and_float_modes_agree(nj, ctx):
    a, b, c = relief(48), (relief(48, 170) * f32(3.0)).astype(f32), tile("rand130")[:48, :48].copy()
    batch = np.stack([a, b, c])
    for eps in (0.0, 1e-4):
        single = [run_gpu(nj, ctx, t, eps, depth=True) for t in (a, b, c)]
        for t, (want, dwant, _, conv) in zip((a, b, c), single):
            assert conv == 1
            assert_bits(want, L.flood(t, eps), "single eps %g" % eps)
            got, d, _, conv = run_gpu(nj, ctx, t, eps, form="rw", depth=True)
            assert conv == 1
            assert_bits(got, want, "rw")
            assert_bits(d, dwant, "rw depth")
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):  # every tile at every batch position
            for form in ("batch", "rw"):
                got, d, passes, conv = run_gpu(nj, ctx, batch[list(order)], eps, form=form, depth=True)
                assert conv == 1 and passes == max(s[2] for s in single)  # the status words cover the whole batch
                for k, j in enumerate(order):
                    assert_bits(got[k], single[j][0], "%s position %d tile %d" % (form, k, j))
                    assert_bits(d[k], single[j][1], "%s depth position %d tile %d" % (form, k, j))
    want = run_gpu(nj, ctx, a, 1e-4, depth=True)
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got = run_gpu(nj, mctx, a, 1e-4, depth=True)
        finally:
            mctx.close()
        assert_bits(got[0], want[0], "float mode %d" % mode)
        assert_bits(got[1], want[1], "float mode %d depth" % mode)
        assert got[2:] == want[2:]


# 3. the depth plane is W - h of the model, zero exactly where nothing was filled; a sea at the median stays
@pytest.mark.parametrize("name", ["fbm97", "rand130", "bowl160"])
def test_depth_and_sea(nj, ctx, name):
    h = tile(name)
    for eps in (0.0, 1e-4):
        W = flood(name, eps)
        got, d, _, conv = run_gpu(nj, ctx, h, eps, depth=True)
        assert conv == 1
        assert_bits(got, W, name)
        assert_bits(d, W - h, name + " depth")
        assert ((d == 0) == (got.view(np.uint32) == h.view(np.uint32))).all() and (d >= 0).all() and (d > 0).any()
    sea = float(np.median(h))
    W = flood(name, 1e-4, sea)
    got, d, _, conv = run_gpu(nj, ctx, h, 1e-4, sea, depth=True)
    low = h <= f32(sea)
    assert conv == 1 and low.any() and not low.all()
    assert_bits(got, W, name + " with a sea")
    assert_bits(got[low], h[low], name + ": the sea cells")
    assert_bits(d, W - h, name + " depth with a sea")
    assert F.pits(got, sea) == 0


# 4. the budget: all or nothing
def test_an_exhausted_budget_leaves_the_heights(nj, ctx):
    h = tile("bowl160")
    for budget in (1, 2, 5):
        for form in ("inplace", "rw", "batch"):
            hh = h[None] if form == "batch" else h
            got, d, passes, conv = run_gpu(nj, ctx, hh, 1e-4, budget=budget, form=form, depth=True)
            assert conv == 0 and passes == budget, (budget, form, passes, conv)
            assert_bits(got, hh, "budget %d %s" % (budget, form))
            assert np.isfinite(got).all() and (d == 0).all()
    first = run_gpu(nj, ctx, h, 1e-4, depth=True)
    assert first[3] == 1 and first[2] < GENEROUS
    # a budget of exactly the passes used converges, one less does not; twice the same payload: same bits, same passes
    assert run_gpu(nj, ctx, h, 1e-4, budget=first[2])[2:] == (first[2], 1)
    assert run_gpu(nj, ctx, h, 1e-4, budget=first[2] - 1)[2:] == (first[2] - 1, 0)
    again = run_gpu(nj, ctx, h, 1e-4, depth=True)
    assert_bits(again[0], first[0], "second run")
    assert_bits(again[1], first[1], "second run depth")
    assert again[2:] == first[2:]
    # the same work planes used twice, uncleared between the runs
    src, work = ctx.from_host(h), ctx.alloc(nj._native.lib.nz_fill_depressions_work_floats(160, 1))
    for k in range(2):
        src.CopyFrom(h)
        ctx.call("nz_fill_depressions", src.ptr, work.ptr, C.byref(desc_of(nj, 1e-4, OFF, GENEROUS)), 160).Complete()
        assert_bits(src.ToArray((160, 160)), first[0], "reused work, run %d" % k)
        assert tuple(ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()) == first[2:]
    src.Dispose()
    work.Dispose()


# 5. the on-chip sweeps do work: fewer passes than the model's whole-grid Jacobi iteration; and the schedule is free
def test_sweeps_save_passes_and_the_schedule_does_not_matter(nj, ctx):
    h = tile("bowl160")
    want = flood("bowl160", 1e-4)
    jacobi_passes = memo(("fill jacobi", "bowl160"), lambda: L.jacobi(h, 1e-4)[1])
    got, _, passes, conv = run_gpu(nj, ctx, h)
    assert conv == 1 and passes < jacobi_passes, (passes, jacobi_passes)
    assert_bits(got, want, "bowl")
    lib = nj._native.lib
    try:
        for sweeps, name in ((1, "bowl160"), (3, "bowl160"), (1, "rand130"), (200, "noisy97")):
            lib.nz_debug_fill_sweeps(sweeps)
            g, _, p, conv = run_gpu(nj, ctx, tile(name), budget=GENEROUS if sweeps > 1 else 4 * GENEROUS)
            assert conv == 1, (sweeps, name, p)
            assert_bits(g, flood(name, 1e-4), "%s with %d sweeps" % (name, sweeps))
            if name == "bowl160":
                assert p > passes  # fewer sweeps, more passes
    finally:
        lib.nz_debug_fill_sweeps(0)


# 6. planes carved from one guarded allocation at four alignments and three mixed pairs: the guards stay silent
@pytest.mark.parametrize("res", [64, 97])
def test_on_slab_carved_planes(nj, ctx, res):
    name = "fbm%d" % res
    h, n = tile(name), res * res
    W = flood(name, 1e-4)
    nwork = nj._native.lib.nz_fill_depressions_work_floats(res, 1)
    for p, q in PAIRS:
        r = p if p == q else (q + 1) % 4
        with carved(ctx, res, src=(n, p, h), work=(nwork, q, None), depth=(n, r, None)) as (s, t):
            ctx.call("nz_fill_depressions", t.src.ptr, t.work.ptr, C.byref(desc_of(nj, 1e-4, OFF, 60, t.depth)), res).Complete()
            assert_bits(t.src.ToArray((res, res)), W, ("in place", res, p, q))
            assert_bits(t.depth.ToArray((res, res)), W - h, ("in place depth", res, p, q))
            assert ctx.wrap(t.work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
            s.check()
        with carved(ctx, res, src=(n, p, h), other=(n, q, None), work=(nwork, r, None), depth=(n, q, None)) as (s, t):
            keep = t.other.ToArray()
            rw = nj._native.RWTile(t.src.ptr, t.other.ptr, res, 1)
            ctx.call("nz_fill_depressions_rw", C.byref(rw), t.work.ptr, C.byref(desc_of(nj, 1e-4, OFF, 60, t.depth))).Complete()
            assert rw.read == t.src.ptr
            assert_bits(t.src.ToArray((res, res)), W, ("rw", res, p, q))
            assert_bits(t.depth.ToArray((res, res)), W - h, ("rw depth", res, p, q))
            assert np.array_equal(t.other.ToArray().view(np.uint32), keep.view(np.uint32))
            s.check()
    count = 3
    hh = memo(("fill batch in", res), lambda: np.stack([h, h[::-1].copy(), h.T.copy()]))
    want = memo(("fill batch", res), lambda: np.stack([L.flood(hh[k], 1e-4) for k in range(count)]))
    nwork = nj._native.lib.nz_fill_depressions_work_floats(res, count)
    for p, q in PAIRS:
        with carved(ctx, res, src=(count * n, p, hh), work=(nwork, q, None)) as (s, t):
            ctx.call("nz_fill_depressions_batch", t.src.ptr, t.work.ptr, C.byref(desc_of(nj, 1e-4, OFF, 60)), res, count).Complete()
            assert_bits(t.src.ToArray((count, res, res)), want, ("batch", res, p, q))
            s.check()


# 7. in front of the fluvial stage: no pits, and all of the rain reaches the outlets
def test_stage_in_a_pipeline(nj, ctx):
    res = 128
    h = relief(res)
    outlets = F.outlets(h)

    def run(stages):
        pipe = nj.BasePipeline(stages, "fill")
        d = nj.GeneratorData("h", ctx.from_host(h), res, 0, 0)
        done = []
        pipe.Enqueue(d, completeAction=done.append)
        pipe.RunToCompletion()
        assert len(done) == 1
        out = d.data.ToArray((res, res)), stages[-1].drainage.ToArray((res, res))
        return out

    fill = nj.DepressionFillStage(ctx, recordDepth=True)
    assert (fill.passes, fill.converged, fill.depth) == (None, None, None)
    still = dict(erodibility=0.0, uplift=0.0)
    got, _ = run([fill, nj.FluvialErosionStage(ctx, iterations=1, **still)])
    W = L.flood(h, 1e-4)
    assert F.pits(h) == 52 and F.pits(got) == 0
    assert_bits(got, W, "the stage's heights")
    assert_bits(fill.depth.ToArray((res, res)), W - h, "the stage's depth")
    assert fill.converged is True and 1 <= fill.passes < 64 + res // 4
    _, drained = run([nj.DepressionFillStage(ctx), nj.FluvialErosionStage(ctx, iterations=400, **still)])
    assert float(drained[outlets].astype(np.float64).sum()) == res * res
    _, cut = run([nj.FluvialErosionStage(ctx, iterations=400, **still)])
    assert float(cut[outlets].astype(np.float64).sum()) < res * res
    # a READ / WRITE pair, a batch payload and a budget that runs out
    for payload in ("rw", "batch"):
        st = nj.DepressionFillStage(ctx, epsilon=0.0, maxPasses=60)
        if payload == "rw":
            d = nj.GeneratorData("h", ctx.from_host(h), res, 0, 0, write=ctx.alloc(res * res))
        else:
            d = nj.GeneratorDataBatch("h", ctx.from_host(np.stack([h, h])), res, None, 2)
        st.ReceiveHandledInput(nj.PipelineWorkItem(d), nj.JobHandle())
        assert st.converged is True and st.depth is None
        assert_bits(d.data.ToArray((-1, res, res))[-1], L.flood(h, 0.0), payload)
        st.OnDestroy()
    st = nj.DepressionFillStage(ctx, maxPasses=2, recordDepth=True)
    d = nj.GeneratorData("h", ctx.from_host(h), res, 0, 0)
    st.ReceiveHandledInput(nj.PipelineWorkItem(d), nj.JobHandle())
    assert st.converged is False and st.passes == 2
    assert_bits(d.data.ToArray((res, res)), h, "budget of 2")
    assert not st.depth.ToArray().any()
    st.OnDestroy()
    assert st.depth is None and st.passes is None


# 7b. one stage instance on payloads of EQUAL length that need work planes of different sizes: 1 x 128^2 is 16 tiles of
# 64 x 16 cells, 64 x 16^2 is 64 of them, 16 x 32^2 is 32 -- the per-tile bytes differ, the cell count does not
def test_a_stage_resizes_its_work_planes_with_the_tile_count(nj, ctx):
    need = nj._native.lib.nz_fill_depressions_work_floats
    shapes = [(128, 1), (16, 64), (32, 16), (128, 1)]
    assert len({r * r * c for r, c in shapes}) == 1 and need(16, 64) > need(32, 16) > need(128, 1)
    big = relief(128)
    for order in (shapes, shapes[::-1][1:]):
        st = nj.DepressionFillStage(ctx, recordDepth=True)
        for res, count in order:
            hh = np.ascontiguousarray(big.reshape(128 // res, res, 128 // res, res).transpose(0, 2, 1, 3).reshape(count, res, res))
            if count == 1:
                d = nj.GeneratorData("h", ctx.from_host(hh), res, 0, 0)
            else:
                d = nj.GeneratorDataBatch("h", ctx.from_host(hh), res, None, count)
            st.ReceiveHandledInput(nj.PipelineWorkItem(d), nj.JobHandle())
            assert st.work.Length == need(res, count), (res, count, st.work.Length)
            assert st.converged is True
            got, depth = d.data.ToArray(hh.shape), st.depth.ToArray(hh.shape)
            for k in range(count):
                W = memo(("fill cut", res, k), lambda: L.flood(hh[k], 1e-4))
                assert_bits(got[k], W, "%d x %d^2, tile %d" % (count, res, k))
                assert_bits(depth[k], W - hh[k], "%d x %d^2, tile %d: depth" % (count, res, k))
            d.data.Dispose()
        st.OnDestroy()


# 7c. the C++ host's stage from a compiled program: heights, depth, the status words, and the same stage instance on a batch
# of equal length and more tiles
def test_cpp_host_runs_the_stage(oracle, tmp_path):
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "noize_job_amd", "host", "host_demo")
    assert os.path.exists(exe), "host_demo not built (run __graft_entry__.build())"
    out = str(tmp_path / "fill.f32")
    res, small, many = 128, 16, 64
    text = subprocess.run([exe, str(res), out, "fill"], check=True, timeout=120, capture_output=True, text=True).stdout
    status = [tuple(int(v) for v in line.split()) for line in text.strip().splitlines()]
    assert len(status) == 2 and all(c == 1 and 1 <= p < 64 + r // 4 for (p, c), r in zip(status, (res, small))), status
    got = np.fromfile(out, dtype=f32)
    n = res * res
    h = oracle.fractal(oracle.SIMPLEX, res, res, 0.4, 1.0, 2.0, 0.0, 6, 37, 11, 300)
    W = L.flood(h, 1e-4)
    assert_bits(got[:n].reshape(res, res), W, "C++ host: heights")
    assert_bits(got[n:2 * n].reshape(res, res), W - h, "C++ host: depth")
    tiles = got[2 * n:].reshape(many, small, small)
    for k in range(many):
        hk = oracle.fractal(oracle.SIMPLEX, small, small, 0.4, 1.0, 2.0, 0.0, 6, k * small, 7 * k, 300)
        assert_bits(tiles[k], L.flood(hk, 1e-4), "C++ host: batch tile %d" % k)


# 8. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    n = res * res
    sentinel = np.full((res, res), 7.25, f32)
    d, other, apart = ctx.from_host(sentinel), ctx.from_host(sentinel), ctx.from_host(sentinel)
    work = ctx.alloc(nj._native.lib.nz_fill_depressions_work_floats(res, 1))
    work.CopyFrom(np.full(work.Length, 7.25, f32))

    def refused(name, desc, entries=("nz_fill_depressions", "nz_fill_depressions_batch", "nz_fill_depressions_rw")):
        t = nj._native.RWTile(d.ptr, other.ptr, res, 1)
        p = C.byref(desc) if desc is not None else None
        calls = {"nz_fill_depressions": ((d.ptr, work.ptr), (res,)), "nz_fill_depressions_batch": ((d.ptr, work.ptr), (res, 1)),
                 "nz_fill_depressions_rw": ((C.byref(t), work.ptr), ())}
        for entry in entries:
            head, tail = calls[entry]
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, *head, p, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))
        assert t.read == d.ptr

    for v in (math.nan, math.inf, -math.inf):
        refused("epsilon", desc_of(nj, v, OFF, 10))
        refused("seaLevel", desc_of(nj, 1e-4, v, 10))
    refused("epsilon", desc_of(nj, -1e-6, OFF, 10))
    refused("maxPasses", desc_of(nj, 1e-4, OFF, 0))
    refused("maxPasses", desc_of(nj, 1e-4, OFF, -3))
    refused("desc", None)
    inside = ctx.wrap(work.ptr + 4 * (work.Length - n // 2), n)  # a plane that begins inside `work`
    half = ctx.wrap(d.ptr + 4 * (n // 2), n)                      # a plane that begins inside `src`
    for plane in (d, inside, half, work):
        refused("depth", desc_of(nj, 1e-4, OFF, 10, plane))
    refused("depth", desc_of(nj, 1e-4, OFF, 10, other), entries=("nz_fill_depressions_rw",))  # the pair's write plane
    ctx.synchronize()
    for t in (d, other, apart):
        assert_bits(t.ToArray((res, res)), sentinel, "a plane of a refused call")
    assert (work.ToArray() == f32(7.25)).all()
    # a sea level of -FLT_MAX and an epsilon of -0 are in range, `other` is a fine depth plane for the in-place form, and
    # the context still works
    h = relief(res)
    d.CopyFrom(h)
    ctx.call("nz_fill_depressions", d.ptr, work.ptr, C.byref(desc_of(nj, -0.0, OFF, 40, other)), res).Complete()
    W = L.flood(h, 0.0)
    assert_bits(d.ToArray((res, res)), W, "after the refusals")
    assert_bits(other.ToArray((res, res)), W - h, "after the refusals: depth")
    for t in (d, other, apart, work):
        t.Dispose()


# 9. 4096^2 with the default budget.  The fill is not local, so no band of the plane can be had from a small model run --
# unless the band is cut off: the two rows either side of it are pushed below a sea level, which makes them outlets, and the
# rows between them are then the model on the band alone.  The band's inner rows, 2032 .. 2063, are the two tile rows either
# side of the launch grid's seam at row 2048; across it run all 64 column seams.
def test_4096_band_matches(nj, ctx):
    res, eps, sea = 4096, 1e-4, -50.0
    d = ctx.alloc(res * res)
    ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 1700).Complete()
    h = d.ToArray((res, res))
    d.Dispose()
    z0, z1 = 2031, 2064
    assert h.min() > sea
    h[z0] = h[z1] = f32(-100.0)
    budget = 64 + res // 4  # the hosts' default
    got, depth, passes, conv = run_gpu(nj, ctx, h, eps, sea, budget=budget, depth=True)
    assert conv == 1 and passes < budget, passes
    assert np.isfinite(got).all() and (got >= h).all() and got.min() >= h.min()
    out = F.outlets(h, sea)
    assert_bits(got[out], h[out], "4096: the outlets")
    assert_bits(depth, got - h, "4096: depth")
    assert (depth > 0).any()
    # a fixed point of the operator on the first 1024 rows (the last row of the cut is no border of the plane: left out)
    cut = slice(0, 1025)
    assert_bits(L.step(got[cut], h[cut], out[cut], f32(eps))[:-1], got[cut][:-1], "4096: a fixed point")
    assert_bits(got[z0:z1 + 1], L.flood(h[z0:z1 + 1], eps, sea), "4096 band")
