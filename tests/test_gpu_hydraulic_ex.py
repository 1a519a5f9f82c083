"""The extended grid hydraulic erosion on the GPU (nz_hydraulic_erosion_ex*, HydraulicErosionStage with border / rainMap /
hardness / recordMasks) against tests/hydraulic_ex_ref.py: heights, water, wear and deposits equal the driver bit for bit
for every option alone and all together, on sizes with partial tiles; the three forms and the three float modes agree;
with everything off the entry is the plain one; a 4096^2 run; the stage in a pipeline; refusals write nothing."""
import ctypes as C

import numpy as np
import pytest

import hydraulic_ex_ref as X
from test_gpu_hydraulic import assert_bits, run_gpu, work_for
from test_hydraulic_ref import NAMES, PARAMS, relief

pytestmark = pytest.mark.gpu
f32 = np.float32


def maps_for(shape, seed):
    """A rain map in [0, 2] and a hardness map in [0, 1] with exact zeros and ones in it."""
    rng = np.random.default_rng(seed)
    rain = (rng.random(shape, dtype=f32) * f32(2.0)).astype(f32)
    hard = np.clip(rng.random(shape, dtype=f32) * f32(1.5) - f32(0.25), 0.0, 1.0).astype(f32)
    return rain, hard


def option_sets(shape, seed=11):
    rain, hard = maps_for(shape, seed)
    return {"open": dict(border=X.OPEN), "rain": dict(rainMap=rain), "hardness": dict(hardness=hard), "masks": dict(masks=True),
            "all": dict(border=X.OPEN, rainMap=rain, hardness=hard, masks=True)}


def run_ex(nj, ctx, h, its, prm, border=X.CLOSED, rainMap=None, hardness=None, masks=False, form="inplace"):
    """One run of an _ex entry on the host plane h (res x res, or count x res x res); -> (result, water, wear, deposits),
    the masks None when not recorded.  The mask planes start as garbage: the entry owes them no clearing by the caller."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    src = ctx.from_host(h)
    work = work_for(nj, ctx, res, count)
    held = [src, work]
    dev = {}
    for name, m in (("rainMap", rainMap), ("hardness", hardness)):
        dev[name] = ctx.from_host(np.ascontiguousarray(m, f32)) if m is not None else None
    for name in ("wear", "deposits"):
        dev[name] = ctx.from_host(np.full(h.shape, 123.5, f32)) if masks else None
    held += [t for t in dev.values() if t is not None]
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731
    desc = nj._native.HydraulicDesc(its, *prm, border, ptr(dev["rainMap"]), ptr(dev["hardness"]), ptr(dev["wear"]),
                                    ptr(dev["deposits"]))
    if form == "rw":
        other = ctx.alloc(h.size)
        held.append(other)
        t = nj._native.RWTile(src.ptr, other.ptr, res, count)
        ctx.call("nz_hydraulic_erosion_ex_rw", C.byref(t), work.ptr, C.byref(desc))
        assert t.read in (src.ptr, other.ptr) and t.write in (src.ptr, other.ptr) and t.read != t.write
        out = src if t.read == src.ptr else other
    elif form == "batch":
        ctx.call("nz_hydraulic_erosion_ex_batch", src.ptr, work.ptr, C.byref(desc), res, count)
        out = src
    else:
        assert count == 1
        ctx.call("nz_hydraulic_erosion_ex", src.ptr, work.ptr, C.byref(desc), res)
        out = src
    got = out.ToArray(h.shape)
    water = work.ToArray()[:h.size].reshape(h.shape)
    wear = dev["wear"].ToArray(h.shape) if masks else None
    deposits = dev["deposits"].ToArray(h.shape) if masks else None
    for t in held:
        t.Dispose()
    return got, water, wear, deposits


def assert_run(got, want, masks, what):
    for k, name in enumerate(("result", "water", "wear", "deposits")):
        if k < 2 or masks:
            assert_bits(got[k], want[k], "%s: %s" % (what, name))


def ref_run(h, its, prm, border=X.CLOSED, rainMap=None, hardness=None, masks=False):
    return X.run(h, its, border=border, rainMap=rainMap, hardness=hardness, **dict(zip(NAMES, prm)))


# 1. every option alone and all four together equal the driver bit for bit; 64: one tile column, 97 and 160: partial tiles
# in both directions; odd and even counts (the in-place form copies once on odd counts)
@pytest.mark.parametrize("option", ["open", "rain", "hardness", "masks", "all"])
@pytest.mark.parametrize("res", [64, 97, 160])
def test_matches_the_driver(nj, ctx, res, option):
    x = np.arange(res, dtype=f32)
    h = (relief(res, 500 if res == 160 else 300) + (x[None, :] * f32(0.004) + x[:, None] * f32(0.001))).astype(f32)
    opts = option_sets(h.shape)[option]
    for k, prm in enumerate(PARAMS[:2] if res == 160 else PARAMS):
        for its in ((1, 2, 7, 40) if res != 160 else (3, 40)):
            got = run_ex(nj, ctx, h, its, prm, **opts)
            want = ref_run(h, its, prm, **opts)
            assert_run(got, want, opts.get("masks"), "%s res %d params %d its %d" % (option, res, k, its))


def test_zero_iterations_clear_the_masks(nj, ctx):
    h = relief(64)
    for form in ("inplace", "rw", "batch"):
        got, water, wear, deposits = run_ex(nj, ctx, h[None] if form == "batch" else h, 0, PARAMS[0], masks=True, form=form)
        assert_bits(got.reshape(h.shape), h, form)
        assert (water == f32(PARAMS[0][0])).all() and not wear.any() and not deposits.any(), form
        assert not np.signbit(wear).any() and not np.signbit(deposits).any()


# 2. _ex, _ex_rw and _ex_batch agree, a batch with different maps per tile is every tile alone, the float modes agree
def test_forms_batch_and_float_modes_agree(nj, ctx):
    a, b, c = relief(96), (relief(96, 170) * f32(3.0)).astype(f32), np.full((96, 96), f32(1.5))
    batch = np.stack([a, b, c])
    rain, hard = maps_for(batch.shape, 23)
    assert not np.array_equal(rain[0], rain[1]) and not np.array_equal(hard[1], hard[2])
    for prm in PARAMS[:2]:
        for its in (1, 4, 9):
            single = [run_ex(nj, ctx, t, its, prm, X.OPEN, rain[k], hard[k], True) for k, t in enumerate((a, b, c))]
            for k, t in enumerate((a, b, c)):
                assert_run(run_ex(nj, ctx, t, its, prm, X.OPEN, rain[k], hard[k], True, form="rw"), single[k], True,
                           "rw tile %d its %d" % (k, its))
            for form in ("batch", "rw"):
                got = run_ex(nj, ctx, batch, its, prm, X.OPEN, rain, hard, True, form=form)
                for k in range(3):
                    assert_run([g[k] for g in got], single[k], True, "%s tile %d its %d" % (form, k, its))
    want = run_ex(nj, ctx, a, 9, PARAMS[1], X.OPEN, rain[0], hard[0], True)
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got = run_ex(nj, mctx, a, 9, PARAMS[1], X.OPEN, rain[0], hard[0], True)
        finally:
            mctx.close()
        assert_run(got, want, True, "float mode %d" % mode)


# 3. with everything off the _ex entry is the plain entry: device against device at 1024^2, 50 iterations
def test_everything_off_is_the_plain_entry(nj, ctx, oracle):
    res, its = 1024, 50
    h = oracle.fractal(oracle.SIMPLEX, res, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 1700)
    for form in ("inplace", "rw"):
        want, wwant = run_gpu(nj, ctx, h, its, PARAMS[0], form)
        got, water, _, _ = run_ex(nj, ctx, h, its, PARAMS[0], form=form)
        assert not np.array_equal(got, h)
        assert_bits(got, want, "result " + form)
        assert_bits(water, wwant, "water " + form)
    ones, zeros = np.ones_like(h), np.zeros_like(h)
    got, water, _, _ = run_ex(nj, ctx, h, its, PARAMS[0], rainMap=ones, hardness=zeros)
    assert_bits(got, want, "neutral maps")
    assert_bits(water, wwant, "neutral maps: water")


# 4. 4096^2, open border, both maps and the masks, 20 iterations, against the driver
def test_4096_everything_on(nj, ctx, oracle):
    res, its = 4096, 20
    h = oracle.fractal(oracle.SIMPLEX, res, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 1700)
    rain, hard = maps_for(h.shape, 5)
    prm = (1e-3, 5e-4, 0.01, 4.0, 0.5, 0.3, 0.01)
    got = run_ex(nj, ctx, h, its, prm, X.OPEN, rain, hard, True)
    assert all(np.isfinite(g).all() for g in got) and got[2].any() and got[3].any()
    want = ref_run(h, its, prm, X.OPEN, rain, hard)
    assert_run(got, want, True, "4096")


# 5. in a BasePipeline after a NoiseStage and a KernelFilterStage; the masks are read through the stage
def test_stage_in_a_pipeline(nj, ctx, oracle):
    res, xp, zp = 160, 4096, -2048
    noise = oracle.fractal(oracle.SIMPLEX, res, res, 0.4, 1.0, 2.0, 0.0, 13, xp, zp, 1700)
    filtered = oracle.kernel_filter(noise, oracle.GAUSS5_S1, 4)
    rain, hard = maps_for(filtered.shape, 31)
    want = X.run(filtered, 30, capacity=2.0, border=X.OPEN, rainMap=rain, hardness=hard)
    drain, dhard = ctx.from_host(rain), ctx.from_host(hard)
    for rw in (False, True):
        hyd = nj.HydraulicErosionStage(ctx, iterations=30, capacity=2.0, border=nj.HydraulicBorder.Open, rainMap=drain,
                                       hardness=dhard, recordMasks=True)
        stages = [nj.NoiseStage(ctx, nj.FractalNoise.Simplex, 0.4, 1.0, 13, 2.0, 0.0, 1700),
                  nj.KernelFilterStage(ctx, nj.KernelFilterType.Gauss5_S1, 4), hyd]
        pipe = nj.BasePipeline(stages, "hydraulic-ex")
        d = nj.GeneratorData("h", ctx.alloc(res * res), res, xp, zp, write=ctx.alloc(res * res) if rw else None)
        done = []
        pipe.Enqueue(d, completeAction=done.append)
        pipe.RunToCompletion()
        assert len(done) == 1
        got = (d.data.ToArray((res, res)), hyd.water.ToArray((res, res)), hyd.wear.ToArray((res, res)),
               hyd.deposits.ToArray((res, res)))
        assert_run(got, want, True, "pipeline rw=%s" % rw)
        pipe.Destroy()
    # a stage with every new argument at its default still runs the plain entries: same bits as the plain driver
    plain = nj.HydraulicErosionStage(ctx, 30, 1e-4, 1e-4, 0.01, 2.0)
    assert plain._desc() is None and plain.wear is None and plain.deposits is None
    drain.Dispose(); dhard.Dispose()


# 6. an invalid border mode, an overlapping mask and a mis-sized map: an error that names the argument, nothing written
def test_refusals_write_nothing(nj, ctx):
    res = 32
    sentinel = np.full((res, res), 7.25, f32)
    d, other, wear, deposits, rain = (ctx.from_host(sentinel) for _ in range(5))
    work = work_for(nj, ctx, res)
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    good = list(PARAMS[0])
    N = nj._native

    def all_entries(desc, name):
        t = N.RWTile(d.ptr, other.ptr, res, 1)
        for entry, head, tail in (("nz_hydraulic_erosion_ex", (d.ptr, work.ptr), (res,)),
                                  ("nz_hydraulic_erosion_ex_batch", (d.ptr, work.ptr), (res, 1)),
                                  ("nz_hydraulic_erosion_ex_rw", (C.byref(t), work.ptr), ())):
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, *head, C.byref(desc) if desc is not None else None, *tail)
            assert e.value.status == N.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))
        assert t.read == d.ptr

    for border in (2, -1, 7):
        all_entries(N.HydraulicDesc(5, *good, border, rain.ptr, None, wear.ptr, deposits.ptr), "border")
    all_entries(None, "desc")
    all_entries(N.HydraulicDesc(5, *good, 1, None, None, d.ptr, deposits.ptr), "wear")
    all_entries(N.HydraulicDesc(5, *good, 1, rain.ptr, None, wear.ptr, rain.ptr), "deposits")
    all_entries(N.HydraulicDesc(5, *good, 1, None, None, wear.ptr, wear.ptr), "wear")
    all_entries(N.HydraulicDesc(5, *good, 1, None, None, work.ptr + 4 * 100, None), "work")
    all_entries(N.HydraulicDesc(-1, *good, 1, None, None, None, None), "iterations")
    bad = list(good)
    bad[4] = 1.5
    all_entries(N.HydraulicDesc(5, *bad, 0, None, None, wear.ptr, None), "dissolve")
    # the stage checks the maps against the payload before any launch
    small = ctx.alloc(res * res - 1)
    for kw in (dict(rainMap=small), dict(hardness=small)):
        hyd = nj.HydraulicErosionStage(ctx, iterations=5, recordMasks=True, **kw)
        with pytest.raises(ValueError) as e:
            hyd.ReceiveHandledInput(nj.PipelineWorkItem(nj.GeneratorData("x", d, res, 0, 0)), nj.JobHandle())
        assert list(kw)[0] in str(e.value)
        hyd.Destroy()
    ctx.synchronize()
    for t, what in ((d, "src"), (other, "write plane"), (wear, "wear"), (deposits, "deposits"), (rain, "rainMap")):
        assert_bits(t.ToArray((res, res)), sentinel, what)
    assert (work.ToArray() == f32(7.25)).all()
    h = relief(res)
    d.CopyFrom(h)
    desc = N.HydraulicDesc(5, *good, 1, None, None, wear.ptr, deposits.ptr)
    ctx.call("nz_hydraulic_erosion_ex", d.ptr, work.ptr, C.byref(desc), res)
    want = X.run(h, 5, border=X.OPEN)
    assert_bits(d.ToArray((res, res)), want[0], "after the refusals")
    assert_bits(wear.ToArray((res, res)), want[2], "after the refusals: wear")
    for t in (d, other, wear, deposits, rain, work, small):
        t.Dispose()


# 7. recordMasks switched off between two payloads of equal length: the stage drops the planes, wear and deposits are empty again
def test_masks_switched_off_are_dropped(nj, ctx):
    res = 64
    h = relief(res)
    hyd = nj.HydraulicErosionStage(ctx, iterations=3, recordMasks=True)
    d = nj.GeneratorData("h", ctx.from_host(h), res, 0, 0)
    hyd.ReceiveHandledInput(nj.PipelineWorkItem(d), nj.JobHandle())
    hyd.jobHandle.Complete()
    want = X.run(h, 3)
    assert_bits(hyd.wear.ToArray((res, res)), want[2], "wear")
    hyd.recordMasks = False
    d.data.CopyFrom(h)
    hyd.ReceiveHandledInput(nj.PipelineWorkItem(d), nj.JobHandle())
    hyd.jobHandle.Complete()
    assert hyd.wear is None and hyd.deposits is None
    assert_bits(d.data.ToArray((res, res)), want[0], "the plain entries after the masks")
    hyd.Destroy()
    d.data.Dispose()
