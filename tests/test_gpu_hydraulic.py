"""Grid hydraulic erosion on the GPU (nz_hydraulic_erosion_stage*, HydraulicErosionStage) against the reference driver of
tests/hydraulic_ref.py: the result and the water plane equal the driver bit for bit on assorted tiles, capacity 0 leaves
the heights alone with the flow map's water, the in-place / _rw / _batch forms and the three float modes agree, a 4096^2
plane conserves its sum, the stage runs in a pipeline, and bad arguments write nothing."""
import ctypes as C
import math

import numpy as np
import pytest

import hydraulic_ref as H
from test_hydraulic_ref import NAMES, PARAMS, relief

pytestmark = pytest.mark.gpu
f32 = np.float32


def tiles():
    rng = np.random.default_rng(7)
    ramp = (np.arange(80, dtype=f32)[None, :] * f32(0.01) + np.arange(80, dtype=f32)[:, None] * f32(0.003)).astype(f32)
    imp = np.zeros((64, 64), f32)
    imp[31, 40] = f32(1.0)
    noisy = (relief(97, 97) + rng.standard_normal((97, 97)).astype(f32) * f32(0.01)).astype(f32)
    return {"fbm64": relief(64), "fbm160": relief(160, 500), "ramp80": ramp, "impulse64": imp,
            "const72": np.full((72, 72), f32(0.375)), "noisy97": noisy}


def work_for(nj, ctx, res, count=1):
    return ctx.alloc(nj._native.lib.nz_hydraulic_erosion_work_floats(res, count))


def run_gpu(nj, ctx, h, its, prm, form="inplace"):
    """One run of the stage on the host plane h (res x res, or count x res x res for the batch); -> (result, water)."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    src = ctx.from_host(h)
    work = work_for(nj, ctx, res, count)
    if form == "rw":
        other = ctx.alloc(h.size)
        t = nj._native.RWTile(src.ptr, other.ptr, res, count)
        ctx.call("nz_hydraulic_erosion_stage_rw", C.byref(t), work.ptr, its, *prm)
        out = src if t.read == src.ptr else other
        assert t.read in (src.ptr, other.ptr) and t.write in (src.ptr, other.ptr) and t.read != t.write
    elif form == "batch":
        ctx.call("nz_hydraulic_erosion_stage_batch", src.ptr, work.ptr, its, *prm, res, count)
        out = src
    else:
        ctx.call("nz_hydraulic_erosion_stage", src.ptr, work.ptr, its, *prm, res)
        out = src
    got = out.ToArray(h.shape)
    water = work.ToArray()[:h.size].reshape(h.shape)
    src.Dispose(); work.Dispose()
    if form == "rw":
        other.Dispose()
    return got, water


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


# 1. the result and the water plane equal the driver bit for bit
@pytest.mark.parametrize("name", ["fbm64", "fbm160", "ramp80", "impulse64", "const72", "noisy97"])
def test_matches_the_driver(nj, ctx, name):
    h = tiles()[name]
    for k, prm in enumerate(PARAMS):
        for its in (1, 2, 7, 50):
            got, water = run_gpu(nj, ctx, h, its, prm)
            want, wwant = H.run(h, its, **dict(zip(NAMES, prm)))
            assert_bits(got, want, "%s params %d its %d: result" % (name, k, its))
            assert_bits(water, wwant, "%s params %d its %d: water" % (name, k, its))


def test_zero_iterations_leave_the_input(nj, ctx):
    h = relief(64)
    for form in ("inplace", "rw", "batch"):
        got, water = run_gpu(nj, ctx, h, 0, PARAMS[0], form)
        assert_bits(got, h, form)
        assert (water == f32(PARAMS[0][0])).all(), form


# 2. capacity 0: the heights stay, the water is the fused flow map's
def test_capacity_zero_is_the_flow_map(nj, ctx):
    for res in (64, 97):
        h = relief(res)
        for its in (1, 3, 5):
            got, water = run_gpu(nj, ctx, h, its, (1e-4, 0.0, 0.0, 0.0, 0.3, 0.3, 0.01))
            assert_bits(got, h, "heights")
            hd = ctx.from_host(h)
            state = [ctx.alloc(res * res) for _ in range(5)]
            pout = (nj._native.dev_ptr * 5)(*[p.ptr for p in state])
            st = nj.Stripe(res, res, 0, res, 0, res, 0)
            ctx.call("nz_flow_fused_stripe", hd.ptr, None, pout, None, C.byref(st), its, 1, 0, 0.0, 1.0)
            assert_bits(water, state[0].ToArray((res, res)), "water res %d its %d" % (res, its))
            hd.Dispose()
            for p in state:
                p.Dispose()


# 3. in-place, _rw and _batch agree; every tile of a batch is the tile alone; all three float modes give the same bits
def test_forms_batch_and_float_modes_agree(nj, ctx):
    a, b, c = relief(96), relief(96, 170) * f32(3.0), np.full((96, 96), f32(1.5))
    b = b.astype(f32)
    batch = np.stack([a, b, c])
    for prm in PARAMS:
        for its in (1, 4, 9):
            single = [run_gpu(nj, ctx, t, its, prm) for t in (a, b, c)]
            for form in ("rw",):
                for t, (want, wwant) in zip((a, b, c), single):
                    got, water = run_gpu(nj, ctx, t, its, prm, form)
                    assert_bits(got, want, "rw its %d" % its)
                    assert_bits(water, wwant, "rw water its %d" % its)
            for form in ("batch", "rw"):
                got, water = run_gpu(nj, ctx, batch, its, prm, form)
                for k, (want, wwant) in enumerate(single):
                    assert_bits(got[k], want, "%s tile %d its %d" % (form, k, its))
                    assert_bits(water[k], wwant, "%s water tile %d its %d" % (form, k, its))
    want, wwant = run_gpu(nj, ctx, a, 9, PARAMS[1])
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got, water = run_gpu(nj, mctx, a, 9, PARAMS[1])
        finally:
            mctx.close()
        assert_bits(got, want, "float mode %d" % mode)
        assert_bits(water, wwant, "float mode %d water" % mode)


# 4. 4096^2, 8 iterations: the sum is conserved, every cell is finite, the plane is the driver's
def test_4096_conserves_and_matches(nj, ctx, oracle):
    res, its = 4096, 8
    h = oracle.fractal(oracle.SIMPLEX, res, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 1700)
    prm = (1e-3, 5e-4, 0.01, 4.0, 0.5, 0.3, 0.01)
    got, water = run_gpu(nj, ctx, h, its, prm)
    assert np.isfinite(got).all() and np.isfinite(water).all()
    s0, s1 = h.astype(np.float64).sum(), got.astype(np.float64).sum()
    assert abs(s1 - s0) <= 1e-6 * np.abs(h.astype(np.float64)).sum(), (s0, s1)
    assert not np.array_equal(got, h)
    want, wwant = H.run(h, its, **dict(zip(NAMES, prm)))
    assert_bits(got, want, "4096 result")
    assert_bits(water, wwant, "4096 water")


# 5. in a BasePipeline after a NoiseStage and a KernelFilterStage, single plane and READ / WRITE pair
def test_stage_in_a_pipeline(nj, ctx, oracle):
    res, xp, zp = 160, 4096, -2048
    noise = oracle.fractal(oracle.SIMPLEX, res, res, 0.4, 1.0, 2.0, 0.0, 13, xp, zp, 1700)
    filtered = oracle.kernel_filter(noise, oracle.GAUSS5_S1, 4)
    want, wwant = H.run(filtered, 30, capacity=2.0)
    for rw in (False, True):
        hyd = nj.HydraulicErosionStage(ctx, iterations=30, capacity=2.0)
        stages = [nj.NoiseStage(ctx, nj.FractalNoise.Simplex, 0.4, 1.0, 13, 2.0, 0.0, 1700),
                  nj.KernelFilterStage(ctx, nj.KernelFilterType.Gauss5_S1, 4), hyd]
        pipe = nj.BasePipeline(stages, "hydraulic")
        d = nj.GeneratorData("h", ctx.alloc(res * res), res, xp, zp, write=ctx.alloc(res * res) if rw else None)
        done = []
        pipe.Enqueue(d, completeAction=done.append)
        pipe.RunToCompletion()
        assert len(done) == 1
        assert_bits(d.data.ToArray((res, res)), want, "pipeline rw=%s" % rw)
        assert_bits(hyd.water.ToArray((res, res)), wwant, "pipeline water rw=%s" % rw)
        pipe.Destroy()


# 6. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    sentinel = np.full((res, res), 7.25, f32)
    d = ctx.from_host(sentinel)
    other = ctx.from_host(sentinel)
    work = work_for(nj, ctx, res)
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    good = list(PARAMS[0])
    bad = []
    for i, name in enumerate(NAMES):
        for v in (math.nan, math.inf, -math.inf, -1e-3):
            bad.append((i, v, name))
        if name in ("evaporation", "dissolve", "deposit"):
            bad.append((i, 1.0 + 1e-6, name))
    for i, v, name in bad:
        prm = list(good)
        prm[i] = v
        t = nj._native.RWTile(d.ptr, other.ptr, res, 1)
        for entry, head, tail in (("nz_hydraulic_erosion_stage", (d.ptr, work.ptr, 5), (res,)),
                                  ("nz_hydraulic_erosion_stage_batch", (d.ptr, work.ptr, 5), (res, 1)),
                                  ("nz_hydraulic_erosion_stage_rw", (C.byref(t), work.ptr, 5), ())):
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, *head, *prm, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, v)
        assert t.read == d.ptr
    with pytest.raises(nj.NoizeError) as e:
        ctx.call("nz_hydraulic_erosion_stage", d.ptr, work.ptr, -1, *good, res)
    assert e.value.status == nj._native.NZ_ERR_INVALID and "iterations" in str(e.value)
    ctx.synchronize()
    assert_bits(d.ToArray((res, res)), sentinel, "src")
    assert_bits(other.ToArray((res, res)), sentinel, "write plane")
    assert (work.ToArray() == f32(7.25)).all()
    h = relief(res)
    d.CopyFrom(h)
    ctx.call("nz_hydraulic_erosion_stage", d.ptr, work.ptr, 5, *good, res)
    want, wwant = H.run(h, 5)
    assert_bits(d.ToArray((res, res)), want, "after the refusals")
    d.Dispose(); other.Dispose(); work.Dispose()
