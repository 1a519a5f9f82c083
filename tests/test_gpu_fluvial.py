"""Stream-power fluvial erosion on the GPU (nz_fluvial_erosion*, FluvialErosionStage) against the numpy model of
tests/fluvial_ref.py, bit for bit throughout: result and drainage on assorted tiles and sizes, the in-place / _rw / _batch
forms and the three float modes, every option, planes carved from a guarded slab at four alignments, drainageIn continuing
the accumulation, a 4096^2 plane on a band around a seam of the launch grid, the stage in a pipeline, and bad arguments."""
import ctypes as C
import math

import numpy as np
import pytest

import fluvial_ref as F
from test_gpu_slab import PAIRS, carved, memo
from test_hydraulic_ref import relief

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
# erodibility, uplift, dt, rain, seaLevel: the defaults, a sea with fractional rain, a long step with strong uplift
PARAMS = [(0.05, 0.002, 1.0, 1.0, OFF), (0.2, 0.0, 0.5, 0.25, 0.3), (0.01, 0.01, 2.0, 3.0, OFF)]
NAMES = ("erodibility", "uplift", "dt", "rain", "seaLevel")


def tiles():
    rng = np.random.default_rng(7)

    def ramp(res):
        return (np.arange(res, dtype=f32)[None, :] * f32(0.01) + np.arange(res, dtype=f32)[:, None] * f32(0.003)).astype(f32)
    imp = np.zeros((64, 64), f32)
    imp[31, 40] = f32(1.0)
    noisy = (relief(97, 97) + rng.standard_normal((97, 97)).astype(f32) * f32(0.01)).astype(f32)
    t = {"fbm64": relief(64), "fbm65": relief(65, 120), "fbm160": relief(160, 500), "ramp17": ramp(17), "ramp97": ramp(97),
         "impulse64": imp, "const65": np.full((65, 65), f32(0.375)), "noisy97": noisy}
    for res in (1, 2, 3):  # every cell lies on the border
        t["rand%d" % res] = rng.random((res, res), dtype=f32)
    return t


def desc_of(nj, its, prm, rainMap=None, hardness=None, upliftMap=None, drainageIn=None):
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731
    return nj._native.FluvialDesc(its, *prm, ptr(rainMap), ptr(hardness), ptr(upliftMap), ptr(drainageIn))


def run_gpu(nj, ctx, h, its, prm, form="inplace", **planes):
    """One run on the host plane h (res x res, or count x res x res); planes: host arrays of the options.
    -> (result, drainage)."""
    h = np.ascontiguousarray(h, f32)
    res = h.shape[-1]
    count = h.shape[0] if h.ndim == 3 else 1
    src = ctx.from_host(h)
    work = ctx.alloc(nj._native.lib.nz_fluvial_erosion_work_floats(res, count))
    dev = {k: ctx.from_host(np.ascontiguousarray(v, f32)) for k, v in planes.items()}
    desc = desc_of(nj, its, prm, **dev)
    other = None
    if form == "rw":
        other = ctx.alloc(h.size)
        t = nj._native.RWTile(src.ptr, other.ptr, res, count)
        ctx.call("nz_fluvial_erosion_rw", C.byref(t), work.ptr, C.byref(desc))
        assert t.read in (src.ptr, other.ptr) and t.write in (src.ptr, other.ptr) and t.read != t.write
        out = src if t.read == src.ptr else other
    elif form == "batch":
        ctx.call("nz_fluvial_erosion_batch", src.ptr, work.ptr, C.byref(desc), res, count)
        out = src
    else:
        assert count == 1
        ctx.call("nz_fluvial_erosion", src.ptr, work.ptr, C.byref(desc), res)
        out = src
    got = out.ToArray(h.shape)
    drainage = work.ToArray()[:h.size].reshape(h.shape)
    for t in [src, work, other] + list(dev.values()):
        if t is not None:
            t.Dispose()
    return got, drainage


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != np.ascontiguousarray(want, f32).view(np.uint32)
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], np.asarray(want)[bad][0])


def ref(h, its, prm, **planes):
    return F.run(h, its, **dict(zip(NAMES, prm)), **planes)


# 1. the result and the drainage equal the model bit for bit
@pytest.mark.parametrize("name", ["fbm64", "fbm65", "fbm160", "ramp17", "ramp97", "impulse64", "const65", "noisy97", "rand1",
                                  "rand2", "rand3"])
def test_matches_the_model(nj, ctx, name):
    h = tiles()[name]
    for k, prm in enumerate(PARAMS):
        for its in (1, 2, 7, 50):
            got, drainage = run_gpu(nj, ctx, h, its, prm)
            want, dwant = ref(h, its, prm)
            assert_bits(got, want, "%s params %d its %d: result" % (name, k, its))
            assert_bits(drainage, dwant, "%s params %d its %d: drainage" % (name, k, its))
    if name == "const65":  # no receivers anywhere: the first iteration only lifts the inner cells and nothing accumulates
        got, drainage = run_gpu(nj, ctx, h, 1, PARAMS[0])
        assert (drainage == 1).all() and (got[1:-1, 1:-1] > h[1:-1, 1:-1]).all() and (got[0] == h[0]).all()


# 2. in-place, _rw and _batch agree; every tile of a batch is the tile alone; all float modes give the same bits
def test_forms_batch_and_float_modes_agree(nj, ctx):
    a, b, c = relief(48), (relief(48, 170) * f32(3.0)).astype(f32), tiles()["ramp97"][:48, :48].copy()
    batch = np.stack([a, b, c])
    for prm in PARAMS[:2]:
        for its in (0, 1, 4, 9):
            single = [run_gpu(nj, ctx, t, its, prm) for t in (a, b, c)]
            for t, (want, dwant) in zip((a, b, c), single):
                mwant, mdwant = ref(t, its, prm)
                assert_bits(want, mwant, "single its %d" % its)
                assert_bits(dwant, mdwant, "single drainage its %d" % its)
                got, drainage = run_gpu(nj, ctx, t, its, prm, "rw")
                assert_bits(got, want, "rw its %d" % its)
                assert_bits(drainage, dwant, "rw drainage its %d" % its)
            for form in ("batch", "rw"):
                got, drainage = run_gpu(nj, ctx, batch, its, prm, form)
                for k, (want, dwant) in enumerate(single):
                    assert_bits(got[k], want, "%s tile %d its %d" % (form, k, its))
                    assert_bits(drainage[k], dwant, "%s drainage tile %d its %d" % (form, k, its))
    want, dwant = run_gpu(nj, ctx, a, 9, PARAMS[1])
    for mode in (1, 2):
        mctx = nj.Context(0)
        try:
            mctx.float_mode = mode
            got, drainage = run_gpu(nj, mctx, a, 9, PARAMS[1])
        finally:
            mctx.close()
        assert_bits(got, want, "float mode %d" % mode)
        assert_bits(drainage, dwant, "float mode %d drainage" % mode)


def test_zero_iterations_leave_the_input(nj, ctx):
    h = relief(64)
    rm = maps_for(h.shape)["rainMap"]
    for form in ("inplace", "rw", "batch"):
        hh = h[None] if form == "batch" else h
        got, drainage = run_gpu(nj, ctx, hh, 0, PARAMS[2], form)
        assert_bits(got, hh, form)
        assert (drainage == f32(3.0)).all(), form
        got, drainage = run_gpu(nj, ctx, hh, 0, PARAMS[2], form, rainMap=rm)
        assert_bits(drainage.reshape(h.shape), f32(3.0) * rm, form + " with a rain map")
        got, drainage = run_gpu(nj, ctx, hh, 0, PARAMS[2], form, drainageIn=h)
        assert_bits(drainage.reshape(h.shape), h, form + " with drainageIn")


# 3. the options
def maps_for(shape, seed=11):
    rng = np.random.default_rng(seed)
    return {"rainMap": (rng.random(shape, dtype=f32) * f32(2.0)).astype(f32),
            "hardness": rng.random(shape, dtype=f32),
            "upliftMap": (rng.random(shape, dtype=f32) * f32(3.0)).astype(f32),
            "drainageIn": (f32(1.0) + rng.random(shape, dtype=f32) * f32(40.0)).astype(f32)}


def test_every_option_alone_and_all_together(nj, ctx):
    h = tiles()["noisy97"]
    maps = maps_for(h.shape)
    for names in [(k,) for k in maps] + [tuple(maps)]:
        planes = {k: maps[k] for k in names}
        for its in (1, 2, 7):  # an odd and an even count: the start plane of the rain map takes either side
            for prm in (PARAMS[0], PARAMS[1]):
                got, drainage = run_gpu(nj, ctx, h, its, prm, **planes)
                want, dwant = ref(h, its, prm, **planes)
                assert_bits(got, want, "%s its %d: result" % (names, its))
                assert_bits(drainage, dwant, "%s its %d: drainage" % (names, its))
    # the identity maps give the no-map bits; a hardness of ones leaves only the uplift
    want, dwant = run_gpu(nj, ctx, h, 7, PARAMS[0])
    ones, zeros = np.ones(h.shape, f32), np.zeros(h.shape, f32)
    for planes in (dict(rainMap=ones), dict(hardness=zeros), dict(upliftMap=ones), dict(rainMap=ones, hardness=zeros, upliftMap=ones)):
        got, drainage = run_gpu(nj, ctx, h, 7, PARAMS[0], **planes)
        assert_bits(got, want, "identity %s" % list(planes))
        assert_bits(drainage, dwant, "identity %s drainage" % list(planes))
    got, _ = run_gpu(nj, ctx, h, 7, PARAMS[0], hardness=ones)
    rise = h.copy()
    for _ in range(7):
        rise = np.where(F.outlets(h), h, rise + f32(1.0) * f32(0.002)).astype(f32)
    assert_bits(got, rise, "hardness of ones")


# 4. planes carved from one guarded allocation at four alignments and three mixed pairs: the guards stay silent
@pytest.mark.parametrize("res", [64, 97])
def test_on_slab_carved_planes(nj, ctx, res):
    h = memo(("fluvial relief", res), lambda: relief(res, 300))
    n, its, prm = res * res, 3, PARAMS[0]
    maps = maps_for((res, res), 5)
    want = memo(("fluvial", res), lambda: ref(h, its, prm))
    want_maps = memo(("fluvial maps", res), lambda: ref(h, its, prm, **maps))
    nwork = nj._native.lib.nz_fluvial_erosion_work_floats(res, 1)
    for p, q in PAIRS:
        what = (res, p, q)
        with carved(ctx, res, src=(n, p, h), work=(nwork, q, None)) as (s, t):
            ctx.call("nz_fluvial_erosion", t.src.ptr, t.work.ptr, C.byref(desc_of(nj, its, prm)), res).Complete()
            assert_bits(t.src.ToArray((res, res)), want[0], ("in place",) + what)
            assert_bits(t.work.ToArray()[:n].reshape(res, res), want[1], ("in place drainage",) + what)
            s.check()
        ph = [p] * 4 if p == q else [q, (q + 1) % 4, (q + 2) % 4, (p + 2) % 4]
        with carved(ctx, res, src=(n, p, h), other=(n, q, None), work=(nwork, ph[0], None), rainMap=(n, ph[1], maps["rainMap"]),
                    hardness=(n, ph[2], maps["hardness"]), upliftMap=(n, ph[3], maps["upliftMap"]),
                    drainageIn=(n, ph[0], maps["drainageIn"])) as (s, t):
            desc = desc_of(nj, its, prm, t.rainMap, t.hardness, t.upliftMap, t.drainageIn)
            rw = nj._native.RWTile(t.src.ptr, t.other.ptr, res, 1)
            ctx.call("nz_fluvial_erosion_rw", C.byref(rw), t.work.ptr, C.byref(desc)).Complete()
            out = t.src if rw.read == t.src.ptr else t.other
            assert_bits(out.ToArray((res, res)), want_maps[0], ("rw with maps",) + what)
            assert_bits(t.work.ToArray()[:n].reshape(res, res), want_maps[1], ("rw with maps drainage",) + what)
            for k in maps:
                assert_bits(getattr(t, k).ToArray((res, res)), maps[k], "%s is read only" % k)
            s.check()
    count = 3
    hh = memo(("fluvial batch in", res), lambda: np.stack([h, h[::-1].copy(), h.T.copy()]))
    want_b = memo(("fluvial batch", res), lambda: [ref(hh[k], its, prm) for k in range(count)])
    nwork = nj._native.lib.nz_fluvial_erosion_work_floats(res, count)
    for p, q in PAIRS:
        with carved(ctx, res, src=(count * n, p, hh), work=(nwork, q, None)) as (s, t):
            ctx.call("nz_fluvial_erosion_batch", t.src.ptr, t.work.ptr, C.byref(desc_of(nj, its, prm)), res, count).Complete()
            got, drainage = t.src.ToArray((count, res, res)), t.work.ToArray()[:count * n].reshape(count, res, res)
            for k in range(count):
                assert_bits(got[k], want_b[k][0], ("batch", k, res, p, q))
                assert_bits(drainage[k], want_b[k][1], ("batch drainage", k, res, p, q))
            s.check()


# 5. the drainage of one call handed to the next continues the Jacobi iteration
def test_drainage_in_continues_the_accumulation(nj, ctx):
    h = relief(96)
    still = (0.0, 0.0, 1.0, 1.0, OFF)
    _, first = run_gpu(nj, ctx, h, 5, still)
    got, second = run_gpu(nj, ctx, h, 6, still, drainageIn=first)
    want, dwant = ref(h, 11, still)
    assert_bits(got, h, "heights")
    assert_bits(second, dwant, "5 + 6 iterations")
    assert_bits(run_gpu(nj, ctx, h, 11, still)[1], dwant, "11 iterations")
    # with erosion on, the heights of the first call go on as well
    h1, a1 = run_gpu(nj, ctx, h, 4, PARAMS[0])
    h2, a2 = run_gpu(nj, ctx, h1, 3, PARAMS[0], drainageIn=a1)
    want, dwant = ref(h, 7, PARAMS[0])
    assert_bits(h2, want, "4 + 3 iterations: result")
    assert_bits(a2, dwant, "4 + 3 iterations: drainage")


# 6. 4096^2, 5 iterations: finite, within the bounds, and the model's bits on a band around a seam of the launch grid
def test_4096_band_matches(nj, ctx):
    res, its, prm = 4096, 5, PARAMS[0]
    d = ctx.alloc(res * res)
    ctx.call("nz_fractal", int(nj.FractalNoise.Simplex), d.ptr, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 1700).Complete()
    h = d.ToArray((res, res))
    d.Dispose()
    got, drainage = run_gpu(nj, ctx, h, its, prm)
    assert np.isfinite(got).all() and np.isfinite(drainage).all()
    assert got.min() >= h.min()
    top = its * 1.0 * 0.002
    assert float((got.astype(np.float64) - h).max()) <= top + its * float(np.spacing(f32(np.abs(h).max() + top)))
    assert (drainage >= f32(1.0)).all() and drainage.max() > 1
    assert not np.array_equal(got, h)
    # rows 1920 .. 2175 straddle the tile seams at multiples of 16 around row 2048; one iteration reaches 2 rows, so 10 rows
    # of margin keep the band's own borders out of it
    z0, z1, margin = 1920, 2176, 2 * its
    want, dwant = ref(h[z0 - margin:z1 + margin], its, prm)
    assert_bits(got[z0:z1], want[margin:-margin], "4096 band: result")
    assert_bits(drainage[z0:z1], dwant[margin:-margin], "4096 band: drainage")


# 7. in a BasePipeline after a NoiseStage and a Gauss filter, single plane and READ / WRITE pair
def test_stage_in_a_pipeline(nj, ctx, oracle):
    res, xp, zp = 160, 4096, -2048
    noise = oracle.fractal(oracle.SIMPLEX, res, res, 0.4, 1.0, 2.0, 0.0, 13, xp, zp, 1700)
    filtered = oracle.kernel_filter(noise, oracle.GAUSS5_S1, 4)
    want, dwant = F.run(filtered, 30, erodibility=0.1)
    for rw in (False, True):
        flu = nj.FluvialErosionStage(ctx, iterations=30, erodibility=0.1)
        stages = [nj.NoiseStage(ctx, nj.FractalNoise.Simplex, 0.4, 1.0, 13, 2.0, 0.0, 1700),
                  nj.KernelFilterStage(ctx, nj.KernelFilterType.Gauss5_S1, 4), flu]
        pipe = nj.BasePipeline(stages, "fluvial")
        d = nj.GeneratorData("h", ctx.alloc(res * res), res, xp, zp, write=ctx.alloc(res * res) if rw else None)
        done = []
        pipe.Enqueue(d, completeAction=done.append)
        pipe.RunToCompletion()
        assert len(done) == 1
        assert_bits(d.data.ToArray((res, res)), want, "pipeline rw=%s" % rw)
        assert_bits(flu.drainage.ToArray((res, res)), dwant, "pipeline drainage rw=%s" % rw)
        pipe.Destroy()


# 8. each invalid argument is NZ_ERR_INVALID, names the argument and writes nothing; the context stays usable
def test_invalid_arguments_write_nothing(nj, ctx):
    res = 32
    n = res * res
    sentinel = np.full((res, res), 7.25, f32)
    d = ctx.from_host(sentinel)
    other = ctx.from_host(sentinel)
    apart = ctx.from_host(sentinel)
    work = ctx.alloc(nj._native.lib.nz_fluvial_erosion_work_floats(res, 1))
    work.CopyFrom(np.full(work.Length, 7.25, f32))
    good = list(PARAMS[0])

    def refused(name, desc):
        t = nj._native.RWTile(d.ptr, other.ptr, res, 1)
        p = C.byref(desc) if desc is not None else None
        for entry, head, tail in (("nz_fluvial_erosion", (d.ptr, work.ptr), (res,)),
                                  ("nz_fluvial_erosion_batch", (d.ptr, work.ptr), (res, 1)),
                                  ("nz_fluvial_erosion_rw", (C.byref(t), work.ptr), ())):
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(entry, *head, p, *tail)
            assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value), (entry, name, str(e.value))
        assert t.read == d.ptr

    for i, name in enumerate(NAMES):
        for v in (math.nan, math.inf, -math.inf) + (() if name == "seaLevel" else (-1e-3,)):
            prm = list(good)
            prm[i] = v
            refused(name, desc_of(nj, 5, prm))
    refused("iterations", desc_of(nj, -1, good))
    refused("desc", None)
    inside = ctx.wrap(work.ptr + 4 * (n + 8), n)  # a plane inside `work`
    half = ctx.wrap(d.ptr + 4 * (n // 2), n)      # a plane that begins inside `src`
    for name in ("drainageIn", "rainMap", "hardness", "upliftMap"):
        for plane in (d, inside, half):
            refused(name, desc_of(nj, 5, good, **{name: plane}))
        # the write plane of the pair counts for the _rw form only
        t = nj._native.RWTile(d.ptr, other.ptr, res, 1)
        with pytest.raises(nj.NoizeError) as e:
            ctx.call("nz_fluvial_erosion_rw", C.byref(t), work.ptr, C.byref(desc_of(nj, 5, good, **{name: other})))
        assert e.value.status == nj._native.NZ_ERR_INVALID and name in str(e.value)
    ctx.synchronize()
    assert_bits(d.ToArray((res, res)), sentinel, "src")
    assert_bits(other.ToArray((res, res)), sentinel, "write plane")
    assert (work.ToArray() == f32(7.25)).all()
    # a sea level of -FLT_MAX is in range, read-only planes may alias each other, and the context still works
    h = relief(res)
    d.CopyFrom(h)
    ones = np.ones((res, res), f32)
    apart.CopyFrom(ones)
    ctx.call("nz_fluvial_erosion", d.ptr, work.ptr, C.byref(desc_of(nj, 5, good, rainMap=apart, upliftMap=apart)), res)
    want, dwant = ref(h, 5, good)
    assert_bits(d.ToArray((res, res)), want, "after the refusals")
    assert_bits(work.ToArray()[:n].reshape(res, res), dwant, "after the refusals: drainage")
    for t in (d, other, apart, work):
        t.Dispose()
