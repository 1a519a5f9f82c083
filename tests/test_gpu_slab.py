"""Every entry on planes carved out of one guarded slab (tests/slab.py), at the four 4-byte phases of the 16-byte alignment.

The other GPU tests hand every plane over as its own nz_tile_alloc allocation: 256-byte aligned and followed by the
allocator's slack.  So the base-pointer term of every aligned / vec decision of the launchers is always zero there, and
no access outside a plane can be seen.  Here every plane of a call lies inside ONE allocation, 4 * phase bytes past a
16-byte boundary, with max(2 * pitch, 1024) floats of the canary word either side.  The result is compared with the same
independent reference, in the same way, as the entry's own test (oracle.*, conv_ref, hydraulic_ref / hydraulic_ex_ref,
fractal_shapes_ref, fractal_warp_ref) -- never with the library's own phase-0 result -- and then slab.check() requires the
canary in every byte outside the planes.  Entries with two or more planes also run the mixed pairs primary / partner =
0 / 1, 2 / 0 and 3 / 2: the combinations an OR-ed alignment flag folds together."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest

import conv_ref as R
import flow_ref as F
from slab import Slab, is_canary

pytestmark = pytest.mark.gpu
f32 = np.float32
SAME = [(0, 0), (1, 1), (2, 2), (3, 3)]
PAIRS = SAME + [(0, 1), (2, 0), (3, 2)]   # (primary, partner)
_memo = {}


def memo(key, fn):
    """A reference is computed once and shared by every phase that needs it; nothing writes to it."""
    if key not in _memo:
        _memo[key] = fn()
        if isinstance(_memo[key], np.ndarray):
            _memo[key].setflags(write=False)
    return _memo[key]


def third(p, q, k=1):
    """Phase of a further plane: the common phase when primary and partner agree, otherwise one of the others."""
    return p if p == q else (q + k) % 4


@contextlib.contextmanager
def carved(ctx, pitch, **planes):
    """name=(n, phase, fill) or (n, phase, fill, dtype) or (n, None, fill, dtype, byte_phase) -> (slab, tiles)."""
    s = Slab(ctx, max(2 * pitch, 1024))
    t = {}
    for name, spec in planes.items():
        n, phase, fill = spec[:3]
        dtype = spec[3] if len(spec) > 3 else f32
        bp = spec[4] if len(spec) > 4 else None
        t[name] = s.carve(n, phase or 0, dtype=dtype, fill=fill, name=name, byte_phase=bp)
    s.upload()
    try:
        yield s, types.SimpleNamespace(**t)
    finally:
        s.Dispose()


def same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(-1))
        raise AssertionError("%s: %d/%d cells differ, first at %d: %r vs %r" % (
            what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


def bits(got, want, what):
    R.assert_bits_equal(np.asarray(got), np.asarray(want), str(what))


@pytest.fixture(scope="module")
def fctx(nj):
    c = nj.Context(0)
    c.float_mode = nj._native.NZ_FLOAT_FAST
    yield c
    c.close()


# ---- element-wise --------------------------------------------------------------------------------------------------------
def _ab(res):
    rng = np.random.default_rng(21 + res)
    a = (rng.random((res, res), dtype=f32) * f32(1.4) - f32(0.2)).astype(f32)
    return a, rng.random((res, res), dtype=f32)


@pytest.mark.parametrize("res", [4, 64, 129, 132])
def test_constant_job(ctx, oracle, res):
    a, _ = _ab(res)
    for op in (0, 1):
        want = memo(("const", res, op), lambda: oracle.constant(a, op, 0.37))
        for p, q in PAIRS:
            with carved(ctx, res, src=(res * res, p, a), tmp=(res * res, q, None)) as (s, t):
                ctx.call("nz_constant_job", op, t.src.ptr, t.tmp.ptr, 0.37, res).Complete()
                same(t.src.ToArray((res, res)), want, ("constant", op, res, p, q))
                s.check()


@pytest.mark.parametrize("res", [4, 64, 129, 132])
def test_reduction_job(ctx, oracle, res):
    a, b = _ab(res)
    for op in range(5):
        want = memo(("reduce", res, op), lambda: oracle.reduce(a, b, op))
        for p, q in PAIRS:
            with carved(ctx, res, srcL=(res * res, p, a), srcR=(res * res, q, b),
                        tmp=(res * res, third(p, q), None)) as (s, t):
                ctx.call("nz_reduction_job", op, t.srcL.ptr, t.srcR.ptr, t.tmp.ptr, res).Complete()
                same(t.srcL.ToArray((res, res)), want, ("reduce", op, res, p, q))
                bits(t.srcR.ToArray((res, res)), b, ("reduce: srcR is read only", op, res, p, q))
                s.check()
    # the special operands of MAX / MIN (NaN loses, a tie keeps the second operand), as test_constant_reduce_curve_stages
    n = max(res, 8)
    sa, sb = np.zeros(n * n, f32).reshape(n, n), np.zeros(n * n, f32).reshape(n, n)
    sa[0, :8] = [0.0, -0.0, 0.0, -0.0, 1.0, np.nan, np.nan, np.inf]
    sb[0, :8] = [-0.0, 0.0, 0.0, -0.0, np.nan, 1.0, np.nan, -np.inf]
    for op in (3, 4):
        want = oracle.reduce(sa, sb, op)
        for p, q in PAIRS:
            with carved(ctx, n, srcL=(n * n, p, sa), srcR=(n * n, q, sb), tmp=(n * n, q, None)) as (s, t):
                ctx.call("nz_reduction_job", op, t.srcL.ptr, t.srcR.ptr, t.tmp.ptr, n).Complete()
                assert np.array_equal(t.srcL.ToArray((n, n)), want, equal_nan=True), (op, n, p, q)
                s.check()


@pytest.mark.parametrize("res", [4, 64, 129, 132])
def test_curve_job(ctx, oracle, res):
    a, _ = _ab(res)
    for fn, samples in ((lambda v: 1.0 - v, 256), (lambda v: 1.5 * v - 0.1, 7), (lambda v: 2.0 * v + 0.25, 2)):
        lut = np.array([fn(f32(i) / f32(samples)) for i in range(samples)], f32)
        want = memo(("curve", res, samples), lambda: oracle.curve(a, lut))
        for p, q in PAIRS:
            for cp in sorted({1, q}):       # the curve array itself off the boundary as well
                with carved(ctx, res, src=(res * res, p, a), tmp=(res * res, q, None), curve=(samples, cp, lut)) as (s, t):
                    ctx.call("nz_curve_job", t.src.ptr, t.tmp.ptr, t.curve.ptr, samples, res).Complete()
                    same(t.src.ToArray((res, res)), want, ("curve", samples, res, p, q, cp))
                    bits(t.curve.ToArray(), lut, "curve array is read only")
                    s.check()


@pytest.mark.parametrize("res", [4, 64, 129, 132])
def test_fill_array(ctx, res):
    for p in range(4):
        with carved(ctx, res, data=(res * res, p, None)) as (s, t):
            ctx.call("nz_fill_array", t.data.ptr, res, 0.0001).Complete()
            bits(t.data.ToArray(), np.full(res * res, 0.0001, f32), ("fill", res, p))
            s.check()


@pytest.mark.parametrize("res", [4, 64, 129, 132])
def test_update_flow_from_track(ctx, oracle, res):
    rng = np.random.default_rng(res)
    pool = np.where(rng.random((res, res)) < 0.35, rng.random((res, res), dtype=f32) * f32(0.3), 0).astype(f32)
    pool[0, :] = f32(0.05)
    flow = rng.random((res, res), dtype=f32)
    track = np.where(rng.random((res, res)) < 0.5, rng.random((res, res), dtype=f32), 0).astype(f32)
    want = oracle.update_flow_from_track(pool, flow, track, 0.05, 0.1, 700.0)
    n = res * res
    for p, q in PAIRS:
        r = p if p == q else 3 - p
        with carved(ctx, res, pool=(n, p, pool), flow=(n, q, flow), track=(n, r, track)) as (s, t):
            ctx.call("nz_update_flow_from_track", t.pool.ptr, t.flow.ptr, t.track.ptr, 0.05, 0.1, 700.0, res).Complete()
            for name, w in zip(("pool", "flow", "track"), want):
                same(getattr(t, name).ToArray((res, res)), w, ("flow from track", name, res, p, q, r))
            s.check()


# ---- range and normalise ---------------------------------------------------------------------------------------------------
def _range_case(n, case):
    rng = np.random.default_rng(n * 10 + case)
    a = (rng.random(n, dtype=f32) * f32(4) - f32(1.5)).astype(f32)
    lim = (np.inf, -np.inf)
    if case == 1:            # NaN cells are skipped
        a[rng.random(n) < 0.3] = np.nan
    elif case == 2:          # minimum zero: the sign of the LAST zero cell stays
        a = np.abs(a); a[rng.integers(0, n, 5)] = f32(0.0); a[rng.integers(0, n, 5)] = f32(-0.0)
    elif case == 3:          # maximum zero
        a = -np.abs(a); a[rng.integers(0, n, 5)] = f32(-0.0); a[rng.integers(0, n, 5)] = f32(0.0)
    elif case == 4:          # limits inside the data's range, and a zero limit with no zero cell
        a = np.abs(a) + f32(0.25); lim = (-0.0, 1.0)
    elif case == 5:          # nothing but NaN
        a[:] = np.nan; lim = (2.0, -3.0)
    return a, lim


@pytest.mark.parametrize("n", [1, 2, 3, 5, 1023, 1026, 4099, 256 * 1024 + 7])
def test_get_map_range_and_normalize_cells(ctx, oracle, n):
    for case in range(6):
        a, lim = _range_case(n, case)
        want = oracle.get_map_range(a, *lim)
        norm = oracle.normalize_args(a.reshape(1, n), want).reshape(n) if case in (0, 4) else None
        for p, q in PAIRS:
            with carved(ctx, 512, map=(n, p, a), res=(3, q, None)) as (s, t):
                h = ctx.call("nz_get_map_range", t.map.ptr, n, t.res.ptr, lim[0], lim[1])
                h.Complete()
                got = t.res.ToArray()
                assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (n, case, p, q, got, want)
                bits(t.map.ToArray(), a, "the map is read only")
                s.check()
                if norm is not None:   # NormalizeMap reading the device {min, max, range} the range job left
                    ctx.call("nz_normalize_cells_dev", t.map.ptr, n, t.res.ptr).Complete()
                    same(t.map.ToArray(), norm, ("normalize cells", n, case, p, q))
                    s.check()


@pytest.mark.parametrize("side", [1, 2, 32, 65, 132])
def test_map_normalize_values_dev(ctx, oracle, side):
    a = np.random.default_rng(side).random((side, side), dtype=f32)
    args = oracle.get_map_range(a)
    want = oracle.normalize_args(a, args)
    n = side * side
    for p, q in PAIRS:
        with carved(ctx, side, src=(n, p, a), tmp=(n, third(p, q), None), args=(3, q, args)) as (s, t):
            ctx.call("nz_map_normalize_values_dev", t.src.ptr, t.tmp.ptr, t.args.ptr, side).Complete()
            same(t.src.ToArray((side, side)), want, ("normalize dev", side, p, q))
            s.check()
        with carved(ctx, side, src=(n, p, a), res=(3, q, None)) as (s, t):   # the chain of the existing test, src as tmp
            h = ctx.call("nz_get_map_range", t.src.ptr, n, t.res.ptr, np.inf, -np.inf)
            ctx.call("nz_map_normalize_values_dev", t.src.ptr, t.src.ptr, t.res.ptr, side, dep=h).Complete()
            same(t.src.ToArray((side, side)), want, ("range -> normalize", side, p, q))
            s.check()


# ---- thermal erosion -------------------------------------------------------------------------------------------------------
THERMAL = ((1, 45, 0.5, 0.75), (3, 20, 0.25, 0.3), (2, 80, 0.5, 2.0))


def _at_rest(res):
    """Constant 0.5 with a few steep 2 x 2 bumps: most quads stay as they are, so one float4 holds a quad that is written
    back next to one that is not; a bump straddles a float4 boundary, one sits in the last column pair."""
    t = np.full((res, res), 0.5, f32)
    for z, x in ((0, 0), (res // 2, 3), (res // 2 + 1, res // 2 + 1), (res - 2, res - 2), (1, res - 2), (res // 3, 6)):
        z, x = min(max(z, 0), res - 2), min(max(x, 0), res - 2)
        t[z:z + 2, x:x + 2] += f32(0.4)
    return t


@pytest.mark.parametrize("res", [4, 8, 66, 256, 2048])
def test_thermal_erosion(ctx, oracle, res):
    planes = {"random": np.random.default_rng(res).random((res, res), dtype=f32), "at rest": _at_rest(res)}
    for name, a in planes.items():
        for iters, talus, inc, ratio in (THERMAL if name == "random" else THERMAL[:2]):
            want = memo(("thermal", res, name, iters), lambda: oracle.thermal_erosion(a, float(talus), inc, ratio, iters))
            if name == "at rest" and res >= 66:   # both outcomes of "this quad is written back"
                assert not np.array_equal(want, a) and (want == a).mean() > 0.5
            for p in range(4):
                with carved(ctx, res, src=(res * res, p, a)) as (s, t):
                    ctx.call("nz_thermal_erosion", t.src.ptr, float(talus), inc, ratio, iters, res).Complete()
                    same(t.src.ToArray((res, res)), want, ("thermal", name, res, iters, p))
                    s.check()


# ---- crop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_res", [64, 150, 161])
def test_crop_job(ctx, oracle, out_res):
    a = np.random.default_rng(5).random((150, 150), dtype=f32)
    want = oracle.crop(a, out_res)
    for p, q in PAIRS:
        with carved(ctx, 161, input=(150 * 150, p, a), output=(out_res * out_res, q, None)) as (s, t):
            ctx.call("nz_crop_job", t.input.ptr, 150, t.output.ptr, out_res).Complete()
            same(t.output.ToArray((out_res, out_res)), want, ("crop", out_res, p, q))
            bits(t.input.ToArray((150, 150)), a, "crop: the input is read only")
            s.check()


# ---- filters ---------------------------------------------------------------------------------------------------------------
CAP = {3: 6, 5: 9, 7: 3, 9: 3}   # fusion depth per launch at 300^2 (CAP / _counts of test_gpu_conv_exact.py)
KSIZE = {0: 9, 1: 7, 2: 5, 3: 3, 8: 3, 11: 3}


def _signed(seed, shape, scale=8.0):
    return ((np.random.default_rng(seed).random(shape, dtype=f32) - f32(0.3)) * f32(scale)).astype(f32)


def _inplace(ctx, name, res, a, p, q, *args, what=None, want=None):
    n = res * res
    with carved(ctx, res, src=(n, p, a), tmp=(n, q, None)) as (s, t):
        ctx.call(name, t.src.ptr, t.tmp.ptr, *args).Complete()
        bits(t.src.ToArray((res, res)), want, what)
        s.check()


def _rw(nj, ctx, name, res, a, p, q, *args, what=None, want=None, cmp=bits):
    n = res * res
    with carved(ctx, res, read=(n, p, a), write=(n, q, None)) as (s, t):
        pair = nj._native.RWTile(t.read.ptr, t.write.ptr, res, 1)
        ctx.call(name, C.byref(pair), *args).Complete()
        assert {pair.read, pair.write} == {t.read.ptr, t.write.ptr} and pair.read != pair.write, what
        out = t.read if pair.read == t.read.ptr else t.write
        cmp(out.ToArray((res, res)), want, what)
        s.check()


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("ft", [3, 2, 1, 0, 11, 8])
def test_kernel_filter_stage(nj, ctx, fctx, ft, mode):
    fast = mode == "fast"
    c = fctx if fast else ctx
    counts = (1, 2, 3) if ft == R.SOBEL3_2D else (1, CAP[KSIZE[ft]], CAP[KSIZE[ft]] + 1)
    for res in (300, 301):
        a = _signed(100 + ft, (res, res))
        ref = memo(("filter", ft, res, fast), lambda: R.filter_apply(a, ft, max(counts), fast=fast, record=counts)[1])
        for p, q in (SAME[:2] if fast else PAIRS):
            for it in counts:
                what = "ft=%d x%d %d^2 %s phases %d/%d" % (ft, it, res, mode, p, q)
                _inplace(c, "nz_kernel_filter_stage", res, a, p, q, ft, it, res, what=what, want=ref[it])
                if ft != R.SOBEL3_2D:
                    _rw(nj, c, "nz_kernel_filter_stage_rw", res, a, p, q, ft, it, what=what + " rw", want=ref[it])
    # Sobel3_2D has no READ / WRITE form: refused by name before any launch, nothing written
    if ft == R.SOBEL3_2D:
        n = 300 * 300
        with carved(c, 300, read=(n, 1, a[:300, :300]), write=(n, 2, None)) as (s, t):
            pair = nj._native.RWTile(t.read.ptr, t.write.ptr, 300, 1)
            with pytest.raises(nj.NoizeError):
                c.call("nz_kernel_filter_stage_rw", C.byref(pair), ft, 1)
            c.synchronize()
            assert is_canary(t.write.ToArray()).all()
            bits(t.read.ToArray(), np.ascontiguousarray(a[:300, :300]).reshape(-1), "refused: read plane unchanged")
            s.check()


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("kind,width", [("gauss", 4), ("gauss", 13), ("gauss", 25), ("smooth", 7), ("series", 5)])
def test_blur_stages_and_series(nj, ctx, fctx, kind, width, mode):
    fast = mode == "fast"
    c = fctx if fast else ctx
    sigma = width % 16
    for res, it in ((300, 2), (301, 1)):
        a = _signed(width * 1000 + res, (res, res))
        if kind == "series":       # one asymmetric 5-tap kernel, one application
            kx = np.array([0.1, -0.3, 0.5, 0.2, 0.7], f32)
            kz = np.array([-1.0, 0.25, 0.5, 0.125, 2.0], f32)
            fac, it = f32(0.37), 1
            name = "nz_separable_series"
            args = (res, 5, kx.ctypes.data_as(nj._native.f32p), kz.ctypes.data_as(nj._native.f32p), 0.37)
        else:
            kx, kz, fac = R.blur_taps(kind, width, sigma)
            name = "nz_gauss_blur_stage" if kind == "gauss" else "nz_smooth_blur_stage"
            args = (width, sigma, it, res) if kind == "gauss" else (width, it, res)
        want = memo(("blur", kind, width, res, fast), lambda: R.separable(a, kx, kz, fac, it, ksize=width, fast=fast))
        for p, q in (SAME[:2] if fast else PAIRS):
            _inplace(c, name, res, a, p, q, *args, what="%s %d x%d %d^2 %s phases %d/%d" % (kind, width, it, res, mode, p, q),
                     want=want)


# ---- min erosion -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [256, 257])
def test_erosion_stage(nj, ctx, oracle, res):
    assert nj._native.lib.nz_erosion_max_fused_iterations() == 8   # 8 | 9 is the threshold the counts cross
    a = np.random.default_rng(res).random((res, res), dtype=f32)
    for it in (1, 8, 9):
        want = memo(("erosion", res, it), lambda: oracle.erosion_min(a, it))
        for p, q in PAIRS:
            what = ("erosion", res, it, p, q)
            n = res * res
            with carved(ctx, res, src=(n, p, a), tmp=(n, q, None)) as (s, t):
                ctx.call("nz_erosion_stage", t.src.ptr, t.tmp.ptr, it, res).Complete()
                same(t.src.ToArray((res, res)), want, what)
                s.check()
            _rw(nj, ctx, "nz_erosion_stage_rw", res, a, p, q, it, what=what + ("rw",), want=want, cmp=same)


# ---- flow map ----------------------------------------------------------------------------------------------------------------
def _terrain(oracle, res):
    return memo(("terrain", res), lambda: oracle.kernel_filter(
        oracle.fractal(oracle.SIMPLEX, res, res, 0.4, 1.0, 2.0, 0.0, 8, 0, 0, 170), oracle.GAUSS5_S1, 2))


@pytest.mark.parametrize("res", [128, 384, 257])
def test_flowmap_stage(nj, ctx, oracle, res):
    lib = nj._native.lib
    assert lib.nz_flow_fused_max_iterations() == 5   # 5: one launch, the state planes stay as they are; 6: two launches
    h = _terrain(oracle, res)
    n = res * res
    nwork, nwork_rw = lib.nz_flowmap_stage_work_floats(res), lib.nz_flowmap_stage_rw_work_floats(res, 1)
    assert nwork == 11 * n and nwork_rw == 10 * n
    for it in (1, 5, 6):
        want = memo(("flow", res, it), lambda: oracle.flowmap(h, it, 0.0, 0.005))
        for p, q in PAIRS:
            what = ("flowmap", res, it, p, q)
            with carved(ctx, res, src=(n, p, h), work=(nwork, q, None)) as (s, t):
                ctx.call("nz_flowmap_stage", t.src.ptr, t.work.ptr, it, 0.0, 0.005, res).Complete()
                same(t.src.ToArray((res, res)), want, what)
                if it <= 5:  # {water, fN, fS, fE, fW} x {READ, WRITE}: never touched by a single launch
                    assert is_canary(t.work.ToArray()[:10 * n]).all(), what
                s.check()
            with carved(ctx, res, read=(n, p, h), write=(n, q, None), work=(nwork_rw, third(p, q), None)) as (s, t):
                pair = nj._native.RWTile(t.read.ptr, t.write.ptr, res, 1)
                ctx.call("nz_flowmap_stage_rw", C.byref(pair), t.work.ptr, it, 0.0, 0.005).Complete()
                assert (pair.read, pair.write) == (t.write.ptr, t.read.ptr), what
                same(t.write.ToArray((res, res)), want, what + ("rw",))
                bits(t.read.ToArray((res, res)), h, "rw: the heights are read only")
                if it <= 5:
                    assert is_canary(t.work.ToArray()).all(), what
                s.check()


@pytest.mark.parametrize("res", [128, 257])
def test_flow_delegates(nj, ctx, oracle, res):
    rng = np.random.default_rng(11 + res)
    h = rng.random((res, res), dtype=f32)
    w = (rng.random((res, res), dtype=f32) * f32(0.01)).astype(f32)
    fl = [(rng.random((res, res), dtype=f32) * f32(0.02)).astype(f32) for _ in range(4)]  # N, S, E, W
    step = oracle.flow_step(h, w, *fl)
    water = oracle.water_step(w, *step)
    vel = oracle.velocity(*step)
    args = np.array([0.0, 0.005, 0.005], f32)
    normed = oracle.normalize(vel, 0.0, 0.005)
    n = res * res
    for p, q in PAIRS:
        ph = [p, q] + [third(p, q, k) for k in (1, 2, 3, 0)]
        planes = dict(h=(n, ph[0], h), w=(n, ph[1], w))
        for k, name in enumerate("NSEW"):
            planes["f" + name] = (n, ph[2 + k], fl[k])
            planes["b" + name] = (n, ph[5 - k], None)
        planes["bw"] = (n, ph[2], None)
        with carved(ctx, res, **planes) as (s, t):
            what = ("flow delegates", res, p, q)
            ctx.call("nz_flowmap_compute_flow", t.h.ptr, t.w.ptr, t.fN.ptr, t.bN.ptr, t.fS.ptr, t.bS.ptr, t.fE.ptr, t.bE.ptr,
                     t.fW.ptr, t.bW.ptr, res).Complete()
            for name, wv in zip("NSEW", step):
                same(getattr(t, "f" + name).ToArray((res, res)), wv, what + ("flux " + name,))
            s.check()
            ctx.call("nz_flowmap_update_water", t.w.ptr, t.bw.ptr, t.fN.ptr, t.fS.ptr, t.fE.ptr, t.fW.ptr, res).Complete()
            same(t.w.ToArray((res, res)), water, what + ("water",))
            s.check()
            ctx.call("nz_flowmap_write_values", t.h.ptr, t.fN.ptr, t.fS.ptr, t.fE.ptr, t.fW.ptr, res).Complete()
            same(t.h.ToArray((res, res)), vel, what + ("velocity",))
            s.check()
            ctx.call("nz_map_normalize_values", t.h.ptr, t.bN.ptr, args.ctypes.data_as(nj._native.f32p), res).Complete()
            same(t.h.ToArray((res, res)), normed, what + ("normalise",))
            for name in ("bN", "bS", "bE", "bW", "bw"):   # the __buff planes: the updates are done in place
                assert is_canary(getattr(t, name).ToArray()).all(), what + (name,)
            s.check()


def test_flow_fused_stripe(nj, ctx, oracle):
    """A first-only launch, then a last-only one that reads what it wrote: a 130 x 97 stripe (an odd row length: every row
    starts at another phase), the height, the five state planes and the result each at a phase of their own."""
    rows, cols, n1, n2 = 130, 97, 3, 2
    h = F.terrain(np.random.default_rng(97), rows, cols)
    state = memo(("flow stripe state",), lambda: np.stack(F.launch(h, n1, True, False)))
    want = memo(("flow stripe",), lambda: F.launch(h, n2, False, True, list(state)))
    assert oracle.flowmap(h, n1 + n2, *F.NORM).tobytes() == want.tobytes()
    n = rows * cols
    st = nj.Stripe(cols, rows, 0, rows, 0, rows, 0)
    for p, q in PAIRS:
        planes = dict(h=(n, p, h), dst=(n, q, None))
        for k in range(5):
            planes["s%d" % k] = (n, third(p, q, k), None)
        with carved(ctx, cols, **planes) as (s, t):
            what = ("flow stripe", p, q)
            ptrs = (nj._native.dev_ptr * 5)(*[getattr(t, "s%d" % k).ptr for k in range(5)])
            ctx.call("nz_flow_fused_stripe", t.h.ptr, None, ptrs, None, C.byref(st), n1, 1, 0, *F.NORM).Complete()
            for k in range(5):
                bits(getattr(t, "s%d" % k).ToArray((rows, cols)), state[k], what + ("state plane", k))
            assert is_canary(t.dst.ToArray()).all(), what
            s.check()
            ctx.call("nz_flow_fused_stripe", t.h.ptr, ptrs, None, t.dst.ptr, C.byref(st), n2, 0, 1, *F.NORM).Complete()
            bits(t.dst.ToArray((rows, cols)), want, what + ("result",))
            for k in range(5):
                bits(getattr(t, "s%d" % k).ToArray((rows, cols)), state[k], what + ("state plane is read only", k))
            bits(t.h.ToArray((rows, cols)), h, "the heights are read only")
            s.check()


# ---- hydraulic erosion -------------------------------------------------------------------------------------------------------
def _relief(res):
    from test_hydraulic_ref import relief
    x = np.arange(res, dtype=f32)
    return memo(("relief", res), lambda: (relief(res, 300) + (x[None, :] * f32(0.004) + x[:, None] * f32(0.001))).astype(f32))


@pytest.mark.parametrize("res", [64, 97])
def test_hydraulic_erosion_stage(nj, ctx, oracle, res):
    import hydraulic_ref as H
    from test_hydraulic_ref import NAMES, PARAMS
    h, prm, n = _relief(res), PARAMS[0], res * res
    nwork = nj._native.lib.nz_hydraulic_erosion_work_floats(res, 1)
    for its in (1, 7):
        want, wwater = memo(("hydraulic", res, its), lambda: H.run(h, its, **dict(zip(NAMES, prm))))
        for p, q in PAIRS:
            with carved(ctx, res, src=(n, p, h), work=(nwork, q, None)) as (s, t):
                ctx.call("nz_hydraulic_erosion_stage", t.src.ptr, t.work.ptr, its, *prm, res).Complete()
                bits(t.src.ToArray((res, res)), want, ("hydraulic", res, its, p, q))
                bits(t.work.ToArray()[:n].reshape(res, res), wwater, ("hydraulic water", res, its, p, q))
                s.check()


@pytest.mark.parametrize("res", [64, 97])
def test_hydraulic_erosion_ex(nj, ctx, oracle, res):
    import hydraulic_ex_ref as X
    from test_gpu_hydraulic_ex import maps_for
    from test_hydraulic_ref import NAMES, PARAMS
    h, prm, n = _relief(res), PARAMS[0], res * res
    rain, hard = maps_for(h.shape, 11)
    nwork = nj._native.lib.nz_hydraulic_erosion_work_floats(res, 1)
    for its in (1, 7):
        want = memo(("hydraulic ex", res, its),
                    lambda: X.run(h, its, border=X.OPEN, rainMap=rain, hardness=hard, **dict(zip(NAMES, prm))))
        for p, q in PAIRS:
            ph = [p] * 5 if p == q else [q, (q + 1) % 4, (q + 2) % 4, (q + 3) % 4, (p + 2) % 4]
            with carved(ctx, res, src=(n, p, h), work=(nwork, ph[0], None), rainMap=(n, ph[1], rain), hardness=(n, ph[2], hard),
                        wear=(n, ph[3], None), deposits=(n, ph[4], None)) as (s, t):
                desc = nj._native.HydraulicDesc(its, *prm, X.OPEN, t.rainMap.ptr, t.hardness.ptr, t.wear.ptr, t.deposits.ptr)
                ctx.call("nz_hydraulic_erosion_ex", t.src.ptr, t.work.ptr, C.byref(desc), res).Complete()
                got = (t.src.ToArray((res, res)), t.work.ToArray()[:n].reshape(res, res), t.wear.ToArray((res, res)),
                       t.deposits.ToArray((res, res)))
                for name, g, w in zip(("result", "water", "wear", "deposits"), got, want):
                    bits(g, w, ("hydraulic ex", name, res, its, p, q))
                bits(t.rainMap.ToArray((res, res)), rain, "the rain map is read only")
                bits(t.hardness.ToArray((res, res)), hard, "the hardness map is read only")
                s.check()


# ---- noise -----------------------------------------------------------------------------------------------------------------
NOISE = (0.4, 1.0, 2.0, 0.0, 4, 37, -11, 300)   # hurst, amp, stepdown, detune, octaves, xpos, zpos, noiseSize
WARP = (37.5, 1.0, 3)


@pytest.mark.parametrize("basis", [1, 3, 5], ids=["Perlin", "Simplex", "Cellular"])
@pytest.mark.parametrize("res", [64, 100])
def test_fractal_entries(ctx, oracle, res, basis):
    from fractal_shapes_ref import RIDGED, fractal_shaped
    from fractal_warp_ref import fractal_warped
    cases = [("nz_fractal", (), lambda: oracle.fractal(basis, res, res, *NOISE[:4], NOISE[4], *NOISE[5:])),
             ("nz_fractal_shaped", (RIDGED, 1.0, 2.0), lambda: fractal_shaped(basis, res, res, *NOISE, shape=RIDGED)),
             ("nz_fractal_warped", (RIDGED, 1.0, 2.0) + WARP,
              lambda: fractal_warped(basis, res, res, *NOISE, shape=RIDGED, warp_strength=WARP[0], warp_scale=WARP[1],
                                     warp_octaves=WARP[2]))]
    for name, extra, ref in cases:
        want = memo((name, basis, res), ref)
        for p in range(4):
            with carved(ctx, res, src=(res * res, p, None)) as (s, t):
                ctx.call(name, basis, t.src.ptr, res, *NOISE, *extra).Complete()
                same(t.src.ToArray((res, res)), np.asarray(want, f32), (name, basis, res, p))
                s.check()


# ---- batch entries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [37, 64])
def test_batch_entries(nj, ctx, oracle, res):
    import hydraulic_ref as H
    from test_hydraulic_ref import NAMES, PARAMS
    lib = nj._native.lib
    count, n = 3, res * res
    pos = np.array([(120, -45), (-3000, 77), (9, 4000)], np.int32)
    a = np.random.default_rng(res).random((count, res, res), dtype=f32)
    hh = np.stack([_relief(res) * f32(k + 1) for k in range(count)]).astype(f32)
    want_noise = memo(("bnoise", res), lambda: np.stack(
        [oracle.fractal(3, res, res, 0.5, 1.0, 2.0, 0.0, 4, int(x), int(z), 50) for x, z in pos]))
    want_filter = memo(("bfilter", res), lambda: np.stack([oracle.kernel_filter(a[k], 2, 7) for k in range(count)]))
    want_erosion = memo(("berosion", res), lambda: np.stack([oracle.erosion_min(a[k], 5) for k in range(count)]))
    want_flow = memo(("bflow", res), lambda: np.stack([oracle.flowmap(a[k], 7, -0.1, 0.1) for k in range(count)]))
    want_hyd = memo(("bhyd", res), lambda: [H.run(hh[k], 3, **dict(zip(NAMES, PARAMS[0]))) for k in range(count)])
    nflow, nhyd = count * lib.nz_flowmap_stage_work_floats(res), lib.nz_hydraulic_erosion_work_floats(res, count)
    for p, q in PAIRS:
        what = (res, p, q)
        # the guard behind `data` starts directly after the LAST tile: check() sees a store past it
        with carved(ctx, res, data=(count * n, p, None), positions=(2 * count, q, pos, np.int32)) as (s, t):
            ctx.call("nz_fractal_batch", 3, t.data.ptr, res, count, t.positions.ptr, 0.5, 1.0, 2.0, 0.0, 4, 50).Complete()
            same(t.data.ToArray((count, res, res)), want_noise, ("fractal batch",) + what)
            s.check()
        with carved(ctx, res, src=(count * n, p, a), tmp=(count * n, q, None)) as (s, t):
            ctx.call("nz_kernel_filter_stage_batch", t.src.ptr, t.tmp.ptr, 2, 7, res, count).Complete()
            bits(t.src.ToArray((count, res, res)), want_filter, ("filter batch",) + what)
            s.check()
        with carved(ctx, res, src=(count * n, p, a), tmp=(count * n, q, None)) as (s, t):
            ctx.call("nz_erosion_stage_batch", t.src.ptr, t.tmp.ptr, 5, res, count).Complete()
            same(t.src.ToArray((count, res, res)), want_erosion, ("erosion batch",) + what)
            s.check()
        with carved(ctx, res, src=(count * n, p, a), work=(nflow, q, None)) as (s, t):
            ctx.call("nz_flowmap_stage_batch", t.src.ptr, t.work.ptr, 7, -0.1, 0.1, res, count).Complete()
            same(t.src.ToArray((count, res, res)), want_flow, ("flow batch",) + what)
            s.check()
        with carved(ctx, res, src=(count * n, p, hh), work=(nhyd, q, None)) as (s, t):
            ctx.call("nz_hydraulic_erosion_stage_batch", t.src.ptr, t.work.ptr, 3, *PARAMS[0], res, count).Complete()
            got, water = t.src.ToArray((count, res, res)), t.work.ToArray()[:count * n].reshape(count, res, res)
            for k in range(count):
                bits(got[k], want_hyd[k][0], ("hydraulic batch", k) + what)
                bits(water[k], want_hyd[k][1], ("hydraulic batch water", k) + what)
            s.check()


def test_single_tile_stages_on_a_tile_of_a_batch(nj, ctx, oracle):
    """The product path: GeneratorDataBatch hands out tile k as data.offset(k * n, n); with res 37 tile 1 lies 4 bytes past
    the phase of the batch, and goes through single-tile stages."""
    res, count = 37, 3
    n = res * res
    a = np.random.default_rng(37).random((count, res, res), dtype=f32)
    lut = np.array([1.0 - f32(i) / f32(256) for i in range(256)], f32)
    want_f, want_c = oracle.kernel_filter(a[1], 2, 7), oracle.curve(a[1], lut)
    for p, q in PAIRS:
        for name in ("filter", "curve"):
            with carved(ctx, res, data=(count * n, p, a), tmp=(n, q, None), curve=(256, q, lut)) as (s, t):
                batch = nj.GeneratorDataBatch("b", t.data, res, None, count)
                tile = batch.tile(1)
                assert tile.ptr == t.data.ptr + 4 * n and tile.ptr % 16 == (4 * p + 4 * n) % 16
                if name == "filter":
                    ctx.call("nz_kernel_filter_stage", tile.ptr, t.tmp.ptr, 2, 7, res).Complete()
                    bits(tile.ToArray((res, res)), want_f, ("filter on tile 1", p, q))
                else:
                    ctx.call("nz_curve_job", tile.ptr, t.tmp.ptr, t.curve.ptr, 256, res).Complete()
                    same(tile.ToArray((res, res)), want_c, ("curve on tile 1", p, q))
                got = t.data.ToArray((count, res, res))
                bits(got[0], a[0], "tile 0 is not the stage's")
                bits(got[2], a[2], "tile 2 is not the stage's")
                s.check()


# ---- mesh ------------------------------------------------------------------------------------------------------------------
MESHES = [(1, 64, 72, 4), (0, 33, 35, 1), (1, 127, 131, 2)]   # type, res, in_res, margin


@pytest.mark.parametrize("mesh_type,res,in_res,margin", MESHES)
def test_heightmap_mesh(nj, ctx, oracle, mesh_type, res, in_res, margin):
    lib = nj._native.lib
    h = np.random.default_rng(res).random((in_res, in_res), dtype=f32)
    nv, ni = lib.nz_mesh_vertex_count(res), lib.nz_mesh_index_count(res)
    assert (nv, ni) == ((res + 1) ** 2, 6 * res * res)
    wv, wi = oracle.mesh_heightmap(mesh_type, h, res, margin, 50.0, 100.0)
    for hp in range(4):          # the guards around the height plane: mesh_h stays inside it for this margin
        for ip in range(4):
            with carved(ctx, in_res, heights=(in_res * in_res, hp, h), vtx=(nv * 12, 0, None),
                        idx=(ni, ip, None, np.uint32)) as (s, t):
                ctx.call("nz_heightmap_mesh", mesh_type, t.vtx.ptr, t.idx.ptr, res, in_res, margin, 50.0, 100.0,
                         t.heights.ptr).Complete()
                assert np.array_equal(t.idx.ToArray(), wi), (res, hp, ip)
                same(t.vtx.ToArray().reshape(-1, 12), wv, ("vertices", res, hp, ip))
                s.check()
        for bp in (2 * hp, 2 * hp + 8):   # the 16-bit stream in 2-byte steps: all eight over the four height phases
            with carved(ctx, in_res, heights=(in_res * in_res, hp, h), vtx=(nv * 12, 0, None),
                        idx=(ni, None, None, np.uint16, bp)) as (s, t):
                ctx.call("nz_heightmap_mesh16", mesh_type, t.vtx.ptr, t.idx.ptr, res, in_res, margin, 50.0, 100.0,
                         t.heights.ptr).Complete()
                assert np.array_equal(t.idx.ToArray(), wi.astype(np.uint16)), (res, hp, bp)
                same(t.vtx.ToArray().reshape(-1, 12), wv, ("vertices 16", res, hp, bp))
                s.check()


@pytest.mark.parametrize("res", [64, 33, 127])
def test_square_grid_mesh(nj, ctx, oracle, res):
    nv, ni = (res + 1) ** 2, 6 * res * res
    wv, wi = oracle.mesh_square_grid(res)
    for ip in range(4):
        with carved(ctx, res, vtx=(nv * 12, 0, None), idx=(ni, ip, None, np.uint32)) as (s, t):
            ctx.call("nz_square_grid_mesh", t.vtx.ptr, t.idx.ptr, res).Complete()
            assert np.array_equal(t.idx.ToArray(), wi), (res, ip)
            same(t.vtx.ToArray().reshape(-1, 12), wv, ("planar vertices", res, ip))
            s.check()


@pytest.mark.parametrize("vp", [1, 2, 3])
def test_a_vertex_stream_off_16_bytes_is_refused_by_name(nj, ctx, vp):
    mesh_type, res, in_res, margin = MESHES[0]
    h = np.random.default_rng(1).random((in_res, in_res), dtype=f32)
    nv, ni = (res + 1) ** 2, 6 * res * res
    calls = [("nz_heightmap_mesh", np.uint32, lambda t: (mesh_type, t.vtx.ptr, t.idx.ptr, res, in_res, margin, 50.0, 100.0,
                                                         t.heights.ptr)),
             ("nz_heightmap_mesh16", np.uint16, lambda t: (mesh_type, t.vtx.ptr, t.idx.ptr, res, in_res, margin, 50.0, 100.0,
                                                           t.heights.ptr)),
             ("nz_square_grid_mesh", np.uint32, lambda t: (t.vtx.ptr, t.idx.ptr, res))]
    for name, itype, args in calls:
        with carved(ctx, in_res, heights=(in_res * in_res, 0, h), vtx=(nv * 12, vp, None), idx=(ni, 0, None, itype)) as (s, t):
            with pytest.raises(nj.NoizeError) as e:
                ctx.call(name, *args(t))
            assert e.value.status == nj._native.NZ_ERR_INVALID and "vertex buffer" in str(e.value), (name, str(e.value))
            ctx.synchronize()
            assert is_canary(t.vtx.ToArray()).all(), name            # nothing was written
            raw = t.idx.ToArray()
            assert is_canary(raw.view(np.uint32)).all(), name
            s.check()


# ---- live grid jobs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,cover", [(66, 1.0), (257, 1.0), (257, 0.03)])
def test_pool_automata(ctx, oracle, res, cover):
    rng = np.random.default_rng(res + int(cover * 100))   # inputs of test_pool_automata_runs_match_the_row_walk
    height = (rng.random((res, res), dtype=f32) * f32(0.2)).astype(f32)
    wet = rng.random((res, res)) < cover
    pool = np.where(wet, f32(0.002) + rng.random((res, res), dtype=f32) * f32(0.3), 0).astype(f32)
    pool[rng.random((res, res)) < 0.1] = f32(0.0005)
    pool[:, res // 2] = f32(0.25)
    pool[res // 3, :] = f32(0.25)
    want = oracle.pool_automata(pool, height, 2)
    n = res * res
    for p, q in PAIRS:
        with carved(ctx, res, pool=(n, p, pool), height=(n, q, height)) as (s, t):
            ctx.call("nz_pool_automata", t.pool.ptr, t.height.ptr, 2, res).Complete()
            same(t.pool.ToArray((res, res)), want, ("pool automata", res, cover, p, q))
            bits(t.height.ToArray((res, res)), height, "the heights are read only")
            s.check()


def test_control_textures_at_every_byte_offset(nj, ctx, oracle):
    """nz_set_rgba32 / nz_curviture_map store single bytes: a texture may start at any byte; the sizes are those of
    test_config4_live_erosion_equals_oracle (512^2 planes, a 496^2 texture)."""
    res, th = 512, 1000
    mres = res - 16
    tm = nj.tile_set_meta(res, height=th, tile_size=2000, tile_res=mres, margin=8)
    rng = np.random.default_rng(4)
    src = (rng.random((res, res), dtype=f32) * f32(1.5) - f32(0.25)).astype(f32)   # below 0 and above 1 after the scale
    height = oracle.fractal(oracle.CELLULAR, res, res, 0.4, 1.0, 2.0, 0.0, 6, 0, 0, 300)
    init = rng.integers(0, 256, (mres, mres, 4), dtype=np.uint8)
    sets = [(scale, ch, oracle.set_rgba32(src, mres, scale, ch, texture=init.copy())) for scale, ch in ((1.0, 3), (2.0, 2), (0.5, 0))]
    cur = oracle.curviture_map(height, mres, th, float(tm.PATCH_RES[0]), 1, texture=init.copy())
    for bp in range(4):
        for p in range(4):
            with carved(ctx, res, src=(res * res, p, src), texture=(mres * mres * 4, None, init, np.uint8, bp)) as (s, t):
                for scale, ch, want in sets:
                    ctx.call("nz_set_rgba32", t.src.ptr, t.texture.ptr, ch, res, mres, scale).Complete()
                    got = t.texture.ToArray((mres, mres, 4))
                    assert np.array_equal(got[..., ch], want[..., ch]), ("set_rgba32", bp, p, ch)
                    s.check()
                assert np.array_equal(got[..., 1], init[..., 1]), ("set_rgba32: the channel nobody set", bp, p)
            with carved(ctx, res, height=(res * res, p, height), texture=(mres * mres * 4, None, init, np.uint8, bp)) as (s, t):
                ctx.call("nz_curviture_map", t.texture.ptr, t.height.ptr, C.byref(tm), 1, res, mres).Complete()
                got = t.texture.ToArray((mres, mres, 4))
                # powf / logf of the device: one byte step at most (as the existing test)
                assert np.abs(got[..., 1].astype(int) - cur[..., 1].astype(int)).max() <= 1, ("curviture", bp, p)
                assert np.array_equal(got[..., [0, 2, 3]], init[..., [0, 2, 3]]), ("curviture: other channels", bp, p)
                s.check()
