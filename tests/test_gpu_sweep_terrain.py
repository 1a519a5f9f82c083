"""Five families of terrain stages -- hydraulic erosion plain and _ex, fluvial erosion, depression filling, drainage area --
on the adversarial tiles of tests/terrain_tiles.py, every plane bit for bit against the numpy models (hydraulic_ref,
hydraulic_ex_ref, fluvial_ref, fill_ref.flood, drainage_ref.accumulate):

    a. odd widths     sizes with two and three live cells in a row's last quad and sizes astride one 16-row tile edge, the
                      forms of each family, batches whose tiles start 4 and 8 bytes off the vector alignment (the donor
                      bytes of the drainage stage then 1 and 2 bytes off their word), guarded slabs
    b. ties           terraces, cones, pits and the checkerboard, sea levels and epsilons that land on cell values
    c. scales         heights in metres, negative, subnormal differences, signed zeros
    d. winding fill   the serpentine: tiles that go quiet and wake up, at three sweep caps and inside a batch
       a chain        fill -> drainage area on the tie tiles, and the fluvial stage's drainage plane against the drainage
                      stage's, kernel against kernel: with epsilon 0 the lakes are flats without receivers
    e. seeded sweep   size, generator, family, form and parameters drawn from a seed; the drainage family draws from a
                      stream of its own (drainage_sweep_cases), the stream of the four older ones is pinned by
                      tests/test_sweep_terrain_cases.py

The drainage family has the tile entry ("inplace") and the batch, no _rw form; its parameters are rain, sea, a rain map
(on = ("rainMap",)) that is positive or, with `signed`, of both signs; its run also has to report converged within
"cells of the longest flow path" + 1 passes.  The four stripe entries on the same tiles: tests/test_gpu_sweep_stripes.py.

tests/test_terrain_tiles.py shows on the CPU that the tiles are what b, c and d take them for.  A case is a dict (family,
form, hh = count x res x res heights, parameters); model(case) and gpu(nj, ctx, case) give its planes.  A case of the sweep
is replayed alone with check(nj, ctx, sweep_cases(seed)[i]) or check(nj, ctx, drainage_sweep_cases(seed)[i])."""
import ctypes as C

import numpy as np
import pytest

import drainage_ref as D
import fill_ref as L
import fluvial_ref as F
import hydraulic_ex_ref as X
import hydraulic_ref as H
import terrain_tiles as T
import test_gpu_drainage as GD
import test_gpu_fill as GL
import test_gpu_fluvial as GF
import test_gpu_hydraulic as GH
import test_gpu_hydraulic_ex as GX
from test_gpu_slab import PAIRS, carved, memo
from test_hydraulic_ref import NAMES, PARAMS

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
FAMILIES = ("hydraulic", "hydraulic_ex", "fluvial", "fill", "drainage")
PLANES = {"hydraulic": ("result", "water"), "hydraulic_ex": ("result", "water", "wear", "deposits"),
          "fluvial": ("result", "drainage"), "fill": ("result", "depth"), "drainage": ("drainage",)}
ALL_ON = ("open", "rainMap", "hardness", "masks")
ALL_MAPS = ("rainMap", "hardness", "upliftMap", "drainageIn")
SWEEP_SIZES = (5, 7, 16, 19, 30, 34, 62, 63, 66, 70, 95, 127, 129, 131, 194)


# ---- a case, its model and its run on the GPU ---------------------------------------------------------------------------------
def drainage_rain_map(shape, seed, signed=False):
    """The rain map of a drainage case: in [0.25, 1.75) from `seed`, or (signed) the sine of the cell index, both signs, as
    drainage_stripe_cases.signed_rain."""
    if signed:
        return np.sin(np.arange(int(np.prod(shape)), dtype=np.float64)).astype(f32).reshape(shape)
    return (np.random.default_rng(seed).random(shape, dtype=f32) * f32(1.5) + f32(0.25)).astype(f32)


def case(family, hh, form="inplace", its=1, prm=None, on=(), eps=1e-4, sea=OFF, depth=True, budget=GL.GENEROUS, seed=11,
         keys=None, rain=1.0, signed=False):
    """hh: one res x res plane or count of them.  on: the options of the _ex entry (ALL_ON), the planes of the fluvial one
    (ALL_MAPS) or ("rainMap",) of the drainage stage, random maps from `seed`; rain and signed belong to the drainage stage.
    keys: one hashable per tile under which its model is shared between cases."""
    hh = np.ascontiguousarray(hh, f32)
    hh = hh[None] if hh.ndim == 2 else hh
    assert form in ("inplace", "rw", "batch") and (form != "inplace" or len(hh) == 1)
    assert family != "drainage" or (form != "rw" and set(on) <= {"rainMap"} and GD.GENEROUS == GL.GENEROUS)
    c = dict(family=family, hh=hh, form=form, its=its, prm=prm, on=tuple(on), eps=eps, sea=sea, depth=depth, budget=budget,
             seed=seed, keys=keys, rain=rain, signed=bool(signed and "rainMap" in on))
    if family == "drainage":
        c["maps"] = {"rainMap": memo(("terrain rain map", hh.shape, seed, c["signed"]),
                                     lambda: drainage_rain_map(hh.shape, seed, c["signed"]))} if "rainMap" in on else {}
    if family == "hydraulic_ex":
        rain, hard = GX.maps_for(hh.shape, seed)
        c["opts"] = dict(border=X.OPEN if "open" in on else X.CLOSED, rainMap=rain if "rainMap" in on else None,
                         hardness=hard if "hardness" in on else None, masks="masks" in on)
    if family == "fluvial":
        maps = GF.maps_for(hh.shape, seed)
        c["maps"] = {k: maps[k] for k in ALL_MAPS if k in on}
    return c


def describe(c):
    if c["family"] == "drainage":
        return "drainage %s %d x %d^2 rain %r sea %r on %r signed %r seed %d" % (
            c["form"], len(c["hh"]), c["hh"].shape[-1], c["rain"], c["sea"], c["on"], c["signed"], c["seed"])
    return "%s %s %d x %d^2 its %d prm %r on %r eps %g sea %r depth %r" % (
        c["family"], c["form"], len(c["hh"]), c["hh"].shape[-1], c["its"], c["prm"], c["on"], c["eps"], c["sea"], c["depth"])


def _model_tile(c, k):
    fam, h = c["family"], c["hh"][k]
    if fam == "hydraulic":
        return H.run(h, c["its"], **dict(zip(NAMES, c["prm"])))
    if fam == "hydraulic_ex":
        o = c["opts"]
        at = lambda m: m[k] if m is not None else None  # noqa: E731
        return X.run(h, c["its"], border=o["border"], rainMap=at(o["rainMap"]), hardness=at(o["hardness"]),
                     **dict(zip(NAMES, c["prm"])))
    if fam == "fluvial":
        return GF.ref(h, c["its"], c["prm"], **{name: m[k] for name, m in c["maps"].items()})
    if fam == "drainage":
        rm = c["maps"].get("rainMap")
        A, height = D.accumulate(h, c["rain"], c["sea"], rm[k] if rm is not None else None)
        return A, np.int64(height)
    W = L.flood(h, c["eps"], c["sea"])
    return W, (W - h).astype(f32)


def model(c):
    """The planes of PLANES[family], each count x res x res; behind them, for the drainage family, the cells of every tile's
    longest flow path."""
    per_tile = []
    for k in range(len(c["hh"])):
        if c["keys"] is None:
            per_tile.append(_model_tile(c, k))
        else:
            # (the random maps of tile k depend on the shape of the whole case)
            key = ("terrain", c["family"], c["keys"][k], c["hh"].shape, k, c["its"], c["prm"], c["on"], c["eps"], c["sea"],
                   c["seed"], c["rain"], c["signed"])
            per_tile.append(memo(key, lambda: tuple(_model_tile(c, k))))
    return [np.stack(p) for p in zip(*per_tile)]


def gpu(nj, ctx, c):
    fam, hh, form = c["family"], c["hh"], c["form"]
    single = len(hh) == 1 and form != "batch"
    arg = hh[0] if single else hh
    at = (lambda m: m[0] if m is not None else None) if single else (lambda m: m)
    if fam == "hydraulic":
        out = GH.run_gpu(nj, ctx, arg, c["its"], c["prm"], form)
    elif fam == "hydraulic_ex":
        o = c["opts"]
        out = GX.run_ex(nj, ctx, arg, c["its"], c["prm"], o["border"], at(o["rainMap"]), at(o["hardness"]), o["masks"], form)
    elif fam == "fluvial":
        out = GF.run_gpu(nj, ctx, arg, c["its"], c["prm"], form, **{name: at(m) for name, m in c["maps"].items()})
    elif fam == "drainage":
        got, passes, converged = GD.run_gpu(nj, ctx, arg, c["rain"], c["sea"], c["budget"], rm=at(c["maps"].get("rainMap")))
        c["passes"], c["converged"] = passes, converged  # check() holds them against the model's tree height
        out = (got,)
    else:
        got, d, passes, converged = GL.run_gpu(nj, ctx, arg, c["eps"], c["sea"], c["budget"], form, c["depth"])
        assert converged == 1 and 1 <= passes <= c["budget"], (describe(c), passes, converged)
        c["passes"] = passes
        out = (got, d)
    return [g.reshape(hh.shape) if g is not None else None for g in out]


def check(nj, ctx, c, what=""):
    want, got = model(c), gpu(nj, ctx, c)
    what = what or describe(c)
    for name, g, w in zip(PLANES[c["family"]], got, want):
        # the models never leave the finite numbers on these inputs: a NaN's payload would be the host's, not the model's
        assert np.isfinite(w).all(), "%s: the model's %s is not finite" % (what, name)
        if g is None:
            assert (c["family"] == "fill" and not c["depth"]) or (c["family"] == "hydraulic_ex" and "masks" not in c["on"])
            continue
        GL.assert_bits(g, w, "%s: %s" % (what, name))
    if c["family"] == "drainage":
        height = int(want[1].max())  # the status words cover the whole batch
        assert c["converged"] == 1 and 2 <= c["passes"] <= height + 1, (what, c["passes"], c["converged"], height)
    return got


def tile(name, res, seed=3):
    return memo(("terrain tile", name, res, seed), lambda: T.GENERATORS[name](res, np.random.default_rng(seed)))


# ---- a. odd widths ---------------------------------------------------------------------------------------------------------------
def odd_cases(res):
    a, b = tile("terraces16", res), tile("noisy", res)
    batch = np.stack([a, b, memo(("terrain tile", "noisy T", res), lambda: np.ascontiguousarray(b.T))])
    keys = ["terraces16", "noisy", "noisy T"]
    out = []
    for its in (1, 7):
        for fam, kw in (("hydraulic", dict(prm=PARAMS[1])), ("hydraulic_ex", dict(prm=PARAMS[0], on=ALL_ON)),
                        ("fluvial", dict(prm=GF.PARAMS[0], on=ALL_MAPS)), ("fill", dict(eps=1e-4, depth=True))):
            if fam == "fill" and its > 1:
                continue
            for k in (0, 1):
                for form in ("inplace", "rw"):
                    out.append(case(fam, batch[k], form, its, keys=keys[k:k + 1], **kw))
            out.append(case(fam, batch, "batch", its, keys=keys, **kw))
    # the drainage stage: unit rain, and a sea level that is a terrace with fractional rain on a map
    for kw in (dict(), dict(rain=0.75, sea=T.sea_at(a, 0.3), on=("rainMap",))):
        for k in (0, 1):
            out.append(case("drainage", batch[k], keys=keys[k:k + 1], **kw))
        out.append(case("drainage", batch, "batch", keys=keys, **kw))
    return out


@pytest.mark.parametrize("res", [66, 67, 130, 131, 15, 18, 31, 33, 47])
def test_odd_widths(nj, ctx, oracle, res):
    if res in (67, 131):  # tiles 1 and 2 of a batch start one and two floats past a 16-byte boundary
        probe = ctx.alloc(4)
        assert probe.ptr % 16 == 0 and [(k * res * res) % 4 for k in range(3)] == [0, 1, 2]
        probe.Dispose()
    for c in odd_cases(res):
        check(nj, ctx, c)


@pytest.mark.parametrize("res", [66, 67])
def test_odd_widths_on_slab_carved_planes(nj, ctx, oracle, res):
    """A tail that stores one cell too many lands in a guard: every family at the four alignments and three mixed pairs."""
    h, n, N = tile("terraces16", res), res * res, nj._native
    its, keys = 3, ["terraces16"]
    plane = lambda t: t.ToArray((res, res))  # noqa: E731
    want = {fam: [w[0] for w in model(case(fam, h, its=its, keys=keys, **kw))] for fam, kw in (
        ("hydraulic", dict(prm=PARAMS[0])), ("hydraulic_ex", dict(prm=PARAMS[0], on=ALL_ON)),
        ("fluvial", dict(prm=GF.PARAMS[0], on=ALL_MAPS)), ("fill", dict()))}
    dcase = case("drainage", h, rain=0.75, sea=T.sea_at(h, 0.3), on=("rainMap",), keys=keys)
    want["drainage"], drain = [model(dcase)[0][0]], dcase["maps"]["rainMap"]
    rain, hard = GX.maps_for((1, res, res), 11)
    maps = GF.maps_for((1, res, res), 11)
    nhyd, nflu = N.lib.nz_hydraulic_erosion_work_floats(res, 1), N.lib.nz_fluvial_erosion_work_floats(res, 1)
    nfill, ndrain = N.lib.nz_fill_depressions_work_floats(res, 1), N.lib.nz_drainage_area_work_floats(res, 1)
    for p, q in PAIRS:
        what = (res, p, q)
        ph = [p] * 5 if p == q else [q, (q + 1) % 4, (q + 2) % 4, (q + 3) % 4, (p + 2) % 4]
        with carved(ctx, res, src=(n, p, h), work=(nhyd, q, None)) as (s, t):
            ctx.call("nz_hydraulic_erosion_stage", t.src.ptr, t.work.ptr, its, *PARAMS[0], res).Complete()
            for name, g, w in zip(PLANES["hydraulic"], (plane(t.src), t.work.ToArray()[:n].reshape(res, res)), want["hydraulic"]):
                GL.assert_bits(g, w, ("hydraulic", name) + what)
            s.check()
        with carved(ctx, res, src=(n, p, h), work=(nhyd, ph[0], None), rainMap=(n, ph[1], rain), hardness=(n, ph[2], hard),
                    wear=(n, ph[3], None), deposits=(n, ph[4], None)) as (s, t):
            desc = N.HydraulicDesc(its, *PARAMS[0], X.OPEN, t.rainMap.ptr, t.hardness.ptr, t.wear.ptr, t.deposits.ptr)
            ctx.call("nz_hydraulic_erosion_ex", t.src.ptr, t.work.ptr, C.byref(desc), res).Complete()
            got = (plane(t.src), t.work.ToArray()[:n].reshape(res, res), plane(t.wear), plane(t.deposits))
            for name, g, w in zip(PLANES["hydraulic_ex"], got, want["hydraulic_ex"]):
                GL.assert_bits(g, w, ("hydraulic ex", name) + what)
            s.check()
        with carved(ctx, res, src=(n, p, h), other=(n, q, None), work=(nflu, ph[0], None), rainMap=(n, ph[1], maps["rainMap"]),
                    hardness=(n, ph[2], maps["hardness"]), upliftMap=(n, ph[3], maps["upliftMap"]),
                    drainageIn=(n, ph[4], maps["drainageIn"])) as (s, t):
            desc = GF.desc_of(nj, its, GF.PARAMS[0], t.rainMap, t.hardness, t.upliftMap, t.drainageIn)
            rw = N.RWTile(t.src.ptr, t.other.ptr, res, 1)
            ctx.call("nz_fluvial_erosion_rw", C.byref(rw), t.work.ptr, C.byref(desc)).Complete()
            out = t.src if rw.read == t.src.ptr else t.other
            for name, g, w in zip(PLANES["fluvial"], (plane(out), t.work.ToArray()[:n].reshape(res, res)), want["fluvial"]):
                GL.assert_bits(g, w, ("fluvial", name) + what)
            s.check()
        with carved(ctx, res, src=(n, p, h), work=(nfill, q, None), depth=(n, ph[1], None)) as (s, t):
            desc = GL.desc_of(nj, 1e-4, OFF, GL.GENEROUS, t.depth)
            ctx.call("nz_fill_depressions", t.src.ptr, t.work.ptr, C.byref(desc), res).Complete()
            assert ctx.wrap(t.work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
            for name, g, w in zip(PLANES["fill"], (plane(t.src), plane(t.depth)), want["fill"]):
                GL.assert_bits(g, w, ("fill", name) + what)
            s.check()
        with carved(ctx, res, src=(n, p, h), drainage=(n, q, None), work=(ndrain, ph[0], None),
                    rainMap=(n, ph[1], drain)) as (s, t):
            desc = GD.desc_of(nj, dcase["rain"], dcase["sea"], GD.GENEROUS, t.rainMap)
            ctx.call("nz_drainage_area", t.src.ptr, t.drainage.ptr, t.work.ptr, C.byref(desc), res).Complete()
            assert ctx.wrap(t.work.ptr, 2, dtype=np.int32).ToArray()[1] == 1
            GL.assert_bits(plane(t.drainage), want["drainage"][0], ("drainage", "drainage") + what)
            GL.assert_bits(plane(t.src), h, ("drainage", "heights") + what)
            s.check()


# ---- b. ties ---------------------------------------------------------------------------------------------------------------------
def tie_cases(name, res):
    h = tile(name, res)
    sea = T.sea_at(h, 0.3)
    assert (h == f32(sea)).any() and (h > f32(sea)).any()  # a level of the tile itself: `<=` decides whole plateaus
    keys = [name]
    out = []
    for its in (1, 6):
        for k, prm in enumerate(PARAMS):
            out.append(case("hydraulic", h, ("inplace", "rw", "batch")[k], its, prm, keys=keys))
        for k, prm in enumerate(PARAMS[:2]):
            out.append(case("hydraulic_ex", h, ("rw", "inplace")[k], its, prm, on=ALL_ON, keys=keys))
        for k, prm in enumerate(((0.05, 0.002, 1.0, 1.0, OFF), (0.2, 0.0, 0.5, 0.25, sea), (0.5, 0.01, 2.0, 3.0, sea))):
            out.append(case("fluvial", h, ("inplace", "rw", "batch")[k], its, prm, on=ALL_MAPS if k == 2 else (), keys=keys))
    for eps in (0.0, 1e-4, 0.25):
        for k, s in enumerate((OFF, sea)):
            out.append(case("fill", h, ("inplace", "rw")[k], eps=eps, sea=s, keys=keys))
    return out + drainage_cases(name, res)


def drainage_cases(name, res):
    """Unit rain; a sea level that is a cell value with fractional rain on a positive map; and, as a batch of the tile, the
    tile upside down and the tile transposed, the same with a map of both signs.  The keys (and so the models) are those
    of the stripe sweep, tests/sweep_stripe_cases.py."""
    h = tile(name, res)
    sea = T.sea_at(h, 0.3)
    three = memo(("terrain tile x3", name, res), lambda: np.stack([h, h[::-1], h.T]))
    return [case("drainage", h, keys=[name]),
            case("drainage", h, rain=0.75, sea=sea, on=("rainMap",), keys=[name]),
            case("drainage", three, "batch", rain=0.3, sea=sea, on=("rainMap",), signed=True,
                 keys=[name, name + " upside down", name + " T"])]


def assert_unit_rain(c, A):
    """Every cell's rain arrives at exactly one cell without a receiver, and float32 counts cells exactly."""
    assert c["family"] == "drainage" and c["rain"] == 1.0 and not c["on"]
    for h, a in zip(c["hh"], A):
        n = h.size
        assert (a == np.floor(a)).all() and float(a[F.receivers(h, c["sea"])[0] == F.NONE].astype(np.float64).sum()) == n


@pytest.mark.parametrize("res", [65, 130])
@pytest.mark.parametrize("name", list(T.TIES))
def test_ties(nj, ctx, oracle, name, res):
    for c in tie_cases(name, res):
        got = check(nj, ctx, c, name + " " + describe(c))
        if c["family"] == "drainage" and c["rain"] == 1.0:
            assert_unit_rain(c, got[0])


# ---- c. scales -------------------------------------------------------------------------------------------------------------------
def scale_cases(name, res):
    h = tile(name, res)
    sea = T.sea_at(h, 0.3)
    keys = [name]
    out = []
    for its in (1, 6):
        for k, prm in enumerate(PARAMS):
            out.append(case("hydraulic", h, ("rw", "batch", "inplace")[k], its, prm, keys=keys))
        for k, prm in enumerate(PARAMS[:2]):
            out.append(case("hydraulic_ex", h, ("inplace", "rw")[k], its, prm, on=ALL_ON, keys=keys))
        for k, prm in enumerate(((0.05, 0.002, 1.0, 1.0, OFF), (0.2, 0.0, 0.5, 0.25, sea), (0.5, 0.0, 2.0, 3.0, OFF))):
            out.append(case("fluvial", h, ("rw", "inplace", "batch")[k], its, prm, on=ALL_MAPS if k == 1 else (), keys=keys))
    for eps in (0.0, 1e-4, 1e-2):
        for k, s in enumerate((OFF, sea)):
            out.append(case("fill", h, ("inplace", "rw")[k], eps=eps, sea=s, keys=keys))
    return out + drainage_cases(name, res)


@pytest.mark.parametrize("res", [66, 97])
@pytest.mark.parametrize("name", list(T.SCALES))
def test_scales(nj, ctx, oracle, name, res):
    for c in scale_cases(name, res):
        got = check(nj, ctx, c, name + " " + describe(c))
        if c["family"] == "drainage" and c["rain"] == 1.0:
            assert_unit_rain(c, got[0])
        if name == "metres" and c["family"] == "fill" and c["sea"] == OFF and c["eps"] > 0:
            # include/noize_hip.h: the epsilon can be absorbed by rounding at the tile's magnitudes.  1e-4 is: the lakes stay
            # flats without receivers, more pits than before; 1e-2 is not: no pit is left.  The kernel does as the model does
            pits, want = F.pits(got[0][0]), F.pits(model(c)[0][0])
            assert pits == want and (pits > F.pits(c["hh"][0]) if c["eps"] < 1e-3 else pits == 0), (res, c["eps"], pits, want)


# ---- d. the winding fill ---------------------------------------------------------------------------------------------------------
def test_the_serpentine_fill(nj, ctx):
    h, eps = memo(("terrain serpentine",), T.serpentine_tile), T.SERPENTINE["eps"]
    keys = ["serpentine"]
    first = check(nj, ctx, case("fill", h, eps=eps, budget=2 * T.SERPENTINE_PASSES[16], keys=keys), "serpentine")
    lib = nj._native.lib
    try:
        for sweeps in (1, 3):  # fewer sweeps on chip: more passes, more tiles at rest in each, the same floats
            lib.nz_debug_fill_sweeps(sweeps)
            c = case("fill", h, eps=eps, budget=2 * T.SERPENTINE_PASSES[sweeps], keys=keys)
            got = check(nj, ctx, c, "serpentine with %d sweeps" % sweeps)
            assert c["passes"] > T.SERPENTINE_PASSES[16] // 2
            for name, g, w in zip(PLANES["fill"], got, first):
                GL.assert_bits(g, w, "serpentine with %d sweeps against 16: %s" % (sweeps, name))
    finally:
        lib.nz_debug_fill_sweeps(0)
    # tile 1 of a batch between two tiles that are at rest after a pass or two: the flag bytes of tile 1 lie behind tile 0's
    quiet = tile("checker", h.shape[0])
    c = case("fill", np.stack([quiet, h, quiet]), "batch", eps=eps, budget=2 * T.SERPENTINE_PASSES[16],
             keys=["checker", "serpentine", "checker"])
    got = check(nj, ctx, c, "serpentine inside a batch")
    for name, g, w in zip(PLANES["fill"], got, first):
        GL.assert_bits(g[1], w[0], "serpentine inside a batch against alone: %s" % name)


# ---- d'. a chain on ties: fill -> drainage area, and the fluvial stage's accumulation against it ---------------------------------
@pytest.mark.parametrize("eps", [0.0, 1e-4])
@pytest.mark.parametrize("name", list(T.TIES))
def test_a_chain_on_ties(nj, ctx, name, eps):
    """nz_fill_depressions, then nz_drainage_area on the filled plane, is drainage_ref.accumulate(fill_ref.flood(h, eps)); and
    nz_fluvial_erosion with erodibility 0 and uplift 0 leaves the heights alone and makes one Jacobi step of the same
    accumulation per iteration, so after "cells of the longest flow path" iterations its drainage plane is the drainage
    stage's -- kernel against kernel, through no model (tools/bench_drainage.py relies on it at 1024^2).  With epsilon 0 the
    lakes are flats without receivers."""
    res = 65
    h = tile(name, res)
    filled = check(nj, ctx, case("fill", h, eps=eps, keys=[name]), "%s eps %g: fill" % (name, eps))[0][0]
    c = case("drainage", filled, keys=[(name, "flooded", eps)])
    A = check(nj, ctx, c, "%s eps %g: drainage of the filled plane" % (name, eps))[0][0]
    assert_unit_rain(c, [A])
    height = int(model(c)[1].max())
    got, drainage = GF.run_gpu(nj, ctx, filled, height, (0.0, 0.0, 1.0, 1.0, OFF))
    GL.assert_bits(got, filled, "%s eps %g: heights after %d iterations without erosion" % (name, eps, height))
    GL.assert_bits(drainage, A, "%s eps %g: the fluvial stage's drainage after %d iterations against the drainage stage's" % (
        name, eps, height))


# ---- e. the seeded sweep ---------------------------------------------------------------------------------------------------------
def sweep_cases(seed, n=5):
    rng = np.random.default_rng(7000 + seed)
    names = sorted(T.GENERATORS)
    out = []
    for _ in range(n):
        res = int(rng.choice(SWEEP_SIZES))
        name = names[int(rng.integers(len(names)))]
        family = FAMILIES[int(rng.integers(4))]
        form = ("inplace", "rw", "batch")[int(rng.integers(3))]
        count = int(rng.integers(2, 5)) if form == "batch" else 1
        hh = np.stack([T.GENERATORS[name](res, rng) for _ in range(count)])
        its = int(rng.integers(1, 13))
        sea = T.sea_at(hh[0], 0.3) if rng.random() < 0.5 else OFF
        pick = lambda names: tuple(k for k in names if rng.random() < 0.5)  # noqa: E731
        mseed = int(rng.integers(1 << 30))
        if family == "hydraulic":
            c = case(family, hh, form, its, PARAMS[int(rng.integers(len(PARAMS)))])
        elif family == "hydraulic_ex":
            c = case(family, hh, form, its, PARAMS[int(rng.integers(len(PARAMS)))], on=pick(ALL_ON), seed=mseed)
        elif family == "fluvial":
            prm = (float(f32(rng.random() * 0.5)), float(f32(rng.random() * 0.01)), float(rng.choice([0.5, 1.0, 2.0])),
                   float(rng.choice([0.25, 1.0, 3.0])), sea)
            c = case(family, hh, form, its, prm, on=pick(ALL_MAPS), seed=mseed)
        else:
            c = case(family, hh, form, eps=float(rng.choice([0.0, 1e-6, 1e-4, 1e-2, 0.25])), sea=sea, depth=bool(rng.random() < 0.5))
        c["name"] = name
        out.append(c)
    return out


def drainage_sweep_cases(seed, n=5):
    """The drainage family's sweep, a stream of its own: sizes, generators and the count of a batch as in sweep_cases."""
    rng = np.random.default_rng(9000 + seed)
    names = sorted(T.GENERATORS)
    out = []
    for _ in range(n):
        res = int(rng.choice(SWEEP_SIZES))
        name = names[int(rng.integers(len(names)))]
        form = ("inplace", "batch")[int(rng.integers(2))]
        count = int(rng.integers(2, 5)) if form == "batch" else 1
        hh = np.stack([T.GENERATORS[name](res, rng) for _ in range(count)])
        sea = T.sea_at(hh[0], 0.3) if rng.random() < 0.5 else OFF
        rain = float(rng.choice([0.0, 0.3, 0.75, 1.0, 2.5]))
        mapped, signed = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
        c = case("drainage", hh, form, rain=rain, sea=sea, on=("rainMap",) if mapped else (), signed=signed,
                 seed=int(rng.integers(1 << 30)))
        c["name"] = name
        out.append(c)
    return out


@pytest.mark.parametrize("seed", range(8))
def test_seeded_drainage_sweep(nj, ctx, seed):
    for i, c in enumerate(drainage_sweep_cases(seed)):
        check(nj, ctx, c, "seed %d case %d (drainage_sweep_cases(%d)[%d]): %s on %s" % (seed, i, seed, i, describe(c), c["name"]))


@pytest.mark.parametrize("seed", range(8))
def test_seeded_sweep(nj, ctx, oracle, seed):
    for i, c in enumerate(sweep_cases(seed)):
        check(nj, ctx, c, "seed %d case %d (sweep_cases(%d)[%d]): %s on %s" % (seed, i, seed, i, describe(c), c["name"]))
