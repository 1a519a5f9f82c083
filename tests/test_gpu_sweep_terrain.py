"""The terrain stages -- hydraulic erosion plain and _ex, fluvial erosion, depression filling -- on the adversarial tiles of
tests/terrain_tiles.py, every plane bit for bit against the numpy models (hydraulic_ref, hydraulic_ex_ref, fluvial_ref,
fill_ref.flood):

    a. odd widths     sizes with two and three live cells in a row's last quad and sizes astride one 16-row tile edge, the
                      three forms, batches whose tiles start 4 and 8 bytes off the vector alignment, guarded slabs
    b. ties           terraces, cones, pits and the checkerboard, sea levels and epsilons that land on cell values
    c. scales         heights in metres, negative, subnormal differences, signed zeros
    d. winding fill   the serpentine: tiles that go quiet and wake up, at three sweep caps and inside a batch
    e. seeded sweep   size, generator, family, form and parameters drawn from a seed

tests/test_terrain_tiles.py shows on the CPU that the tiles are what b, c and d take them for.  A case is a dict (family,
form, hh = count x res x res heights, parameters); model(case) and gpu(nj, ctx, case) give its planes.  A case of the sweep
is replayed alone with check(nj, ctx, sweep_cases(seed)[i])."""
import ctypes as C

import numpy as np
import pytest

import fill_ref as L
import fluvial_ref as F
import hydraulic_ex_ref as X
import hydraulic_ref as H
import terrain_tiles as T
import test_gpu_fill as GL
import test_gpu_fluvial as GF
import test_gpu_hydraulic as GH
import test_gpu_hydraulic_ex as GX
from test_gpu_slab import PAIRS, carved, memo
from test_hydraulic_ref import NAMES, PARAMS

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = float(F.SEA_OFF)
FAMILIES = ("hydraulic", "hydraulic_ex", "fluvial", "fill")
PLANES = {"hydraulic": ("result", "water"), "hydraulic_ex": ("result", "water", "wear", "deposits"),
          "fluvial": ("result", "drainage"), "fill": ("result", "depth")}
ALL_ON = ("open", "rainMap", "hardness", "masks")
ALL_MAPS = ("rainMap", "hardness", "upliftMap", "drainageIn")
SWEEP_SIZES = (5, 7, 16, 19, 30, 34, 62, 63, 66, 70, 95, 127, 129, 131, 194)


# ---- a case, its model and its run on the GPU ---------------------------------------------------------------------------------
def case(family, hh, form="inplace", its=1, prm=None, on=(), eps=1e-4, sea=OFF, depth=True, budget=GL.GENEROUS, seed=11,
         keys=None):
    """hh: one res x res plane or count of them.  on: the options of the _ex entry (ALL_ON) or the planes of the fluvial one
    (ALL_MAPS), random maps from `seed`.  keys: one hashable per tile under which its model is shared between cases."""
    hh = np.ascontiguousarray(hh, f32)
    hh = hh[None] if hh.ndim == 2 else hh
    assert form in ("inplace", "rw", "batch") and (form != "inplace" or len(hh) == 1)
    c = dict(family=family, hh=hh, form=form, its=its, prm=prm, on=tuple(on), eps=eps, sea=sea, depth=depth, budget=budget,
             seed=seed, keys=keys)
    if family == "hydraulic_ex":
        rain, hard = GX.maps_for(hh.shape, seed)
        c["opts"] = dict(border=X.OPEN if "open" in on else X.CLOSED, rainMap=rain if "rainMap" in on else None,
                         hardness=hard if "hardness" in on else None, masks="masks" in on)
    if family == "fluvial":
        maps = GF.maps_for(hh.shape, seed)
        c["maps"] = {k: maps[k] for k in ALL_MAPS if k in on}
    return c


def describe(c):
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
    W = L.flood(h, c["eps"], c["sea"])
    return W, (W - h).astype(f32)


def model(c):
    """The planes of PLANES[family], each count x res x res."""
    per_tile = []
    for k in range(len(c["hh"])):
        if c["keys"] is None:
            per_tile.append(_model_tile(c, k))
        else:
            # (the random maps of tile k depend on the shape of the whole case)
            key = ("terrain", c["family"], c["keys"][k], c["hh"].shape, k, c["its"], c["prm"], c["on"], c["eps"], c["sea"],
                   c["seed"])
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
    rain, hard = GX.maps_for((1, res, res), 11)
    maps = GF.maps_for((1, res, res), 11)
    nhyd, nflu = N.lib.nz_hydraulic_erosion_work_floats(res, 1), N.lib.nz_fluvial_erosion_work_floats(res, 1)
    nfill = N.lib.nz_fill_depressions_work_floats(res, 1)
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
    return out


@pytest.mark.parametrize("res", [65, 130])
@pytest.mark.parametrize("name", list(T.TIES))
def test_ties(nj, ctx, oracle, name, res):
    for c in tie_cases(name, res):
        check(nj, ctx, c, name + " " + describe(c))


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
    return out


@pytest.mark.parametrize("res", [66, 97])
@pytest.mark.parametrize("name", list(T.SCALES))
def test_scales(nj, ctx, oracle, name, res):
    for c in scale_cases(name, res):
        got = check(nj, ctx, c, name + " " + describe(c))
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


@pytest.mark.parametrize("seed", range(8))
def test_seeded_sweep(nj, ctx, oracle, seed):
    for i, c in enumerate(sweep_cases(seed)):
        check(nj, ctx, c, "seed %d case %d (sweep_cases(%d)[%d]): %s on %s" % (seed, i, seed, i, describe(c), c["name"]))
