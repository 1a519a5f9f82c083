"""The cases and the models of tests/test_gpu_sweep_relax.py: six newer terrain stages -- watershed, stream order, the
implicit fluvial step, hillslope diffusion, multiple-flow drainage, the multiple-flow implicit fluvial step -- on the
adversarial tiles of tests/terrain_tiles.py and on one tile more, `faint`, whose heights are themselves subnormal.  Plain
numpy and the case helpers of the existing sweep (tests/test_gpu_sweep_terrain.py): nothing here opens a GPU, and
tests/test_relax_sweep_cases.py runs without one.

A case is a dict (family, form, hh = count x res x res heights, parameters).  model(case) gives the planes of
PLANES[family], each count x res x res, and the bound on passes the stage's own GPU test uses (None for the hillslope stage,
which is no relaxation):

    watershed         watershed_ref.walk + fluvial_ref.receivers     hops.max() + 2
    stream_order      stream_order_ref.walk                          chain + 2
    fluvial_implicit  fluvial_implicit_ref.walk                      hops.max() + 2 (the watershed's dependency graph)
    hillslope         hillslope_ref.diffuse                          --
    drainage_mfd      drainage_mfd_ref.walk                          DAG height + 1
    fluvial_implicit_mfd  fluvial_implicit_mfd_ref.walk              DAG height + 1 (the budget: one pass more)

Forms are "tile" and "batch", for the hillslope stage also "inplace".  The drainage plane of a stream-order case
(drainage=True) and of every implicit-fluvial case is drainage_ref.accumulate of the same heights and sea under unit rain;
that of a multiple-flow implicit case is drainage_mfd_ref.walk of the same heights, sea, rain, rain map and exponent -- the
rain map is positive or none: a signed one gives negative areas, whose square root is no number.  A
plane handed in as an array (the chain of the GPU test, kernel feeding kernel) is used as it is.  keys: one hashable per
tile under which its model is shared between cases; with a plane handed in the key has to name that plane too.

The seeded sweep, relax_sweep_cases(seed), draws from SWEEP_FAMILIES, the five older families, and is pinned by
tests/test_relax_sweep_cases.py; the multiple-flow implicit step has a stream of its own, mfd_sweep_cases(seed), pinned there
too.  A case of either is replayed alone with check(nj, ctx, relax_sweep_cases(seed)[i]) of the GPU test."""
import numpy as np

import drainage_mfd_ref as M
import drainage_ref as D
import fluvial_implicit_mfd_ref as R2
import fluvial_implicit_ref as R
import fluvial_ref as F
import hillslope_ref as HS
import stream_order_ref as S
import terrain_tiles as T
import watershed_ref as W
from test_gpu_slab import memo
from test_gpu_sweep_terrain import SWEEP_SIZES, drainage_rain_map

f32 = np.float32
OFF = float(F.SEA_OFF)
# the five relax_sweep_cases draws from: its pinned digests hang on this tuple.  The sixth has a stream of its own
SWEEP_FAMILIES = ("watershed", "stream_order", "fluvial_implicit", "hillslope", "drainage_mfd")
FAMILIES = SWEEP_FAMILIES + ("fluvial_implicit_mfd",)
# the five with a pass count and a sweep cap
RELAXATIONS = ("watershed", "stream_order", "fluvial_implicit", "drainage_mfd", "fluvial_implicit_mfd")
PLANES = {"watershed": ("basin", "length", "receivers"), "stream_order": ("order", "link"), "fluvial_implicit": ("out",),
          "hillslope": ("out",), "drainage_mfd": ("out",), "fluvial_implicit_mfd": ("out",)}
# what a case of each family carries, in the order describe() prints it
PARAMETERS = {"watershed": ("sea", "cellSize", "length", "receivers"),
              "stream_order": ("sea", "drained", "threshold", "links"),
              "fluvial_implicit": ("erodibility", "uplift", "dt", "sea", "maps", "seed"),
              "hillslope": ("diffusivity", "dt", "iterations"),
              "drainage_mfd": ("rain", "sea", "exponent", "rainmap", "seed"),
              "fluvial_implicit_mfd": ("erodibility", "uplift", "dt", "sea", "exponent", "rain", "maps", "rainmap", "seed")}
_OUTPUT_ONLY = ("length", "receivers", "links")  # which planes are asked for: the model does not depend on it
EXPONENTS = (1, 2, 3, 4, 16)
RS = (0.01, 1.0, 100.0, 1e4)
DTS = (1.0, 50.0, 200.0)
UPLIFTS = (0.0, 0.002)
ERODIBILITIES = (0.0, 0.05, 0.5)


def faint(res, rng):
    """relief * 3e-38: heights of 6e-39 .. 1.7e-38 either side of the smallest normal number, 1.18e-38 -- a quarter to a half of
    the cells are subnormal themselves, and so are all their differences."""
    return (T.relief(res, rng) * f32(3e-38)).astype(f32)


TILES = {**T.GENERATORS, "faint": faint}
SCALES = {**T.SCALES, "faint": faint}


def tile(name, res, seed=3):
    """The tile of the existing sweep for the names it has (the same key, so the same array)."""
    return memo(("terrain tile", name, res, seed), lambda: TILES[name](res, np.random.default_rng(seed)))


def subnormal(a):
    """The cells of a float32 plane that are subnormal: not zero, and below the smallest normal number."""
    a = np.abs(np.asarray(a, f32))
    return (a > 0) & (a < np.finfo(f32).tiny)


def implicit_maps(shape, seed):
    """(hardness in [0, 1), upliftMap in [0, 2)) of a case's shape."""
    rng = np.random.default_rng(seed)
    return rng.random(shape, dtype=f32), (rng.random(shape, dtype=f32) * f32(2.0)).astype(f32)


# ---- a case and its model ------------------------------------------------------------------------------------------------------
def case(family, hh, form="tile", keys=None, seed=11, budget=None, sea=OFF, cellSize=1.0, length=True, receivers=True,
         drainage=None, threshold=0.0, links=True, erodibility=0.05, uplift=0.002, dt=1.0, maps=False, diffusivity=0.01,
         iterations=1, rain=1.0, exponent=1, rainmap=None):
    """hh: one res x res plane or count of them.  drainage: None, True (accumulate of the heights) or the planes themselves;
    maps: hardness and upliftMap from `seed`; rainmap: None, "positive" or "signed", from `seed`; budget: the passes the
    call may take, None for "the stage's GENEROUS, or the model's bound where that is more"."""
    hh = np.ascontiguousarray(hh, f32)
    hh = hh[None] if hh.ndim == 2 else hh
    assert family in FAMILIES and form in ("tile", "batch", "inplace") and (form == "batch" or len(hh) == 1)
    assert form != "inplace" or family == "hillslope"
    assert rainmap in (None, "positive", "signed") and (keys is None or len(keys) == len(hh))
    mfd = family == "fluvial_implicit_mfd"
    assert not mfd or rainmap in (None, "positive")  # a signed map gives negative A: sqrt(A) leaves the finite numbers
    given = isinstance(drainage, np.ndarray)
    drained = True if family in ("fluvial_implicit", "fluvial_implicit_mfd") else given or bool(drainage)
    c = dict(family=family, hh=hh, form=form, keys=keys, seed=seed, budget=budget, sea=sea, cellSize=cellSize, length=length,
             receivers=receivers, drained=drained, given=given, threshold=threshold, links=links, erodibility=erodibility,
             uplift=uplift, dt=dt, maps=bool(maps), diffusivity=diffusivity, iterations=iterations, rain=rain,
             exponent=exponent, rainmap=rainmap, drainage=None, hardness=None, upliftMap=None, rainMap=None)
    if family in ("stream_order", "fluvial_implicit") and drained:
        if given:
            c["drainage"] = np.ascontiguousarray(drainage, f32).reshape(hh.shape)
        else:
            area = lambda k: D.accumulate(hh[k], 1.0, sea)[0]  # noqa: E731
            c["drainage"] = np.stack([area(k) if keys is None else memo(("relax area", keys[k], hh.shape[-1], sea), lambda: area(k))
                                      for k in range(len(hh))])
    if family in ("fluvial_implicit", "fluvial_implicit_mfd") and maps:
        c["hardness"], c["upliftMap"] = memo(("relax implicit maps", hh.shape, seed), lambda: implicit_maps(hh.shape, seed))
    if family in ("drainage_mfd", "fluvial_implicit_mfd") and rainmap:
        c["rainMap"] = memo(("terrain rain map", hh.shape, seed, rainmap == "signed"),
                            lambda: drainage_rain_map(hh.shape, seed, rainmap == "signed"))
    if mfd:  # the multiple-flow drainage of the same heights, sea, rain and exponent
        if given:
            c["drainage"] = np.ascontiguousarray(drainage, f32).reshape(hh.shape)
        else:
            rm = c["rainMap"]
            area = lambda k: M.walk(hh[k], rain, sea, rm[k] if rm is not None else None, exponent)[0]  # noqa: E731
            # (the rain map of tile k depends on the shape of the whole case)
            where = lambda k: (hh.shape, k, seed) if rm is not None else hh.shape[-1]  # noqa: E731
            c["drainage"] = np.stack([area(k) if keys is None else
                                      memo(("relax mfd area", keys[k], where(k), rain, sea, exponent), lambda: area(k))
                                      for k in range(len(hh))])
    return c


def describe(c):
    return "%s %s %d x %d^2 %s" % (c["family"], c["form"], len(c["hh"]), c["hh"].shape[-1],
                                   " ".join("%s %r" % (p, c[p]) for p in PARAMETERS[c["family"]]))


def hops(h, sea):
    """The moves of every cell's flow path to its outlet or pit."""
    return W.walk(h, sea)[2]


def _model_tile(c, k):
    """(planes, bound) of tile k."""
    fam, h, sea = c["family"], c["hh"][k], c["sea"]
    at = lambda m: m[k] if m is not None else None  # noqa: E731
    if fam == "watershed":
        basin, length, hop = W.walk(h, sea, c["cellSize"])
        return (basin, length, F.receivers(h, sea)[0]), int(hop.max()) + 2
    if fam == "stream_order":
        order, link, chain = S.walk(h, sea, at(c["drainage"]), c["threshold"])
        return (order, link), chain + 2
    if fam == "fluvial_implicit":
        out = R.walk(h, c["drainage"][k], erodibility=c["erodibility"], uplift=c["uplift"], dt=c["dt"], seaLevel=sea,
                     hardness=at(c["hardness"]), upliftMap=at(c["upliftMap"]))
        return (out,), int(hops(h, sea).max()) + 2
    if fam == "fluvial_implicit_mfd":
        out, height = R2.walk(h, c["drainage"][k], erodibility=c["erodibility"], uplift=c["uplift"], dt=c["dt"], seaLevel=sea,
                              exponent=c["exponent"], hardness=at(c["hardness"]), upliftMap=at(c["upliftMap"]))
        return (out,), height + 1
    if fam == "hillslope":
        return (HS.diffuse(h, c["diffusivity"], c["dt"], c["iterations"]),), None
    A, height = M.walk(h, c["rain"], sea, at(c["rainMap"]), c["exponent"])
    return (A,), height + 1


def model(c):
    """(the planes of PLANES[family], each count x res x res; the bound on passes, over the whole batch as the status words
    are, or None)."""
    per_tile = []
    for k in range(len(c["hh"])):
        if c["keys"] is None:
            per_tile.append(_model_tile(c, k))
        else:
            prm = tuple(c[p] for p in PARAMETERS[c["family"]] if p not in _OUTPUT_ONLY)
            # (the random maps of tile k depend on the shape of the whole case)
            where = (c["hh"].shape, k) if c["hardness"] is not None or c["rainMap"] is not None else c["hh"].shape[-1]
            per_tile.append(memo(("relax", c["family"], c["keys"][k], where, prm, c["given"]), lambda: _model_tile(c, k)))
    planes = [np.stack(p) for p in zip(*(t[0] for t in per_tile))]
    bounds = [t[1] for t in per_tile]
    return planes, (max(bounds) if bounds[0] is not None else None)


# ---- a. odd widths -------------------------------------------------------------------------------------------------------------
def odd_cases(res):
    """terraces16 and noisy singly in every form, and the batch [terraces16, noisy, noisy T]: at an odd size tiles 1 and 2
    start one and two floats past a 16-byte boundary, the receiver and order bytes one and two bytes off a word."""
    a, b = tile("terraces16", res), tile("noisy", res)
    batch = np.stack([a, b, memo(("terrain tile", "noisy T", res), lambda: np.ascontiguousarray(b.T))])
    keys = ["terraces16", "noisy", "noisy T"]
    sea = T.sea_at(a, 0.3)
    out = []
    for fam, kw in (("watershed", dict()), ("watershed", dict(cellSize=0.3, length=False, receivers=False)),
                    ("stream_order", dict(drainage=True, threshold=2.0)), ("stream_order", dict()),
                    ("fluvial_implicit", dict(maps=True, sea=sea, dt=200.0)),
                    ("hillslope", dict(diffusivity=100.0, dt=1.0, iterations=3)),
                    ("drainage_mfd", dict(rain=0.75, exponent=1, rainmap="positive")),
                    ("drainage_mfd", dict(rain=0.75, exponent=16, rainmap="positive")),
                    ("fluvial_implicit_mfd", dict(maps=True, sea=sea, dt=200.0, exponent=1, rain=0.75, rainmap="positive")),
                    ("fluvial_implicit_mfd", dict(maps=True, sea=sea, dt=200.0, exponent=16, rain=0.75, rainmap="positive"))):
        for k in (0, 1):
            for form in ("tile", "inplace") if fam == "hillslope" else ("tile",):
                out.append(case(fam, batch[k], form, keys[k:k + 1], **kw))
        out.append(case(fam, batch, "batch", keys, **kw))
    return out


# ---- b. ties -------------------------------------------------------------------------------------------------------------------
def three(name, res):
    """The tile, the tile upside down and the tile transposed, with their keys."""
    h = tile(name, res)
    return (memo(("terrain tile x3", name, res), lambda: np.stack([h, h[::-1], h.T])),
            [name, name + " upside down", name + " T"])


def tie_cases(name, res):
    h = tile(name, res)
    sea = T.sea_at(h, 0.3)
    assert (h == f32(sea)).any() and (h > f32(sea)).any()  # a level of the tile itself: `<=` decides whole plateaus
    keys = [name]
    hhh, keys3 = three(name, res)
    out = []
    for s, cs in ((OFF, 1.0), (sea, 0.3)):
        out.append(case("watershed", h, keys=keys, sea=s, cellSize=cs))
        out.append(case("fluvial_implicit", h, keys=keys, sea=s, dt=200.0, maps=s != OFF))
        for e in (1, 3, 16):
            out.append(case("drainage_mfd", h, keys=keys, sea=s, exponent=e, rain=1.0 if s == OFF else 0.75,
                            rainmap=None if s == OFF else "positive"))
            out.append(case("fluvial_implicit_mfd", h, keys=keys, sea=s, exponent=e, dt=200.0, maps=s != OFF))
    out.append(case("hillslope", h, keys=keys, diffusivity=0.01))
    out.append(case("hillslope", h, "inplace", keys, diffusivity=1e4, iterations=3))
    # once per tile the batch of three, every family; the stream-order stage runs singly on these tiles in its own file
    out.append(case("watershed", hhh, "batch", keys3, sea=sea, cellSize=0.3))
    out.append(case("stream_order", hhh, "batch", keys3, sea=sea, drainage=True, threshold=2.0))
    out.append(case("stream_order", hhh, "batch", keys3))
    out.append(case("fluvial_implicit", hhh, "batch", keys3, sea=sea, dt=50.0))
    out.append(case("hillslope", hhh, "batch", keys3, diffusivity=1e4))
    out.append(case("drainage_mfd", hhh, "batch", keys3, sea=sea, exponent=3, rain=0.3, rainmap="signed"))
    out.append(case("fluvial_implicit_mfd", hhh, "batch", keys3, sea=sea, exponent=3, dt=50.0))
    return out


# ---- c. scales -----------------------------------------------------------------------------------------------------------------
def scale_cases(name, res):
    h = tile(name, res)
    sea = T.sea_at(h, 0.3)
    keys = [name]
    hhh, keys3 = three(name, res)
    out = [case("watershed", h, keys=keys, cellSize=0.3),
           case("watershed", hhh, "batch", keys3, sea=sea),
           case("stream_order", h, keys=keys, sea=sea, drainage=True, threshold=2.0),
           case("stream_order", hhh, "batch", keys3),
           case("fluvial_implicit", h, keys=keys, dt=50.0, maps=True),
           case("fluvial_implicit", hhh, "batch", keys3, sea=sea, dt=200.0),
           case("fluvial_implicit", h, keys=keys, uplift=0.0, dt=1.0),
           case("fluvial_implicit", h, keys=keys, uplift=0.0, dt=200.0),
           identity_case(h, keys)]
    for r in RS:
        for its in (1, 3):
            out.append(case("hillslope", h, "inplace" if its == 3 and r == 1.0 else "tile", keys, diffusivity=r, iterations=its))
    out.append(case("hillslope", hhh, "batch", keys3, diffusivity=100.0, iterations=3))
    for e in (4, 16):
        out.append(case("drainage_mfd", h, keys=keys, exponent=e, rain=0.3, rainmap="signed"))
    out.append(case("drainage_mfd", hhh, "batch", keys3, sea=sea, exponent=16, rain=0.3, rainmap="signed"))
    out += [case("fluvial_implicit_mfd", h, keys=keys, exponent=4, dt=50.0, maps=True),
            case("fluvial_implicit_mfd", h, keys=keys, exponent=16, dt=200.0),
            case("fluvial_implicit_mfd", hhh, "batch", keys3, sea=sea, exponent=16, dt=200.0),
            case("fluvial_implicit_mfd", h, keys=keys, uplift=0.0, dt=1.0),
            case("fluvial_implicit_mfd", h, keys=keys, uplift=0.0, dt=200.0),
            identity_case(h, keys, "fluvial_implicit_mfd")]
    return out


def identity_case(h, keys=None, family="fluvial_implicit"):
    """erodibility 0 and uplift 0: f = +0 and du = +0 everywhere, so out = (h + 0) / 1 -- the heights bit for bit, but that a
    -0 with a receiver comes back as +0.  In the multiple-flow step every f_k is +0 too: N = (h + 0) plus zeros, D = 1, and
    where no gate is open out = b = h + 0 -- the heights again, but that every -0 that is no outlet comes back as +0."""
    return case(family, h, keys=keys, erodibility=0.0, uplift=0.0, dt=200.0)


# ---- f. the seeded sweep -------------------------------------------------------------------------------------------------------
# 11000 + seed left the stream-order stage without a batch in seeds 0 to 7; tests/test_relax_sweep_cases.py asks every family
# for both forms, and this is the first offset from there on that gives it and all sixteen tiles
SWEEP_OFFSET = 11010


def relax_sweep_cases(seed, n=5):
    """Size, tile, family, form and parameters from a seed.  Every case makes the same draws in the same order, whatever its
    family uses of them, but for the heights, which take what their generator takes."""
    rng = np.random.default_rng(SWEEP_OFFSET + seed)
    names = sorted(TILES)
    pick = lambda values: values[int(rng.integers(len(values)))]  # noqa: E731
    coin = lambda: bool(rng.random() < 0.5)  # noqa: E731
    out = []
    for _ in range(n):
        res = int(rng.choice(SWEEP_SIZES))
        name = pick(names)
        family = pick(SWEEP_FAMILIES)
        form = pick(("tile", "batch"))
        count = int(rng.integers(2, 5))
        in_place = coin()
        if form == "tile":
            count = 1
            if family == "hillslope" and in_place:
                form = "inplace"
        hh = np.stack([TILES[name](res, rng) for _ in range(count)])
        sea = T.sea_at(hh[0], 0.3) if coin() else OFF
        prm = dict(sea=sea, cellSize=pick((0.3, 1.0)), length=coin(), receivers=coin(), drainage=coin(),
                   threshold=pick((0.0, 2.0, 8.0)), links=coin(), erodibility=pick(ERODIBILITIES), uplift=pick(UPLIFTS),
                   dt=pick(DTS), maps=coin(), diffusivity=pick(RS), iterations=int(rng.integers(1, 4)),
                   rain=pick((0.3, 0.75, 1.0)), exponent=pick(EXPONENTS), rainmap=pick((None, "positive", "signed")),
                   seed=int(rng.integers(1 << 30)))
        if family == "hillslope":
            prm["dt"] = 1.0  # r is the one product: the list RS holds it
        c = case(family, hh, form, **prm)
        c["name"] = name
        out.append(c)
    return out


# 13000 + seed reaches both forms, `faint`, exponent 16 and a rain map in seeds 0 to 7, but its exponent-16 cases and its
# faint ones all have erodibility 0 and one of its tiles is 194^2; this is the first offset from there on at which a faint
# tile and an exponent-16 case that is neither flat nor the checkerboard erode, at sizes up to 131
MFD_SWEEP_OFFSET = 13028


def mfd_sweep_cases(seed, n=3):
    """The multiple-flow implicit step's sweep, a stream of its own so that relax_sweep_cases stays as it is pinned: size,
    tile, form, count, heights, sea, erodibility, uplift, dt, maps, exponent, rain, rain map (positive or none) and seed,
    every case the same draws in the same order."""
    rng = np.random.default_rng(MFD_SWEEP_OFFSET + seed)
    names = sorted(TILES)
    pick = lambda values: values[int(rng.integers(len(values)))]  # noqa: E731
    coin = lambda: bool(rng.random() < 0.5)  # noqa: E731
    out = []
    for _ in range(n):
        res = int(rng.choice(SWEEP_SIZES))
        name = pick(names)
        form = pick(("tile", "batch"))
        count = int(rng.integers(2, 5))
        if form == "tile":
            count = 1
        hh = np.stack([TILES[name](res, rng) for _ in range(count)])
        sea = T.sea_at(hh[0], 0.3) if coin() else OFF
        prm = dict(sea=sea, erodibility=pick(ERODIBILITIES), uplift=pick(UPLIFTS), dt=pick(DTS), maps=coin(),
                   exponent=pick(EXPONENTS), rain=pick((0.3, 0.75, 1.0)), rainmap="positive" if coin() else None,
                   seed=int(rng.integers(1 << 30)))
        c = case("fluvial_implicit_mfd", hh, form, **prm)
        c["name"] = name
        out.append(c)
    return out
