"""Six newer terrain stages -- watershed, stream order, the implicit fluvial step, hillslope diffusion, multiple-flow
drainage, the multiple-flow implicit fluvial step -- on the adversarial tiles of tests/terrain_tiles.py and on `faint`, every
plane bit for bit against the numpy models (watershed_ref.walk with fluvial_ref.receivers, stream_order_ref.walk,
fluvial_implicit_ref.walk, hillslope_ref.diffuse, drainage_mfd_ref.walk, fluvial_implicit_mfd_ref.walk).  The cases and the
models are tests/relax_sweep_cases.py; tests/test_relax_sweep_cases.py shows on the CPU that the tiles are what b, c and d take
them for.

    a. odd widths     sizes with two and three live cells in a row's last quad and sizes astride one 16-row tile edge, every
                      form of each family, batches whose tiles start 4 and 8 bytes off the vector alignment (the receiver and
                      order bytes then 1 and 2 bytes off their word); the multiple-flow implicit step with a sea on a cell
                      value, both maps and a rain map, at exponents 1 and 16
    b. ties           terraces, cones, pits and the checkerboard, a sea level that lands on cell values, the batch of a tile,
                      the tile upside down and the tile transposed; exponents 1, 3 and 16, for the multiple-flow drainage
                      and for the implicit step on it
    c. scales         heights in metres, negative, subnormal differences, signed zeros, subnormal heights: results that are
                      subnormal or -0, weights that underflow and shut single gates of the multiple-flow implicit step, both
                      implicit steps without erosion and uplift
    d. a chain        fill -> drainage area -> watershed, stream order and the implicit step, and fill -> multiple-flow
                      drainage -> multiple-flow implicit step, on the tie tiles, kernel feeding kernel; the basin sizes
                      counted on the host are the drainage areas of the outlets
    e. schedules      the checkerboard between two terraces in a batch at sweep caps 1, 3 and the default
    f. seeded sweep   size, tile, family, form and parameters drawn from a seed (relax_sweep_cases), and the multiple-flow
                      implicit step's stream of its own (mfd_sweep_cases)

check() asserts converged == 1 and a pass count within the bound the stage's own test uses; the run helpers of the six stage
tests assert that the inputs come back untouched.  A case of the sweeps is replayed alone with
check(nj, ctx, relax_sweep_cases(seed)[i]) or check(nj, ctx, mfd_sweep_cases(seed)[i])."""
import numpy as np
import pytest

import relax_sweep_cases as RC
import terrain_tiles as T
import test_gpu_drainage_mfd as GM
import test_gpu_fluvial_implicit as GI
import test_gpu_fluvial_implicit_mfd as GI2
import test_gpu_hillslope as GH
import test_gpu_stream_order as GS
import test_gpu_sweep_terrain as TS
import test_gpu_watershed as GW
from relax_sweep_cases import (PLANES, RELAXATIONS, case, describe, mfd_sweep_cases, model, odd_cases, relax_sweep_cases,
                               scale_cases, tie_cases)
from test_relax_sweep_cases import assert_labels_count_the_drainage, assert_labels_follow_the_receivers

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = RC.OFF
GENEROUS = {"watershed": GW.GENEROUS, "stream_order": GS.GENEROUS, "fluvial_implicit": GI.GENEROUS, "drainage_mfd": GM.GENEROUS,
            "fluvial_implicit_mfd": GI2.GENEROUS}
# the passes a budget has to hold beyond the bound: the multiple-flow implicit step's own test asks for the DAG height + 2 and
# sees the step converge within the DAG height + 1
SPARE = {"fluvial_implicit_mfd": 1}


def assert_same(got, want, what):
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    g, w = (got, want) if got.dtype.itemsize == 1 else (got.view(np.uint32), want.view(np.uint32))
    bad = g != w
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


# ---- a case's run on the GPU, and its comparison -------------------------------------------------------------------------------
def gpu(nj, ctx, c, budget):
    """The planes of PLANES[family], each count x res x res, one not asked for None; c["passes"] and c["converged"] for the
    five relaxations."""
    fam, hh = c["family"], c["hh"]
    single = c["form"] != "batch"
    arg = hh[0] if single else hh
    at = (lambda m: m[0] if m is not None else None) if single else (lambda m: m)
    if fam == "watershed":
        *out, passes, conv = GW.run_gpu(nj, ctx, arg, c["sea"], c["cellSize"], budget, c["length"], c["receivers"])
    elif fam == "stream_order":
        *out, passes, conv = GS.run_gpu(nj, ctx, arg, c["sea"], at(c["drainage"]), c["threshold"], budget, c["links"])
    elif fam == "fluvial_implicit":
        *out, passes, conv = GI.run_gpu(nj, ctx, arg, at(c["drainage"]), budget, hardness=at(c["hardness"]),
                                        upliftMap=at(c["upliftMap"]), erodibility=c["erodibility"], uplift=c["uplift"],
                                        dt=c["dt"], seaLevel=c["sea"])
    elif fam == "drainage_mfd":
        *out, passes, conv = GM.run_gpu(nj, ctx, arg, c["rain"], c["sea"], budget, at(c["rainMap"]), c["exponent"])
    elif fam == "fluvial_implicit_mfd":
        *out, passes, conv = GI2.run_gpu(nj, ctx, arg, at(c["drainage"]), budget, hardness=at(c["hardness"]),
                                         upliftMap=at(c["upliftMap"]), erodibility=c["erodibility"], uplift=c["uplift"],
                                         dt=c["dt"], seaLevel=c["sea"], exponent=c["exponent"])
    else:
        out = [GH.run_gpu(nj, ctx, arg, c["diffusivity"], c["dt"], c["iterations"], in_place=c["form"] == "inplace")]
        passes = conv = None
    c["passes"], c["converged"] = passes, conv
    return [g.reshape(hh.shape) if g is not None else None for g in out]


def check(nj, ctx, c, what=""):
    want, bound = model(c)
    what = what or describe(c)
    budget = c["budget"] or (max(GENEROUS[c["family"]], bound + SPARE.get(c["family"], 0)) if bound is not None else None)
    got = gpu(nj, ctx, c, budget)
    assert len(got) == len(want) == len(PLANES[c["family"]])
    for name, g, w in zip(PLANES[c["family"]], got, want):
        # the models never leave the finite numbers on these inputs: a NaN's payload would be the host's, not the model's
        assert np.isfinite(w).all(), "%s: the model's %s is not finite" % (what, name)
        if g is None:
            assert not c[{"length": "length", "receivers": "receivers", "link": "links"}[name]], (what, name)
            continue
        assert_same(g, w, "%s: %s" % (what, name))
    if c["family"] in RELAXATIONS:
        assert c["converged"] == 1 and 1 <= c["passes"] <= bound, (what, c["passes"], c["converged"], bound)
    return got


# ---- a. odd widths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [66, 67, 130, 131, 15, 18, 31, 33, 47])
def test_odd_widths(nj, ctx, res):
    if res in (67, 131):  # tiles 1 and 2 of a batch start one and two floats past a 16-byte boundary; their bytes one and two
        probe = ctx.alloc(4)
        assert probe.ptr % 16 == 0 and [(k * res * res) % 4 for k in range(3)] == [0, 1, 2]
        probe.Dispose()
    cases = odd_cases(res)
    assert {(c["family"], c["form"]) for c in cases} >= {(f, "batch") for f in RC.FAMILIES} | {("hillslope", "inplace")}
    for c in cases:
        check(nj, ctx, c)


# ---- b. ties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [65, 130])
@pytest.mark.parametrize("name", list(T.TIES))
def test_ties(nj, ctx, name, res):
    for c in tie_cases(name, res):
        check(nj, ctx, c, name + " " + describe(c))


# ---- c. scales -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [66, 97])
@pytest.mark.parametrize("name", list(RC.SCALES))
def test_scales(nj, ctx, name, res):
    for c in scale_cases(name, res):
        got = check(nj, ctx, c, name + " " + describe(c))
        if c["family"] in ("fluvial_implicit", "fluvial_implicit_mfd") and c["erodibility"] == 0 and c["uplift"] == 0:
            # the model's bits are the heights but on `zeros`, where a -0 with a receiver comes back as +0 -- in the
            # multiple-flow step every -0 that is no outlet: tests/test_relax_sweep_cases.py holds both models to that set
            assert np.array_equal(got[0], c["hh"])
            if name != "zeros":
                assert_same(got[0], c["hh"], name + ": the heights bit for bit")


# ---- d. a chain on ties, kernel feeding kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 1e-4])
@pytest.mark.parametrize("name", list(T.TIES))
def test_a_chain_on_ties(nj, ctx, name, eps):
    """nz_fill_depressions, nz_drainage_area on the filled plane, then nz_watershed, nz_stream_order and nz_fluvial_implicit on
    the planes the GPU made, and on the same filled plane nz_drainage_mfd, then nz_fluvial_implicit_mfd on the plane that
    made: every output is the numpy chain's.  With epsilon 0 the lakes are flats without receivers and without a lower
    neighbour, every cell of them a basin of its own."""
    res = 65
    h = RC.tile(name, res)
    what = "%s eps %g: " % (name, eps)
    key = (name, "flooded", eps)
    filled = TS.check(nj, ctx, TS.case("fill", h, eps=eps, keys=[name]), what + "fill")[0][0]
    A = TS.check(nj, ctx, TS.case("drainage", filled, keys=[key]), what + "drainage of the filled plane")[0][0]
    basin, _, r = check(nj, ctx, case("watershed", filled, keys=[key]), what + "watershed")
    check(nj, ctx, case("stream_order", filled, keys=[key], drainage=A, threshold=2.0), what + "stream order")
    check(nj, ctx, case("fluvial_implicit", filled, keys=[key], drainage=A, dt=200.0), what + "implicit step")
    # the multiple-flow branch on the same filled plane: nz_drainage_mfd, then nz_fluvial_implicit_mfd on the plane it made
    Am = check(nj, ctx, case("drainage_mfd", filled, keys=[key], exponent=3), what + "multiple-flow drainage")[0][0]
    check(nj, ctx, case("fluvial_implicit_mfd", filled, keys=[key], drainage=Am, exponent=3, dt=200.0),
          what + "multiple-flow implicit step")
    # without a model: the cells that carry a label are the drainage area of that outlet, and a label follows the receivers
    assert_labels_count_the_drainage(basin[0], r[0], A)
    assert_labels_follow_the_receivers(basin[0], r[0])


# ---- e. schedule freedom on a tie tile -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", RELAXATIONS)
def test_the_sweep_cap_does_not_matter_on_ties(nj, ctx, family):
    """The checkerboard is at rest after a pass or two, the terraces either side of it are not: the flag bytes of tile 1 lie
    behind tile 0's.  Fewer sweeps on chip: more passes, the same planes."""
    res = 97
    hh = np.stack([RC.tile("terraces4", res), RC.tile("checker", res), RC.tile("terraces4", res)])
    kw = {"watershed": dict(cellSize=0.3), "stream_order": dict(drainage=True, threshold=2.0),
          "fluvial_implicit": dict(dt=200.0, maps=True), "drainage_mfd": dict(exponent=3, rain=0.75, rainmap="signed"),
          "fluvial_implicit_mfd": dict(dt=200.0, maps=True, exponent=3)}[family]
    hook = getattr(nj._native.lib, "nz_debug_%s_sweeps" % family)
    runs = {}
    try:
        for cap in (1, 3, 0):  # 0: the default
            hook(cap)
            c = case(family, hh, "batch", ["terraces4", "checker", "terraces4"], sea=T.sea_at(hh[0], 0.3), **kw)
            runs[cap] = (check(nj, ctx, c, "%s with a cap of %d sweeps" % (family, cap)), c["passes"])
    finally:
        hook(0)
    for cap in (1, 3):
        for name, g, w in zip(PLANES[family], runs[cap][0], runs[0][0]):
            assert_same(g, w, "%s with a cap of %d sweeps against the default: %s" % (family, cap, name))
    assert runs[1][1] >= max(runs[3][1], runs[0][1]), {cap: r[1] for cap, r in runs.items()}


# ---- f. the seeded sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_seeded_sweep(nj, ctx, seed):
    for i, c in enumerate(relax_sweep_cases(seed)):
        check(nj, ctx, c, "seed %d case %d (relax_sweep_cases(%d)[%d]): %s on %s" % (seed, i, seed, i, describe(c), c["name"]))
    for i, c in enumerate(mfd_sweep_cases(seed)):
        check(nj, ctx, c, "seed %d case %d (mfd_sweep_cases(%d)[%d]): %s on %s" % (seed, i, seed, i, describe(c), c["name"]))
