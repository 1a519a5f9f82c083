"""CPU checks of the extended hydraulic erosion model (tests/hydraulic_ex_ref.py): with every option off it is
tests/hydraulic_ref.py bit for bit, neutral maps change nothing, an open border loses water and material where a closed
one conserves them, the masks account for the result, and the C ABI / the three hosts carry the extension."""
import ctypes
import os
import re

import numpy as np
import pytest

import hydraulic_ex_ref as X
import hydraulic_ref as H
from conftest import ROOT
from test_hydraulic_ref import NAMES, PARAMS, relief

f32 = np.float32
f64 = np.float64
ENTRIES = ("nz_hydraulic_erosion_ex", "nz_hydraulic_erosion_ex_rw", "nz_hydraulic_erosion_ex_batch")


def tilted(res=64):
    """A plane that drains towards the corner (0, 0), with a fifth of a smoothed fBm tile on it."""
    x = np.arange(res, dtype=f32)
    plane = (x[None, :] * f32(0.02) + x[:, None] * f32(0.005)).astype(f32)
    return (plane + relief(res) * f32(0.2)).astype(f32)


@pytest.mark.parametrize("prm", PARAMS, ids=["defaults", "strong", "dry-start"])
def test_all_options_off_is_the_plain_driver(prm):
    # also the check of this file's numpy flux and water update against the oracle's C functions
    kw = dict(zip(NAMES, prm))
    for h, its in ((relief(64), 150), (relief(48), 12), (relief(16), 1)):
        want, wwant = H.run(h, its, **kw)
        got, water, wear, deposits = X.run(h, its, **kw)
        assert np.array_equal(got, want) and np.array_equal(water, wwant), (h.shape, its)
    got, water, wear, deposits = X.run(relief(16), 0, **kw)
    assert np.array_equal(got, relief(16)) and (water == f32(prm[0])).all() and not wear.any() and not deposits.any()


@pytest.mark.parametrize("prm", PARAMS, ids=["defaults", "strong", "dry-start"])
def test_neutral_maps_change_nothing(prm):
    kw = dict(zip(NAMES, prm))
    h = relief(64)
    for border in (X.CLOSED, X.OPEN):
        plain = X.run(h, 60, border=border, **kw)
        for maps in (dict(rainMap=np.ones_like(h)), dict(hardness=np.zeros_like(h)),
                     dict(rainMap=np.ones_like(h), hardness=np.zeros_like(h))):
            for a, b in zip(X.run(h, 60, border=border, **maps, **kw), plain):
                assert np.array_equal(a, b), (border, sorted(maps))


def test_closed_conserves_and_open_drains():
    # tilted(64), the defaults, 200 iterations (float64 sums of the float32 planes, measured with this file's driver):
    #   input 3728.139402;  CLOSED result 3728.139387, water 125.280;  OPEN result 3725.194197, water 11.871
    # the open tile has lost 2.9 of height and keeps a tenth of the water: five orders of magnitude above the 1.5e-5 by which
    # the closed sum moves through rounding
    t = tilted()
    s0 = t.astype(f64).sum()
    closed = X.run(t, 200, border=X.CLOSED)
    opened = X.run(t, 200, border=X.OPEN)
    cs, os_ = closed[0].astype(f64).sum(), opened[0].astype(f64).sum()
    cw, ow = closed[1].astype(f64).sum(), opened[1].astype(f64).sum()
    print("input %.6f closed result %.6f water %.6f open result %.6f water %.6f" % (s0, cs, cw, os_, ow))
    assert abs(cs - s0) <= 1e-6 * np.abs(t.astype(f64)).sum(), (s0, cs)  # as tests/test_hydraulic_ref.py checks it
    assert os_ < cs and ow < cw
    assert cs - os_ > 1.0 and cw - ow > 50.0
    assert np.isfinite(opened[0]).all() and (opened[1] >= 0).all()


def test_full_hardness_leaves_no_wear():
    h = relief(64)
    got, water, wear, deposits = X.run(h, 100, hardness=np.ones_like(h))
    assert not wear.any() and not deposits.any() and np.array_equal(got, h)
    half = np.zeros_like(h)
    half[:, :32] = 1.0
    got, water, wear, deposits = X.run(h, 100, hardness=half, **dict(zip(NAMES, PARAMS[1])))
    assert not wear[:, :32].any() and wear[:, 32:].any()


# max |result - (input - wear + deposits)| in float64 over the cells, measured with this file's driver at 150 iterations:
#   relief(64) defaults 4.31e-6, relief(64) PARAMS[1] 8.64e-7, tilted(64) defaults OPEN 8.14e-6
# (the masks are float32 running sums of up to 150 terms next to heights of order 1: a few ulps of the height).  The bound
# is 4 x the measured value.
@pytest.mark.parametrize("name,bound", [("defaults", 4 * 4.31e-6), ("strong", 4 * 8.64e-7), ("open", 4 * 8.14e-6)])
def test_the_masks_account_for_the_result(name, bound):
    tile, kw = {"defaults": (relief(64), {}), "strong": (relief(64), dict(zip(NAMES, PARAMS[1]))),
                "open": (tilted(), dict(border=X.OPEN))}[name]
    got, water, wear, deposits = X.run(tile, 150, **kw)
    assert wear.any() and deposits.any() and (wear >= 0).all() and (deposits >= 0).all()
    resid = np.abs(got.astype(f64) - (tile.astype(f64) - wear + deposits)).max()
    print("%s: residual %.3e (bound %.3e)" % (name, resid, bound))
    assert resid <= bound


def test_no_wear_where_no_water_has_been():
    # no water to start with and rain on the east half only: water and flux spread one cell per iteration (every step is a
    # radius-1 stencil), and a cell erodes in the iteration the water reaches it at the earliest (its discharge reads the
    # neighbours' flux of the same iteration).  After n iterations columns x < 32 - n are dry and unworn.
    h, n = relief(64), 20
    rm = np.zeros_like(h)
    rm[:, 32:] = 1.0
    got, water, wear, deposits = X.run(h, n, initialWater=0.0, rainMap=rm)
    dry = slice(0, 32 - n)
    assert not water[:, dry].any() and not wear[:, dry].any() and not deposits[:, dry].any()
    assert np.array_equal(got[:, dry], h[:, dry])
    assert wear[:, 32:].any() and water[:, 32:].any()


def test_the_abi_exports_and_binds_the_extension(nj):
    N = nj._native
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    # nz_hydraulic_desc field by field against the header and the C# struct
    hdr = open(os.path.join(ROOT, "include", "noize_hip.h")).read()
    body = re.search(r"typedef struct nz_hydraulic_desc \{(.*?)\} nz_hydraulic_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if "*" in decl:  # one plane per declaration
            c_fields.append(("ptr", decl.rsplit("*", 1)[1].strip()))
        elif decl:
            ctype, rest = decl.split(" ", 1)
            c_fields += [(ctype, n.strip()) for n in rest.split(",")]
    kind = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "ptr": ctypes.c_void_p}
    assert [(n, kind[t]) for t, n in c_fields] == list(N.HydraulicDesc._fields_)
    assert [n for _, n in c_fields] == ["iterations", "initialWater", "rain", "evaporation", "capacity", "dissolve", "deposit",
                                        "minTilt", "border", "rainMap", "hardness", "wear", "deposits"]
    assert ctypes.sizeof(N.HydraulicDesc) == 72 and N.HydraulicDesc.rainMap.offset == 40
    cs = open(os.path.join(ROOT, "host-cs", "Runtime.cs")).read()
    cs_body = re.search(r"public struct NzHydraulicDesc\s*\{(.*?)\}", cs, re.S).group(1)
    cs_fields = []
    for t, names in re.findall(r"public\s+(\w+)\s+([^;]+);", cs_body):
        cs_fields += [(t, n.strip()) for n in names.split(",")]
    cs_kind = {"int32_t": "int", "float": "float", "ptr": "IntPtr"}
    assert cs_fields == [(cs_kind[t], n) for t, n in c_fields]
    assert (N.NZ_HYDRAULIC_BORDER_CLOSED, N.NZ_HYDRAULIC_BORDER_OPEN) == (0, 1)
    assert "NZ_HYDRAULIC_BORDER_CLOSED = 0, NZ_HYDRAULIC_BORDER_OPEN = 1" in hdr
    native_cs = open(os.path.join(ROOT, "host-cs", "Native.cs")).read()
    for name in ENTRIES:
        assert re.search(r" %s\(IntPtr ctx, [^)]*ref NzHydraulicDesc desc" % name, native_cs), name


def test_every_host_has_the_extension(nj):
    assert "HydraulicBorder" in nj.__all__ and int(nj.HydraulicBorder.Closed) == 0 and int(nj.HydraulicBorder.Open) == 1
    import inspect
    params = list(inspect.signature(nj.HydraulicErosionStage.__init__).parameters)
    assert params[-4:] == ["border", "rainMap", "hardness", "recordMasks"] and params[2:10] == ["iterations"] + list(NAMES)
    hpp = open(os.path.join(ROOT, "noize_job_amd", "host", "noize_pipeline.hpp")).read()
    cs = open(os.path.join(ROOT, "host-cs", "Stages", "Stages.cs")).read()
    assert "enum class HydraulicBorder { Closed, Open }" in hpp and re.search(r"enum HydraulicBorder\s*\{\s*Closed\s*=\s*0,\s*Open\s*=\s*1\s*\}", cs)
    for member in ("border", "rainMap", "hardness", "recordMasks"):
        assert re.search(r"\b%s\b" % member, hpp[hpp.index("class HydraulicErosionStage"):]), member
        assert re.search(r"public [\w.]+ %s\b" % member, cs[cs.index("class HydraulicErosionStage"):]), member
    for entry in ENTRIES:
        assert entry + "(" in hpp and "Native." + entry + "(" in cs, entry
    # with every option at its default the hosts still call the plain entries
    for entry in ("nz_hydraulic_erosion_stage(", "nz_hydraulic_erosion_stage_rw(", "nz_hydraulic_erosion_stage_batch("):
        assert entry in hpp and "Native." + entry in cs, entry
