"""The C++ host's stage classes (noize_job_amd/host/noize_pipeline.hpp) run on the device by host_demo's `stage` mode
(host_demo_stages.hpp), one scenario per class, one process per scenario, every plane bit for bit against the numpy model
the stage's Python test uses (tests/*_ref.py) on the tiles those tests use: tile(97) of test_gpu_drainage_mfd and
terraces16 of terrain_tiles.  The steps of a scenario: a accessors before any payload, b the defaults through a
BasePipeline, t the tie tile, c every option (c2: an option off again), d2 / d3 / d1 the READ / WRITE pair with an even and
an odd count and no WRITE plane, e96 / e32 / e33 one instance on 96^2, 9 x 32^2 (equal length, another tiling) and
3 x 33^2, f a budget of 2 (f2: the implicit stages' drainage out of budget in front of a trivial solve), g OnDestroy, h one
more payload.  The one-call stages: s1, s2, s3."""
import os
import subprocess
import time

import numpy as np
import pytest

import drainage_mfd_ref as M
import drainage_ref as D
import fill_ref
import fluvial_implicit_mfd_ref as RM
import fluvial_implicit_ref as R
import fluvial_ref as F
import hillslope_ref
import hydraulic_ex_ref as X
import hydraulic_ref as H
import stream_order_ref as S
import terrain_tiles as T
import watershed_ref as W
from test_gpu_drainage_mfd import rain_map, tile
from test_gpu_slab import memo

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "noize_job_amd", "host", "host_demo")
TERRAIN = ["HydraulicErosionStage", "FluvialErosionStage", "DrainageAreaStage", "MfdDrainageStage", "WatershedStage",
           "StreamOrderStage", "ImplicitFluvialStage", "MfdFluvialStage", "HillslopeDiffusionStage"]
ONE_CALL = ["ShapedNoiseStage", "WarpedNoiseStage", "StageGaussianBlur", "StageSmoothBlur", "ConstantStage", "CurveStage",
            "StageThermalErosion", "CropStage", "UpsampleStage", "DownsampleStage", "MeshTileStage"]
SCENARIOS = TERRAIN + ONE_CALL
OFF = float(F.SEA_OFF)
SEA = 0.4          # host_demo_stages.hpp: SEA, AMPLE, SENTINEL
AMPLE = 600
DTYPES = {"f32": f32, "i32": np.int32, "u8": np.uint8}
BROKEN = []        # the reason every later test of the file skips: a process that ended on a signal or an abort


# ---- the process ---------------------------------------------------------------------------------------------------------
class Output:
    def __init__(self, planes, values):
        self.planes, self.values = planes, values

    def plane(self, name, shape):
        assert name in self.planes, "%s is not among the planes %s" % (name, sorted(self.planes))
        return self.planes[name].reshape(shape)

    def value(self, name):
        assert name in self.values, "%s is not among the values %s" % (name, sorted(self.values))
        return self.values[name]


def run_scenario(name, planes, tmp_path):
    """host_demo once on the planes (float32 arrays, in the order the scenario documents) -> Output."""
    if BROKEN:
        pytest.skip(BROKEN[0])
    assert os.path.exists(EXE), "host_demo not built (run __graft_entry__.build())"
    src, out = str(tmp_path / "in.f32"), str(tmp_path / "out.bin")
    np.concatenate([np.ascontiguousarray(p, f32).ravel() for p in planes]).tofile(src)
    t0 = time.perf_counter()
    p = subprocess.run([EXE, "0", out, "stage", name, src], timeout=120, capture_output=True, text=True)
    print("host_demo stage %s: %.2f s" % (name, time.perf_counter() - t0))
    if p.returncode < 0 or p.returncode in (134, 137, 139):
        BROKEN.append("host_demo stage %s ended with status %d: %s" % (name, p.returncode, p.stderr[-400:]))
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    raw = np.fromfile(out, np.uint8)
    got, values, at = {}, {}, 0
    for line in p.stdout.splitlines():
        w = line.split()
        if w[0] == "plane":
            assert w[1] not in got, "plane %s twice" % w[1]
            n = int(w[3]) * np.dtype(DTYPES[w[2]]).itemsize
            got[w[1]] = raw[at:at + n].view(DTYPES[w[2]])
            at += n
        else:
            assert w[0] == "value" and w[1] not in values, line
            values[w[1]] = int(w[2])
    assert at == raw.size, "out.bin holds %d bytes, the plane lines describe %d" % (raw.size, at)
    return Output(got, values)


def same(got, want, what):
    """Bit for bit on uint32 views for float planes, array_equal for int32 and byte planes."""
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == f32:
        assert want.dtype == f32, what
        bad = got.view(np.uint32) != want.view(np.uint32)
    else:
        assert np.issubdtype(want.dtype, np.integer), what
        bad = got != want
    assert not bad.any(), "%s: %d/%d cells differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


# ---- the tiles -----------------------------------------------------------------------------------------------------------
def tiles(filled):
    """{"h97", "h96", "h32" (9), "h33" (3), "ties"}: tile(97), its 96^2 corner, that corner's nine 32^2 blocks, three 33^2
    windows of it, and terraces16; `filled`: each flooded on its own, as behind a DepressionFillStage."""
    def make():
        h = tile(97)
        h96 = np.ascontiguousarray(h[:96, :96])
        t = {"h97": h, "h96": h96,
             "h32": np.stack([h96[32 * z:32 * z + 32, 32 * x:32 * x + 32] for z in range(3) for x in range(3)]),
             "h33": np.stack([h[:33, :33], h[32:65, 30:63], h[64:, 64:]]),
             "ties": np.ascontiguousarray(T.GENERATORS["terraces16"](97, np.random.default_rng(5)), f32)}
        if filled:
            t["serpentine"] = T.serpentine_tile()  # one channel of some 1 500 cells that winds across every tile edge
            flood = lambda a: fill_ref.flood(np.ascontiguousarray(a, f32))  # noqa: E731
            t = {k: np.stack([flood(x) for x in v]) if v.ndim == 3 else flood(v) for k, v in t.items()}
        return {k: np.ascontiguousarray(v, f32) for k, v in t.items()}
    return memo(("cpp host tiles", filled), make)


def terrain_input(t, maps):
    zero = np.zeros((97, 97), f32)
    return [t["h97"], t["h96"], t["h32"], t["h33"], t["ties"]] + [m if m is not None else zero for m in maps]


PAYLOADS = {"b": ("h97", 97, 1), "t": ("ties", 97, 1), "c": ("h97", 97, 1), "c2": ("h97", 97, 1), "cm": ("h97", 97, 1),
            "d2": ("h97", 97, 1), "d3": ("h97", 97, 1), "d1": ("h97", 97, 1), "e96": ("h96", 96, 1), "e32": ("h32", 32, 9),
            "e33": ("h33", 33, 3), "f": ("h97", 97, 1), "fm": ("h97", 97, 1), "f2": ("serpentine", 97, 1), "h": ("h33", 33, 1)}


def payload(t, step):
    """The host planes of a step as (count, res, res), and its key for memoised models."""
    name, res, count = PAYLOADS[step]
    h = t[name]
    h = h[None] if h.ndim == 2 else h[:count]
    return h, (name, count)


def per_tile(o, step, what, count, res):
    return o.plane("%s.%s" % (step, what), (count, res, res))


def reads_only(o, t, steps, what="height"):
    """The stage passes the heights through: "<step>.height" is the payload."""
    for step in steps:
        h, _ = payload(t, step)
        same(o.plane("%s.%s" % (step, what), h.shape), h, "%s: the heights pass through" % step)


def pair_facts(o, implicit):
    """Step d: with a WRITE plane `data` and `write` are the two planes of the pair (the implicit stages: `data` is the
    first plane exactly after an even count); without one the result is in the payload's own plane."""
    for n in (2, 3):
        assert o.value("d%d.pair_kept" % n) == 1
        if implicit:
            assert o.value("d%d.data_is_first" % n) == (1 if n % 2 == 0 else 0)
    assert o.value("d1.data_is_first") == 1 and o.value("d1.write_null") == 1


def work_follows(o, sizes_differ=True):
    """Step e: the work buffer has the entry's own size for every tiling, and 96^2 and 9 x 32^2 -- equal length -- need
    different sizes, so a stage that looks at the length alone keeps a stale buffer."""
    for step in ("e96", "e32", "e33"):
        assert o.value(step + ".work_floats") == o.value(step + ".work_need") > 0, step
    if sizes_differ:
        assert o.value("e96.work_need") != o.value("e32.work_need")


# ---- HydraulicErosionStage -------------------------------------------------------------------------------------------------
def hydraulic_maps():
    def make():
        rng = np.random.default_rng(31)  # test_gpu_hydraulic_ex.maps_for: rain in [0, 2], hardness in [0, 1] with exact ends
        rain = (rng.random((97, 97), dtype=f32) * f32(2.0)).astype(f32)
        return rain, np.clip(rng.random((97, 97), dtype=f32) * f32(1.5) - f32(0.25), 0.0, 1.0).astype(f32)
    return memo("cpp host hydraulic maps", make)


def test_hydraulic_erosion_stage(tmp_path):
    t = tiles(False)
    rain, hard = hydraulic_maps()
    o = run_scenario("HydraulicErosionStage", terrain_input(t, [rain, hard, None, None]), tmp_path)
    assert (o.value("a.water_null"), o.value("a.wear_null"), o.value("a.deposits_null")) == (1, 1, 1)
    for step, its in (("b", 8), ("t", 8), ("d2", 2), ("d3", 3), ("d1", 3), ("e96", 4), ("e32", 4), ("e33", 4), ("h", 4)):
        h, key = payload(t, step)
        assert (o.value(step + ".water_null"), o.value(step + ".wear_null"), o.value(step + ".deposits_null")) == (0, 1, 1)
        for k in range(h.shape[0]):
            want = memo(("cpp host hydraulic", key, k, its), lambda: H.run(h[k], its))
            same(per_tile(o, step, "height", *h.shape[:2])[k], want[0], "%s tile %d: heights" % (step, k))
            same(per_tile(o, step, "water", *h.shape[:2])[k], want[1], "%s tile %d: water" % (step, k))
    want = X.run(t["h97"], 7, capacity=2.0, border=X.OPEN, rainMap=rain, hardness=hard)
    for step in ("c", "c2"):
        same(o.plane(step + ".height", (97, 97)), want[0], step + ": heights")
        same(o.plane(step + ".water", (97, 97)), want[1], step + ": water")
    assert (o.value("c.wear_null"), o.value("c.deposits_null")) == (0, 0)
    same(o.plane("c.wear", (97, 97)), want[2], "c: wear")
    same(o.plane("c.deposits", (97, 97)), want[3], "c: deposits")
    assert (o.value("c2.wear_null"), o.value("c2.deposits_null")) == (1, 1)  # recordMasks off again
    same(o.plane("c2.rainMap", (97, 97)), rain, "the rain map is read only")
    same(o.plane("c2.hardness", (97, 97)), hard, "the hardness is read only")
    pair_facts(o, False)
    assert (o.value("g.water_null"), o.value("g.wear_null"), o.value("g.deposits_null")) == (1, 1, 1)


# ---- FluvialErosionStage ---------------------------------------------------------------------------------------------------
def test_fluvial_erosion_stage(tmp_path):
    t = tiles(False)
    hard, upl = R_maps()
    rm = rain_map(97)
    warm = memo("cpp host fluvial warm start", lambda: D.accumulate(t["h97"], 0.75, SEA, rm)[0])
    o = run_scenario("FluvialErosionStage", terrain_input(t, [rm, hard, upl, warm]), tmp_path)
    assert o.value("a.drainage_null") == 1
    for step, its in (("b", 8), ("t", 8), ("d2", 2), ("d3", 3), ("d1", 3), ("e96", 4), ("e32", 4), ("e33", 4), ("h", 4)):
        h, key = payload(t, step)
        assert o.value(step + ".drainage_null") == 0
        for k in range(h.shape[0]):
            want = memo(("cpp host fluvial", key, k, its), lambda: F.run(h[k], its))
            same(per_tile(o, step, "height", *h.shape[:2])[k], want[0], "%s tile %d: heights" % (step, k))
            same(per_tile(o, step, "drainage", *h.shape[:2])[k], want[1], "%s tile %d: drainage" % (step, k))
    want = F.run(t["h97"], 5, erodibility=0.1, uplift=0.004, dt=0.5, rain=0.75, seaLevel=SEA, rainMap=rm, hardness=hard,
                 upliftMap=upl, drainageIn=warm)
    same(o.plane("c.height", (97, 97)), want[0], "c: heights")
    same(o.plane("c.drainage", (97, 97)), want[1], "c: drainage")
    for k, m in enumerate((rm, hard, upl, warm)):
        same(o.plane("c.m%d" % k, (97, 97)), m, "c: map %d is read only" % k)
    pair_facts(o, False)
    assert o.value("g.drainage_null") == 1


def R_maps():
    """(hardness in [0, 1), upliftMap in [0, 2)) at 97^2: test_gpu_fluvial_implicit.maps."""
    def make():
        rng = np.random.default_rng(100 + 97)
        return rng.random((97, 97), dtype=f32), (rng.random((97, 97), dtype=f32) * f32(2.0)).astype(f32)
    return memo("cpp host implicit maps", make)


# ---- DrainageAreaStage, MfdDrainageStage -----------------------------------------------------------------------------------
def drainage_like(name, tmp_path, walk, budget, mfd):
    """walk(h, rain, sea, rainMap, exponent) -> (A, height of the flow graph)."""
    t = tiles(True)
    rm = rain_map(97)
    o = run_scenario(name, terrain_input(t, [rm, None, None, None]), tmp_path)
    assert (o.value("a.drainage_null"), o.value("a.passes"), o.value("a.converged"), o.value("a.work_floats")) == (1, -1, 0, 0)
    reads_only(o, t, ("b", "t", "c", "c2", "e96", "e32", "e33", "f", "h"))
    for step, args in (("b", (1.0, OFF, None, 1)), ("t", (1.0, OFF, None, 1)), ("c", (0.5, SEA, rm, 4)), ("c2", (0.5, SEA, None, 4)),
                       ("e96", (1.0, OFF, None, 2)), ("e32", (1.0, OFF, None, 2)), ("e33", (1.0, OFF, None, 2)),
                       ("h", (1.0, OFF, None, 2))):
        h, key = payload(t, step)
        if not mfd:
            args = args[:3] + (1,)
        heights = []
        for k in range(h.shape[0]):
            want, height = memo(("cpp host drainage", name, key, k, args[0], args[1], args[2] is not None, args[3]),
                                lambda: walk(h[k], *args))
            heights.append(height)
            same(per_tile(o, step, "drainage", *h.shape[:2])[k], want, "%s tile %d" % (step, k))
        assert o.value(step + ".converged") == 1 and 1 <= o.value(step + ".passes") <= min(
            max(heights) + 1, AMPLE if step in ("c", "c2") else budget(h.shape[1])), (step, o.value(step + ".passes"), heights)
    assert (o.value("c.drainage_is_out"), o.value("c2.drainage_is_out")) == (1, 0)
    same(o.plane("c2.out", (97, 97)), o.plane("c.drainage", (97, 97)), "the caller's plane after it was taken away")
    same(o.plane("c.rainMap", (97, 97)), rm, "the rain map is read only")
    work_follows(o)
    assert (o.value("f.converged"), o.value("f.passes")) == (0, 2)
    same(o.plane("f.drainage", (97, 97)), np.ones((97, 97), f32), "a budget of 2: rain everywhere")
    assert (o.value("g.drainage_null"), o.value("g.passes"), o.value("g.converged"), o.value("g.work_floats")) == (1, -1, 0, 0)


def test_drainage_area_stage(tmp_path):
    drainage_like("DrainageAreaStage", tmp_path, lambda h, rain, sea, rm, e: D.accumulate(h, rain, sea, rm),
                  lambda res: 64 + res // 4, False)


def test_mfd_drainage_stage(tmp_path):
    drainage_like("MfdDrainageStage", tmp_path, M.walk, lambda res: 128 + res // 2, True)


# ---- WatershedStage ----------------------------------------------------------------------------------------------------------
def test_watershed_stage(tmp_path):
    t = tiles(True)
    o = run_scenario("WatershedStage", terrain_input(t, [None] * 4), tmp_path)
    empty = ("basin_null", "length_null", "receivers_null")
    for step in ("a", "g"):
        assert tuple(o.value("%s.%s" % (step, k)) for k in empty) == (1, 1, 1)
        assert (o.value(step + ".passes"), o.value(step + ".converged"), o.value(step + ".work_floats")) == (-1, 0, 0)
    reads_only(o, t, ("b", "t", "c", "c2", "e96", "e32", "e33", "f", "h"))
    # (sea, cellSize, length, receivers) of every step
    for step, (sea, cs, length, receivers) in (("b", (OFF, 1.0, True, False)), ("t", (OFF, 1.0, True, False)),
                                               ("c", (SEA, 0.3, False, True)), ("c2", (SEA, 0.3, True, False)),
                                               ("e96", (OFF, 1.0, True, True)), ("e32", (OFF, 1.0, True, True)),
                                               ("e33", (OFF, 1.0, True, True)), ("h", (OFF, 1.0, True, False))):
        h, key = payload(t, step)
        assert tuple(o.value("%s.%s" % (step, k)) for k in empty) == (0, 0 if length else 1, 0 if receivers else 1), step
        hops = []
        for k in range(h.shape[0]):
            wb, wl, hp, wr = memo(("cpp host watershed", key, k, sea, cs), lambda: W.walk(h[k], sea, cs) + (F.receivers(h[k], sea)[0],))
            hops.append(int(hp.max()))
            same(per_tile(o, step, "basin", *h.shape[:2])[k], wb, "%s tile %d: basin" % (step, k))
            if length:
                same(per_tile(o, step, "length", *h.shape[:2])[k], wl, "%s tile %d: length" % (step, k))
            if receivers:
                same(per_tile(o, step, "receivers", *h.shape[:2])[k], wr, "%s tile %d: receivers" % (step, k))
        assert o.value(step + ".converged") == 1 and 1 <= o.value(step + ".passes") <= min(
            max(hops) + 2, AMPLE if step in ("c", "c2") else 64 + h.shape[1] // 4), (step, o.value(step + ".passes"), hops)
    work_follows(o)
    assert (o.value("f.converged"), o.value("f.passes")) == (0, 2)
    same(o.plane("f.basin", (97, 97)), np.arange(97 * 97, dtype=np.int32).reshape(97, 97), "a budget of 2: labels")
    assert not o.plane("f.length", (97, 97)).any() and o.value("f.receivers_null") == 1


# ---- StreamOrderStage --------------------------------------------------------------------------------------------------------
def test_stream_order_stage(tmp_path):
    t = tiles(True)
    area = memo("cpp host stream order area", lambda: D.accumulate(t["h97"])[0])
    o = run_scenario("StreamOrderStage", terrain_input(t, [area, None, None, None]), tmp_path)
    for step in ("a", "g"):
        assert (o.value(step + ".order_null"), o.value(step + ".links_null")) == (1, 1)
        assert (o.value(step + ".passes"), o.value(step + ".converged"), o.value(step + ".work_floats")) == (-1, 0, 0)
    reads_only(o, t, ("b", "t", "c", "c2", "e96", "e32", "e33", "f", "h"))
    # (sea, drainage, threshold, links) of every step
    for step, (sea, dr, thr, links) in (("b", (OFF, None, 0.0, False)), ("t", (OFF, None, 0.0, False)),
                                        ("c", (SEA, area, 6.0, True)), ("c2", (SEA, area, 6.0, False)),
                                        ("e96", (OFF, None, 0.0, True)), ("e32", (OFF, None, 0.0, True)),
                                        ("e33", (OFF, None, 0.0, True)), ("h", (OFF, None, 0.0, True))):
        h, key = payload(t, step)
        assert (o.value(step + ".order_null"), o.value(step + ".links_null")) == (0, 0 if links else 1), step
        chains = []
        for k in range(h.shape[0]):
            wo, wl, chain = memo(("cpp host stream order", key, k, sea, dr is not None, thr), lambda: S.walk(h[k], sea, dr, thr))
            chains.append(chain)
            same(per_tile(o, step, "order", *h.shape[:2])[k], wo, "%s tile %d: order" % (step, k))
            if links:
                same(per_tile(o, step, "links", *h.shape[:2])[k], wl, "%s tile %d: links" % (step, k))
        assert o.value(step + ".converged") == 1 and 1 <= o.value(step + ".passes") <= min(
            max(chains) + 2, AMPLE if step in ("c", "c2") else 64 + h.shape[1] // 4), (step, o.value(step + ".passes"), chains)
    wo = S.walk(t["h97"], SEA, area, 6.0)[0]
    assert 0 < (wo > 0).sum() < 97 * 97 and wo.max() >= 2  # a proper sub-network
    same(o.plane("c.drainage", (97, 97)), area, "the drainage is read only")
    work_follows(o)
    assert (o.value("f.converged"), o.value("f.passes")) == (0, 2)
    same(o.plane("f.order", (97, 97)), np.ones((97, 97), np.uint8), "a budget of 2: order")
    same(o.plane("f.links", (97, 97)), np.arange(97 * 97, dtype=np.int32).reshape(97, 97), "a budget of 2: links")


# ---- ImplicitFluvialStage, MfdFluvialStage -----------------------------------------------------------------------------------
def implicit_like(name, tmp_path, chain, budget, mfd):
    """chain(h, iterations, **kw) -> (heights, drainage)."""
    t = tiles(True)
    hard, upl = R_maps()
    rm = rain_map(97)
    o = run_scenario(name, terrain_input(t, [rm, hard, upl, t["serpentine"]]), tmp_path)
    for step in ("a", "g"):
        assert (o.value(step + ".drainage_null"), o.value(step + ".steps"), o.value(step + ".passes"),
                o.value(step + ".work_floats")) == (1, -1, -1, 0)
    options = dict(erodibility=0.1, uplift=0.01, dt=20.0, rain=2.0, seaLevel=SEA, rainMap=rm, hardness=hard, upliftMap=upl)
    e = dict(exponent=2) if mfd else {}
    steps = [("b", 1, {}), ("t", 1, {}), ("c", 1, dict(options, exponent=4) if mfd else options),
             ("d2", 2, dict(dt=50.0, **e)), ("d3", 3, dict(dt=50.0, **e)), ("d1", 3, dict(dt=50.0, **e)),
             ("e96", 2, dict(dt=50.0, **e)), ("e32", 2, dict(dt=50.0, **e)), ("e33", 2, dict(dt=50.0, **e)),
             ("h", 1, dict(dt=50.0, **e))]
    if not mfd:
        steps.append(("cm", 1, dict(options, routing=4)))
    for step, its, kw in steps:
        h, key = payload(t, step)
        for k in range(h.shape[0]):
            tag = tuple(sorted((a, b if np.isscalar(b) else True) for a, b in kw.items()))
            wh, wA = memo(("cpp host implicit", name, key, k, its, tag), lambda: chain(h[k], its, **kw))
            same(per_tile(o, step, "height", *h.shape[:2])[k], wh, "%s tile %d: heights" % (step, k))
            same(per_tile(o, step, "drainage", *h.shape[:2])[k], wA, "%s tile %d: drainage" % (step, k))
            if step == "b":
                assert not R.same(wh, h[k])  # the step moves the heights
        cap = AMPLE if step in ("c", "cm") else budget(h.shape[1])
        assert o.value(step + ".steps") == its and o.value(step + ".converged") == 1, step
        assert 1 <= o.value(step + ".passes") <= its * cap, (step, o.value(step + ".passes"))
    for k, m in enumerate((rm, hard, upl)):
        same(o.plane("c.m%d" % k, (97, 97)), m, "c: map %d is read only" % k)
    pair_facts(o, True)
    work_follows(o)
    # a budget of 2: the drainage series does not converge, no step is applied, the heights are as they were
    for step in ("f",) if mfd else ("f", "fm"):
        assert (o.value(step + ".steps"), o.value(step + ".passes"), o.value(step + ".converged")) == (0, 0, 0), step
        same(o.plane(step + ".height", (97, 97)), t["h97"], step + ", a budget of 2: heights")
        same(o.plane(step + ".drainage", (97, 97)), np.ones((97, 97), f32), step + ", a budget of 2: the drainage's start state")
    # a budget of 3 on the long channel with erodibility 0: the solve alone would be done at once (h + uplift * dt), so only
    # the drainage's converged word -- not its pass count, the word in front of it -- can have held it back
    assert (o.value("f2.steps"), o.value("f2.passes"), o.value("f2.converged")) == (0, 0, 0)
    same(o.plane("f2.height", (97, 97)), t["serpentine"], "a budget of 3 on the long channel: heights")
    same(o.plane("f2.drainage", (97, 97)), np.ones((97, 97), f32), "a budget of 3 on the long channel: drainage")


def steepest_or_multiple(h, iterations, routing=None, **kw):
    """ImplicitFluvialStage's chain: R.chain, or with routing = the flow exponent the multiple-flow area in front of the
    same solve (test_gpu_drainage_mfd.mfd_chain with the options)."""
    if routing is None:
        return R.chain(h, iterations, **kw)
    h = np.array(h, f32)
    solve = {k: v for k, v in kw.items() if k not in ("rain", "rainMap")}
    A = None
    for _ in range(iterations):
        A = M.walk(h, kw.get("rain", 1.0), kw.get("seaLevel", OFF), kw.get("rainMap"), routing)[0]
        h = R.walk(h, A, **solve)
    return h, A


def test_implicit_fluvial_stage(tmp_path):
    implicit_like("ImplicitFluvialStage", tmp_path, steepest_or_multiple, lambda res: 64 + res // 4, False)


def test_mfd_fluvial_stage(tmp_path):
    implicit_like("MfdFluvialStage", tmp_path, RM.chain, lambda res: 128 + res // 2, True)


# ---- HillslopeDiffusionStage ---------------------------------------------------------------------------------------------------
def test_hillslope_diffusion_stage(tmp_path):
    t = tiles(False)
    o = run_scenario("HillslopeDiffusionStage", terrain_input(t, [None] * 4), tmp_path)
    assert o.value("a.work_floats") == 0 == o.value("g.work_floats")
    for step, args in (("b", (0.01, 1.0, 1)), ("t", (0.01, 1.0, 1)), ("c", (2.5, 4.0, 3)), ("e96", (2.5, 4.0, 3)),
                       ("e32", (2.5, 4.0, 3)), ("e33", (2.5, 4.0, 3)), ("h", (2.5, 4.0, 3))):
        h, key = payload(t, step)
        for k in range(h.shape[0]):
            want = memo(("cpp host hillslope", key, k, args), lambda: hillslope_ref.diffuse(h[k], *args))
            same(per_tile(o, step, "height", *h.shape[:2])[k], want, "%s tile %d" % (step, k))
    assert not hillslope_ref.same(hillslope_ref.diffuse(t["h97"], 0.01, 1.0, 1), t["h97"])
    work_follows(o, sizes_differ=False)  # the two tables depend on the resolution alone
    assert o.value("e96.work_floats") != o.value("e32.work_floats")


# ---- the one-call stages: s1, s2, ... are payloads through one instance; the comparisons of the stage's Python test ---------
def field(o, step, resolution, count=1, pos=None):
    """What TransformData (or nothing) made of the payload's fields."""
    assert (o.value(step + ".resolution"), o.value(step + ".count")) == (resolution, count), step
    assert o.value(step + ".length") == count * resolution * resolution, step
    if pos is not None and count == 1:
        assert (o.value(step + ".xpos"), o.value(step + ".zpos")) == pos, step
    elif pos is not None:
        assert o.plane(step + ".positions", (count, 2)).tolist() == pos, step
    return o.plane(step + ".data", (count, resolution, resolution) if count > 1 else (resolution, resolution))


def uniform(shape, seed):
    return memo(("cpp host uniform", shape, seed), lambda: np.random.default_rng(seed).random(shape, dtype=f32))


def test_constant_stage(oracle, tmp_path):
    a = (uniform((130, 130), 21) * f32(1.4) - f32(0.2)).astype(f32)  # test_constant_reduce_curve_stages' plane
    b = uniform((33, 33), 22)
    o = run_scenario("ConstantStage", [a, b], tmp_path)
    same(field(o, "s1", 130), oracle.constant(a, 0, 0.37), "MULTIPLY")
    same(field(o, "s2", 130), oracle.constant(a, 1, 0.37), "BINARIZE")
    same(field(o, "s3", 33), oracle.constant(b, 0, -1.5), "MULTIPLY on another length")


def test_curve_stage(oracle, tmp_path):
    a = (uniform((130, 130), 21) * f32(1.4) - f32(0.2)).astype(f32)
    b = uniform((33, 33), 22)
    o = run_scenario("CurveStage", [a, b], tmp_path)
    table = lambda fn, n: np.array([fn(f32(i) / f32(n)) for i in range(n)], f32)  # noqa: E731
    smooth = table(lambda t: t * t * (f32(3.0) - f32(2.0) * t), 64)
    for step in ("s1", "s2"):
        same(field(o, step, 130), oracle.curve(a, smooth), step + ": smoothstep in 64 samples")
    same(field(o, "s3", 33), oracle.curve(b, table(lambda t: f32(1.5) * t - f32(0.1), 7)), "a line in 7 samples")


def test_thermal_erosion_stage(oracle, tmp_path):
    a, b = uniform((65, 65), 65), uniform((33, 33), 33)
    o = run_scenario("StageThermalErosion", [a, b], tmp_path)
    same(field(o, "s1", 65), oracle.thermal_erosion(a, 20.0, 0.25, 0.3, 3), "65^2")
    same(field(o, "s2", 33), oracle.thermal_erosion(b, 80.0, 0.5, 2.0, 2), "33^2")


def test_crop_stage(oracle, tmp_path):
    a = uniform((150, 150), 5)
    o = run_scenario("CropStage", [a], tmp_path)
    for step, res in (("s1", 64), ("s2", 161)):
        same(o.plane(step + ".data", (res, res)), oracle.crop(a, res), "cropped to %d" % res)
        same(o.plane(step + ".input", (150, 150)), a, "the input is read only")


def test_gaussian_blur_stage(oracle, tmp_path):
    a, b = uniform((90, 90), 90), uniform((3, 37, 37), 37)
    o = run_scenario("StageGaussianBlur", [a, b], tmp_path)
    same(field(o, "s1", 90), oracle.gauss(a, oracle.limit_width(4), 1, 3), "an even width")
    got = field(o, "s2", 37, 3)
    for k in range(3):
        same(got[k], oracle.gauss(b[k], 13, 5, 2), "batch tile %d" % k)
    same(field(o, "s3", 90), oracle.gauss(a, 9, 3, 2), "with a WRITE plane")
    assert o.value("s3.pair_kept") == 1


def test_smooth_blur_stage(oracle, tmp_path):
    a, b = uniform((77, 77), 77), uniform((33, 33), 33)
    o = run_scenario("StageSmoothBlur", [a, b], tmp_path)
    same(field(o, "s1", 77), oracle.smooth(a, 7, 2), "width 7")
    same(field(o, "s2", 33), oracle.smooth(b, 25, 1), "width 25 on another length")
    same(field(o, "s3", 77), oracle.smooth(a, oracle.limit_width(6), 3), "an even width with a WRITE plane")
    assert o.value("s3.pair_kept") == 1


NOISE_POSITIONS = [[0, 0], [-4096, 512], [300000, -70000]]  # host_demo_stages.hpp: noise_positions()


def test_shaped_noise_stage(tmp_path):
    from fractal_shapes_ref import BILLOW, RIDGED, fractal_shaped
    o = run_scenario("ShapedNoiseStage", [np.zeros(0, f32)], tmp_path)
    first = (0.5938, 1.3, 1.9168, 0.0317, 6)
    want = fractal_shaped(3, 61, 61, *first, -2100, -777, 97, shape=RIDGED, offset=0.9, gain=3.5)
    same(field(o, "s1", 61, pos=(-2100, -777)), want, "Simplex, ridged")
    second = (0.45, 1.0, 2.0, 0.01, 9)
    got = field(o, "s2", 64, 3, NOISE_POSITIONS)
    for k, (xp, zp) in enumerate(NOISE_POSITIONS):
        same(got[k], fractal_shaped(5, 64, 64, *second, xp, zp, 700, shape=BILLOW), "Cellular, billow: batch tile %d" % k)
    same(field(o, "s3", 40, pos=(300000, 2000)), fractal_shaped(5, 40, 40, *second, 300000, 2000, 700, shape=BILLOW),
         "another length")


def test_warped_noise_stage(tmp_path):
    from fractal_shapes_ref import FBM, RIDGED
    from fractal_warp_ref import fractal_warped
    o = run_scenario("WarpedNoiseStage", [np.zeros(0, f32)], tmp_path)
    first = (0.5938, 1.3, 1.9168, 0.0317, 6)
    want = fractal_warped(4, 40, 40, *first, -2100, -777, 97, shape=RIDGED, warp_strength=-200.0, warp_scale=0.25, warp_octaves=2)
    same(field(o, "s1", 40, pos=(-2100, -777)), want, "RotatedSimplex, ridged")
    second = (0.45, 1.0, 2.0, 0.01, 9)
    warp = dict(shape=FBM, warp_strength=37.5, warp_scale=1.0, warp_octaves=3)
    got = field(o, "s2", 64, 3, NOISE_POSITIONS)
    for k, (xp, zp) in enumerate(NOISE_POSITIONS):
        same(got[k], fractal_warped(3, 64, 64, *second, xp, zp, 700, **warp), "Simplex, fBm: batch tile %d" % k)
    same(field(o, "s3", 61, pos=(0, 0)), fractal_warped(3, 61, 61, *second, 0, 0, 700, **warp), "another length")


RESAMPLE_POSITIONS = [[0, 0], [64, -64], [-130, 7]]  # host_demo_stages.hpp: resample_positions()


def test_upsample_stage(tmp_path):
    import resample_ref as RS
    a, b, base = uniform((37, 37), 1), uniform((3, 16, 16), 2), uniform((74, 74), 3)
    o = run_scenario("UpsampleStage", [a, b, base], tmp_path)
    same(field(o, "s1", 74, pos=(12, -10)), RS.upsample(a, 2, RS.BILINEAR, base), "factor 2, bilinear, a base plane")
    assert o.value("s1.data_is_output") == 1
    same(o.plane("s1.input", (37, 37)), a, "the input is read only")
    same(o.plane("s1.base", (74, 74)), base, "the base is read only")
    got = field(o, "s2", 64, 3, [[4 * x, 4 * z] for x, z in RESAMPLE_POSITIONS])
    for k in range(3):
        same(got[k], RS.upsample(b[k], 4, RS.NEAREST), "factor 4, nearest: batch tile %d" % k)
    same(o.plane("s2.input", (3, 16, 16)), b, "the batch is read only")
    up = RS.upsample(a, 2, RS.CATMULL_ROM)
    same(o.plane("s3.middle", (74, 74)), up, "up, then down: the plane in between")
    same(field(o, "s3", 37, pos=(6, -5)), RS.downsample(up, 2), "up, then down")
    assert o.value("g.output_null") == 1


def test_downsample_stage(tmp_path):
    import resample_ref as RS
    a, b = uniform((64, 64), 4), uniform((3, 32, 32), 5)
    o = run_scenario("DownsampleStage", [a, b], tmp_path)
    same(field(o, "s1", 32, pos=(3, -3)), RS.downsample(a, 2), "factor 2")
    assert o.value("s1.data_is_output") == 1
    same(o.plane("s1.input", (64, 64)), a, "the input is read only")
    got = field(o, "s2", 8, 3, [[x // 4, z // 4] for x, z in RESAMPLE_POSITIONS])
    for k in range(3):
        same(got[k], RS.downsample(b[k], 4), "factor 4: batch tile %d" % k)
    same(o.plane("s2.input", (3, 32, 32)), b, "the batch is read only")
    down = RS.downsample(a, 2)
    same(o.plane("s3.middle", (32, 32)), down, "down, then up: the plane in between")
    same(field(o, "s3", 64, pos=(6, -6)), RS.upsample(down, 2, RS.CATMULL_ROM), "down, then up")
    assert o.value("g.output_null") == 1


def test_mesh_tile_stage(oracle, tmp_path):
    a, b = uniform((35, 35), 33), uniform((4, 72, 72), 64)
    o = run_scenario("MeshTileStage", [a, b], tmp_path)
    v, i = oracle.mesh_heightmap(0, a, 33, 1, 25.0, 100.0)
    assert (o.value("s1.vertex_count"), o.value("s1.index_count")) == (len(v), len(i))
    same(o.plane("s1.vertices", v.shape), np.ascontiguousarray(v, f32), "square grid: vertices")
    assert np.array_equal(o.plane("s1.indices", i.shape).view(np.uint32), i), "square grid: indices"
    same(o.plane("s1.input", (35, 35)), a, "the heights are read only")
    vtx = o.plane("s2.vertices", (4, -1, 12))
    idx = o.plane("s2.indices", (4, -1)).view(np.uint32)
    for k in range(4):
        v, i = oracle.mesh_heightmap(1, b[k], 64, 4, 25.0, 100.0)
        same(vtx[k], np.ascontiguousarray(v, f32), "overshoot, batch tile %d: vertices" % k)
        assert np.array_equal(idx[k], i), "overshoot, batch tile %d: indices" % k
    assert (o.value("s2.vertex_count"), o.value("s2.index_count")) == (vtx.shape[0] * vtx.shape[1], idx.size)
    same(o.plane("s2.input", (4, 72, 72)), b, "the heights are read only")
