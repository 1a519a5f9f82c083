"""The seven iterate-to-rest entries (nz_fill_depressions, nz_drainage_area, nz_drainage_mfd, nz_watershed, nz_stream_order,
nz_fluvial_implicit, nz_fluvial_implicit_mfd, each single and _batch) against tests/relax_schedule.py, the pass protocol and
tile schedule in numpy: not only the walk's bits, which cannot show a broken skip or gate, but the exact pass count, the
verdict, the pass at which a budget cuts the series, and the per-tile bytes each pass leaves in `work`.  Everything compared
is an integer or a bit pattern.

  1. ordinary tiles   passes, converged and planes on the usual tiles at 66^2, 97^2 and 130^2, at sweep caps 1, 3 and 16,
                      single and as a batch
  2. wake-up tiles    every tile of relax_schedule.wake_tiles() -- a front that crosses a tile corner while both edge
                      neighbours rest, in the four directions, and tiles woken through an edge after an odd and an even
                      rest -- ends in the walk's bits with the model's count, at caps 16 and 3, alone and with the tiles of
                      one resolution stacked into one _batch call.  test_relax_schedule.py shows that a skip rule without
                      the diagonals, or without neighbours, loses each of them
  3. batch isolation  [quiet, wake-up tile, quiet] and [wake-up tile, quiet, the tile mirrored]: the tile bytes of the
                      planes are neighbours in memory and not in the plane
  4. budget           maxPasses one short of the model's count: converged 0 and the all-or-nothing result in every plane; the
                      count: converged.  Single calls, and batches whose planes come to rest at different passes
  5. tile bytes       a run cut at p passes leaves the byte generations of passes p - 1 and p - 2 in `work`; they are the
                      model's moved maps, for p = 1, 2, mid-series and the last pass, single and for a batch of three"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import relax_schedule as R
import test_gpu_drainage as TD
import test_gpu_drainage_mfd as TM
import test_gpu_fill as TF
import test_gpu_fluvial_implicit as TI
import test_gpu_fluvial_implicit_mfd as TIM
import test_gpu_stream_order as TS
import test_gpu_watershed as TW
from test_gpu_slab import memo
from test_relax_schedule import CAPS, FAMILIES, WAKE_CAPS, schedule, tiles, usual, wake_run

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF = TD.OFF
AMPLE = 20000  # passes: a launch behind the series' rest returns at once
SIZES = (66, 97, 130)
WAKING = [f for f in FAMILIES if f != "watershed"]


@contextlib.contextmanager
def sweep_cap(nj, family, cap):
    hook = getattr(nj._native.lib, "nz_debug_%s_sweeps" % family)
    hook(cap)
    try:
        yield
    finally:
        hook(0)


def gpu(nj, ctx, family, h, kw, budget=AMPLE):
    """One call of the family's entry on h (res x res, or count x res x res: the _batch entry) -> (the model's planes,
    passes, converged, the head of `work` as bytes)."""
    h = np.ascontiguousarray(h, f32)
    res, count = h.shape[-1], (h.shape[0] if h.ndim == 3 else 1)
    lib = nj._native.lib
    opt = {k: v for k, v in kw.items() if k in ("erodibility", "uplift", "dt", "hardness", "upliftMap")}
    if family == "fill":
        work = ctx.alloc(lib.nz_fill_depressions_work_floats(res, count))
        src = ctx.from_host(h)
        desc = TF.desc_of(nj, kw.get("epsilon", 1e-4), OFF, budget)
        if h.ndim == 3:
            ctx.call("nz_fill_depressions_batch", src.ptr, work.ptr, C.byref(desc), res, count).Complete()
        else:
            ctx.call("nz_fill_depressions", src.ptr, work.ptr, C.byref(desc), res).Complete()
        status = ctx.wrap(work.ptr, 2, dtype=np.int32).ToArray()
        planes, passes, conv = [src.ToArray(h.shape)], int(status[0]), int(status[1])
        src.Dispose()
    elif family == "drainage":
        work = ctx.alloc(lib.nz_drainage_area_work_floats(res, count))
        got, passes, conv = TD.run_gpu(nj, ctx, h, kw.get("rain", 1.0), OFF, budget, rm=kw.get("rainMap"), work=work)
        planes = [got]
    elif family == "drainage_mfd":
        work = ctx.alloc(lib.nz_drainage_mfd_work_floats(res, count))
        got, passes, conv = TM.run_gpu(nj, ctx, h, kw.get("rain", 1.0), OFF, budget, kw.get("rainMap"), kw.get("exponent", 1), work=work)
        planes = [got]
    elif family == "watershed":
        length = kw.get("length", True)
        work = ctx.alloc(lib.nz_watershed_work_floats(res, count, 1 if length else 0))
        b, l, _, passes, conv = TW.run_gpu(nj, ctx, h, OFF, kw.get("cellSize", 1.0), budget, length=length, work=work)
        planes = [b, l] if length else [b]
    elif family == "stream_order":
        links = kw.get("links", True)
        work = ctx.alloc(lib.nz_stream_order_work_floats(res, count, 1 if links else 0))
        o, l, passes, conv = TS.run_gpu(nj, ctx, h, OFF, kw.get("drainage"), kw.get("threshold", 0.0), budget, links=links, work=work)
        planes = [o, l] if links else [o]
    elif family == "fluvial_implicit":
        work = ctx.alloc(lib.nz_fluvial_implicit_work_floats(res, count))
        got, passes, conv = TI.run_gpu(nj, ctx, h, kw["A"], budget=budget, work=work, **opt)
        planes = [got]
    else:
        assert family == "fluvial_implicit_mfd"
        work = ctx.alloc(lib.nz_fluvial_implicit_mfd_work_floats(res, count))
        got, passes, conv = TIM.run_gpu(nj, ctx, h, kw["A"], budget=budget, work=work, exponent=kw.get("exponent", 1), **opt)
        planes = [got]
    head = ctx.wrap(work.ptr, R.head_bytes(res, res, count), dtype=np.uint8).ToArray()
    work.Dispose()
    return planes, passes, conv, head


def stacked(cases):
    """[(h, kw)] of one family -> (h, kw) of the batch: planes stacked, scalars as they are."""
    kws = [kw for _, kw in cases]
    kw = {k: (np.stack([d[k] for d in kws]) if isinstance(v, np.ndarray) else v) for k, v in kws[0].items()}
    return np.stack([h for h, _ in cases]), kw


def assert_planes(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        b = np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, i, a.dtype, b.dtype)
        bad = a.view(np.uint32) != b.view(np.uint32) if a.dtype == f32 else a != b
        assert not bad.any(), "%s: plane %d, %d/%d cells differ, first at %s: %r vs %r" % (
            what, i, int(bad.sum()), bad.size, np.argwhere(bad)[0], a[bad][0], b[bad][0])


def assert_bytes(head, res, count, p, moved, what):
    """The byte generation pass p wrote against the model's map of pass p."""
    got = R.tile_bytes(head, res, res, count, p)
    want = np.asarray(moved).reshape(got.shape)
    assert np.array_equal(got, want), "%s: the tile bytes of pass %d\n%s\nthe model's\n%s" % (
        what, p, got.astype(int), want.astype(int))


# 1.
@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("family", FAMILIES)
def test_ordinary_tiles_take_the_models_passes(nj, ctx, family, res):
    h, kw, want = usual(family, (res, res))
    for cap in CAPS:
        model = schedule(family, (res, res), cap)
        what = "%s %d^2 cap %d" % (family, res, cap)
        with sweep_cap(nj, family, cap):
            planes, passes, conv, _ = gpu(nj, ctx, family, h, kw)
            print("%s: %d passes, the model %d" % (what, passes, model.passes))
            assert (passes, conv) == (model.passes, 1), what
            assert_planes(planes, want, what)
            bh, bkw = stacked([(h, kw), (h, kw)])
            planes, passes, conv, _ = gpu(nj, ctx, family, bh, bkw)
            assert (passes, conv) == (model.passes, 1), what + " batch"
            for k in range(2):
                assert_planes([p[k] for p in planes], want, what + " batch plane %d" % k)


def mirrored(h, kw):
    return np.ascontiguousarray(h[::-1]), {k: (np.ascontiguousarray(v[::-1]) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def wake_walk(t):
    return memo(("relax schedule wake walk", t.name), t.walk)


def budget_cut(nj, ctx, family, cases, walks, count, what):
    """`cases` [(h, kw)] as one call -- a batch when there are several -- with a budget of the model's count less one, and of
    the count."""
    h, kw = stacked(cases) if len(cases) > 1 else cases[0]
    each = (lambda planes, k: [p[k] for p in planes]) if len(cases) > 1 else (lambda planes, k: planes)
    planes, passes, conv, _ = gpu(nj, ctx, family, h, kw, budget=count - 1)
    assert (passes, conv) == (count - 1, 0), what
    for k, (ph, pkw) in enumerate(cases):
        assert_planes(each(planes, k), R.nothing(family, ph, **pkw), "%s plane %d: all or nothing" % (what, k))
    planes, passes, conv, _ = gpu(nj, ctx, family, h, kw, budget=count)
    assert (passes, conv) == (count, 1), what
    for k, want in enumerate(walks):
        assert_planes(each(planes, k), want, "%s plane %d" % (what, k))


# 2.
@pytest.mark.parametrize("family", WAKING)
def test_wake_up_tiles(nj, ctx, family):
    for t in tiles(family):
        want = wake_walk(t)
        for cap in WAKE_CAPS:
            model = wake_run(t, cap)
            what = "%s cap %d" % (t.name, cap)
            with sweep_cap(nj, family, cap):
                planes, passes, conv, head = gpu(nj, ctx, family, t.h, t.kw)
            print("%s: %d passes, the model %d" % (what, passes, model.passes))
            assert (passes, conv) == (model.passes, 1), what
            assert_planes(planes, want, what)
            for p in (model.passes - 1, model.passes - 2):
                assert_bytes(head, t.res, 1, p, model.moved[p], what)
    # ... and through the _batch entry: the tiles of one resolution as one call, planes that rest at different passes
    for res in (66, 130):
        group = [t for t in tiles(family) if t.res == res]
        for cap in WAKE_CAPS:
            model = R.as_batch([wake_run(t, cap) for t in group])
            what = "%s wake-up tiles %d^2 as a batch, cap %d" % (family, res, cap)
            with sweep_cap(nj, family, cap):
                planes, passes, conv, head = gpu(nj, ctx, family, *stacked([(t.h, t.kw) for t in group]))
            assert (passes, conv) == (model.passes, 1), what
            for k, t in enumerate(group):
                assert_planes([p[k] for p in planes], wake_walk(t), "%s plane %d" % (what, k))
            for p in (model.passes - 1, model.passes - 2):
                assert_bytes(head, res, len(group), p, model.moved[p], what)


# 3.
@pytest.mark.parametrize("family", WAKING)
def test_a_wake_up_tile_between_quiet_planes(nj, ctx, family):
    t = tiles(family)[0]  # a diagonal at 66^2: 2 x 5 tiles
    tile = (t.h, t.kw)
    quiet = (np.full_like(t.h, R.WALL), t.kw)  # walls alone: nothing flows
    mirror = mirrored(*tile)
    cases = dict(tile=tile, quiet=quiet, mirror=mirror)
    for cap in WAKE_CAPS:
        with sweep_cap(nj, family, cap):
            single = {name: gpu(nj, ctx, family, *case) for name, case in cases.items()}
            assert_planes(single["tile"][0], wake_walk(t), t.name)
            assert_planes(single["mirror"][0], R.walk(family, mirror[0], **mirror[1]), t.name + " mirrored")
            assert single["tile"][1] == wake_run(t, cap).passes > single["quiet"][1], (t.name, cap)
            for order in (("quiet", "tile", "quiet"), ("tile", "quiet", "mirror")):
                what = "%s cap %d batch %s" % (t.name, cap, order)
                model = R.run_batch([R.model(family, cases[name][0], **cases[name][1]) for name in order], sweeps=cap)
                planes, passes, conv, head = gpu(nj, ctx, family, *stacked([cases[name] for name in order]))
                assert (passes, conv) == (model.passes, 1) and passes == max(single[name][1] for name in order), what
                for k, name in enumerate(order):
                    assert_planes([p[k] for p in planes], single[name][0], what + " plane %d" % k)
                for p in (passes - 1, passes - 2):  # the bytes of the last two passes, plane beside plane
                    assert_bytes(head, t.res, 3, p, model.moved[p], what)


# 4.
@pytest.mark.parametrize("family", FAMILIES)
def test_the_budget_cuts_at_the_models_pass(nj, ctx, family):
    h, kw, want = usual(family, (97, 97))
    budget_cut(nj, ctx, family, [(h, kw)], [want], schedule(family, (97, 97), 16).passes, family + " usual 97^2")
    # a batch whose planes come to rest at different passes: the usual tile, the same mirrored, a level plane
    h, kw, want = usual(family, (66, 66))
    cases = [(h, kw), mirrored(h, kw), (np.full_like(h, h[33, 33]), kw)]
    runs = [schedule(family, (66, 66), 16)] + [R.run(R.model(family, ph, **pkw)) for ph, pkw in cases[1:]]
    assert len({r.passes for r in runs}) > 1, [r.passes for r in runs]
    walks = [want] + [R.walk(family, ph, **pkw) for ph, pkw in cases[1:]]
    budget_cut(nj, ctx, family, cases, walks, R.as_batch(runs).passes, family + " usual 66^2, mirrored, level")
    if family in WAKING:
        t = tiles(family)[1]
        budget_cut(nj, ctx, family, [(t.h, t.kw)], [wake_walk(t)], wake_run(t, 16).passes, t.name)
        group = [t for t in tiles(family) if t.res == 66]
        runs = [wake_run(t, 16) for t in group]
        assert len({r.passes for r in runs}) > 1, [r.passes for r in runs]
        budget_cut(nj, ctx, family, [(t.h, t.kw) for t in group], [wake_walk(t) for t in group], R.as_batch(runs).passes,
                   family + " wake-up tiles 66^2 as a batch")


# 5.
@pytest.mark.parametrize("family", FAMILIES)
def test_the_tile_bytes_are_the_models_moved_maps(nj, ctx, family):
    cases = [("usual 130^2", usual(family, (130, 130))[:2], schedule(family, (130, 130), 16), 16)]
    if family in WAKING:
        t = tiles(family)[2]  # a diagonal at 130^2, at the cap that takes the most passes
        cases.append((t.name, (t.h, t.kw), wake_run(t, 3), 3))
    for name, (h, kw), model, cap in cases:
        res = h.shape[-1]
        with sweep_cap(nj, family, cap):
            for p in sorted({1, 2, model.passes // 2, model.passes}):
                what = "%s %s cut at %d of %d passes" % (family, name, p, model.passes)
                _, passes, conv, head = gpu(nj, ctx, family, h, kw, budget=p)
                assert (passes, conv) == (p, int(p == model.passes)), what
                assert_bytes(head, res, 1, p - 1, model.moved[p - 1], what)
                if p >= 2:
                    assert_bytes(head, res, 1, p - 2, model.moved[p - 2], what)
        if name.startswith("usual"):  # the batch: the planes' bytes back to back, both generations
            mh, mkw = mirrored(h, kw)
            batch = R.as_batch([model, R.run(R.model(family, mh, **mkw), sweeps=cap), model])
            for p in sorted({2, batch.passes // 2, batch.passes}):
                what = "%s %s, mirrored, the same: cut at %d of %d passes" % (family, name, p, batch.passes)
                with sweep_cap(nj, family, cap):
                    _, passes, conv, head = gpu(nj, ctx, family, *stacked([(h, kw), (mh, mkw), (h, kw)]), budget=p)
                assert (passes, conv) == (p, int(p == batch.passes)), what
                assert_bytes(head, res, 3, p - 1, batch.moved[p - 1], what)
                assert_bytes(head, res, 3, p - 2, batch.moved[p - 2], what)
