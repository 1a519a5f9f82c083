"""tests/relax_schedule.py, the pass protocol and tile schedule of the seven iterate-to-rest series in numpy, checked on the
CPU: that it is right, and that the inputs it offers the GPU tests bite.

  1. result bits   for every family the schedule ends in the family's walk, bit for bit, on a 24 x 200 grid (4 x 2 tiles)
                   and on 66^2 and 97^2, at sweep caps 1, 3 and 16
  2. counts        its pass count equals every single-call entry of tests/golden/relax_passes.json -- recordings of the
                   kernels on an MI355X -- so the recorded counts are now derived ones
  3. wake-up tiles every tile of wake_tiles() ends in its walk under the real rule and is lost by its mutant: wake="four" on
                   the diagonal tiles, each in the direction the maps show, wake="self" on the edge tiles (one of them at
                   cap 3 only), and the Jacobi order changes the count where a channel runs along a row and nowhere else
  4. the gap       wake="four" is NOT caught on the filled fbm130 tile the recorded counts use, nor is wake="self" for
                   drainage and watershed: same bits, same counts.  That is what the directed tiles are for.  The Jacobi
                   order, and wake="self" for the stream order, the recorded counts do catch
  5. watershed     has no wake-up tile, and the model shows why: a cell that is not final changes in every pass (its label
                   is the index of the furthest ancestor reached so far, and those are all different), so a tile that moves
                   in pass p moved in pass p - 1 already and no wake rule is ever consulted for a visit that matters"""
import json
import os

import numpy as np
import pytest

import drainage_ref as D
import fill_ref as L
import relax_schedule as R
from conftest import GOLDEN
from test_gpu_slab import memo
from test_hydraulic_ref import relief

f32 = np.float32
CAPS = (1, 3, 16)
WAKE_CAPS = (16, 3)
SHAPES = ((24, 200), (66, 66), (97, 97))
FAMILIES = tuple(R.FAMILIES)
HEADINGS = {(1, 1), (1, -1), (-1, 1), (-1, -1)}


def relief_of(shape):
    rows, cols = shape
    return memo(("relax schedule relief", shape), lambda: np.ascontiguousarray(relief(max(shape))[:rows, :cols], f32))


def usual(family, shape):
    """(h, kw, the walk's planes) of the family's usual tile of a shape."""
    def make():
        h, kw = R.usual_case(family, relief_of(shape))
        return h, kw, R.walk(family, h, **kw)
    return memo(("relax schedule usual", family, shape), make)


def schedule(family, shape, cap):
    """The model's run on the usual tile: shared with tests/test_gpu_relax_schedule.py."""
    h, kw, _ = usual(family, shape)
    return memo(("relax schedule run", family, shape, cap), lambda: R.run(R.model(family, h, **kw), sweeps=cap))


def wake_run(tile, cap):
    return memo(("relax schedule wake run", tile.name, cap), lambda: R.run(tile.model(), sweeps=cap))


def tiles(family):
    return memo(("relax schedule wake tiles", family), lambda: R.wake_tiles(family))


def woken_by_a_diagonal_alone(r):
    """The passes in which a tile moved that neither itself nor an edge neighbour had woken."""
    return [p for p in range(1, r.passes) if (r.moved[p] & ~R.woken(r.moved[p - 1], "four")).any()]


def diagonal_crossings(r):
    """The directions (dx, dz), in tiles, from a tile that moved in pass p - 1 to a diagonal neighbour that moved in pass p
    and that neither itself nor an edge neighbour had woken: where the front went through a corner, read off the maps."""
    out = set()
    for p in woken_by_a_diagonal_alone(r):
        for tz, tx in np.argwhere(r.moved[p] & ~R.woken(r.moved[p - 1], "four")):
            for dz in (-1, 1):
                for dx in (-1, 1):
                    sz, sx = tz - dz, tx - dx
                    if 0 <= sz < r.moved[p].shape[0] and 0 <= sx < r.moved[p].shape[1] and r.moved[p - 1][sz, sx]:
                        out.add((dx, dz))
    return out


# 1.
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_the_schedule_ends_in_the_walk(family, shape):
    _, _, want = usual(family, shape)
    for cap in CAPS:
        r = schedule(family, shape, cap)
        assert r.converged == 1 and R.same_planes(r.planes, want), (family, shape, cap)
        assert len(r.moved) == r.passes and r.moved[0].all() and not r.moved[-1].any()
        assert all((m <= v).all() for m, v in zip(r.moved, r.visited))  # only a visited tile moves
    # a budget one short of the count is cut mid-series; the count itself is enough
    h, kw, _ = usual(family, shape)
    full = schedule(family, shape, 16)
    cut = R.run(R.model(family, h, **kw), budget=full.passes - 1)
    assert (cut.passes, cut.converged) == (full.passes - 1, 0)
    assert all(np.array_equal(a, b) for a, b in zip(cut.moved, full.moved))


# 2.
def recorded_inputs():
    """The inputs of tests/test_gpu_relax_passes.measure, entry by entry, as (key, family, h or a batch, kw, cap)."""
    import test_gpu_drainage as TD
    import test_gpu_fill as TF
    import test_gpu_stream_order as TS
    import test_gpu_watershed as TW
    out = []
    for name in ("bowl160", "fbm97", "rand130", "const65"):
        for eps in (0.0, 1e-4):
            out.append(("fill %s eps %g" % (name, eps), "fill", TF.tile(name), dict(epsilon=eps), 16))
    batch = np.stack([relief(48), (relief(48, 170) * f32(3.0)).astype(f32), TF.tile("rand130")[:48, :48].copy()])
    for eps in (0.0, 1e-4):
        out.append(("fill batch 3x48 eps %g" % eps, "fill", batch, dict(epsilon=eps), 16))
    out.append(("drainage serpentine160", "drainage", TD.serpentine()[0], {}, 16))
    filled = memo("relax schedule filled fbm130", lambda: L.flood(TD.tile(130), 1e-4))
    area = memo("relax schedule filled fbm130 area", lambda: D.accumulate(filled)[0])
    for cap in CAPS:
        out.append(("drainage filled fbm130 rain map cap %d" % cap, "drainage", filled, dict(rain=0.75, rainMap=TD.rain_map(130)), cap))
        out.append(("watershed filled fbm130 length cap %d" % cap, "watershed", filled, dict(length=True), cap))
        out.append(("stream order filled fbm130 drainage threshold 8 links cap %d" % cap, "stream_order", filled,
                    dict(drainage=area, threshold=8.0, links=True), cap))
    out.append(("watershed serpentine160", "watershed", TW.serpentine()[0], {}, 16))
    for which, (h, dr, _, _, _) in enumerate(TS.long_tiles()):
        out.append(("stream order long chain %d" % which, "stream_order", h, dict(drainage=dr, threshold=0.5, links=True), 16))
    return out


def recorded_run(key, family, h, kw, cap, **mutant):
    def make():
        if h.ndim == 3:
            return R.run_batch([R.model(family, t, **kw) for t in h], sweeps=cap, **mutant)
        return R.run(R.model(family, h, **kw), sweeps=cap, **mutant)
    return memo(("relax schedule recorded", key, tuple(sorted(mutant.items()))), make)


def test_the_recorded_pass_counts_are_the_schedules():
    with open(os.path.join(GOLDEN, "relax_passes.json")) as f:
        table = json.load(f)
    want = dict(table["passes"], **table["passes on 0da72c4"])
    del want["fill stripes bowl world 2"]  # a series per round, against frozen rows: not this model's
    got = {}
    for key, family, h, kw, cap in recorded_inputs():
        r = recorded_run(key, family, h, kw, cap)
        assert r.converged == 1, key
        got[key] = r.passes
    print(json.dumps(got))
    assert got == want


# 3.
@pytest.mark.parametrize("family", [f for f in FAMILIES if f != "watershed"])
def test_wake_up_tiles_are_lost_by_their_mutants(family):
    ts = tiles(family)
    assert {t.heading for t in ts if t.kind == "diagonal"} == HEADINGS
    assert {t.res for t in ts if t.kind == "diagonal"} == {66, 130}
    for t in ts:
        want, m = t.walk(), t.model()
        for cap in WAKE_CAPS:
            r = wake_run(t, cap)
            assert r.converged == 1 and R.same_planes(r.planes, want), (t.name, cap)
            if t.kind == "diagonal":
                # the corner the front goes through, read off the maps, is the one the tile is labelled with
                assert diagonal_crossings(r) == {t.heading}, (t.name, cap, diagonal_crossings(r))
                lost = R.run(m, sweeps=cap, wake="four")
                assert lost.converged == 1 and lost.passes < r.passes and not R.same_planes(lost.planes, want), (t.name, cap)
            if t.kind != "diagonal":
                lost = R.run(m, sweeps=cap, wake="self")
                if t.kind == "row" and cap == 16 and family in R.UPSTREAM:
                    # the one edge tile that is blind: the outlet's column is 2 cells wide, the front crosses a tile per
                    # pass at this cap and arrives in the third tile column while every tile is still awake
                    assert lost.passes == r.passes and R.same_planes(lost.planes, want), (t.name, cap)
                else:
                    assert lost.converged == 1 and not R.same_planes(lost.planes, want), (t.name, cap)
                assert R.same_planes(R.run(m, sweeps=cap, wake="four").planes, want), (t.name, cap)  # an edge is enough here
            if t.kind == "column" and cap == 16:
                assert {1, 2} <= R.rests(r), (t.name, R.rests(r))  # woken after an odd and after an even rest
            # four cells per sweep against one: a row is the one place where the order inside a thread shows.  A diagonal
            # or a column has one channel cell per thread and cannot tell: the same count, pinned here
            jacobi = R.run(m, sweeps=cap, order=R.JACOBI)
            assert R.same_planes(jacobi.planes, want), (t.name, cap)
            if t.kind == "row":
                assert jacobi.passes > r.passes, (t.name, cap, jacobi.passes, r.passes)
            else:
                assert jacobi.passes == r.passes, (t.name, cap, jacobi.passes, r.passes)


# 4.
def test_the_mutants_are_not_caught_on_the_recorded_tile():
    """The gap: on the filled fbm130 tile of the recorded counts (drainage, watershed and stream order, at the three caps) a
    skip rule without diagonals gives the recorded count and the walk's bits, and so does one without any neighbour for
    drainage and watershed.  Stream order on that tile does lose wake="self" (its orders rest and are woken), and the Jacobi
    order is caught by every recorded count: those two the recordings did cover."""
    seen = 0
    for key, family, h, kw, cap in recorded_inputs():
        if "filled fbm130" not in key:
            continue
        r = recorded_run(key, family, h, kw, cap)
        four = recorded_run(key, family, h, kw, cap, wake="four")
        assert four.passes == r.passes and four.converged == 1 and R.same_planes(four.planes, r.planes), key
        alone = recorded_run(key, family, h, kw, cap, wake="self")
        if family == "stream_order":
            assert alone.passes < r.passes and not R.same_planes(alone.planes, r.planes), key
        else:
            assert alone.passes == r.passes and alone.converged == 1 and R.same_planes(alone.planes, r.planes), key
        jacobi = recorded_run(key, family, h, kw, cap, order=R.JACOBI)
        assert jacobi.passes > r.passes and R.same_planes(jacobi.planes, r.planes), key
        seen += 1
    assert seen == 9


# 5.
def test_the_watershed_has_no_wake_up_tile():
    """... and neither has the link plane of the stream order, which is copied down a reach as a label is copied up a basin:
    with links the wake-up tiles of the stream order are blind, which is why they run order only."""
    assert R.wake_tiles("watershed") == []
    for t in tiles("stream_order"):
        kw = dict(t.kw, links=True)
        want = R.walk("stream_order", t.h, **kw)
        for cap in WAKE_CAPS:
            r = R.run(R.model("stream_order", t.h, **kw), sweeps=cap)
            assert r.converged == 1 and R.same_planes(r.planes, want)
            assert all((r.moved[p] <= r.moved[p - 1]).all() for p in range(1, r.passes)), (t.name, cap)
    cases = [R.front_case("watershed", res, R.diagonal_cells(res, zc, xc, sx, sz)) for res, zc, xc, sx, sz in R.DIAGONALS]
    cases += [R.front_case("watershed", 66, R.column_cells(66, 10)), R.front_case("watershed", 130, R.row_cells(130, 10))]
    cases += [usual("watershed", shape)[:2] for shape in SHAPES]
    for h, kw in cases:
        want = R.walk("watershed", h, **kw)
        for cap in WAKE_CAPS:
            r = R.run(R.model("watershed", h, **kw), sweeps=cap)
            assert r.converged == 1 and R.same_planes(r.planes, want)
            # a tile that moves has moved in the pass before: nothing is ever woken
            assert all((r.moved[p] <= r.moved[p - 1]).all() for p in range(1, r.passes))
            assert not R.rests(r) and not woken_by_a_diagonal_alone(r)
            lost = R.run(R.model("watershed", h, **kw), sweeps=cap, wake="self")
            assert lost.passes == r.passes and R.same_planes(lost.planes, want)
