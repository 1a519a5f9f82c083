"""Every launch form of the fused flow map, at the smallest shapes that select it by the default rule.

nz_launch_flow_fused runs a launch as 32-, 48- or 64-row tiles or as the row-streaming kernel; nz_flow_launch_form says which
(the rule itself, not a copy).  Every shape below is found through that query.  What is compared:

  * NZ_FLOAT_STRICT and NZ_FLOAT_FAST (which runs the strict flow forms): the bit patterns of tests/flow_ref.py -- the
    oracle's flow_step / water_step / velocity / normalize chained per launch; the sign of a zero counts, a NaN matches a NaN;
  * NZ_FLOAT_RELAXED (v_rcp_f32 / v_sqrt_f32, no restatement): every form equals, bit for bit, the same cells computed in that
    mode by the 32-row tile -- a tile of a batch alone with count 1, a tall stripe cut into stripes of 32-row launches -- and
    stays within the distribution tests/test_gpu_fast.py grants the mode against the strict oracle: at most
    max(8, 0.02 * cells) cells outside 1e-5 relative / 1e-6 absolute, none by 1e-3 or more.

Each test runs its case in all three modes on one set of inputs and one reference.  With NZ_FLOW_STREAM, NZ_FLOW_TINY or
NZ_FLOW_NMAX set the file compares whatever forms the query reports; only the "every form was reached" assertions are
dropped."""
import ctypes as C
import os

import numpy as np
import pytest

import flow_ref as F
import terrain_tiles as T
from conftest import adversarial_tiles

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = {0: "strict", 1: "fast", 2: "relaxed"}
TILE48, TILE32, TILE64, STREAM = 0, 1, 2, 3
FORM = {TILE48: "tile48", TILE32: "tile32", TILE64: "tile64", STREAM: "stream"}
KNOBS = any(os.environ.get(k) for k in ("NZ_FLOW_STREAM", "NZ_FLOW_TINY", "NZ_FLOW_NMAX"))
STREAM_CELLS = 8 * 1024 * 1024   # only the search range of the batch counts: 1 .. STREAM_CELLS / res^2 + 1
PADS = (0, 1, 3)
RTOL, ATOL = 1e-5, 1e-6


@pytest.fixture(scope="module")
def ctxs(nj):
    cs = {}
    for mode in MODES:
        cs[mode] = nj.Context(0)
        cs[mode].float_mode = mode
        assert cs[mode].float_mode == mode
    yield cs
    for c in cs.values():
        c.close()


# ---- the query ------------------------------------------------------------------------------------------------------
def form(nj, ctx, cols, rows, count, n, first, last):
    f = nj._native.lib.nz_flow_launch_form(ctx._h, cols, rows, count, n, int(first), int(last))
    assert f in FORM, (f, nj._native.lib.nz_last_error())
    return f


def cap(nj):
    return nj._native.lib.nz_flow_fused_max_iterations()


def smallest_counts(nj, ctx, res, n):
    """form -> the smallest count in 1 .. 8M / res^2 + 1 whose whole stage of n iterations takes it ({} if n is split)."""
    found = {}
    if n <= cap(nj):
        for c in range(1, STREAM_CELLS // (res * res) + 2):
            found.setdefault(form(nj, ctx, res, res, c, n, 1, 1), c)
    return found


def smallest_rows(nj, ctx, cols, n, want, limit=20000):
    for r in range(1, limit):
        if form(nj, ctx, cols, r, 1, n, 0, 0) == want:
            return r
    return None


def chunk_rows_32(nj, ctx, cols, n, first, last):
    """The most rows one 32-row launch takes (the rule is monotone in the rows); 64 rows of whatever form when a knob rules
    the 32-row tile out."""
    if form(nj, ctx, cols, 1, 1, n, first, last) != TILE32:
        return 64
    lo, hi = 1, 1 << 24
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if form(nj, ctx, cols, mid, 1, n, first, last) == TILE32 else (lo, mid - 1)
    return lo


def stream_rows(nj, ctx, cols, n):
    """The fewest rows of `cols` cells whose whole stage streams (monotone: a cell count)."""
    top = (1 << 24) // cols + 1
    if form(nj, ctx, cols, top, 1, n, 1, 1) != STREAM:
        return (STREAM_CELLS + cols - 1) // cols   # a knob: the same grid, whatever form it takes
    lo, hi = 1, top
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if form(nj, ctx, cols, mid, 1, n, 1, 1) == STREAM else (mid + 1, hi)
    return lo


# ---- inputs ---------------------------------------------------------------------------------------------------------
terrain = F.terrain


def distinct_tiles(seed, count, res):
    """Even tiles: terrain; odd tiles: uniform heights in [0, 1) -- slopes far above the water column, most cells run dry."""
    rng = np.random.default_rng(seed)
    return np.stack([terrain(rng, res, res) if k % 2 == 0 else rng.random((res, res), dtype=f32) for k in range(count)])


def special_planes(res):
    rng = np.random.default_rng(9000 + res)
    t = dict(adversarial_tiles(res, rng))
    t["tiny"] = T.tiny(res, rng)      # subnormal drops
    t["zeros"] = T.zeros(res, rng)    # +-0 with specks of +-1e-45
    nf = terrain(rng, res, res)
    nf[0, 0], nf[-1, -1] = np.nan, np.inf                                # corners
    nf[res // 2, 0], nf[0, res // 3], nf[-1, res // 2] = np.inf, np.nan, -np.inf   # edges
    nf[res // 3, res // 4], nf[res // 2, res // 2], nf[2 * res // 3, res - 5] = np.nan, -np.inf, np.inf   # interior
    t["non_finite"] = nf
    z = np.zeros((res, res), f32)     # sparse impulses on zeros: the flux sums that drive the flow are subnormal
    z[0, 0] = z[-1, -1] = z[0, -1] = 1.0
    z[res // 3, 4] = -2.0
    z[res // 2, res // 2] = 1e-45
    t["impulses"] = z
    return t


SPECIAL_NAMES = ("uniform", "constant", "impulse_centre", "impulse_corner", "impulse_edge", "ramp_x", "ramp_z", "tiny",
                 "zeros", "non_finite", "impulses")


# ---- comparisons ----------------------------------------------------------------------------------------------------
def within_relaxed_band(got, want, what):
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(w)
    d = np.abs(g - w)
    ok = np.where(fin, d <= RTOL * np.abs(w) + ATOL, (g == w) | (np.isnan(g) & np.isnan(w)))
    bad = int(ok.size - ok.sum())
    ab = float(np.where(fin, d, 0.0).max()) if w.size else 0.0   # a NaN where the oracle is finite makes this NaN
    assert bad <= max(8, 0.02 * w.size) and ab < 1e-3, "%s: %d of %d cells outside 1e-5 rel / 1e-6 abs, max abs %g" % (
        what, bad, w.size, ab)


def compare(mode, got, want, by_tile32, what):
    """strict / fast: the oracle's bits.  relaxed: the 32-row tile's bits in that mode, and the mode's band."""
    what = "%s [%s]" % (what, MODES[mode])
    if mode < 2:
        F.assert_bits_equal(got, want, what)
    else:
        F.assert_bits_equal(got, by_tile32, what + " against the 32-row tile")
        within_relaxed_band(got, want, what)


# ---- a. the stage entries by batch count ----------------------------------------------------------------------------
class Batch:
    """Device planes for batches of up to `count` tiles, reused by every launch of a test."""

    def __init__(self, nj, ctx, res, count):
        self.nj, self.ctx, self.res, self.n = nj, ctx, res, res * res
        self.src, self.dst = ctx.alloc(count * self.n), ctx.alloc(count * self.n)
        self.work = ctx.alloc(11 * count * self.n)

    def run(self, entry, planes, its):
        count = planes.shape[0]
        src = self.src.offset(0, count * self.n)
        src.CopyFrom(planes)
        if entry == "batch":     # in place, the heights kept in the stage's 11th plane
            self.ctx.call("nz_flowmap_stage_batch", src.ptr, self.work.ptr, its, *F.NORM, self.res, count).Complete()
            return src.ToArray(planes.shape)
        pair = self.nj._native.RWTile(src.ptr, self.dst.ptr, self.res, count)
        self.ctx.call("nz_flowmap_stage_rw", C.byref(pair), self.work.ptr, its, *F.NORM).Complete()
        assert (pair.read, pair.write) == (self.dst.ptr, src.ptr)
        return self.dst.offset(0, count * self.n).ToArray(planes.shape)

    def Dispose(self):
        for t in (self.src, self.dst, self.work):
            t.Dispose()


def alone(nj, b, planes, its):
    """Every plane through the stage on its own, count 1: the 32-row tile at these sizes."""
    if not KNOBS:
        for n, first, last in launches(nj, its):
            assert form(nj, b.ctx, b.res, b.res, 1, n, first, last) == TILE32
    return np.stack([b.run("rw" if k & 1 else "batch", planes[k:k + 1], its)[0] for k in range(planes.shape[0])])


def launches(nj, its):
    split = F.split_iterations(its, cap(nj))
    return [(n, int(i == 0), int(i == len(split) - 1)) for i, n in enumerate(split)]


@pytest.mark.parametrize("n", range(1, 6))
@pytest.mark.parametrize("res", [253, 254, 256])   # odd: scalar path, three strips; rows 8-byte, not 16-byte aligned; aligned
def test_stage_entries_by_batch_count(nj, ctxs, oracle, res, n):
    found = smallest_counts(nj, ctxs[0], res, n)
    top = STREAM_CELLS // (res * res) + 1
    if not KNOBS:
        assert set(found) == set(FORM), "forms reached at %d^2 x%d: %s" % (res, n, found)
        assert found[TILE32] == 1
    counts = sorted(set(found.values()) | ({1, top} if KNOBS else set()))
    tiles = distinct_tiles(res * 10 + n, max(counts), res)
    want = [oracle.flowmap(t, n, *F.NORM) for t in tiles]
    special = special_planes(res)
    # Two special planes ride in each batch of two tiles or more.  Batch i (in the order of the counts: 32-, 48-, 64-row,
    # streaming) of case idx = (resolution, n) takes planes idx + 3i + 7 and idx + 3i + 1 of the eleven: every form meets
    # every plane over the fifteen cases, and the streaming batch of 253^2 (the scalar streaming path, the odd last column)
    # carries the NaN / +-inf plane at n = 5 and the sparse impulses at n = 1.
    idx = (253, 254, 256).index(res) * 5 + n - 1
    riders = []   # per batch: {position: name}
    for i, count in enumerate(counts):
        pos = (idx + i) % count
        r = {pos: SPECIAL_NAMES[(idx + 3 * i + 7) % len(SPECIAL_NAMES)]}
        if count > 1:
            r[(pos + count // 2) % count] = SPECIAL_NAMES[(idx + 3 * i + 1) % len(SPECIAL_NAMES)]
        riders.append(r)
    swant = {name: oracle.flowmap(special[name], n, *F.NORM) for r in riders for name in r.values()}
    for mode, ctx in ctxs.items():
        b = Batch(nj, ctx, res, max(counts))
        try:
            solo = alone(nj, b, tiles, n)
            ssolo = {name: alone(nj, b, special[name][None], n)[0] for name in swant}
            # (a tile alone IS the 32-row tile: in relaxed mode its own bits are the reference it is handed, and only the band
            # against the strict oracle checks it here; the cross-form comparisons are those of the batches below)
            for k in range(len(tiles)):
                compare(mode, solo[k], want[k], solo[k], "%d^2 x%d tile %d alone" % (res, n, k))
            for name in swant:
                compare(mode, ssolo[name], swant[name], ssolo[name], "%d^2 x%d %s alone" % (res, n, name))
            for i, count in enumerate(counts):
                planes = tiles[:count].copy()
                for pos, name in riders[i].items():
                    planes[pos] = special[name]
                fm = FORM[form(nj, ctx, res, res, count, n, 1, 1)] if n <= cap(nj) else "split"
                for entry in ("batch", "rw"):
                    got = b.run(entry, planes, n)
                    for k in range(count):
                        name = riders[i].get(k)
                        w, s = (swant[name], ssolo[name]) if name else (want[k], solo[k])
                        what = "%s %d x %d^2 x%d (%s) tile %d%s" % (entry, count, res, n, fm, k, " = " + name if name else "")
                        compare(mode, got[k], w, s, what)
                        if name:   # the same tile run alone gives the same bits, in every mode
                            F.assert_bits_equal(got[k], s, what + " against the tile alone")
        finally:
            b.Dispose()


# ---- b. stages of several launches on the large forms ---------------------------------------------------------------
MULTI = (6, 7, 11, 12)
MULTI_RES = (253, 256)


def multi_plan(nj, ctx, res):
    """[(its, count, [(n, first, last, form), ...]), ...]: count 1 and the counts that select the 48- and 64-row tile at n = 3 and
    the streaming kernel at n = 5 as whole stages."""
    c3, c5 = smallest_counts(nj, ctx, res, min(3, cap(nj))), smallest_counts(nj, ctx, res, min(5, cap(nj)))
    counts = sorted({1} | {c3[f] for f in (TILE48, TILE64) if f in c3} | {c5[f] for f in (STREAM,) if f in c5})
    return [(its, c, [(n, first, last, form(nj, ctx, res, res, c, n, first, last)) for n, first, last in launches(nj, its)])
            for its in MULTI for c in counts]


@pytest.mark.parametrize("its", MULTI)
@pytest.mark.parametrize("res", MULTI_RES)
def test_multi_launch_stages(nj, ctxs, oracle, res, its):
    cases = [(c, ls) for i, c, ls in multi_plan(nj, ctxs[0], res) if i == its]
    top = max(c for c, _ in cases)
    tiles = distinct_tiles(res * 100 + its, top, res)
    want = [oracle.flowmap(t, its, *F.NORM) for t in tiles]
    for mode, ctx in ctxs.items():
        b = Batch(nj, ctx, res, top)
        try:
            solo = alone(nj, b, tiles, its)
            for count, ls in cases:
                fm = "+".join("%d:%s" % (n, FORM[f]) for n, _, _, f in ls)
                for entry in ("batch", "rw"):
                    got = b.run(entry, tiles[:count], its)
                    for k in range(count):
                        compare(mode, got[k], want[k], solo[k], "%s %d x %d^2 x%d (%s) tile %d" % (entry, count, res, its, fm, k))
        finally:
            b.Dispose()


def test_multi_launch_stages_reach_every_tile_form_in_every_role(nj, ctxs):
    seen = {(first, last, f) for res in MULTI_RES for _, _, ls in multi_plan(nj, ctxs[0], res) for _, first, last, f in ls}
    if not KNOBS:
        for role in ((1, 0), (0, 0), (0, 1)):
            for f in (TILE32, TILE48, TILE64):
                assert role + (f,) in seen, "first=%d last=%d never ran as %s: %s" % (role + (FORM[f], sorted(seen)))


# ---- c. the stripe entry, directly ----------------------------------------------------------------------------------
class StripeBuffers:
    """One stripe buffer of rows x pitch per plane: height, five state-in planes, two sets of outputs (the launch under
    test, and the same rows cut into 32-row launches), and a plane of NaN the outputs are reset from on the device."""

    def __init__(self, nj, ctx, rows, cols, pitch, second):
        self.nj, self.ctx, self.rows, self.cols, self.pitch = nj, ctx, rows, cols, pitch
        n = rows * pitch
        self.nan = ctx.from_host(np.full(n, np.nan, f32))
        self.h, self.sin = ctx.alloc(n), None
        self.out = [[ctx.alloc(n) for _ in range(5)] for _ in range(2 if second else 1)]
        self.tiles = [self.nan, self.h] + [t for s in self.out for t in s]

    def padded(self, plane, r0=0):
        """`plane` at rows r0.. of a NaN buffer, pads NaN"""
        buf = np.full((self.rows, self.pitch), np.nan, f32)
        buf[r0:r0 + plane.shape[0], :self.cols] = plane
        return buf

    def set_state_in(self, bufs):
        if self.sin is None:
            self.sin = [self.ctx.alloc(self.rows * self.pitch) for _ in range(5)]
            self.tiles += self.sin
        for t, a in zip(self.sin, bufs):
            t.CopyFrom(a)

    def reset(self, which, planes):
        for t in self.out[which][:planes]:
            self.ctx.call("nz_flush_write_slice", t.ptr, self.nan.ptr, self.rows * self.pitch, handle=False)

    def call(self, which, st, n, first, last):
        N = self.nj._native
        pin = None if first else (N.dev_ptr * 5)(*[t.ptr for t in self.sin])
        pout = None if last else (N.dev_ptr * 5)(*[t.ptr for t in self.out[which]])
        self.ctx.call("nz_flow_fused_stripe", self.h.ptr, pin, pout, self.out[which][0].ptr if last else None, C.byref(st), n,
                      first, last, *F.NORM, handle=False)

    def results(self, which, planes):
        self.ctx.synchronize()
        return [t.ToArray((self.rows, self.pitch)) for t in self.out[which][:planes]]

    def Dispose(self):
        for t in self.tiles:
            t.Dispose()


def run_stripe(nj, mode, sb, grow0, grows, own0, own1, n, first, last, want, what):
    """The launch on owned rows [own0, own1) of the buffer; `want`: the planes' owned rows.  Everything outside the owned
    rows x cols stays NaN.  relaxed: the same rows in 32-row launches into the second set of outputs."""
    planes = 1 if last else 5
    st = nj.Stripe(sb.cols, sb.rows, grow0, grows, own0, own1, sb.pitch)
    sb.reset(0, planes)
    sb.call(0, st, n, first, last)
    got = sb.results(0, planes)
    by32 = [None] * planes
    if mode == 2:
        step = chunk_rows_32(nj, sb.ctx, sb.cols, n, first, last)
        sb.reset(1, planes)
        for o0 in range(own0, own1, step):
            sb.call(1, nj.Stripe(sb.cols, sb.rows, grow0, grows, o0, min(o0 + step, own1), sb.pitch), n, first, last)
        by32 = [p[own0:own1, :sb.cols] for p in sb.results(1, planes)]
    for k in range(planes):
        g = got[k]
        assert np.isnan(g[:own0]).all() and np.isnan(g[own1:]).all() and np.isnan(g[:, sb.cols:]).all(), \
            "%s plane %d: written outside the owned rows x cols" % (what, k)
        compare(mode, g[own0:own1, :sb.cols], want[k], by32[k], "%s plane %d" % (what, k))


ROLES = ((1, 1), (1, 0), (0, 0), (0, 1))


@pytest.mark.parametrize("n", range(1, 6))
@pytest.mark.parametrize("cols", [131, 253])
def test_stripe_entry_tile_forms(nj, ctxs, oracle, cols, n):
    if n > cap(nj):
        n = cap(nj)   # NZ_FLOW_NMAX: the entry fuses no more
    halo, extra = 2 * n, (2, 3)   # rows of NaN beyond the ghost rows, above / below
    for fi, fm in enumerate((TILE32, TILE48, TILE64)):
        owned = smallest_rows(nj, ctxs[0], cols, n, fm)
        if KNOBS and owned is None:
            owned = (1, 1500, 3600)[fi]
        assert owned is not None, "no stripe of %d cols x%d runs as %s" % (cols, n, FORM[fm])
        grows = owned + 2 * (halo + 5)
        grid = terrain(np.random.default_rng(cols * 100 + n * 10 + fi), grows, cols)
        state = F.launch(grid, 2, True, False)   # what a launch that is not the first reads
        wants = {(f, l): F.launch(grid, n, f, l, None if f else state) for f, l in ROLES}
        for pi, g0 in enumerate((0, halo + 4, grows - owned)):   # top border, inside, bottom border
            g1 = g0 + owned
            pitch = cols + PADS[(pi + fi + n) % 3]
            b0, b1 = max(0, g0 - halo - extra[0]), min(grows, g1 + halo + extra[1])   # the buffer: rows b0 .. b1 of the grid
            v0, v1 = max(0, g0 - halo), min(grows, g1 + halo)                         # ... of which these hold values
            for mode, ctx in ctxs.items():
                sb = StripeBuffers(nj, ctx, b1 - b0, cols, pitch, second=mode == 2)
                try:
                    sb.h.CopyFrom(sb.padded(grid[v0:v1], v0 - b0))
                    sb.set_state_in([sb.padded(p[v0:v1], v0 - b0) for p in state])
                    for first, last in ROLES:
                        if not KNOBS:
                            assert form(nj, ctx, cols, owned, 1, n, first, last) == fm
                        w = wants[(first, last)]
                        w = [w[g0:g1]] if last else [p[g0:g1] for p in w]
                        run_stripe(nj, mode, sb, b0, grows, g0 - b0, g1 - b0, n, first, last, w,
                                   "stripe %d cols pitch %d x%d %s first=%d last=%d rows %d..%d of %d" % (
                                       cols, pitch, n, FORM[fm], first, last, g0, g1, grows))
                finally:
                    sb.Dispose()


# cols 1, 3, 100: one strip, both x borders in one wave; 131: two border strips; 254 / 253: three strips, ~680 row segments,
# the interior strip's pipeline fill, a partial last segment, border segments shorter than interior ones
STREAMING = ([(cols, n, "whole") for cols in (1, 3, 100, 131, 254, 253) for n in (1, 5)] +
             [(254, n, "whole") for n in (2, 3, 4)] + [(254, n, "inside") for n in range(1, 6)])


@pytest.mark.parametrize("cols,n,where", STREAMING, ids=["%d-x%d-%s" % c for c in STREAMING])
def test_stripe_entry_streaming(nj, ctxs, oracle, cols, n, where):
    if n > cap(nj):
        n = cap(nj)
    owned = stream_rows(nj, ctxs[0], cols, n)
    if not KNOBS:
        assert form(nj, ctxs[0], cols, owned, 1, n, 1, 1) == STREAM and form(nj, ctxs[0], cols, owned - 1, 1, n, 1, 1) != STREAM
    halo = 2 * n
    ci = (1, 3, 100, 131, 254, 253).index(cols)
    pitch = cols + PADS[(ci + n) % 3]
    rng = np.random.default_rng(cols * 10 + n)
    if where == "whole":     # the whole grid in one stripe
        rows, grow0, grows, own0 = owned, 0, owned, 0
        h = terrain(rng, rows, cols)
        want = oracle.flowmap(h, n, *F.NORM)
    else:                    # owned rows inside a taller grid, exactly 2n ghost rows either side
        rows, grow0, grows, own0 = owned + 2 * halo, 7, owned + 2 * halo + 14, halo
        h = terrain(rng, rows, cols)
        want = oracle.flowmap(h, n, *F.NORM)[halo:halo + owned]   # (tests/test_flow_ref.py: rows 2n from an edge do not see it)
    for mode, ctx in ctxs.items():
        sb = StripeBuffers(nj, ctx, rows, cols, pitch, second=mode == 2)
        try:
            sb.h.CopyFrom(sb.padded(h))
            run_stripe(nj, mode, sb, grow0, grows, own0, own0 + owned, n, 1, 1, [want],
                       "stream %d rows x %d cols pitch %d x%d %s" % (owned, cols, pitch, n, where))
        finally:
            sb.Dispose()


def test_stripe_entry_refusals(nj, ctxs):
    ctx, N = ctxs[0], nj._native
    cols, rows, n, top = 37, 40, 2, cap(nj)
    rng = np.random.default_rng(37)
    nan = np.full(rows * cols, np.nan, f32)
    h = ctx.from_host(terrain(rng, rows, cols))
    sin = [ctx.from_host(rng.random(rows * cols, dtype=f32) * f32(1e-4)) for _ in range(5)]
    sout = [ctx.from_host(nan) for _ in range(5)]
    dst = ctx.from_host(nan)
    whole = nj.Stripe(cols, rows, 0, rows, 0, rows, 0)
    short = nj.Stripe(cols, rows, 5, 100, 2 * n - 1, rows - 2 * n, 0)   # 2n - 1 rows above the owned ones, the grid goes on
    ok = nj.Stripe(cols, rows, 5, 100, 2 * n, rows - 2 * n, 0)

    def arr(tiles, hole=None):
        return (N.dev_ptr * 5)(*[None if k == hole else t.ptr for k, t in enumerate(tiles)])

    def refused(word, height, pin, pout, d, st, its, first, last):
        with pytest.raises(nj.NoizeError) as e:
            ctx.call("nz_flow_fused_stripe", height, pin, pout, d, C.byref(st), its, first, last, *F.NORM)
        assert e.value.status == N.NZ_ERR_INVALID and word in str(e.value), (word, str(e.value))
        ctx.synchronize()
        for t in sout + [dst]:
            assert np.isnan(t.ToArray()).all(), "refused (%s), yet an output plane was written" % word

    try:
        refused("iterations", h.ptr, arr(sin), arr(sout), None, whole, 0, 0, 0)
        refused("iterations", h.ptr, arr(sin), arr(sout), None, whole, top + 1, 0, 0)
        refused("height is NULL", None, arr(sin), arr(sout), None, whole, n, 0, 0)
        refused("state_in is NULL", h.ptr, None, arr(sout), None, whole, n, 0, 0)
        refused("state_in[2]", h.ptr, arr(sin, 2), arr(sout), None, whole, n, 0, 0)
        refused("state_out[3]", h.ptr, arr(sin), arr(sout, 3), None, whole, n, 0, 0)
        refused("state_out is NULL", h.ptr, arr(sin), None, None, whole, n, 0, 0)
        refused("dst is NULL", h.ptr, arr(sin), None, None, whole, n, 0, 1)
        refused("dst must not alias height", h.ptr, arr(sin), None, h.ptr, whole, n, 0, 1)
        refused("ghost rows", h.ptr, None, None, dst.ptr, short, n, 1, 1)
        # the same stripe with its 2n ghost rows is taken, and a first launch needs no state_in
        ctx.call("nz_flow_fused_stripe", h.ptr, None, None, dst.ptr, C.byref(ok), n, 1, 1, *F.NORM).Complete()
        out = dst.ToArray((rows, cols))
        assert np.isfinite(out[2 * n:rows - 2 * n]).all() and np.isnan(out[:2 * n]).all() and np.isnan(out[rows - 2 * n:]).all()
    finally:
        for t in [h, dst] + sin + sout:
            t.Dispose()


def test_the_query_refuses_what_no_launch_takes(nj, ctxs):
    lib, h = nj._native.lib, ctxs[0]._h
    for args in ((0, 8, 1, 1), (8, 0, 1, 1), (8, 8, 0, 1), (8, 8, 1, 0), (8, 8, 1, cap(nj) + 1)):
        assert lib.nz_flow_launch_form(h, *args, 1, 1) == nj._native.NZ_ERR_INVALID, args
    assert lib.nz_flow_launch_form(None, 8, 8, 1, 1, 1, 1) == nj._native.NZ_ERR_INVALID
    # only a whole stage streams; the tile forms do not depend on the role
    if not KNOBS:
        assert form(nj, ctxs[0], 4096, 4096, 1, 5, 1, 1) == STREAM
        assert {form(nj, ctxs[0], 4096, 4096, 1, 5, f, l) for f, l in ROLES[1:]} == {TILE48}
