"""The pass protocol and the tile schedule of the seven iterate-to-rest series in plain numpy, stated once: what a series of
launches does, launch by launch, as csrc/nz_relax_pass.hpp, csrc/nz_tile64.hpp and the header comment of each .hip file
state it.  The tiled() models of the *_ref.py files are Jacobi inside a tile and cannot predict a pass count; this one can.

    geometry   64 x 16 tiles over rows x cols; the planes of a batch are independent and share one pass word (run_batch)
    pass 0     starts from the family's start state, visits every tile, and moves by decree
    pass p     runs only if pass p - 1 moved a tile (the gate); a tile is visited only if it or one of its eight neighbours
               inside the plane moved in pass p - 1 (the skip); a skipped tile's byte is zero
    a visit    the ring is frozen at the state of the pass's start; up to `sweeps` sweeps; in a sweep every thread -- four
               consecutive cells of a row, starting at a multiple of 4 -- updates its cells in the order 0 1 2 3 2 1 0, its
               own cells from its registers, every other cell from the LDS snapshot of the sweep's start; the loop ends at
               the first sweep without a change, and the tile's byte is "some sweep changed"
    a change   the family's own rule: the fill looks at the net effect of a sweep on the thread's cells (W only falls), the
               other six at every single update, by bits
    the end    `passes` is the status word: the passes that ran, the one that found rest included; converged is "the last
               pass that ran moved no tile"

run() returns the planes, passes, converged and, per pass that ran, the map of tiles that moved (the byte generation the
pass wrote) and the map of tiles visited.  `wake` ("eight", "four", "self") and `order` (a tuple of cell numbers, or JACOBI:
every cell once from the snapshot) exist so that the tests can break the model and see which inputs notice.

The seven families plug in one cell update each, built from the *_ref.py functions for outlets, receivers, donor bits,
weights, b and f.  tile_bytes() reads the moved maps back out of a stage's `work` buffer; the layout it assumes is
relax_work's in csrc/nz_terrain_stages.cpp ("begins the same way for all of them").  wake_tiles() are the directed inputs
on which a broken skip shows in the result."""
import numpy as np

import drainage_mfd_ref as M
import drainage_ref as D
import fill_ref as L
import fluvial_implicit_mfd_ref as IM
import fluvial_implicit_ref as I
import stream_order_ref as S
import watershed_ref as WS
from fluvial_ref import NEIGHBOURS, NONE, SEA_OFF, outlets, rain_plane, receivers

f32 = np.float32
FX, FZ = 64, 16                 # nz_tile64.hpp: the tile
ORDER = (0, 1, 2, 3, 2, 1, 0)   # a thread's four cells, left to right and back
JACOBI = "jacobi"               # the mutant: every cell once, from the snapshot
WAKES = {"eight": [(dx, dz) for dz in (-1, 0, 1) for dx in (-1, 0, 1)],
         "four": [(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)],
         "self": [(0, 0)]}


def tiles_of(rows, cols):
    return -(-rows // FZ), -(-cols // FX)


def _bits(a):
    return a.view(np.uint32) if a.dtype == f32 else a


class Family:
    """A family: the start planes and one cell update.  Planes are padded to whole tiles; a cell outside the grid holds
    `outside` and is never updated (its update returns what it has)."""
    net = False  # "changed" is the net effect of a sweep (the fill) instead of every single update

    def __init__(self, shape):
        self.rows, self.cols = shape
        self.tnz, self.tnx = tiles_of(*shape)

    def pad(self, a, fill):
        out = np.full((self.tnz * FZ, self.tnx * FX), fill, a.dtype)
        out[:self.rows, :self.cols] = a
        return out

    def crop(self, a):
        return np.ascontiguousarray(a[:self.rows, :self.cols])


class Fill(Family):
    """nz_fill.hip: W = max(h, min over the eight neighbours + epsilon) off the outlets."""
    net = True

    def __init__(self, h, epsilon=1e-4, seaLevel=SEA_OFF):
        h = np.ascontiguousarray(h, f32)
        super().__init__(h.shape)
        self.h, self.fixed = self.pad(h, f32(0)), self.pad(outlets(h, seaLevel), True)
        self.eps = f32(epsilon) + f32(0.0)
        self.start, self.outside = [self.pad(L.start(h, seaLevel), L.INF)], [L.INF]

    def update(self, sl, own, nb):
        mn = nb(0)[0]
        for k in range(1, 8):
            mn = np.minimum(mn, nb(k)[0])
        m, h = mn + self.eps, self.h[sl]
        return [np.where(self.fixed[sl], own[0], np.where(h > m, h, m))]


class Drainage(Family):
    """nz_drainage.hip: A = rain_c + the A of the donors, k ascending."""

    def __init__(self, h, rain=1.0, seaLevel=SEA_OFF, rainMap=None):
        h = np.ascontiguousarray(h, f32)
        super().__init__(h.shape)
        rc = rain_plane(h.shape, rain, rainMap)
        don = self.pad(S.donor_bits(h, seaLevel)[1], 0)
        self.rc, self.don = self.pad(rc, f32(0)), [(don >> k) & 1 != 0 for k in range(8)]  # per k: is neighbour k a donor
        self.start, self.outside = [self.pad(rc, f32(0))], [f32(0)]

    def update(self, sl, own, nb):
        a = self.rc[sl]
        for k in range(8):
            a = np.where(self.don[k][sl], a + nb(k)[0], a)
        return [a]


class DrainageMfd(Family):
    """nz_drainage_mfd.hip: A = rain_c + w * A over the incoming weights w > 0, k ascending."""

    def __init__(self, h, rain=1.0, seaLevel=SEA_OFF, rainMap=None, exponent=1):
        h = np.ascontiguousarray(h, f32)
        super().__init__(h.shape)
        rc = rain_plane(h.shape, rain, rainMap)
        self.rc = self.pad(rc, f32(0))
        self.w = [self.pad(w, f32(0)) for w in M.incoming(M.weights(h, seaLevel, exponent))]
        self.on = [w > 0 for w in self.w]
        self.start, self.outside = [self.pad(rc, f32(0))], [f32(0)]

    def update(self, sl, own, nb):
        a = self.rc[sl]
        for k in range(8):
            a = np.where(self.on[k][sl], a + self.w[k][sl] * nb(k)[0], a)
        return [a]


class Watershed(Family):
    """nz_watershed.hip: basin and length from the cell the receiver code names."""

    def __init__(self, h, seaLevel=SEA_OFF, cellSize=1.0, length=True):
        h = np.ascontiguousarray(h, f32)
        super().__init__(h.shape)
        r = receivers(h, seaLevel)[0]
        self.st = self.pad(WS.steps_of(cellSize)[r], f32(0))
        self.at = [self.pad(r == k, False) for k in range(8)]  # per k: does the receiver code name neighbour k
        self.start = [self.pad(np.arange(h.size, dtype=np.int32).reshape(h.shape), 0)]
        self.outside = [np.int32(0)]
        if length:
            self.start.append(self.pad(np.zeros(h.shape, f32), f32(0)))
            self.outside.append(f32(0))

    def update(self, sl, own, nb):
        new = list(own)
        for k in range(8):
            at, v = self.at[k][sl], nb(k)
            new[0] = np.where(at, v[0], new[0])
            if len(own) > 1:
                new[1] = np.where(at, v[1] + self.st[sl], new[1])
        return new


class StreamOrder(Family):
    """nz_stream_order.hip: order = max(m1, m2 + 1) over the two largest donor orders; link from the one donor."""

    def __init__(self, h, seaLevel=SEA_OFF, drainage=None, threshold=0.0, links=True):
        h = np.ascontiguousarray(h, f32)
        super().__init__(h.shape)
        ch, bits = S.donor_bits(h, seaLevel, drainage, threshold)
        self.don = self.pad(np.where(ch, bits, 0).astype(np.uint8), 0)  # no channel: the donor byte is dropped
        self.bit = [(self.don >> k) & 1 != 0 for k in range(8)]
        self.one = [self.don == (1 << k) for k in range(8)]  # neighbour k is the one donor
        self.any = self.don != 0
        order, link = S.start(ch)
        self.start, self.outside = [self.pad(order, 0)], [np.uint8(0)]
        if links:
            self.start.append(self.pad(link, -1))
            self.outside.append(np.int32(-1))

    def update(self, sl, own, nb):
        m1 = m2 = np.zeros(own[0].shape, np.uint8)  # (order <= 31: a byte holds m2 + 1)
        vs = [nb(k) for k in range(8)]
        for k in range(8):
            v = np.where(self.bit[k][sl], vs[k][0], np.uint8(0))
            m2 = np.maximum(m2, np.minimum(m1, v))
            m1 = np.maximum(m1, v)
        new = [np.where(self.any[sl], np.maximum(m1, m2 + np.uint8(1)), own[0])]
        if len(own) > 1:  # a head and a confluence keep their own index, which the start state holds
            l = own[1]
            for k in range(8):
                l = np.where(self.one[k][sl], vs[k][1], l)
            new.append(l)
        return new


class FluvialImplicit(Family):
    """nz_fluvial_implicit.hip: h' = (b + f * h'[receiver]) / (1 + f)."""

    def __init__(self, h, A, seaLevel=SEA_OFF, **kw):
        h = np.ascontiguousarray(h, f32)
        super().__init__(h.shape)
        _, _, b, f = I.coefficients(h, A, seaLevel=seaLevel, **kw)
        r = receivers(h, seaLevel)[0]
        self.at, self.has = [self.pad(r == k, False) for k in range(8)], self.pad(r != NONE, False)
        self.b, self.f = self.pad(b, f32(0)), self.pad(f, f32(0))
        self.start, self.outside = [self.pad(b, f32(0))], [f32(0)]

    def update(self, sl, own, nb):
        b, f = self.b[sl], self.f[sl]
        q = own[0]
        for k in range(8):
            q = np.where(self.at[k][sl], nb(k)[0], q)
        return [np.where(self.has[sl], (b + f * q) / (I.ONE + f), own[0])]


class FluvialImplicitMfd(Family):
    """nz_fluvial_implicit_mfd.hip: h' = (b + sum f_k * h'[k]) / (1 + sum f_k) over the open gates, k ascending."""

    def __init__(self, h, A, **kw):
        h = np.ascontiguousarray(h, f32)
        super().__init__(h.shape)
        G, b, F = IM.coefficients(h, A, **kw)
        self.g = [self.pad(g, False) for g in G]
        self.fk = [self.pad(fk, f32(0)) for fk in F]
        self.b, self.open = self.pad(b, f32(0)), self.pad(G.any(axis=0), False)
        d = np.ones(self.b.shape, f32)  # D is rebuilt from the f, k ascending over the gates
        for k in range(8):
            d = np.where(self.g[k], d + self.fk[k], d)
        self.d = d
        self.start, self.outside = [self.pad(b, f32(0))], [f32(0)]

    def update(self, sl, own, nb):
        n = self.b[sl]
        for k in range(8):
            n = np.where(self.g[k][sl], n + self.fk[k][sl] * nb(k)[0], n)
        return [np.where(self.open[sl], n / self.d[sl], own[0])]


FAMILIES = {"fill": Fill, "drainage": Drainage, "drainage_mfd": DrainageMfd, "watershed": Watershed,
            "stream_order": StreamOrder, "fluvial_implicit": FluvialImplicit, "fluvial_implicit_mfd": FluvialImplicitMfd}


class Result:
    """planes: the state when the series stopped (of the grid's shape); passes, converged: the status words; moved[p],
    visited[p]: the tiles [tile row, tile column] that moved in pass p (its byte generation) and that it visited."""

    def __init__(self, planes, passes, converged, moved, visited):
        self.planes, self.passes, self.converged, self.moved, self.visited = planes, passes, converged, moved, visited


def woken(moved, wake="eight"):
    """The tiles the pass behind `moved` visits: tile_live, over the neighbours inside the plane."""
    tnz, tnx = moved.shape
    pad = np.pad(moved, 1)
    live = np.zeros_like(moved)
    for dx, dz in WAKES[wake]:
        live |= pad[1 + dz:1 + dz + tnz, 1 + dx:1 + dx + tnx]
    return live


def _same_tile(Z, X):
    """Per neighbour k: does the neighbour of cell [z, x] lie in the cell's own tile (else it is a ring cell)?"""
    z, x = np.arange(Z)[:, None] % FZ, np.arange(X)[None, :] % FX
    return [((x + dx >= 0) & (x + dx < FX)) & ((z + dz >= 0) & (z + dz < FZ)) for dx, dz in NEIGHBOURS]


def run(fam, sweeps=16, budget=None, wake="eight", order=ORDER):
    """The series of one plane: at most `budget` launches (None: until the gate closes), `sweeps` the cap."""
    tnz, tnx = fam.tnz, fam.tnx
    Z, X = tnz * FZ, tnx * FX
    same = _same_tile(Z, X)
    registers = order != JACOBI
    cells = (0, 1, 2, 3) if not registers else tuple(order)
    # P: the planes at the start of the pass, with a rim of cells outside the grid
    P = [np.pad(s, 1, constant_values=o) for s, o in zip(fam.start, fam.outside)]
    n = len(P)
    moved_maps, visited_maps = [], []
    p = 0
    with np.errstate(all="ignore"):
        while budget is None or p < budget:
            if p and not moved_maps[-1].any():
                break  # the gate: the pass before changed nothing, this launch and every later one returns at once
            visit = woken(moved_maps[-1], wake) if p else np.ones((tnz, tnx), bool)
            moved = np.zeros((tnz, tnx), bool)
            lds = [a.copy() for a in P]  # the own cells as the last write phase left them; P is the frozen ring
            act = visit.copy()
            for _ in range(sweeps):
                if not act.any():
                    break  # every visited tile has left its loop
                # only the box of the tiles still in their loop is worked on
                tz, tx = np.nonzero(act.any(axis=1))[0], np.nonzero(act.any(axis=0))[0]
                za, zb, xa, xb = tz[0] * FZ, (tz[-1] + 1) * FZ, tx[0] * FX, (tx[-1] + 1) * FX
                box, tbox = (slice(za, zb), slice(xa, xb)), (slice(tz[0], tz[-1] + 1), slice(tx[0], tx[-1] + 1))

                def shifted(a, k):  # neighbour k of every cell of the box, from a rimmed plane
                    dx, dz = NEIGHBOURS[k]
                    return a[1 + za + dz:1 + zb + dz, 1 + xa + dx:1 + xb + dx]

                cell_act = np.repeat(np.repeat(act[tbox], FZ, axis=0), FX, axis=1)
                snap = [[np.where(same[k][box], shifted(lds[i], k), shifted(P[i], k)) for i in range(n)] for k in range(8)]
                V = [a[1:-1, 1:-1][box].copy() for a in lds]  # the registers: at a sweep's start they equal LDS
                before = [v.copy() for v in V] if fam.net else None
                ch = np.zeros(cell_act.shape, bool)
                for j in cells:
                    here = (slice(None), slice(j, None, 4))
                    own = [v[here] for v in V]

                    def nb(k):
                        if registers and k == 0 and j > 0:  # a W or E neighbour among the thread's own four
                            return [v[:, j - 1::4] for v in V]
                        if registers and k == 1 and j < 3:
                            return [v[:, j + 1::4] for v in V]
                        return [snap[k][i][here] for i in range(n)]

                    new = fam.update((slice(za, zb), slice(xa + j, xb, 4)), own, nb)
                    for i in range(n):
                        nw = np.where(cell_act[here], new[i], own[i]).astype(own[i].dtype)
                        if not fam.net:
                            ch[here] |= _bits(nw) != _bits(own[i])
                        V[i][here] = nw
                if fam.net:
                    for i in range(n):
                        ch |= _bits(V[i]) != _bits(before[i])
                tch = ch.reshape(tz[-1] + 1 - tz[0], FZ, tx[-1] + 1 - tx[0], FX).any(axis=(1, 3))
                moved[tbox] |= tch
                act[tbox] &= tch  # a tile whose sweep changed nothing leaves the loop
                for i in range(n):
                    lds[i][1:-1, 1:-1][box] = V[i]
            P = lds
            if p == 0:
                moved[:] = True  # by decree
            moved_maps.append(moved)
            visited_maps.append(visit)
            p += 1
    # series_at_rest: the word of the last pass that ran (pass 0's is 1 by decree)
    return Result([fam.crop(a[1:-1, 1:-1]) for a in P], p, int(not moved_maps[-1].any()), moved_maps, visited_maps)


def run_batch(fams, **kw):
    """The planes of a batch: each runs as alone, the pass word is shared -- the series goes on while any plane moves -- and
    a plane at rest has every tile skipped.  The maps are stacked [plane, tile row, tile column]."""
    return as_batch([run(f, **kw) for f in fams])


def as_batch(rs):
    """The batch of planes whose runs alone (same cap, same budget) are `rs`."""
    passes = max(r.passes for r in rs)

    def stack(which):
        return [np.stack([getattr(r, which)[p] if p < r.passes else np.zeros_like(getattr(r, which)[0]) for r in rs])
                for p in range(passes)]
    return Result([r.planes for r in rs], passes, int(all(r.converged for r in rs)), stack("moved"), stack("visited"))


# ---- the moved maps of a real run, out of `work` ----
# The layout is relax_work's in csrc/nz_terrain_stages.cpp ("begins the same way for all of them"): 16 status words, then two
# generations of one byte per tile of the call, each rounded up to 16 bytes; run_tile_series has pass p write generation
# p & 1.  tools/bench_fluvial_implicit_mfd.py reads the same bytes.  A layout change fails here, in one place.
STATUS_WORDS = 16


def tile_bytes(work_bytes, rows, cols, count, p):
    """The byte generation pass p wrote, as [plane, tile row, tile column] bools, out of the first bytes of a stage's `work`
    (a uint8 array): generation p & 1, each generation rounded up to 16 bytes."""
    tnz, tnx = tiles_of(rows, cols)
    tiles = tnz * tnx * count
    gen = (tiles + 15) // 16 * 16
    at = 4 * STATUS_WORDS + gen * (p & 1)
    return work_bytes[at:at + tiles].reshape(count, tnz, tnx) != 0


def head_bytes(rows, cols, count):
    """The bytes of `work` that hold the status words and the two byte generations."""
    tnz, tnx = tiles_of(rows, cols)
    return 4 * STATUS_WORDS + 2 * ((tnz * tnx * count + 15) // 16 * 16)


# ---- a family by name: the model, and the walk it must end in ----
def model(family, h, **kw):
    return FAMILIES[family](h, **kw)


def walk(family, h, **kw):
    """The planes of the family's walk (the *_ref.py reference), in the order of the model's planes."""
    if family == "fill":
        return [L.flood(h, kw.get("epsilon", 1e-4), kw.get("seaLevel", SEA_OFF))]
    if family == "drainage":
        return [D.accumulate(h, **kw)[0]]
    if family == "drainage_mfd":
        return [M.walk(h, **kw)[0]]
    if family == "watershed":
        kw = dict(kw)
        length = kw.pop("length", True)
        return list(WS.walk(h, **kw)[:2 if length else 1])
    if family == "stream_order":
        kw = dict(kw)
        links = kw.pop("links", True)
        return list(S.walk(h, **kw)[:2 if links else 1])
    if family == "fluvial_implicit":
        return [I.walk(h, kw["A"], **{k: v for k, v in kw.items() if k != "A"})]
    assert family == "fluvial_implicit_mfd"
    return [IM.walk(h, kw["A"], **{k: v for k, v in kw.items() if k != "A"})[0]]


def same_planes(got, want):
    return len(got) == len(want) and all(
        a.dtype == np.asarray(b).dtype and np.array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b)))
        for a, b in zip(got, want))


# ---- wake-up tiles: one channel between walls, along which a front travels ----
WALL = f32(1e4)


def diagonal_cells(res, zc, xc, sx, sz, margin=2):
    """The cells (z, x), head first, of the straight diagonal that flows in direction (sx, sz) through the tile corner
    (zc, xc): from the tile behind the corner into its diagonal neighbour, touching neither edge neighbour with a channel
    cell.  It starts `margin` cells inside the grid and ends on the border cell it runs into, the outlet."""
    z, x = (zc - 1 if sz > 0 else zc), (xc - 1 if sx > 0 else xc)  # the last cell before the corner
    while margin <= z - sz <= res - 1 - margin and margin <= x - sx <= res - 1 - margin:
        z, x = z - sz, x - sx
    cells = [(z, x)]
    while 0 < z < res - 1 and 0 < x < res - 1:
        z, x = z + sz, x + sx
        cells.append((z, x))
    return cells


def column_cells(res, x, sz=1, margin=2):
    """A channel down (sz = 1) or up column x: it crosses tiles through their edges only."""
    zs = range(margin, res) if sz > 0 else range(res - 1 - margin, -1, -1)
    return [(z, x) for z in zs]


def channel(res, cells, top=None):
    """Walls of 1e4 and the channel `cells`, descending 0.25 per cell from `top` (default: down to 0 on the outlet)."""
    h = np.full((res, res), WALL, f32)
    top = f32(0.25) * f32(len(cells) - 1) if top is None else f32(top)
    for i, (z, x) in enumerate(cells):
        h[z, x] = top - f32(0.25) * f32(i)
    return h


def front_case(family, res, cells):
    """(h, kw) for `family`: the channel with whatever turns the family's iteration into a front along it.
    drainage, drainage_mfd  a rain map that is 1 on the head and 0 elsewhere: A is 0 until the source's water arrives
    stream_order            the channel as the `drainage` plane at threshold 0.5, and the two wall cells behind the head (they
                            drain into it) marked as channel too: the head is a confluence, and order 2 travels down a
                            channel that the start state holds at order 1.  Order only: a link is copied down a reach from
                            its head, so with the link plane every channel cell changes in every pass until it is final, as
                            in the watershed, and no tile ever rests before it is woken
    fill                    epsilon 0 (the walls are final at 1e4 as soon as the border's level reaches them); the front
                            climbs the channel from the outlet
    the implicit solves     heights below zero with an uplift map of -h on the channel, uplift 1 and dt 1: b is +0 on every
                            channel cell and the start state is at rest there until the outlet's value climbs; A is 1e6 on
                            the channel and 0 on the walls, whose f is then +0: they hold b for good
    watershed               nothing turns it into a front (test_relax_schedule says why); the plain channel"""
    (z0, x0), (z1, x1) = cells[0], cells[1]
    if family in ("drainage", "drainage_mfd"):
        rm = np.zeros((res, res), f32)
        rm[z0, x0] = 1
        return channel(res, cells), dict(rainMap=rm)
    if family == "stream_order":
        dr = np.zeros((res, res), f32)
        for z, x in cells:
            dr[z, x] = 1
        if z1 != z0 and x1 != x0:
            dr[z0, x0 - (x1 - x0)] = dr[z0 - (z1 - z0), x0] = 1
        elif x1 == x0:  # a column: the cells beside the head
            dr[z0, x0 - 1] = dr[z0, x0 + 1] = 1
        else:           # a row: the cells above and below it
            dr[z0 - 1, x0] = dr[z0 + 1, x0] = 1
        return channel(res, cells), dict(drainage=dr, threshold=0.5, links=False)
    if family == "fill":
        return channel(res, cells), dict(epsilon=0.0)
    if family == "watershed":
        return channel(res, cells), {}
    assert family in ("fluvial_implicit", "fluvial_implicit_mfd")
    h = channel(res, cells, top=-0.25)
    on = h < 0
    return h, dict(A=np.where(on, f32(1e6), f32(0)).astype(f32), uplift=1.0, dt=1.0,
                   upliftMap=np.where(on, -h, f32(0)).astype(f32))


def row_cells(res, z, sx=1, margin=2):
    """A channel along row z, eastward (sx = 1) or westward: a thread's four cells lie along it, so the order inside a
    thread decides how far a sweep carries the front."""
    xs = range(margin, res) if sx > 0 else range(res - 1 - margin, -1, -1)
    return [(z, x) for x in xs]


# The fronts of drainage, drainage_mfd and stream_order travel downstream, those of the fill and the implicit solves climb from
# the outlet, so what crosses a corner in direction (sx, sz) for the first group crosses it in (-sx, -sz) for the second.  A
# front that meets its corner in pass 0 or 1 proves nothing (every tile is visited then), so the long arm of the diagonal
# has to lie behind the corner: at 66^2, whose one corner column is x = 64, that fixes sx per group.  130^2 has room for the
# other two directions, and for the main diagonal, which crosses both (64, 64) and (128, 128).
DOWNSTREAM = ("drainage", "drainage_mfd", "stream_order")
UPSTREAM = ("fill", "fluvial_implicit", "fluvial_implicit_mfd")
DIAGONALS = ((66, 32, 64, 1, 1), (66, 32, 64, 1, -1), (130, 48, 64, -1, 1), (130, 48, 64, -1, -1), (130, 64, 64, 1, 1))


class WakeTile:
    """One directed tile: name, family, kind ("diagonal": the front crosses a tile corner while both edge neighbours rest;
    "column", "row": it crosses edges, into tiles that have rested), the inputs (h, kw) and the front's direction."""

    def __init__(self, family, kind, res, cells, heading):
        self.family, self.kind, self.res, self.heading = family, kind, res, heading
        self.h, self.kw = front_case(family, res, cells)
        self.name = "%s %s %d^2 heading %+d%+d from (%d, %d)" % ((family, kind, res) + heading + cells[0])

    def model(self):
        return model(self.family, self.h, **self.kw)

    def walk(self):
        return walk(self.family, self.h, **self.kw)


def wake_tiles(family):
    """The directed tiles of a family.  The watershed has none: see test_relax_schedule."""
    if family == "watershed":
        return []
    flip = -1 if family in UPSTREAM else 1  # the channel flows against an upstream front
    out = []
    for res, zc, xc, sx, sz in DIAGONALS:
        if (res, zc) == (130, 64):  # the main diagonal serves both groups as it is
            out.append(WakeTile(family, "diagonal", res, diagonal_cells(res, zc, xc, sx, sz), (sx * flip, sz * flip)))
        else:
            out.append(WakeTile(family, "diagonal", res, diagonal_cells(res, zc, xc, sx * flip, sz * flip), (sx, sz)))
    # a column at 66^2: tile row k is woken in pass k at the default cap, after k - 2 passes of rest -- odd and even
    out.append(WakeTile(family, "column", 66, column_cells(66, 10, flip, margin=2 if flip > 0 else 1), (0, 1)))
    out.append(WakeTile(family, "row", 130, row_cells(130, 10, flip), (1, 0)))
    return out


def rests(result):
    """The lengths of the runs of skipped passes behind which a tile was visited and moved."""
    out = set()
    idle = np.zeros(result.moved[0].shape, np.int64)
    for visited, moved in zip(result.visited, result.moved):
        out |= set(idle[moved & (idle > 0)].tolist())
        idle = np.where(visited, 0, idle + 1)
    return out


def usual_case(family, relief):
    """(h, kw) for `family` on a relief tile, the way its own tests feed it: the fill takes the relief as it is, the others
    the filled relief (priority-flood, epsilon 1e-4) with a rain map, a drainage plane and threshold, or a hardness and an
    uplift map where the family has one."""
    relief = np.ascontiguousarray(relief, f32)
    if family == "fill":
        return relief, dict(epsilon=1e-4)
    h = L.flood(relief, 1e-4)
    rng = np.random.default_rng(100 + h.shape[0] + h.shape[1])
    rm = (rng.random(h.shape, dtype=f32) * f32(1.5) + f32(0.25)).astype(f32)
    if family == "drainage":
        return h, dict(rain=0.75, rainMap=rm)
    if family == "drainage_mfd":
        return h, dict(rain=0.75, rainMap=rm, exponent=2)
    if family == "watershed":
        return h, dict(cellSize=1.0, length=True)
    if family == "stream_order":
        return h, dict(drainage=D.accumulate(h)[0], threshold=8.0, links=True)
    maps = dict(hardness=rng.random(h.shape, dtype=f32), upliftMap=(rng.random(h.shape, dtype=f32) * f32(2.0)).astype(f32))
    if family == "fluvial_implicit":
        return h, dict(A=D.accumulate(h)[0], dt=50.0, **maps)
    assert family == "fluvial_implicit_mfd"
    return h, dict(A=M.walk(h)[0], dt=50.0, exponent=2, **maps)


def nothing(family, h, **kw):
    """The "nothing" of all or nothing: what an entry returns in the model's planes when its budget ran out -- the start
    state, or for the fill and the implicit solves (whose start state is no result) the heights as they were."""
    h = np.ascontiguousarray(h, f32)
    if family in ("fill", "fluvial_implicit", "fluvial_implicit_mfd"):
        return [h]
    fam = model(family, h, **kw)
    return [fam.crop(s) for s in fam.start]
