"""The xi-q sediment step of nz_fluvial_sediment (include/noize_hip.h) in plain numpy, float32 throughout, every operation
rounded once: fluvial_implicit_ref's solve wrapped in K Gauss-Seidel iterations that put a deposition term into its
right-hand side (Yuan, Braun, Guerit, Rouby & Cordonnier 2019).  Planes are rows x cols arrays indexed [z, x].

    has, q, b0, f = fluvial_implicit_ref.coefficients(h, A, ...);  r, outlets as in fluvial_ref;  G = deposition
    solve(b):  h'[c] = b[c] without a receiver, else (b[c] + f[c] * h'[q[c]]) / (1 + f[c])
    h0 = solve(b0)
    for k = 1 .. K:
        e      = b0 - h(k-1)
        Q[c]   = e[c] + Q[d] over the donors d of c, neighbour order 0..7      (fluvial_ref.drainage(Q, r, e) at rest)
        Qin[c] = +0 + Q[d] over the same donors, then Qin < 0 ? +0 : Qin       (a NaN passes)
        bk[c]  = b0[c] on outlets and where not A[c] > 0, else b0[c] + (G * Qin[c]) / A[c]
        hk     = solve(bk)
    residual = max |hK - h(K-1)| taken with d > m (+0 when K = 0);  flux = Q of iteration K (+0 when K = 0)

Q is a fixed function of the final values of strictly higher cells, a solve of strictly lower ones, so every schedule ends
in the same bits:

    walk(h, A, ...) -> (h', flux, residual, residuals)   both recurrences as walks over the sorted cells
    jacobi(h, A, ...) -> the same                        every series as Jacobi steps until a step changes no bit
    tiled(h, A, ..., tile, sweeps) -> the same           every series as Jacobi inside 64 x 16 tiles against frozen rings
    history(h, A, ...) -> [(h', flux, residual)]         the walk's results at K = 0, 1, .. sedimentIterations
    series(h, A, ...) -> dict                            the planes of the last iteration, for fixed-point checks
    chain(h, iterations, ...) -> (h', A, flux, residual) the hosts' SedimentFluvialStage: drainage_ref.accumulate, then walk"""
import numpy as np

import fluvial_implicit_ref as imp
from drainage_ref import accumulate
from fluvial_ref import NEIGHBOURS, OPPOSITE, SEA_OFF, drainage, outlets, receivers

f32 = np.float32
ZERO, ONE = f32(0.0), f32(1.0)
same = imp.same
DEFAULT_G, DEFAULT_K = 0.5, 4


def _donor_planes(r):
    """Per neighbour k: (mask, index) of the donor of every cell in that direction, flat; index 0 where there is none."""
    rows, cols = r.shape
    idx = np.arange(rows * cols).reshape(rows, cols)
    masks, where = [], []
    for k, (dx, dz) in enumerate(NEIGHBOURS):
        m, d = np.zeros(r.shape, bool), np.zeros(r.shape, np.int64)
        x0, x1, z0, z1 = max(0, -dx), cols - max(0, dx), max(0, -dz), rows - max(0, dz)
        if x1 > x0 and z1 > z0:
            own, nb = (slice(z0, z1), slice(x0, x1)), (slice(z0 + dz, z1 + dz), slice(x0 + dx, x1 + dx))
            m[own] = r[nb] == OPPOSITE[k]
            d[own] = np.where(m[own], idx[nb], 0)
        masks.append(m.reshape(-1))
        where.append(d.reshape(-1))
    return masks, where


def _levels(rank):
    """The cells of every rank >= 1, lowest rank first."""
    order = np.argsort(rank, kind="stable")
    cuts = np.searchsorted(rank[order], np.arange(1, int(rank.max()) + 2 if rank.size else 1))
    return [order[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def deposit(Q, r, b0, A, out, G):
    """(Qin, bk) from the final Q of an iteration."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        qin = drainage(Q, r, np.zeros(Q.shape, f32))
        qin = np.where(qin < ZERO, ZERO, qin).astype(f32)
        term = ((f32(G) * qin) / A).astype(f32)
        bk = np.where(out | ~(A > ZERO), b0, b0 + term).astype(f32)
    return qin, bk


class _Model:
    def __init__(self, h, A, deposition, seaLevel, kw):
        self.h = np.ascontiguousarray(h, f32)
        self.A = np.ascontiguousarray(A, f32)
        self.G = deposition
        self.has, self.q, self.b0, self.f = imp.coefficients(self.h, self.A, seaLevel=seaLevel, **kw)
        self.r = receivers(self.h, seaLevel)[0]
        self.out = outlets(self.h, seaLevel)


def _iterate(m, K, solve, gather):
    """The iteration on top of a solve(b) -> h' and a gather(e) -> Q; returns (h', flux, residual, residuals, last)."""
    hk = solve(m.b0)
    flux = np.zeros(m.h.shape, f32)
    res, last = [], dict(b=m.b0, e=None, Q=None, h=hk)
    m.history = [(hk, flux, ZERO)]  # (h, flux, residual) after k = 0, 1, .. iterations
    for _ in range(K):
        with np.errstate(invalid="ignore", over="ignore"):
            e = (m.b0 - hk).astype(f32)
        Q = gather(e)
        bk = deposit(Q, m.r, m.b0, m.A, m.out, m.G)[1]
        nxt = solve(bk)
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.abs(nxt - hk).reshape(-1)
        d = d[d > ZERO]  # "d > m" from m = +0: a NaN never enters
        res.append(f32(d.max()) if d.size else ZERO)
        hk, flux = nxt, Q
        m.history.append((hk, flux, res[-1]))
        last = dict(b=bk, e=e, Q=Q, h=hk)
    return hk, flux, (res[-1] if res else ZERO), res, last


def _walks(m):
    """solve and gather as walks in dependency order: a cell after the one cell (solve) or the donors (gather) it reads.
    Cells of equal rank do not read each other and are taken together."""
    n = m.h.size
    hl, ql = m.has.reshape(-1).tolist(), m.q.reshape(-1).tolist()
    order = np.argsort(m.h.reshape(-1).astype(np.float64), kind="stable").tolist()
    depth, height = [0] * n, [0] * n
    for c in order:  # lowest first: the receiver has its depth
        if hl[c]:
            depth[c] = depth[ql[c]] + 1
    for c in reversed(order):  # highest first: every donor has its height
        if hl[c] and height[ql[c]] < height[c] + 1:
            height[ql[c]] = height[c] + 1
    up, down = _levels(np.array(depth)), _levels(np.array(height))
    qf, ff = m.q.reshape(-1), m.f.reshape(-1)
    masks, where = _donor_planes(m.r)

    def solve(b):
        hn, bf = b.reshape(-1).copy(), b.reshape(-1)
        with np.errstate(invalid="ignore", over="ignore"):
            for lv in up:
                hn[lv] = (bf[lv] + ff[lv] * hn[qf[lv]]) / (ONE + ff[lv])
        return hn.reshape(m.h.shape)

    def gather(e):
        Q = e.reshape(-1).copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for lv in down:
                a = Q[lv]
                for mk, wk in zip(masks, where):  # neighbour order 0..7
                    a = np.where(mk[lv], a + Q[wk[lv]], a)
                Q[lv] = a
        return Q.reshape(m.h.shape)

    return solve, gather


def _args(kw):
    kw = dict(kw)
    return kw.pop("deposition", DEFAULT_G), kw.pop("sedimentIterations", DEFAULT_K), kw.pop("seaLevel", SEA_OFF), kw


def walk(h, A, **kw):
    G, K, sea, kw = _args(kw)
    m = _Model(h, A, G, sea, kw)
    return _iterate(m, K, *_walks(m))[:4]


def history(h, A, **kw):
    """[(h', flux, residual)] of walk(...) at sedimentIterations = 0, 1, .. K, from one run."""
    G, K, sea, kw = _args(kw)
    m = _Model(h, A, G, sea, kw)
    _iterate(m, K, *_walks(m))
    return m.history


def series(h, A, **kw):
    G, K, sea, kw = _args(kw)
    m = _Model(h, A, G, sea, kw)
    last = _iterate(m, K, *_walks(m))[4]
    last.update(has=m.has, q=m.q, f=m.f, r=m.r)
    return last


def jacobi(h, A, **kw):
    G, K, sea, kw = _args(kw)
    m = _Model(h, A, G, sea, kw)

    def solve(b):
        hn = b.copy()
        while True:
            nxt = imp.step(hn, m.has, m.q, b, m.f)
            if same(nxt, hn):
                return hn
            hn = nxt

    def gather(e):
        Q = e.copy()
        while True:
            with np.errstate(invalid="ignore", over="ignore"):
                nxt = drainage(Q, m.r, e)
            if same(nxt, Q):
                return Q
            Q = nxt

    return _iterate(m, K, solve, gather)[:4]


def tiled(h, A, tile=(64, 16), sweeps=None, **kw):
    G, K, sea, kw = _args(kw)
    m = _Model(h, A, G, sea, kw)
    rows, cols = m.h.shape
    tx, tz = tile

    def passes(start, step):
        cur = start.copy()
        while True:
            nxt = cur.copy()
            for z0 in range(0, rows, tz):
                for x0 in range(0, cols, tx):
                    own = (slice(z0, min(z0 + tz, rows)), slice(x0, min(x0 + tx, cols)))
                    t, s = cur.copy(), 0
                    while sweeps is None or s < sweeps:
                        n = step(t)
                        if same(n[own], t[own]):
                            break
                        t[own] = n[own]
                        s += 1
                    nxt[own] = t[own]
            if same(nxt, cur):
                return cur
            cur = nxt

    def gather_step(e):
        def step(t):
            with np.errstate(invalid="ignore", over="ignore"):
                return drainage(t, m.r, e)
        return step

    return _iterate(m, K, lambda b: passes(b, lambda t: imp.step(t, m.has, m.q, b, m.f)),
                    lambda e: passes(e, gather_step(e)))[:4]


def chain(h, iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=SEA_OFF, rainMap=None, hardness=None,
          upliftMap=None, deposition=DEFAULT_G, sedimentIterations=DEFAULT_K, area=accumulate):
    """`area(h, rain, seaLevel, rainMap) -> (A, ...)`: the drainage model of the stage's routing."""
    h = np.array(h, f32)
    A, flux, residual = None, np.zeros(h.shape, f32), ZERO
    for _ in range(iterations):
        A = area(h, rain, seaLevel, rainMap)[0]
        h, flux, residual, _ = walk(h, A, erodibility=erodibility, uplift=uplift, dt=dt, seaLevel=seaLevel, hardness=hardness,
                                    upliftMap=upliftMap, deposition=deposition, sedimentIterations=sedimentIterations)
    return h, A, flux, residual
