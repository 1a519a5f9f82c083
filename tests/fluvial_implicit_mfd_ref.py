"""The multiple-flow implicit stream-power step of nz_fluvial_implicit_mfd (include/noize_hip.h) in plain numpy, float32
throughout, every operation rounded once: drainage_mfd_ref.weights, solved upstream.  Planes are rows x cols arrays indexed
[z, x], c = z * cols + x.

    du = dt * uplift (* upliftMap[c]),  kc = erodibility (* (1 - hardness[c])),  b = h[c] on an outlet, else h[c] + du
    outlet:  h'[c] = h[c]              no k with w_k > 0 (pit, flat):  h'[c] = b
    otherwise:  e = kc * sqrt(A[c]);  f_k = ((e * invL_k) * dt) * w_k for every k with w_k > 0
                N = b; D = 1; for k ascending with w_k > 0: N = N + (f_k * h'[k]); D = D + f_k;  h'[c] = N / D

The gate is w_k > 0, never the value of f_k or of h'.  A neighbour that takes flow is strictly lower in the old heights, so
the graph is a DAG whose leaves are fixed, and every schedule of updates ends in the same bits, from any start state:

    coefficients(h, A, ...) -> (G, b, F)            what the kernels' setup launch stores: G[k] the gate w_k > 0, F[k] = f_k
                                                    and +0 where the gate is shut; b is the final value where no gate is open
    step(hn, G, b, F) -> h'                         one Jacobi step, for fixed-point checks of a result
    walk(h, A, ...) -> (h', height)                 the model as a walk, cells lowest first (stable sort); height = the cells
                                                    of the longest path of the flow DAG
    jacobi(h, A, ..., start) -> (h', steps)         step until no bit changes; start "b" (the kernels') or "h"
    tiled(h, A, ..., tile, sweeps) -> (h', passes)  Jacobi inside the kernel's tiles: 64 x 16 tiles swept against frozen rings
    one_sweep_passes(h, A, limit, ...) -> passes    the pass launches the kernels need at a sweep cap of 1: a thread's four
                                                    cells left to right and back, everything else as the pass before
    single_closure(h, seaLevel, exponent) -> mask   the cells with exactly one positive weight whose whole downstream path
                                                    has exactly one too: there the model is nz_fluvial_implicit's
    chain(h, iterations, ...) -> (h', A)            the hosts' MfdFluvialStage: drainage_mfd_ref.walk, then walk, per
                                                    iteration"""
import numpy as np

import drainage_mfd_ref as M
from fluvial_ref import DIAG, NEIGHBOURS, SEA_OFF, _window, outlets

f32 = np.float32
ONE = f32(1.0)
INV_L = tuple(ONE if k < 4 else DIAG for k in range(8))
DEFAULTS = dict(iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=float(SEA_OFF), exponent=1)
same = M.same


def coefficients(h, A, erodibility=0.05, uplift=0.002, dt=1.0, seaLevel=SEA_OFF, exponent=1, hardness=None, upliftMap=None):
    h = np.ascontiguousarray(h, f32)
    A = np.ascontiguousarray(A, f32)
    W = M.weights(h, seaLevel, exponent)
    G = W > 0
    du = f32(dt) * f32(uplift)
    if upliftMap is not None:
        du = du * np.asarray(upliftMap, f32)
    kc = f32(erodibility) if hardness is None else f32(erodibility) * (ONE - np.asarray(hardness, f32))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        b = np.where(outlets(h, seaLevel), h, h + du).astype(f32)
        e = (kc * np.sqrt(A)).astype(f32)
        F = np.zeros(W.shape, f32)
        for k in range(8):
            F[k] = np.where(G[k], ((e * INV_L[k]) * f32(dt)) * W[k], f32(0.0))
    return G, b, F


def step(hn, G, b, F):
    """One Jacobi step: every cell with an open gate from the cells its gates name."""
    N, D = b.copy(), np.ones(b.shape, f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for k, (dx, dz) in enumerate(NEIGHBOURS):
            c, n = _window(hn.shape, dx, dz)
            g = G[k][c]
            N[c] = np.where(g, N[c] + F[k][c] * hn[n], N[c])
            D[c] = np.where(g, D[c] + F[k][c], D[c])
        return np.where(G.any(axis=0), N / D, hn).astype(f32)


def walk(h, A, **kw):
    h = np.ascontiguousarray(h, f32)
    G, b, F = coefficients(h, A, **kw)
    cols = h.shape[1]
    hn = b.reshape(-1).copy()
    Gl, Fl = G.reshape(8, -1), F.reshape(8, -1)
    opens = G.any(axis=0).reshape(-1).tolist()
    height = [1] * h.size
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for c in np.argsort(h.reshape(-1).astype(np.float64), kind="stable").tolist():
            if not opens[c]:
                continue
            n, d, deep = hn[c], ONE, 0
            for k, (dx, dz) in enumerate(NEIGHBOURS):
                if Gl[k, c]:  # the neighbour exists and is strictly lower: it has its final value already
                    q = c + dz * cols + dx
                    n = f32(n + f32(Fl[k, c] * hn[q]))
                    d = f32(d + Fl[k, c])
                    deep = max(deep, height[q])
            hn[c] = f32(n / d)
            height[c] = deep + 1
    return hn.reshape(h.shape), max(height)


def jacobi(h, A, start="b", **kw):
    G, b, F = coefficients(h, A, **kw)
    hn, steps = {"b": b, "h": np.ascontiguousarray(h, f32)}[start].copy(), 0
    if start == "h":  # the leaves take their final value in the first step
        hn = np.where(G.any(axis=0), hn, b)
    while True:
        nxt = step(hn, G, b, F)
        if same(nxt, hn):
            return hn, steps
        hn, steps = nxt, steps + 1


def tiled(h, A, tile=(64, 16), sweeps=None, **kw):
    G, b, F = coefficients(h, A, **kw)
    hn, passes = b.copy(), 0
    rows, cols = hn.shape
    tx, tz = tile
    while True:
        nxt = hn.copy()
        for z0 in range(0, rows, tz):
            for x0 in range(0, cols, tx):
                z1, x1 = min(z0 + tz, rows), min(x0 + tx, cols)
                # the tile with its ring, cut from the state of the pass before; the ring is never written.  An open gate
                # never points out of the grid, so the cut's coefficients are the whole plane's
                za, xa, zb, xb = max(z0 - 1, 0), max(x0 - 1, 0), min(z1 + 1, rows), min(x1 + 1, cols)
                own = (slice(z0 - za, z1 - za), slice(x0 - xa, x1 - xa))
                t, gg, bb, ff = hn[za:zb, xa:xb].copy(), G[:, za:zb, xa:xb], b[za:zb, xa:xb], F[:, za:zb, xa:xb]
                s = 0
                while sweeps is None or s < sweeps:
                    n = step(t, gg, bb, ff)
                    if same(n[own], t[own]):
                        break
                    t[own] = n[own]
                    s += 1
                nxt[z0:z1, x0:x1] = t[own]
        if same(nxt, hn):
            return hn, passes
        hn, passes = nxt, passes + 1


def one_sweep_passes(h, A, limit, **kw):
    """The kernel's schedule at a sweep cap of 1, exactly: per pass every aligned group of four cells of a row is updated in
    the order 0 1 2 3 2 1 0, a W or E neighbour inside the group taken as just updated, every other cell as the pass before
    left it.  -> the passes run until one changes no bit, that one included; None beyond `limit`."""
    G, b, F = coefficients(h, A, **kw)
    opens, xs = G.any(axis=0), np.arange(b.shape[1])
    prev = b.copy()
    for passes in range(1, limit + 1):
        cur = prev.copy()
        for j in (0, 1, 2, 3, 2, 1, 0):
            N, D = b.copy(), np.ones(b.shape, f32)
            with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
                for k, (dx, dz) in enumerate(NEIGHBOURS):
                    c, n = _window(b.shape, dx, dz)
                    src = cur if (k == 0 and j > 0) or (k == 1 and j < 3) else prev
                    N[c] = np.where(G[k][c], N[c] + F[k][c] * src[n], N[c])
                    D[c] = np.where(G[k][c], D[c] + F[k][c], D[c])
                new = np.where(opens, N / D, cur).astype(f32)
            cur[:, xs % 4 == j] = new[:, xs % 4 == j]
        if same(cur, prev):
            return passes
        prev = cur
    return None


def single_closure(h, seaLevel=SEA_OFF, exponent=1):
    """The cells with exactly one positive weight whose target has none (an outlet, a pit) or is in the closure itself."""
    h = np.ascontiguousarray(h, f32)
    G = M.weights(h, seaLevel, exponent) > 0
    cols = h.shape[1]
    count = G.sum(axis=0).reshape(-1).tolist()
    Gl = G.reshape(8, -1)
    closed = [False] * h.size
    for c in np.argsort(h.reshape(-1).astype(np.float64), kind="stable").tolist():
        if count[c] == 1:
            k = int(np.argmax(Gl[:, c]))
            q = c + NEIGHBOURS[k][1] * cols + NEIGHBOURS[k][0]
            closed[c] = count[q] == 0 or closed[q]
    return np.array(closed).reshape(h.shape)


def chain(h, iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=SEA_OFF, exponent=1, rainMap=None,
          hardness=None, upliftMap=None):
    h = np.array(h, f32)
    A = None
    for _ in range(iterations):
        A = M.walk(h, rain, seaLevel, rainMap, exponent)[0]
        h = walk(h, A, erodibility=erodibility, uplift=uplift, dt=dt, seaLevel=seaLevel, exponent=exponent, hardness=hardness,
                 upliftMap=upliftMap)[0]
    return h, A
