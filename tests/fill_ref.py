"""Depression filling in plain numpy: the model of nz_fill_depressions (include/noize_hip.h), float32 throughout.  Planes
are res x res arrays indexed [z, x] (any rows x cols grid works).

    Outlets: border cells and cells with h <= seaLevel (fluvial_ref.outlets); W = h there.
    Operator at every other cell: m = +inf; for k ascending: t = W[k] + epsilon; m = t < m ? t : m; F(W) = h > m ? h : m.
    Start: W = +inf at the non-outlets.  Result: the fixed point reached from that start.

Three schedules that must give the same floats:
    flood(h, epsilon, seaLevel)                       a heap priority-flood, cell by cell in order of W
    jacobi(h, epsilon, seaLevel) -> (W, passes)       the whole grid at once, pass after pass
    tiled(h, epsilon, seaLevel, tile, sweeps) -> (W, passes)
                                                      Jacobi inside the kernel's tiles: per pass every tile of `tile` = (columns, rows)
                                                      cells sweeps against the frozen ring of the pass before, until a sweep
                                                      changes nothing or `sweeps` of them are done
`passes` counts the passes that changed a cell.  tiled(..., record=[]) appends one bool array per pass, the last one
included: which tiles [tile row, tile column] changed a cell in it."""
import heapq

import numpy as np

from fluvial_ref import NEIGHBOURS, SEA_OFF, _window, outlets

f32 = np.float32
INF = f32(np.inf)


def start(h, seaLevel=SEA_OFF):
    h = np.asarray(h, f32)
    return np.where(outlets(h, seaLevel), h, INF).astype(f32)


def step(W, h, out, eps):
    """F(W): one application of the operator to every cell."""
    m = np.full(h.shape, INF, f32)
    for dx, dz in NEIGHBOURS:
        c, n = _window(h.shape, dx, dz)
        t = W[n] + eps
        m[c] = np.where(t < m[c], t, m[c])
    return np.where(out, h, np.where(h > m, h, m)).astype(f32)


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def jacobi(h, epsilon=1e-4, seaLevel=SEA_OFF, maxPasses=None):
    h = np.ascontiguousarray(h, f32)
    out, eps = outlets(h, seaLevel), f32(epsilon)
    W, passes = start(h, seaLevel), 0
    while maxPasses is None or passes < maxPasses:
        nxt = step(W, h, out, eps)
        if same(nxt, W):
            break
        W, passes = nxt, passes + 1
    return W, passes


def tiled(h, epsilon=1e-4, seaLevel=SEA_OFF, tile=(64, 16), sweeps=None, record=None):
    h = np.ascontiguousarray(h, f32)
    rows, cols = h.shape
    out, eps = outlets(h, seaLevel), f32(epsilon)
    W, passes = start(h, seaLevel), 0
    tx, tz = tile
    while True:
        nxt = W.copy()
        moved = np.zeros((-(-rows // tz), -(-cols // tx)), bool)
        for z0 in range(0, rows, tz):
            for x0 in range(0, cols, tx):
                z1, x1 = min(z0 + tz, rows), min(x0 + tx, cols)
                # the tile with its ring, cut from the state of the pass before; the ring is never written
                za, xa, zb, xb = max(z0 - 1, 0), max(x0 - 1, 0), min(z1 + 1, rows), min(x1 + 1, cols)
                own = (slice(z0 - za, z1 - za), slice(x0 - xa, x1 - xa))
                frozen = np.ones((zb - za, xb - xa), bool)
                frozen[own] = out[z0:z1, x0:x1]
                w, hh = W[za:zb, xa:xb].copy(), h[za:zb, xa:xb]
                s = 0
                while sweeps is None or s < sweeps:
                    # `frozen` stands in for the outlet mask: step() returns hh there, so put the ring back
                    n = np.where(frozen, w, step(w, hh, frozen, eps))
                    if same(n, w):
                        break
                    w, s = n, s + 1
                nxt[z0:z1, x0:x1] = w[own]
                moved[z0 // tz, x0 // tx] = s > 0
        if record is not None:
            record.append(moved)
        if same(nxt, W):
            return W, passes
        W, passes = nxt, passes + 1


def flood(h, epsilon=1e-4, seaLevel=SEA_OFF):
    h = np.ascontiguousarray(h, f32)
    rows, cols = h.shape
    eps = f32(epsilon)
    fixed = outlets(h, seaLevel).reshape(-1).tolist()
    hl = h.reshape(-1).tolist()  # Python floats that hold float32 values exactly
    inf = float("inf")
    W = [hv if o else inf for hv, o in zip(hl, fixed)]
    heap = [(W[c], c) for c in range(rows * cols) if fixed[c]]
    heapq.heapify(heap)
    while heap:
        w, c = heapq.heappop(heap)
        if w > W[c]:
            continue  # a stale entry
        t = float(f32(w) + eps)  # the one rounded operation, in float32
        z, x = divmod(c, cols)
        for dx, dz in NEIGHBOURS:
            nx, nz = x + dx, z + dz
            if nx < 0 or nx >= cols or nz < 0 or nz >= rows:
                continue
            n = nz * cols + nx
            if fixed[n]:
                continue
            cand = hl[n] if hl[n] > t else t
            if cand < W[n]:
                W[n] = cand
                heapq.heappush(heap, (cand, n))
    return np.array(W, f32).reshape(rows, cols)
