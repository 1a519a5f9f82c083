"""The multiple-flow drainage model of nz_drainage_mfd (include/noize_hip.h) in plain numpy, float32 throughout, every
operation rounded once.  Outlets, the neighbour order W E S N SW SE NW NE, "a neighbour outside the tile does not exist" and
DIAG are fluvial_ref's.  Per cell c that is no outlet, with `best` the S of its receiver rule:

    for k ascending over the existing neighbours: d = h[c] - h[k]; s_k = d (k < 4) or d * DIAG; k takes flow iff s_k > 0
    q_k = s_k / best; g_k = q_k, then exponent - 1 times g_k = g_k * q_k
    T = +0; for k ascending with g_k > 0: T = T + g_k;  w_k = g_k / T for g_k > 0, else the edge carries nothing

and the plane: A[c] = rain_c; for k ascending over the existing neighbours whose weight towards c is w > 0:
A[c] = A[c] + (w * A[k]).  Flow goes strictly downhill, so the graph has no cycle and every schedule ends in the same floats:

    weights(h, sea, exponent) -> W[8]       W[k][c]: the weight cell c sends to its neighbour k (+0: nothing)
    incoming(W) -> I[8]                     I[k][c]: the weight neighbour k of c sends to c
    step(A, I, rain_c)                      one Jacobi step of the gather
    walk(h, ...) -> (A, height)             cells highest first, height = cells of the longest path of the DAG
    jacobi(h, ...) -> (A, steps)            step from rain_c until nothing changes
    tiled(h, ..., sweeps) -> (A, passes)    Jacobi inside the kernel's tiles: 64 x 16 tiles swept against frozen rings
    walk64(h, ...) -> A                     the same text in float64: what float32 rounds"""
import numpy as np

from fluvial_ref import DIAG, NEIGHBOURS, OPPOSITE, SEA_OFF, _window, outlets, rain_plane

f32 = np.float32


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _weights(h, seaLevel, exponent, ft, diag):
    """The model's text at precision ft (the slopes s and `best` are formed at ft from the float32 heights)."""
    h = np.asarray(h, f32).astype(ft)
    best = np.zeros(h.shape, ft)
    s = np.zeros((8,) + h.shape, ft)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for k, (dx, dz) in enumerate(NEIGHBOURS):
            c, n = _window(h.shape, dx, dz)
            d = h[c] - h[n]
            s[k][c] = d if k < 4 else d * diag
            best[c] = np.where(s[k][c] > best[c], s[k][c], best[c])
        g = np.zeros_like(s)
        for k in range(8):
            q = s[k] / best
            p = q
            for _ in range(exponent - 1):
                p = p * q
            g[k] = np.where(s[k] > 0, p, ft(0))
        g[:, outlets(np.asarray(h, f32), seaLevel)] = ft(0)
        T = np.zeros(h.shape, ft)
        for k in range(8):
            T = np.where(g[k] > 0, T + g[k], T)
        W = np.zeros_like(g)
        for k in range(8):
            W[k] = np.where(g[k] > 0, g[k] / T, ft(0))
    return W


def weights(h, seaLevel=SEA_OFF, exponent=1):
    assert 1 <= exponent <= 16
    return _weights(h, seaLevel, exponent, f32, DIAG)


def incoming(W):
    I = np.zeros_like(W)
    for k, (dx, dz) in enumerate(NEIGHBOURS):
        c, n = _window(W.shape[1:], dx, dz)
        I[k][c] = W[OPPOSITE[k]][n]
    return I


def step(A, I, rain_c):
    out = np.array(rain_c, A.dtype)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k, (dx, dz) in enumerate(NEIGHBOURS):
            c, n = _window(A.shape, dx, dz)
            out[c] = np.where(I[k][c] > 0, out[c] + I[k][c] * A[n], out[c])
    return out


def _walk(h, I, rc):
    rows, cols = h.shape
    A = rc.reshape(-1).copy()
    rcl = rc.reshape(-1)
    live = (I > 0).reshape(8, -1)
    Il = I.reshape(8, -1)
    height = [1] * h.size
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for c in np.argsort(-h.reshape(-1).astype(np.float64), kind="stable").tolist():
            if not live[:, c].any():
                continue
            a, d = rcl[c], 0
            for k, (dx, dz) in enumerate(NEIGHBOURS):
                if live[k, c]:  # the neighbour exists and is strictly higher: it has its final value already
                    q = c + dz * cols + dx
                    a = a + Il[k, c] * A[q]
                    d = max(d, height[q])
            A[c] = a
            height[c] = d + 1
    return A.reshape(h.shape), max(height)


def walk(h, rain=1.0, seaLevel=SEA_OFF, rainMap=None, exponent=1):
    h = np.ascontiguousarray(h, f32)
    return _walk(h, incoming(weights(h, seaLevel, exponent)), rain_plane(h.shape, rain, rainMap))


def walk64(h, rain=1.0, seaLevel=SEA_OFF, rainMap=None, exponent=1):
    """The float64 restatement: the same weights and gather at double precision (rain_c stays the float32 product).
    NaN heights take the end of the order and send and receive nothing, as in float32."""
    h = np.ascontiguousarray(h, f32)
    W = _weights(h, seaLevel, exponent, np.float64, float(np.sqrt(0.5)))
    return _walk(h, incoming(W), rain_plane(h.shape, rain, rainMap).astype(np.float64))[0]


def jacobi(h, rain=1.0, seaLevel=SEA_OFF, rainMap=None, exponent=1):
    h = np.ascontiguousarray(h, f32)
    I = incoming(weights(h, seaLevel, exponent))
    rc = rain_plane(h.shape, rain, rainMap)
    A, steps = rc.copy(), 0
    while True:
        nxt = step(A, I, rc)
        if same(nxt, A):
            return A, steps
        A, steps = nxt, steps + 1


def tiled(h, rain=1.0, seaLevel=SEA_OFF, rainMap=None, exponent=1, tile=(64, 16), sweeps=None):
    h = np.ascontiguousarray(h, f32)
    rows, cols = h.shape
    I = incoming(weights(h, seaLevel, exponent))
    rc = rain_plane(h.shape, rain, rainMap)
    A, passes = rc.copy(), 0
    tx, tz = tile
    while True:
        nxt = A.copy()
        for z0 in range(0, rows, tz):
            for x0 in range(0, cols, tx):
                z1, x1 = min(z0 + tz, rows), min(x0 + tx, cols)
                # the tile with its ring, cut from the state of the pass before; the ring is never written.  The cut's
                # weights are the whole plane's
                za, xa, zb, xb = max(z0 - 1, 0), max(x0 - 1, 0), min(z1 + 1, rows), min(x1 + 1, cols)
                own = (slice(z0 - za, z1 - za), slice(x0 - xa, x1 - xa))
                a, ii, cc = A[za:zb, xa:xb].copy(), I[:, za:zb, xa:xb], rc[za:zb, xa:xb]
                s = 0
                while sweeps is None or s < sweeps:
                    n = a.copy()
                    n[own] = step(a, ii, cc)[own]
                    if same(n, a):
                        break
                    a, s = n, s + 1
                nxt[z0:z1, x0:x1] = a[own]
        if same(nxt, A):
            return A, passes
        A, passes = nxt, passes + 1
