"""The drainage-area model of nz_drainage_area (include/noize_hip.h) in plain numpy, float32 throughout: the accumulation
over the receiver tree of fluvial_ref.receivers.  A receiver is strictly lower than its donor, so the tree has no cycle and
every schedule of updates ends in the same floats:

    accumulate(h, ...) -> (A, height)  the model as a topological walk: cells highest first (stable sort), each cell
                                       gathering its donors for k ascending; height = cells of the longest flow path
    jacobi(h, ...) -> (A, steps)       fluvial_ref.drainage from rain_c until a step changes nothing
    tiled(h, ..., sweeps) -> (A, passes)  Jacobi inside the kernel's tiles: 64 x 16 tiles swept against frozen rings, at most `sweeps`
                                       sweeps per tile and pass
    serpentine(res) -> h               one channel of res^2 / 2 cells between walls: the long chain"""
import numpy as np

from fluvial_ref import NEIGHBOURS, NONE, OPPOSITE, SEA_OFF, drainage, rain_plane, receivers

f32 = np.float32


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def accumulate(h, rain=1.0, seaLevel=SEA_OFF, rainMap=None):
    h = np.ascontiguousarray(h, f32)
    rows, cols = h.shape
    r = receivers(h, seaLevel)[0].reshape(-1).tolist()
    rc = rain_plane(h.shape, rain, rainMap).reshape(-1)
    A = rc.copy()
    height = [1] * h.size
    for c in np.argsort(-h.reshape(-1).astype(np.float64), kind="stable").tolist():
        z, x = divmod(c, cols)
        a, d = rc[c], 0
        for k, (dx, dz) in enumerate(NEIGHBOURS):
            qx, qz = x + dx, z + dz
            if 0 <= qx < cols and 0 <= qz < rows:
                q = qz * cols + qx
                if r[q] == OPPOSITE[k]:  # a donor is strictly higher: it has its final value already
                    a = f32(a + A[q])
                    d = max(d, height[q])
        A[c] = a
        height[c] = d + 1
    return A.reshape(h.shape), max(height)


def jacobi(h, rain=1.0, seaLevel=SEA_OFF, rainMap=None):
    h = np.ascontiguousarray(h, f32)
    r = receivers(h, seaLevel)[0]
    rc = rain_plane(h.shape, rain, rainMap)
    A, steps = rc.copy(), 0
    while True:
        nxt = drainage(A, r, rc)
        if same(nxt, A):
            return A, steps
        A, steps = nxt, steps + 1


def tiled(h, rain=1.0, seaLevel=SEA_OFF, rainMap=None, tile=(64, 16), sweeps=None):
    h = np.ascontiguousarray(h, f32)
    rows, cols = h.shape
    r = receivers(h, seaLevel)[0]
    rc = rain_plane(h.shape, rain, rainMap)
    A, passes = rc.copy(), 0
    tx, tz = tile
    while True:
        nxt = A.copy()
        for z0 in range(0, rows, tz):
            for x0 in range(0, cols, tx):
                z1, x1 = min(z0 + tz, rows), min(x0 + tx, cols)
                # the tile with its ring, cut from the state of the pass before; the ring is never written.  The cut's
                # receivers are the whole plane's: a ring cell may drain somewhere else, and then nothing gathers it
                za, xa, zb, xb = max(z0 - 1, 0), max(x0 - 1, 0), min(z1 + 1, rows), min(x1 + 1, cols)
                own = (slice(z0 - za, z1 - za), slice(x0 - xa, x1 - xa))
                a, rr, cc = A[za:zb, xa:xb].copy(), r[za:zb, xa:xb], rc[za:zb, xa:xb]
                s = 0
                while sweeps is None or s < sweeps:
                    n = a.copy()
                    n[own] = drainage(a, rr, cc)[own]
                    if same(n, a):
                        break
                    a, s = n, s + 1
                nxt[z0:z1, x0:x1] = a[own]
        if same(nxt, A):
            return A, passes
        A, passes = nxt, passes + 1


def serpentine(res=160):
    """Walls of 1e4 and one channel that descends 0.25 per cell along the rows 1, 3, 5, ... -- two apart, joined in turn at
    the right and the left end through the wall row between them -- to a single low border cell.  Every height is a
    multiple of 0.25 below 2^12, exact in float32."""
    h = np.full((res, res), f32(1e4), f32)
    path = []
    zs = list(range(1, res - 1, 2))
    for i, z in enumerate(zs):
        xs = range(1, res - 1) if i % 2 == 0 else range(res - 2, 0, -1)
        path += [(z, x) for x in xs]
        if z != zs[-1]:
            path.append((z + 1, path[-1][1]))  # through the wall row, below the end of this row
    z, x = path[-1]
    path.append((z, 0 if x == 1 else res - 1))  # the outlet
    for i, (z, x) in enumerate(path):
        h[z, x] = f32(0.25) * f32(len(path) - 1 - i)
    return h
