"""The watershed model of nz_watershed (include/noize_hip.h) in plain numpy: basin labels and flow length over the receiver
tree of fluvial_ref.receivers, read upstream.  Planes are rows x cols arrays indexed [z, x], c = z * cols + x.

    r(c) == NONE:  basin[c] = c (int32), length[c] = +0
    otherwise, q the neighbour r(c) names:  basin[c] = basin[q], length[c] = length[q] + step_k
    step_k = cellSize for k < 4, cellSize * SQRT2 (one float32 product) for k >= 4

A receiver is strictly lower than its donor, so the graph is a forest, a cell's value is a fixed function of one other
cell's final value and every schedule of updates ends in the same bits:

    walk(h, seaLevel, cellSize) -> (basin, length, hops)    the model as a walk, cells lowest first (stable sort): a cell's
                                                            receiver has its final value already; hops = moves to the label
    jacobi(h, ...) -> (basin, length, steps)                every cell from its receiver's value of the step before, until a
                                                            step changes nothing
    tiled(h, ..., tile, sweeps) -> (basin, length, passes)  Jacobi inside the kernel's tiles: 64 x 16 tiles against frozen rings, at
                                                            most `sweeps` sweeps per tile and pass"""
import numpy as np

from fluvial_ref import NEIGHBOURS, NONE, SEA_OFF, receivers

f32 = np.float32
SQRT2 = f32(float.fromhex("0x1.6a09e6p+0"))  # 1.41421354f


def steps_of(cellSize):
    """The step of a move along code k = 0..7, and +0 at NONE."""
    cs = f32(cellSize)
    return np.array([cs] * 4 + [f32(cs * SQRT2)] * 4 + [f32(0.0)], f32)


def targets(r):
    """The flat index of the cell every cell looks at: the neighbour its code names, itself without a receiver."""
    rows, cols = r.shape
    off = np.array([dz * cols + dx for dx, dz in NEIGHBOURS] + [0], np.int64)
    return (np.arange(r.size, dtype=np.int64) + off[r.reshape(-1)]).reshape(r.shape)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def walk(h, seaLevel=SEA_OFF, cellSize=1.0):
    h = np.ascontiguousarray(h, f32)
    r = receivers(h, seaLevel)[0]
    q = targets(r).reshape(-1).tolist()
    st = steps_of(cellSize)[r.reshape(-1)]
    rl = r.reshape(-1).tolist()
    basin = np.arange(h.size, dtype=np.int32)
    length = np.zeros(h.size, f32)
    hops = np.zeros(h.size, np.int64)
    for c in np.argsort(h.reshape(-1).astype(np.float64), kind="stable").tolist():
        if rl[c] != NONE:  # the receiver is strictly lower: it has its final value already
            basin[c] = basin[q[c]]
            length[c] = f32(length[q[c]] + st[c])
            hops[c] = hops[q[c]] + 1
    return basin.reshape(h.shape), length.reshape(h.shape), hops.reshape(h.shape)


def _start(h, seaLevel, cellSize):
    h = np.ascontiguousarray(h, f32)
    r = receivers(h, seaLevel)[0]
    return (r != NONE, targets(r), steps_of(cellSize)[r],
            np.arange(h.size, dtype=np.int32).reshape(h.shape), np.zeros(h.shape, f32))


def _step(basin, length, has, q, st):
    """One Jacobi step: every cell with a receiver from the cell it looks at."""
    nb = np.where(has, basin.reshape(-1)[q], basin)
    nl = np.where(has, (length.reshape(-1)[q] + st).astype(f32), length)
    return nb.astype(np.int32), nl.astype(f32)


def jacobi(h, seaLevel=SEA_OFF, cellSize=1.0):
    has, q, st, basin, length = _start(h, seaLevel, cellSize)
    steps = 0
    while True:
        nb, nl = _step(basin, length, has, q, st)
        if same(nb, basin) and same(nl, length):
            return basin, length, steps
        basin, length, steps = nb, nl, steps + 1


def tiled(h, seaLevel=SEA_OFF, cellSize=1.0, tile=(64, 16), sweeps=None):
    has, q, st, basin, length = _start(h, seaLevel, cellSize)
    rows, cols = basin.shape
    tx, tz = tile
    passes = 0
    while True:
        nb_plane, nl_plane = basin.copy(), length.copy()
        for z0 in range(0, rows, tz):
            for x0 in range(0, cols, tx):
                own = (slice(z0, min(z0 + tz, rows)), slice(x0, min(x0 + tx, cols)))
                # the state of the pass before everywhere, of which only the own cells are updated: the ring is frozen
                b, l = basin.copy(), length.copy()
                s = 0
                while sweeps is None or s < sweeps:
                    nb, nl = _step(b, l, has, q, st)
                    if same(nb[own], b[own]) and same(nl[own], l[own]):
                        break
                    b[own], l[own] = nb[own], nl[own]
                    s += 1
                nb_plane[own], nl_plane[own] = b[own], l[own]
        if same(nb_plane, basin) and same(nl_plane, length):
            return basin, length, passes
        basin, length, passes = nb_plane, nl_plane, passes + 1
