"""The implicit stream-power step of nz_fluvial_implicit (include/noize_hip.h) in plain numpy, float32 throughout, every
operation rounded once: the receiver tree of fluvial_ref.receivers, solved upstream.  Planes are rows x cols arrays indexed
[z, x], c = z * cols + x.

    du = dt * uplift (* upliftMap[c]),  kc = erodibility (* (1 - hardness[c]))
    outlet:  h'[c] = h[c]              pit:  h'[c] = h[c] + du
    otherwise, q the neighbour r(c) = k names:
        b = h[c] + du,  f = ((kc * sqrt(A[c])) * invL_k) * dt,  invL_k = 1 (k < 4) or DIAG (k >= 4)
        h'[c] = (b + f * h'[q]) / (1 + f)

A receiver is strictly lower than its donor and the roots of the forest -- outlets and pits -- are fixed, so a cell's new
height is a fixed function of one other cell's new height and every schedule of updates ends in the same bits, from any
start state:

    coefficients(h, A, ...) -> (has, q, b, f)      what the kernels' setup launch stores: b is the final value where has is
                                                   False, f is +0 there
    walk(h, A, ...) -> h'                          the model as a walk, cells lowest first (stable sort)
    jacobi(h, A, ..., start) -> (h', steps)        every cell from its receiver's value of the step before, until a step
                                                   changes no bit; start "b" (the kernels') or "h" (the nothing of all or nothing)
    tiled(h, A, ..., tile, sweeps) -> (h', passes) Jacobi inside the kernel's tiles: 64 x 16 tiles swept against frozen rings
    step(hn, has, q, b, f) -> h'                   one Jacobi step, for fixed-point checks of a result
    chain(h, iterations, ...) -> (h', A)           the hosts' ImplicitFluvialStage: drainage_ref.accumulate, then walk, per
                                                   iteration"""
import numpy as np

from drainage_ref import accumulate
from fluvial_ref import DIAG, NONE, SEA_OFF, outlets, receivers
from watershed_ref import targets

f32 = np.float32
ONE = f32(1.0)
DEFAULTS = dict(iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=float(SEA_OFF))


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def coefficients(h, A, erodibility=0.05, uplift=0.002, dt=1.0, seaLevel=SEA_OFF, hardness=None, upliftMap=None):
    h = np.ascontiguousarray(h, f32)
    A = np.ascontiguousarray(A, f32)
    r = receivers(h, seaLevel)[0]
    has = r != NONE
    du = f32(dt) * f32(uplift)
    if upliftMap is not None:
        du = du * np.asarray(upliftMap, f32)
    kc = f32(erodibility) if hardness is None else f32(erodibility) * (ONE - np.asarray(hardness, f32))
    inv_l = np.where(r < 4, ONE, DIAG).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        b = np.where(outlets(h, seaLevel), h, h + du).astype(f32)
        f = np.where(has, ((kc * np.sqrt(A)) * inv_l) * f32(dt), f32(0.0)).astype(f32)
    return has, targets(r), b, f


def step(hn, has, q, b, f):
    """One Jacobi step: every cell with a receiver from the cell it looks at."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(has, (b + f * hn.reshape(-1)[q]) / (ONE + f), hn).astype(f32)


def walk(h, A, **kw):
    h = np.ascontiguousarray(h, f32)
    has, q, b, f = coefficients(h, A, **kw)
    hn = b.reshape(-1).copy()
    hl, ql, bf, ff = has.reshape(-1).tolist(), q.reshape(-1).tolist(), b.reshape(-1), f.reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in np.argsort(h.reshape(-1).astype(np.float64), kind="stable").tolist():
            if hl[c]:  # the receiver is strictly lower: it has its final value already
                hn[c] = f32(f32(bf[c] + f32(ff[c] * hn[ql[c]])) / f32(ONE + ff[c]))
    return hn.reshape(h.shape)


def _start(h, b, start):
    return {"b": b, "h": np.ascontiguousarray(h, f32)}[start].copy()


def jacobi(h, A, start="b", **kw):
    has, q, b, f = coefficients(h, A, **kw)
    hn, steps = _start(h, b, start), 0
    if start == "h":  # the roots take their final value in the first step
        hn = np.where(has, hn, b)
    while True:
        nxt = step(hn, has, q, b, f)
        if same(nxt, hn):
            return hn, steps
        hn, steps = nxt, steps + 1


def tiled(h, A, tile=(64, 16), sweeps=None, **kw):
    has, q, b, f = coefficients(h, A, **kw)
    hn, passes = b.copy(), 0
    rows, cols = hn.shape
    tx, tz = tile
    while True:
        nxt = hn.copy()
        for z0 in range(0, rows, tz):
            for x0 in range(0, cols, tx):
                own = (slice(z0, min(z0 + tz, rows)), slice(x0, min(x0 + tx, cols)))
                # the state of the pass before everywhere, of which only the own cells are updated: the ring is frozen
                t, s = hn.copy(), 0
                while sweeps is None or s < sweeps:
                    n = step(t, has, q, b, f)
                    if same(n[own], t[own]):
                        break
                    t[own] = n[own]
                    s += 1
                nxt[own] = t[own]
        if same(nxt, hn):
            return hn, passes
        hn, passes = nxt, passes + 1


def chain(h, iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=SEA_OFF, rainMap=None, hardness=None,
          upliftMap=None):
    h = np.array(h, f32)
    A = None
    for _ in range(iterations):
        A = accumulate(h, rain, seaLevel, rainMap)[0]
        h = walk(h, A, erodibility=erodibility, uplift=uplift, dt=dt, seaLevel=seaLevel, hardness=hardness, upliftMap=upliftMap)
    return h, A
