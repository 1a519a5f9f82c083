"""Stream-power fluvial erosion with drainage area in plain numpy: the model of nz_fluvial_erosion (include/noize_hip.h)
operation for operation, float32 throughout, one function per step.  Planes are res x res arrays indexed [z, x] (any
rows x cols grid works: a band of rows of a larger tile is a grid of its own).

    r, S, drop = receivers(h, seaLevel)            step 1   r: 0..7 (W E S N SW SE NW NE), NONE without a receiver
    A1 = drainage(A, r, rain_c)                    step 2   one Jacobi step of the accumulation, a gather in k order
    h1 = erode(h, A1, S, drop, outlets(h, sea), ...)  step 3
    run(h, iterations, ...) -> (heights, drainage)

exact_accumulation(h, ...) is the float64 accumulation over the receiver tree in height order, the fixed point of step 2."""
import numpy as np

f32 = np.float32
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))  # (dx, dz) of k = 0..7
OPPOSITE = (1, 0, 3, 2, 7, 6, 5, 4)
NONE = 8
DIAG = f32(float.fromhex("0x1.6a09e6p-1"))  # 0.70710678f, bits 0x3F3504F3
SEA_OFF = -np.finfo(f32).max
DEFAULTS = dict(erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=float(SEA_OFF))


def _window(shape, dx, dz):
    """Slices (cells, their neighbour at (dx, dz)) over the cells whose neighbour exists."""
    x0, x1 = max(0, -dx), shape[1] - max(0, dx)
    z0, z1 = max(0, -dz), shape[0] - max(0, dz)
    return (slice(z0, z1), slice(x0, x1)), (slice(z0 + dz, z1 + dz), slice(x0 + dx, x1 + dx))


def outlets(h, seaLevel=SEA_OFF):
    o = h <= f32(seaLevel)
    o[0, :] = o[-1, :] = True
    o[:, 0] = o[:, -1] = True
    return o


def receivers(h, seaLevel=SEA_OFF):
    h = np.asarray(h, f32)
    best = np.zeros(h.shape, f32)
    drop = np.zeros(h.shape, f32)
    r = np.full(h.shape, NONE, np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (dx, dz) in enumerate(NEIGHBOURS):
            c, n = _window(h.shape, dx, dz)
            d = h[c] - h[n]
            s = d if k < 4 else d * DIAG
            take = s > best[c]
            best[c] = np.where(take, s, best[c])
            drop[c] = np.where(take, d, drop[c])
            r[c] = np.where(take, np.uint8(k), r[c])
    o = outlets(h, seaLevel)
    r[o] = NONE
    best[o] = f32(0.0)
    drop[o] = f32(0.0)
    return r, best, drop


def rain_plane(shape, rain, rainMap=None):
    if rainMap is None:
        return np.full(shape, f32(rain), f32)
    return (f32(rain) * np.asarray(rainMap, f32)).astype(f32)


def drainage(A, r, rain_c):
    out = np.array(rain_c, f32)
    for k, (dx, dz) in enumerate(NEIGHBOURS):
        c, n = _window(A.shape, dx, dz)
        out[c] = np.where(r[n] == OPPOSITE[k], out[c] + A[n], out[c])
    return out


def erode(h, A1, S, drop, outlet, erodibility, uplift, dt, hardness=None, upliftMap=None):
    kc = f32(erodibility) if hardness is None else f32(erodibility) * (f32(1.0) - np.asarray(hardness, f32))
    du = f32(dt) * f32(uplift)
    if upliftMap is not None:
        du = du * np.asarray(upliftMap, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        e = ((kc * np.sqrt(A1)) * S) * f32(dt)
        lim = drop * f32(0.5)
        e = np.where(lim < e, lim, e)
        out = (h - e) + du
    return np.where(outlet, h, out).astype(f32)


def run(h, iterations, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=SEA_OFF, rainMap=None, hardness=None,
        upliftMap=None, drainageIn=None):
    h = np.array(h, f32)
    rc = rain_plane(h.shape, rain, rainMap)
    A = np.array(drainageIn, f32) if drainageIn is not None else rc.copy()
    for _ in range(iterations):
        r, S, drop = receivers(h, seaLevel)
        A = drainage(A, r, rc)
        h = erode(h, A, S, drop, outlets(h, seaLevel), erodibility, uplift, dt, hardness, upliftMap)
    return h, A


def pits(h, seaLevel=SEA_OFF):
    """Count of cells that are no outlet and have no receiver."""
    r, _, _ = receivers(h, seaLevel)
    return int(((r == NONE) & ~outlets(h, seaLevel)).sum())


def exact_accumulation(h, rain=1.0, seaLevel=SEA_OFF):
    """The accumulation over the receiver tree, highest cell first, in float64."""
    r, _, _ = receivers(h, seaLevel)
    res = h.shape[1]
    A = np.full(h.size, float(f32(rain)), np.float64)
    rf = r.reshape(-1)
    for c in np.argsort(-np.asarray(h, np.float64).reshape(-1), kind="stable"):
        k = rf[c]
        if k != NONE:
            dx, dz = NEIGHBOURS[k]
            A[c + dz * res + dx] += A[c]
    return A.reshape(h.shape)
