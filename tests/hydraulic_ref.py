"""Reference driver of grid hydraulic erosion (nz_hydraulic_erosion_stage*, HydraulicErosionStage).  Cell state: height b,
water d, suspended sediment s and the four outflows fN fS fE fW of the flow map (N is +z, E is +x).  Start: d = initialWater,
s = 0, flux 0.  DT = 0.2 (the flow map's TIMESTEP).  Every iteration, every step one numpy float32 operation in this order
("clamped": a clamp-to-edge read, as in the flow map):

    d1 = d + rain
    (fN, fS, fE, fW) = oracle.flow_step(b, d1, fN, fS, fE, fW)            the pipe model's new flux
    d2 = oracle.water_step(d1, fN, fS, fE, fW)                              its water update (clamped in-terms)
    q  = oracle.velocity(fN, fS, fE, fW)                                   discharge, not normalised
    gx = (b[x+1] - b[x-1]) * 0.5          gz = (b[z+1] - b[z-1]) * 0.5     clamped, b before this iteration's erosion
    g2 = gx*gx + gz*gz                    S  = max(minTilt, sqrt(g2 / (1 + g2)))
    C  = (capacity * q) * S
    C > s:     e = min(dissolve * (C - s), max(0, b - bmin4));  b = b - e;  s = s + e
    otherwise: e = deposit * (s - C);                           b = b + e;  s = s - e
    r  = d1 >= 2^-126 ? DT / d1 : 0       a_X = s * (fX * r)                for X in W, E, S, N
    out = ((a_W + a_E) + a_S) + a_N
    in  = ((a_E[x-1] + a_W[x+1]) + a_N[z-1]) + a_S[z+1]                    0 where the neighbour is outside the tile
    s  = max(0, (s - out) + in)
    d  = d2 * (1 - evaporation)

r's guard is the smallest normal float, not 0: below it DT / d1 overflows, 0 * inf is NaN and the cell's sediment would
vanish (water drains to subnormal depths when rain is 0).  bmin4 = min(min(min(b[x-1], b[x+1]), b[z-1]), b[z+1]) over the
clamped neighbours.  min(a, c) is the select `c < a ? c : a`
and max(lo, v) is `v > lo ? v : lo`: a tie keeps the first operand, so max(0, -0) is +0 and the sign of a zero never depends
on the hardware's min / max.  After the last iteration the sediment settles: the result is b + s, and the water plane is d.
The kernel must match this bit for bit."""
import numpy as np

import oracle as O

f32 = np.float32
DT = f32(0.2)
WET = f32(2.0 ** -126)  # the shallowest water that carries sediment: DT / WET is finite
# the stage's defaults (include/noize_hip.h): finite over thousands of iterations on a quickstart tile
DEFAULTS = dict(initialWater=1e-4, rain=1e-4, evaporation=0.01, capacity=1.0, dissolve=0.3, deposit=0.3, minTilt=0.01)


def _smax(lo, v):
    return np.where(v > lo, v, lo).astype(f32)


def _smin(a, c):
    return np.where(c < a, c, a).astype(f32)


def _nb(a):
    """The four clamped neighbours (W, E, S, N) of every cell."""
    p = np.pad(a, 1, mode="edge")
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def _in(a):
    """The four unclamped neighbours (W, E, S, N), 0 outside the tile."""
    p = np.pad(a, 1, mode="constant")
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def step(b, d, s, flux, rain, evaporation, capacity, dissolve, deposit, minTilt):
    """One iteration: returns (b, d, s, flux)."""
    rain, evaporation, capacity = f32(rain), f32(evaporation), f32(capacity)
    dissolve, deposit, minTilt = f32(dissolve), f32(deposit), f32(minTilt)
    d1 = (d + rain).astype(f32)
    fN, fS, fE, fW = O.flow_step(b, d1, *flux)
    d2 = O.water_step(d1, fN, fS, fE, fW)
    q = O.velocity(fN, fS, fE, fW)
    bW, bE, bS, bN = _nb(b)
    gx = (bE - bW) * f32(0.5)
    gz = (bN - bS) * f32(0.5)
    g2 = gx * gx + gz * gz
    S = _smax(minTilt, np.sqrt(g2 / (f32(1.0) + g2)))
    C = (capacity * q) * S
    bmin4 = _smin(_smin(_smin(bW, bE), bS), bN)
    ero = C > s
    e_ero = _smin(dissolve * (C - s), _smax(f32(0.0), b - bmin4))
    e_dep = deposit * (s - C)
    b = np.where(ero, b - e_ero, b + e_dep).astype(f32)
    s = np.where(ero, s + e_ero, s - e_dep).astype(f32)
    wet = d1 >= WET
    r = np.where(wet, DT / np.where(wet, d1, f32(1.0)), f32(0.0)).astype(f32)
    aW, aE, aS, aN = (s * (fX * r) for fX in (fW, fE, fS, fN))
    out = ((aW + aE) + aS) + aN
    inW = _in(aE)[0]  # a_E of the west neighbour
    inE = _in(aW)[1]  # a_W of the east neighbour
    inS = _in(aN)[2]  # a_N of the south neighbour
    inN = _in(aS)[3]  # a_S of the north neighbour
    s = _smax(f32(0.0), (s - out) + (((inW + inE) + inS) + inN))
    d = (d2 * (f32(1.0) - evaporation)).astype(f32)
    return b, d, s, (fN, fS, fE, fW)


def run(height, iterations, initialWater=DEFAULTS["initialWater"], rain=DEFAULTS["rain"],
        evaporation=DEFAULTS["evaporation"], capacity=DEFAULTS["capacity"], dissolve=DEFAULTS["dissolve"],
        deposit=DEFAULTS["deposit"], minTilt=DEFAULTS["minTilt"], state=False):
    """`iterations` iterations on one tile.  Returns (result, water), or (b, d, s, flux) with state=True."""
    b = np.ascontiguousarray(height, f32).copy()
    d = np.full(b.shape, f32(initialWater), f32)
    s = np.zeros(b.shape, f32)
    flux = tuple(np.zeros(b.shape, f32) for _ in range(4))
    if iterations == 0 and not state:
        return b, d  # no iteration: the input unchanged
    for _ in range(iterations):
        b, d, s, flux = step(b, d, s, flux, rain, evaporation, capacity, dissolve, deposit, minTilt)
    if state:
        return b, d, s, flux
    return (b + s).astype(f32), d
