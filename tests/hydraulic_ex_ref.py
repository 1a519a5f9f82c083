"""Reference driver of the extended grid hydraulic erosion (nz_hydraulic_erosion_ex*, HydraulicErosionStage with border /
rainMap / hardness / recordMasks): the model of tests/hydraulic_ref.py with four independent options.  With all four off
every operation is that file's, and run() returns its result and water bit for bit (tests/test_hydraulic_ex_ref.py).  Every
step is one numpy float32 operation, in the order of the comment block in include/noize_hip.h:

    d1 = d + rain                         no rain map
    d1 = d + rain * rainMap               rain map: one multiply, one add
    flux: ComputeFlowStep over the neighbours' total height t = d1 + b.  CLOSED: a neighbour beyond the border is the
          clamped read (the cell's own t, so no head).  OPEN: it stands at the cell's own bed b with no water on it, so the
          head towards the outside is (b + d1) - b; the outflow over the border is scaled by the same K as the other three
    water: UpdateWaterStep.  CLOSED: the in-term of a neighbour beyond the border is the clamped read.  OPEN: it is +0
    q, gx, gz, S, C: as in hydraulic_ref (clamped reads in both border modes)
    C > s:     e = min(kd * (C - s), max(0, b - bmin4)),  kd = dissolve, or dissolve * (1 - hardness) with a hardness map;
               b -= e;  s += e;  wear += e        (bmin4 over the clamped neighbours in both border modes)
    otherwise: e = deposit * (s - C);  b += e;  s -= e;  deposits += e
    sediment transport and evaporation: as in hydraulic_ref (0 from beyond the border; every a_X counts in `out`, so with
    an open border the sediment leaves with the water)

wear and deposits are float32 running sums in iteration order from +0: every iteration adds e to the mask of the branch the
cell took and +0 to the other.  After the last iteration the settled sediment s is added to deposits, so
result = input - wear + deposits up to rounding.  The flux and the water update are restated here in numpy (the oracle's
C functions know the closed border only; with the border closed they are checked against them bit for bit); the discharge
is the oracle's.  The kernel must match this bit for bit."""
import numpy as np

import oracle as O
from hydraulic_ref import DEFAULTS, DT, WET, _in, _nb, _smax, _smin, f32

CLOSED, OPEN = 0, 1
ZERO, ONE = f32(0.0), f32(1.0)


def _fmax0(v):
    """fmaxf(0, v): 0 unless v is larger (a NaN gives 0)."""
    return np.where(v > ZERO, v, ZERO).astype(f32)


def flow_step(b, d1, flux, border):
    """ComputeFlowStep (compute_flow of nz_flow_common.hpp) with water_0 = d1; returns the new (fN, fS, fE, fW)."""
    fN, fS, fE, fW = flux
    t = (d1 + b).astype(f32)
    tW, tE, tS, tN = (a.copy() for a in _nb(t))
    if border == OPEN:  # beyond the border: the border cell's own bed with no water on it
        tW[:, 0] = b[:, 0]
        tE[:, -1] = b[:, -1]
        tS[0, :] = b[0, :]
        tN[-1, :] = b[-1, :]
    w = _fmax0(fW + (t - tW))
    e = _fmax0(fE + (t - tE))
    s = _fmax0(fS + (t - tS))
    n = _fmax0(fN + (t - tN))
    sum_ = ((w + e) + (s + n)).astype(f32)
    pos = sum_ > ZERO
    with np.errstate(all="ignore"):  # a product that underflows to 0 divides to inf or NaN, as on the device
        K = (d1 / (sum_ * DT)).astype(f32)
    K = _fmax0(np.where(K < ONE, K, ONE).astype(f32))  # fmaxf(0, fminf(1, K)): a NaN gives 1
    w, e, s, n = (np.where(pos, f * K, ZERO).astype(f32) for f in (w, e, s, n))
    return n, s, e, w


def water_step(d1, flux, border):
    """UpdateWaterStep (update_water of nz_flow_common.hpp)."""
    fN, fS, fE, fW = flux
    nb = _in if border == OPEN else _nb
    out = (((fW + fE) + fS) + fN).astype(f32)
    inn = ((((ZERO + nb(fE)[0]) + nb(fW)[1]) + nb(fN)[2]) + nb(fS)[3]).astype(f32)
    return _fmax0(d1 + ((inn - out) * DT))


def step(b, d, s, flux, wear, deposits, rain, evaporation, capacity, dissolve, deposit, minTilt, border=CLOSED, rainMap=None,
         hardness=None):
    """One iteration: returns (b, d, s, flux, wear, deposits)."""
    rain, evaporation, capacity = f32(rain), f32(evaporation), f32(capacity)
    dissolve, deposit, minTilt = f32(dissolve), f32(deposit), f32(minTilt)
    if rainMap is None:
        d1 = (d + rain).astype(f32)
    else:
        d1 = (d + (rain * rainMap).astype(f32)).astype(f32)
    fN, fS, fE, fW = flow_step(b, d1, flux, border)
    d2 = water_step(d1, (fN, fS, fE, fW), border)
    q = O.velocity(fN, fS, fE, fW)
    bW, bE, bS, bN = _nb(b)
    gx = (bE - bW) * f32(0.5)
    gz = (bN - bS) * f32(0.5)
    g2 = gx * gx + gz * gz
    S = _smax(minTilt, np.sqrt(g2 / (ONE + g2)))
    C = (capacity * q) * S
    bmin4 = _smin(_smin(_smin(bW, bE), bS), bN)
    kd = dissolve if hardness is None else (dissolve * (ONE - hardness).astype(f32)).astype(f32)
    ero = C > s
    e_ero = _smin((kd * (C - s)).astype(f32), _smax(ZERO, b - bmin4))
    e_dep = (deposit * (s - C)).astype(f32)
    b = np.where(ero, b - e_ero, b + e_dep).astype(f32)
    s = np.where(ero, s + e_ero, s - e_dep).astype(f32)
    wear = (wear + np.where(ero, e_ero, ZERO).astype(f32)).astype(f32)
    deposits = (deposits + np.where(ero, ZERO, e_dep).astype(f32)).astype(f32)
    wet = d1 >= WET
    r = np.where(wet, DT / np.where(wet, d1, ONE), ZERO).astype(f32)
    aW, aE, aS, aN = ((s * (fX * r)).astype(f32) for fX in (fW, fE, fS, fN))
    out = ((aW + aE) + aS) + aN
    inW = _in(aE)[0]  # a_E of the west neighbour
    inE = _in(aW)[1]  # a_W of the east neighbour
    inS = _in(aN)[2]  # a_N of the south neighbour
    inN = _in(aS)[3]  # a_S of the north neighbour
    s = _smax(ZERO, (s - out) + (((inW + inE) + inS) + inN))
    d = (d2 * (ONE - evaporation)).astype(f32)
    return b, d, s, (fN, fS, fE, fW), wear, deposits


def run(height, iterations, initialWater=DEFAULTS["initialWater"], rain=DEFAULTS["rain"],
        evaporation=DEFAULTS["evaporation"], capacity=DEFAULTS["capacity"], dissolve=DEFAULTS["dissolve"],
        deposit=DEFAULTS["deposit"], minTilt=DEFAULTS["minTilt"], border=CLOSED, rainMap=None, hardness=None):
    """`iterations` iterations on one tile.  Returns (result, water, wear, deposits)."""
    b = np.ascontiguousarray(height, f32).copy()
    d = np.full(b.shape, f32(initialWater), f32)
    s = np.zeros(b.shape, f32)
    flux = tuple(np.zeros(b.shape, f32) for _ in range(4))
    wear, deposits = np.zeros(b.shape, f32), np.zeros(b.shape, f32)
    if rainMap is not None:
        rainMap = np.ascontiguousarray(rainMap, f32)
    if hardness is not None:
        hardness = np.ascontiguousarray(hardness, f32)
    if iterations == 0:
        return b, d, wear, deposits  # no iteration: the input unchanged, empty masks
    for _ in range(iterations):
        b, d, s, flux, wear, deposits = step(b, d, s, flux, wear, deposits, rain, evaporation, capacity, dissolve, deposit,
                                             minTilt, border, rainMap, hardness)
    return (b + s).astype(f32), d, wear, (deposits + s).astype(f32)
