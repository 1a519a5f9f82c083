"""The resampling model of include/noize_hip.h, restated in numpy (float32 arithmetic in the order given; numpy does not
contract).  Upsample by f in {2, 4, 8}: cell-centred samples, clamp to edge, a separable X then Z pass whose row results are
float32, tap sums seeded with +0 in ascending tap order; downsample: the mean of the f x f block, rows left to right, then
top to bottom, times 1 / f^2.  A NaN this arithmetic produces is stored as the canonical quiet NaN (sign and payload of
an arithmetic NaN differ between processors); NEAREST without base copies bits.

The stripe forms work on a buffer of rows [grow0, grow0 + rows) of a grid and clamp at the grid's border only; the monolithic
forms are the stripe forms on the whole grid."""
from fractions import Fraction

import numpy as np

f32 = np.float32
NEAREST, BILINEAR, CATMULL_ROM = 0, 1, 2
FILTERS = (NEAREST, BILINEAR, CATMULL_ROM)
FACTORS = (2, 4, 8)
HALO = {NEAREST: 0, BILINEAR: 1, CATMULL_ROM: 2}
CANONICAL_NAN = np.uint32(0x7FC00000)


def phase(f, p):
    """-> (i0 - i, t) of fine cell i f + p."""
    c = Fraction(2 * p + 1, 2 * f)
    return (-1, c + Fraction(1, 2)) if p < f // 2 else (0, c - Fraction(1, 2))


def taps_exact(f, filt, p):
    """-> (offset of the first tap from i, the weights as exact rationals)."""
    d, t = phase(f, p)
    if filt == NEAREST:
        return 0, [Fraction(1)]
    if filt == BILINEAR:
        return d, [1 - t, t]
    return d - 1, [(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2,
                   (t ** 3 - t ** 2) / 2]


def taps(f, filt, p):
    """The weights as the kernels hold them: float32, evaluated in double from t (exact: dyadic rationals)."""
    d, t = phase(f, p)
    t = float(t)
    if filt == NEAREST:
        return 0, [f32(1)]
    if filt == BILINEAR:
        return d, [f32(1.0 - t), f32(t)]
    return d - 1, [f32((-t * t * t + 2 * t * t - t) / 2), f32((3 * t * t * t - 5 * t * t + 2) / 2),
                   f32((-3 * t * t * t + 4 * t * t + t) / 2), f32((t * t * t - t * t) / 2)]


def _canon(a):
    a = np.ascontiguousarray(a, f32)
    a.view(np.uint32)[np.isnan(a)] = CANONICAL_NAN
    return a


def _expand(a, f, filt, cells, lo, hi, off):
    """One pass along axis 0: fine cells of the coarse cells `cells` (global indices) from rows of `a`, where global coarse
    index i is row i - off of `a` and indices clamp to [lo, hi].  -> (len(cells) * f, ...) float32."""
    cells = np.asarray(cells, np.int64)
    out = np.empty((len(cells) * f,) + a.shape[1:], f32)
    for p in range(f):
        first, w = taps(f, filt, p)
        if filt == NEAREST:
            out[p::f] = a[np.clip(cells, lo, hi) - off]
            continue
        s = np.zeros((len(cells),) + a.shape[1:], f32)  # +0
        for k, wk in enumerate(w):
            idx = np.clip(cells + first + k, lo, hi) - off
            if idx.size and (idx.min() < 0 or idx.max() >= a.shape[0]):
                raise ValueError("row %d of the grid is not in the buffer" % (idx.min() + off if idx.min() < 0 else idx.max() + off))
            s = s + a[idx] * wk
        out[p::f] = s
    return out


def upsample_stripe(buf, grow0, grows, g0, g1, f, filt, base=None):
    """Fine global rows [g0, g1) of the grid whose coarse rows [grow0, grow0 + len(buf)) are `buf` (rows x cols).  base: the
    same rows of the fine base plane.  -> (g1 - g0, cols * f) float32."""
    buf = np.ascontiguousarray(buf, f32)
    with np.errstate(all="ignore"):
        cols = buf.shape[1]
        x = _expand(buf.T, f, filt, np.arange(cols), 0, cols - 1, 0).T  # every row of the buffer, X pass
        if g1 <= g0:
            return np.empty((0, cols * f), f32)
        c0, c1 = g0 // f, (g1 - 1) // f
        if filt == NEAREST:
            idx = np.arange(c0, c1 + 1) - grow0
            if idx.min() < 0 or idx.max() >= buf.shape[0]:
                raise ValueError("a coarse row is not in the buffer")
        z = _expand(x, f, filt, np.arange(c0, c1 + 1), 0, grows - 1, grow0)
        out = z[g0 - c0 * f:g1 - c0 * f]
        if base is not None:
            out = np.asarray(base, f32) + out
        if base is not None or filt != NEAREST:
            out = _canon(out)
    return np.ascontiguousarray(out, f32)


def upsample(src, f, filt, base=None):
    src = np.ascontiguousarray(src, f32)
    return upsample_stripe(src, 0, src.shape[0], 0, src.shape[0] * f, f, filt, base)


def downsample_stripe(buf, grow0, g0, g1, f):
    """Coarse global rows [g0, g1) from the fine buffer rows [grow0, grow0 + len(buf))."""
    buf = np.ascontiguousarray(buf, f32)
    r0, r1 = f * g0 - grow0, f * g1 - grow0
    if g1 > g0 and (r0 < 0 or r1 > buf.shape[0]):
        raise ValueError("a fine row is not in the buffer")
    assert buf.shape[1] % f == 0
    with np.errstate(all="ignore"):
        v = buf[r0:r1].reshape(g1 - g0, f, buf.shape[1] // f, f)
        r = v[..., 0]
        for k in range(1, f):
            r = r + v[..., k]
        m = r[:, 0]
        for k in range(1, f):
            m = m + r[:, k]
        m = m * f32(1.0 / (f * f))
    return _canon(m)


def downsample(src, f):
    src = np.ascontiguousarray(src, f32)
    assert src.shape[0] % f == 0
    return downsample_stripe(src, 0, 0, src.shape[0] // f, f)
