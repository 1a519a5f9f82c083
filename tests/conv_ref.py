"""Independent numpy restatement of the separable convolution, in both float modes, for bit-for-bit tests.

The C oracle is one restatement of the reference; this is a second one, written from the operator definitions
(KernelSampleXOperator / KernelSampleZOperator, Filter/Kernel/KernelOperators.cs:18-67) and not from the oracle's code:

  * STRICT: per output cell `t = +0; for each tap: t = t + v * k; out = t * factor`.  X taps ascending, the Z pass reads
    `Kernel[k_off - k]` with k descending, i.e. tap i against row z + k_off - i.  Clamp-to-edge per pass.
  * FAST (NZ_FLOAT_FAST and NZ_FLOAT_RELAXED): the same sequence with every `t + v * k` contracted to `fmaf(v, k, t)`,
    still seeded with +0.
  * a float64 evaluation of the same operation with an a-priori error bound, which ties both fp32 sequences to the
    mathematics.

`fmaf` is the correctly rounded fp32 fused multiply-add: the product is exact in float64 (24 + 24 bits), a TwoSum with
the addend gives the exact sum as a pair, rounding that pair to odd in float64 and then to nearest fp32 is correct
rounding (53 >= 24 + 2).

Planes are (..., rows, cols) float32 arrays: leading axes are independent grids (a batch).  Even kernel sizes touch
2 * ((ksize - 1) // 2) + 1 taps, as the reference does."""
import numpy as np

f32 = np.float32
U32 = 2.0 ** -24  # unit roundoff of fp32


# ---- correctly rounded fp32 FMA --------------------------------------------------------------------------------
def _fmaf_exact(p, c64):
    """fp32(p + c) correctly rounded, p and c float64 with p exact: TwoSum, round to odd, round to fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)  # p + c == s + err exactly
        # round to odd: of the two doubles around p + c, take the one with an odd last bit
        fix = (err != 0) & np.isfinite(s) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
        return s.astype(f32)


def _fma_add(p, c):
    """fp32(p + c) correctly rounded for an exact float64 product p and an fp32 addend c."""
    c64 = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c64
        r = s.astype(f32)
        # rounding p + c to double and then to fp32 is correct unless the double sits exactly halfway between two fp32
        # values (low 29 bits 1000...0 for a normal result) or in the fp32 denormal range: those cells go the exact way
        sus = ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) | (np.abs(s) < 2.0 ** -126)
    if sus.any():
        r[sus] = _fmaf_exact(p[sus], c64[sus])
    return r


def fmaf(a, b, c):
    a, b, c = np.broadcast_arrays(*(np.atleast_1d(np.asarray(x, f32)) for x in (a, b, c)))
    shape = np.broadcast_shapes(*(np.shape(x) for x in (a, b, c)))
    return _fma_add(a.astype(np.float64) * b.astype(np.float64), c).reshape(shape)  # (the product is exact)


# ---- tap tables ------------------------------------------------------------------------------------------------
def gauss_taps(sigma, width):
    """exp(-i^2 / (2 sigma^2)) normalised, in float64, rounded to fp32 (BlurKernels.cs / KernelJob.cs:97-105)."""
    o = (width - 1) // 2
    d = np.arange(width, dtype=np.float64) - o
    w = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(f32)


def limit_width(width):  # BlurHelper.limitWidth, BlurKernels.cs:29-36
    if width % 2 == 0:
        width += 1
    return max(3, min(width, 25))


SOBEL3_2D = 11
_FIXED3 = {8: ([1, 1, 1], [1, 1, 1], 1.0 / 3.0), 9: ([-1, 0, 1], [1, 2, 1], 1.0), 10: ([1, 2, 1], [1, 0, -1], 1.0),
           12: ([1, 0, -1], [1, 1, 1], 1.0), 13: ([1, 1, 1], [-1, 0, 1], 1.0)}


def filter_taps(ft):
    """(kx, kz, factor) of KernelFilterType `ft` (KernelJob.cs:97-136); Sobel3_2D has none (it is two filters)."""
    if 0 <= ft <= 7:
        w = (9, 7, 5, 3)[ft & 3]
        k = gauss_taps(2.0 if ft >= 4 else 1.0, w)
        return k, k.copy(), f32(1.0)
    kx, kz, fac = _FIXED3[ft]
    return np.array(kx, f32), np.array(kz, f32), f32(fac)


def blur_taps(kind, width, sigma=0):
    """Taps of the blur stages' pass of kernelSize `width`: Gaussian of limitWidth(width) taps (GaussFilter) or 1/width
    (SmoothFilter), factor 1."""
    if kind == "gauss":
        k = gauss_taps(0.5 * (sigma + 1), limit_width(width))
    else:
        k = np.full(width, f32(1.0) / f32(width), f32)
    return k, k.copy(), f32(1.0)


# ---- the passes ------------------------------------------------------------------------------------------------
def _used(ksize):
    o = (ksize - 1) // 2
    return o, 2 * o + 1


def pass_x(a, k, factor, ksize=None, fast=False):
    """KernelSampleXOperator: out[z, x] = (sum over taps i ascending of a[z, clamp(x + i - o)] * k[i]) * factor."""
    a = np.asarray(a, f32)
    o, n = _used(len(k) if ksize is None else ksize)
    cols = a.shape[-1]
    base = np.arange(cols)
    t = np.zeros_like(a)
    src = a.astype(np.float64) if fast else a
    for i in range(n):
        v = src[..., np.clip(base + i - o, 0, cols - 1)]
        t = _fma_add(v * float(k[i]), t) if fast else t + v * k[i]  # fast: fmaf(v, k, t), the product exact in float64
    return t * f32(factor)


def pass_z(a, k, factor, ksize=None, fast=False, zc0=0, zc1=None):
    """KernelSampleZOperator: out[z, x] = (sum over k = o .. -o of a[clamp(z + k), x] * K[o - k]) * factor; rows clamp to
    [zc0, zc1] (a stripe's grid rows), default the whole plane."""
    a = np.asarray(a, f32)
    o, n = _used(len(k) if ksize is None else ksize)
    rows = a.shape[-2]
    zc1 = rows - 1 if zc1 is None else zc1
    base = np.arange(rows)
    t = np.zeros_like(a)
    src = a.astype(np.float64) if fast else a
    for i in range(n):
        v = src[..., np.clip(base + o - i, zc0, zc1), :]
        t = _fma_add(v * float(k[i]), t) if fast else t + v * k[i]
    return t * f32(factor)


def separable(a, kx, kz, factor, iterations=1, ksize=None, fast=False, record=()):
    """`iterations` applications of X pass then Z pass.  record: application counts whose result is returned as well,
    {count: plane} (one trajectory serves every count along it)."""
    out = {}
    for it in range(1, iterations + 1):
        a = pass_z(pass_x(a, kx, factor, ksize, fast), kz, factor, ksize, fast)
        if it in record:
            out[it] = a
    return (a, out) if record else a


def filter_apply(a, ft, iterations=1, fast=False, record=()):
    """KernelFilterStage(ft, iterations); Sobel3_2D: sqrt(h^2 + v^2) of the horizontal filter of the plane and the
    vertical filter of the same plane, per iteration (ScheduleReduce, KernelJob.cs:187-215), kernelFactor 1."""
    if ft != SOBEL3_2D:
        kx, kz, fac = filter_taps(ft)
        return separable(a, kx, kz, fac, iterations, fast=fast, record=record)
    hx, hz, _ = filter_taps(9)
    vx, vz, _ = filter_taps(10)
    out = {}
    a = np.asarray(a, f32)
    for it in range(1, iterations + 1):
        h = separable(a, hx, hz, 1.0, fast=fast)
        v = separable(a, vx, vz, 1.0, fast=fast)
        a = np.sqrt(h * h + v * v)
        if it in record:
            out[it] = a
    return (a, out) if record else a


def banded(fn, a, reach, bands):
    """fn's result on rows `bands` = [(r0, r1), ...] of a plane too large to restate whole: each band is restated on
    rows [r0 - reach, r1 + reach) cut to the plane, at full width (column clamps are real at both sides).  Rows clamp
    at the band's ends, but a wrong row spreads `reach` rows at most, so rows [r0, r1) are exact as long as `reach` is
    the operation's whole reach (T * O for T applications of an O-tap-radius kernel).  Returns [(r0, r1, rows)]."""
    rows = a.shape[-2]
    out = []
    for r0, r1 in bands:
        b0, b1 = max(0, r0 - reach), min(rows, r1 + reach)
        res = fn(a[..., b0:b1, :])
        out.append((r0, r1, res[..., r0 - b0:r1 - b0, :]))
    return out


# ---- float64 reference with an a-priori bound --------------------------------------------------------------------
def _pass64(a, k, axis, ksize=None, zc0=0, zc1=None):
    o, n = _used(len(k) if ksize is None else ksize)
    size = a.shape[axis]
    base = np.arange(size)
    hi = size - 1 if (axis == -1 or zc1 is None) else zc1
    lo = 0 if axis == -1 else zc0
    t = np.zeros(a.shape, np.float64)
    for i in range(n):
        idx = np.clip(base + (i - o if axis == -1 else o - i), lo, hi)
        t += np.take(a, idx, axis=axis) * float(k[i])
    return t


def separable64(a, kx, kz, factor, iterations=1, ksize=None):
    """The exact operation in float64, and per cell a bound on |fp32 result - float64 result| that holds for the STRICT
    and the FAST sequence alike.  Per pass, with input error B and n taps (a dot product of n terms rounded either way
    is within gamma_n * sum |k_i v_i|, and the factor adds one rounding):
        B' = |f| * (sum |k_i| B_i + (gamma_n + 2u) * sum |k_i| (|v_i| + B_i)) + n * 2^-149
    (the last term: products that underflow into the denormals lose up to half a denormal step each)."""
    a = np.asarray(a, f32).astype(np.float64)
    B = np.zeros_like(a)
    o, n = _used(len(kx) if ksize is None else ksize)
    gam = n * U32 / (1 - n * U32) + 2 * U32
    f = float(factor)
    for _ in range(iterations):
        for k, axis in ((kx, -1), (kz, -2)):
            absk = np.abs(np.asarray(k, np.float64))
            av = _pass64(np.abs(a), absk, axis, ksize)
            aB = _pass64(B, absk, axis, ksize)
            a = _pass64(a, k, axis, ksize) * f
            B = abs(f) * (aB + gam * (av + aB)) + n * 2.0 ** -149
    return a, B


# ---- comparisons -------------------------------------------------------------------------------------------------
def assert_bits_equal(got, want, what=""):
    """Bit-for-bit equality of two fp32 planes: the sign of zero counts, any NaN stands for any NaN (payloads are not
    part of the contract).  Reports the first differing cell with both bit patterns."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    assert got.dtype == f32 and want.dtype == f32, "%s: dtypes %s / %s" % (what, got.dtype, want.dtype)
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = (g != w) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        i = np.unravel_index(np.flatnonzero(bad)[0], bad.shape)
        raise AssertionError("%s: %d/%d cells differ; first at %s: got %r (0x%08x) want %r (0x%08x)" % (
            what, int(bad.sum()), bad.size, tuple(int(j) for j in i), got[i], int(g[i]), want[i], int(w[i])))


def assert_within(got, want, what="", rtol=1e-5, atol=1e-6):
    """|got - want| <= rtol |want| + atol where want is finite; non-finite cells must match (any NaN for a NaN)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    bad = np.where(fin, ~(np.abs(got - want) <= rtol * np.abs(want) + atol), ~same)
    if bad.any():
        i = np.unravel_index(np.flatnonzero(bad)[0], bad.shape)
        raise AssertionError("%s: %d/%d cells outside %g rel / %g abs; first at %s: got %r want %r" % (
            what, int(bad.sum()), bad.size, rtol, atol, tuple(int(j) for j in i), got[i], want[i]))


def signed_zero_tiles(res):
    """Planes on which every product of a tap sum is -0: -0 everywhere; the smallest negative denormal, whose
    products with taps below 0.5 underflow to -0; +0 (under all-negative taps, see NEG_TAPS)."""
    return {"neg_zero": np.full((res, res), -0.0, f32),
            "neg_denormal": np.full((res, res), -1e-45, f32),
            "zero": np.zeros((res, res), f32)}


NEG_TAPS = {3: np.array([-0.25, -0.5, -0.25], f32), 5: np.array([-0.1, -0.2, -0.4, -0.2, -0.1], f32)}
