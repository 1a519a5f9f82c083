"""The FMA fold of the power-of-two octave ladder (snoise2_tab_ladder in noize_job_amd/csrc/nz_fractal.hip), in exact rational
arithmetic: the ladder forms the unskew's first difference as fmaf(f, x, -i) = RN32(f x - i) where the reference forms
RN32(RN32(f x) - i).  With f a power of two the product is exact and the two agree bit for bit; with any other f they do not
always, which is why the table, recurrence and guarded loops keep the separate subtraction.

    f   2^k, k = -3 .. 12 (descending and ascending ladders)
    x   float32: the metric's coordinates (j + pos) / 1700, magnitudes 2^-20 .. 2^8 of both signs, exact zeros of both signs,
        values one ulp on either side of an integer
    i   the floor of the sample's skewed coordinate, formed as the kernel forms it (integer-valued)

RN32 is round-to-nearest-even onto float32 (subnormals included), written out on fractions.Fraction; a numpy float32
evaluation of the reference's two operations is held against it, so that the model is the arithmetic the oracle runs."""
from fractions import Fraction

import numpy as np

f32 = np.float32
CY = f32(0.366025403784439)
LADDER = [2.0 ** k for k in range(-3, 13)]


def rn32(q):
    """The float32 nearest to the rational q, ties to even, as a Fraction.  |q| < 2^128."""
    if q == 0:
        return Fraction(0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and e < 128
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n, r = divmod(a, ulp)
    if r * 2 > ulp or (r * 2 == ulp and n % 2 == 1):
        n += 1
    return n * ulp if q > 0 else -(n * ulp)


def samples():
    """(x, z) pairs of float32 coordinates; every x sample also serves as a z."""
    rng = np.random.default_rng(13)
    cols = np.concatenate([np.arange(0, 4096, 41), [1, 2, 1699, 1700, 1701, 4095]]).astype(f32)
    metric = [(cols + f32(pos)) / f32(1700) for pos in (0, -4096, 3400, 100000)]
    mag = np.exp2(rng.uniform(-20, 8, 160)).astype(f32) * rng.choice([f32(-1), f32(1)], 160)
    ints = np.array([-300, -289, -2, -1, 1, 2, 3, 17, 255, 256], dtype=f32)
    near = np.concatenate([np.nextafter(ints, f32(np.inf)), np.nextafter(ints, f32(-np.inf))])
    zeros = np.array([0.0, -0.0], dtype=f32)
    x = np.concatenate(metric + [mag, near, zeros, ints]).astype(f32)
    z = rng.permutation(x)
    assert x.dtype == f32 and z.dtype == f32
    return x, z


def skew_floors(f, x, z):
    """The reference's octave opening in float32: v = f (x, z), s = vx Cy + vz Cy, floors of v + s."""
    vx, vz = f32(f) * x, f32(f) * z
    s = vx * CY + vz * CY
    fx, fz = np.floor(vx + s), np.floor(vz + s)
    assert all(a.dtype == f32 for a in (vx, vz, s, fx, fz))
    return vx, vz, fx, fz


def split_and_fused(f, c, i):
    """RN32(RN32(f c) - i) and RN32(f c - i) for one float32 c and one integer-valued float32 i."""
    F, Cq, I = Fraction(float(f)), Fraction(float(c)), Fraction(float(i))
    return rn32(rn32(F * Cq) - I), rn32(F * Cq - I)


def test_rn32_is_float32_rounding():
    rng = np.random.default_rng(5)
    a = np.exp2(rng.uniform(-30, 30, 200)).astype(f32) * rng.choice([f32(-1), f32(1)], 200)
    b = np.exp2(rng.uniform(-30, 30, 200)).astype(f32)
    for p, q in zip(a, b):
        assert rn32(Fraction(float(p)) * Fraction(float(q))) == Fraction(float(p * q))
        assert rn32(Fraction(float(p)) - Fraction(float(q))) == Fraction(float(p - q))
    tiny = Fraction(3, 2 ** 150)  # a tie between two subnormals: to the even one
    assert rn32(tiny) == Fraction(2, 2 ** 149)


def test_power_of_two_fold_is_exact():
    x, z = samples()
    assert (x == 0).any() and (np.abs(x) < 2.0 ** -19).any() and (np.abs(x) > 200).any()
    checked = 0
    for f in LADDER:
        vx, vz, fx, fz = skew_floors(f, x, z)
        split32_x, split32_z = vx - fx, vz - fz  # the reference's two roundings, in float32
        for c, i, v, d32 in list(zip(x, fx, vx, split32_x)) + list(zip(z, fz, vz, split32_z)):
            assert Fraction(float(v)) == Fraction(f) * Fraction(float(c)), "f c is exact for f = 2^k"
            split, fused = split_and_fused(f, c, i)
            assert split == fused, "f=%g c=%r i=%r" % (f, c, i)
            assert split == Fraction(float(d32)), "the model is float32's subtraction"
            checked += 1
    print("checked %d (f, coordinate, floor) triples" % checked)
    assert checked == len(LADDER) * 2 * len(x)


def test_other_frequencies_need_the_subtraction():
    """f = 2.5 (the table loop's stepdown in the GPU tests): f c rounds, and rounding f c - i once is not rounding it twice."""
    x, z = samples()
    vx, vz, fx, fz = skew_floors(2.5, x, z)
    differ = 0
    for c, i in list(zip(x, fx)) + list(zip(z, fz)):
        split, fused = split_and_fused(2.5, c, i)
        differ += split != fused
    print("f = 2.5: %d of %d samples differ between the fused and the split form" % (differ, 2 * len(x)))
    assert differ >= 1
