"""The float32 identities behind the flow map's shared height differences and its one-sided K clamp (nz_flow_common.hpp).

Two adjacent cells with totals a and b need a - b and b - a.  The strict streaming kernel forms D = a - b once and hands it
to the other cell, which subtracts it: fmaxf(0, old - D) in place of fmaxf(0, old + (b - a)).  That is bit-equal for every
old flux in +0 .. +inf (no flux is -0 or NaN) -- but not for the map's first iteration, whose flux is fmaxf(0, b - a) of the
difference itself: there the sign of a zero reaches fmaxf.  And K = fminf(1, water / sum) is never below +0, so the
reference's fmaxf(0, .) around it returns its argument.

numpy's float32 arithmetic is IEEE round-to-nearest with denormals, like the kernels'.  fmaxf / fminf are modelled the way
the device computes them: a NaN operand yields the other operand, and of two zeros fmaxf(+0, x) is decided by the operand
order of v_max_f32 -- both orders are checked wherever a zero's sign could matter."""
import numpy as np

f32 = np.float32
N = 1 << 22


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def fmax0(x):
    """fmaxf(+0, x): +0 for a NaN and for either zero, x above zero.  Every x this module compares is the same in both forms
    whenever it is a zero, except in the first-iteration check, which looks at the sign itself."""
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, f32(0.0)).astype(f32)


def fmax0_keeps_zero_sign(x):
    """fmaxf(+0, x) of an implementation that returns x for x == -0 (either zero is a correct IEEE maximum of +0 and -0)"""
    with np.errstate(invalid="ignore"):
        return np.where((x > 0) | ((x == 0) & np.signbit(x)), x, f32(0.0)).astype(f32)


def special(rng, n, nonneg):
    """n float32: random bit patterns (every exponent, denormals, NaNs) with +-0, +-inf, NaN and denormals salted in, and
    small integers so that equal pairs are common; `nonneg`: +0 .. +inf only, no NaN"""
    x = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(f32).copy()
    salt = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0, 3.4e38, -3.4e38], f32)
    k = rng.integers(0, 4, n)
    x[k == 0] = salt[rng.integers(0, salt.size, int((k == 0).sum()))]
    x[k == 1] = rng.integers(-3, 4, int((k == 1).sum())).astype(f32)
    if nonneg:
        x = np.abs(x)
        x[np.isnan(x)] = f32(0.0)
    return x


def triples(seed):
    rng = np.random.default_rng(seed)
    a, b, old = special(rng, N, False), special(rng, N, False), special(rng, N, True)
    assert not np.signbit(old).any() and not np.isnan(old).any()
    return a, b, old


def test_subtracting_the_neighbours_difference_is_bit_equal():
    a, b, old = triples(11)
    with np.errstate(all="ignore"):
        D = a - b
        shared, direct = old - D, old + (b - a)
        # the sums themselves differ only where both are NaN (a NaN's sign) -- which fmaxf replaces
        differ = bits(shared) != bits(direct)
        assert np.isnan(shared[differ]).all() and np.isnan(direct[differ]).all()
        for fmax in (fmax0, fmax0_keeps_zero_sign):
            assert np.array_equal(bits(fmax(shared)), bits(fmax(direct)))
    # the sample does reach what the argument is about
    assert (D == 0).sum() > N // 100 and np.isnan(D).sum() > N // 100 and np.isinf(D).sum() > N // 100
    assert ((old == 0) & (D == 0)).sum() > 1000


def test_the_first_iteration_cannot_take_the_negated_difference():
    a, b, _ = triples(12)
    with np.errstate(all="ignore"):
        D = a - b
        own, negated = b - a, -D
    # a == b: b - a is +0, -(a - b) is -0
    differ = bits(own) != bits(negated)
    assert differ.sum() > N // 100
    assert ((own[differ] == 0) | np.isnan(own[differ])).all()
    zeros = differ & (own == 0)
    assert zeros.any() and not np.signbit(own[zeros]).any() and np.signbit(negated[zeros]).all()
    # ... and fmaxf(+0, -0) may return either zero: the flux, and everything downstream of it, would depend on the
    # implementation's choice, so the first iteration keeps a subtraction of its own
    assert not np.array_equal(bits(fmax0_keeps_zero_sign(own)), bits(fmax0_keeps_zero_sign(negated)))


def test_k_is_never_below_plus_zero():
    rng = np.random.default_rng(13)
    w, s = special(rng, N, True), special(rng, N, True)
    with np.errstate(all="ignore"):
        sdt = s * f32(0.2)
        assert not np.signbit(sdt).any() and not np.isnan(sdt).any()
        q = w / sdt
        assert np.isnan(q).sum() > N // 100  # 0 / 0 and inf / inf are there
        k = np.where(q < 1, q, f32(1.0)).astype(f32)  # fminf(1, q): 1 for a NaN
    assert not np.isnan(k).any() and not np.signbit(k).any() and (k >= 0).all() and (k <= 1).all()
    assert np.array_equal(bits(fmax0(k)), bits(k)) and np.array_equal(bits(fmax0_keeps_zero_sign(k)), bits(k))
