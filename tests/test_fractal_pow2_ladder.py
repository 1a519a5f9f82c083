"""The power-of-two octave ladder of the strict simplex fBm kernel (fractal_simplex_tab_kernel, nz_octave_table.ladder_lo),
restated in numpy float32 and compared bit for bit with the reference's skew (np_noise.snoise2: vx = f x, s = vx Cy + vy Cy,
u = v + s, floor): when every octave frequency f is 2^k, u = f * (x + (x Cy + y Cy)) has the same bits, so the kernel forms
x + s0 once per row and multiplies.  Two predicates decide where the kernel does that; both are restated here as the C++
has them, and the test asserts that EVERY input they admit is bit-equal -- u, both floors and the full snoise value, for
every octave of the table:

    host    ladder_lo(f[0..n))   0 unless 1 <= n <= 16 and every f[i] is a positive, normal, exact power of two;
                                 otherwise 2^-64 / min(1, min f[i])                      (nz_stages.cpp, fractal_octave_table)
    device  ladder_row           ladder_lo > 0, fmax * reach < 2^20 (NZ_TAB_LIMIT), and every coordinate is 0 or at
                                 least ladder_lo in magnitude; a NaN fails                (nz_fractal.hip, ladder_row)
"""
import numpy as np
import pytest

import np_noise as N

f32 = np.float32
CY = f32(0.366025403784439)
NZ_OCT_TAB = 16
NZ_TAB_LIMIT = f32(1048576.0)
OCTAVES = 13


def octave_freqs(stepdown, detune, octaves):
    """f_0 = 1, f_{i+1} = f_i * (stepdown - detune_{i+1}), one float32 rounding per step (fractal_octave_table)."""
    out, f, det = [], f32(1.0), f32(0.0)
    with np.errstate(over="ignore", under="ignore"):
        for _ in range(octaves):
            out.append(f)
            det = det + f32(detune)
            f = f * (f32(stepdown) - det)
    return np.array(out, f32)


def ladder_lo(freqs):
    """The host predicate: the flag (0 = no ladder) and the guard's lower bound in one value."""
    if not 1 <= len(freqs) <= NZ_OCT_TAB:
        return f32(0.0)
    g = f32(1.0)
    for fi in freqs:
        m, _ = np.frexp(fi)
        if not (np.isfinite(fi) and fi >= f32(2.0) ** -126 and m == f32(0.5)):
            return f32(0.0)
        g = min(g, fi)
    return f32(2.0) ** -64 / g


def ladder_row(lo, fmax, x, y):
    """The device predicate, per cell (the kernel also wants it of every lane of the wave, which only narrows it)."""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    with np.errstate(invalid="ignore"):
        reach = np.maximum(np.abs(x), np.abs(y))
        ok = (lo > 0) & (f32(fmax) * reach < NZ_TAB_LIMIT)
        for c in (x, y):
            ok = ok & ((c == 0) | (np.abs(c) >= lo))
    return ok


def skew_reference(f, x, y):
    vx, vy = f * x, f * y
    s = vx * CY + vy * CY
    return vx, vy, vx + s, vy + s


def skew_ladder(f, x, y):
    s0 = x * CY + y * CY
    return f * x, f * y, f * (x + s0), f * (y + s0)


def snoise2_skewed(vx, vy, ux, uy):
    """np_noise.snoise2 from the floors on (the part of snoise2_tab the ladder leaves as it is)."""
    f = f32
    Cx, Cz, Cw = f(0.211324865405187), f(-0.577350269189626), f(0.024390243902439)
    ix, iy = np.floor(ux), np.floor(uy)
    t = ix * Cx + iy * Cx
    x0x, x0y = vx - ix + t, vy - iy + t
    gt = x0x > x0y
    i1x, i1y = np.where(gt, f(1.0), f(0.0)), np.where(gt, f(0.0), f(1.0))
    x12 = [x0x + Cx - i1x, x0y + Cx - i1y, x0x + Cz, x0y + Cz]
    ix, iy = N.mod289(ix), N.mod289(iy)
    p = [N.permute(N.permute(iy + f(0.0)) + ix + f(0.0)), N.permute(N.permute(iy + i1y) + ix + i1x),
         N.permute(N.permute(iy + f(1.0)) + ix + f(1.0))]
    m = [np.maximum(f(0.5) - (x0x * x0x + x0y * x0y), f(0.0)),
         np.maximum(f(0.5) - (x12[0] * x12[0] + x12[1] * x12[1]), f(0.0)),
         np.maximum(f(0.5) - (x12[2] * x12[2] + x12[3] * x12[3]), f(0.0))]
    m = [v * v for v in m]
    m = [v * v for v in m]
    x = [f(2.0) * N.frac(v * Cw) - f(1.0) for v in p]
    h = [np.abs(v) - f(0.5) for v in x]
    a0 = [a - np.floor(a + f(0.5)) for a in x]
    m = [mk * (f(1.79284291400159) - f(0.85373472095314) * (a * a + hh * hh)) for mk, a, hh in zip(m, a0, h)]
    g0 = a0[0] * x0x + h[0] * x0y
    g1 = a0[1] * x12[0] + h[1] * x12[1]
    g2 = a0[2] * x12[2] + h[2] * x12[3]
    return f(130.0) * (m[0] * g0 + m[1] * g1 + m[2] * g2)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def coordinate_cases(lo, fmax, rng):
    """(x, y, name -> slice): every family of inputs the guard has to get right, scaled to this ladder's bounds."""
    top = NZ_TAB_LIMIT / f32(fmax)  # coordinates up to the table limit at the largest frequency
    below_top = np.nextafter(top, f32(0.0))
    up, down = np.nextafter(lo, f32(1.0)), np.nextafter(lo, f32(0.0))
    fam = {}
    n = 4096
    fam["uniform"] = (rng.uniform(-1, 1, n) * top, rng.uniform(-1, 1, n) * top)
    fam["negative"] = (-rng.uniform(0, 1, n) * top, -rng.uniform(0, 1, n) * top)
    big = rng.uniform(0.9, 1, n) * below_top
    fam["large"] = (np.minimum(big, below_top), rng.uniform(-1, 1, n) * below_top)
    fam["at the limit"] = (np.array([below_top, -below_top, below_top, top, -top]),
                           np.array([below_top, below_top, -below_top, f32(1.0), f32(0.0)]))
    # every magnitude between the guard's bound and the table limit
    e = rng.uniform(np.log2(float(lo)), np.log2(float(top)), (2, n))
    sg = rng.choice([-1.0, 1.0], (2, n))
    fam["log-uniform"] = (sg[0] * 2.0 ** e[0], sg[1] * 2.0 ** e[1])
    a = (sg[0] * 2.0 ** e[0]).astype(f32)
    fam["x = -y"] = (a, -a)  # exact cancellation in s0
    fam["x ~ -y"] = (np.concatenate([a, a]), np.concatenate([-np.nextafter(a, f32(0.0)), -np.nextafter(a, a * f32(2.0))]))
    z = np.array([0.0, -0.0], f32)
    fam["zeros"] = (np.concatenate([np.repeat(z, 2), a[:64], np.zeros(64, f32)]),
                    np.concatenate([np.tile(z, 2), np.zeros(64, f32), a[:64]]))
    fam["at the bound"] = (np.array([lo, -lo, up, -up, lo, f32(0.0), up, lo]),
                           np.array([lo, lo, -up, up, f32(0.0), -lo, -lo, f32(1.0) if top > 1 else up]))
    fam["below the bound"] = (np.array([down, -down, lo, f32(0.0), down, down * f32(0.5)]),
                              np.array([lo, lo, -down, down, down, f32(1.0) if top > 1 else lo]))
    tiny = 2.0 ** rng.uniform(np.log2(float(lo)) - 8, np.log2(float(lo)) + 8, (2, n))
    fam["around the bound"] = (tiny[0], -tiny[1])
    fam["nan"] = (np.array([np.nan, 1.0, np.nan]), np.array([1.0, np.nan, np.nan]))
    xs, ys, where, at = [], [], {}, 0
    for name, (x, y) in fam.items():
        x, y = np.asarray(x, np.float64).astype(f32), np.asarray(y, np.float64).astype(f32)
        assert x.shape == y.shape
        xs.append(x); ys.append(y)
        where[name] = slice(at, at + x.size)
        at += x.size
    return np.concatenate(xs), np.concatenate(ys), where


# stepdown, what the bound must be: 2^-64 over the smallest frequency at or below 1
LADDERS = [(2.0, 2.0 ** -64), (4.0, 2.0 ** -64), (0.5, 2.0 ** -52)]


@pytest.mark.parametrize("stepdown,want_lo", LADDERS, ids=["x2", "x4", "x0.5"])
def test_every_admitted_input_is_bit_equal(stepdown, want_lo):
    freqs = octave_freqs(stepdown, 0.0, OCTAVES)
    lo, fmax = ladder_lo(freqs), freqs.max()
    assert lo == f32(want_lo)
    x, y, where = coordinate_cases(lo, fmax, np.random.default_rng(20240611))
    ok = ladder_row(lo, fmax, x, y)
    # the predicate admits what it is meant to admit, and turns the rest away (so nothing below is vacuous)
    for name in ("uniform", "negative", "large", "log-uniform", "x = -y", "x ~ -y", "zeros", "at the bound"):
        assert ok[where[name]].mean() > 0.99, name
    assert ok[where["zeros"]].all() and ok[where["at the bound"]].all()
    assert not ok[where["below the bound"]].any() and not ok[where["nan"]].any()
    lim = ok[where["at the limit"]]
    assert lim[:3].all() and not lim[3:].any()  # one ulp inside the table limit: in; at it: out
    assert 0.05 < ok[where["around the bound"]].mean() < 0.5
    xa, ya = x[ok], y[ok]
    assert xa.size > 20000
    for f in freqs:
        with np.errstate(all="raise"):  # an overflow or an underflow among admitted inputs: a hole in the guard's proof
            vx, vy, ux, uy = skew_reference(f, xa, ya)
            wx, wy, lx, ly = skew_ladder(f, xa, ya)
        for got, want, what in ((wx, vx, "vx"), (wy, vy, "vy"), (lx, ux, "ux"), (ly, uy, "uy"),
                                (np.floor(lx), np.floor(ux), "floor(ux)"), (np.floor(ly), np.floor(uy), "floor(uy)")):
            bad = bits(got) != bits(want)
            assert not bad.any(), "f=%g %s: %d differ, first at x=%r y=%r" % (f, what, bad.sum(), xa[bad][0], ya[bad][0])
        want = N.snoise2(vx, vy)
        assert np.array_equal(bits(snoise2_skewed(vx, vy, ux, uy)), bits(want)), "the restated tail is not snoise2"
        assert np.array_equal(bits(snoise2_skewed(wx, wy, lx, ly)), bits(want)), "f=%g: snoise differs" % f


def test_guard_keeps_clear_of_the_subnormals():
    """The proof's bound: among admitted inputs no nonzero intermediate of either form is below 2^-114, for the ladder
    with the smallest frequencies a table can hold here (x0.5 over 16 octaves)."""
    freqs = octave_freqs(0.5, 0.0, NZ_OCT_TAB)
    lo, fmax = ladder_lo(freqs), freqs.max()
    assert lo == f32(2.0 ** -49) and fmax == 1
    x, y, _ = coordinate_cases(lo, fmax, np.random.default_rng(7))
    ok = ladder_row(lo, fmax, x, y)
    xa, ya = x[ok], y[ok]
    s0 = xa * CY + ya * CY
    for v in (xa, ya, xa * CY, ya * CY, s0, xa + s0, ya + s0):
        for f in freqs:
            nz = np.abs((f * v)[v != 0])
            assert nz.min() >= f32(2.0 ** -114) and nz.max() < f32(2.0 ** 22)


@pytest.mark.parametrize("stepdown,detune,octaves", [(2.0, 0.01, 13), (3.0, 0.0, 13), (1.9168, 0.0317, 6), (2.0, 0.0, 17),
                                                     (2.0, 0.0, 0), (-2.0, 0.0, 4), (0.0, 0.0, 3), (2.0 ** -20, 0.0, 8),
                                                     (2.0 ** 20, 0.0, 8)])
def test_host_predicate_says_no(stepdown, detune, octaves):
    # not a power of two; no table (more octaves than it holds, none at all); negative, zero, subnormal and infinite steps
    freqs = octave_freqs(stepdown, detune, octaves)
    assert ladder_lo(freqs) == 0
    assert not ladder_row(ladder_lo(freqs), 1.0, f32(0.25), f32(0.5))


def test_host_predicate_says_yes():
    for stepdown, octaves, lo in ((2.0, 1, -64), (2.0, 16, -64), (4.0, 16, -64), (0.5, 16, -49), (0.25, 13, -40), (1.0, 5, -64)):
        assert ladder_lo(octave_freqs(stepdown, 0.0, octaves)) == f32(2.0) ** lo, (stepdown, octaves)
    # a table whose steps differ but are all powers of two (stepdown -3, detune -3.5: factors 0.5 and 4) is a ladder too
    freqs = octave_freqs(-3.0, -3.5, 3)
    assert list(freqs) == [1.0, 0.5, 2.0] and ladder_lo(freqs) == f32(2.0) ** -63
