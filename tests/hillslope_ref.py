"""Hillslope diffusion of nz_hillslope_diffusion (include/noize_hip.h) in plain numpy, float32 throughout, every operation
rounded once: vectorised over the lines, sequential along a line.  Planes are res x res arrays indexed [z, x],
c = z * res + x.

The scheme is backward Euler split by direction, (I - r Lx)(I - r Lz) h' = h, with the border cells held (Dirichlet): they
keep their bits.  The amplification 1 / ((1 + r lx)(1 + r lz)) is positive for every r, so nothing oscillates at a large dt
(Peaceman-Rachford tends to -1 there).

    r = diffusivity * dt (one product),  B = 1 + 2 * r
    tables, i = 1 .. res-2:  den_1 = B,  den_i = B - r * cp_{i-1},  inv_i = 1 / den_i,  cp_i = r * inv_i
    one line solve over v_0 .. v_{n-1}:
        p_0 = v_0;          p_i = (v_i + r * p_{i-1}) * inv_i   for i = 1 .. n-2
        x_{n-1} = v_{n-1};  x_i = p_i + cp_i * x_{i+1}          for i = n-2 .. 1;     x_0 = v_0
    one step: half-step X solves every row z = 1 .. res-2 along x (rows 0 and res-1 are copied), half-step Z solves every
    column x = 1 .. res-2 of that result along z; `iterations` steps follow one another on the same tables.

res < 3 gives out = h; r == 0 gives out = h bit for bit by definition (the recurrence would flip the sign of a -0.0); border
cells keep their bits; in exact arithmetic the result stays within the input's minimum and maximum; a NaN or inf in a line
spreads along that line and then across it.

    tables(r, n, dtype) -> (inv, cp)               entries 1 .. n-2 (0 and n-1 are unused and hold 0)
    solve_lines(v, r, inv, cp) -> x                the line solve along the LAST axis of v, every line at once
    step(h, r, inv, cp) -> h'                      half-step X, then half-step Z
    diffuse_r(h, r, iterations, dtype) -> h'       the model for a given r; dtype float64: the same recurrences in double
    diffuse(h, diffusivity, dt, iterations) -> h'  the model, the hosts' HillslopeDiffusionStage
    dense(h, r) -> h'                              one step by a dense float64 solve of (I - r Lz)(I - r Lx), small tiles"""
import numpy as np

f32 = np.float32
DEFAULTS = dict(diffusivity=0.01, dt=1.0, iterations=1)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def coefficient(diffusivity, dt):
    return f32(diffusivity) * f32(dt)


def tables(r, n, dtype=f32):
    r = dtype(r)
    B = dtype(1.0) + dtype(2.0) * r
    inv, cp = np.zeros(n, dtype), np.zeros(n, dtype)
    for i in range(1, n - 1):
        den = B if i == 1 else B - r * cp[i - 1]
        inv[i] = dtype(1.0) / den
        cp[i] = r * inv[i]
    return inv, cp


def solve_lines(v, r, inv, cp):
    """v: (lines, n), n >= 3.  Every line solved along its n values; the two ends are held."""
    n = v.shape[-1]
    x = v.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, n - 1):           # p_i into x
            x[:, i] = (v[:, i] + r * x[:, i - 1]) * inv[i]
        for i in range(n - 2, 0, -1):       # x_i over p_i
            x[:, i] = x[:, i] + cp[i] * x[:, i + 1]
    return x


def step(h, r, inv, cp):
    g = h.copy()
    g[1:-1, :] = solve_lines(h[1:-1, :], r, inv, cp)                                    # rows 1 .. res-2 along x
    out = g.copy()
    out[:, 1:-1] = np.ascontiguousarray(solve_lines(np.ascontiguousarray(g[:, 1:-1].T), r, inv, cp).T)  # columns along z
    return out


def diffuse_r(h, r, iterations=1, dtype=f32):
    src = np.ascontiguousarray(h, f32)
    res = src.shape[0]
    assert src.shape == (res, res)
    r = f32(r)
    if res < 3 or r == f32(0.0):
        return src.astype(dtype)
    inv, cp = tables(r, res, dtype)
    out = src.astype(dtype)
    for _ in range(iterations):
        out = step(out, dtype(r), inv, cp)
    return out


def diffuse(h, diffusivity=0.01, dt=1.0, iterations=1):
    return diffuse_r(h, coefficient(diffusivity, dt), iterations)


def dense(h, r):
    """One step of the scheme as two dense float64 solves over the interior unknowns, the held cells on the right-hand side."""
    h = np.asarray(h, np.float64)
    res = h.shape[0]
    r = float(f32(r))
    m = res - 2
    A = (1.0 + 2.0 * r) * np.eye(m) - r * (np.eye(m, k=1) + np.eye(m, k=-1))
    g = h.copy()
    rhs = h[1:-1, 1:-1].copy()                 # rows z = 1 .. res-2, unknowns x = 1 .. res-2
    rhs[:, 0] += r * h[1:-1, 0]
    rhs[:, -1] += r * h[1:-1, -1]
    g[1:-1, 1:-1] = np.linalg.solve(A, rhs.T).T
    out = g.copy()
    rhs = g[1:-1, 1:-1].copy()                 # columns x = 1 .. res-2, unknowns z = 1 .. res-2
    rhs[0, :] += r * g[0, 1:-1]
    rhs[-1, :] += r * g[-1, 1:-1]
    out[1:-1, 1:-1] = np.linalg.solve(A, rhs)
    return out
