"""Reference driver of the domain warp (nz_fractal_warped*, WarpedNoiseStage): the shaped octave loop of
tests/fractal_shapes_ref.py read at coordinates displaced by a plain fBm of the same basis.  For the cell in column c and
row r of a tile at (xpos, zpos), ns = (float)noiseSize, every step one numpy float32 operation in this order:

    X  = c + xpos                 Z  = r + zpos
    xi = X / ns                   zi = Z / ns
    u  = xi * warpScale           v  = zi * warpScale
    qx = D(u, v)                  qz = D(u + 5.2, v + 1.3)
    Xw = X + (2 qx - 1) * s       Zw = Z + (2 qz - 1) * s          (s = warpStrength, in cells)
    px = Xw / ns                  pz = Zw / ns
    result = the shaped octave loop at (px, pz) / norm

D is the fBm (shape 0) over warpOctaves octaves with the same hurst, amplitude, stepdown and detune, divided by
oracle.fractal_norm(hurst, warpOctaves).  warpOctaves == 0 means no warp (D would be 0 / 0): the plain shaped plane.
The strict kernels must match this bit for bit."""
import numpy as np

import oracle as O
from fractal_shapes_ref import FBM, _libm, _noise, fractal_shaped, shape_octave

f32 = np.float32
OFF_X, OFF_Z = f32(5.2), f32(1.3)  # 0x40a66666, 0x3fa66666


def warp_coordinate(X, q, strength):
    """X + (2q - 1) * strength in float32 (2q is exact)."""
    return f32(X) + (f32(2.0) * f32(q) - f32(1.0)) * f32(strength)


def _octaves(noise, x, z, octaves, hurst, amp, stepdown, detune, shape=FBM, offset=1.0, gain=2.0):
    """The shaped octave sum (before the division by the norm) at per-cell coordinates x, z."""
    G = f32(_libm.exp2f(-f32(hurst)))
    t = np.zeros(x.shape, f32)
    w = np.ones(x.shape, f32)
    det, f, a = f32(0.0), f32(1.0), f32(amp)
    for _ in range(octaves):
        t, w = shape_octave(shape, t, w, a, noise(f * x, f * z), f32(offset), f32(gain))
        det = det + f32(detune)
        f = f * (f32(stepdown) - det)
        a = a * G
    return t


def _cells(rows, cols, xpos, zpos, row_ids):
    r = np.arange(rows) if row_ids is None else np.asarray(row_ids)
    X = np.arange(cols).astype(f32) + f32(xpos)
    Z = r.astype(f32) + f32(zpos)
    return np.broadcast_arrays(X[None, :], Z[:, None])


def displacement(noise_type, rows, cols, hurst=0.0, amp=1.0, stepdown=2.0, detune=0.0, xpos=0, zpos=0, noise_size=1000,
                 warp_scale=1.0, warp_octaves=4, row_ids=None):
    """(qx, qz): D at (u, v) and at (u + 5.2, v + 1.3) for every cell."""
    X, Z = _cells(rows, cols, xpos, zpos, row_ids)
    ns = f32(noise_size)
    u = X / ns * f32(warp_scale)
    v = Z / ns * f32(warp_scale)
    noise = _noise(noise_type)
    norm = f32(O.fractal_norm(hurst, warp_octaves, amp))
    qx = _octaves(noise, u, v, warp_octaves, hurst, amp, stepdown, detune) / norm
    qz = _octaves(noise, u + OFF_X, v + OFF_Z, warp_octaves, hurst, amp, stepdown, detune) / norm
    return qx, qz


def fractal_warped(noise_type, rows, cols, hurst=0.0, amp=1.0, stepdown=2.0, detune=0.0, octaves=1, xpos=0, zpos=0,
                   noise_size=1000, shape=FBM, offset=1.0, gain=2.0, warp_strength=0.0, warp_scale=1.0, warp_octaves=4,
                   row_ids=None):
    """The (rows, cols) plane nz_fractal_warped writes for a tile at (xpos, zpos); row_ids: only these rows."""
    if warp_octaves == 0:
        return fractal_shaped(noise_type, rows, cols, hurst, amp, stepdown, detune, octaves, xpos, zpos, noise_size,
                              shape, offset, gain, row_ids=row_ids)
    X, Z = _cells(rows, cols, xpos, zpos, row_ids)
    qx, qz = displacement(noise_type, rows, cols, hurst, amp, stepdown, detune, xpos, zpos, noise_size, warp_scale,
                          warp_octaves, row_ids)
    ns = f32(noise_size)
    px = warp_coordinate(X, qx, warp_strength) / ns
    pz = warp_coordinate(Z, qz, warp_strength) / ns
    norm = f32(O.fractal_norm(hurst, octaves, amp))
    return _octaves(_noise(noise_type), px, pz, octaves, hurst, amp, stepdown, detune, shape, offset, gain) / norm
