"""Reference driver of the octave shapes (nz_fractal_shaped, enum nz_fractal_shape): FractalGenerator.NoiseValue's octave
loop (Noise/Fractal/Fractal.cs:114-131, oracle fractal_value) with the accumulation replaced per shape, evaluated per cell
over the oracle's basis value (oracle.noise_value) and norm (oracle.fractal_norm).  Every step is one numpy float32
operation in the order the kernels use, so the strict kernels must match it bit for bit:

    Fbm     t += a * v
    Billow  s = |2v - 1|;  t += a * s
    Ridged  r = offset - |2v - 1|;  r = r * r;  r = r * w;  t += a * r;  w = fmin(fmax(r * gain, 0), 1)     (w = 1 first)

and the result is t / norm.  Needs no change to the oracle."""
import ctypes
import ctypes.util

import numpy as np

import oracle as O

f32 = np.float32
FBM, BILLOW, RIDGED = 0, 1, 2

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.exp2f.argtypes = [ctypes.c_float]
_libm.exp2f.restype = ctypes.c_float


def shape_octave(shape, t, w, a, v, offset=f32(1.0), gain=f32(2.0)):
    """One octave of the table above: (t, w) -> (t, w).  Arrays or scalars, all float32; fmin / fmax are C's (a NaN
    operand yields the other one), as on the device."""
    if shape == FBM:
        return t + a * v, w
    e = np.abs(f32(2.0) * v - f32(1.0))
    if shape == BILLOW:
        return t + a * e, w
    if shape != RIDGED:
        raise ValueError("unknown octave shape %r" % (shape,))
    r = f32(offset) - e
    r = r * r
    r = r * w
    t = t + a * r
    w = np.fmin(np.fmax(r * f32(gain), f32(0.0)), f32(1.0))
    return t, w


def _noise(noise_type):
    return np.vectorize(lambda x, z: O.noise_value(noise_type, float(x), float(z)), otypes=[f32])


def fractal_shaped(noise_type, rows, cols, hurst=0.0, amp=1.0, stepdown=2.0, detune=0.0, octaves=1, xpos=0, zpos=0,
                   noise_size=1000, shape=FBM, offset=1.0, gain=2.0, row_ids=None):
    """The (rows, cols) plane nz_fractal_shaped writes for a tile at (xpos, zpos); row_ids: evaluate only these rows of
    it (returns len(row_ids) rows)."""
    z = np.arange(rows) if row_ids is None else np.asarray(row_ids)
    xi = (np.arange(cols).astype(f32) + f32(xpos)) / f32(noise_size)
    zi = (z.astype(f32) + f32(zpos)) / f32(noise_size)
    XI, ZI = np.broadcast_arrays(xi[None, :], zi[:, None])
    G = f32(_libm.exp2f(-f32(hurst)))  # exp2f(-hurst) of the host libm, as nz_stages.cpp and the oracle
    norm = f32(O.fractal_norm(hurst, octaves, amp))
    noise = _noise(noise_type)
    t = np.zeros(XI.shape, f32)
    w = np.ones(XI.shape, f32)
    det, f, a = f32(0.0), f32(1.0), f32(amp)
    for _ in range(octaves):
        xV, zV = f * XI, f * ZI
        t, w = shape_octave(shape, t, w, a, noise(xV, zV), f32(offset), f32(gain))
        det = det + f32(detune)
        f = f * (f32(stepdown) - det)
        a = a * G
    return t / norm
