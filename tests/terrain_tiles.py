"""Adversarial height tiles for the terrain stages (hydraulic erosion plain and _ex, fluvial erosion, depression filling,
drainage area) and their stripe entries:
plain numpy, no GPU and no oracle, so this module and tests/test_terrain_tiles.py import without a build.  Every generator
takes (res, rng) and returns a contiguous float32 res x res plane indexed [z, x].  tests/test_terrain_tiles.py checks with
the numpy models alone that each one does what its name says; tests/test_gpu_sweep_terrain.py runs the kernels on them.

    ties     terraces(K)   a smooth relief rounded to multiples of 1/K, K dyadic: differences are exact, plateaus and equal
                           neighbours everywhere
             cheb_cone     max(|x-c|, |z-c|) / 4: a cardinal and two diagonal neighbours are equally lower, the cardinal has to
                           win through d > d * DIAG          (cheb_pit: the same upside down)
             manh_cone     (|x-c| + |z-c|) / 4: two cardinals are lower by d and the diagonal between them by 2d, the diagonal
                           has to win through 2d * DIAG > d   (manh_pit: upside down; on its axes two diagonals tie)
             checker       ((x + z) & 1) / 2: every inner cell is a pit or a peak, a peak's four cardinal slopes tie, as do
                           its four diagonal zeros
    scales   metres        relief * 1e4 + 3000: an ulp there is 2^-12 .. 2^-10, the fill's default epsilon is rounded away
             negative      -(relief * 50)
             tiny          relief * 1e-36: neighbouring cells differ by subnormal amounts
             zeros         +0 / -0 by a random mask with about 1 % of the cells at +-1e-45 (the smallest subnormal)
    winding  serpentine(pitch)  walls with one gap each at alternating ends behind a high border with one low cell at the
                           mouth: the way out of the far end is back along every corridor, so the fill's front comes
                           through the same 64 x 16 tiles again and again
    plain    relief, noisy, uniform, wide: a smooth relief in [0, 1], the same with N(0, 0.01) on it, uniform random cells,
                           and both signs over a random power of ten (as tests/test_gpu_sweep.py)

cut_rows, cut_ties and cut_subnormal say what a tile holds across the cuts of a split into row stripes."""
import functools

import numpy as np

f32 = np.float32


def _value_noise(res, rng, cell):
    """Uniform values on a lattice of `cell` cells at a random phase, interpolated with the smoothstep weight."""
    g = rng.random((res // cell + 3, res // cell + 3))
    t = (np.arange(res) + rng.random() * cell) / cell
    i = t.astype(np.int64)
    f = t - i
    f = f * f * (3.0 - 2.0 * f)
    rows = g[i] * (1.0 - f)[:, None] + g[i + 1] * f[:, None]
    return rows[:, i] * (1.0 - f)[None, :] + rows[:, i + 1] * f[None, :]


def relief(res, rng):
    """A smooth relief inside [0, 1]: value noise with features of 48 cells and, at 0.3 of the weight, of 12 cells.  It
    spans 0.3 to 0.6 on these tiles; neighbouring cells differ by about 0.01 and less."""
    return np.ascontiguousarray((_value_noise(res, rng, 48) + 0.3 * _value_noise(res, rng, 12)) / 1.3, f32)


def noisy(res, rng):
    return (relief(res, rng) + rng.standard_normal((res, res)).astype(f32) * f32(0.01)).astype(f32)


def uniform(res, rng):
    return rng.random((res, res), dtype=f32)


def wide(res, rng):
    return ((rng.random((res, res), dtype=f32) - f32(0.5)) * f32(10.0) ** int(rng.integers(-3, 4))).astype(f32)


def terraces(res, rng, K=16):
    """Multiples of 1/K of four times the relief: plateaus a few cells wide, their edges and corners."""
    assert K & (K - 1) == 0
    return (np.round(relief(res, rng) * f32(4 * K)) / f32(K)).astype(f32)


def _xz(res):
    z, x = np.mgrid[0:res, 0:res].astype(f32)
    c = f32((res - 1) / 2)  # a whole or a half number: every height below is a multiple of 1/8
    return np.abs(x - c), np.abs(z - c)


def cheb_cone(res, rng=None):
    ax, az = _xz(res)
    return np.ascontiguousarray(np.maximum(ax, az) * f32(0.25), f32)


def manh_cone(res, rng=None):
    ax, az = _xz(res)
    return np.ascontiguousarray((ax + az) * f32(0.25), f32)


def cheb_pit(res, rng=None):
    h = cheb_cone(res)
    return np.ascontiguousarray(h.max() - h, f32)


def manh_pit(res, rng=None):
    h = manh_cone(res)
    return np.ascontiguousarray(h.max() - h, f32)


def checker(res, rng=None):
    z, x = np.mgrid[0:res, 0:res]
    return np.ascontiguousarray(((x + z) & 1) * f32(0.5), f32)


def metres(res, rng):
    return (relief(res, rng) * f32(1e4) + f32(3000.0)).astype(f32)


def negative(res, rng):
    return (-(relief(res, rng) * f32(50.0))).astype(f32)


def tiny(res, rng):
    return (relief(res, rng) * f32(1e-36)).astype(f32)


def zeros(res, rng):
    h = np.where(rng.random((res, res)) < 0.5, f32(0.0), f32(-0.0)).astype(f32)
    speck = rng.random((res, res)) < 0.01
    sign = np.where(rng.random((res, res)) < 0.5, f32(1.0), f32(-1.0)).astype(f32)
    least = np.array([1], np.uint32).view(f32)[0]  # 1e-45, the smallest subnormal
    return np.ascontiguousarray(np.where(speck, sign * least, h), f32)


def serpentine(res, rng, pitch=6):
    """Corridors along x, `pitch` - 1 rows wide, between walls of height 5 on every row that is a multiple of `pitch`; wall
    k has its one gap at the east end when k is odd and at the west end when it is even.  The border is a wall as well, but
    for the cell (0, 1): the mouth, the one way out.  The floor is noise in [0, 0.01), far below the walls."""
    assert res >= 2 * pitch + 1 and pitch >= 2
    h = (rng.random((res, res), dtype=f32) * f32(0.01)).astype(f32)
    for k, z in enumerate(range(pitch, res - 1, pitch), 1):
        h[z, :] = f32(5.0)
        h[z, res - 2 if k & 1 else 1] = f32(0.005)
    h[0, :] = h[-1, :] = h[:, 0] = h[:, -1] = f32(5.0)
    h[0, 1] = f32(-1.0)
    return np.ascontiguousarray(h, f32)


# the tie group, the scale group and the plain tiles, by name
TIES = {"terraces4": functools.partial(terraces, K=4), "terraces16": functools.partial(terraces, K=16), "cheb_cone": cheb_cone,
        "manh_cone": manh_cone, "cheb_pit": cheb_pit, "manh_pit": manh_pit, "checker": checker}
SCALES = {"metres": metres, "negative": negative, "tiny": tiny, "zeros": zeros}
PLAIN = {"relief": relief, "noisy": noisy, "uniform": uniform, "wide": wide}
GENERATORS = {**TIES, **SCALES, **PLAIN}  # serpentine has a test of its own: its fill takes a hundred passes

# The serpentine of the GPU test, and what the model tests/fill_ref.py needs for it (tests/test_terrain_tiles.py holds the
# constants to the model): passes that changed a cell with the kernel's 64 x 16 tiles and a cap of 16, 3 and 1 sweeps.
SERPENTINE = dict(res=97, pitch=6, seed=5, eps=1e-4)
SERPENTINE_PASSES = {16: 96, 3: 505, 1: 1506}


def serpentine_tile():
    s = SERPENTINE
    return serpentine(s["res"], np.random.default_rng(s["seed"]), s["pitch"])


def sea_at(h, q=0.3):
    """The cell value at the q quantile of the tile: a value the tile holds, so `h <= seaLevel` decides whole plateaus."""
    flat = np.sort(np.asarray(h, f32).reshape(-1))
    return float(flat[int(q * (flat.size - 1))])


def cut_rows(rows, world):
    """The first owned row of the ranks 1 .. world - 1 of noize_job_amd.sharded.StripePlan: the cuts of `rows` rows."""
    base, rem = divmod(rows, world)
    return [k * base + min(k, rem) for k in range(1, world)]


def _across(h, world, test):
    out = []
    for r in cut_rows(h.shape[0], world):
        a, b = h[r - 1], h[r]
        out.append(int(test(a, b).sum() + test(a[1:], b[:-1]).sum() + test(a[:-1], b[1:]).sum()))
    return out


def cut_ties(h, world):
    """Per cut: the pairs of cells either side of it, straight or diagonal, of equal height -- a receiver of a first or
    last owned row is then chosen among equal drops, some of them in a ghost row."""
    return _across(np.asarray(h, f32), world, lambda a, b: a == b)


def cut_subnormal(h, world):
    """Per cut: the pairs either side of it, straight or diagonal, whose heights differ by a subnormal amount."""
    def test(a, b):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        return (d > 0) & (d < 2.0 ** -126)
    return _across(np.asarray(h, f32), world, test)
