"""The pool automaton (PoolAutomataJob: `iterations` x four colour passes of WorldTile.SpreadPool), restated a second time.

Three parts, none of which shares code with the library or with the C oracle:

  a. the walk itself in float32 scalars (spread_pool, pool_automata): slow, for planes of 34^2 cells and fewer.
     tests/test_pool_ref.py requires it to equal oracle/noize_oracle.c (nzo_spread_pool, :1062-1103) and the drain form of
     oracle/noize_oracle_live.c bit for bit on the planes of adversarial_planes(), so that the C oracle has an independently
     written witness on exactly the inputs where the neighbour sort matters;
  b. the geometry of the acting-step masks, from the comments of noize_job_amd/csrc/nz_elementwise.hip (pool_masks,
     pool_mark_acting, pool_masks_kernel): which (class, word, walk) a cell's step falls in, how many words a plane has;
  c. the rule by which pool_job (noize_job_amd/csrc/nz_stages.cpp) and pool_sparse_kernel choose a launch form:
     expected_form().  A second statement of the rule: if the rule moves, tests/test_gpu_pool_forms.py fails loudly and is
     updated with it.

Planes are indexed [x, z] (x * res + z in memory)."""
import numpy as np

f32 = np.float32
ACT = f32(1e-3)          # SpreadPool's `hWater < 1E-3f` (LiveErosionDataTypes.cs:938-1010)
QUARTER = f32(0.25)
NEIGHBOURS = ((0, 1), (1, 0), (0, -1), (-1, 0))   # up, right, down, left; SafeIdx clamps at the border


# ---- a. the walk ----------------------------------------------------------------------------------------------------
def float_hash(v):
    """float.GetHashCode: the bits as a signed int, +-0 -> 0"""
    v = f32(v)
    return 0 if v == 0 else int(v.view(np.int32))


def _cmp(a, b):
    """FloodedNeighbor.CompareTo: the same cell -> 0, otherwise by the hash of height + water"""
    if a[0] == b[0]:
        return 0
    return 1 if float_hash(a[1] + a[2]) > float_hash(b[1] + b[2]) else -1


def _sort4(b):
    """NativeArray.Sort() on four elements: insertion sort, element i + 1 moves left while it compares < 0"""
    for i in range(3):
        j, t = i, b[i + 1]
        while j >= 0 and _cmp(t, b[j]) < 0:
            b[j + 1] = b[j]
            j -= 1
        b[j + 1] = t


def spread_pool(pool, height, x, z, drain=None):
    """One SpreadPool call at (x, z), in place.  drain: None = drainParticles off; a list = on, and a pool that finds a dry,
    lower neighbour is appended as (px, pz, water) instead of wetting it."""
    res = pool.shape[0]
    land, water = height[x, z], pool[x, z]
    if water <= 0:
        return
    surface = land + water
    flat = pool.reshape(-1)
    b = []
    for dx, dz in NEIGHBOURS:
        nx, nz = min(max(x + dx, 0), res - 1), min(max(z + dz, 0), res - 1)
        b.append((nx * res + nz, height[nx, nz], pool[nx, nz]))
    _sort4(b)
    for idx, bh, bw in b:   # (the values as the sort found them, not as earlier transfers of this call left them)
        diff = surface - (bh + bw)
        if water < ACT:
            continue
        if bw <= 0 and land >= bh:          # a drain: all of the water goes there
            if drain is None:
                flat[idx] = bw + water
            else:
                drain.append((idx // res, idx % res, water))
            water = f32(0)
            surface = land
        elif diff > 0:
            if water <= 0:
                continue
            fill = min(QUARTER * water, QUARTER * diff)
            water = water - fill
            surface = land + water
            flat[idx] = bw + fill
        elif diff < 0:
            if bw <= 0:
                continue
            fill = min(QUARTER * bw, f32(-0.25) * diff)
            water = water + fill
            surface = land + water
            flat[idx] = bw + f32(-1) * fill
    pool[x, z] = water


def pool_automata(pool, height, iterations, drain=False):
    """-> the new plane; with drain, (plane, [(px, pz, water), ...]) in the order of a sequential walk"""
    pool = np.array(pool, f32, order="C")
    height = np.ascontiguousarray(height, f32)
    res = pool.shape[0]
    assert pool.shape == height.shape == (res, res) and res >= 2
    queue = [] if drain else None
    for _ in range(iterations):
        for xoff in range(2):
            for zoff in range(2):
                for k in range(res // 2):
                    z = 2 * k + zoff
                    for x in range(xoff + (k & 1), res, 2):
                        if pool[x, z] > 0:
                            spread_pool(pool, height, x, z, queue)
    return (pool, queue) if drain else pool


# ---- b. the masks ---------------------------------------------------------------------------------------------------
def walks(res):
    return res // 2


def words(res):
    return ((res + 1) // 2 + 31) // 32


def total_words(res):
    return 4 * words(res) * walks(res)


def acts(w):
    """pool_step_acts: w > 0 and not (w < 1e-3), in float32"""
    w = np.asarray(w, f32)
    return (w > 0) & ~(w < ACT)


def step_of(x, z, res):
    """(class, word, walk, bit) of the step at cell (x, z), None if no pass has a step there"""
    k = z >> 1
    t = x - (k & 1)
    if k >= walks(res) or t < 0:
        return None
    return 2 * (t & 1) + (z & 1), (t >> 1) >> 5, k, (t >> 1) & 31


def _word_keys(pool):
    """the acting steps of a plane as (class * words + word) * walks + walk, one per step"""
    res = pool.shape[0]
    x, z = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    k = z >> 1
    t = x - (k & 1)
    on = acts(pool) & (k < walks(res)) & (t >= 0)
    cls, word = 2 * (t & 1) + (z & 1), (t >> 1) >> 5
    return ((cls * words(res) + word) * walks(res) + k)[on]


def acting_steps(pool):
    return int(_word_keys(pool).size)


def nonempty_words(pool):
    return int(np.unique(_word_keys(pool)).size)


def words_ever(planes):
    """the words that hold an acting step in any of the planes"""
    seen = set()
    for p in planes:
        seen.update(np.unique(_word_keys(p)).tolist())
    return seen


# ---- c. the rule ----------------------------------------------------------------------------------------------------
LIMIT = 1024           # nz_stages.cpp, pool_job: `constexpr int LIMIT = 1024` -- the words the one workgroup takes on
SMALL = LIMIT // 2     # pool_job: `dense = ... !(fresh && (unsigned)hint <= LIMIT / 2)`
LIST_CAP = 8192        # nz_elementwise.hip: `constexpr int NZ_POOL_LIST_CAP = 8192`
WET_SHARE = (7, 8)     # pool_sparse_kernel: `acting * 8 >= res * res * 7` -> ctl[3]
HINT_AGE = 8           # pool_job: `fresh = hint_seq != 0 && seq - hint_seq <= 8 && seq > hint_seq`


def expected_form(runs, sparse, previous, nonempty, acting, res, age=1):
    """info[2:5] of nz_debug_pool_last_job -- (the host enqueued the dense launches, the one-workgroup launch took the job,
    the dense passes walk whole rows) -- for a job on a plane with `nonempty` non-empty words and `acting` steps.
    previous: the word count the context's last one-workgroup launch reported, `age` such jobs ago; None if there was none."""
    if not runs:
        return (0, 0, 0)
    if not sparse:
        return (1, 0, 0)
    wet = int(acting * WET_SHARE[1] >= res * res * WET_SHARE[0])
    fresh = previous is not None and 1 <= age <= HINT_AGE
    dense = 0 if sparse == 2 else int(not (fresh and previous <= SMALL))
    took = int(not dense or nonempty <= LIMIT)
    return (dense, took, wet)


# ---- inputs where the walk goes wrong -------------------------------------------------------------------------------
BELOW, ABOVE = np.nextafter(ACT, f32(0)), np.nextafter(ACT, f32(1))


def _put(a, x, z, v):
    if 0 <= x < a.shape[0] and 0 <= z < a.shape[1]:
        a[x, z] = v


def _puddles(rng, res, cover):
    wet = rng.random((res, res)) < cover
    return np.where(wet, f32(0.002) + rng.random((res, res), dtype=f32) * f32(0.3), 0).astype(f32)


def adversarial_planes(res):
    """name -> (pool, height), float32 [x, z]"""
    rng = np.random.default_rng(7700 + res)
    P = {}
    checker = (np.add.outer(np.arange(res), np.arange(res)) & 1).astype(bool)

    # negative terrain: the hash order inverts among negative sums and folds the two zeros together
    P["negative_terrain"] = (_puddles(rng, res, 0.4), (rng.random((res, res), dtype=f32) * f32(2) - f32(1)).astype(f32))
    P["all_negative"] = (_puddles(rng, res, 0.4), (-f32(0.01) - rng.random((res, res), dtype=f32)).astype(f32))
    h = np.where(rng.random((res, res)) < 0.5, f32(-0.0), f32(0.0)).astype(f32)
    p = rng.choice(np.array([0, 0, 0.01, 0.02, 0.04], f32), (res, res)).astype(f32)
    P["signed_zeros"] = (p, h)

    # ties: all four neighbours of every cell equal in height and water, and different from the cell
    P["flat_lake"] = (np.where(checker, f32(0.3), f32(0.1)).astype(f32), np.full((res, res), 0.5, f32))
    h = (rng.integers(0, 13, (res, res)) / 64.0).astype(f32)      # a level surface (0.5 exactly) over an uneven bed ...
    p = (f32(0.5) - h).astype(f32)
    p[checker & (rng.random((res, res)) < 0.3)] += f32(0.125)      # ... with mounds that spread among tied neighbours
    P["level_surface"] = (p, h)

    # thresholds: water at 0.0005, just under 1e-3, at it, just above; large cells beside them (their neighbours cross upward
    # by receiving), cells just above the threshold on a slope (they cross downward by giving)
    cyc = np.array([0.0005, BELOW, ACT, ABOVE, 0.0, 0.004, 0.0011, 0.3], f32)
    x, z = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    p = cyc[(x * 3 + z * 5 + (x * z) // 3) % len(cyc)].astype(f32)
    h = (rng.random((res, res), dtype=f32) * f32(0.01) + f32(0.002) * (x + z).astype(f32)).astype(f32)
    P["thresholds"] = (p, h)

    # border: acting water on the four border lines and corners (a clamped neighbour is the cell itself)
    p = np.zeros((res, res), f32)
    for line in (p[0, :], p[-1, :], p[:, 0], p[:, -1]):
        line[:] = f32(0.05) + rng.random(res, dtype=f32) * f32(0.1)
    P["border"] = (p, (rng.random((res, res), dtype=f32) * f32(0.2) - f32(0.1)).astype(f32))

    # runs: a full row and a full column; in step space (cell x = xoff + (k & 1) + 2 s of walk k) a run that ends at step 31, one
    # that starts at step 32, one from step 28 to the end of the row (three words at 130), two runs with one sub-threshold cell
    # between them; the same on an odd walk of the other z parity
    p = np.zeros((res, res), f32)
    p[:, res // 2] = f32(0.25)
    p[res // 3, :] = f32(0.25)
    for k, zoff, spans in ((2, 0, [(20, 32)]), (4, 0, [(32, 41)]), (6, 0, [(28, res)]), (8, 0, [(3, 10), (11, 16)]),
                           (3, 1, [(20, 32), (33, 40)]), (5, 1, [(0, res)]), (7, 1, [(32, 64), (65, res)])):
        z0 = 2 * k + zoff
        for s0, s1 in spans:
            for s in range(s0, s1):
                _put(p, (k & 1) + 2 * s, z0, f32(0.05) + f32(0.001) * f32(s % 7))
        if len(spans) == 2:
            _put(p, (k & 1) + 2 * spans[0][1], z0, f32(0.0005))
    P["runs"] = (p, (rng.random((res, res), dtype=f32) * f32(0.05)).astype(f32))

    # drains: a slope with isolated pools (drain on: particles), and pits whose water stays below the rim (none)
    h = (f32(0.01) * x + f32(0.003) * z + rng.random((res, res), dtype=f32) * f32(0.001)).astype(f32)
    p = np.where(rng.random((res, res)) < 0.06, f32(0.05), 0).astype(f32)
    p[-1, 0], p[-2, 0] = f32(0.05), f32(0)     # one pool beside a dry, lower cell at every size
    P["slope_pools"] = (p, h)
    h = (f32(1) + rng.random((res, res), dtype=f32) * f32(0.02)).astype(f32)
    p = np.zeros((res, res), f32)
    for cx in range(0, res - 1, 4):
        for cz in range(int(rng.integers(0, 3)), res, 3):
            h[cx, cz], h[cx + 1, cz] = f32(0.5), f32(0.6)
            p[cx, cz], p[cx + 1, cz] = f32(0.3), f32(0.0)
    P["pit_field"] = (p, h)
    return P


DRAINING = ("slope_pools",)     # drain on: the oracle queues particles at every size
NOT_DRAINING = ("pit_field",)   # ... and none


def mixture(res, cover, seed=0):
    """A plane with a share `cover` of its cells acting that mixes the cases above: negative terrain on one half and a
    quantised bed (tied sums) on the other, water in puddles, at the threshold values and in full lines, dry cells between."""
    rng = np.random.default_rng(8800 + res * 7 + seed)
    h = (rng.random((res, res), dtype=f32) * f32(0.4) - f32(0.2)).astype(f32)
    h[:, res // 2:] = (rng.integers(-6, 7, (res, res - res // 2)) / 64.0).astype(f32)
    p = rng.choice(np.array([0.002, ACT, ABOVE, 0.25, 0.0625, 0.3], f32), (res, res)).astype(f32)
    p += np.where(rng.random((res, res)) < 0.5, rng.random((res, res), dtype=f32) * f32(0.1), 0).astype(f32)
    gaps = np.array([0.0, 0.0, 0.0005, BELOW], f32)
    off = rng.random((res, res)) >= cover
    p[off] = rng.choice(gaps, int(off.sum()))
    if cover < 0.8:
        p[:, res // 3] = f32(0.25)
        p[res // 2, :] = f32(0.25)
    return p, h


def pits(res, n, depth, seed):
    """Isolated deep pits on a slightly bumpy floor: n random interior cells at height -0.5 holding `depth` of water, which
    spreads outward about one ring of cells per pass."""
    rng = np.random.default_rng(seed)
    h = (rng.random((res, res), dtype=f32) * f32(0.02)).astype(f32)
    p = np.zeros((res, res), f32)
    xs, zs = rng.integers(1, res - 1, n), rng.integers(1, res - 1, n)
    h[xs, zs] = f32(-0.5)
    p[xs, zs] = f32(depth)
    return p, h
