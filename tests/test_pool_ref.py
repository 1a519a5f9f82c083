"""tests/pool_ref.py against the C oracle (the walk), against hand-placed cells (the mask geometry) and against the table of
launch forms it restates (the rule).  No GPU."""
import numpy as np
import pytest

import pool_ref as R

f32 = np.float32
ORDER = ["px", "pz", "water"]


def oracle_drain(oracle, pool, height, iterations):
    """-> (plane, queue sorted by (px, pz, water)) of the oracle's drainParticles form"""
    L = oracle.LiveErosionOracle(height, oracle.erosion_params(), capacity=4 * pool.size * max(iterations, 1) + 16)
    L.pool[:] = pool
    L.pool_automata(iterations, drain=True)
    assert L.count.value <= len(L.queue)
    return L.pool, np.sort(L.queued()[ORDER], order=ORDER)


def as_queue(items):
    q = np.zeros(len(items), [("px", np.int32), ("pz", np.int32), ("water", np.float32)])
    for i, (px, pz, w) in enumerate(items):
        q[i] = (px, pz, w)
    return np.sort(q, order=ORDER)


# ---- a. the walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [2, 3, 9, 33, 34])
def test_the_python_walk_equals_the_c_oracle_bit_for_bit(oracle, res):
    drained = {}
    for name, (pool, height) in R.adversarial_planes(res).items():
        for iterations in (1, 3):
            want = oracle.pool_automata(pool, height, iterations)
            got = R.pool_automata(pool, height, iterations)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, res, iterations)
            wplane, wq = oracle_drain(oracle, pool, height, iterations)
            gplane, gq = R.pool_automata(pool, height, iterations, drain=True)
            assert np.array_equal(gplane.view(np.uint32), wplane.view(np.uint32)), (name, res, iterations, "drain")
            gq = as_queue(gq)
            assert len(gq) == len(wq) and np.array_equal(gq, wq), (name, res, iterations, len(gq), len(wq))
            drained[name] = len(wq)
    for name in R.DRAINING:
        assert drained[name] > 0, (name, res)
    for name in R.NOT_DRAINING:
        assert drained[name] == 0, (name, res)


def test_the_walk_on_known_answers():
    # a drain: the dry, lower neighbour takes all of it (or it leaves as one particle)
    h = np.tile(np.linspace(0.2, 0.8, 8, dtype=f32)[:, None], (1, 8))
    p = np.zeros((8, 8), f32)
    p[4, 4] = 0.01
    q = []
    a = p.copy()
    R.spread_pool(a, h, 4, 4)
    assert a[3, 4] == f32(0.01) and a.sum() == f32(0.01)
    a = p.copy()
    R.spread_pool(a, h, 4, 4, q)
    assert q == [(3, 4, f32(0.01))] and not a.any()
    # below the threshold nothing moves; at it, it does
    for w, moves in ((R.BELOW, False), (R.ACT, True)):
        a = p.copy()
        a[4, 4] = w
        R.spread_pool(a, h, 4, 4)
        assert (a[4, 4] == 0) == moves
    # the hash: the bits as a signed int, the two zeros folded; negative sums order backwards
    assert R.float_hash(f32(-0.0)) == R.float_hash(f32(0.0)) == 0
    assert R.float_hash(f32(-2.0)) > R.float_hash(f32(-1.0)) and R.float_hash(f32(-1.0)) < R.float_hash(f32(1e-30))
    # ties: `t` moves left while cmp < 0, and cmp is -1 on equal hashes, so four tied neighbours end up in reverse order
    b = [(1, f32(0.5), f32(0)), (2, f32(0.5), f32(0)), (3, f32(0.5), f32(0)), (4, f32(0.5), f32(0))]
    R._sort4(b)
    assert [e[0] for e in b] == [4, 3, 2, 1]
    # the same cell twice (a corner's clamped neighbours) compares 0 and keeps its place
    b = [(7, f32(0.5), f32(0)), (7, f32(0.5), f32(0)), (3, f32(0.1), f32(0)), (4, f32(0.9), f32(0))]
    R._sort4(b)
    assert [e[0] for e in b] == [3, 7, 7, 4]


@pytest.mark.parametrize("res", [9, 66, 130])
def test_the_adversarial_planes_hold_what_they_are_named_for(oracle, res):
    P = R.adversarial_planes(res)
    # thresholds: within three iterations cells start acting by receiving (new mask bits) and stop acting by giving while
    # still wet (stale bits, which the clean between iterations drops)
    pool, height = P["thresholds"]
    for v in (f32(0.0005), R.BELOW, R.ACT, R.ABOVE):
        assert (pool == v).any()
    planes = [pool]
    for _ in range(3):
        planes.append(oracle.pool_automata(planes[-1], height, 1))
    up = sum(int((~R.acts(a) & R.acts(b)).sum()) for a, b in zip(planes, planes[1:]))
    down = sum(int((R.acts(a) & ~R.acts(b) & (b > 0)).sum()) for a, b in zip(planes, planes[1:]))
    assert up > 0 and down > 0, (up, down)
    # negative terrain, the two zeros, ties
    assert (P["negative_terrain"][1] < 0).any() and (P["negative_terrain"][1] > 0).any() and (P["all_negative"][1] < 0).all()
    zh = P["signed_zeros"][1]
    assert not zh.any() and np.signbit(zh).any() and not np.signbit(zh).all()
    pool, height = P["flat_lake"]
    assert np.unique(height).size == 1 and np.unique(pool[::2, ::2]).size == 1 and pool[0, 0] != pool[0, 1]
    pool, height = P["level_surface"]
    assert np.unique(height).size > 4 and ((pool + height) == f32(0.5)).sum() > pool.size // 2
    # border: all four lines and corners act
    pool = P["border"][0]
    assert R.acts(pool[0, :]).all() and R.acts(pool[-1, :]).all() and R.acts(pool[:, 0]).all() and R.acts(pool[:, -1]).all()
    # runs: a full row and a full column; at 130 a run of consecutive steps through three words, one that ends at step 31, one
    # that starts at step 32, and two with a wet cell that does not act between them
    pool = P["runs"][0]
    assert R.acts(pool[:, res // 2]).all() and R.acts(pool[res // 3, :]).all()
    if res == 130:
        steps = lambda k, zoff: R.acts(pool[(k & 1)::2, 2 * k + zoff])   # the xoff = 0 steps of walk k
        assert steps(6, 0)[28:65].all() and {R.step_of(2 * s, 12, res)[1] for s in range(28, 65)} == {0, 1, 2}
        assert steps(2, 0)[20:32].all() and not steps(2, 0)[32] and R.step_of(62, 4, res)[3] == 31
        assert steps(4, 0)[32:41].all() and not steps(4, 0)[31] and R.step_of(64, 8, res)[1:] == (1, 4, 0)
        assert steps(8, 0)[3:10].all() and steps(8, 0)[11:16].all() and pool[20, 16] == f32(0.0005)


# ---- b. the masks ---------------------------------------------------------------------------------------------------
def one(res, x, z, w=0.5):
    p = np.zeros((res, res), f32)
    p[x, z] = w
    return p


def test_mask_geometry_known_answers():
    assert (R.total_words(172), R.total_words(160), R.total_words(514)) == (1032, 960, 9252)
    assert [(R.walks(r), R.words(r)) for r in (2, 3, 64, 65, 66, 130)] == [(1, 1), (1, 1), (32, 1), (32, 2), (33, 2), (65, 3)]
    # res 2: four cells, one walk, four classes, bit 0 each
    assert [R.step_of(x, z, 2) for x in (0, 1) for z in (0, 1)] == [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 0, 0)]
    # res 3: the last row of an odd plane is written but never walked
    assert all(R.step_of(x, 2, 3) is None for x in range(3)) and R.step_of(2, 1, 3) == (1, 0, 0, 1)
    assert R.nonempty_words(one(3, 1, 2)) == 0 and R.acting_steps(one(3, 1, 2)) == 0
    for res in (64, 65, 66, 130):
        # column 0 of an odd walk (k = 1: rows 2 and 3) has no step; of an even walk it is step 0 of class 0 / 1
        assert R.step_of(0, 2, res) is None and R.step_of(0, 3, res) is None
        assert R.step_of(0, 0, res) == (0, 0, 0, 0) and R.step_of(0, 5, res) == (1, 0, 2, 0)
        assert R.nonempty_words(one(res, 0, 2)) == 0 and R.nonempty_words(one(res, 0, 4)) == 1
        # an odd walk starts at column 1: class 0 there, class 2 at column 2
        assert R.step_of(1, 2, res) == (0, 0, 1, 0) and R.step_of(2, 2, res) == (2, 0, 1, 0)
        # the last step of word 0: x = 62 + (k & 1) for xoff = 0, one further for xoff = 1
        assert R.step_of(62, 0, res) == (0, 0, 0, 31) and R.step_of(63, 2, res) == (0, 0, 1, 31)
        assert R.step_of(63, 1, res) == (3, 0, 0, 31)
        if res % 2:
            assert all(R.step_of(x, res - 1, res) is None for x in (0, 1, res - 1))
    for res in (65, 66, 130):
        # cell x = 64 + (k & 1) starts word 1
        assert R.step_of(64, 0, res) == (0, 1, 0, 0) and R.step_of(64, 1, res) == (1, 1, 0, 0)
        assert R.step_of(64, 2, res) == (2, 0, 1, 31)
        if res > 65:
            assert R.step_of(65, 2, res) == (0, 1, 1, 0) and R.step_of(65, 0, res) == (2, 1, 0, 0)
    assert R.step_of(128, 0, 130) == (0, 2, 0, 0) and R.step_of(129, 2, 130) == (0, 2, 1, 0) and R.step_of(129, 0, 130) == (2, 2, 0, 0)
    # counts: two cells of one word, a cell of its neighbour class, a cell that does not act, a cell without a step
    p = one(130, 4, 0) + one(130, 6, 0) + one(130, 5, 0) + one(130, 8, 0, R.BELOW) + one(130, 0, 2) + one(130, 70, 0, R.ACT)
    assert R.acting_steps(p) == 4 and R.nonempty_words(p) == 3
    assert len(R.words_ever([p, one(130, 4, 0), one(130, 4, 1)])) == 4
    # an all-wet plane: every word, except where the last word of a walk holds one step only (res = 64 n + 2): on an odd walk
    # that step of the xoff = 1 classes is cell x = res, outside the plane
    for res in (2, 64, 172):
        assert R.nonempty_words(np.ones((res, res), f32)) == R.total_words(res)
    for res in (66, 130):
        assert R.nonempty_words(np.ones((res, res), f32)) == R.total_words(res) - 2 * (R.walks(res) // 2)
    assert R.acting_steps(np.ones((66, 66), f32)) == 66 * 66 - 33 // 2 * 2      # column 0 of the 16 odd walks, both rows
    assert R.acting_steps(np.ones((65, 65), f32)) == 65 * 64 - 32
    assert [float(v) for v in (R.BELOW, R.ACT, R.ABOVE)] == sorted(float(v) for v in (R.BELOW, R.ACT, R.ABOVE))
    assert list(R.acts(np.array([0, -1, 0.0005, R.BELOW, R.ACT, R.ABOVE, 1], f32))) == [False] * 4 + [True] * 3


# ---- c. the rule ----------------------------------------------------------------------------------------------------
def test_the_rule_restates_the_table_of_forms():
    E = R.expected_form
    big, res = R.LIMIT + 1, 172
    few, most = res * res // 2, (res * res * 7 + 7) // 8
    assert (R.LIMIT, R.SMALL, R.LIST_CAP, R.WET_SHARE, R.HINT_AGE) == (1024, 512, 8192, (7, 8), 8)
    assert E(1, 1, None, R.LIMIT, few, res) == (1, 1, 0)              # A
    assert E(1, 1, None, big, few, res) == (1, 0, 0)                  # B
    assert E(1, 1, None, big, most, res) == (1, 0, 1)                 # C
    assert E(1, 1, None, big, most - 1, res) == (1, 0, 0)
    assert E(1, 1, R.SMALL, R.LIMIT, few, res) == (0, 1, 0)           # D
    assert E(1, 1, R.SMALL, big, few, res) == (0, 1, 0)               # E
    assert E(1, 1, R.SMALL + 1, 5, few, res) == (1, 1, 0)             # a larger report: dense again, A
    assert E(1, 1, R.SMALL, 5, few, res, age=R.HINT_AGE + 1) == (1, 1, 0)   # a report too old to count
    assert E(1, 1, R.SMALL, 5, few, res, age=R.HINT_AGE) == (0, 1, 0)
    assert E(0, 1, R.SMALL, big, most, res) == (0, 0, 0)              # G
    assert E(1, 0, R.SMALL, big, most, res) == (1, 0, 0)              # H
    assert E(1, 2, None, big, few, res) == (0, 1, 0)                  # I
