"""Every launch form of the pool automaton (nz_pool_automata, nz_pool_automata_job), reached on purpose.

pool_job (noize_job_amd/csrc/nz_stages.cpp) runs one job -- `iterations` x four colour passes of SpreadPool -- in one of
several ways; which one depends on two process-wide switches, on what the context's previous job reported, and on two
decisions taken on the device.  nz_debug_pool_forms sets the switches, nz_debug_pool_last_job says how the last job ran, and
tests/pool_ref.py restates the rule (expected_form) and the mask geometry every shape below is found through.

  A  first job of a context (or a job after a report above LIMIT / 2), at most LIMIT non-empty words: the dense launches are
     enqueued, the one-workgroup launch takes the job
  B  the same with more than LIMIT words: dense runs            C  ... and seven steps in eight acting: dense row walks
  D  after a report of at most LIMIT / 2, at most LIMIT words: the one-workgroup launch alone, from its list
  E  after such a report, more than LIMIT words (the hint is out of date): one workgroup scans every word
  F  at most LIMIT words at the start, and the list passes its capacity while the job runs
  G  nz_debug_pool_forms(0, -1): one lane per row, no masks
  H  nz_debug_pool_forms(-1, 0): dense runs with no list and no control block
  I  nz_debug_pool_forms(-1, 2) with more than LIMIT words: the one-workgroup launch, always

Every form runs with drain off and drain on.  After every job the plane must equal oracle.pool_automata bit for bit, with
drain on the queue (its length, and its particles sorted) the oracle's queue, and nz_debug_pool_last_job what expected_form
says.  Every test makes a context of its own: no other file's jobs are in the hint.  With NZ_POOL_RUNS or NZ_POOL_SPARSE set
in the environment the results are still compared; only the form assertions are dropped."""
import ctypes as C
import os

import numpy as np
import pytest

import pool_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
KNOBS = any(os.environ.get(k) for k in ("NZ_POOL_RUNS", "NZ_POOL_SPARSE"))
ORDER = ["px", "pz", "water", "pid"]
REACHED = set()        # (form, drain), entered after the form's assertions held
FORMS = "ABCDEFGHI"
SMALL_RES = (2, 3, 9, 65, 66, 130)   # 130: the first size with three words per walk


@pytest.fixture
def fresh(nj):
    """a context of the test's own, and the environment's switches back in force afterwards"""
    ctx = nj.Context(0)
    try:
        yield ctx
    finally:
        nj._native.lib.nz_debug_pool_forms(-1, -1)
        ctx.close()


def last_job(nj, ctx):
    info = (C.c_int32 * 6)()
    rc = nj._native.lib.nz_debug_pool_last_job(ctx._h, info)
    assert rc == nj._native.NZ_OK, nj._native.lib.nz_last_error()
    return list(info)


class Wanted:
    """The oracle's answer for a plane: the pool after `iterations`, and with drain the queue."""

    def __init__(self, oracle, pool, height, iterations, drain):
        self.pool, self.height, self.iterations, self.drain = pool, height, iterations, drain
        self.nonempty, self.acting = R.nonempty_words(pool), R.acting_steps(pool)
        if drain:
            L = oracle.LiveErosionOracle(height, oracle.erosion_params(), capacity=1 << 17)
            L.pool[:] = pool
            L.pool_automata(iterations, drain=True)
            self.count = L.count.value
            assert self.count <= len(L.queue)
            self.plane, self.queue = L.pool, np.sort(L.queued(), order=ORDER)
        else:
            self.count, self.queue = 0, None
            self.plane = oracle.pool_automata(pool, height, iterations)


class Runner:
    """Jobs on one context, one after the other, each completed and compared before the next."""

    def __init__(self, nj, ctx):
        self.nj, self.ctx = nj, ctx
        self.runs = self.sparse = 1   # what a job reads when neither the environment nor the hook says otherwise
        self.previous = None          # the word count the last one-workgroup launch reported
        self.tiles = {}
        self.forms(-1, -1)

    def forms(self, runs, sparse):
        assert self.nj._native.lib.nz_debug_pool_forms(runs, sparse) == self.nj._native.NZ_OK
        self.runs, self.sparse = (1 if runs < 0 else int(runs != 0)), (1 if sparse < 0 else sparse)

    def planes(self, res):
        if res not in self.tiles:
            self.tiles[res] = (self.ctx.alloc(res * res), self.ctx.alloc(res * res))
        return self.tiles[res]

    def enqueue(self, w):
        """-> (handle, pool tile, queue or None)"""
        res = w.pool.shape[0]
        d_pool, d_h = self.planes(res)
        d_pool.CopyFrom(w.pool)
        d_h.CopyFrom(w.height)
        if not w.drain:
            return self.ctx.call("nz_pool_automata", d_pool.ptr, d_h.ptr, w.iterations, res), d_pool, None
        # a full queue drops whichever particle arrives last, which is not deterministic: room for all of them
        q = self.nj.ParticleQueue(self.ctx, w.count + 64)
        q.Clear(handle=False)
        return self.ctx.call("nz_pool_automata_job", d_pool.ptr, d_h.ptr, q._h, None, None, w.iterations, res, 1), d_pool, q

    def compare(self, w, d_pool, q, what):
        res = w.pool.shape[0]
        got = d_pool.ToArray((res, res))
        same = got.view(np.uint32) == w.plane.view(np.uint32)
        assert same.all(), "%s: %d of %d cells differ from the oracle, first at %s" % (
            what, int((~same).sum()), same.size, tuple(np.argwhere(~same)[0]))
        if q is not None:
            try:
                assert q.capacity > w.count
                assert q.Count == w.count, "%s: %d particles queued, the oracle has %d" % (what, q.Count, w.count)
                gq = np.sort(q.ToArray(), order=ORDER)
                for f in ORDER:
                    assert np.array_equal(gq[f], w.queue[f]), "%s: the queues differ in %s" % (what, f)
            finally:
                q.Dispose()

    def job(self, w, form=None, what=""):
        """runs the job, compares it, checks how it ran; `form`: the letter this job is meant to reach"""
        h, d_pool, q = self.enqueue(w)
        h.Complete()
        what = "%s %d^2 x%d drain=%d form %s" % (what, w.pool.shape[0], w.iterations, int(w.drain), form)
        self.compare(w, d_pool, q, what)
        info = last_job(self.nj, self.ctx)
        if not KNOBS:
            res = w.pool.shape[0]
            want = R.expected_form(self.runs, self.sparse, self.previous, w.nonempty, w.acting, res)
            assert tuple(info[:2]) == (self.runs, self.sparse), (what, info)
            assert tuple(info[2:5]) == want, "%s: ran as %s, the rule says %s (previous report %s, %d words, %d steps)" % (
                what, info, want, self.previous, w.nonempty, w.acting)
            if self.runs and self.sparse:   # the masks kernel stops counting once the list has overflowed
                assert info[5] == w.nonempty if w.nonempty <= R.LIST_CAP else info[5] > R.LIST_CAP, (what, info, w.nonempty)
            else:
                assert info[5] == -1, (what, info)
            if form is not None:
                assert tuple(info[2:5]) == FORM_INFO[form](w) or FORM_INFO[form](w) is None, (what, info)
                REACHED.add((form, bool(w.drain)))
        if info[5] >= 0:
            self.previous = info[5]
        return info

    def Dispose(self):
        for pair in self.tiles.values():
            for t in pair:
                t.Dispose()


def wet(w):
    return int(w.acting * 8 >= w.pool.size * 7)


# what the issue's table says of info[2:5] for each form, beside expected_form (None: set by the switches, checked there)
FORM_INFO = {"A": lambda w: (1, 1, wet(w)), "B": lambda w: (1, 0, 0), "C": lambda w: (1, 0, 1), "D": lambda w: (0, 1, wet(w)),
             "E": lambda w: (0, 1, wet(w)), "F": lambda w: None, "G": lambda w: (0, 0, 0), "H": lambda w: (1, 0, 0),
             "I": lambda w: (0, 1, wet(w))}


def spacer(oracle, res, value, drain):
    """an all-wet plane on a tilted bed: 172^2 reports 1032 words (above LIMIT / 2), 2^2 reports 4"""
    x = np.arange(res, dtype=f32)
    return Wanted(oracle, np.full((res, res), value, f32), (f32(0.001) * np.add.outer(x, f32(0.5) * x)).astype(f32), 1, drain)


# ---- A, D, G, H on the adversarial planes ---------------------------------------------------------------------------
@pytest.mark.parametrize("drain", [False, True], ids=["wet", "drain"])
@pytest.mark.parametrize("res", SMALL_RES)
def test_small_planes_in_forms_A_D_G_H(nj, fresh, oracle, res, drain):
    run = Runner(nj, fresh)
    planes = R.adversarial_planes(res)
    names = list(planes)
    first = names[SMALL_RES.index(res) % len(names)]   # the plane that is the context's first job: another one at every size
    names.remove(first)
    large, small = spacer(oracle, 172, 0.25, drain), spacer(oracle, 2, 0.25, drain)
    assert large.nonempty > R.SMALL and small.nonempty <= R.SMALL
    try:
        for i, name in enumerate([first] + names):
            w = Wanted(oracle, *planes[name], 3, drain)
            assert w.nonempty <= R.LIMIT
            if drain and name in R.DRAINING:
                assert w.count > 0, (name, res)
            if drain and name in R.NOT_DRAINING:
                assert w.count == 0, (name, res)
            if i == 0:
                run.job(w, "A", name + " (first job)")
            run.job(large, None, "spacer")
            run.job(w, "A", name + " (after a large report)")   # dense again: A, not D
            run.job(small, None, "spacer")
            run.job(w, "D", name)
            run.forms(0, -1)
            run.job(w, "G", name)
            run.forms(-1, 0)
            run.job(w, "H", name)
            run.forms(-1, -1)
    finally:
        run.Dispose()


def test_a_small_job_after_a_large_report_is_dense_again(nj, fresh, oracle):
    run = Runner(nj, fresh)
    w = Wanted(oracle, *R.adversarial_planes(66)["negative_terrain"], 3, False)
    large, small = spacer(oracle, 172, 0.25, False), spacer(oracle, 2, 0.25, False)
    try:
        a = run.job(w, "A", "first")
        d = run.job(w, "D", "after its own small report")
        run.job(large, None, "a large job, itself after a small report")
        a2 = run.job(w, "A", "after a large report")
        d2 = run.job(w, "D", "after its own small report again")
        if not KNOBS:
            assert (a[2], d[2], a2[2], d2[2]) == (1, 0, 1, 0) and a[5] == d[5] == a2[5] == w.nonempty <= R.SMALL
    finally:
        run.Dispose()


# ---- B, C, E, I (and G, H) on planes with more than LIMIT words -------------------------------------------------------
def first_res_above_limit(cover, odd):
    """the first size at which the mixture plane has more than LIMIT non-empty words, searched upward from the first size
    with that many words at all"""
    res = 2
    while R.total_words(res) <= R.LIMIT:
        res += 1
    while R.nonempty_words(R.mixture(res, cover)[0]) <= R.LIMIT:
        res += 1
    if odd:   # one odd size above it
        res += 1 + res % 2
        while R.nonempty_words(R.mixture(res, cover)[0]) <= R.LIMIT:
            res += 2
    return res


@pytest.mark.parametrize("drain", [False, True], ids=["wet", "drain"])
@pytest.mark.parametrize("odd", [False, True], ids=["first", "odd"])
@pytest.mark.parametrize("cover,form", [(0.5, "B"), (0.97, "C")])
def test_large_planes_in_forms_B_C_E_I_G_H(nj, fresh, oracle, cover, form, odd, drain):
    res = first_res_above_limit(cover, odd)
    assert res % 2 == 1 if odd else R.nonempty_words(R.mixture(res - 1, cover)[0]) <= R.LIMIT
    run = Runner(nj, fresh)
    w = Wanted(oracle, *R.mixture(res, cover), 3, drain)
    small = spacer(oracle, 2, 0.25, drain)
    assert w.nonempty > R.LIMIT and wet(w) == int(form == "C"), (res, w.nonempty, w.acting)
    if drain:
        assert w.count > 0
    try:
        run.job(w, form, "mixture %.2f (first job)" % cover)
        run.job(small, None, "spacer")      # after a report above LIMIT / 2: dense
        run.job(w, "E", "mixture %.2f" % cover)
        run.forms(-1, 2)
        run.job(w, "I", "mixture %.2f" % cover)
        run.forms(0, -1)
        run.job(w, "G", "mixture %.2f" % cover)
        run.forms(-1, 0)
        run.job(w, "H", "mixture %.2f" % cover)
        run.forms(-1, -1)
        run.job(w, form, "mixture %.2f (after its own large report)" % cover)
    finally:
        run.Dispose()


# ---- F: the list overflows while the job runs -------------------------------------------------------------------------
F_RES, F_MOST = 640, 12


def pit_plane(n, depth, seed, drain):
    """pool_ref.pits.  With drain on, water that reaches the dry, bumpy floor leaves as particles and the pools stop
    spreading (the words ever touched stay near 3 700 of 12 800 at 1000 pits): there the floor carries a film of 0.0005 -- too
    little to act, so the start is as sparse -- except on one cell in fifty, which still drains."""
    pool, height = R.pits(F_RES, n, depth, seed)
    if drain:
        rng = np.random.default_rng(seed + 99)
        film = np.where(rng.random(pool.shape) < 0.02, f32(0), f32(0.0005)).astype(f32)
        pool = np.where(pool > 0, pool, film).astype(f32)
    return pool, height


def overflowing_job(oracle, pool, height, drain, start_limit):
    """The job of the fewest iterations n whose list has passed LIST_CAP, by the oracle's planes after 0 .. n - 2 iterations:
    at least one whole iteration and one clean run after the overflow.  (A lower bound on the list: every cell that acts at an
    iteration boundary has its bit set, a word enters the list with its first bit, and entries are never dropped.)"""
    assert R.nonempty_words(pool) <= start_limit, (R.nonempty_words(pool), start_limit)
    L = oracle.LiveErosionOracle(height, oracle.erosion_params(), capacity=1 << 17)
    L.pool[:] = pool
    seen = R.words_ever([pool])
    done = 0
    while len(seen) <= R.LIST_CAP:
        L.pool_automata(1, drain=drain)
        done += 1
        seen |= R.words_ever([L.pool])
        assert done + 2 <= F_MOST, "after %d iterations only %d words were ever non-empty" % (done, len(seen))
    return Wanted(oracle, pool, height, done + 2, drain)


@pytest.mark.parametrize("drain", [False, True], ids=["wet", "drain"])
@pytest.mark.parametrize("second", [False, True], ids=["first-job", "after-a-small-report"])
def test_the_list_overflows_while_the_job_runs(nj, fresh, oracle, second, drain):
    n, depth, seed = (500, 3.0, 2) if second else (1000, 1.0, 1)
    w = overflowing_job(oracle, *pit_plane(n, depth, seed, drain), drain, R.SMALL if second else R.LIMIT)
    if drain:
        assert w.count > 0
    run = Runner(nj, fresh)
    try:
        if second:
            run.job(spacer(oracle, 2, 0.25, drain), None, "spacer")
        info = run.job(w, "F", "%d pits" % n)
        if not KNOBS:
            assert (info[2], info[3]) == (0 if second else 1, 1), info
    finally:
        run.Dispose()


# ---- three jobs in flight -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drain", [False, True], ids=["wet", "drain"])
def test_three_jobs_chained_without_a_wait(nj, fresh, oracle, drain):
    """small -> F-sized -> small, each on its own buffers, chained by `dep`.  The host may or may not have seen the earlier
    job's report when it enqueues the next: the form is not asserted, the results must be right either way."""
    run = Runner(nj, fresh)
    ws = [Wanted(oracle, *R.adversarial_planes(66)["runs"], 3, drain),
          overflowing_job(oracle, *pit_plane(1000, 1.0, 1, drain), drain, R.LIMIT),
          Wanted(oracle, *R.adversarial_planes(130)["thresholds"], 3, drain)]
    tiles = [(fresh.alloc(w.pool.size), fresh.alloc(w.pool.size)) for w in ws]
    try:
        jobs, dep = [], None
        for w, pair in zip(ws, tiles):   # (the uploads synchronise the stream; the three jobs are enqueued below)
            pair[0].CopyFrom(w.pool)
            pair[1].CopyFrom(w.height)
        queues = [nj.ParticleQueue(fresh, w.count + 64) if drain else None for w in ws]
        for q in queues:
            if q is not None:
                q.Clear(handle=False)
        fresh.synchronize()
        for w, (d_pool, d_h), q in zip(ws, tiles, queues):
            res = w.pool.shape[0]
            if drain:
                dep = fresh.call("nz_pool_automata_job", d_pool.ptr, d_h.ptr, q._h, None, None, w.iterations, res, 1, dep=dep)
            else:
                dep = fresh.call("nz_pool_automata_job", d_pool.ptr, d_h.ptr, None, None, None, w.iterations, res, 0, dep=dep)
            jobs.append((w, d_pool, q))
        dep.Complete()
        for i, (w, d_pool, q) in enumerate(jobs):
            run.compare(w, d_pool, q, "chained job %d" % i)
    finally:
        for pair in tiles:
            for t in pair:
                t.Dispose()
        run.Dispose()


# ---- the hooks themselves -------------------------------------------------------------------------------------------
def test_the_hooks_refuse_what_they_cannot_answer(nj, fresh, oracle):
    lib, N = nj._native.lib, nj._native
    info = (C.c_int32 * 6)()
    assert lib.nz_debug_pool_last_job(fresh._h, info) == N.NZ_ERR_INVALID      # no pool job yet
    assert lib.nz_debug_pool_last_job(None, info) == N.NZ_ERR_INVALID
    assert lib.nz_debug_pool_last_job(fresh._h, None) == N.NZ_ERR_INVALID
    assert lib.nz_debug_pool_forms(1, 3) == N.NZ_ERR_INVALID
    run = Runner(nj, fresh)
    w = Wanted(oracle, *R.adversarial_planes(9)["border"], 1, False)
    try:
        # a job of no iterations launches nothing and is no job to report
        fresh.call("nz_pool_automata", *[t.ptr for t in run.planes(9)], 0, 9).Complete()
        assert lib.nz_debug_pool_last_job(fresh._h, info) == N.NZ_ERR_INVALID
        run.forms(0, 2)
        a = run.job(w, None, "runs off wins over sparse")
        run.forms(-1, -1)
        b = run.job(w, None, "the environment's switches again")
        if not KNOBS:
            assert a == [0, 2, 0, 0, 0, -1] and b[:4] == [1, 1, 1, 1] and b[5] == w.nonempty
    finally:
        run.Dispose()


def test_every_form_was_reached():
    if KNOBS:
        return
    missing = sorted((f, d) for f in FORMS for d in (False, True) if (f, d) not in REACHED)
    assert not missing, "forms never reached (form, drain): %s" % missing
