"""Row-stripe sharding of one large grid over the GPUs of a node (new-framework feature; the
reference only has independent clamped tiles, Scripts/MeshTileGenerator.cs:166-192).

Rank r of P owns rows [r*R/P, (r+1)*R/P) x all columns of a (grows x cols) grid.  The
noise stage needs no communication (world offsets, Noise/Fractal/Fractal.cs:109-116); every other
stage is a small-radius stencil.  Two ways of feeding the stencils their ghost rows:

  * haloMode "recompute" (default for the metric pipeline, whose source is closed-form noise): each
    rank evaluates the noise on its owned rows plus the total stencil radius of the pipeline
    (Gauss 17x2 + flow 5x2 + erosion 5 = 49 rows) and every launch produces a window that shrinks by
    the radius it consumed.  No data-path communication at all; ~2.4 % redundant rows per side at
    2048-row stripes.
  * haloMode "exchange": before each launch the ranks exchange the ghost rows that launch consumes
    with their two neighbours (rank-1 / rank+1 only) -- the form a pipeline needs whose source plane
    is not recomputable (an uploaded height map).
  * haloMode "exchange_once": the source plane is produced on the owned rows only, its ghost rows for
    the WHOLE pipeline (49 rows) are exchanged once, and everything after runs like "recompute" -- one
    latency-bound exchange instead of one per launch, for the price of the same redundant rows.

Because the kernels compute each cell with the same operations wherever it sits, either way the
sharded result equals the single-GPU monolithic result bit for bit; the only clamps are at the
global border.

The schedule below is host logic shared by two compute back ends:
  * HipStripeOps  -- the product path: C-ABI stripe entry points on device buffers (torch CUDA tensors
    used as plain HBM allocations), halo exchange by torch.distributed P2P on the `nccl` backend
    (= RCCL over xGMI);
  * any object with the same methods (tests/ supplies one built on the CPU oracle, driven over `gloo`).
"""
import copy
import ctypes as C

from . import _native as N


class StripePlan:
    """Geometry of one rank's stripe.  Every plane buffer has `halo` ghost rows above and below the
    owned rows (the ones hanging over the global border are never read)."""

    def __init__(self, rank, world, grows, cols, halo, neighbours_own_halo=True):
        assert 0 <= rank < world and grows >= world
        base, rem = divmod(grows, world)
        self.rank, self.world, self.grows, self.cols, self.halo = rank, world, grows, cols, halo
        self.g0 = rank * base + min(rank, rem)           # first owned global row
        self.nown = base + (1 if rank < rem else 0)
        self.rows = self.nown + 2 * halo                 # rows in every buffer
        self.own0, self.own1 = halo, halo + self.nown
        self.grow0 = self.g0 - halo
        # an exchange takes ghost rows from the adjacent rank only; recomputed ghost rows may reach further
        assert self.nown >= halo or not neighbours_own_halo, "stripe thinner than the halo"

    def stripe(self, pitch=0):
        return N.Stripe(self.cols, self.rows, self.grow0, self.grows, self.own0, self.own1, pitch)

    def widened(self, up, down):
        """The same buffer with the produced rows grown by `up` rows above and `down` rows below the
        owned ones, clipped to the global grid: what a launch has to produce so that later launches
        find their ghost rows without an exchange."""
        if up == 0 and down == 0:
            return self
        assert up <= self.halo and down <= self.halo
        v = copy.copy(self)
        v.own0 = max(self.own0 - up, -self.grow0)
        v.own1 = min(self.own1 + down, self.grows - self.grow0)
        v.g0, v.nown = self.grow0 + v.own0, v.own1 - v.own0
        return v

    def rows_window(self, a, b):
        """The same buffer producing only buffer rows [a, b) of the owned ones (a launch split into an interior part,
        which reads no ghost row, and the border parts that wait for the halo exchange)."""
        v = copy.copy(self)
        v.own0, v.own1 = max(a, self.own0), min(b, self.own1)
        v.g0, v.nown = self.grow0 + v.own0, max(0, v.own1 - v.own0)
        return v

    @property
    def up(self):
        return self.rank - 1 if self.rank > 0 else None

    @property
    def down(self):
        return self.rank + 1 if self.rank + 1 < self.world else None


def split_iterations(n, cap):
    """n applications in launches of at most `cap` (any count: stripes ping-pong between two buffers)."""
    launches = (n + cap - 1) // cap
    base, rem = divmod(n, launches)
    return [base + (1 if i < rem else 0) for i in range(launches)]


class PipelineParams:
    """The metric pipeline's stage parameters."""

    def __init__(self, noiseType=3, hurst=0.4, startingAmplitude=1.0, stepdown=2.0, detuneRate=0.0, octaves=13,
                 xpos=0, zpos=0, noiseSize=1700, filter=2, gaussIterations=17, flowIterations=5, normMin=0.0,
                 normMax=0.005, erosionIterations=5, haloMode="exchange"):
        assert haloMode in ("exchange", "recompute", "exchange_once")
        self.__dict__.update(locals())
        del self.__dict__["self"]


FLOW_PLANES = 5  # water, fN, fS, fE, fW: state buffers are [5, rows, cols]


def _launch_radii(ops, p):
    """Per launch of the schedule: (stage, fused applications, rows consumed above, rows consumed below)."""
    out = []
    if p.gaussIterations > 0:
        k_off = ops.kernel_filter_halo_rows(p.filter, 1)
        cap = max(1, ops.kernel_filter_max_fused(p.filter))
        out += [("gauss", T, T * k_off, T * k_off) for T in split_iterations(p.gaussIterations, cap)]
    if p.flowIterations > 0:
        # whole iterations fused on chip, <= flow_fused_max() per launch; a launch of n iterations reads
        # height and state 2n rows beyond the rows it produces
        out += [("flow", n, 2 * n, 2 * n) for n in split_iterations(p.flowIterations, ops.flow_fused_max())]
    left = p.erosionIterations
    while left > 0:
        E = min(left, ops.erosion_max_fused())
        out.append(("erosion", E, E, 0))                # the min window reaches upwards only
        left -= E
    return out


def halo_rows_needed(ops, p):
    """Ghost rows every plane buffer needs on each side: the widest single launch when ghost rows are
    exchanged before each launch, the whole pipeline's radius when they are recomputed."""
    radii = _launch_radii(ops, p)
    if p.haloMode in ("recompute", "exchange_once"):
        return max(sum(r[2] for r in radii), sum(r[3] for r in radii), 1)
    return max([max(r[2], r[3]) for r in radii] + [1])


def pipeline_steps(ops, plan, p, bufs, result, on_stage=None):
    """The sharded metric pipeline as a generator: yields (planes, up_rows, down_rows) wherever the
    ranks must exchange ghost rows (never in haloMode "recompute", once in "exchange_once"), runs the stripe
    kernels in between.
    bufs = (A, B, S0, S1): two height planes [plan.rows, cols] and two flow-state buffers
    [5, plan.rows, cols].  The plane whose owned rows hold the result is appended to `result`.
    `on_stage(name)` (optional) is called where a stage begins ("noise", "gauss", "flow", "erosion") and
    once at the end ("end"): the hook bench.py hangs its stream markers on."""
    A, B, S0, S1 = bufs
    mark = on_stage if on_stage is not None else (lambda name: None)
    current = "noise"
    mark(current)
    cur, nxt = A, B
    s_cur, s_nxt = S0, S1
    radii = _launch_radii(ops, p)
    recompute = p.haloMode in ("recompute", "exchange_once")   # launches produce shrinking windows, no per-launch exchange
    # rows beyond the owned ones that the remaining launches will still consume
    need_up = sum(r[2] for r in radii) if recompute else 0
    need_down = sum(r[3] for r in radii) if recompute else 0
    if p.haloMode == "exchange_once":
        ops.fractal(cur, plan, p)                 # stands for any source plane, e.g. an uploaded height map
        answer = yield [cur], need_up, need_down  # its ghost rows for the whole pipeline, once
        if answer == "async":
            yield ("finish",)                     # everything that follows reads them
    else:
        ops.fractal(cur, plan.widened(need_up, need_down), p)
    flow_launches = [i for i, r in enumerate(radii) if r[0] == "flow"]
    def split_launch(launch, win, up, down, answer):
        """Runs `launch(window)` once -- or, when the exchange that was just requested is asynchronous (the runner
        answered "async"), first on the interior rows, which read no ghost row, while the halos are in flight, then
        (after the runner has finished the exchange) on the border rows."""
        lo, hi = win.own0 + up, win.own1 - down
        if answer != "async" or hi <= lo:
            if answer == "async":
                yield ("finish",)
            launch(win)
            return
        launch(win.rows_window(lo, hi))
        yield ("finish",)
        if up > 0:
            launch(win.rows_window(win.own0, lo))
        if down > 0:
            launch(win.rows_window(hi, win.own1))

    for i, (stage, n, up, down) in enumerate(radii):
        if stage != current:
            current = stage
            mark(current)
        if recompute:
            need_up, need_down = need_up - up, need_down - down
        win = plan.widened(need_up, need_down)
        answer = None
        if stage == "gauss":
            if not recompute:
                answer = yield [cur], up, down
            yield from split_launch(lambda w: ops.kernel_filter(cur, nxt, w, p.filter, n), win, up, down, answer)
            cur, nxt = nxt, cur
        elif stage == "flow":
            first, last = i == flow_launches[0], i == flow_launches[-1]
            if not recompute:
                if first:  # height: exchanged once, read by every launch
                    widest = max(radii[j][2] for j in flow_launches)
                    answer = yield [cur], widest, widest
                else:
                    answer = yield [s_cur[k] for k in range(FLOW_PLANES)], up, down
            yield from split_launch(lambda w: ops.flow_fused(cur, s_cur, s_nxt, nxt, w, n, first, last, p.normMin, p.normMax),
                                    win, up, down, answer)
            s_cur, s_nxt = s_nxt, s_cur
            if last:
                cur, nxt = nxt, cur
        else:
            if not recompute:
                answer = yield [cur], up, down
            yield from split_launch(lambda w: ops.erosion(cur, nxt, w, n), win, up, down, answer)
            cur, nxt = nxt, cur
    mark("end")
    result.append(cur)


def run_pipeline(ops, comm, plan, p, bufs, on_stage=None):
    """One pass of the sharded metric pipeline on this rank; returns the plane holding the result.
    A comm with begin() / finish() exchanges asynchronously: the launch that needs the ghost rows runs its interior
    rows while they travel (RCCL P2P on the process group's own stream) and its border rows after finish()."""
    result = []
    gen = pipeline_steps(ops, plan, p, bufs, result, on_stage)
    overlap = getattr(comm, "overlap", False)
    pending = None
    try:
        req = next(gen)
        while True:
            if req == ("finish",):
                comm.finish(pending)
                pending = None
                req = next(gen)
                continue
            planes, up_rows, down_rows = req
            if overlap:
                pending = comm.begin(planes, plan, up_rows, down_rows)
                req = gen.send("async")
            else:
                comm.exchange(planes, plan, up_rows, down_rows)
                req = next(gen)
    except StopIteration:
        pass
    return result[0]


def _copy_ghost_rows(reqs, plans, copy_rows):
    """One exchange of a lockstep rehearsal: every rank's request (planes, up_rows, down_rows) served by direct copies
    from its neighbours' planes."""
    for r, (planes, up_rows, down_rows) in enumerate(reqs):
        pl = plans[r]
        for i, t in enumerate(planes):
            if up_rows > 0 and pl.up is not None:
                q = plans[pl.up]
                copy_rows(t, pl.own0 - up_rows, reqs[pl.up][0][i], q.own1 - up_rows, up_rows)
            if down_rows > 0 and pl.down is not None:
                q = plans[pl.down]
                copy_rows(t, pl.own1, reqs[pl.down][0][i], q.own0, down_rows)


VOTE = "vote"  # a generator's request (VOTE, word): the maximum of every rank's word, in place, and its value sent back


def _stage_params(defaults, what, params, kw=None):
    """`defaults` overridden from a dict and / or keyword arguments; a name that is not among them is not `what`."""
    prm = dict(defaults)
    for src in (params or {}, kw or {}):
        for name, v in src.items():
            assert name in prm, "%s is not %s" % (name, what)
            prm[name] = v
    return prm


def _run_steps(gen, comm, plan):
    """Drives one rank's *_steps generator to its end and returns its value.  An exchange request (planes, up_rows,
    down_rows) is completed through comm.exchange before the generator goes on, and answered with None; a vote request
    (VOTE, word) goes through comm.allreduce_max, whose value is sent back (TorchComm, NativeComm, NoComm)."""
    answer = None
    try:
        while True:
            req = gen.send(answer)
            if req[0] == VOTE:
                answer = comm.allreduce_max(req[1])
            else:
                comm.exchange(req[0], plan, req[1], req[2])
                answer = None
    except StopIteration as done:
        return done.value


def _run_steps_lockstep(gens, plans, copy_rows):
    """All ranks of a grid inside ONE process (tests, single-GPU rehearsal): the per-rank generators advance in lockstep
    and every rank's value is returned.  Ghost rows are copied directly, copy_rows(dst_plane, d0, src_plane, s0, n); a
    vote is the maximum taken in process and written back to every rank's word."""
    results = [None] * len(gens)
    answer = None
    while True:
        reqs = []
        for r, g in enumerate(gens):
            try:
                reqs.append(g.send(answer))
            except StopIteration as done:
                results[r] = done.value
                reqs.append(None)
        if all(r is None for r in reqs):
            return results
        assert all(r is not None for r in reqs), "ranks left the schedule at different points"
        votes = [r[0] == VOTE for r in reqs]
        assert all(votes) or not any(votes), "ranks left the schedule at different points"
        if votes[0]:
            answer = max(int(r[1][0]) for r in reqs)
            for r in reqs:
                r[1].fill_(answer)
        else:
            _copy_ghost_rows(reqs, plans, copy_rows)
            answer = None


def run_pipeline_lockstep(ops_list, plans, p, bufs_list, copy_rows):
    """All ranks of a grid inside ONE process (tests, single-GPU rehearsal): the per-rank generators
    advance in lockstep and ghost rows are copied directly, copy_rows(dst_plane, d0, src_plane, s0, n)."""
    results = [[] for _ in plans]
    _run_steps_lockstep([pipeline_steps(o, pl, p, b, r) for o, pl, b, r in zip(ops_list, plans, bufs_list, results)],
                        plans, copy_rows)
    return [r[0] for r in results]


# ---- grid hydraulic erosion on row stripes (nz_hydraulic_stripe) ---------------------------------------------------------
HYDRAULIC_STATE = 6  # d, s, fN, fS, fE, fW: state buffers are [6, rows, cols]
HYDRAULIC_SCALARS = ("initialWater", "rain", "evaporation", "capacity", "dissolve", "deposit", "minTilt")
HYDRAULIC_DEFAULTS = dict(iterations=200, initialWater=1e-4, rain=1e-4, evaporation=0.01, capacity=1.0, dissolve=0.3,
                          deposit=0.3, minTilt=0.01, border=N.NZ_HYDRAULIC_BORDER_CLOSED)
HYDRAULIC_PLANES = ("rainMap", "hardness", "wear", "deposits")


def hydraulic_halo_rows(k):
    """Ghost rows on each side that k iterations without an exchange read beyond the owned rows: heights and water at
    radius 3 per iteration."""
    return 3 * k


def hydraulic_params(params=None, **kw):
    """The scalar fields of nz_hydraulic_desc (and `border`) from a dict and / or keyword arguments, the hosts' stage
    defaults for the rest.  The four planes of the desc are per-rank buffers and travel in `bufs`."""
    return _stage_params(HYDRAULIC_DEFAULTS, "a scalar field of nz_hydraulic_desc", params, kw)


def hydraulic_steps(ops, plan, params, bufs, exchange_every=1):
    """Grid hydraulic erosion on one rank's stripe as a generator in the style of pipeline_steps: the iterations run in
    blocks of at most `exchange_every` (split_iterations), every block one ops.hydraulic call that recomputes the ghost
    rows its later iterations need, and before every block it yields (planes, up_rows, down_rows) for the exchange:
      before the first block   the height plane, and the rain and hardness maps when given, 3 * n rows of block n
      before each later block  the height plane and the six state planes, 3 * n rows
    bufs: dict with the height planes "A" (holds the input on its owned rows) and "B", the state buffers "S0" and "S1"
    ([6, rows, cols]), "work" ([7, rows, cols]; needed when exchange_every > 1) and, optionally, the planes "rainMap",
    "hardness" (owned rows filled), "wear", "deposits"; every plane has plan.rows rows with plan.halo >= 3 * exchange_every.
    Returns (height plane, water plane) whose owned rows hold the result."""
    prm = hydraulic_params(params)
    blocks = split_iterations(prm["iterations"], exchange_every)
    planes = {k: bufs.get(k) for k in HYDRAULIC_PLANES}
    cur, nxt = bufs["A"], bufs["B"]
    s_cur, s_nxt = bufs["S0"], bufs["S1"]
    for i, n in enumerate(blocks):
        first, last = i == 0, i == len(blocks) - 1
        rows = hydraulic_halo_rows(n)
        if first:
            yield [cur] + [planes[k] for k in ("rainMap", "hardness") if planes[k] is not None], rows, rows
        else:
            yield [cur] + [s_cur[j] for j in range(HYDRAULIC_STATE)], rows, rows
        ops.hydraulic(cur, nxt, None if first else s_cur, s_nxt, bufs.get("work"), plan, prm, n, first, last, **planes)
        cur, nxt = nxt, cur
        s_cur, s_nxt = s_nxt, s_cur
    return cur, s_cur[0]


def run_hydraulic(ops, comm, plan, params, bufs, exchange_every=1):
    """hydraulic_steps on this rank, every exchange completed before the block that reads it (TorchComm, NativeComm,
    NoComm); returns (height plane, water plane)."""
    return _run_steps(hydraulic_steps(ops, plan, params, bufs, exchange_every), comm, plan)


def run_hydraulic_lockstep(ops_list, plans, params, bufs_list, copy_rows, exchange_every=1):
    """All ranks inside one process, as run_pipeline_lockstep; returns every rank's (height plane, water plane)."""
    gens = [hydraulic_steps(o, pl, params, b, exchange_every) for o, pl, b in zip(ops_list, plans, bufs_list)]
    return _run_steps_lockstep(gens, plans, copy_rows)


# ---- stream-power fluvial erosion on row stripes (nz_fluvial_stripe) ------------------------------------------------------
FLUVIAL_SCALARS = ("erodibility", "uplift", "dt", "rain", "seaLevel")
FLUVIAL_DEFAULTS = dict(iterations=100, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=-3.4028234663852886e38)
FLUVIAL_MAPS = ("rainMap", "hardness", "upliftMap")


def fluvial_halo_rows(k):
    """Ghost rows on each side that k iterations without an exchange read beyond the owned rows: an iteration gathers
    along the receivers of the cells 1 row away, which look at the heights 2 rows away."""
    return 2 * k


def fluvial_params(params=None, **kw):
    """The scalar fields of nz_fluvial_desc from a dict and / or keyword arguments, the hosts' stage defaults for the
    rest.  The maps of the desc are per-rank buffers and travel in `bufs`."""
    return _stage_params(FLUVIAL_DEFAULTS, "a scalar field of nz_fluvial_desc", params, kw)


def fluvial_steps(ops, plan, params, bufs, exchange_every=1):
    """Fluvial erosion on one rank's stripe as a generator in the style of hydraulic_steps: the iterations run in blocks
    of at most `exchange_every` (split_iterations), every block one ops.fluvial call that recomputes the ghost rows its
    later iterations need, and before every block it yields (planes, up_rows, down_rows) for the exchange:
      before the first block   the height plane and, once, the maps that are given, 2 * n rows of block n
      before each later block  the height plane and the drainage plane, 2 * n rows
    The maps are read by every block; split_iterations puts the longest block first, so their one exchange covers the
    later blocks.  bufs: dict with the height planes "A" (holds the input on its owned rows) and
    "B", the drainage planes "D0" and "D1", "work" ([2, rows, cols]; needed when exchange_every > 1) and, optionally,
    "rainMap", "hardness", "upliftMap" (owned rows filled) and "drainageIn" (the drainage to start from, owned rows
    filled; it is exchanged with the heights).  Returns (height plane, drainage plane) whose owned rows hold the result."""
    prm = fluvial_params(params)
    blocks = split_iterations(prm["iterations"], exchange_every) if prm["iterations"] > 0 else []
    maps = {k: bufs.get(k) for k in FLUVIAL_MAPS}
    cur, nxt = bufs["A"], bufs["B"]
    d_cur, d_nxt = bufs.get("drainageIn"), bufs["D0"]
    for i, n in enumerate(blocks):
        rows = fluvial_halo_rows(n)
        if i == 0:
            given = [maps[k] for k in FLUVIAL_MAPS if maps[k] is not None]
            yield [cur] + ([d_cur] if d_cur is not None else []) + given, rows, rows
        else:
            yield [cur, d_cur], rows, rows
        ops.fluvial(cur, nxt, d_cur, d_nxt, bufs.get("work"), plan, prm, n, **maps)
        cur, nxt = nxt, cur
        d_cur, d_nxt = d_nxt, (bufs["D1"] if d_nxt is bufs["D0"] else bufs["D0"])
    return cur, d_cur


def run_fluvial(ops, comm, plan, params, bufs, exchange_every=1):
    """fluvial_steps on this rank, every exchange completed before the block that reads it (TorchComm, NativeComm, NoComm);
    returns (height plane, drainage plane)."""
    return _run_steps(fluvial_steps(ops, plan, params, bufs, exchange_every), comm, plan)


def run_fluvial_lockstep(ops_list, plans, params, bufs_list, copy_rows, exchange_every=1):
    """All ranks inside one process, as run_hydraulic_lockstep; returns every rank's (height plane, drainage plane)."""
    gens = [fluvial_steps(o, pl, params, b, exchange_every) for o, pl, b in zip(ops_list, plans, bufs_list)]
    return _run_steps_lockstep(gens, plans, copy_rows)


# ---- depression filling on row stripes (nz_fill_stripe) -----------------------------------------------------------------
FILL_DEFAULTS = dict(epsilon=1e-4, seaLevel=-3.4028234663852886e38, maxPasses=64, maxRounds=64)


def fill_steps(ops, plan, params, bufs):
    """Depression filling on one rank's stripe as a generator: rounds of ops.fill (at most maxPasses passes over the owned
    rows against one frozen ghost row of W on each side), and between them
      an exchange request (planes, 1, 1)   the height plane before round 0, the W plane before every later round
      a vote request (VOTE, word)          after every round: the driver reduces the int32 word "did my stripe change" to
                                           the maximum over all ranks, in place, and sends its value back
    An exchange request is a 3-tuple of (list, int, int), a vote request a 2-tuple whose first item is VOTE.  The rounds
    stop when the vote is 0 or after maxRounds; round r > 0 is handed the vote of round r - 1 as its `proceed` word, which
    is the form a compiled host enqueues without reading back.  Then ops.fill_finalise with the verdict vote == 0 on every
    rank: all or nothing.  bufs: "H" (the heights on the owned rows; receives the result), "W", "work"
    (nz_fill_stripe_work_floats), "words" (int32[3]) and optionally "depth"; plan.halo >= 1.
    Returns (height plane, depth plane or None, rounds, converged)."""
    prm = _stage_params(FILL_DEFAULTS, "a parameter of the sharded fill", params)
    words = bufs["words"]
    vote, rounds = 1, 0
    while vote != 0 and rounds < prm["maxRounds"]:
        yield [bufs["H"] if rounds == 0 else bufs["W"]], 1, 1
        word = words[rounds & 1:(rounds & 1) + 1]
        ops.fill(bufs["H"], bufs["W"], bufs["work"], plan, prm, rounds == 0,
                 None if rounds == 0 else words[(rounds - 1) & 1:((rounds - 1) & 1) + 1], word)
        vote = yield VOTE, word
        rounds += 1
    words[2:3].fill_(1 if vote == 0 else 0)
    ops.fill_finalise(bufs["H"], bufs["W"], bufs.get("depth"), plan, words[2:3])
    return bufs["H"], bufs.get("depth"), rounds, vote == 0


def run_fill(ops, comm, plan, params, bufs):
    """fill_steps on this rank: exchanges through comm.exchange, votes through comm.allreduce_max (TorchComm, NativeComm,
    NoComm); returns (height plane, depth plane or None, rounds, converged)."""
    return _run_steps(fill_steps(ops, plan, params, bufs), comm, plan)


def run_fill_lockstep(ops_list, plans, params, bufs_list, copy_rows):
    """All ranks inside one process, as run_fluvial_lockstep; a vote is the maximum taken in process and written back to
    every rank's word."""
    return _run_steps_lockstep([fill_steps(o, pl, params, b) for o, pl, b in zip(ops_list, plans, bufs_list)], plans,
                               copy_rows)


# ---- drainage area on row stripes (nz_drainage_stripe_round) --------------------------------------------------------------------
DRAINAGE_DEFAULTS = dict(rain=1.0, seaLevel=-3.4028234663852886e38, maxPasses=64, maxRounds=64)


def drainage_steps(ops, plan, params, bufs):
    """The drainage area on one rank's stripe as a generator like fill_steps: rounds of ops.drainage (at most maxPasses
    passes over the owned rows against one frozen ghost row of A on each side), and between them
      an exchange request (planes, n, n)   before round 0 the height plane -- and the rain map when given -- 2 rows (a
                                           ghost-row cell's receiver looks one row further out); before every later round
                                           the A plane, 1 row
      a vote request (VOTE, word)          after every round, as in fill_steps
    The rounds stop when the vote is 0 or after maxRounds; round r > 0 is handed the vote of round r - 1 as its `proceed`
    word.  Then ops.drainage_finalise with the verdict vote == 0 on every rank: all or nothing.  bufs: "H" (the heights on
    the owned rows; not modified), "A", "work" (nz_drainage_stripe_work_floats), "words" (int32[3]) and optionally
    "rainMap" (owned rows filled); plan.halo >= 2.  Returns (A plane, rounds, converged); the A plane serves as
    bufs["drainageIn"] of fluvial_steps as it stands."""
    prm = _stage_params(DRAINAGE_DEFAULTS, "a parameter of the sharded drainage area", params)
    assert plan.halo >= 2, "the heights need 2 ghost rows"
    words, rain_map = bufs["words"], bufs.get("rainMap")
    maps = dict(rainMap=rain_map) if rain_map is not None else {}
    vote, rounds = 1, 0
    while vote != 0 and rounds < prm["maxRounds"]:
        if rounds == 0:
            yield [bufs["H"]] + ([rain_map] if rain_map is not None else []), 2, 2
        else:
            yield [bufs["A"]], 1, 1
        word = words[rounds & 1:(rounds & 1) + 1]
        ops.drainage(bufs["H"], bufs["A"], bufs["work"], plan, prm, rounds == 0,
                     None if rounds == 0 else words[(rounds - 1) & 1:((rounds - 1) & 1) + 1], word, **maps)
        vote = yield VOTE, word
        rounds += 1
    words[2:3].fill_(1 if vote == 0 else 0)
    ops.drainage_finalise(bufs["A"], plan, prm, words[2:3], **maps)
    return bufs["A"], rounds, vote == 0


def run_drainage(ops, comm, plan, params, bufs):
    """drainage_steps on this rank: exchanges through comm.exchange, votes through comm.allreduce_max (TorchComm,
    NativeComm, NoComm); returns (A plane, rounds, converged)."""
    return _run_steps(drainage_steps(ops, plan, params, bufs), comm, plan)


def run_drainage_lockstep(ops_list, plans, params, bufs_list, copy_rows):
    """All ranks inside one process, as run_fill_lockstep; returns every rank's (A plane, rounds, converged)."""
    return _run_steps_lockstep([drainage_steps(o, pl, params, b) for o, pl, b in zip(ops_list, plans, bufs_list)], plans,
                               copy_rows)


# ---- implicit fluvial erosion on row stripes (nz_implicit_fluvial_stripe_round) -------------------------------------------
FLUVIAL_IMPLICIT_SCALARS = ("erodibility", "uplift", "dt", "seaLevel")
FLUVIAL_IMPLICIT_DEFAULTS = dict(iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0,
                                 seaLevel=-3.4028234663852886e38, maxPasses=64, maxRounds=64)
FLUVIAL_IMPLICIT_MAPS = ("hardness", "upliftMap")


def fluvial_implicit_steps(ops, plan, params, bufs):
    """Implicit fluvial erosion on one rank's stripe as a generator like drainage_steps.  Per iteration:
      the drainage area of the current heights (yield from drainage_steps: rain, seaLevel, maxPasses and maxRounds are
      shared with it); when it does not converge the step is not applied and the loop ends;
      rounds of ops.fluvial_implicit (at most maxPasses passes over the owned rows against one frozen ghost row of h' on
      each side), with an exchange request (planes, 1, 1) before each -- the height plane before round 0, the `out` plane
      before every later round -- and a vote request (VOTE, word) after each; round r > 0 is handed the vote of round
      r - 1 as its `proceed` word; the rounds stop when the vote is 0 or after maxRounds;
      ops.fluvial_implicit_finalise with the verdict vote == 0 on every rank (all or nothing), and the height and `out`
      planes swap; a solve that did not converge ends the loop.
    bufs: "H" (the heights on the owned rows), "out", "A", "work" (nz_implicit_fluvial_stripe_work_floats), "drainageWork"
    (nz_drainage_stripe_work_floats), "words" (int32[3]) and optionally "rainMap", "hardness", "upliftMap" (owned rows
    filled); plan.halo >= 2.  Returns (height plane, A plane, steps applied, rounds of the last solve, converged)."""
    prm = _stage_params(FLUVIAL_IMPLICIT_DEFAULTS, "a parameter of the sharded implicit fluvial erosion", params)
    assert plan.halo >= 2, "the drainage area needs 2 ghost rows of the heights"
    words = bufs["words"]
    maps = {k: bufs[k] for k in FLUVIAL_IMPLICIT_MAPS if bufs.get(k) is not None}
    drain_prm = {k: prm[k] for k in DRAINAGE_DEFAULTS}
    h, out = bufs["H"], bufs["out"]
    steps, rounds, converged = 0, 0, True
    for _ in range(prm["iterations"]):
        dbufs = dict(H=h, A=bufs["A"], work=bufs["drainageWork"], words=words)
        if bufs.get("rainMap") is not None:
            dbufs["rainMap"] = bufs["rainMap"]
        _, _, converged = yield from drainage_steps(ops, plan, drain_prm, dbufs)
        if not converged:
            break
        vote, rounds = 1, 0
        while vote != 0 and rounds < prm["maxRounds"]:
            yield [h if rounds == 0 else out], 1, 1
            word = words[rounds & 1:(rounds & 1) + 1]
            ops.fluvial_implicit(h, bufs["A"], out, bufs["work"], plan, prm, rounds == 0,
                                 None if rounds == 0 else words[(rounds - 1) & 1:((rounds - 1) & 1) + 1], word, **maps)
            vote = yield VOTE, word
            rounds += 1
        converged = vote == 0
        words[2:3].fill_(1 if converged else 0)
        ops.fluvial_implicit_finalise(h, out, plan, words[2:3])
        h, out = out, h
        if not converged:
            break
        steps += 1
    return h, bufs["A"], steps, rounds, converged


def run_fluvial_implicit(ops, comm, plan, params, bufs):
    """fluvial_implicit_steps on this rank: exchanges through comm.exchange, votes through comm.allreduce_max (TorchComm,
    NativeComm, NoComm); returns (height plane, A plane, steps applied, rounds of the last solve, converged)."""
    return _run_steps(fluvial_implicit_steps(ops, plan, params, bufs), comm, plan)


def run_fluvial_implicit_lockstep(ops_list, plans, params, bufs_list, copy_rows):
    """All ranks inside one process, as run_drainage_lockstep; returns every rank's (height plane, A plane, steps applied,
    rounds of the last solve, converged)."""
    return _run_steps_lockstep([fluvial_implicit_steps(o, pl, params, b) for o, pl, b in zip(ops_list, plans, bufs_list)],
                               plans, copy_rows)


class HipStripeOps:
    """Stripe operations on device memory through the C ABI.  Buffers are objects with `.data_ptr()`
    (torch CUDA tensors used as plain HBM allocations); state buffers are indexable by plane."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.lib = N.lib

    def kernel_filter_halo_rows(self, filter, iterations):
        return self.lib.nz_kernel_filter_halo_rows(filter, iterations)

    def kernel_filter_max_fused(self, filter):
        return self.lib.nz_kernel_filter_max_fused(filter)

    def erosion_max_fused(self):
        return self.lib.nz_erosion_max_fused_iterations()

    def _call(self, name, *args):
        N.check(getattr(self.lib, name)(self.ctx._h, *args, 0, None), name)

    def fractal(self, buf, plan, p):
        st = plan.stripe()
        self._call("nz_fractal_stripe", p.noiseType, buf.data_ptr(), C.byref(st), p.hurst, p.startingAmplitude,
                   p.stepdown, p.detuneRate, p.octaves, p.xpos, p.zpos, p.noiseSize)

    def kernel_filter(self, src, dst, plan, filter, T):
        st = plan.stripe()
        self._call("nz_kernel_filter_stripe", src.data_ptr(), dst.data_ptr(), C.byref(st), filter, T)

    def erosion(self, src, dst, plan, E):
        st = plan.stripe()
        self._call("nz_erosion_stripe", src.data_ptr(), dst.data_ptr(), C.byref(st), E)

    def flow_fused_max(self):
        return self.lib.nz_flow_fused_max_iterations()

    def flow_fused(self, h, S_in, S_out, dst, plan, n, first, last, normMin, normMax):
        st = plan.stripe()
        arr = N.dev_ptr * FLOW_PLANES
        pin = arr(*[S_in[i].data_ptr() for i in range(FLOW_PLANES)])
        pout = arr(*[S_out[i].data_ptr() for i in range(FLOW_PLANES)])
        self._call("nz_flow_fused_stripe", h.data_ptr(), pin, pout, dst.data_ptr(), C.byref(st), n, int(first),
                   int(last), normMin, normMax)


    def hydraulic(self, h_in, h_out, S_in, S_out, work, plan, prm, n, first, last, rainMap=None, hardness=None, wear=None,
                  deposits=None, pitch=0):
        """nz_hydraulic_stripe: n iterations of `prm` (hydraulic_params) in one call.  S_in may be None with `first`."""
        st = plan.stripe(pitch)
        arr = N.dev_ptr * HYDRAULIC_STATE
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        pin = arr(*[S_in[i].data_ptr() for i in range(HYDRAULIC_STATE)]) if S_in is not None else None
        pout = arr(*[ptr(S_out[i]) for i in range(HYDRAULIC_STATE)])
        desc = N.HydraulicDesc(n, *[prm[k] for k in HYDRAULIC_SCALARS], prm["border"], ptr(rainMap), ptr(hardness),
                               ptr(wear), ptr(deposits))
        self._call("nz_hydraulic_stripe", h_in.data_ptr(), h_out.data_ptr(), pin, pout, ptr(work), C.byref(st),
                   C.byref(desc), int(first), int(last))

    def fluvial(self, h_in, h_out, d_in, d_out, work, plan, prm, n, rainMap=None, hardness=None, upliftMap=None, pitch=0):
        """nz_fluvial_stripe: n iterations of `prm` (fluvial_params) in one call.  d_in None: the drainage starts at rain_c."""
        st = plan.stripe(pitch)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        desc = N.FluvialDesc(n, *[prm[k] for k in FLUVIAL_SCALARS], ptr(rainMap), ptr(hardness), ptr(upliftMap), ptr(d_in))
        self._call("nz_fluvial_stripe", h_in.data_ptr(), h_out.data_ptr(), d_out.data_ptr(), ptr(work), C.byref(st),
                   C.byref(desc))

    def fill(self, h, w, work, plan, prm, first, proceed, changed, pitch=0):
        """nz_fill_stripe: one round, at most prm["maxPasses"] passes.  proceed: an int32 device word or None; changed: one."""
        st = plan.stripe(pitch)
        desc = N.FillDesc(prm["epsilon"], prm["seaLevel"], prm["maxPasses"], None)
        self._call("nz_fill_stripe", h.data_ptr(), w.data_ptr(), work.data_ptr(), C.byref(st), C.byref(desc), int(first),
                   proceed.data_ptr() if proceed is not None else None, changed.data_ptr())

    def fill_finalise(self, h, w, depth, plan, converged, pitch=0):
        """nz_fill_stripe_finalise on the owned rows, by the int32 device word `converged`."""
        st = plan.stripe(pitch)
        self._call("nz_fill_stripe_finalise", h.data_ptr(), w.data_ptr(), depth.data_ptr() if depth is not None else None,
                   C.byref(st), converged.data_ptr())

    def _drainage_desc(self, prm, rainMap):
        return N.DrainageDesc(prm["rain"], prm["seaLevel"], prm["maxPasses"], rainMap.data_ptr() if rainMap is not None else None)

    def drainage(self, h, a, work, plan, prm, first, proceed, changed, rainMap=None, pitch=0):
        """nz_drainage_stripe_round: one round, at most prm["maxPasses"] passes.  proceed: an int32 device word or None; changed: one."""
        st = plan.stripe(pitch)
        desc = self._drainage_desc(prm, rainMap)
        self._call("nz_drainage_stripe_round", h.data_ptr(), a.data_ptr(), work.data_ptr(), C.byref(st), C.byref(desc), int(first),
                   proceed.data_ptr() if proceed is not None else None, changed.data_ptr())

    def drainage_finalise(self, a, plan, prm, converged, rainMap=None, pitch=0):
        """nz_drainage_stripe_finalise on the owned rows, by the int32 device word `converged`."""
        st = plan.stripe(pitch)
        desc = self._drainage_desc(prm, rainMap)
        self._call("nz_drainage_stripe_finalise", a.data_ptr(), C.byref(st), C.byref(desc), converged.data_ptr())

    def fluvial_implicit(self, h, a, out, work, plan, prm, first, proceed, changed, hardness=None, upliftMap=None, pitch=0):
        """nz_implicit_fluvial_stripe_round: one round, at most prm["maxPasses"] passes.  proceed: an int32 device word or
        None; changed: one."""
        st = plan.stripe(pitch)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        desc = N.FluvialImplicitDesc(*[prm[k] for k in FLUVIAL_IMPLICIT_SCALARS], prm["maxPasses"], ptr(hardness),
                                     ptr(upliftMap), None, None)
        self._call("nz_implicit_fluvial_stripe_round", h.data_ptr(), a.data_ptr(), out.data_ptr(), work.data_ptr(),
                   C.byref(st), C.byref(desc), int(first), ptr(proceed), changed.data_ptr())

    def fluvial_implicit_finalise(self, h, out, plan, converged, pitch=0):
        """nz_implicit_fluvial_stripe_finalise on the owned rows, by the int32 device word `converged`."""
        st = plan.stripe(pitch)
        self._call("nz_implicit_fluvial_stripe_finalise", h.data_ptr(), out.data_ptr(), C.byref(st), converged.data_ptr())

    def upsample_halo_rows(self, filter):
        return self.lib.nz_upsample_stripe_halo_rows(int(filter))

    def upsample(self, src, src_st, dst, dst_st, factor, filter, base=None):
        """nz_upsample_stripe: the owned rows of the fine stripe `dst_st` from the coarse stripe `src_st` (nz_stripe
        structs; the fine grid is `factor` times the coarse one).  base: None, dst itself or a plane apart from it."""
        self._call("nz_upsample_stripe", src.data_ptr(), C.byref(src_st), dst.data_ptr(), C.byref(dst_st), int(factor),
                   int(filter), base.data_ptr() if base is not None else None)

    def downsample(self, src, src_st, dst, dst_st, factor):
        """nz_downsample_stripe: the owned rows of the coarse stripe `dst_st` from the fine stripe `src_st`."""
        self._call("nz_downsample_stripe", src.data_ptr(), C.byref(src_st), dst.data_ptr(), C.byref(dst_st), int(factor))

    def map_range(self, buf, n, res, lim_min=float("inf"), lim_max=float("-inf")):
        """GetMapRangeJob over the first n floats of `buf` into the 3-float device buffer `res`."""
        self._call("nz_get_map_range", buf.data_ptr(), n, res.data_ptr(), lim_min, lim_max)

    def normalize_args(self, buf, plan, args):
        """NormalizeMap on the stripe's owned rows with args = device {min, max, range}."""
        owned = buf.data_ptr() + plan.own0 * plan.cols * 4
        self._call("nz_normalize_cells_dev", owned, plan.nown * plan.cols, args.data_ptr())


class ImplicitFluvialStripe:
    """The compiled hosts' ImplicitFluvialStripe (noize_pipeline.hpp, Stages.cs) under the same name: the scalars and the
    two optional stripe-shaped map planes of the implicit solve, and one round / the finalise of its stripe form on the
    caller's planes and device words -- a thin wrapper over HipStripeOps.fluvial_implicit(_finalise).  The exchanges and the
    votes between the rounds are the caller's: fluvial_implicit_steps is the schedule."""

    def __init__(self, ctx, erodibility=0.05, uplift=0.002, dt=1.0, seaLevel=-3.4028234663852886e38, hardnessRows=None,
                 upliftMapRows=None):
        self.ops = HipStripeOps(ctx)
        self.erodibility, self.uplift, self.dt, self.seaLevel = erodibility, uplift, dt, seaLevel
        self.hardnessRows, self.upliftMapRows = hardnessRows, upliftMapRows

    def ScheduleStripe(self, heightRows, drainageRows, outRows, stripeWork, plan, passes, first, proceed, changed, pitch=0):
        prm = dict(erodibility=self.erodibility, uplift=self.uplift, dt=self.dt, seaLevel=self.seaLevel, maxPasses=passes)
        self.ops.fluvial_implicit(heightRows, drainageRows, outRows, stripeWork, plan, prm, first, proceed, changed,
                                  hardness=self.hardnessRows, upliftMap=self.upliftMapRows, pitch=pitch)

    def FinaliseStripe(self, heightRows, outRows, plan, converged, pitch=0):
        self.ops.fluvial_implicit_finalise(heightRows, outRows, plan, converged, pitch=pitch)


def map_range_work_floats(world):
    return 5 * world + 6


def global_map_range(ops, dist, plane, plan, res, work, lim_min=float("inf"), lim_max=float("-inf")):
    """{min, max, range} of the WHOLE grid in every rank's `res` (3 floats): GetMapRangeJob (Filter/NormalizeJob.cs:17-55)
    over the owned rows of `plane`, one all-gather of the per-rank {min, max, range}, and the same fold over the
    gathered minima and maxima in rank order -- which is the order the monolithic job walks the grid in, so the result
    (down to the sign of a zero extreme) is the monolithic one.  The one collective of the path: data-dependent
    normalisation needs every rank's extremes.  `work` = map_range_work_floats(world) floats on the device of `res`.
    The limits must not be NaN."""
    w = plan.world
    gathered, mins, maxs = work[:3 * w], work[3 * w:4 * w], work[4 * w:5 * w]
    lo, hi = work[5 * w:5 * w + 3], work[5 * w + 3:5 * w + 6]
    ops.map_range(plane[plan.own0:plan.own1], plan.nown * plan.cols, res)
    if dist is not None:  # one rank included: the collective is the same call at every world size
        dist.all_gather_into_tensor(gathered, res)
    else:
        gathered.copy_(res)
    mins.copy_(gathered.view(w, 3)[:, 0])
    maxs.copy_(gathered.view(w, 3)[:, 1])
    ops.map_range(mins, w, lo, lim_min, float("-inf"))
    ops.map_range(maxs, w, hi, float("inf"), lim_max)
    res[0:1].copy_(lo[0:1])
    res[1:2].copy_(hi[1:2])
    res[2:3].copy_(res[1:2] - res[0:1])  # IEEE fp32 subtraction, as `max_ - min_` in the job
    return res


class TorchComm:
    """Neighbour halo exchange with torch.distributed P2P (backend `nccl` = RCCL over xGMI on the GPU
    box, `gloo` in the CPU tests).  Each exchange is one grouped batch: at most two neighbours."""

    def __init__(self, dist, overlap=True):
        self.dist = dist
        self.overlap = overlap  # False: every exchange completes before the launch that follows is enqueued

    def begin(self, planes, plan, up_rows, down_rows):
        """Posts the batch; returns the requests.  On `nccl` the transfers run on the process group's stream behind
        everything already enqueued on the current stream, and finish() makes the current stream wait for them."""
        d = self.dist
        ops = []
        for t in planes:
            if up_rows > 0:  # my top ghost rows <- the rows just above, owned by rank-1
                if plan.down is not None:
                    ops.append(d.P2POp(d.isend, t[plan.own1 - up_rows:plan.own1], plan.down))
                if plan.up is not None:
                    ops.append(d.P2POp(d.irecv, t[plan.own0 - up_rows:plan.own0], plan.up))
            if down_rows > 0:  # my bottom ghost rows <- the rows just below, owned by rank+1
                if plan.up is not None:
                    ops.append(d.P2POp(d.isend, t[plan.own0:plan.own0 + down_rows], plan.up))
                if plan.down is not None:
                    ops.append(d.P2POp(d.irecv, t[plan.own1:plan.own1 + down_rows], plan.down))
        return d.batch_isend_irecv(ops) if ops else []

    def exchange(self, planes, plan, up_rows, down_rows):
        self.finish(self.begin(planes, plan, up_rows, down_rows))

    def finish(self, reqs):
        for req in reqs:
            req.wait()

    def allreduce_max(self, words):
        """The maximum of the int32 tensor `words` over the ranks, in place; returns words[0] on the host."""
        self.dist.all_reduce(words, op=self.dist.ReduceOp.MAX)
        return int(words[0])


class NoComm:
    """world == 1: nothing to exchange (clamp-to-edge at both borders)."""

    def exchange(self, planes, plan, up_rows, down_rows):
        pass

    def allreduce_max(self, words):
        return int(words[0])


# ---- the same schedule behind the C ABI (nz_comm.cpp): what a C# / C++ host calls ----------------------------------------
HALO_MODES = {"recompute": N.NZ_HALO_RECOMPUTE, "exchange": N.NZ_HALO_EXCHANGE, "exchange_once": N.NZ_HALO_EXCHANGE_ONCE}
# record layout of nz_sharded_plan
OP_NOISE, OP_XBEGIN, OP_XFINISH, OP_FILTER, OP_FLOW, OP_EROSION, OP_MARK = 1, 2, 3, 4, 5, 6, 7


def rccl_version():
    v = C.c_int32(0)
    N.check(N.lib.nz_comm_rccl_version(C.byref(v)), "nz_comm_rccl_version")
    return v.value


class NativeComm:
    """nz_comm: an RCCL communicator (ncclCommInitRank) on the context's device plus its own stream.  `unique_id()` is
    made by ONE rank and handed to the others out of band (bench.py broadcasts it through torch.distributed)."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * N.NZ_COMM_ID_BYTES)()
        N.check(N.lib.nz_comm_unique_id(buf), "nz_comm_unique_id")
        return bytes(buf)

    def __init__(self, ctx, uid, rank, world):
        assert len(uid) == N.NZ_COMM_ID_BYTES
        self.ctx = ctx
        h = C.c_void_p()
        buf = (C.c_uint8 * N.NZ_COMM_ID_BYTES).from_buffer_copy(uid)
        N.check(N.lib.nz_comm_init(ctx._h, buf, rank, world, C.byref(h)), "nz_comm_init")
        self._h = h
        self.rank, self.world = rank, world

    def close(self):
        """nz_comm_destroy.  The library refuses while nz_sharded grids still hold the communicator (close them first):
        the status is raised and the handle KEPT, so that a later close() can still reach ncclCommDestroy."""
        if self._h:
            N.check(N.lib.nz_comm_destroy(self._h), "nz_comm_destroy")
            self._h = None

    # the TorchComm interface on top of nz_halo_exchange (one stripe per rank): lets run_pipeline drive the Python schedule
    # over the native exchange
    overlap = True

    def begin(self, planes, plan, up_rows, down_rows):
        arr = (N.dev_ptr * len(planes))(*[t.data_ptr() for t in planes])
        st = plan.stripe()
        N.check(N.lib.nz_halo_exchange_begin(self.ctx._h, self._h, arr, len(planes), C.byref(st), up_rows, down_rows, 0),
                "nz_halo_exchange_begin")
        return True

    def finish(self, reqs):
        N.check(N.lib.nz_halo_exchange_finish(self.ctx._h, self._h, None), "nz_halo_exchange_finish")

    def exchange(self, planes, plan, up_rows, down_rows):
        self.finish(self.begin(planes, plan, up_rows, down_rows))

    def allreduce_max(self, words):
        """nz_comm_allreduce_max_i32 on the int32 device tensor `words`, in place; returns words[0] on the host."""
        N.check(N.lib.nz_comm_allreduce_max_i32(self.ctx._h, self._h, words.data_ptr(), words.numel(), 0, None),
                "nz_comm_allreduce_max_i32")
        return int(words[0])

    def allgather_range(self, map_ptr, n_floats, res_ptr, lim_min=float("inf"), lim_max=float("-inf")):
        N.check(N.lib.nz_comm_allgather_range(self.ctx._h, self._h, map_ptr, n_floats, res_ptr, lim_min, lim_max, 0, None),
                "nz_comm_allgather_range")


def terrain_params(p):
    """PipelineParams -> nz_terrain_params."""
    return N.TerrainParams(p.noiseType, p.hurst, p.startingAmplitude, p.stepdown, p.detuneRate, p.octaves, p.noiseSize,
                           p.filter, p.gaussIterations, p.flowIterations, p.normMin, p.normMax, p.erosionIterations)


class ShardedGrid:
    """nz_sharded: the stock stage list on a grows x cols grid cut into `stripes` row stripes over all ranks of `comm`
    (None: one rank, device copies instead of RCCL).  The library owns the planes and the launch plan; `run()` replays
    it (one C call per pass)."""

    def __init__(self, ctx, comm, grows, cols, p, stripes=None, overlap=0, external_source=False, as_rank=None):
        world = comm.world if comm is not None else 1
        if as_rank is not None:
            world = as_rank[1]
        self.ctx, self.comm, self.p = ctx, comm, p
        # overlap: 0 = exchanges on the compute stream itself; 1 / True = interior rows first, border rows after the wait;
        # 2 = border rows first, the exchange for the next launch travels while the interior runs
        self.desc = N.ShardedDesc(grows, cols, stripes if stripes is not None else world, HALO_MODES[p.haloMode],
                                  int(overlap), p.xpos, p.zpos, int(bool(external_source)),
                                  as_rank[0] if as_rank is not None else 0, as_rank[1] if as_rank is not None else 0)
        self.tp = terrain_params(p)
        h = C.c_void_p()
        # ctx None: a plan-only object (no planes, cannot run): the launch plan of rank as_rank[0] of as_rank[1]
        N.check(N.lib.nz_sharded_create(ctx._h if ctx is not None else None, comm._h if comm is not None else None,
                                        C.byref(self.desc), C.byref(self.tp), C.byref(h)), "nz_sharded_create")
        self._h = h
        self.local_stripes = N.lib.nz_sharded_local_stripes(h)

    def close(self):
        if self._h:
            N.lib.nz_sharded_destroy(self._h)
            self._h = None

    def stripe(self, i):
        """(nz_stripe, source plane address, result plane address) of local stripe i."""
        st, src, res = N.Stripe(), N.dev_ptr(), N.dev_ptr()
        N.check(N.lib.nz_sharded_stripe(self._h, i, C.byref(st), C.byref(src), C.byref(res)), "nz_sharded_stripe")
        return st, src.value, res.value

    def plan(self):
        """The compiled plan as tuples (op, stripe, n, a, b, own0, own1, planes) -- see include/noize_hip.h."""
        n = C.c_int32(0)
        N.check(N.lib.nz_sharded_plan(self._h, None, 0, C.byref(n)), "nz_sharded_plan")
        rec = (C.c_int32 * (8 * n.value))()
        N.check(N.lib.nz_sharded_plan(self._h, rec, n.value, C.byref(n)), "nz_sharded_plan")
        return [tuple(rec[8 * i:8 * i + 8]) for i in range(n.value)]

    def transfers(self):
        """The exchanges' transfers in the order this rank posts them: tuples (exchange, source rank, destination rank,
        floats).  On a plan-only object: the lists of rank as_rank[0] of the real as_rank[1]-rank job."""
        n = C.c_int32(0)
        N.check(N.lib.nz_sharded_transfers(self._h, None, 0, C.byref(n)), "nz_sharded_transfers")
        rec = (C.c_int32 * (4 * max(1, n.value)))()
        N.check(N.lib.nz_sharded_transfers(self._h, rec, n.value, C.byref(n)), "nz_sharded_transfers")
        return [tuple(rec[4 * i:4 * i + 4]) for i in range(n.value)]

    def run(self, marks=False, dep=0):
        """One pass (enqueue only).  marks: also return the five stage-boundary handles."""
        from .runtime import JobHandle
        out = N.handle_t(0)
        if marks:
            m = (N.handle_t * 5)()
            N.check(N.lib.nz_sharded_pipeline(self.ctx._h, self._h, m, dep, C.byref(out)), "nz_sharded_pipeline")
            return JobHandle(self.ctx, out.value), [JobHandle(self.ctx, v) for v in m]
        N.check(N.lib.nz_sharded_pipeline(self.ctx._h, self._h, None, dep, C.byref(out)), "nz_sharded_pipeline")
        return JobHandle(self.ctx, out.value)

    def traffic(self):
        n, b = C.c_int32(0), C.c_size_t(0)
        N.check(N.lib.nz_sharded_traffic(self._h, C.byref(n), C.byref(b)), "nz_sharded_traffic")
        return n.value, b.value

    def set_timing(self, on):
        N.check(N.lib.nz_sharded_set_timing(self._h, int(bool(on))), "nz_sharded_set_timing")

    def exchange_ms(self):
        ms = C.c_float(0)
        N.check(N.lib.nz_sharded_exchange_ms(self._h, C.byref(ms)), "nz_sharded_exchange_ms")
        return ms.value

    def map_range(self, res_ptr, lim_min=float("inf"), lim_max=float("-inf")):
        N.check(N.lib.nz_sharded_map_range(self.ctx._h, self._h, res_ptr, lim_min, lim_max, 0, None), "nz_sharded_map_range")

    def normalize(self, args_ptr):
        N.check(N.lib.nz_sharded_normalize(self.ctx._h, self._h, args_ptr, 0, None), "nz_sharded_normalize")

    def owned_rows(self, i):
        """Host copy of local stripe i's result rows: (first global row, array [rows, cols])."""
        import numpy as np
        st, _, res = self.stripe(i)
        n = (st.own1 - st.own0) * st.cols
        out = np.empty(n, np.float32)
        N.check(N.lib.nz_tile_download(self.ctx._h, res + st.own0 * st.cols * 4, out.ctypes.data, n, 0, None), "download")
        self.ctx.synchronize()
        return st.grow0 + st.own0, out.reshape(st.own1 - st.own0, st.cols)


class _PlanRecorder:
    """A stripe-ops object that launches nothing: it writes down what pipeline_steps asks for, in the record layout of
    nz_sharded_plan -- the Python schedule as the specification the native plan is checked against."""

    def __init__(self, lib=None):
        self.lib = lib or N.lib
        self.records = []
        self.ids = {}

    def kernel_filter_halo_rows(self, filter, iterations):
        return self.lib.nz_kernel_filter_halo_rows(filter, iterations)

    def kernel_filter_max_fused(self, filter):
        return self.lib.nz_kernel_filter_max_fused(filter)

    def erosion_max_fused(self):
        return self.lib.nz_erosion_max_fused_iterations()

    def flow_fused_max(self):
        return self.lib.nz_flow_fused_max_iterations()

    def _id(self, buf):
        return self.ids[id(buf)]

    def fractal(self, buf, plan, p):
        if plan.own1 > plan.own0:
            self.records.append((OP_NOISE, 0, 0, 0, plan.own0, plan.own1, self._id(buf) | (self._id(buf) << 8)))

    def kernel_filter(self, src, dst, plan, filter, T):
        if plan.own1 > plan.own0:
            self.records.append((OP_FILTER, T, 0, 0, plan.own0, plan.own1, self._id(src) | (self._id(dst) << 8)))

    def erosion(self, src, dst, plan, E):
        if plan.own1 > plan.own0:
            self.records.append((OP_EROSION, E, 0, 0, plan.own0, plan.own1, self._id(src) | (self._id(dst) << 8)))

    def flow_fused(self, h, S_in, S_out, dst, plan, n, first, last, normMin, normMax):
        if plan.own1 > plan.own0:
            self.records.append((OP_FLOW, n, int(first), int(last), plan.own0, plan.own1,
                                 self._id(h) | (self._id(dst) << 8) | (self._id(S_in) << 16) | (self._id(S_out) << 24)))


class _Named:
    def __init__(self, planes=None):
        self.planes = planes

    def __getitem__(self, k):
        return self.planes[k]


def python_plan(rank, world, grows, cols, p, overlap=True):
    """What pipeline_steps does for stripe `rank` of `world`, as records (op, n, a, b, own0, own1, planes) comparable with
    ShardedGrid.plan() (whose records also carry the local stripe index)."""
    rec = _PlanRecorder()
    halo = halo_rows_needed(rec, p)
    plan = StripePlan(rank, world, grows, cols, halo, neighbours_own_halo=p.haloMode != "recompute")
    A, B = _Named(), _Named()
    S0, S1 = _Named([_Named() for _ in range(FLOW_PLANES)]), _Named([_Named() for _ in range(FLOW_PLANES)])
    rec.ids = {id(A): 0, id(B): 1, id(S0): 0, id(S1): 1}
    first_plane = {id(A): 0, id(B): 1}
    for k in range(FLOW_PLANES):
        first_plane[id(S0[k])] = 2 + k
        first_plane[id(S1[k])] = 7 + k
    marks = {"noise": 0, "gauss": 1, "flow": 2, "erosion": 3, "end": 4}
    result = []
    gen = pipeline_steps(rec, plan, p, (A, B, S0, S1), result,
                         on_stage=lambda name: rec.records.append((OP_MARK, marks[name], 0, 0, 0, 0, 0)))
    try:
        req = next(gen)
        while True:
            if req == ("finish",):
                rec.records.append((OP_XFINISH, 0, 0, 0, 0, 0, 0))
                req = next(gen)
                continue
            planes, up_rows, down_rows = req
            rec.records.append((OP_XBEGIN, len(planes), up_rows, down_rows, 0, 0, first_plane[id(planes[0])]))
            if overlap:
                req = gen.send("async")
            else:
                rec.records.append((OP_XFINISH, 0, 0, 0, 0, 0, 0))
                req = next(gen)
    except StopIteration:
        pass
    return rec.records, rec.ids[id(result[0])], plan
