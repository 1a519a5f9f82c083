"""The stripe sweep shared by tests/test_sweep_stripes_ref.py (CPU, the numpy stripe ops) and tests/test_gpu_sweep_stripes.py
(nz_hydraulic_stripe, nz_fluvial_stripe, nz_fill_stripe(_finalise), nz_drainage_stripe_round(_finalise),
nz_implicit_fluvial_stripe_round(_finalise)): a square adversarial
tile of tests/terrain_tiles.py cut into row stripes and driven by the run_*_lockstep functions of noize_job_amd.sharded has to
equal the whole tile's model bit for bit, in every plane the family returns.

    tiles     every tile of T.TIES, `zeros` and `tiny`: tests/test_terrain_tiles.py shows that each of them has equal heights
              (tiny: heights a subnormal amount apart) across every cut below, straight or diagonal -- so a receiver on a
              first or last owned row is chosen among equal drops of which some lie in a ghost row, a `<=` against a sea
              level that is a cell value decides ghost cells, and flats without a receiver span the cuts
    splits    (65, 3): cuts at rows 22 and 44; (65, 8): stripes of 8 and 9 rows, thinner than the 16-row kernel tile;
              (130, 3): cuts at rows 44 and 87, inside kernel tiles
    pitch     terraces16 at 67 over 3 ranks, every plane with a pitch of 72 floats and NaN in the pads (the numpy ops know
              no pitch: the CPU half runs this case dense)
    families  hydraulic   PARAMS[0] closed without maps and PARAMS[1] open with both maps, masks recorded in both; 6
                          iterations, an exchange every 1 and every 2 iterations
              fluvial     the stage's defaults without maps and a sea level that is a cell value with the three maps; 6
                          iterations, an exchange every 1 and every 2
              fill        epsilon 0, 1e-4, 0.25 with and without a sea level that is a cell value, depth recorded
              drainage    the tile as it is (pits and flats) and flooded with 1e-4; unit rain, a sea with fractional
                          rain on a positive map, the same on a map of both signs; the maps cut into stripes
              fluvial_implicit  the tile as it is (pits, plateaus, flats that span the cuts) through
                          run_fluvial_implicit_lockstep, drainage rounds and solve rounds on the same stripes: the stage's
                          defaults at dt 200 in 1 iteration; a sea level that is a cell value with the hardness and uplift
                          maps of fluvial_implicit_stripe_cases at dt 50 in 2 iterations, the second on heights the first
                          solve wrote and finalise swapped.  Heights and the last iteration's drainage area against
                          fluvial_implicit_ref.chain; in the first set the area is integral and sums to res * res over
                          the cells without a receiver, with no model asked
A stripe has to hold the ghost rows its neighbour asks for, 2 * exchange_every <= rows // world in the drivers' tests: the
thinnest stripes here have 8 rows, so no exchange_every 2 case is dropped (every_for() returns (1, 2) for every split).

The whole-grid models are the tile models through test_gpu_sweep_terrain.model, under the tile sweep's keys: where the
parameters coincide they are computed once for both sweeps; the implicit family's chain is kept under a key of the same kind.
Budgets: FILL_BUDGET (test_gpu_fill_stripe.PARAMS), drainage_stripe_cases.PARAMS and, for the implicit family,
fluvial_implicit_stripe_cases.PARAMS -- 128 passes and 128 rounds, which its driver shares with the drainage rounds; the CPU
half asserts that every case converges inside them.  The implicit family through the numpy ops, all nine tiles at the three
splits and the pitched case dense: at most 7 rounds of a solve (tiny, 65^2 over 8, the first set) and 66 Jacobi steps in one
round (manh_pit, 130^2 over 3), every case well under a second."""
import numpy as np

import drainage_stripe_cases as DC
import fill_stripe_cases as LC
import fluvial_implicit_ref as R
import fluvial_implicit_stripe_cases as IC
import fluvial_ref as F
import fluvial_stripe_cases as FC
import terrain_tiles as T
import test_gpu_sweep_terrain as S
import test_hydraulic_stripe_ref as HC
from test_hydraulic_ref import PARAMS as HYDRAULIC_PARAMS

OFF = S.OFF
TILES = tuple(T.TIES) + ("zeros", "tiny")
SPLITS = ((65, 3), (65, 8), (130, 3))
PITCHED = ("terraces16", 67, 3, 72)  # tile, size, world, pitch
ITS = 6
FILL_BUDGET = dict(maxPasses=400, maxRounds=400)
DRAINAGE_BUDGET = DC.PARAMS
FLUVIAL_IMPLICIT_BUDGET = IC.PARAMS  # shared by the drainage rounds and the solve rounds of an iteration
HYDRAULIC_SETS = ((0, ()), (1, S.ALL_ON))  # (index into PARAMS, options of the _ex entry)
FILL_EPS = (0.0, 1e-4, 0.25)
FLOOD_EPS = 1e-4


def every_for(rows, world):
    return tuple(e for e in (1, 2) if 2 * e <= rows // world)


class Backend:
    """Where a case runs: the sharded module, one ops object per family, the device of the buffers and (GPU) the package
    that sizes the work planes."""

    def __init__(self, sh, ops, device="cpu", nj=None):
        self.sh, self.ops, self.device, self.nj = sh, ops, device, nj

    def pitch(self, pitch):
        return pitch if self.nj is not None else None

    def work_floats(self, module, pitch):
        return module.work_floats(self.nj, pitch or 0) if self.nj is not None else (lambda plan: 0)

    def drain_floats(self, module, pitch):
        """The drainage rounds' work plane of a family that runs them before its own."""
        return module.drain_floats(self.nj, pitch or 0) if self.nj is not None else (lambda plan: 0)


def cpu_backend():
    from drainage_stripe_ops import DrainageStripeOps
    from fill_stripe_ops import FillStripeOps
    from fluvial_implicit_stripe_ops import FluvialImplicitStripeOps
    from fluvial_stripe_ops import FluvialStripeOps
    from hydraulic_stripe_ops import HydraulicStripeOps
    from noize_job_amd import sharded as sh
    return Backend(sh, dict(hydraulic=HydraulicStripeOps(), fluvial=FluvialStripeOps(), fill=FillStripeOps(),
                            drainage=DrainageStripeOps(), fluvial_implicit=FluvialImplicitStripeOps()))


def gpu_backend(nj, sh, ops):
    return Backend(sh, dict.fromkeys(("hydraulic", "fluvial", "fill", "drainage", "fluvial_implicit"), ops), "cuda", nj)


class Pitched:
    """HipStripeOps with `pitch` added to every stripe call: the drivers know no pitch, the entries do."""

    def __init__(self, ops, pitch):
        self.ops, self.pitch = ops, pitch

    def __getattr__(self, name):
        entry = getattr(self.ops, name)
        return lambda *args, **kw: entry(*args, pitch=self.pitch, **kw)


def assert_pads(bufs_list, cols, pitch, what):
    """Every plane of every rank keeps the NaN of its pad floats."""
    for rank, bufs in enumerate(bufs_list):
        for name, t in bufs.items():
            if t is not None and t.is_floating_point() and t.ndim >= 2 and t.shape[-1] == pitch:
                assert bool(t[..., cols:].isnan().all()), "%s: rank %d: pad floats of %s" % (what, rank, name)


def first(m):
    return np.array(m[0]) if m is not None else None


def tile(name, res):
    """The tile sweep's tile (shared, read only), as a copy that torch may wrap."""
    return np.array(S.tile(name, res))


# ---- one family on one tile and split: every parameter set -----------------------------------------------------------------------
def hydraulic(be, name, res, world, pitch=None):
    h, pitch = tile(name, res), be.pitch(pitch)
    sh, ops = be.sh, be.ops["hydraulic"]
    for k, on in HYDRAULIC_SETS:
        prm = HYDRAULIC_PARAMS[k]
        c = S.case("hydraulic_ex", h, its=ITS, prm=prm, on=on, keys=[name])
        want = [w[0] for w in S.model(c)]
        o = c["opts"]
        opts = dict(border=o["border"], rainMap=first(o["rainMap"]), hardness=first(o["hardness"]), masks=True)
        for every in every_for(res, world):
            what = "hydraulic %s %d^2 over %d, params %d on %r, every %d, pitch %s" % (name, res, world, k, on, every, pitch)
            if pitch is None:
                got = HC.lockstep(sh, ops, world, every, h, ITS, prm, opts, be.device)
            else:
                plans = [sh.StripePlan(r, world, res, res, sh.hydraulic_halo_rows(every)) for r in range(world)]
                bufs = [HC.stripe_bufs(sh, pl, h, opts, every, be.device, pitch) for pl in plans]
                out = sh.run_hydraulic_lockstep([Pitched(ops, pitch)] * world, plans, HC.sharded_params(ITS, prm, opts["border"]),
                                                bufs, HC.copy_rows, exchange_every=every)
                got = HC.gather(plans, out, bufs, True)
                assert_pads(bufs, res, pitch, what)
            HC.assert_run(got, want, True, what)


def fluvial_sets(h):
    return (((0.05, 0.002, 1.0, 1.0, OFF), ()), ((0.2, 0.0, 0.5, 0.25, T.sea_at(h, 0.3)), FC.MAPS))


def fluvial(be, name, res, world, pitch=None):
    h, pitch = tile(name, res), be.pitch(pitch)
    sh, ops = be.sh, be.ops["fluvial"]
    for prm, on in fluvial_sets(h):
        c = S.case("fluvial", h, its=ITS, prm=prm, on=on, keys=[name])
        want = [w[0] for w in S.model(c)]
        opts = {m: c["maps"][m][0] if m in c["maps"] else None for m in FC.MAPS}
        for every in every_for(res, world):
            what = "fluvial %s %d^2 over %d, prm %r on %r, every %d, pitch %s" % (name, res, world, prm, on, every, pitch)
            if pitch is None:
                got = FC.lockstep(sh, ops, world, every, h, ITS, prm, opts, be.device)
            else:
                plans = [sh.StripePlan(r, world, res, res, sh.fluvial_halo_rows(every)) for r in range(world)]
                bufs = [FC.stripe_bufs(pl, h, opts, every, be.device, pitch) for pl in plans]
                out = sh.run_fluvial_lockstep([Pitched(ops, pitch)] * world, plans, FC.sharded_params(ITS, prm), bufs,
                                              HC.copy_rows, exchange_every=every)
                got = FC.gather(plans, out)
                assert_pads(bufs, res, pitch, what)
            FC.assert_run(got, want, what)


def fill(be, name, res, world, pitch=None):
    """-> the rounds of every case, for the tests that print them."""
    h, pitch = tile(name, res), be.pitch(pitch)
    sh, ops = be.sh, be.ops["fill"]
    sized = be.work_floats(LC, pitch)
    rounds_of = []
    for eps in FILL_EPS:
        for sea in (OFF, T.sea_at(h, 0.3)):
            what = "fill %s %d^2 over %d, eps %g sea %r, pitch %s" % (name, res, world, eps, sea, pitch)
            want, want_depth = [w[0] for w in S.model(S.case("fill", h, eps=eps, sea=sea, keys=[name]))]
            params = dict(FILL_BUDGET, epsilon=eps, seaLevel=sea)
            if pitch is None:
                got, depth, rounds, converged, _, _ = LC.lockstep(sh, ops, world, h, params, sized, be.device)
            else:
                plans = [sh.StripePlan(r, world, res, res, 1) for r in range(world)]
                bufs = [LC.stripe_bufs(pl, h, sized(pl), be.device, pitch) for pl in plans]
                out = sh.run_fill_lockstep([Pitched(ops, pitch)] * world, plans, params, bufs, HC.copy_rows)
                assert len({(r[2], r[3]) for r in out}) == 1, "%s: the ranks disagree about rounds / converged" % what
                got, depth = FC.gather(plans, out)
                rounds, converged = out[0][2], out[0][3]
                assert_pads(bufs, res, pitch, what)
            assert converged and 1 <= rounds <= FILL_BUDGET["maxRounds"], (what, rounds, converged)
            assert np.isfinite(want).all() and np.isfinite(want_depth).all(), what
            LC.assert_bits(got, want, what + ": heights")
            LC.assert_bits(depth, want_depth, what + ": depth")
            rounds_of.append(rounds)
    return rounds_of


def drainage_planes(name, res):
    """(key, heights) of the tile as it is and of the tile flooded with FLOOD_EPS (the tile sweep's flood)."""
    h = tile(name, res)
    flooded = np.array(S.model(S.case("fill", h, eps=FLOOD_EPS, keys=[name]))[0][0])
    return ((name, h), ((name, "flooded", FLOOD_EPS), flooded))


def drainage(be, name, res, world, pitch=None):
    pitch = be.pitch(pitch)
    sh, ops = be.sh, be.ops["drainage"]
    sized = be.work_floats(DC, pitch)
    rounds_of = []
    for key, h in drainage_planes(name, res):
        sea = T.sea_at(h, 0.3)
        for kw in (dict(), dict(rain=0.75, sea=sea, on=("rainMap",)), dict(rain=0.3, sea=sea, on=("rainMap",), signed=True)):
            c = S.case("drainage", h, keys=[key], **kw)
            what = "%s over %d, plane %r, pitch %s" % (S.describe(c), world, key, pitch)
            want = S.model(c)[0][0]
            rm = first(c["maps"].get("rainMap"))
            params = dict(DRAINAGE_BUDGET, rain=c["rain"], seaLevel=c["sea"])
            if pitch is None:
                got, rounds, converged, _, _ = DC.lockstep(sh, ops, world, h, params, sized, be.device, rain_map=rm)
            else:
                plans = [sh.StripePlan(r, world, res, res, DC.HALO) for r in range(world)]
                bufs = [DC.stripe_bufs(pl, h, sized(pl), be.device, pitch, rm) for pl in plans]
                out = sh.run_drainage_lockstep([Pitched(ops, pitch)] * world, plans, params, bufs, HC.copy_rows)
                assert len({(r[1], r[2]) for r in out}) == 1, "%s: the ranks disagree about rounds / converged" % what
                got = np.concatenate([r[0][pl.own0:pl.own1, :pl.cols].cpu().numpy() for r, pl in zip(out, plans)])
                rounds, converged = out[0][1], out[0][2]
                assert_pads(bufs, res, pitch, what)
            assert converged and 2 <= rounds <= DRAINAGE_BUDGET["maxRounds"], (what, rounds, converged)
            assert np.isfinite(want).all(), what
            DC.assert_bits(got, want, what)
            if not kw:  # unit rain: every cell's rain arrives at exactly one cell without a receiver
                roots = F.receivers(h)[0] == F.NONE
                assert (got == np.floor(got)).all() and float(got[roots].astype(np.float64).sum()) == res * res, what
            rounds_of.append(rounds)
    return rounds_of


def fluvial_implicit_sets(h):
    """(scalars, iterations, maps?) of the two parameter sets."""
    return ((dict(dt=200.0), 1, False), (dict(dt=50.0, seaLevel=T.sea_at(h, 0.3)), 2, True))


def fluvial_implicit(be, name, res, world, pitch=None):
    """The tile as it is -- pits, plateaus and flats that span the cuts -- through run_fluvial_implicit_lockstep: drainage
    rounds, then solve rounds, per iteration on the same stripes.  -> the rounds of the last solve of every case."""
    h, pitch = tile(name, res), be.pitch(pitch)
    sh, ops = be.sh, be.ops["fluvial_implicit"]
    sized, drain_sized = be.work_floats(IC, pitch), be.drain_floats(IC, pitch)
    rounds_of = []
    for k, (scalars, iterations, mapped) in enumerate(fluvial_implicit_sets(h)):
        maps = dict(hardness=IC.hard_map(h.shape), upliftMap=IC.uplift_map(h.shape)) if mapped else {}
        what = "fluvial_implicit %s %d^2 over %d, set %d %r x %d maps %r, pitch %s" % (
            name, res, world, k + 1, scalars, iterations, mapped, pitch)
        want, want_a = S.memo(("terrain", "fluvial_implicit chain", name, res, iterations, tuple(sorted(scalars.items())), mapped),
                              lambda: R.chain(h, iterations, **scalars, **maps))
        params = dict(FLUVIAL_IMPLICIT_BUDGET, iterations=iterations, **scalars)
        if pitch is None:
            got, A, steps, rounds, converged, _, _ = IC.lockstep(sh, ops, world, h, params, sized, drain_sized, be.device, **maps)
        else:
            plans = [sh.StripePlan(r, world, res, res, IC.HALO) for r in range(world)]
            bufs = [IC.stripe_bufs(pl, h, sized(pl), drain_sized(pl), be.device, pitch, **maps) for pl in plans]
            out = sh.run_fluvial_implicit_lockstep([Pitched(ops, pitch)] * world, plans, params, bufs, HC.copy_rows)
            assert len({r[2:] for r in out}) == 1, "%s: the ranks disagree about steps / rounds / converged" % what
            got, A = FC.gather(plans, out)
            steps, rounds, converged = out[0][2:]
            assert_pads(bufs, res, pitch, what)
        assert converged and steps == iterations and 1 <= rounds <= FLUVIAL_IMPLICIT_BUDGET["maxRounds"], (
            what, steps, rounds, converged)
        assert np.isfinite(want).all() and np.isfinite(want_a).all(), what
        IC.assert_bits(A, want_a, what + ": the drainage area of the last iteration")
        IC.assert_bits(got, want, what + ": heights")
        if k == 0:  # unit rain, one iteration: every cell's rain arrives at exactly one cell without a receiver
            roots = F.receivers(h)[0] == F.NONE
            assert (A == np.floor(A)).all() and float(A[roots].astype(np.float64).sum()) == res * res, what
        rounds_of.append(rounds)
    return rounds_of


FAMILIES = dict(hydraulic=hydraulic, fluvial=fluvial, fill=fill, drainage=drainage, fluvial_implicit=fluvial_implicit)
CASES = [(name, res, world) for name in TILES for res, world in SPLITS]
