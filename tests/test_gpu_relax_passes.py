"""The pass counts of the iterate-to-rest series (nz_fill_depressions*, nz_fill_stripe, nz_drainage_area, nz_watershed,
nz_stream_order), pinned exactly.
Result bits cannot show a broken tile skip or series gate (csrc/nz_relax_pass.hpp): a series that skips too little, or
notices rest one pass late, ends in the same floats more slowly.  The count is deterministic -- no launch has a race, the
ring of a tile is frozen during its sweeps and barriers separate the phases -- so it is an integer to compare, not a time
to bound.  tests/golden/relax_passes.json holds what the series took before the protocol moved into its own header, and what the
watershed and stream-order series took before their mask kernels, launchers and host drivers were shared; `measure` is
what recorded either table, on the commit its key names.
The counts are now also derived: tests/relax_schedule.py is the protocol and the tile schedule in numpy,
tests/test_relax_schedule.py finds every single-call entry of the table with it on the CPU, and
tests/test_gpu_relax_schedule.py holds all seven series to it."""
import json
import os

import numpy as np
import pytest
import torch

import test_gpu_drainage as TD
import test_gpu_fill as TF
import test_gpu_stream_order as TS
import test_gpu_watershed as TW
from conftest import GOLDEN
from fill_stripe_cases import EPS as STRIPE_EPS
from fill_stripe_cases import grid, lockstep, stripe_ops, work_floats
from test_hydraulic_ref import relief

pytestmark = pytest.mark.gpu
f32 = np.float32
FILL_TILES = ("bowl160", "fbm97", "rand130", "const65")
EPS = (0.0, 1e-4)
CAPS = (1, 3, 16)
AMPLE = 20000  # passes: a launch behind the series' rest returns at once
PARAMS = dict(epsilon=STRIPE_EPS, maxPasses=400, maxRounds=400)  # the budget of tests/test_gpu_fill_stripe.py


class Recording:
    """HipStripeOps that notes, after every round, (rank, the round's `changed` word, the passes the round ran)."""

    def __init__(self, ops):
        self.ops, self.rounds = ops, []

    def __getattr__(self, name):
        return getattr(self.ops, name)

    def fill(self, h, w, work, plan, prm, first, proceed, changed, pitch=0):
        self.ops.fill(h, w, work, plan, prm, first, proceed, changed, pitch=pitch)
        self.rounds.append([plan.rank, int(changed[0]), int(work[:1].view(torch.int32)[0])])


def measure(nj, ctx, hip):
    got = {}
    for name in FILL_TILES:
        for eps in EPS:
            _, _, passes, conv = TF.run_gpu(nj, ctx, TF.tile(name), eps)
            assert conv == 1
            got["fill %s eps %g" % (name, eps)] = passes
    batch = np.stack([relief(48), (relief(48, 170) * f32(3.0)).astype(f32), TF.tile("rand130")[:48, :48].copy()])
    for eps in EPS:
        _, _, passes, conv = TF.run_gpu(nj, ctx, batch, eps, form="batch")
        assert conv == 1
        got["fill batch 3x48 eps %g" % eps] = passes
    h, _, height = TD.serpentine()
    _, passes, conv = TD.run_gpu(nj, ctx, h, budget=height + 2)
    assert conv == 1
    got["drainage serpentine160"] = passes
    filled, _, _, conv = TF.run_gpu(nj, ctx, TD.tile(130), 1e-4)
    assert conv == 1
    lib = nj._native.lib
    try:
        for cap in CAPS:
            lib.nz_debug_drainage_sweeps(cap)
            _, passes, conv = TD.run_gpu(nj, ctx, filled, 0.75, budget=AMPLE, rm=TD.rain_map(130))
            assert conv == 1
            got["drainage filled fbm130 rain map cap %d" % cap] = passes
    finally:
        lib.nz_debug_drainage_sweeps(0)
    h, _, _, hops = TW.serpentine()
    _, _, _, passes, conv = TW.run_gpu(nj, ctx, h, budget=int(hops.max()) + 2)
    assert conv == 1
    got["watershed serpentine160"] = passes
    for which, (h, dr, _, _, chain) in enumerate(TS.long_tiles()):
        _, _, passes, conv = TS.run_gpu(nj, ctx, h, TS.OFF, dr, 0.5, budget=chain + 2)
        assert conv == 1
        got["stream order long chain %d" % which] = passes
    area, _, conv = TD.run_gpu(nj, ctx, filled, budget=AMPLE)
    assert conv == 1
    try:
        for cap in CAPS:
            lib.nz_debug_watershed_sweeps(cap)
            _, _, _, passes, conv = TW.run_gpu(nj, ctx, filled, budget=AMPLE, length=True)
            assert conv == 1
            got["watershed filled fbm130 length cap %d" % cap] = passes
            lib.nz_debug_stream_order_sweeps(cap)
            _, _, passes, conv = TS.run_gpu(nj, ctx, filled, TS.OFF, area, 8.0, budget=AMPLE, links=True)
            assert conv == 1
            got["stream order filled fbm130 drainage threshold 8 links cap %d" % cap] = passes
    finally:
        lib.nz_debug_watershed_sweeps(0)
        lib.nz_debug_stream_order_sweeps(0)
    sh, ops = hip
    rec = Recording(ops)
    _, _, rounds, converged, _, _ = lockstep(sh, rec, 2, grid("bowl"), PARAMS, work_floats(nj), "cuda")
    assert converged
    got["fill stripes bowl world 2"] = {"rounds": rounds, "rank, changed, passes of every round": rec.rounds}
    return got


def test_pass_counts_are_the_recorded_ones(nj, ctx):
    with open(os.path.join(GOLDEN, "relax_passes.json")) as f:
        table = json.load(f)
    want = dict(table["passes"], **table["passes on 0da72c4"])
    with stripe_ops(nj) as hip:
        got = measure(nj, ctx, hip)
    print(json.dumps(got))
    assert got == want
