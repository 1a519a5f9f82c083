"""Fluvial erosion on row stripes, the schedule on the CPU: fluvial_steps / run_fluvial / run_fluvial_lockstep of
noize_job_amd.sharded driven with the numpy reference as compute back end (tests/fluvial_stripe_ops.py) equal
fluvial_ref.run on the whole grid bit for bit in heights and drainage -- in one process and over `gloo`; the same input
tells a halo of 1 row per iteration from the 2 the model needs; the exchanges are the ones documented."""
import os

import numpy as np
import pytest
import torch

import fluvial_ref as F
from conftest import ROOT
from fluvial_stripe_cases import (CASES, ITS, PARAM_SETS, PARAMS, assert_run, count_differing, gather, lockstep, options,
                                  reference, sharded_params, stripe_bufs, terrain)


# 1. all ranks in one process: the stripes equal the whole grid
@pytest.mark.parametrize("with_maps", [False, True])
@pytest.mark.parametrize("shape,world,exchange_every", CASES)
def test_lockstep_equals_the_whole_grid(shape, world, exchange_every, with_maps):
    from fluvial_stripe_ops import FluvialStripeOps
    from noize_job_amd import sharded as sh
    h = terrain(*shape)
    for k in PARAM_SETS:
        got = lockstep(sh, FluvialStripeOps(), world, exchange_every, h, ITS, PARAMS[k], options(with_maps, shape))
        assert_run(got, reference(*shape, ITS, k, with_maps), "world %d every %d params %d" % (world, exchange_every, k))


# 2. negative control: with 1 ghost row per iteration the cut, which the reference takes for a border of outlets, reaches
# the owned rows: the row next to the cut gathers no drainage across it and sees no receiver beyond it
@pytest.mark.parametrize("world,exchange_every", [(2, 1), (3, 2), (8, 1), (8, 4)])
def test_a_short_halo_is_noticed(world, exchange_every):
    from fluvial_stripe_ops import FluvialStripeOps
    from noize_job_amd import sharded as sh
    shape = (70, 97)
    got = lockstep(sh, FluvialStripeOps(ghost=1), world, exchange_every, terrain(*shape), ITS, PARAMS[0],
                   options(False, shape))
    n = count_differing(got, reference(*shape, ITS, 0, False))
    print("world %d every %d: %d values differ" % (world, exchange_every, n))
    assert n > 0


# 3. the same over gloo: run_fluvial with TorchComm, one process per rank
def _worker(rank, world, port, shape, exchange_every, with_maps, k, out_path):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from fluvial_stripe_ops import FluvialStripeOps
    from noize_job_amd import sharded as sh
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    plan = sh.StripePlan(rank, world, shape[0], shape[1], sh.fluvial_halo_rows(exchange_every))
    bufs = stripe_bufs(plan, terrain(*shape), options(with_maps, shape), exchange_every)
    res = sh.run_fluvial(FluvialStripeOps(), sh.TorchComm(dist), plan, sharded_params(ITS, PARAMS[k]), bufs,
                         exchange_every=exchange_every)
    parts = [None] * world
    dist.all_gather_object(parts, (plan.g0, gather([plan], [res])))
    if rank == 0:
        parts.sort(key=lambda t: t[0])
        np.savez(out_path, heights=np.concatenate([p[0] for _, p in parts], axis=0),
                 drainage=np.concatenate([p[1] for _, p in parts], axis=0))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_ranks_equal_the_whole_grid(tmp_path):
    from test_sharded_cpu import _spawn
    shape, world, exchange_every = (70, 333), 3, 2
    out = str(tmp_path / "fluvial.npz")
    _spawn(_worker, world, lambda port: (world, port, shape, exchange_every, True, 1, out))
    got = np.load(out)
    assert_run([got["heights"], got["drainage"]], reference(*shape, ITS, 1, True), "gloo world %d" % world)


# 4. one rank: NoComm, nothing to exchange; the drainage of one run carried into the next
def test_one_rank_with_nocomm_and_a_carried_drainage():
    from fluvial_stripe_ops import FluvialStripeOps
    from noize_job_amd import sharded as sh
    shape = (70, 333)
    plan = sh.StripePlan(0, 1, shape[0], shape[1], sh.fluvial_halo_rows(4))
    bufs = stripe_bufs(plan, terrain(*shape), options(True, shape), 4)
    h, a = sh.run_fluvial(FluvialStripeOps(), sh.NoComm(), plan, sharded_params(4, PARAMS[1]), bufs, exchange_every=4)
    bufs2 = dict(bufs, A=h.clone(), drainageIn=a.clone())
    res = sh.run_fluvial(FluvialStripeOps(), sh.NoComm(), plan, sharded_params(ITS - 4, PARAMS[1]), bufs2, exchange_every=4)
    assert_run(gather([plan], [res]), reference(*shape, ITS, 1, True), "one rank, 4 + 3 iterations")


# 5. the exchanges: the height and the maps before the first block, height and drainage before every later one, 2 rows
# per iteration of the block
def test_steps_ask_for_the_documented_ghost_rows():
    from noize_job_amd import sharded as sh
    assert [sh.fluvial_halo_rows(k) for k in (0, 1, 2, 5)] == [0, 2, 4, 10]
    calls = []

    class Rec:
        def fluvial(self, h_in, h_out, d_in, d_out, work, plan, prm, n, **maps):
            calls.append((h_in, h_out, d_in, d_out, work, n, maps))

    for with_maps in (False, True):
        calls.clear()
        bufs = dict(A="A", B="B", D0="D0", D1="D1", work="W")
        if with_maps:
            bufs.update(rainMap="R", upliftMap="U")
        plan = sh.StripePlan(1, 3, 90, 8, sh.fluvial_halo_rows(3))
        gen = sh.fluvial_steps(Rec(), plan, dict(iterations=7, rain=2.0), bufs, exchange_every=3)
        reqs = []
        try:
            while True:
                reqs.append(next(gen))
        except StopIteration as done:
            result = done.value
        assert reqs == [(["A"] + (["R", "U"] if with_maps else []), 6, 6), (["B", "D0"], 4, 4), (["A", "D1"], 4, 4)]
        assert [c[:6] for c in calls] == [("A", "B", None, "D0", "W", 3), ("B", "A", "D0", "D1", "W", 2),
                                          ("A", "B", "D1", "D0", "W", 2)]
        assert all(c[6] == dict(rainMap="R" if with_maps else None, hardness=None, upliftMap="U" if with_maps else None)
                   for c in calls)
        assert result == ("B", "D0")
    prm = sh.fluvial_params(dict(iterations=3), rain=2.0)
    assert (prm["iterations"], prm["rain"], prm["erodibility"], prm["seaLevel"]) == (3, 2.0, 0.05, float(F.SEA_OFF))
    with pytest.raises(AssertionError):
        sh.fluvial_params(iteration=3)
