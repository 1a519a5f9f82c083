"""Fluvial erosion on row stripes on the GPU (nz_fluvial_stripe, HipStripeOps.fluvial, run_fluvial_lockstep) against
tests/fluvial_ref.py, bit for bit in heights and drainage: one stripe is the model on a rectangle, as one call and as calls
that carry the drainage; a square stripe is nz_fluvial_erosion; a pitch leaves the pad floats and the rows outside the
widened window alone; the stripes of a grid equal the whole grid, down to stripes thinner than the kernel's 16-row tile;
the float modes agree; refusals write nothing.  Every buffer starts as NaN, so a ghost row that nobody filled shows in the
result."""
import ctypes as C

import numpy as np
import pytest
import torch

import fluvial_ref as F
from fluvial_stripe_cases import (CASES, ITS, MAPS, NAMES, PARAMS, assert_bits, assert_run, gather, lockstep, options,
                                  reference, sharded_params, stripe_bufs, terrain)
from test_gpu_fluvial import run_gpu

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def hip(nj):
    """(sharded module, HipStripeOps) on a context that shares torch's stream: the buffers are torch CUDA tensors."""
    from noize_job_amd import sharded as sh
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tctx = nj.Context(0, stream=stream.cuda_stream)
        yield sh, sh.HipStripeOps(tctx)
        stream.synchronize()
        tctx.close()


def one_stripe(hip, h, its, prm, opts, carry=False, pitch=None, ops=None):
    """The whole rows x cols grid as one stripe: one call of `its` iterations, or (carry) `its` calls of one iteration that
    hand the drainage on.  -> ([heights, drainage], bufs)"""
    sh, default_ops = hip
    ops = ops or default_ops
    plan = sh.StripePlan(0, 1, h.shape[0], h.shape[1], 0)
    assert (plan.rows, plan.own0, plan.own1, plan.grow0) == (h.shape[0], 0, h.shape[0], 0)
    bufs = stripe_bufs(plan, h, opts, 1 if carry else its, "cuda", pitch)
    prm = sharded_params(its, prm)
    maps = {k: bufs.get(k) for k in MAPS}
    if carry:
        cur, nxt, d_cur, d_nxt = bufs["A"], bufs["B"], None, bufs["D0"]
        for _ in range(its):
            ops.fluvial(cur, nxt, d_cur, d_nxt, None, plan, prm, 1, pitch=pitch or 0, **maps)
            cur, nxt = nxt, cur
            d_cur, d_nxt = d_nxt, (bufs["D1"] if d_nxt is bufs["D0"] else bufs["D0"])
        res = (cur, d_cur)
    else:
        ops.fluvial(bufs["A"], bufs["B"], None, bufs["D0"], bufs["work"], plan, prm, its, pitch=pitch or 0, **maps)
        res = (bufs["B"], bufs["D0"])
    return gather([plan], [res]), bufs


# 1. one stripe is the model on a rectangle: partial tiles in both directions (4-byte path: 333 columns), one tile column and
# a width of 200 (16-byte path); one call and carried drainage
@pytest.mark.parametrize("with_maps", [False, True])
@pytest.mark.parametrize("shape", [(70, 333), (333, 200), (64, 64)])
def test_one_stripe_is_the_model_on_a_rectangle(hip, shape, with_maps):
    h = terrain(*shape)
    opts = options(with_maps, shape)
    for k in range(2):
        for its in (1, 2, ITS):
            want = F.run(h, its, **dict(zip(NAMES, PARAMS[k])), **opts) if its != ITS else reference(*shape, ITS, k, with_maps)
            for carry in (False, True):
                got, _ = one_stripe(hip, h, its, PARAMS[k], opts, carry)
                assert_run(got, want, "%s maps %s params %d its %d carry %s" % (shape, with_maps, k, its, carry))


# ... and on a square it is nz_fluvial_erosion, device against device
@pytest.mark.parametrize("with_maps", [False, True])
def test_a_square_stripe_is_the_tile_entry(hip, nj, ctx, with_maps):
    shape = (160, 160)
    h = terrain(*shape)
    opts = options(with_maps, shape)
    for k in range(2):
        want = run_gpu(nj, ctx, h, ITS, PARAMS[k], **{n: v for n, v in opts.items() if v is not None})
        got, _ = one_stripe(hip, h, ITS, PARAMS[k], opts)
        assert_run(got, want, "maps %s params %d" % (with_maps, k))
        assert_run(got, reference(*shape, ITS, k, with_maps), "maps %s params %d: reference" % (with_maps, k))


# 2. a pitch on every plane: the same results, and neither the pad floats nor the rows outside the first launch's widened
# window are written.  Rank 1 of 3 with two ghost rows more than a call of 3 iterations reads.  pitch = cols + 5 takes the
# 4-byte path, cols + 8 the 16-byte one.
@pytest.mark.parametrize("with_maps", [False, True])
@pytest.mark.parametrize("pad", [5, 8])
def test_pitch_and_rows_outside_the_window_keep_their_guard(hip, pad, with_maps):
    sh, ops = hip
    shape = rows, cols = (333, 200)
    n, spare, pitch = 3, 2, cols + pad
    h = terrain(rows, cols)
    opts = options(with_maps, shape)
    want = F.run(h, n, **dict(zip(NAMES, PARAMS[1])), **opts)
    got_1, _ = one_stripe(hip, h, n, PARAMS[1], opts, pitch=pitch)
    assert_run(got_1, want, "one stripe with a pitch")
    plan = sh.StripePlan(1, 3, rows, cols, sh.fluvial_halo_rows(n) + spare)
    bufs = stripe_bufs(plan, h, opts, n, "cuda", pitch)
    # the ghost rows the call reads, straight from the grid: 2 * n rows, the spare rows stay NaN
    lo, hi = plan.own0 - 2 * n, plan.own1 + 2 * n
    for name, a in [("A", h)] + [(m, opts[m]) for m in MAPS]:
        if a is not None:
            bufs[name][lo:hi, :cols] = torch.from_numpy(np.ascontiguousarray(a[plan.grow0 + lo:plan.grow0 + hi])).cuda()
    ops.fluvial(bufs["A"], bufs["B"], None, bufs["D0"], bufs["work"], plan, sharded_params(n, PARAMS[1]), n, pitch=pitch,
                **{m: bufs.get(m) for m in MAPS})
    got = gather([plan], [(bufs["B"], bufs["D0"])])
    own = slice(plan.g0, plan.g0 + plan.nown)
    assert_run(got, [w[own] for w in want], "rank 1 of 3 with a pitch")
    w0, w1 = plan.own0 - 2 * (n - 1), plan.own1 + 2 * (n - 1)  # the first launch's window
    for i, t in enumerate([bufs["B"], bufs["D0"], bufs["work"][0], bufs["work"][1]]):
        t = t.cpu().numpy()
        assert np.isnan(t[:, cols:]).all(), "plane %d: pad floats" % i
        assert np.isnan(t[:w0]).all() and np.isnan(t[w1:]).all(), "plane %d: rows outside the window" % i
    assert np.isnan(bufs["D1"].cpu().numpy()).all()
    # the inputs are not modified
    assert_bits(bufs["A"].cpu().numpy()[lo:hi, :cols], h[plan.grow0 + lo:plan.grow0 + hi], "height_in")
    assert np.isnan(bufs["A"].cpu().numpy()[:lo]).all() and np.isnan(bufs["A"].cpu().numpy()[hi:]).all()


# 3. the stripes of a grid equal the whole grid: the reference and the one-stripe run.  Parameter set 1 has a sea level
@pytest.mark.parametrize("with_maps", [False, True])
@pytest.mark.parametrize("shape,world,exchange_every", CASES)
def test_stripes_equal_the_whole_grid(hip, shape, world, exchange_every, with_maps):
    sh, ops = hip
    h = terrain(*shape)
    opts = options(with_maps, shape)
    for k in range(2):
        got = lockstep(sh, ops, world, exchange_every, h, ITS, PARAMS[k], opts, "cuda")
        assert_run(got, reference(*shape, ITS, k, with_maps), "world %d params %d" % (world, k))
        one, _ = one_stripe(hip, h, ITS, PARAMS[k], opts)
        assert_run(got, one, "world %d params %d: one stripe" % (world, k))


# 4. strict arithmetic in every float mode
def test_float_modes_give_the_same_bits(hip, nj):
    sh, _ = hip
    shape = (70, 333)
    h = terrain(*shape)
    opts = options(True, shape)
    want = reference(*shape, ITS, 1, True)
    for mode in (1, 2):
        mctx = nj.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        try:
            mctx.float_mode = mode
            ops = sh.HipStripeOps(mctx)
            got, _ = one_stripe(hip, h, ITS, PARAMS[1], opts, ops=ops)
            assert_run(got, want, "float mode %d: one stripe" % mode)
            got = lockstep(sh, ops, 8, 2, h, ITS, PARAMS[1], opts, "cuda")
            assert_run(got, want, "float mode %d: 8 stripes" % mode)
            torch.cuda.current_stream().synchronize()
        finally:
            mctx.close()


# 5. refusals: NZ_ERR_INVALID, and no output plane is touched
def test_refusals_write_nothing(hip, nj):
    sh, ops = hip
    N = nj._native
    rows, cols = 40, 48
    h = terrain(rows, cols)
    hh = np.tile(h, (3, 1))
    opts = {k: np.tile(v, (3, 1)) for k, v in options(True, (rows, cols)).items()}
    plan = sh.StripePlan(1, 3, 3 * rows, cols, 4)  # 4 ghost rows: enough for 2 iterations
    assert plan.nown == rows
    bufs = stripe_bufs(plan, hh, opts, 2, "cuda")
    for name, a in [("A", hh)] + list(opts.items()):
        bufs[name][:] = torch.from_numpy(np.ascontiguousarray(a[plan.grow0:plan.grow0 + plan.rows])).cuda()
    st = plan.stripe()
    good = list(PARAMS[0])
    A, B, D, W = (bufs[k].data_ptr() for k in ("A", "B", "D0", "work"))

    def desc(n, prm=good, rain=bufs["rainMap"].data_ptr(), drainage_in=None):
        return N.FluvialDesc(n, *prm, rain, bufs["hardness"].data_ptr(), bufs["upliftMap"].data_ptr(), drainage_in)

    def refused(name, h_in, h_out, d_out, work, stripe, d):
        with pytest.raises(nj.NoizeError) as e:
            ops.ctx.call("nz_fluvial_stripe", h_in, h_out, d_out, work, C.byref(stripe), d if d is None else C.byref(d))
        assert e.value.status == N.NZ_ERR_INVALID and name in str(e.value), (name, str(e.value))

    refused("ghost rows", A, B, D, W, st, desc(3))               # 6 ghost rows needed, 4 in the buffer
    refused("iterations", A, B, D, W, st, desc(0))
    refused("iterations", A, B, D, W, st, desc(-2))
    refused("desc", A, B, D, W, st, None)
    refused("height_out", A, A + 4 * cols, D, W, st, desc(2))    # height_out overlaps height_in
    refused("drainage_out", A, B, B + 4 * cols, W, st, desc(2))  # the two output planes overlap
    refused("drainageIn", A, B, D, W, st, desc(2, drainage_in=D + 4 * 8))
    refused("rainMap", A, B, D, W, st, desc(2, rain=W + 4 * 100))  # a map overlaps work
    refused("work", A, B, D, None, st, desc(2))
    refused("drainage_out", A, B, None, W, st, desc(2))
    bad = list(good)
    bad[2] = float("nan")
    refused("dt", A, B, D, W, st, desc(2, prm=bad))
    bad = list(good)
    bad[0] = -0.5
    refused("erodibility", A, B, D, W, st, desc(2, prm=bad))
    narrow = plan.stripe()
    narrow.pitch = cols - 1
    refused("pitch", A, B, D, W, narrow, desc(2))
    torch.cuda.current_stream().synchronize()
    for name in ("B", "D0", "D1", "work"):
        assert np.isnan(bufs[name].cpu().numpy()).all(), name
    # ... and the same arguments put right run
    ops.ctx.call("nz_fluvial_stripe", A, B, D, W, C.byref(st), C.byref(desc(2)))
    want = F.run(hh, 2, **dict(zip(NAMES, good)), **opts)
    got = gather([plan], [(bufs["B"], bufs["D0"])])
    own = slice(plan.g0, plan.g0 + plan.nown)
    assert_run(got, [w[own] for w in want], "after the refusals")
    assert N.lib.nz_fluvial_stripe_halo_rows(4) == 8 == sh.fluvial_halo_rows(4)
    assert N.lib.nz_fluvial_stripe_work_floats(C.byref(st), 1) == 0
    assert N.lib.nz_fluvial_stripe_work_floats(C.byref(st), 2) == 2 * plan.rows * cols
