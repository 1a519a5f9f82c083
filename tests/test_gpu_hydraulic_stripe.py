"""Grid hydraulic erosion on row stripes on the GPU (nz_hydraulic_stripe, HipStripeOps.hydraulic, run_hydraulic_lockstep)
against tests/hydraulic_ex_ref.py, bit for bit: one stripe is the model on a rectangle, as one call and as calls that carry
the state; a pitch leaves the pad floats and the rows outside the widened window alone; the stripes of a grid equal the
whole grid, down to stripes thinner than the kernel's 16-row tile; the float modes agree; refusals write nothing.
Every buffer starts as NaN, so a ghost row that nobody filled shows in the result."""
import ctypes as C

import numpy as np
import pytest
import torch

import hydraulic_ex_ref as X
from test_gpu_hydraulic import assert_bits
from test_gpu_hydraulic_ex import option_sets, run_ex
from test_hydraulic_ref import NAMES, PARAMS
from test_hydraulic_stripe_ref import GRID, ITS, WORLDS, assert_run, gather, lockstep, sharded_params, stripe_bufs, terrain

pytestmark = pytest.mark.gpu
f32 = np.float32
OPTIONS = ["off", "open", "rain", "hardness", "masks", "all"]
_refs = {}


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


def opts_for(option, shape):
    """test_gpu_hydraulic_ex's option sets in the form of test_hydraulic_stripe_ref.options, plus "off"."""
    o = option_sets(shape)[option] if option != "off" else {}
    return dict(border=o.get("border", X.CLOSED), rainMap=o.get("rainMap"), hardness=o.get("hardness"),
                masks=bool(o.get("masks")))


def ref_for(shape, its, k, option):
    key = (shape, its, k, option)
    if key not in _refs:
        o = opts_for(option, shape)
        _refs[key] = X.run(terrain(*shape), its, border=o["border"], rainMap=o["rainMap"], hardness=o["hardness"],
                           **dict(zip(NAMES, PARAMS[k])))
    return _refs[key]


def one_stripe(hip, h, its, prm, opts, carry=False, pitch=None, ops=None):
    """The whole rows x cols grid as one stripe: one call of `its` iterations with first and last set, or (carry) `its`
    calls of one iteration that hand the state on.  -> (result, water, wear, deposits)."""
    sh, default_ops = hip
    ops = ops or default_ops
    plan = sh.StripePlan(0, 1, h.shape[0], h.shape[1], 0)
    assert (plan.rows, plan.own0, plan.own1, plan.grow0) == (h.shape[0], 0, h.shape[0], 0)
    bufs = stripe_bufs(sh, plan, h, opts, 1 if carry else its, "cuda", pitch)
    prm = sharded_params(its, prm, opts["border"])
    planes = {k: bufs.get(k) for k in sh.HYDRAULIC_PLANES}
    if carry:
        cur, nxt, s_cur, s_nxt = bufs["A"], bufs["B"], bufs["S0"], bufs["S1"]
        for it in range(its):
            ops.hydraulic(cur, nxt, None if it == 0 else s_cur, s_nxt, None, plan, prm, 1, it == 0, it == its - 1,
                          pitch=pitch or 0, **planes)
            cur, nxt, s_cur, s_nxt = nxt, cur, s_nxt, s_cur
        res = (cur, s_cur[0])
    else:
        ops.hydraulic(bufs["A"], bufs["B"], None, bufs["S1"], bufs["work"], plan, prm, its, True, True, pitch=pitch or 0,
                      **planes)
        res = (bufs["B"], bufs["S1"][0])
    return gather([plan], [res], [bufs], opts["masks"]), bufs


# 1. one stripe is the model on a rectangle: partial tiles in both directions, one tile column; one call and carried state
@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("shape", [(70, 333), (333, 200), (64, 64)])
def test_one_stripe_is_the_model_on_a_rectangle(hip, oracle, shape, option):
    h = terrain(*shape)
    opts = opts_for(option, shape)
    for k in range(2):
        for its in (1, 2, 7):
            want = ref_for(shape, its, k, option)
            for carry in (False, True):
                got, _ = one_stripe(hip, h, its, PARAMS[k], opts, carry)
                assert_run(got, want, opts["masks"], "%s %s params %d its %d carry %s" % (shape, option, k, its, carry))


# ... and on a square it is nz_hydraulic_erosion_ex, device against device
@pytest.mark.parametrize("option", OPTIONS)
def test_a_square_stripe_is_the_tile_entry(hip, nj, ctx, oracle, option):
    shape = (160, 160)
    h = terrain(*shape)
    opts = opts_for(option, shape)
    for k in range(2):
        want = run_ex(nj, ctx, h, ITS, PARAMS[k], **opts)
        got, _ = one_stripe(hip, h, ITS, PARAMS[k], opts)
        assert_run(got, want, opts["masks"], "%s params %d" % (option, k))
        assert_run(got, ref_for(shape, ITS, k, option), opts["masks"], "%s params %d: reference" % (option, k))


# 2. pitch = cols + 5 on every plane: the same results, and neither the pad floats nor the rows outside the first launch's
# widened window are written.  Rank 1 of 3 with two ghost rows more than a call of 2 iterations reads.
@pytest.mark.parametrize("option", ["off", "all"])
def test_pitch_and_rows_outside_the_window_keep_their_guard(hip, oracle, option):
    sh, ops = hip
    rows, cols = GRID
    n, spare, pitch = 2, 2, cols + 5
    h = terrain(rows, cols)
    opts = opts_for(option, GRID)
    got_1, _ = one_stripe(hip, h, n, PARAMS[1], opts, pitch=pitch)
    want = ref_for(GRID, n, 1, option)
    assert_run(got_1, want, opts["masks"], "one stripe with a pitch")
    plan = sh.StripePlan(1, 3, rows, cols, sh.hydraulic_halo_rows(n) + spare)
    bufs = stripe_bufs(sh, plan, h, opts, n, "cuda", pitch)
    # the ghost rows the call reads, straight from the grid: 3 * n rows, the spare rows stay NaN
    lo, hi = plan.own0 - 3 * n, plan.own1 + 3 * n
    for name, a in (("A", h), ("rainMap", opts["rainMap"]), ("hardness", opts["hardness"])):
        if a is not None:
            bufs[name][lo:hi, :cols] = torch.from_numpy(np.ascontiguousarray(a[plan.grow0 + lo:plan.grow0 + hi])).cuda()
    planes = {k: bufs.get(k) for k in sh.HYDRAULIC_PLANES}
    ops.hydraulic(bufs["A"], bufs["B"], None, bufs["S1"], bufs["work"], plan, sharded_params(n, PARAMS[1], opts["border"]), n,
                  True, True, pitch=pitch, **planes)
    got = gather([plan], [(bufs["B"], bufs["S1"][0])], [bufs], opts["masks"])
    own = slice(plan.g0, plan.g0 + plan.nown)
    assert_run(got, [w[own] for w in want], opts["masks"], "rank 1 of 3 with a pitch")
    w0, w1 = plan.own0 - 3 * (n - 1), plan.own1 + 3 * (n - 1)  # the first launch's window
    written = [bufs["B"]] + [bufs["S1"][i] for i in range(6)] + [bufs["work"][i] for i in range(7)]
    for i, t in enumerate(written):
        t = t.cpu().numpy()
        assert np.isnan(t[:, cols:]).all(), "plane %d: pad floats" % i
        assert np.isnan(t[:w0]).all() and np.isnan(t[w1:]).all(), "plane %d: rows outside the window" % i
    assert np.isfinite(bufs["B"].cpu().numpy()[plan.own0:plan.own1, :cols]).all()
    if opts["masks"]:
        for name in ("wear", "deposits"):
            t = bufs[name].cpu().numpy()
            assert np.isnan(t[:, cols:]).all() and np.isnan(t[:plan.own0]).all() and np.isnan(t[plan.own1:]).all(), name
    # the inputs are not modified
    assert_bits(bufs["A"].cpu().numpy()[lo:hi, :cols], h[plan.grow0 + lo:plan.grow0 + hi], "height_in")


# 3. the stripes of a grid equal the whole grid: the reference and the one-stripe run; 70 rows over 8 ranks are stripes of 8
# and 9 rows, thinner than the 16-row tile
@pytest.mark.parametrize("option", ["off", "all"])
@pytest.mark.parametrize("shape,world,exchange_every", [(GRID, w, e) for w, e in WORLDS] + [((70, 333), 8, 2)])
def test_stripes_equal_the_whole_grid(hip, oracle, shape, world, exchange_every, option):
    sh, ops = hip
    h = terrain(*shape)
    opts = opts_for(option, shape)
    for k in range(2):
        got = lockstep(sh, ops, world, exchange_every, h, ITS, PARAMS[k], opts, "cuda")
        assert_run(got, ref_for(shape, ITS, k, option), opts["masks"], "world %d params %d" % (world, k))
        one, _ = one_stripe(hip, h, ITS, PARAMS[k], opts)
        assert_run(got, one, opts["masks"], "world %d params %d: one stripe" % (world, k))


# 4. strict arithmetic in every float mode
def test_float_modes_give_the_same_bits(hip, nj, oracle):
    sh, _ = hip
    shape = (70, 333)
    h = terrain(*shape)
    opts = opts_for("all", shape)
    want = ref_for(shape, ITS, 1, "all")
    for mode in (1, 2):
        mctx = nj.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        try:
            mctx.float_mode = mode
            ops = sh.HipStripeOps(mctx)
            got, _ = one_stripe(hip, h, ITS, PARAMS[1], opts, ops=ops)
            assert_run(got, want, True, "float mode %d: one stripe" % mode)
            got = lockstep(sh, ops, 8, 2, h, ITS, PARAMS[1], opts, "cuda")
            assert_run(got, want, True, "float mode %d: 8 stripes" % mode)
            torch.cuda.current_stream().synchronize()
        finally:
            mctx.close()


# 5. refusals: NZ_ERR_INVALID, and no output plane is touched
def test_refusals_write_nothing(hip, nj, oracle):
    sh, ops = hip
    N = nj._native
    rows, cols = 40, 48
    h = terrain(rows, cols)
    opts = opts_for("all", (rows, cols))
    plan = sh.StripePlan(1, 3, 3 * rows, cols, 6)  # 6 ghost rows: enough for 2 iterations
    assert plan.nown == rows
    hh = np.tile(h, (3, 1))
    big_opts = dict(opts, rainMap=np.tile(opts["rainMap"], (3, 1)), hardness=np.tile(opts["hardness"], (3, 1)))
    bufs = stripe_bufs(sh, plan, hh, big_opts, 2, "cuda")
    for name, a in (("A", hh), ("rainMap", big_opts["rainMap"]), ("hardness", big_opts["hardness"])):
        bufs[name][:] = torch.from_numpy(np.ascontiguousarray(a[plan.grow0:plan.grow0 + plan.rows])).cuda()
    arr = N.dev_ptr * 6
    s_in, s_out = arr(*[bufs["S0"][i].data_ptr() for i in range(6)]), arr(*[bufs["S1"][i].data_ptr() for i in range(6)])
    st = plan.stripe()
    good = list(PARAMS[0])

    def desc(n, prm=good, wear=bufs["wear"].data_ptr(), deposits=bufs["deposits"].data_ptr()):
        return N.HydraulicDesc(n, *prm, 1, bufs["rainMap"].data_ptr(), bufs["hardness"].data_ptr(), wear, deposits)

    def refused(name, h_in, h_out, sin, sout, work, stripe, d, first, last):
        with pytest.raises(nj.NoizeError) as e:
            ops.ctx.call("nz_hydraulic_stripe", h_in, h_out, sin, sout, work, C.byref(stripe), C.byref(d), first, last)
        assert e.value.status == N.NZ_ERR_INVALID and name in str(e.value), (name, str(e.value))

    A, B, W = bufs["A"].data_ptr(), bufs["B"].data_ptr(), bufs["work"].data_ptr()
    refused("ghost rows", A, B, None, s_out, W, st, desc(3), 1, 1)           # 9 ghost rows needed, 6 in the buffer
    refused("iterations", A, B, None, s_out, W, st, desc(0), 1, 1)
    refused("iterations", A, B, None, s_out, W, st, desc(-2), 1, 1)
    refused("state_in", A, B, None, s_out, W, st, desc(2), 0, 1)
    refused("height_out", A, A + 4 * cols, None, s_out, W, st, desc(2), 1, 1)  # height_out overlaps height_in
    refused("work", A, B, None, s_out, W, st, desc(2, wear=W + 4 * 100), 1, 1)  # a mask overlaps work
    refused("work", A, B, None, s_out, None, st, desc(2), 1, 1)
    refused("state_out", A, B, None, arr(*([bufs["S1"][0].data_ptr()] + [None] * 5)), W, st, desc(2), 1, 1)
    refused("state_in", A, B, s_out, s_out, W, st, desc(2), 0, 0)               # state_out overlaps state_in
    bad = list(good)
    bad[4] = 1.5
    refused("dissolve", A, B, None, s_out, W, st, desc(2, prm=bad), 1, 1)
    torch.cuda.current_stream().synchronize()
    for name in ("B", "S1", "work", "wear", "deposits"):
        assert np.isnan(bufs[name].cpu().numpy()).all(), name
    # ... and the same arguments put right run
    ops.ctx.call("nz_hydraulic_stripe", A, B, None, s_out, W, C.byref(st), C.byref(desc(2)), 1, 1)
    want = X.run(hh, 2, border=X.OPEN, rainMap=big_opts["rainMap"], hardness=big_opts["hardness"], **dict(zip(NAMES, good)))
    got = gather([plan], [(bufs["B"], bufs["S1"][0])], [bufs], True)
    own = slice(plan.g0, plan.g0 + plan.nown)
    assert_run(got, [w[own] for w in want], True, "after the refusals")
    assert N.lib.nz_hydraulic_stripe_halo_rows(4) == 12 == sh.hydraulic_halo_rows(4)
    assert N.lib.nz_hydraulic_stripe_work_floats(C.byref(st), 1) == 0
    assert N.lib.nz_hydraulic_stripe_work_floats(C.byref(st), 2) == 7 * plan.rows * cols
