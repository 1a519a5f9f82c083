"""The GPU side of tests/test_gpu_chain_plan.py: one case per process, because the filter's knobs (NZ_CONV_SMALL,
NZ_CONV_CHAIN) are read once per process.  usage: chain_plan_child.py <case> [out.npy]; exit status 0 and a last line
`ok` when every comparison held.

Planes are compared on their bit patterns with the CPU oracle (oracle.kernel_filter).  A grid that is not a square tile runs
through nz_debug_kernel_filter_window as a window of two larger planes that are NaN everywhere else, rows above and below
the window included: a NaN that reached a cell of the window would stay (a NaN tap makes a NaN sum), and a store outside the
window would replace one."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noize_job_amd as nj  # noqa: E402
import oracle as O  # noqa: E402

f32 = np.float32
GAUSS9, GAUSS5 = 0, 2
lib = nj._native.lib


def plane(rows, cols, seed):
    return ((np.random.default_rng(seed).random((rows, cols), dtype=f32) - f32(0.3)) * f32(8)).astype(f32)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert got.shape == want.shape and not bad.any(), "%s: %d of %d cells differ, first at %s" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]) if bad.any() else None)


_want = {}


def oracle(t, key, ft, it):
    if (key, ft, it) not in _want:
        _want[(key, ft, it)] = O.kernel_filter(t, ft, it)
    return _want[(key, ft, it)]


def window(ctx, t, ft, it, pitch, above=3, below=2):
    """`it` applications on t as a window of two NaN planes; returns the filtered window"""
    rows, cols = t.shape
    buf = np.full((above + rows + below, pitch), np.nan, f32)
    buf[above:above + rows, :cols] = t
    a, b = ctx.from_host(buf), ctx.from_host(np.full(buf.shape, np.nan, f32))
    st = nj.Stripe(cols, buf.shape[0], -above, rows, above, above + rows, pitch)
    swapped = C.c_int32(-1)
    ctx.call("nz_debug_kernel_filter_window", a.ptr, b.ptr, C.byref(st), ft, it, C.byref(swapped)).Complete()
    assert swapped.value in (0, 1)
    out, other = (b, a) if swapped.value else (a, b)
    got, rest = out.ToArray(buf.shape), other.ToArray(buf.shape)
    a.Dispose()
    b.Dispose()
    for p in (got, rest):  # nothing outside the window was written, in either plane
        assert np.isnan(p[:above]).all() and np.isnan(p[above + rows:]).all() and np.isnan(p[:, cols:]).all(), "a store left the window"
    return got[above:above + rows, :cols]


def stage(ctx, t, ft, it):
    res = t.shape[0]
    src, tmp = ctx.from_host(t), ctx.alloc(res * res)
    ctx.call("nz_kernel_filter_stage", src.ptr, tmp.ptr, ft, it, res).Complete()
    got = src.ToArray(t.shape)
    src.Dispose()
    tmp.Dispose()
    return got


def stage_rw(ctx, t, ft, it):
    res = t.shape[0]
    data, write = ctx.from_host(t), ctx.alloc(res * res)
    tile = nj._native.RWTile(data.ptr, write.ptr, res, 1)
    ctx.call("nz_kernel_filter_stage_rw", C.byref(tile), ft, it).Complete()
    got = ctx.wrap(tile.read, res * res).ToArray(t.shape)
    data.Dispose()
    write.Dispose()
    return got


SERIES = ((GAUSS5, 17), (GAUSS5, 13), (GAUSS9, 12))  # 4 launches, 3 launches (odd: the result changes planes), 4 launches


def case_metric():
    """NZ_CONV_SMALL=0 NZ_CONV_CHAIN=2: the 512 x 8 tile, chained from two launches on"""
    shapes = [(352, 352, 352),    # one fully interior tile, edge tiles on all four sides
              (360, 1000, 1000),  # 36 tiles per launch, uneven class counts
              (263, 301, 301),    # unaligned rows: the 4-byte path
              (352, 350, 352),    # aligned rows that are no whole groups of four columns: the 4-byte path again
              (350, 352, 356)]    # whole groups, a pitch beyond the row
    with nj.Context(0) as ctx:
        for rows, cols, pitch in shapes:
            t = plane(rows, cols, rows * 1000 + cols)
            for ft, it in SERIES:
                got = window(ctx, t, ft, it, pitch)
                assert np.isfinite(got).all(), "%dx%d ft=%d x%d: a value from outside the window reached it" % (rows, cols, ft, it)
                same_bits(got, oracle(t, (rows, cols), ft, it), "window %d rows x %d cols pitch %d ft=%d x%d" % (rows, cols, pitch, ft, it))
        t = plane(352, 352, 352352)
        same_bits(stage(ctx, t, GAUSS5, 17), oracle(t, (352, 352), GAUSS5, 17), "stage 352^2 Gauss5 x17")
        same_bits(stage_rw(ctx, t, GAUSS5, 13), oracle(t, (352, 352), GAUSS5, 13), "stage_rw 352^2 Gauss5 x13")
        same_bits(stage(ctx, t, GAUSS9, 12), oracle(t, (352, 352), GAUSS9, 12), "stage 352^2 Gauss9 x12")
        assert lib.nz_ctx_chain_plan_uploads(ctx._h) >= 3, "the chained form did not run"


def case_default():
    """default knobs: 512^2 and 768^2 run the 1024 x 2 shape for 5 taps and 512 x 4 for 9; 800^2 runs 512 x 4 for 5 taps"""
    with nj.Context(0) as ctx:
        for res in (512, 768, 800):
            t = plane(res, res, res)
            same_bits(stage(ctx, t, GAUSS5, 17), oracle(t, res, GAUSS5, 17), "stage %d^2 Gauss5 x17" % res)
            same_bits(stage_rw(ctx, t, GAUSS5, 13), oracle(t, res, GAUSS5, 13), "stage_rw %d^2 Gauss5 x13" % res)
            same_bits(stage(ctx, t, GAUSS9, 12), oracle(t, res, GAUSS9, 12), "stage %d^2 Gauss9 x12" % res)
        assert lib.nz_ctx_chain_plan_uploads(ctx._h) >= 3, "the chained form did not run"


def case_fast(out):
    """FAST mode, Gauss5 x17 and x13 on 352^2 and on the 360 x 1000 window: the planes go to `out` for the parent to compare
    across NZ_CONV_CHAIN settings"""
    with nj.Context(0) as ctx:
        ctx.float_mode = 1
        t, w = plane(352, 352, 1), plane(360, 1000, 2)
        got = [stage(ctx, t, GAUSS5, 17).ravel(), stage_rw(ctx, t, GAUSS5, 13).ravel(), window(ctx, w, GAUSS5, 17, 1000).ravel()]
        chained = lib.nz_ctx_chain_plan_uploads(ctx._h)
        assert (chained > 0) == (os.environ["NZ_CONV_CHAIN"] != "0"), "chained launches: %d" % chained
    np.save(out, np.concatenate(got))


def case_cache():
    """one context: geometry A, B, A with another iteration count, A again; then two more contexts interleaved"""
    up = lib.nz_ctx_chain_plan_uploads
    a, b = plane(512, 512, 11), plane(768, 768, 12)
    with nj.Context(0) as ctx:
        assert up(ctx._h) == 0
        same_bits(stage(ctx, a, GAUSS5, 17), oracle(a, "a", GAUSS5, 17), "A x17")
        assert up(ctx._h) == 1
        same_bits(stage(ctx, b, GAUSS5, 17), oracle(b, "b", GAUSS5, 17), "B x17")
        assert up(ctx._h) == 2
        same_bits(stage(ctx, a, GAUSS5, 12), oracle(a, "a", GAUSS5, 12), "A x12")
        assert up(ctx._h) == 3
        same_bits(stage(ctx, a, GAUSS5, 17), oracle(a, "a", GAUSS5, 17), "A x17 again")
        assert up(ctx._h) == 3, "the second call on A uploaded a plan"
        same_bits(stage(ctx, b, GAUSS5, 17), oracle(b, "b", GAUSS5, 17), "B x17 again")
        assert up(ctx._h) == 3
        # five plans through four slots: the least recently used one (A x12) goes, and comes back with an upload
        same_bits(stage(ctx, a, GAUSS9, 12), oracle(a, "a", GAUSS9, 12), "A Gauss9 x12")
        same_bits(stage(ctx, b, GAUSS9, 12), oracle(b, "b", GAUSS9, 12), "B Gauss9 x12")
        assert up(ctx._h) == 5
        same_bits(stage(ctx, a, GAUSS5, 17), oracle(a, "a", GAUSS5, 17), "A x17 after two more plans")
        assert up(ctx._h) == 5
        same_bits(stage(ctx, a, GAUSS5, 12), oracle(a, "a", GAUSS5, 12), "A x12 after its plan was replaced")
        assert up(ctx._h) == 6
        with nj.Context(0) as c2, nj.Context(0) as c3:
            for k in range(2):
                same_bits(stage(c2, a, GAUSS5, 17), oracle(a, "a", GAUSS5, 17), "context 2, A, round %d" % k)
                same_bits(stage(c3, b, GAUSS5, 17), oracle(b, "b", GAUSS5, 17), "context 3, B, round %d" % k)
                same_bits(stage(c2, b, GAUSS5, 17), oracle(b, "b", GAUSS5, 17), "context 2, B, round %d" % k)
                same_bits(stage(c3, a, GAUSS5, 17), oracle(a, "a", GAUSS5, 17), "context 3, A, round %d" % k)
            assert up(c2._h) == 2 and up(c3._h) == 2
        assert up(ctx._h) == 6 and up(None) == -1


def case_nan_window():
    """a finite 352 x 352 window of NaN planes, rows above and below it: the 16-byte edge accesses stay inside"""
    with nj.Context(0) as ctx:
        t = plane(352, 352, 99)
        for ft, it in SERIES:
            got = window(ctx, t, ft, it, 352, above=40, below=40)
            assert np.isfinite(got).all(), "ft=%d x%d: a value from outside the window reached it" % (ft, it)
            same_bits(got, oracle(t, 99, ft, it), "NaN-framed window ft=%d x%d" % (ft, it))
        assert lib.nz_ctx_chain_plan_uploads(ctx._h) == 3


if __name__ == "__main__":
    case = sys.argv[1]
    if case == "fast":
        case_fast(sys.argv[2])
    else:
        {"metric": case_metric, "default": case_default, "cache": case_cache, "nan_window": case_nan_window}[case]()
    print("ok")
