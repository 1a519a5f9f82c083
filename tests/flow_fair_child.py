"""The GPU side of tests/test_gpu_flow_fair.py: every case of CASES through the row-streaming flow kernel, in all three
float modes, in ONE process -- NZ_FLOW_STREAM and NZ_FLOW_FAIR are read once per process, so the parent starts one child
per setting.  usage: flow_fair_child.py <out.npz>; exit status 0 and a last line `ok` when every launch streamed and ran.

The child compares nothing but the form: it writes, per mode and case, the whole destination buffer (the pads and the NaN
rows around a slab-carved plane included) and the parent compares those with the oracle and with the other child's.

A case is (kind, n, rows, cols, count, pad):
  "stripe": rows x cols cells, the whole grid in one stripe of nz_flow_fused_stripe (first and last), pitch cols + pad;
  "slab"  : the same entry on owned rows inside a taller grid, 2n ghost rows either side, in a buffer whose other rows and
            pads are NaN;
  "batch" : count tiles of rows x rows cells through nz_flowmap_stage_batch."""
import ctypes as C
import os
import sys

import numpy as np

f32 = np.float32
MODES = {0: "strict", 1: "fast", 2: "relaxed"}
STREAM = 3
# rows: the pipeline fill only (1, 9); one 16-row segment whose steps after the fill end on a whole three-step trip or leave
# one or two (16, 17, 18); two segments (17 .. 33); seven segments, the inner ones with their fill away from the grid's first
# rows (97).  columns: one strip, both x borders in one wave (1, 2, 107 at n = 5, 108 at n = 5); the two border strips only
# (109, and 107 / 108 at n = 4); an inner strip between them (217), at odd and even widths
ROWS = (1, 9, 16, 17, 18, 19, 33, 97)
COLS = (1, 2, 107, 108, 109, 217)
CASES = ([("stripe", n, rows, cols, 1, 0) for n in (4, 5) for rows in ROWS for cols in COLS] +
         [("batch", n, res, res, count, 0) for n in (4, 5) for res in (17, 97, 109) for count in (1, 2)] +
         [("slab", n, 33, 217, 1, 3) for n in (4, 5)])
ABOVE, BELOW = 2, 3   # NaN rows of a slab beyond its ghost rows


def case_id(case):
    return "%s-x%d-%dx%d-c%d-p%d" % case


def inputs(case):
    """The heights of a case, (count, grid rows, cols): relief and roughness on the scale of the water column."""
    import flow_ref as F
    kind, n, rows, cols, count, pad = case
    rng = np.random.default_rng(CASES.index(case) + 77)
    grows = rows + 4 * n if kind == "slab" else rows
    return np.stack([F.terrain(rng, grows, cols) for _ in range(count)])


def main(out):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import noize_job_amd as nj
    import flow_ref as F

    lib, planes = nj._native.lib, {}
    for mode in MODES:
        with nj.Context(0) as ctx:
            ctx.float_mode = mode
            assert ctx.float_mode == mode
            for case in CASES:
                kind, n, rows, cols, count, pad = case
                h = inputs(case)
                form = lib.nz_flow_launch_form(ctx._h, cols, rows, count, n, 1, 1)
                assert form == STREAM, "%s takes form %d, not the streaming kernel" % (case_id(case), form)
                if kind == "batch":
                    src, work = ctx.from_host(h), ctx.alloc(11 * h.size)
                    ctx.call("nz_flowmap_stage_batch", src.ptr, work.ptr, n, *F.NORM, rows, count).Complete()
                    got = src.ToArray(h.shape)
                    tiles = [src, work]
                else:
                    pitch, halo = cols + pad, 2 * n if kind == "slab" else 0
                    above, below = (ABOVE, BELOW) if kind == "slab" else (0, 0)
                    buf = np.full((above + h.shape[1] + below, pitch), np.nan, f32)
                    buf[above:above + h.shape[1], :cols] = h[0]
                    own0 = above + halo
                    # the grid goes on above and below a slab: its 2n ghost rows are the first and last rows with values
                    st = nj.Stripe(cols, buf.shape[0], 7 - above if kind == "slab" else 0,
                                   h.shape[1] + 14 if kind == "slab" else rows, own0, own0 + rows, pitch)
                    src, dst = ctx.from_host(buf), ctx.from_host(np.full(buf.shape, np.nan, f32))
                    ctx.call("nz_flow_fused_stripe", src.ptr, None, None, dst.ptr, C.byref(st), n, 1, 1, *F.NORM, handle=False)
                    ctx.synchronize()
                    got = dst.ToArray(buf.shape)
                    tiles = [src, dst]
                for t in tiles:
                    t.Dispose()
                planes["%s/%s" % (MODES[mode], case_id(case))] = got
    np.savez(out, **planes)
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
