"""The GPU side of tests/test_gpu_strict_valu.py: one environment per process, because the launch-form knobs (NZ_CONV_SYM,
NZ_CONV_SMALL, NZ_CONV_CHAIN, NZ_FLOW_STREAM) are read once per process.

usage: strict_valu_child.py conv|flow <cases.npz> [group]; exit status 0 and a last line `ok` when every comparison held.
The parent wrote the inputs and the CPU oracle's planes into <cases.npz> once; every environment compares against the same
reference, on bit patterns (the sign of a zero counts)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noize_job_amd as nj  # noqa: E402
from chain_plan_child import same_bits, stage, window  # noqa: E402
from flow_ref import NORM, assert_bits_equal  # noqa: E402
from slab import Slab  # noqa: E402

f32 = np.float32
STREAM = 3  # nz_flow_launch_form


def stage_in_slab(ctx, t, ft, it, phase):
    """nz_kernel_filter_stage on planes carved from one slab, each `phase` floats past a 16-byte boundary"""
    res = t.shape[0]
    with Slab(ctx, guard=max(2 * res, 1024)) as slab:
        src = slab.carve(t.size, phase=phase, fill=t, name="src")
        tmp = slab.carve(t.size, phase=phase, name="tmp")
        slab.upload()
        ctx.call("nz_kernel_filter_stage", src.ptr, tmp.ptr, ft, it, res).Complete()
        got = src.ToArray(t.shape)
        slab.check()
    return got


def conv(cases, group):
    meta = json.loads(str(cases["meta"]))
    with nj.Context(0) as ctx:
        for c in meta:
            if c["group"] != group:
                continue
            t = cases[c["key"]]
            for ft in c["filters"]:
                for it in c["iterations"]:
                    if c["kind"] == "slab":
                        got = stage_in_slab(ctx, t, ft, it, 1)
                    elif c["kind"] == "window":
                        got = window(ctx, t, ft, it, t.shape[1] + 1)
                    else:
                        got = stage(ctx, t, ft, it)
                    same_bits(got, cases["%s_%d_%d" % (c["key"], ft, it)],
                              "%s %s %dx%d ft=%d x%d" % (c["kind"], c["key"], t.shape[0], t.shape[1], ft, it))


def flow(cases):
    meta = json.loads(str(cases["meta"]))
    want_stream = os.environ.get("NZ_FLOW_STREAM") == "2"
    lib = nj._native.lib
    with nj.Context(0) as ctx:
        for c in meta:
            h = cases[c["key"]]
            rows, cols = h.shape
            src, dst = ctx.from_host(h), ctx.alloc(h.size)
            st = nj.Stripe(cols, rows, 0, rows, 0, rows, cols)
            for n in c["iterations"]:
                form = lib.nz_flow_launch_form(ctx._h, cols, rows, 1, n, 1, 1)
                assert (form == STREAM) == want_stream, "%d x %d x%d runs as form %d" % (rows, cols, n, form)
                ctx.call("nz_flow_fused_stripe", src.ptr, None, None, dst.ptr, C.byref(st), n, 1, 1, *NORM).Complete()
                assert_bits_equal(dst.ToArray(h.shape), cases["%s_%d" % (c["key"], n)],
                                  "flow %s %d rows x %d cols x%d (form %d)" % (c["key"], rows, cols, n, form))
            src.Dispose()
            dst.Dispose()


if __name__ == "__main__":
    with np.load(sys.argv[2]) as cases:
        if sys.argv[1] == "conv":
            conv(cases, sys.argv[3])
        else:
            flow(cases)
    print("ok")
