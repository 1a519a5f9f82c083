"""The drainage stage's stripe form across the ABI and the hosts: the header declares the four entries, the library exports
them and the binding knows them; Native.cs is generated with the header's signatures and Stages.cs / noize_pipeline.hpp
carry the round and the finalise on DrainageAreaStage, as DepressionFillStage has them; the sharded module has the
drivers; the documents no longer list the stripe form as missing.  On the GPU the compiled C++ mirror runs one round plus
finalise and equals the Python path bit for bit."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_drainage_stripe_halo_rows", "nz_drainage_stripe_work_floats", "nz_drainage_stripe_round", "nz_drainage_stripe_finalise")


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_header_declares_the_entries_and_the_library_exports_them(nj):
    N = nj._native
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "noize_hip.h"), flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    flat = " ".join(hdr.split())
    assert "int32_t nz_drainage_stripe_halo_rows(void);" in flat
    assert "size_t nz_drainage_stripe_work_floats(const nz_stripe *st);" in flat
    assert ("int32_t nz_drainage_stripe_round(nz_ctx *ctx, const float *height, float *a, float *work, const nz_stripe *st, "
            "const nz_drainage_desc *desc, int32_t first, const int32_t *proceed, int32_t *changed, nz_handle dep, "
            "nz_handle *out);") in flat
    assert ("int32_t nz_drainage_stripe_finalise(nz_ctx *ctx, float *a, const nz_stripe *st, const nz_drainage_desc *desc, "
            "const int32_t *converged, nz_handle dep, nz_handle *out);") in flat
    # the desc is what it was
    body = re.search(r"typedef struct nz_drainage_desc \{(.*?)\} nz_drainage_desc;", hdr, re.S).group(1)
    assert [" ".join(d.split()) for d in body.split(";") if d.strip()] == ["float rain, seaLevel", "int32_t maxPasses",
                                                                           "const float *rainMap"]
    # the work planes: the fill stripe's status words and tile bytes, the donor bytes, one plane; nothing for a stripe
    # that cannot be sized
    assert N.lib.nz_drainage_stripe_halo_rows() == 2
    w = N.lib.nz_drainage_stripe_work_floats
    assert w(None) == 0 and w(ctypes.byref(N.Stripe(0, 4, 0, 4, 0, 4, 0))) == 0
    for cols, own, pitch in ((97, 23, 0), (96, 24, 104), (4096, 512, 0), (130, 2, 135)):
        st = N.Stripe(cols, own + 4, 10, 10000, 2, 2 + own, pitch)
        plane = (own + 4) * (pitch or cols)
        fill = N.lib.nz_fill_stripe_work_floats(ctypes.byref(st))
        assert w(ctypes.byref(st)) == fill + (plane + 15) // 16 * 4, (cols, own, pitch)


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES:
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert ("nz_drainage_stripe_round(IntPtr ctx, IntPtr height, IntPtr a, IntPtr work, ref NzStripe st, ref NzDrainageDesc desc, "
            "int first, IntPtr proceed, IntPtr changed, ulong dep, out ulong @out)") in cs
    assert ("nz_drainage_stripe_finalise(IntPtr ctx, IntPtr a, ref NzStripe st, ref NzDrainageDesc desc, IntPtr converged, "
            "ulong dep, out ulong @out)") in cs


def test_the_hosts_carry_the_round_and_the_finalise():
    from noize_job_amd import sharded as sh
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")

    def body(src, head, nxt):
        i = src.index(head)
        return src[i:src.index(nxt, i + 1)]

    bhpp = body(hpp, "class DrainageAreaStage ", "\nclass ")
    bcs = body(cs, "public class DrainageAreaStage ", "    public class ")
    for b, call in ((bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES[2:]:
            assert call % entry in b, (entry, call)
        assert "ScheduleStripe(" in b and "FinaliseStripe(" in b
    assert "const nz_drainage_desc desc{rain, seaLevel, passes, rainMapRows};" in bhpp
    assert "rain = rain, seaLevel = seaLevel, maxPasses = passes, rainMap = rainMapRows" in bcs
    for name in ("drainage_steps", "run_drainage", "run_drainage_lockstep"):
        assert callable(getattr(sh, name)), name
    assert callable(sh.HipStripeOps.drainage) and callable(sh.HipStripeOps.drainage_finalise)
    assert sh.DRAINAGE_DEFAULTS == dict(rain=1.0, seaLevel=-3.4028234663852886e38, maxPasses=64, maxRounds=64)
    # the documents: the stripe form is there, and nowhere listed as missing
    assert "run_drainage(" in read("README.md")
    assert "nz_drainage_stripe_round" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "nz_drainage_stripe_round" in design and "no stripe form" not in design
    assert "no stripe form" not in read("include", "noize_hip.h") and "no stripe form" not in read("noize_job_amd", "csrc", "nz_drainage.hip")
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_drainage_stripe.py"))


@pytest.mark.gpu
def test_the_cpp_mirror_runs_a_round_and_the_finalise(nj, tmp_path):
    """host_demo's drainage-stripe mode: a filled simplex tile as one stripe through DrainageAreaStage::ScheduleStripe with
    `first` and FinaliseStripe with a word of 1; the same through HipStripeOps on the heights it wrote."""
    import torch
    import drainage_ref as D
    from drainage_stripe_cases import assert_bits, stripe_bufs, stripe_ops, work_floats
    exe = os.path.join(ROOT, "noize_job_amd", "host", "host_demo")
    assert os.path.exists(exe), "host_demo not built (run __graft_entry__.build())"
    res, out = 160, str(tmp_path / "planes.f32")
    changed = subprocess.run([exe, str(res), out, "drainage-stripe"], check=True, capture_output=True, text=True).stdout.split()
    assert changed == ["1"]
    h, got = np.fromfile(out, dtype=np.float32).reshape(2, res, res)
    with stripe_ops(nj) as (sh, ops):
        plan = sh.StripePlan(0, 1, res, res, 0)
        bufs = stripe_bufs(plan, h, work_floats(nj)(plan), "cuda")
        prm = dict(sh.DRAINAGE_DEFAULTS, maxPasses=64 + res // 4)
        ops.drainage(bufs["H"], bufs["A"], bufs["work"], plan, prm, True, None, bufs["words"][0:1])
        bufs["words"][2:3].fill_(1)
        ops.drainage_finalise(bufs["A"], plan, prm, bufs["words"][2:3])
        torch.cuda.current_stream().synchronize()
        assert int(bufs["words"][0]) == 1
        assert_bits(got, bufs["A"].cpu().numpy(), "the C++ mirror against the Python path")
    assert_bits(got, D.accumulate(h)[0], "the walk")
