"""The implicit fluvial stage's stripe form across the ABI and the hosts: the header declares the four entries, the library
exports them and the binding knows them; Native.cs is generated with the header's signatures; the three hosts carry
ImplicitFluvialStripe -- a class of its own, not ImplicitFluvialStage -- with the round and the finalise; the sharded module
has the drivers; the documents name the entries and no longer list the stripe form as missing."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_implicit_fluvial_stripe_halo_rows", "nz_implicit_fluvial_stripe_work_floats", "nz_implicit_fluvial_stripe_round",
           "nz_implicit_fluvial_stripe_finalise")


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
    assert "int32_t nz_implicit_fluvial_stripe_halo_rows(void);" in flat
    assert "size_t nz_implicit_fluvial_stripe_work_floats(const nz_stripe *st);" in flat
    assert ("int32_t nz_implicit_fluvial_stripe_round(nz_ctx *ctx, const float *height, const float *drainage, float *out, "
            "float *work, const nz_stripe *st, const nz_fluvial_implicit_desc *desc, int32_t first, const int32_t *proceed, "
            "int32_t *changed, nz_handle dep, nz_handle *out_handle);") in flat
    assert ("int32_t nz_implicit_fluvial_stripe_finalise(nz_ctx *ctx, const float *height, float *out, const nz_stripe *st, "
            "const int32_t *converged, nz_handle dep, nz_handle *out_handle);") in flat
    # directly after the tile entry's test hook
    assert flat.index("nz_debug_fluvial_implicit_sweeps(int32_t sweeps);") < flat.index(ENTRIES[0]) < flat.index("nz_hillslope_desc")
    # the desc is what it was
    body = re.search(r"typedef struct nz_fluvial_implicit_desc \{(.*?)\} nz_fluvial_implicit_desc;", hdr, re.S).group(1)
    assert [" ".join(d.split()) for d in body.split(";") if d.strip()] == [
        "float erodibility, uplift, dt, seaLevel", "int32_t maxPasses", "const float *hardness", "const float *upliftMap",
        "const int32_t *proceed", "int32_t *tally"]
    # the work planes: the tile entry's layout over the stripe's plane -- the fill stripe's head, the receiver bytes, b, f
    # and the second h' plane; nothing for a stripe that cannot be sized
    assert N.lib.nz_implicit_fluvial_stripe_halo_rows() == 1
    w = N.lib.nz_implicit_fluvial_stripe_work_floats
    assert w(None) == 0 and w(ctypes.byref(N.Stripe(0, 4, 0, 4, 0, 4, 0))) == 0
    for cols, own, pitch in ((97, 23, 0), (96, 24, 104), (4096, 512, 0), (130, 2, 135)):
        st = N.Stripe(cols, own + 4, 10, 10000, 2, 2 + own, pitch)
        plane = (own + 4) * (pitch or cols)
        fill = N.lib.nz_fill_stripe_work_floats(ctypes.byref(st))  # the head and one plane
        assert w(ctypes.byref(st)) == fill + (plane + 15) // 16 * 4 + 2 * plane, (cols, own, pitch)
    # one stripe over a square grid: the tile entry's floats
    for res in (64, 97, 160):
        assert w(ctypes.byref(N.Stripe(res, res, 0, res, 0, res, 0))) == N.lib.nz_fluvial_implicit_work_floats(res, 1)


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES:
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert ("nz_implicit_fluvial_stripe_round(IntPtr ctx, IntPtr height, IntPtr drainage, IntPtr @out, IntPtr work, "
            "ref NzStripe st, ref NzFluvialImplicitDesc desc, int first, IntPtr proceed, IntPtr changed, ulong dep, "
            "out ulong out_handle)") in cs
    assert ("nz_implicit_fluvial_stripe_finalise(IntPtr ctx, IntPtr height, IntPtr @out, ref NzStripe st, IntPtr converged, "
            "ulong dep, out ulong out_handle)") in cs


def test_the_three_hosts_carry_the_stripe_class():
    from noize_job_amd import sharded as sh
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")

    def body(src, head, nxt):
        i = src.index(head)
        return src[i:src.index(nxt, i + 1)]

    # a class of its own, without a base class, behind MfdFluvialStage (and behind HillslopeDiffusionStage, which
    # tests/test_fluvial_implicit_mfd_hosts.py keeps directly behind MfdFluvialStage)
    bhpp = body(hpp, "class ImplicitFluvialStripe {", "\nclass ")
    bcs = body(cs, "public class ImplicitFluvialStripe {", "    public class ")
    assert hpp.index("class MfdFluvialStage ") < hpp.index("class ImplicitFluvialStripe {")
    assert cs.index("public class MfdFluvialStage ") < cs.index("public class ImplicitFluvialStripe {")
    for b, call in ((bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES[2:]:
            assert call % entry in b, (entry, call)
        assert "ScheduleStripe(" in b and "FinaliseStripe(" in b
        for field in ("erodibility", "uplift", "dt", "seaLevel", "hardnessRows", "upliftMapRows"):
            assert re.search(r"\b%s\b" % field, b), field
    assert "const nz_fluvial_implicit_desc desc{erodibility, uplift, dt, seaLevel, passes, hardnessRows, upliftMapRows, nullptr, nullptr};" in bhpp
    assert "maxPasses = passes" in bcs and "proceed = IntPtr.Zero, tally = IntPtr.Zero" in bcs
    # ... and ImplicitFluvialStage is what it was
    assert "stripe" not in body(hpp, "class ImplicitFluvialStage ", "\nclass ").lower()
    # the Python host: the same name over HipStripeOps, the drivers and the defaults
    assert callable(sh.ImplicitFluvialStripe.ScheduleStripe) and callable(sh.ImplicitFluvialStripe.FinaliseStripe)
    for name in ("fluvial_implicit_steps", "run_fluvial_implicit", "run_fluvial_implicit_lockstep"):
        assert callable(getattr(sh, name)), name
    assert callable(sh.HipStripeOps.fluvial_implicit) and callable(sh.HipStripeOps.fluvial_implicit_finalise)
    assert sh.FLUVIAL_IMPLICIT_DEFAULTS == dict(iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0,
                                                seaLevel=-3.4028234663852886e38, maxPasses=64, maxRounds=64)
    demo = read("noize_job_amd", "host", "host_demo.cpp")
    assert '"fluvial-implicit-stripe"' in demo and "ImplicitFluvialStripe solve(ctx);" in demo


def test_the_documents_name_the_stripe_form():
    assert "run_fluvial_implicit(" in read("README.md")
    assert "bench_fluvial_implicit_stripe.py" in read("README.md")
    for doc in (("INTEGRATION.md",), ("DESIGN.md",), ("HISTORY.md",), ("host-cs", "README.md")):
        assert "nz_implicit_fluvial_stripe_round" in read(*doc), doc
    # DESIGN section 9 no longer says of nz_fluvial_implicit that it has no stripe form; what is still missing stays listed
    design = read("DESIGN.md")
    nine = design[design.index("\n## 9"):]
    i = nine.index("* Implicit fluvial erosion (`nz_fluvial_implicit`")
    bullet = nine[i:nine.index("\n* ", i + 1)] if "\n* " in nine[i + 1:] else nine[i:]
    assert "nz_implicit_fluvial_stripe_round" in bullet and "row-stripe forms" in bullet
    assert not re.search(r"[Nn]o row-stripe|tile and batch forms only", bullet)
    for still in ("watershed", "stream-order", "nz_sharded_"):
        assert still in nine, still
    hdr = read("include", "noize_hip.h")
    assert "There is no row-stripe form and no _rw pair form" not in hdr
    assert "nz_implicit_fluvial_stripe_round / _finalise" in hdr
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_fluvial_implicit_stripe.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "fluvial_implicit_stripe.txt"))
