"""The multiple-flow implicit fluvial stage across the ABI and the three hosts, without a GPU: the header declares the entries
and nz_fluvial_implicit_mfd_desc, the library exports them, and the Python binding, Native.cs / Runtime.cs, Stages.cs and
noize_pipeline.hpp each carry MfdFluvialStage with the same parameters, defaults, default budget, entries, placement and
members."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_fluvial_implicit_mfd_work_floats", "nz_fluvial_implicit_mfd", "nz_fluvial_implicit_mfd_batch")
HOOK = "nz_debug_fluvial_implicit_mfd_sweeps"
FLOATS = ["erodibility", "uplift", "dt", "seaLevel"]
INTS = ["maxPasses", "exponent"]
POINTERS = ["hardness", "upliftMap", "proceed", "tally"]
BUDGET_PY, BUDGET_C = "128 + self.resolution // 2", "128 + resolution / 2"
# what one iteration of the stage calls besides its own entry, in every host
CHAIN = ("nz_tile_upload", "nz_drainage_mfd", "nz_drainage_mfd_batch", "nz_flush_write_slice")


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def body(src, head, nxt):
    i = src.index(head)
    return src[i:src.index(nxt, i + 1)]


def test_the_header_declares_the_entries_and_the_library_exports_them(nj):
    N = nj._native
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "noize_hip.h"), flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES + (HOOK,):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    flat = " ".join(hdr.split())
    assert "size_t nz_fluvial_implicit_mfd_work_floats(int32_t resolution, int32_t count);" in flat
    assert ("int32_t nz_fluvial_implicit_mfd(nz_ctx *ctx, const float *height, const float *drainage, float *out, "
            "float *work, const nz_fluvial_implicit_mfd_desc *desc, int32_t resolution, nz_handle dep, "
            "nz_handle *out_handle);") in flat
    assert ("int32_t nz_fluvial_implicit_mfd_batch(nz_ctx *ctx, const float *height, const float *drainage, float *out, "
            "float *work, const nz_fluvial_implicit_mfd_desc *desc, int32_t resolution, int32_t count, nz_handle dep, "
            "nz_handle *out_handle);") in flat
    assert "int32_t %s(int32_t sweeps);" % HOOK in flat
    assert not re.search(r"\bnz_fluvial_implicit_mfd\w*_stripe\w*\b|\bnz_fluvial_implicit_mfd\w*_rw\b", hdr)
    assert len(N.SIGNATURES["nz_fluvial_implicit_mfd"][1]) == 9 and len(N.SIGNATURES["nz_fluvial_implicit_mfd_batch"][1]) == 10
    # nz_fluvial_implicit_mfd_desc field by field against the binding and the C# struct
    decl = re.search(r"typedef struct nz_fluvial_implicit_mfd_desc \{(.*?)\} nz_fluvial_implicit_mfd_desc;", hdr, re.S).group(1)
    decls = [" ".join(d.split()) for d in decl.split(";") if d.strip()]
    assert decls == ["float erodibility, uplift, dt, seaLevel", "int32_t maxPasses", "int32_t exponent", "const float *hardness",
                     "const float *upliftMap", "const int32_t *proceed", "int32_t *tally"]
    D = N.FluvialImplicitMfdDesc
    assert [f[0] for f in D._fields_] == FLOATS + INTS + POINTERS
    assert [f[1] for f in D._fields_] == [ctypes.c_float] * 4 + [ctypes.c_int32] * 2 + [ctypes.c_void_p] * 4
    assert ctypes.sizeof(D) == 56 and D.exponent.offset == 20 and D.hardness.offset == 24
    cs_body = re.search(r"public struct NzFluvialImplicitMfdDesc\s*\{(.*?)\}", read("host-cs", "Runtime.cs"), re.S).group(1)
    cs = [(t, n.strip()) for t, d in re.findall(r"public\s+(\w+)\s+([^;]+);", cs_body) for n in d.split(",")]
    assert cs == [("float", n) for n in FLOATS] + [("int", n) for n in INTS] + [("IntPtr", n) for n in POINTERS]
    # the single-flow desc is what it was
    assert ctypes.sizeof(N.FluvialImplicitDesc) == 56 and not hasattr(N.FluvialImplicitDesc, "exponent")


def test_the_work_planes_have_a_floor_and_a_ceiling(nj):
    # at least the gate bytes, b, the eight f planes and the second h' plane; on top of that no more than a D plane, the
    # header, the tile bytes and slack
    w = nj._native.lib.nz_fluvial_implicit_mfd_work_floats
    assert w(0, 1) == 0 and w(64, 0) == 0 and w(0, 0) == 0 and w(-3, 2) == 0 and w(8, -1) == 0
    for res, count in ((1, 1), (64, 1), (97, 3), (4096, 1)):
        n = res * res * count
        tiles = -(-res // 64) * -(-res // 16) * count
        floor = 10 * n + -(-n // 4)
        assert floor <= w(res, count) <= 11 * n + -(-n // 4) + 16 + 2 * (tiles + 15) // 4 + 12, (res, count)
    assert w(97, 3) > 3 * w(97, 1) - 3 * 16  # a batch is its tiles back to back, one header
    assert w(64, 1) % 4 == 0


def test_the_sweep_hook_is_this_stage_s_own(nj):
    lib = nj._native.lib
    others = ("nz_debug_fill_sweeps", "nz_debug_drainage_sweeps", "nz_debug_watershed_sweeps", "nz_debug_stream_order_sweeps",
              "nz_debug_fluvial_implicit_sweeps", "nz_debug_drainage_mfd_sweeps")
    before = [getattr(lib, o)(0) for o in others]
    hook = getattr(lib, HOOK)
    d = hook(5)
    assert d == 16 and hook(0) == 5 and hook(0) == d
    assert hook(-2) == d and hook(0) == d
    assert [getattr(lib, o)(0) for o in others] == before  # it does not disturb the other six
    for o in others[4:]:
        getattr(lib, o)(3)
        assert hook(0) == d and getattr(lib, o)(0) == 3  # ... nor they it
        assert getattr(lib, o)(0) == 16


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES + (HOOK,):
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert "public static extern UIntPtr nz_fluvial_implicit_mfd_work_floats(int resolution, int count);" in cs
    assert ("nz_fluvial_implicit_mfd(IntPtr ctx, IntPtr height, IntPtr drainage, IntPtr @out, IntPtr work, "
            "ref NzFluvialImplicitMfdDesc desc, int resolution, ulong dep, out ulong out_handle)") in cs
    assert ("nz_fluvial_implicit_mfd_batch(IntPtr ctx, IntPtr height, IntPtr drainage, IntPtr @out, IntPtr work, "
            "ref NzFluvialImplicitMfdDesc desc, int resolution, int count, ulong dep, out ulong out_handle)") in cs
    assert '"nz_fluvial_implicit_mfd_desc": "NzFluvialImplicitMfdDesc"' in read("tools", "gen_native_cs.py")


def test_the_three_hosts_carry_the_stage_with_the_same_defaults(nj):
    st = nj.MfdFluvialStage(None)
    assert isinstance(st, nj.PipelineStage) and "MfdFluvialStage" in nj.__all__
    # a class of its own on PipelineStage, as in the other two hosts: none of the single-flow stage's members
    assert not isinstance(st, nj.ImplicitFluvialStage) and nj.MfdFluvialStage.__bases__ == (nj.PipelineStage,)
    assert not hasattr(st, "routing") and not hasattr(st, "flowExponent")
    got = (st.iterations, st.erodibility, st.uplift, st.dt, st.rain, st.exponent, st.maxPasses, st.rainMap, st.hardness,
           st.upliftMap)
    assert got == (1, 0.05, 0.002, 1.0, 1.0, 1, None, None, None, None)
    assert np.float32(st.seaLevel) == -np.finfo(np.float32).max == np.float32(nj.ImplicitFluvialStage(None).seaLevel)
    assert (st.drainage, st.steps, st.passes, st.converged) == (None, None, None, None)  # no payload yet
    a, b, c = object(), object(), object()
    other = nj.MfdFluvialStage(None, 4, 0.1, 0.01, 250.0, 2.0, 0.25, 3, 7, a, b, c)  # the positional order of the signature
    assert (other.iterations, other.erodibility, other.uplift, other.dt, other.rain, other.seaLevel, other.exponent,
            other.maxPasses) == (4, 0.1, 0.01, 250.0, 2.0, 0.25, 3, 7)
    assert (other.rainMap, other.hardness, other.upliftMap) == (a, b, c)
    pipe = nj.BasePipeline([nj.NoiseStage(None, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300),
                            nj.DepressionFillStage(None), st, nj.HillslopeDiffusionStage(None)], "fans")
    assert pipe is not None
    py = read("noize_job_amd", "pipeline.py")
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")
    assert re.search(r"class MfdFluvialStage\s*:\s*public PipelineStage", hpp)
    assert re.search(r"class MfdFluvialStage\s*:\s*PipelineStage", cs)
    bpy = body(py, "class MfdFluvialStage(", "\nclass ")
    bhpp = body(hpp, "class MfdFluvialStage ", "\nclass ")
    bcs = body(cs, "public class MfdFluvialStage ", "    public class ")
    # placed directly behind the implicit stage and in front of the hillslope stage in each host
    for src, head, nxt in ((py, "class %s(", "\nclass "), (hpp, "class %s ", "\nclass "), (cs, "public class %s ", "    public class ")):
        i = src.index(head % "ImplicitFluvialStage")
        j = src.index(nxt, i + 1)
        assert src[j:].lstrip("\n ").startswith((head % "MfdFluvialStage").strip()), head
        k = src.index(nxt, j + 1)
        assert src[k:].lstrip("\n ").startswith((head % "HillslopeDiffusionStage").strip()), head
    # the same parameters in the same order, the same defaults, the same default budget, the same entries, the same members
    flat = " ".join(bpy.split())
    assert "iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=SEA_OFF, exponent=1," in flat
    assert "exponent=1, maxPasses=None, rainMap=None, hardness=None, upliftMap=None):" in flat
    assert "int iterations = 1;" in bhpp and "public int iterations = 1;" in bcs
    assert "float erodibility = .05f, uplift = .002f, dt = 1.f, rain = 1.f, seaLevel = -3.402823466e+38f;" in bhpp
    assert "float erodibility = 0.05f, uplift = 0.002f, dt = 1f, rain = 1f, seaLevel = -float.MaxValue;" in bcs
    assert "int exponent = 1;" in bhpp and "public int exponent = 1;" in bcs
    assert "*rainMap = nullptr, *hardness = nullptr, *upliftMap = nullptr;" in bhpp
    assert "DeviceTile rainMap = null, hardness = null, upliftMap = null;" in bcs
    assert "int? maxPasses = null;" in bcs and re.search(r"int maxPasses = 0;\s*// < 1: %s" % re.escape(BUDGET_C), bhpp)
    # the members in the order of the signature: the exponent in front of the budget
    for b in (bhpp, bcs):
        assert b.index("int exponent = 1;") < b.index("maxPasses = ") < b.index("rainMap = null")
    assert BUDGET_PY in bpy and BUDGET_C in bhpp and BUDGET_C in bcs
    assert "64 + self.resolution // 4" not in bpy and "64 + resolution / 4" not in bhpp + bcs  # one budget for both series
    for b, call in ((bpy, '"%s"'), (bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES + CHAIN:
            assert call % entry in b or (entry.endswith("work_floats") and entry + "(" in b), (entry, call)
        assert "nz_drainage_mfd_work_floats(" in b
        # no pair form, no stripe form, not the tree's drainage and not the single-flow solve
        assert "_rw" not in b and "stripe" not in b.lower() and "nz_drainage_area" not in b
        assert not re.search(r"nz_fluvial_implicit(_batch)?\(|\"nz_fluvial_implicit(_batch)?\"", b)
    # both calls take the same exponent, and the solve is told to proceed by the drainage call's converged word
    assert "N.DrainageMfdDesc(self.rain, self.seaLevel, budget, self.exponent, opt(self.rainMap))" in bpy
    assert "self.seaLevel, budget, self.exponent," in bpy
    assert bhpp.count("budget, exponent,") == 2 and bcs.count("maxPasses = budget, exponent = exponent") == 2
    assert "self.drainageWork.ptr + 4" in bpy and "(drainageWork->ptr) + 1" in bhpp and "IntPtr.Add(drainageWork.Ptr, 4)" in bcs
    for m in ("drainage", "steps", "passes", "converged"):
        assert isinstance(getattr(nj.MfdFluvialStage, m), property), m
    for b, members in ((bhpp, ("drainage() const", "int steps() const", "int passes() const", "bool converged() const")),
                       (bcs, ("DeviceTile Drainage", "int? Steps", "int? Passes", "bool? Converged"))):
        for m in members:
            assert m in b, m
    # the header states the same defaults and says what follows and what is left out
    words = " ".join(body(read("include", "noize_hip.h"), "---- multiple-flow implicit fluvial erosion:",
                          "typedef struct nz_fluvial_implicit_mfd_desc").split())
    words = words.replace(" * ", " ")
    assert "iterations 1, erodibility 0.05, uplift 0.002, dt 1, rain 1, seaLevel -FLT_MAX (off), exponent 1" in words
    assert ("maxPasses " + BUDGET_C) in words
    for must in ("exactly one positive weight has w == 1", "erodibility == 0 gives h + du off the outlets",
                 "outlets keep their bits", "min_k h'[k] <= h'[c] <= h[c] + du", "NaN heights send and receive nothing",
                 "travels upstream", "overflows", "pits stay pits", "ALL OR NOTHING", "out = h bit for bit",
                 "\"cells of the longest path of the flow DAG\" + 2", "The gate is w_k > 0, never the value of f_k or of h'",
                 "no row-stripe form and no _rw form", "exponent outside 1..16", "(not through the division)"):
        assert must in words, must


def test_the_single_flow_stage_is_what_it_was(nj):
    st = nj.ImplicitFluvialStage(None, routing=nj.FlowRouting.Multiple, flowExponent=4)
    assert not isinstance(st, nj.MfdFluvialStage) and (st.routing, st.flowExponent) == (nj.FlowRouting.Multiple, 4)
    bpy = body(read("noize_job_amd", "pipeline.py"), "class ImplicitFluvialStage(", "\nclass ")
    assert "nz_fluvial_implicit_mfd" not in bpy and "steepest receiver" in bpy


def test_the_documents_name_the_stage_and_the_tool_exists():
    readme = read("README.md")
    assert "MfdFluvialStage(" in readme and "nz_fluvial_implicit_mfd" in readme and "tools/bench_fluvial_implicit_mfd.py" in readme
    integ = read("INTEGRATION.md")
    assert "nz_fluvial_implicit_mfd(" in integ and "nz_fluvial_implicit_mfd_batch(" in integ and "NzFluvialImplicitMfdDesc" in integ
    design = read("DESIGN.md")
    assert "nz_fluvial_implicit_mfd.hip" in design and "| f13 " in design and HOOK in design
    assert "another linear system, not a tree" not in design
    assert "MfdFluvialStage" in read("host-cs", "README.md")
    assert "MfdFluvialStage" in read("HISTORY.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_fluvial_implicit_mfd.py"))
    mk = read("noize_job_amd", "csrc", "Makefile")
    assert "nz_fluvial_implicit_mfd.hip" in mk
    for hdr in ("nz_receiver.hpp", "nz_tile64.hpp", "nz_relax_pass.hpp", "nz_mfd_weights.hpp"):
        assert re.search(r"build/nz_fluvial_implicit_mfd\.o[^\n]*: %s" % re.escape(hdr), mk), hdr
    assert re.search(r"build/nz_drainage_mfd\.o[^\n]*: nz_mfd_weights\.hpp", mk)
    # one statement of the weights: the drainage file includes it and defines none of its own
    dm = read("noize_job_amd", "csrc", "nz_drainage_mfd.hip")
    assert '#include "nz_mfd_weights.hpp"' in dm and "float mfd_power(" not in dm and "void mfd_send_terms(" not in dm
