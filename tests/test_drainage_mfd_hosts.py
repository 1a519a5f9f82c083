"""The multiple-flow drainage stage across the ABI and the three hosts, without a GPU: the header declares the entries and
nz_drainage_mfd_desc, the library exports them, and the Python binding, Native.cs / Runtime.cs, Stages.cs and
noize_pipeline.hpp each carry MfdDrainageStage and ImplicitFluvialStage's routing with the same parameters, defaults,
positional order and entries."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_drainage_mfd_work_floats", "nz_drainage_mfd", "nz_drainage_mfd_batch")
HOOK = "nz_debug_drainage_mfd_sweeps"
BUDGET_PY, BUDGET_C = "128 + self.resolution // 2", "128 + resolution / 2"


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
    assert "size_t nz_drainage_mfd_work_floats(int32_t resolution, int32_t count);" in flat
    assert ("int32_t nz_drainage_mfd(nz_ctx *ctx, const float *height, float *drainage, float *work, "
            "const nz_drainage_mfd_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out);") in flat
    assert ("int32_t nz_drainage_mfd_batch(nz_ctx *ctx, const float *height, float *drainage, float *work, "
            "const nz_drainage_mfd_desc *desc, int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);") in flat
    assert "int32_t nz_debug_drainage_mfd_sweeps(int32_t sweeps);" in flat
    assert not re.search(r"\bnz_drainage_mfd\w*_stripe\w*\b|\bnz_drainage_mfd\w*_rw\b", hdr)
    assert len(N.SIGNATURES["nz_drainage_mfd"][1]) == 8 and len(N.SIGNATURES["nz_drainage_mfd_batch"][1]) == 9
    # nz_drainage_mfd_desc field by field against the binding and the C# struct
    decl = re.search(r"typedef struct nz_drainage_mfd_desc \{(.*?)\} nz_drainage_mfd_desc;", hdr, re.S).group(1)
    decls = [" ".join(d.split()) for d in decl.split(";") if d.strip()]
    assert decls == ["float rain, seaLevel", "int32_t maxPasses", "int32_t exponent", "const float *rainMap"]
    assert N.DrainageMfdDesc._fields_ == [("rain", ctypes.c_float), ("seaLevel", ctypes.c_float), ("maxPasses", ctypes.c_int32),
                                          ("exponent", ctypes.c_int32), ("rainMap", ctypes.c_void_p)]
    assert ctypes.sizeof(N.DrainageMfdDesc) == 24 and N.DrainageMfdDesc.exponent.offset == 12 and N.DrainageMfdDesc.rainMap.offset == 16
    cs_body = re.search(r"public struct NzDrainageMfdDesc\s*\{(.*?)\}", read("host-cs", "Runtime.cs"), re.S).group(1)
    cs = [(t, n.strip()) for t, d in re.findall(r"public\s+(\w+)\s+([^;]+);", cs_body) for n in d.split(",")]
    assert cs == [("float", "rain"), ("float", "seaLevel"), ("int", "maxPasses"), ("int", "exponent"), ("IntPtr", "rainMap")]


def test_the_work_planes_are_the_head_eight_weight_planes_and_one_area_plane(nj):
    w, tree = nj._native.lib.nz_drainage_mfd_work_floats, nj._native.lib.nz_drainage_area_work_floats
    assert w(0, 1) == 0 and w(64, 0) == 0 and w(0, 0) == 0 and w(-3, 2) == 0 and w(8, -1) == 0
    for res, count in ((1, 1), (3, 1), (64, 1), (97, 3), (4096, 1), (512, 64)):
        n = res * res * count
        tiles = -(-res // 64) * -(-res // 16) * count
        head = 16 + 2 * (-(-tiles // 16) * 4)  # the status words and two generations of tile bytes, in floats
        assert w(res, count) == head + 9 * n, (res, count)
        assert w(res, count) - 9 * n == tree(res, count) - n - (-(-n // 16) * 4)  # the same head as the tree's
    assert w(64, 1) % 4 == 0  # the planes behind the head start 16-byte aligned


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES + (HOOK,):
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert "public static extern UIntPtr nz_drainage_mfd_work_floats(int resolution, int count);" in cs
    assert ("nz_drainage_mfd(IntPtr ctx, IntPtr height, IntPtr drainage, IntPtr work, ref NzDrainageMfdDesc desc, "
            "int resolution, ulong dep, out ulong @out)") in cs
    assert ("nz_drainage_mfd_batch(IntPtr ctx, IntPtr height, IntPtr drainage, IntPtr work, ref NzDrainageMfdDesc desc, "
            "int resolution, int count, ulong dep, IntPtr @out)") in cs  # the form the implicit stage chains without a handle
    assert '"nz_drainage_mfd_desc": "NzDrainageMfdDesc"' in read("tools", "gen_native_cs.py")


def test_the_three_hosts_carry_the_stage_with_the_same_defaults(nj):
    st = nj.MfdDrainageStage(None)
    assert isinstance(st, nj.DrainageAreaStage) and "MfdDrainageStage" in nj.__all__ and "FlowRouting" in nj.__all__
    assert (np.float32(st.rain), st.exponent, st.maxPasses, st.rainMap, st.out) == (np.float32(1.0), 1, None, None, None)
    assert np.float32(st.seaLevel) == -np.finfo(np.float32).max == np.float32(nj.DrainageAreaStage(None).seaLevel)
    assert (st.drainage, st.passes, st.converged) == (None, None, None)  # no payload yet
    other = nj.MfdDrainageStage(None, 0.5, 0.25, 4, 7, "a map", "a plane")  # the positional order of the signature
    assert (other.rain, other.seaLevel, other.exponent, other.maxPasses, other.rainMap, other.out) == (0.5, 0.25, 4, 7, "a map", "a plane")
    tree = nj.DrainageAreaStage(None, 0.5, 0.25, 7, "a map", "a plane")  # ... and DrainageAreaStage's is what it was
    assert (tree.rain, tree.seaLevel, tree.maxPasses, tree.rainMap, tree.out) == (0.5, 0.25, 7, "a map", "a plane")
    pipe = nj.BasePipeline([nj.NoiseStage(None, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300), nj.DepressionFillStage(None),
                            st, nj.StreamOrderStage(None)], "spread rivers")
    assert pipe is not None
    py = read("noize_job_amd", "pipeline.py")
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")
    assert re.search(r"class MfdDrainageStage\s*:\s*public PipelineStage", hpp)
    assert re.search(r"class MfdDrainageStage\s*:\s*PipelineStage", cs)
    bpy = body(py, "class MfdDrainageStage(", "\nclass ")
    bhpp = body(hpp, "class MfdDrainageStage ", "\nclass ")
    bcs = body(cs, "public class MfdDrainageStage ", "    public class ")
    # placed behind the drainage-area stage and in front of the watershed stage in each host
    for src, head in ((py, "class %s("), (hpp, "class %s "), (cs, "public class %s ")):
        assert src.index(head % "DrainageAreaStage") < src.index(head % "MfdDrainageStage") < src.index(head % "WatershedStage")
    # the same parameters in the same order, the same defaults, the same default budget, the same entries, the same members
    assert "rain=1.0, seaLevel=DrainageAreaStage.SEA_OFF, exponent=1, maxPasses=None, rainMap=None, out=None" in bpy
    assert "float rain = 1.f, seaLevel = -3.402823466e+38f;" in bhpp and "int exponent = 1;" in bhpp
    assert "const DeviceTile *rainMap = nullptr;" in bhpp and "DeviceTile *out = nullptr;" in bhpp
    assert "float rain = 1f, seaLevel = -float.MaxValue;" in bcs and "public int exponent = 1;" in bcs
    assert "DeviceTile rainMap = null;" in bcs and "DeviceTile @out = null;" in bcs
    assert "int? maxPasses = null;" in bcs and re.search(r"int maxPasses = 0;\s*// < 1: %s" % re.escape(BUDGET_C), bhpp)
    assert BUDGET_PY in bpy and BUDGET_C in bhpp and BUDGET_C in bcs
    assert "N.DrainageMfdDesc(self.rain, self.seaLevel, budget, self.exponent, rainMap)" in bpy
    for b, call in ((bpy, '"%s"'), (bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES:
            assert call % entry in b or (entry.endswith("work_floats") and entry + "(" in b), (entry, call)
        assert "nz_fluvial" not in b and "_rw" not in b and "nz_drainage_area" not in b  # no pair form, no erosion, not the tree
        assert not re.search(r"stripe\w*\(", b.lower())                                   # and no stripe form
    for b, members in ((nj.MfdDrainageStage, ("drainage", "passes", "converged")),):
        for m in members:
            assert isinstance(getattr(b, m), property), m
    for b, members in ((bhpp, ("drainage() const", "int passes() const", "bool converged() const")),
                       (bcs, ("DeviceTile Drainage", "int? Passes", "bool? Converged"))):
        for m in members:
            assert m in b, m
    # the header states the same defaults and says what is left out
    words = " ".join(body(read("include", "noize_hip.h"), "---- multiple-flow drainage:", "typedef struct nz_drainage_mfd_desc").split())
    words = words.replace(" * ", " ")
    assert "rain 1, seaLevel -FLT_MAX (off), exponent 1, maxPasses " + BUDGET_C in words
    for must in ("HEIGHT DIFFERENCES MUST BE FINITE", "no row-stripe form and no _rw form", "exponent outside 1..16",
                 "usable as nz_fluvial_implicit_desc.proceed", "The gate is w > 0, never the value of A"):
        assert must in words, must


def test_the_implicit_stage_routes_either_way_in_the_three_hosts(nj):
    st = nj.ImplicitFluvialStage(None)
    assert st.routing is nj.FlowRouting.Steepest and st.flowExponent == 1
    assert [(m.name, int(m)) for m in nj.FlowRouting] == [("Steepest", 0), ("Multiple", 1)]
    other = nj.ImplicitFluvialStage(None, 4, 0.1, 0.01, 250.0, 2.0, 0.25, 7, "a", "b", "c", nj.FlowRouting.Multiple, 4)
    assert (other.upliftMap, other.routing, other.flowExponent) == ("c", nj.FlowRouting.Multiple, 4)
    assert nj.ImplicitFluvialStage(None, routing=1).routing is nj.FlowRouting.Multiple
    py = read("noize_job_amd", "pipeline.py")
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")
    bpy = body(py, "class ImplicitFluvialStage(", "\nclass ")
    bhpp = body(hpp, "class ImplicitFluvialStage ", "\nclass ")
    bcs = body(cs, "public class ImplicitFluvialStage ", "    public class ")
    assert "upliftMap=None, routing=FlowRouting.Steepest, flowExponent=1):" in bpy
    assert "FlowRouting routing = FlowRouting::Steepest;" in bhpp and "int flowExponent = 1;" in bhpp
    assert "public FlowRouting routing = FlowRouting.Steepest;" in bcs and "public int flowExponent = 1;" in bcs
    assert "enum class FlowRouting { Steepest, Multiple };" in hpp and "public enum FlowRouting { Steepest = 0, Multiple = 1 }" in cs
    for b, call in ((bpy, '"%s"'), (bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ("nz_drainage_mfd", "nz_drainage_mfd_batch", "nz_drainage_area", "nz_drainage_area_batch"):
            assert call % entry in b, (entry, call)
        assert "nz_drainage_mfd_work_floats(" in b and "nz_drainage_area_work_floats(" in b
        assert BUDGET_PY in b or BUDGET_C in b
    # one proceed word whichever entry wrote it, and every host says that the solve keeps the steepest receiver
    assert bpy.count("self.drainageWork.ptr + 4") == 1 and bhpp.count("(drainageWork->ptr) + 1") == 1
    assert bcs.count("IntPtr.Add(drainageWork.Ptr, 4)") == 1
    for src, head in ((py, "class %s("), (hpp, "class %s "), (cs, "public class %s ")):
        i = src.index(head % "ImplicitFluvialStage")
        text = " ".join(src[max(0, i - 2500):i + 2500].replace("//", " ").split())
        assert "steepest receiver" in text and ("only the area" in text or "only the area A" in text.replace("Only", "only")), head


def test_the_documents_name_the_stage_and_the_tool_exists():
    readme = read("README.md")
    assert "MfdDrainageStage(" in readme and "nz_drainage_mfd" in readme and "tools/bench_drainage_mfd.py" in readme
    integ = read("INTEGRATION.md")
    assert "nz_drainage_mfd(" in integ and "nz_drainage_mfd_batch(" in integ and "NzDrainageMfdDesc" in integ
    design = read("DESIGN.md")
    assert "nz_drainage_mfd.hip" in design and "| f12 " in design and HOOK in design
    assert "MfdDrainageStage" in read("host-cs", "README.md")
    assert "MfdDrainageStage" in read("HISTORY.md") or "nz_drainage_mfd" in read("HISTORY.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_drainage_mfd.py"))
    assert "nz_drainage_mfd.hip" in read("noize_job_amd", "csrc", "Makefile")
