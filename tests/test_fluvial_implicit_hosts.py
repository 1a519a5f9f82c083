"""The implicit fluvial stage across the ABI and the three hosts, without a GPU: the header declares the entries and
nz_fluvial_implicit_desc, the library exports them, and the Python binding, Native.cs / Runtime.cs, Stages.cs and
noize_pipeline.hpp each carry the stage with the same parameters, defaults, default budget, entries and members."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_fluvial_implicit_work_floats", "nz_fluvial_implicit", "nz_fluvial_implicit_batch")
HOOK = "nz_debug_fluvial_implicit_sweeps"
FLOATS = ["erodibility", "uplift", "dt", "seaLevel"]
POINTERS = ["hardness", "upliftMap", "proceed", "tally"]
BUDGET_PY, BUDGET_C = "64 + self.resolution // 4", "64 + resolution / 4"
# what one iteration of the stage calls besides its own entry, in every host
CHAIN = ("nz_tile_upload", "nz_drainage_area", "nz_drainage_area_batch", "nz_flush_write_slice")


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_header_declares_the_entries_and_the_library_exports_them(nj):
    N = nj._native
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "noize_hip.h"), flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES + (HOOK,):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    flat = " ".join(hdr.split())
    assert "size_t nz_fluvial_implicit_work_floats(int32_t resolution, int32_t count);" in flat
    assert ("int32_t nz_fluvial_implicit(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work, "
            "const nz_fluvial_implicit_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out_handle);") in flat
    assert ("int32_t nz_fluvial_implicit_batch(nz_ctx *ctx, const float *height, const float *drainage, float *out, "
            "float *work, const nz_fluvial_implicit_desc *desc, int32_t resolution, int32_t count, nz_handle dep, "
            "nz_handle *out_handle);") in flat
    assert "int32_t %s(int32_t sweeps);" % HOOK in flat
    assert not re.search(r"\bnz_fluvial_implicit_stripe\w*\b|\bnz_fluvial_implicit_rw\b", hdr)  # not built, DESIGN.md section 9
    assert len(N.SIGNATURES["nz_fluvial_implicit"][1]) == 9 and len(N.SIGNATURES["nz_fluvial_implicit_batch"][1]) == 10
    # nz_fluvial_implicit_desc field by field against the binding and the C# struct
    body = re.search(r"typedef struct nz_fluvial_implicit_desc \{(.*?)\} nz_fluvial_implicit_desc;", hdr, re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["float erodibility, uplift, dt, seaLevel", "int32_t maxPasses", "const float *hardness",
                     "const float *upliftMap", "const int32_t *proceed", "int32_t *tally"]
    assert [f[0] for f in N.FluvialImplicitDesc._fields_] == FLOATS + ["maxPasses"] + POINTERS
    assert [f[1] for f in N.FluvialImplicitDesc._fields_] == [ctypes.c_float] * 4 + [ctypes.c_int32] + [ctypes.c_void_p] * 4
    assert ctypes.sizeof(N.FluvialImplicitDesc) == 56 and N.FluvialImplicitDesc.hardness.offset == 24
    cs_body = re.search(r"public struct NzFluvialImplicitDesc\s*\{(.*?)\}", read("host-cs", "Runtime.cs"), re.S).group(1)
    cs = [(t, n.strip()) for t, d in re.findall(r"public\s+(\w+)\s+([^;]+);", cs_body) for n in d.split(",")]
    assert cs == [("float", n) for n in FLOATS] + [("int", "maxPasses")] + [("IntPtr", n) for n in POINTERS]


def test_the_work_planes_have_a_floor_and_a_ceiling(nj):
    # at least the receiver bytes, b, f and the second h' plane; on top of that no more than the header, the tile bytes
    # and slack
    w = nj._native.lib.nz_fluvial_implicit_work_floats
    assert w(0, 1) == 0 and w(64, 0) == 0 and w(0, 0) == 0 and w(-3, 2) == 0 and w(8, -1) == 0
    for res, count in ((1, 1), (64, 1), (97, 3), (4096, 1)):
        n = res * res * count
        tiles = -(-res // 64) * -(-res // 16) * count
        floor = 3 * n + -(-n // 4)
        assert floor <= w(res, count) <= floor + 16 + 2 * (tiles + 15) // 4 + 12, (res, count)
    assert w(97, 3) > 3 * w(97, 1) - 3 * 16  # a batch is its tiles back to back, one header


def test_the_sweep_hook_is_this_stage_s_own(nj):
    lib = nj._native.lib
    others = ("nz_debug_fill_sweeps", "nz_debug_drainage_sweeps", "nz_debug_watershed_sweeps", "nz_debug_stream_order_sweeps")
    before = [getattr(lib, o)(0) for o in others]
    hook = getattr(lib, HOOK)
    d = hook(5)
    assert d == 16 and hook(0) == 5 and hook(0) == d
    assert hook(-2) == d and hook(0) == d
    assert [getattr(lib, o)(0) for o in others] == before  # it does not disturb the other four
    getattr(lib, others[2])(3)
    assert hook(0) == d and getattr(lib, others[2])(0) == 3  # ... nor they it
    assert lib.nz_version() == 100


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES + (HOOK,):
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert "public static extern UIntPtr nz_fluvial_implicit_work_floats(int resolution, int count);" in cs
    assert ("nz_fluvial_implicit_batch(IntPtr ctx, IntPtr height, IntPtr drainage, IntPtr @out, IntPtr work, "
            "ref NzFluvialImplicitDesc desc, int resolution, int count, ulong dep, out ulong out_handle)") in cs
    assert '"nz_fluvial_implicit_desc": "NzFluvialImplicitDesc"' in read("tools", "gen_native_cs.py")


def test_the_three_hosts_carry_the_stage_with_the_same_defaults(nj):
    st = nj.ImplicitFluvialStage(None)
    assert isinstance(st, nj.PipelineStage) and "ImplicitFluvialStage" in nj.__all__
    got = (st.iterations, st.erodibility, st.uplift, st.dt, st.rain, st.maxPasses, st.rainMap, st.hardness, st.upliftMap)
    assert got == (1, 0.05, 0.002, 1.0, 1.0, None, None, None, None)
    assert np.float32(st.seaLevel) == -np.finfo(np.float32).max == np.float32(nj.FluvialErosionStage(None).seaLevel)
    assert (st.drainage, st.steps, st.passes, st.converged) == (None, None, None, None)  # no payload yet
    a, b, c = object(), object(), object()
    other = nj.ImplicitFluvialStage(None, 4, 0.1, 0.01, 250.0, 2.0, 0.25, 7, a, b, c)  # the positional order of the signature
    assert (other.iterations, other.erodibility, other.uplift, other.dt, other.rain, other.seaLevel, other.maxPasses) == \
        (4, 0.1, 0.01, 250.0, 2.0, 0.25, 7)
    assert (other.rainMap, other.hardness, other.upliftMap) == (a, b, c)
    pipe = nj.BasePipeline([nj.NoiseStage(None, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300),
                            nj.DepressionFillStage(None), st], "valleys")
    assert pipe is not None
    py = read("noize_job_amd", "pipeline.py")
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")
    assert re.search(r"class ImplicitFluvialStage\s*:\s*public PipelineStage", hpp)
    assert re.search(r"class ImplicitFluvialStage\s*:\s*PipelineStage", cs)

    def body(src, head, nxt):
        i = src.index(head)
        return src[i:src.index(nxt, i + 1)]

    bpy = body(py, "class ImplicitFluvialStage(", "\nclass ")
    bhpp = body(hpp, "class ImplicitFluvialStage ", "\nclass ")
    bcs = body(cs, "public class ImplicitFluvialStage ", "    public class ")
    # placed behind the stream-order stage and in front of the mesh stage in each host
    for src, head in ((py, "class %s("), (hpp, "class %s "), (cs, "public class %s ")):
        assert src.index(head % "StreamOrderStage") < src.index(head % "ImplicitFluvialStage") < src.index(head % "MeshTileStage")
    # the same parameters, the same defaults, the same default budget, the same entries, the same members
    assert ("iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=SEA_OFF, maxPasses=None,"
            in " ".join(bpy.split()))
    assert "rainMap=None, hardness=None, upliftMap=None" in bpy
    assert "int iterations = 1;" in bhpp and "public int iterations = 1;" in bcs
    assert "float erodibility = .05f, uplift = .002f, dt = 1.f, rain = 1.f, seaLevel = -3.402823466e+38f;" in bhpp
    assert "float erodibility = 0.05f, uplift = 0.002f, dt = 1f, rain = 1f, seaLevel = -float.MaxValue;" in bcs
    assert "*rainMap = nullptr, *hardness = nullptr, *upliftMap = nullptr;" in bhpp
    assert "DeviceTile rainMap = null, hardness = null, upliftMap = null;" in bcs
    assert "int? maxPasses = null;" in bcs and re.search(r"int maxPasses = 0;\s*// < 1: %s" % re.escape(BUDGET_C), bhpp)
    assert BUDGET_PY in bpy and BUDGET_C in bhpp and BUDGET_C in bcs
    for b, call in ((bpy, '"%s"'), (bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES + CHAIN:
            assert call % entry in b or (entry.endswith("work_floats") and entry + "(" in b), (entry, call)
        assert "nz_drainage_area_work_floats(" in b
        # no pair form and no stripe form, and the explicit stage's entries stay where they are
        assert "_rw" not in b and "stripe" not in b.lower() and not re.search(r"nz_fluvial_erosion\w*\(", b)
    # the solve is told to proceed by the drainage call's converged word, the second int32 of its work planes
    assert "self.drainageWork.ptr + 4" in bpy and "(drainageWork->ptr) + 1" in bhpp and "IntPtr.Add(drainageWork.Ptr, 4)" in bcs
    for b, members in ((bpy, ("def drainage", "def steps", "def passes", "def converged")),
                       (bhpp, ("drainage() const", "int steps() const", "int passes() const", "bool converged() const")),
                       (bcs, ("DeviceTile Drainage", "int? Steps", "int? Passes", "bool? Converged"))):
        for m in members:
            assert m in b, m
    # the header states the same defaults
    words = " ".join(body(read("include", "noize_hip.h"), "---- implicit fluvial erosion:",
                          "typedef struct nz_fluvial_implicit_desc").split())
    assert "iterations 1, erodibility 0.05, uplift 0.002, dt 1, rain 1" in words and ("maxPasses " + BUDGET_C) in words
    for must in ("overflows", "finite and >= 0", "pits stay pits"):  # said plainly
        assert must in words, must


def test_the_documents_name_the_stage_and_the_tool_exists():
    readme = read("README.md")
    assert "ImplicitFluvialStage(" in readme and "nz_fluvial_implicit" in readme
    integ = read("INTEGRATION.md")
    assert "nz_fluvial_implicit(" in integ and "nz_fluvial_implicit_batch(" in integ and "NzFluvialImplicitDesc" in integ
    design = read("DESIGN.md")
    assert "nz_fluvial_implicit.hip" in design and "| f10 " in design and HOOK in design
    assert "ImplicitFluvialStage" in read("host-cs", "README.md")
    assert "ImplicitFluvialStage" in read("HISTORY.md") or "nz_fluvial_implicit" in read("HISTORY.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_fluvial_implicit.py"))
    mk = read("noize_job_amd", "csrc", "Makefile")
    assert "nz_fluvial_implicit.hip" in mk
    for hdr in ("nz_receiver.hpp", "nz_donor_front.hpp", "nz_tile64.hpp", "nz_relax_pass.hpp"):
        assert re.search(r"build/nz_fluvial_implicit\.o[^\n]*: %s" % re.escape(hdr), mk), hdr
