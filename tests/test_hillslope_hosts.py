"""The hillslope diffusion stage across the ABI and the three hosts, without a GPU: the header declares the entries and
nz_hillslope_desc, the library exports them, and the Python binding, Native.cs / Runtime.cs, Stages.cs and noize_pipeline.hpp
each carry the stage with the same parameters, defaults, positional order and entries."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_hillslope_diffusion_work_floats", "nz_hillslope_diffusion", "nz_hillslope_diffusion_batch")


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
    assert "size_t nz_hillslope_diffusion_work_floats(int32_t resolution, int32_t count);" in flat
    assert ("int32_t nz_hillslope_diffusion(nz_ctx *ctx, const float *height, float *out, float *work, "
            "const nz_hillslope_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out_handle);") in flat
    assert ("int32_t nz_hillslope_diffusion_batch(nz_ctx *ctx, const float *height, float *out, float *work, "
            "const nz_hillslope_desc *desc, int32_t resolution, int32_t count, nz_handle dep, nz_handle *out_handle);") in flat
    assert not re.search(r"\bnz_hillslope\w*_stripe\w*\b|\bnz_hillslope\w*_rw\b|\bnz_debug_hillslope", hdr)
    assert len(N.SIGNATURES["nz_hillslope_diffusion"][1]) == 8 and len(N.SIGNATURES["nz_hillslope_diffusion_batch"][1]) == 9
    assert lib.nz_version() == 100
    # nz_hillslope_desc field by field against the binding and the C# struct
    body = re.search(r"typedef struct nz_hillslope_desc \{(.*?)\} nz_hillslope_desc;", hdr, re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["float diffusivity, dt", "int32_t iterations"]
    assert N.HillslopeDesc._fields_ == [("diffusivity", ctypes.c_float), ("dt", ctypes.c_float), ("iterations", ctypes.c_int32)]
    assert ctypes.sizeof(N.HillslopeDesc) == 12 and N.HillslopeDesc.iterations.offset == 8
    cs_body = re.search(r"public struct NzHillslopeDesc\s*\{(.*?)\}", read("host-cs", "Runtime.cs"), re.S).group(1)
    cs = [(t, n.strip()) for t, d in re.findall(r"public\s+(\w+)\s+([^;]+);", cs_body) for n in d.split(",")]
    assert cs == [("float", "diffusivity"), ("float", "dt"), ("int", "iterations")]


def test_the_work_planes_are_the_two_tables(nj):
    w = nj._native.lib.nz_hillslope_diffusion_work_floats
    assert w(0, 1) == 0 and w(64, 0) == 0 and w(0, 0) == 0 and w(-3, 2) == 0 and w(8, -1) == 0
    for res, count in ((1, 1), (3, 1), (64, 1), (97, 3), (4096, 1), (512, 64)):
        assert 2 * res <= w(res, count) <= 2 * res + 8, (res, count)  # inv and cp, one entry per line position each
        assert w(res, count) == w(res, 1)                              # shared by the tiles of a batch


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES:
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert "public static extern UIntPtr nz_hillslope_diffusion_work_floats(int resolution, int count);" in cs
    assert ("nz_hillslope_diffusion(IntPtr ctx, IntPtr height, IntPtr @out, IntPtr work, ref NzHillslopeDesc desc, "
            "int resolution, ulong dep, out ulong out_handle)") in cs
    assert ("nz_hillslope_diffusion_batch(IntPtr ctx, IntPtr height, IntPtr @out, IntPtr work, ref NzHillslopeDesc desc, "
            "int resolution, int count, ulong dep, out ulong out_handle)") in cs
    assert '"nz_hillslope_desc": "NzHillslopeDesc"' in read("tools", "gen_native_cs.py")


def test_the_three_hosts_carry_the_stage_with_the_same_defaults(nj):
    st = nj.HillslopeDiffusionStage(None)
    assert isinstance(st, nj.PipelineStage) and "HillslopeDiffusionStage" in nj.__all__
    assert (st.diffusivity, st.dt, st.iterations, st.work) == (0.01, 1.0, 1, None)
    other = nj.HillslopeDiffusionStage(None, 0.5, 250.0, 4)  # the positional order of the signature
    assert (other.diffusivity, other.dt, other.iterations) == (0.5, 250.0, 4)
    pipe = nj.BasePipeline([nj.DepressionFillStage(None), nj.ImplicitFluvialStage(None, dt=100.0),
                            nj.HillslopeDiffusionStage(None, dt=100.0)], "evolve")
    assert pipe is not None
    py = read("noize_job_amd", "pipeline.py")
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")
    assert re.search(r"class HillslopeDiffusionStage\s*:\s*public PipelineStage", hpp)
    assert re.search(r"class HillslopeDiffusionStage\s*:\s*PipelineStage", cs)

    def body(src, head, nxt):
        i = src.index(head)
        return src[i:src.index(nxt, i + 1)]

    bpy = body(py, "class HillslopeDiffusionStage(", "\nclass ")
    bhpp = body(hpp, "class HillslopeDiffusionStage ", "\nclass ")
    bcs = body(cs, "public class HillslopeDiffusionStage ", "    public class ")
    # placed behind the implicit fluvial stage and in front of the mesh stage in each host
    for src, head in ((py, "class %s("), (hpp, "class %s "), (cs, "public class %s ")):
        assert src.index(head % "ImplicitFluvialStage") < src.index(head % "HillslopeDiffusionStage") < src.index(head % "MeshTileStage")
    # the same parameters in the same order, the same defaults, the same entries
    assert "def __init__(self, ctx, diffusivity=0.01, dt=1.0, iterations=1):" in bpy
    assert "float diffusivity = .01f, dt = 1.f;" in bhpp and "int iterations = 1;" in bhpp
    assert "public float diffusivity = 0.01f, dt = 1f;" in bcs and "public int iterations = 1;" in bcs
    assert "nz_hillslope_desc desc{diffusivity, dt, iterations}" in bhpp
    assert "N.HillslopeDesc(self.diffusivity, self.dt, self.iterations)" in bpy
    assert "diffusivity = diffusivity, dt = dt, iterations = iterations" in bcs
    for b, call in ((bpy, '"%s"'), (bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES:
            assert call % entry in b or (entry.endswith("work_floats") and entry + "(" in b), (entry, call)
        assert "stripe" not in b.lower() and "_rw" not in b
    # in place on the payload's data: the plane goes in as `height` and as `out`
    assert "d.data.ptr,\n" in bpy and bpy.count("d.data.ptr") == 2
    assert bhpp.count("d->data->ptr, d->data->ptr, work->ptr") == 2 and bcs.count("d.data.Ptr, d.data.Ptr, work.Ptr") == 2
    # the defaults are a choice, and every host says so (the C++ and C# hosts document a stage above its class line)
    for src, head in ((py, "class %s("), (hpp, "class %s "), (cs, "public class %s ")):
        i = src.index(head % "HillslopeDiffusionStage")
        assert "a choice, not pinned by any picture" in " ".join(src[max(0, i - 1500):i + 1500].replace("//", " ").split())
    # the header states the same defaults and the limits
    words = " ".join(body(read("include", "noize_hip.h"), "---- hillslope diffusion:", "typedef struct nz_hillslope_desc").split())
    assert "diffusivity 0.01, dt 1, iterations 1" in words.replace(" * ", " ")
    for must in ("border cells keep their bits", "No sea-level cells are held", "no per-cell diffusivity map", "no row-stripe form",
                 "flip the sign"):
        assert must in words.replace(" * ", " "), must


def test_the_documents_name_the_stage_and_the_tool_exists():
    readme = read("README.md")
    assert "HillslopeDiffusionStage(" in readme and "nz_hillslope" in readme and "tools/bench_hillslope.py" in readme
    integ = read("INTEGRATION.md")
    assert "nz_hillslope_diffusion(" in integ and "nz_hillslope_diffusion_batch(" in integ and "NzHillslopeDesc" in integ
    design = read("DESIGN.md")
    assert "nz_hillslope.hip" in design and "| f11 " in design
    assert "HillslopeDiffusionStage" in read("host-cs", "README.md")
    assert "HillslopeDiffusionStage" in read("HISTORY.md") or "nz_hillslope_diffusion" in read("HISTORY.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_hillslope.py"))
    assert "nz_hillslope.hip" in read("noize_job_amd", "csrc", "Makefile")
