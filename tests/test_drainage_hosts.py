"""The drainage-area stage across the ABI and the three hosts, without a GPU: the header declares the entries and
nz_drainage_desc, the library exports them, and the Python binding, Native.cs / Runtime.cs, Stages.cs and
noize_pipeline.hpp each carry the stage with the same parameters, defaults, default budget, entries and members."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_drainage_area_work_floats", "nz_drainage_area", "nz_drainage_area_batch")
FIELDS = ["rain", "seaLevel", "maxPasses", "rainMap"]
BUDGET_PY, BUDGET_C = "64 + self.resolution // 4", "64 + resolution / 4"  # the measured default, DESIGN.md section 4


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_header_declares_the_entries_and_the_library_exports_them(nj):
    N = nj._native
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "noize_hip.h"), flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES + ("nz_debug_drainage_sweeps",):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    flat = " ".join(hdr.split())
    assert "size_t nz_drainage_area_work_floats(int32_t resolution, int32_t count);" in flat
    assert ("int32_t nz_drainage_area(nz_ctx *ctx, const float *height, float *drainage, float *work, "
            "const nz_drainage_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out);") in flat
    assert ("int32_t nz_drainage_area_batch(nz_ctx *ctx, const float *height, float *drainage, float *work, "
            "const nz_drainage_desc *desc, int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);") in flat
    assert "int32_t nz_debug_drainage_sweeps(int32_t sweeps);" in flat
    assert not re.search(r"\bnz_drainage_area_rw\b|\bnz_drainage_stripe\b", hdr)  # follow-ups, DESIGN.md section 9
    # nz_drainage_desc field by field against the binding and the C# struct
    body = re.search(r"typedef struct nz_drainage_desc \{(.*?)\} nz_drainage_desc;", hdr, re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["float rain, seaLevel", "int32_t maxPasses", "const float *rainMap"]
    assert [f[0] for f in N.DrainageDesc._fields_] == FIELDS
    assert [f[1] for f in N.DrainageDesc._fields_] == [ctypes.c_float, ctypes.c_float, ctypes.c_int32, ctypes.c_void_p]
    assert ctypes.sizeof(N.DrainageDesc) == 16 + ctypes.sizeof(ctypes.c_void_p)  # 12 bytes of scalars, padded to the pointer
    cs_body = re.search(r"public struct NzDrainageDesc\s*\{(.*?)\}", read("host-cs", "Runtime.cs"), re.S).group(1)
    cs = [(t, n.strip()) for t, d in re.findall(r"public\s+(\w+)\s+([^;]+);", cs_body) for n in d.split(",")]
    assert cs == [("float", "rain"), ("float", "seaLevel"), ("int", "maxPasses"), ("IntPtr", "rainMap")]
    # the work planes: at least one plane and the donor bytes; on top of that no more than the header, the tile bytes and slack
    w = N.lib.nz_drainage_area_work_floats
    assert w(0, 1) == 0 and w(64, 0) == 0 and w(0, 0) == 0
    for res, count in ((1, 1), (64, 1), (97, 3), (4096, 1)):
        n = res * res * count
        tiles = -(-res // 64) * -(-res // 16) * count
        floor = n + -(-n // 4)
        assert floor <= w(res, count) <= floor + 16 + 2 * (tiles + 15) // 4 + 12, (res, count)
    # the sweep hook hands back the cap that was in force and restores the default on 0; it is not the fill stage's
    d = N.lib.nz_debug_drainage_sweeps(5)
    f = N.lib.nz_debug_fill_sweeps(0)
    assert d >= 1 and N.lib.nz_debug_drainage_sweeps(0) == 5 and N.lib.nz_debug_drainage_sweeps(0) == d
    assert N.lib.nz_debug_fill_sweeps(0) == f


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES + ("nz_debug_drainage_sweeps",):
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert ("nz_drainage_area_batch(IntPtr ctx, IntPtr height, IntPtr drainage, IntPtr work, ref NzDrainageDesc desc, "
            "int resolution, int count, ulong dep, out ulong @out)") in cs


def test_the_three_hosts_carry_the_stage_with_the_same_defaults(nj):
    st = nj.DrainageAreaStage(None)
    assert isinstance(st, nj.PipelineStage)
    assert (np.float32(st.rain), st.maxPasses, st.rainMap, st.out) == (np.float32(1.0), None, None, None)
    assert np.float32(st.seaLevel) == -np.finfo(np.float32).max == np.float32(nj.FluvialErosionStage(None).seaLevel)
    assert (st.drainage, st.passes, st.converged) == (None, None, None)  # no payload yet
    other = nj.DrainageAreaStage(None, 0.5, 0.25, 7, "a map", "a plane")  # the positional order of the signature
    assert (other.rain, other.seaLevel, other.maxPasses, other.rainMap, other.out) == (0.5, 0.25, 7, "a map", "a plane")
    pipe = nj.BasePipeline([nj.NoiseStage(None, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300),
                            nj.DepressionFillStage(None), st, nj.FluvialErosionStage(None)], "rivers")
    assert pipe is not None
    py = read("noize_job_amd", "pipeline.py")
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")
    assert re.search(r"class DrainageAreaStage\s*:\s*public PipelineStage", hpp)
    assert re.search(r"class DrainageAreaStage\s*:\s*PipelineStage", cs)

    def body(src, head, nxt):
        i = src.index(head)
        return src[i:src.index(nxt, i + 1)]

    bpy = body(py, "class DrainageAreaStage(", "\nclass ")
    bhpp = body(hpp, "class DrainageAreaStage ", "\nclass ")
    bcs = body(cs, "public class DrainageAreaStage ", "    public class ")
    # the same parameters, the same defaults, the same default budget, the same entries, the same members
    assert "rain=1.0, seaLevel=SEA_OFF, maxPasses=None, rainMap=None, out=None" in bpy
    assert "float rain = 1.f, seaLevel = -3.402823466e+38f;" in bhpp
    assert "const DeviceTile *rainMap = nullptr;" in bhpp and "DeviceTile *out = nullptr;" in bhpp
    assert "float rain = 1f, seaLevel = -float.MaxValue;" in bcs
    assert "DeviceTile rainMap = null;" in bcs and "DeviceTile @out = null;" in bcs
    assert "int? maxPasses = null;" in bcs and re.search(r"int maxPasses = 0;\s*// < 1: %s" % re.escape(BUDGET_C), bhpp)
    assert BUDGET_PY in bpy and BUDGET_C in bhpp and BUDGET_C in bcs
    for b, call in ((bpy, '"%s"'), (bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES:
            assert call % entry in b or (entry.endswith("work_floats") and entry + "(" in b), (entry, call)
        assert "nz_fluvial" not in b and "_rw" not in b  # the heights pass through: no pair form, and no erosion
    for b, members in ((bpy, ("def drainage", "def passes", "def converged")),
                       (bhpp, ("drainage() const", "int passes() const", "bool converged() const")),
                       (bcs, ("DeviceTile Drainage", "int? Passes", "bool? Converged"))):
        for m in members:
            assert m in b, m
    # the header states the same default; the fluvial stage is what it was
    assert ("maxPasses " + BUDGET_C) in " ".join(read("include", "noize_hip.h").split())
    assert "drainageIn=None" in body(py, "class FluvialErosionStage(", "\nclass ")
    # the documents name the stage
    readme = read("README.md")
    assert "DrainageAreaStage(ctx" in readme and "drainageIn=" in readme
    assert "nz_drainage_area" in read("INTEGRATION.md")
    design = read("DESIGN.md")
    assert "nz_drainage.hip" in design and "| f7 " in design
    assert "DrainageAreaStage" in read("HISTORY.md") or "nz_drainage_area" in read("HISTORY.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_drainage.py"))
