"""The watershed stage across the ABI and the three hosts, without a GPU: the header declares the entries and
nz_watershed_desc, the library exports them, and the Python binding, Native.cs / Runtime.cs, Stages.cs and
noize_pipeline.hpp each carry the stage with the same parameters, defaults, default budget, entries and members."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_watershed_work_floats", "nz_watershed", "nz_watershed_batch")
FIELDS = ["seaLevel", "cellSize", "maxPasses"]
BUDGET_PY, BUDGET_C = "64 + self.resolution // 4", "64 + resolution / 4"  # the measured default, DESIGN.md section 4


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_header_declares_the_entries_and_the_library_exports_them(nj):
    N = nj._native
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "noize_hip.h"), flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES + ("nz_debug_watershed_sweeps",):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    flat = " ".join(hdr.split())
    assert "size_t nz_watershed_work_floats(int32_t resolution, int32_t count, int32_t withLength);" in flat
    assert ("int32_t nz_watershed(nz_ctx *ctx, const float *height, int32_t *basin, float *length, uint8_t *receivers, "
            "float *work, const nz_watershed_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out);") in flat
    assert ("int32_t nz_watershed_batch(nz_ctx *ctx, const float *height, int32_t *basin, float *length, "
            "uint8_t *receivers, float *work, const nz_watershed_desc *desc, int32_t resolution, int32_t count, "
            "nz_handle dep, nz_handle *out);") in flat
    assert "int32_t nz_debug_watershed_sweeps(int32_t sweeps);" in flat
    assert not re.search(r"\bnz_watershed_stripe\w*\b|\bnz_watershed_rw\b", hdr)  # follow-ups, DESIGN.md section 9
    assert len(N.SIGNATURES["nz_watershed"][1]) == 10 and len(N.SIGNATURES["nz_watershed_batch"][1]) == 11
    # nz_watershed_desc field by field against the binding and the C# struct
    body = re.search(r"typedef struct nz_watershed_desc \{(.*?)\} nz_watershed_desc;", hdr, re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["float seaLevel, cellSize", "int32_t maxPasses"]
    assert [f[0] for f in N.WatershedDesc._fields_] == FIELDS
    assert [f[1] for f in N.WatershedDesc._fields_] == [ctypes.c_float, ctypes.c_float, ctypes.c_int32]
    assert ctypes.sizeof(N.WatershedDesc) == 12
    cs_body = re.search(r"public struct NzWatershedDesc\s*\{(.*?)\}", read("host-cs", "Runtime.cs"), re.S).group(1)
    cs = [(t, n.strip()) for t, d in re.findall(r"public\s+(\w+)\s+([^;]+);", cs_body) for n in d.split(",")]
    assert cs == [("float", "seaLevel"), ("float", "cellSize"), ("int", "maxPasses")]
    # the work planes: at least the second planes and the receiver bytes; on top of that no more than the header, the tile
    # bytes and slack
    w = N.lib.nz_watershed_work_floats
    for wl in (0, 1):
        assert w(0, 1, wl) == 0 and w(64, 0, wl) == 0 and w(0, 0, wl) == 0 and w(-3, 2, wl) == 0 and w(8, -1, wl) == 0
        for res, count in ((1, 1), (64, 1), (97, 3), (4096, 1)):
            n = res * res * count
            tiles = -(-res // 64) * -(-res // 16) * count
            floor = (1 + wl) * n + -(-n // 4)
            assert floor <= w(res, count, wl) <= floor + 16 + 2 * (tiles + 15) // 4 + 12, (res, count, wl)
    assert w(97, 3, 1) - w(97, 3, 0) == 97 * 97 * 3 and w(64, 1, 7) == w(64, 1, 1)
    # the sweep hook hands back the cap that was in force and restores the default on 0; it is not the drainage stage's
    d = N.lib.nz_debug_watershed_sweeps(5)
    a = N.lib.nz_debug_drainage_sweeps(0)
    f = N.lib.nz_debug_fill_sweeps(0)
    assert d >= 1 and N.lib.nz_debug_watershed_sweeps(0) == 5 and N.lib.nz_debug_watershed_sweeps(0) == d
    assert N.lib.nz_debug_watershed_sweeps(-2) == d and N.lib.nz_debug_watershed_sweeps(0) == d
    assert N.lib.nz_debug_drainage_sweeps(0) == a and N.lib.nz_debug_fill_sweeps(0) == f
    assert N.lib.nz_version() == 100


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES + ("nz_debug_watershed_sweeps",):
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert "public static extern UIntPtr nz_watershed_work_floats(int resolution, int count, int withLength);" in cs
    assert ("nz_watershed_batch(IntPtr ctx, IntPtr height, IntPtr basin, IntPtr length, IntPtr receivers, IntPtr work, "
            "ref NzWatershedDesc desc, int resolution, int count, ulong dep, out ulong @out)") in cs
    assert '"nz_watershed_desc": "NzWatershedDesc"' in read("tools", "gen_native_cs.py")


def test_the_three_hosts_carry_the_stage_with_the_same_defaults(nj):
    st = nj.WatershedStage(None)
    assert isinstance(st, nj.PipelineStage) and "WatershedStage" in nj.__all__
    assert (np.float32(st.cellSize), st.maxPasses, st.withLength, st.recordReceivers) == (np.float32(1.0), None, True, False)
    assert np.float32(st.seaLevel) == -np.finfo(np.float32).max == np.float32(nj.DrainageAreaStage(None).seaLevel)
    assert (st.basin, st.length, st.receivers, st.passes, st.converged) == (None, None, None, None, None)  # no payload yet
    other = nj.WatershedStage(None, 0.25, 2.5, 7, False, True)  # the positional order of the signature
    assert (other.seaLevel, other.cellSize, other.maxPasses, other.withLength, other.recordReceivers) == (0.25, 2.5, 7, False, True)
    pipe = nj.BasePipeline([nj.NoiseStage(None, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300),
                            nj.DepressionFillStage(None), nj.DrainageAreaStage(None), st], "basins")
    assert pipe is not None
    py = read("noize_job_amd", "pipeline.py")
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")
    assert re.search(r"class WatershedStage\s*:\s*public PipelineStage", hpp)
    assert re.search(r"class WatershedStage\s*:\s*PipelineStage", cs)

    def body(src, head, nxt):
        i = src.index(head)
        return src[i:src.index(nxt, i + 1)]

    bpy = body(py, "class WatershedStage(", "\nclass ")
    bhpp = body(hpp, "class WatershedStage ", "\nclass ")
    bcs = body(cs, "public class WatershedStage ", "    public class ")
    # placed behind the drainage stage in each host
    for src, head in ((py, "class %s("), (hpp, "class %s "), (cs, "public class %s ")):
        assert src.index(head % "DrainageAreaStage") < src.index(head % "WatershedStage") < src.index(head % "MeshTileStage")
    # the same parameters, the same defaults, the same default budget, the same entries, the same members
    assert "seaLevel=SEA_OFF, cellSize=1.0, maxPasses=None, length=True, recordReceivers=False" in bpy
    assert "float seaLevel = -3.402823466e+38f, cellSize = 1.f;" in bhpp
    assert "bool length = true;" in bhpp and "bool recordReceivers = false;" in bhpp
    assert "float seaLevel = -float.MaxValue, cellSize = 1f;" in bcs
    assert "bool length = true;" in bcs and "bool recordReceivers = false;" in bcs
    assert "int? maxPasses = null;" in bcs and re.search(r"int maxPasses = 0;\s*// < 1: %s" % re.escape(BUDGET_C), bhpp)
    assert BUDGET_PY in bpy and BUDGET_C in bhpp and BUDGET_C in bcs
    for b, call in ((bpy, '"%s"'), (bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES:
            assert call % entry in b or (entry.endswith("work_floats") and entry + "(" in b), (entry, call)
        # the heights pass through: no pair form, no erosion, and none of the other stages' entries
        assert "_rw" not in b and not re.search(r"nz_(fluvial|drainage|fill)\w*\(", b)
    assert "dtype=np.int32" in bpy  # the labels are handed out as an int32 view
    for b, members in ((bpy, ("def basin", "def length", "def receivers", "def passes", "def converged")),
                       (bhpp, ("basin() const", "flowLength() const", "receivers() const", "int passes() const",
                               "bool converged() const")),
                       (bcs, ("DeviceTile Basin", "DeviceTile Length", "DeviceTile Receivers", "int? Passes", "bool? Converged"))):
        for m in members:
            assert m in b, m
    # the header states the same default
    assert ("maxPasses " + BUDGET_C) in " ".join(body(read("include", "noize_hip.h"), "---- watershed:", "typedef struct nz_watershed_desc").split())


def test_the_documents_name_the_stage_and_the_tool_exists():
    readme = read("README.md")
    assert "WatershedStage(ctx" in readme and "nz_watershed" in readme
    integ = read("INTEGRATION.md")
    assert "nz_watershed(" in integ and "nz_watershed_batch(" in integ and "NzWatershedDesc" in integ
    design = read("DESIGN.md")
    assert "nz_watershed.hip" in design and "| f8 " in design and "nz_debug_watershed_sweeps" in design
    assert "has no receiver-code output" not in design  # the limit of section 9 is lifted
    assert "WatershedStage" in read("HISTORY.md") or "nz_watershed" in read("HISTORY.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_watershed.py"))
    mk = read("noize_job_amd", "csrc", "Makefile")
    assert "nz_watershed.hip" in mk
    for hdr in ("nz_receiver.hpp", "nz_tile64.hpp", "nz_relax_pass.hpp"):
        assert re.search(r"build/nz_watershed\.o[^\n]*: %s" % re.escape(hdr), mk), hdr
