"""The depression-filling stage across the ABI and the three hosts, without a GPU: the header declares the entries and
nz_fill_desc, the library exports them, and the Python binding, Native.cs / Runtime.cs, Stages.cs and noize_pipeline.hpp
each carry the stage with the same parameters and defaults."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_fill_depressions_work_floats", "nz_fill_depressions", "nz_fill_depressions_rw", "nz_fill_depressions_batch")
FIELDS = ["epsilon", "seaLevel", "maxPasses", "depth"]


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_header_declares_the_entries_and_the_library_exports_them(nj):
    N = nj._native
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "noize_hip.h"), flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES + ("nz_debug_fill_sweeps",):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    flat = " ".join(hdr.split())
    assert "size_t nz_fill_depressions_work_floats(int32_t resolution, int32_t count);" in flat
    assert ("int32_t nz_fill_depressions(nz_ctx *ctx, float *src, float *work, const nz_fill_desc *desc, int32_t resolution, "
            "nz_handle dep, nz_handle *out);") in flat
    assert ("int32_t nz_fill_depressions_rw(nz_ctx *ctx, nz_rw_tile *tile, float *work, const nz_fill_desc *desc, nz_handle dep, "
            "nz_handle *out);") in flat
    assert ("int32_t nz_fill_depressions_batch(nz_ctx *ctx, float *src, float *work, const nz_fill_desc *desc, "
            "int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);") in flat
    # nz_fill_desc field by field against the binding and the C# struct
    body = re.search(r"typedef struct nz_fill_desc \{(.*?)\} nz_fill_desc;", hdr, re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["float epsilon, seaLevel", "int32_t maxPasses", "float *depth"]
    assert [f[0] for f in N.FillDesc._fields_] == FIELDS
    assert [f[1] for f in N.FillDesc._fields_] == [ctypes.c_float, ctypes.c_float, ctypes.c_int32, ctypes.c_void_p]
    assert ctypes.sizeof(N.FillDesc) == 16 + ctypes.sizeof(ctypes.c_void_p)  # 12 bytes of scalars, padded to the pointer
    cs_body = re.search(r"public struct NzFillDesc\s*\{(.*?)\}", read("host-cs", "Runtime.cs"), re.S).group(1)
    cs = [(t, n.strip()) for t, d in re.findall(r"public\s+(\w+)\s+([^;]+);", cs_body) for n in d.split(",")]
    assert cs == [("float", "epsilon"), ("float", "seaLevel"), ("int", "maxPasses"), ("IntPtr", "depth")]
    # the work planes: a header, the tile bytes and two planes; nothing for an empty payload
    w = N.lib.nz_fill_depressions_work_floats
    assert w(0, 1) == 0 and w(64, 0) == 0
    for res, count in ((1, 1), (64, 1), (97, 3), (4096, 1)):
        n = res * res * count
        tiles = -(-res // 64) * -(-res // 16) * count
        assert 2 * n + 2 < w(res, count) <= 2 * n + 16 + 2 * (tiles + 15) // 4 + 8, (res, count)
    # the sweep hook hands back the cap that was in force and restores the default on 0
    d = N.lib.nz_debug_fill_sweeps(5)
    assert d >= 1 and N.lib.nz_debug_fill_sweeps(0) == 5 and N.lib.nz_debug_fill_sweeps(0) == d


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES:
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert "nz_fill_depressions_rw(IntPtr ctx, ref NzRwTile tile, IntPtr work, ref NzFillDesc desc, ulong dep, out ulong @out)" in cs


def test_the_three_hosts_carry_the_stage_with_the_same_defaults(nj):
    st = nj.DepressionFillStage(None)
    assert isinstance(st, nj.PipelineStage)
    assert (np.float32(st.epsilon), st.maxPasses, st.recordDepth) == (np.float32(1e-4), None, False)
    assert np.float32(st.seaLevel) == -np.finfo(np.float32).max == np.float32(nj.FluvialErosionStage(None).seaLevel)
    assert (st.depth, st.passes, st.converged) == (None, None, None)  # no payload yet
    other = nj.DepressionFillStage(None, 0.0, 0.25, 7, True)  # the positional order of the issue's signature
    assert (other.epsilon, other.seaLevel, other.maxPasses, other.recordDepth) == (0.0, 0.25, 7, True)
    pipe = nj.BasePipeline([nj.NoiseStage(None, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300), st,
                            nj.FluvialErosionStage(None)], "fill")
    assert pipe is not None
    py = read("noize_job_amd", "pipeline.py")
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")
    assert re.search(r"class DepressionFillStage\s*:\s*public PipelineStage", hpp)
    assert re.search(r"class DepressionFillStage\s*:\s*PipelineStage", cs)

    def body(src, head, nxt):
        i = src.index(head)
        return src[i:src.index(nxt, i + 1)]

    bpy = body(py, "class DepressionFillStage(", "\nclass ")
    bhpp = body(hpp, "class DepressionFillStage ", "\nclass ")
    bcs = body(cs, "public class DepressionFillStage ", "    public class ")
    # the same parameters, the same defaults, the same default budget, the same three entries
    assert "epsilon=1e-4, seaLevel=SEA_OFF, maxPasses=None, recordDepth=False" in bpy
    assert "float epsilon = 1e-4f, seaLevel = -3.402823466e+38f;" in bhpp and "bool recordDepth = false;" in bhpp
    assert "float epsilon = 1e-4f, seaLevel = -float.MaxValue;" in bcs and "bool recordDepth = false;" in bcs
    assert "int? maxPasses = null;" in bcs and re.search(r"int maxPasses = 0;\s*// < 1: 64 \+ resolution / 4", bhpp)
    assert "64 + self.resolution // 4" in bpy and "64 + resolution / 4" in bhpp and "64 + resolution / 4" in bcs
    for b, call in ((bpy, '"%s"'), (bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES:
            assert call % entry in b or (entry.endswith("work_floats") and entry + "(" in b), (entry, call)
    for b, members in ((bpy, ("def depth", "def passes", "def converged")),
                       (bhpp, ("depth() const", "int passes() const", "bool converged() const")),
                       (bcs, ("DeviceTile Depth", "int? Passes", "bool? Converged"))):
        for m in members:
            assert m in b, m
    # the documents name the stage
    assert "DepressionFillStage(ctx, recordDepth=True)" in read("README.md")
    assert "nz_fill_depressions" in read("INTEGRATION.md") and "nz_fill.hip" in read("DESIGN.md")
