"""The stream-order stage across the ABI and the three hosts, without a GPU: the header declares the entries and
nz_stream_order_desc, the library exports them, and the Python binding, Native.cs / Runtime.cs, Stages.cs and
noize_pipeline.hpp each carry the stage with the same parameters, defaults, default budget, entries and members."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_stream_order_work_floats", "nz_stream_order", "nz_stream_order_batch")
FIELDS = ["seaLevel", "threshold", "maxPasses", "drainage"]
BUDGET_PY, BUDGET_C = "64 + self.resolution // 4", "64 + resolution / 4"  # the measured default, DESIGN.md section 4


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_header_declares_the_entries_and_the_library_exports_them(nj):
    N = nj._native
    hdr = re.sub(r"/\*.*?\*/", " ", read("include", "noize_hip.h"), flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES + ("nz_debug_stream_order_sweeps",):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    flat = " ".join(hdr.split())
    assert "size_t nz_stream_order_work_floats(int32_t resolution, int32_t count, int32_t withLinks);" in flat
    assert ("int32_t nz_stream_order(nz_ctx *ctx, const float *height, uint8_t *order, int32_t *link, float *work, "
            "const nz_stream_order_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out);") in flat
    assert ("int32_t nz_stream_order_batch(nz_ctx *ctx, const float *height, uint8_t *order, int32_t *link, float *work, "
            "const nz_stream_order_desc *desc, int32_t resolution, int32_t count, nz_handle dep, nz_handle *out);") in flat
    assert "int32_t nz_debug_stream_order_sweeps(int32_t sweeps);" in flat
    assert not re.search(r"\bnz_stream_order_stripe\w*\b|\bnz_stream_order_rw\b", hdr)  # not built, DESIGN.md section 9
    assert flat.index("nz_debug_watershed_sweeps(") < flat.index("typedef struct nz_stream_order_desc")  # behind the watershed block
    assert len(N.SIGNATURES["nz_stream_order"][1]) == 9 and len(N.SIGNATURES["nz_stream_order_batch"][1]) == 10
    # nz_stream_order_desc field by field against the binding and the C# struct
    body = re.search(r"typedef struct nz_stream_order_desc \{(.*?)\} nz_stream_order_desc;", hdr, re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["float seaLevel, threshold", "int32_t maxPasses", "const float *drainage"]
    assert [f[0] for f in N.StreamOrderDesc._fields_] == FIELDS
    assert [f[1] for f in N.StreamOrderDesc._fields_] == [ctypes.c_float, ctypes.c_float, ctypes.c_int32, ctypes.c_void_p]
    assert ctypes.sizeof(N.StreamOrderDesc) == 24 and N.StreamOrderDesc.drainage.offset == 16
    cs_body = re.search(r"public struct NzStreamOrderDesc\s*\{(.*?)\}", read("host-cs", "Runtime.cs"), re.S).group(1)
    cs = [(t, n.strip()) for t, d in re.findall(r"public\s+(\w+)\s+([^;]+);", cs_body) for n in d.split(",")]
    assert cs == [("float", "seaLevel"), ("float", "threshold"), ("int", "maxPasses"), ("IntPtr", "drainage")]


def test_the_work_planes_and_the_sweep_hook(nj):
    N = nj._native
    # the work planes: at least the donor bytes, the second order plane and, with links, the second link plane; on top of
    # that no more than the status words, the tile bytes and slack
    w = N.lib.nz_stream_order_work_floats
    for wl in (0, 1):
        assert w(0, 1, wl) == 0 and w(64, 0, wl) == 0 and w(0, 0, wl) == 0 and w(-3, 2, wl) == 0 and w(8, -1, wl) == 0
        for res, count in ((1, 1), (64, 1), (97, 3), (4096, 1)):
            n = res * res * count
            tiles = -(-res // 64) * -(-res // 16) * count
            floor = 2 * -(-n // 4) + wl * n
            assert floor <= w(res, count, wl) <= floor + 16 + 2 * (tiles + 15) // 4 + 12, (res, count, wl)
    assert w(97, 3, 1) - w(97, 3, 0) == 97 * 97 * 3 and w(64, 1, 7) == w(64, 1, 1) and w(64, 1, -1) == w(64, 1, 1)
    # the sweep hook hands back the cap that was in force and restores the default on <= 0; it is no other stage's
    d = N.lib.nz_debug_stream_order_sweeps(5)
    s = N.lib.nz_debug_watershed_sweeps(0)
    a = N.lib.nz_debug_drainage_sweeps(0)
    f = N.lib.nz_debug_fill_sweeps(0)
    assert d >= 1 and N.lib.nz_debug_stream_order_sweeps(0) == 5 and N.lib.nz_debug_stream_order_sweeps(0) == d
    assert N.lib.nz_debug_stream_order_sweeps(-2) == d and N.lib.nz_debug_stream_order_sweeps(0) == d
    assert N.lib.nz_debug_watershed_sweeps(0) == s and N.lib.nz_debug_drainage_sweeps(0) == a and N.lib.nz_debug_fill_sweeps(0) == f
    N.lib.nz_debug_watershed_sweeps(3)
    assert N.lib.nz_debug_stream_order_sweeps(0) == d and N.lib.nz_debug_watershed_sweeps(0) == 3
    assert N.lib.nz_version() == 100


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES + ("nz_debug_stream_order_sweeps",):
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert "public static extern UIntPtr nz_stream_order_work_floats(int resolution, int count, int withLinks);" in cs
    assert ("nz_stream_order_batch(IntPtr ctx, IntPtr height, IntPtr order, IntPtr link, IntPtr work, "
            "ref NzStreamOrderDesc desc, int resolution, int count, ulong dep, out ulong @out)") in cs
    assert '"nz_stream_order_desc": "NzStreamOrderDesc"' in read("tools", "gen_native_cs.py")


def test_the_three_hosts_carry_the_stage_with_the_same_defaults(nj):
    st = nj.StreamOrderStage(None)
    assert isinstance(st, nj.PipelineStage) and "StreamOrderStage" in nj.__all__
    assert (np.float32(st.threshold), st.maxPasses, st.drainage, st.recordLinks) == (np.float32(0.0), None, None, False)
    assert np.float32(st.seaLevel) == -np.finfo(np.float32).max == np.float32(nj.DrainageAreaStage(None).seaLevel)
    assert (st.order, st.links, st.passes, st.converged) == (None, None, None, None)  # no payload yet
    plane = object()
    other = nj.StreamOrderStage(None, 0.25, 8.0, 7, plane, True)  # the positional order of the signature
    assert (other.seaLevel, other.threshold, other.maxPasses, other.drainage, other.recordLinks) == (0.25, 8.0, 7, plane, True)
    pipe = nj.BasePipeline([nj.NoiseStage(None, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300),
                            nj.DepressionFillStage(None), nj.DrainageAreaStage(None), st], "rivers")
    assert pipe is not None
    py = read("noize_job_amd", "pipeline.py")
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")
    assert re.search(r"class StreamOrderStage\s*:\s*public PipelineStage", hpp)
    assert re.search(r"class StreamOrderStage\s*:\s*PipelineStage", cs)

    def body(src, head, nxt):
        i = src.index(head)
        return src[i:src.index(nxt, i + 1)]

    bpy = body(py, "class StreamOrderStage(", "\nclass ")
    bhpp = body(hpp, "class StreamOrderStage ", "\nclass ")
    bcs = body(cs, "public class StreamOrderStage ", "    public class ")
    # placed behind the watershed stage and in front of the mesh stage in each host
    for src, head in ((py, "class %s("), (hpp, "class %s "), (cs, "public class %s ")):
        assert src.index(head % "WatershedStage") < src.index(head % "StreamOrderStage") < src.index(head % "MeshTileStage")
    # the same parameters, the same defaults, the same default budget, the same entries, the same members
    assert "seaLevel=SEA_OFF, threshold=0.0, maxPasses=None, drainage=None, recordLinks=False" in bpy
    assert "float seaLevel = -3.402823466e+38f, threshold = 0.f;" in bhpp
    assert "const DeviceTile *drainage = nullptr;" in bhpp and "bool recordLinks = false;" in bhpp
    assert "float seaLevel = -float.MaxValue, threshold = 0f;" in bcs
    assert "DeviceTile drainage = null;" in bcs and "bool recordLinks = false;" in bcs
    assert "int? maxPasses = null;" in bcs and re.search(r"int maxPasses = 0;\s*// < 1: %s" % re.escape(BUDGET_C), bhpp)
    assert BUDGET_PY in bpy and BUDGET_C in bhpp and BUDGET_C in bcs
    for b in (bhpp, bcs):  # the declaration order is the positional order
        at = [b.index(name) for name in ("seaLevel", "threshold", "maxPasses", "drainage", "recordLinks")]
        assert at == sorted(at)
    for b, call in ((bpy, '"%s"'), (bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES:
            assert call % entry in b or (entry.endswith("work_floats") and entry + "(" in b), (entry, call)
        # the heights pass through: no pair form, no erosion, and none of the other stages' entries
        assert "_rw" not in b and not re.search(r"nz_(fluvial|drainage|fill|watershed)\w*\(", b)
    assert "dtype=np.int32" in bpy and "np.uint8" in bpy  # the links are handed out as an int32 view, the orders as bytes
    for b, members in ((bpy, ("def order", "def links", "def passes", "def converged")),
                       (bhpp, ("order() const", "links() const", "int passes() const", "bool converged() const")),
                       (bcs, ("DeviceTile Order", "DeviceTile Links", "int? Passes", "bool? Converged"))):
        for m in members:
            assert m in b, m
    # the header states the same default
    assert ("maxPasses " + BUDGET_C) in " ".join(body(read("include", "noize_hip.h"), "---- stream order:", "typedef struct nz_stream_order_desc").split())


def test_a_drainage_plane_that_is_no_device_tile_of_the_payload_raises(nj):
    class Tile:  # what Schedule looks at
        def __init__(self, length):
            self.ptr, self.Length, self.dtype = 4096, length, np.dtype(np.float32)

    for bad in (np.zeros(16, np.float32), 3.0, Tile(15)):
        st = nj.StreamOrderStage(None, drainage=bad)
        d = nj.GeneratorData("h", Tile(16), 4, 0, 0)
        with pytest.raises((ValueError, TypeError)):
            st.Schedule(nj.PipelineWorkItem(d), nj.JobHandle())
        assert st.work is None  # before any allocation or launch


def test_the_documents_name_the_stage_and_the_tool_exists():
    readme = read("README.md")
    assert "StreamOrderStage(ctx" in readme and "nz_stream_order" in readme and "tools/bench_stream_order.py" in readme
    integ = read("INTEGRATION.md")
    assert "nz_stream_order(" in integ and "nz_stream_order_batch(" in integ and "NzStreamOrderDesc" in integ
    design = read("DESIGN.md")
    assert "nz_stream_order.hip" in design and "| f9 " in design and "nz_debug_stream_order_sweeps" in design
    assert "profiles/stream_order.txt" in design and os.path.exists(os.path.join(ROOT, "profiles", "stream_order.txt"))
    assert "StreamOrderStage" in read("host-cs", "README.md")
    assert "StreamOrderStage" in read("HISTORY.md") or "nz_stream_order" in read("HISTORY.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_stream_order.py"))
    hdr = read("include", "noize_hip.h")
    assert "@EVIDENCE@" not in hdr and "row-stripe form is not built" in " ".join(hdr.split())
    mk = read("noize_job_amd", "csrc", "Makefile")
    assert "nz_stream_order.hip" in mk
    for h in ("nz_receiver.hpp", "nz_tile64.hpp", "nz_relax_pass.hpp"):
        assert re.search(r"build/nz_stream_order\.o[^\n]*: %s" % re.escape(h), mk), h
        assert re.search(r"build/nz_watershed\.o[^\n]*: %s" % re.escape(h), mk), h
        assert '#include "%s"' % h in read("noize_job_amd", "csrc", "nz_stream_order.hip")
