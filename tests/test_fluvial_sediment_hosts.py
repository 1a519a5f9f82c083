"""The sediment stage across the ABI and the three hosts, without a GPU: the header declares the entries and
nz_fluvial_sediment_desc and states the model and its limits, the library exports them, and the Python binding, Native.cs /
Runtime.cs, Stages.cs and noize_pipeline.hpp each carry SedimentFluvialStage as a subclass of ImplicitFluvialStage with the
same parameters, order, defaults, entries and members."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nz_fluvial_sediment_work_floats", "nz_fluvial_sediment", "nz_fluvial_sediment_batch")
HOOK = "nz_debug_fluvial_sediment_sweeps"
FLOATS = ["erodibility", "uplift", "dt", "seaLevel"]
POINTERS = ["hardness", "upliftMap", "proceed", "tally"]


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
    assert "size_t nz_fluvial_sediment_work_floats(int32_t resolution, int32_t count);" in flat
    assert ("int32_t nz_fluvial_sediment(nz_ctx *ctx, const float *height, const float *drainage, float *out, float *work, "
            "const nz_fluvial_sediment_desc *desc, int32_t resolution, nz_handle dep, nz_handle *out_handle);") in flat
    assert ("int32_t nz_fluvial_sediment_batch(nz_ctx *ctx, const float *height, const float *drainage, float *out, "
            "float *work, const nz_fluvial_sediment_desc *desc, int32_t resolution, int32_t count, nz_handle dep, "
            "nz_handle *out_handle);") in flat
    assert "int32_t %s(int32_t sweeps);" % HOOK in flat
    assert not re.search(r"\bnz_fluvial_sediment_(stripe|rw)\w*", hdr)
    assert len(N.SIGNATURES["nz_fluvial_sediment"][1]) == 9 and len(N.SIGNATURES["nz_fluvial_sediment_batch"][1]) == 10
    # the desc: the implicit desc's fields in its order, then the three new ones -- header, binding, C# struct
    def fields(name):
        b = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        return [" ".join(d.split()) for d in b.split(";") if d.strip()]
    parent = fields("nz_fluvial_implicit_desc")
    assert fields("nz_fluvial_sediment_desc") == parent + ["float deposition", "int32_t iterations", "float *flux"]
    assert N.FluvialSedimentDesc._fields_[:9] == N.FluvialImplicitDesc._fields_
    assert N.FluvialSedimentDesc._fields_[9:] == [("deposition", ctypes.c_float), ("iterations", ctypes.c_int32),
                                                  ("flux", ctypes.c_void_p)]
    assert ctypes.sizeof(N.FluvialSedimentDesc) == 72 and N.FluvialSedimentDesc.deposition.offset == 56
    assert N.FluvialSedimentDesc.flux.offset == 64
    cs_body = re.search(r"public struct NzFluvialSedimentDesc\s*\{(.*?)\}", read("host-cs", "Runtime.cs"), re.S).group(1)
    cs = [(t, n.strip()) for t, d in re.findall(r"public\s+(\w+)\s+([^;]+);", cs_body) for n in d.split(",")]
    assert cs == ([("float", n) for n in FLOATS] + [("int", "maxPasses")] + [("IntPtr", n) for n in POINTERS] +
                  [("float", "deposition"), ("int", "iterations"), ("IntPtr", "flux")])


def test_the_work_planes_have_a_floor_and_a_ceiling(nj):
    # the receiver and the donor bytes, b0, f, e / bk, two Q planes and two h' planes; on top no more than the two heads,
    # the tile bytes and slack
    w = nj._native.lib.nz_fluvial_sediment_work_floats
    assert w(0, 1) == 0 and w(64, 0) == 0 and w(0, 0) == 0 and w(-3, 2) == 0 and w(8, -1) == 0
    for res, count in ((1, 1), (64, 1), (97, 3), (4096, 1)):
        n = res * res * count
        tiles = -(-res // 64) * -(-res // 16) * count
        floor = 7 * n + 2 * -(-n // 4)
        assert floor <= w(res, count) <= floor + 32 + 2 * (tiles + 15) // 4 + 16, (res, count)
    assert w(97, 3) > 3 * w(97, 1) - 3 * 32  # a batch is its tiles back to back, one head


def test_the_sweep_hook_is_this_stage_s_own(nj):
    lib = nj._native.lib
    others = ("nz_debug_fluvial_implicit_sweeps", "nz_debug_drainage_sweeps", "nz_debug_fluvial_implicit_mfd_sweeps")
    before = [getattr(lib, o)(0) for o in others]
    hook = getattr(lib, HOOK)
    d = hook(5)
    assert d == 16 and hook(0) == 5 and hook(0) == d
    assert hook(-2) == d and hook(0) == d
    assert [getattr(lib, o)(0) for o in others] == before
    lib.nz_debug_fluvial_implicit_sweeps(3)
    assert hook(0) == d and lib.nz_debug_fluvial_implicit_sweeps(0) == 3


def test_native_cs_is_generated_with_the_entries():
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_native_cs.py"), "--check"], capture_output=True)
    assert gen.returncode == 0, "run tools/gen_native_cs.py"
    cs = read("host-cs", "Native.cs")
    for name in ENTRIES + (HOOK,):
        assert re.search(r"public static extern \w+ %s\(" % name, cs), name
    assert "public static extern UIntPtr nz_fluvial_sediment_work_floats(int resolution, int count);" in cs
    assert ("nz_fluvial_sediment_batch(IntPtr ctx, IntPtr height, IntPtr drainage, IntPtr @out, IntPtr work, "
            "ref NzFluvialSedimentDesc desc, int resolution, int count, ulong dep, out ulong out_handle)") in cs
    assert '"nz_fluvial_sediment_desc": "NzFluvialSedimentDesc"' in read("tools", "gen_native_cs.py")


def test_the_three_hosts_carry_the_subclass_with_the_same_defaults(nj):
    st = nj.SedimentFluvialStage(None)
    assert isinstance(st, nj.ImplicitFluvialStage) and "SedimentFluvialStage" in nj.__all__
    assert (st.deposition, st.sedimentIterations, st.recordFlux) == (0.5, 4, False)
    assert (st.iterations, st.erodibility, st.uplift, st.dt, st.rain, st.maxPasses) == (1, 0.05, 0.002, 1.0, 1.0, None)
    assert (st.drainage, st.steps, st.passes, st.converged, st.flux, st.residual) == (None,) * 6  # no payload yet
    # the parent's parameters in the parent's order, then the three new ones
    mine = list(inspect.signature(nj.SedimentFluvialStage.__init__).parameters)
    theirs = list(inspect.signature(nj.ImplicitFluvialStage.__init__).parameters)
    assert mine == theirs + ["deposition", "sedimentIterations", "recordFlux"]
    a, b, c = object(), object(), object()
    o = nj.SedimentFluvialStage(None, 4, 0.1, 0.01, 250.0, 2.0, 0.25, 7, a, b, c, nj.FlowRouting.Multiple, 3, 1.0, 2, True)
    assert (o.iterations, o.erodibility, o.uplift, o.dt, o.rain, o.seaLevel, o.maxPasses) == (4, 0.1, 0.01, 250.0, 2.0, 0.25, 7)
    assert (o.rainMap, o.hardness, o.upliftMap, o.routing, o.flowExponent) == (a, b, c, nj.FlowRouting.Multiple, 3)
    assert (o.deposition, o.sedimentIterations, o.recordFlux) == (1.0, 2, True)
    # a Schedule of the parent's alone: the subclass supplies the solve and the work size through the hook
    assert "Schedule" not in vars(nj.SedimentFluvialStage)
    assert {"_enqueue_solve", "_solve_work_floats"} <= set(vars(nj.SedimentFluvialStage)) & set(vars(nj.ImplicitFluvialStage))
    py = read("noize_job_amd", "pipeline.py")
    hpp = read("noize_job_amd", "host", "noize_pipeline.hpp")
    cs = read("host-cs", "Stages", "Stages.cs")
    assert re.search(r"class SedimentFluvialStage\s*:\s*public ImplicitFluvialStage", hpp)
    assert re.search(r"class SedimentFluvialStage\s*:\s*ImplicitFluvialStage", cs)
    bpy = body(py, "class SedimentFluvialStage(", "\nclass ")
    bhpp = body(hpp, "class SedimentFluvialStage ", "\nclass ")
    bcs = body(cs, "public class SedimentFluvialStage ", "    public class ")
    # behind the hillslope stage and in front of the mesh stage in each host
    for src, head in ((py, "class %s("), (hpp, "class %s "), (cs, "public class %s ")):
        assert src.index(head % "HillslopeDiffusionStage") < src.index(head % "SedimentFluvialStage") < src.index(head % "MeshTileStage")
    assert "deposition=0.5, sedimentIterations=4, recordFlux=False" in bpy
    assert "float deposition = .5f;" in bhpp and "int sedimentIterations = 4;" in bhpp and "bool recordFlux = false;" in bhpp
    assert ("public float deposition = 0.5f;" in bcs and "public int sedimentIterations = 4;" in bcs and
            "public bool recordFlux = false;" in bcs)
    for b, call in ((bpy, '"%s"'), (bhpp, "%s(ctx, "), (bcs, "Native.%s(ctx.Handle, ")):
        for entry in ENTRIES:
            assert call % entry in b or (entry.endswith("work_floats") and entry + "(" in b), (entry, call)
        # everything else is inherited: no drainage call, no proceed word, no tally, no Schedule of its own
        assert "nz_drainage" not in b and "drainageWork" not in b and "nz_tile_upload" not in b and "Schedule(" not in b
        assert "_rw" not in b and "stripe" not in b.lower()
    for b, members in ((bpy, ("def flux", "def residual")), (bhpp, ("flux() const", "float residual() const")),
                       (bcs, ("DeviceTile Flux", "float? Residual"))):
        for m in members:
            assert m in b, m
    # the parent has the hook in every host, and calls it once per iteration
    ppy = body(py, "class ImplicitFluvialStage(", "\nclass ")
    phpp = body(hpp, "class ImplicitFluvialStage ", "\nclass ")
    pcs = body(cs, "public class ImplicitFluvialStage ", "    public class ")
    assert ppy.count("self._enqueue_solve(") == 1 and "def _enqueue_solve(" in ppy and "def _solve_work_floats(" in ppy
    assert phpp.count("enqueueSolve(") == 2 and "virtual void enqueueSolve(" in phpp and "virtual size_t solveWorkFloats(" in phpp
    assert pcs.count("EnqueueSolve(") == 2 and "protected virtual void EnqueueSolve(" in pcs and "protected virtual int SolveWorkFloats(" in pcs
    demo = read("noize_job_amd", "host", "host_demo.cpp")
    assert '"sediment"' in demo and "SedimentFluvialStage st(r.ctx);" in read("noize_job_amd", "host", "host_demo_stages.hpp")


def test_the_header_states_the_model_and_the_limits():
    block = body(read("include", "noize_hip.h"), "---- implicit fluvial erosion with sediment deposition",
                 "typedef struct nz_fluvial_sediment_desc")
    words = " ".join(re.sub(r"(?m)^ \* ?", "", block).split())
    for must in ("Yuan, Braun, Guerit, Rouby & Cordonnier (2019)", "h0 = solve(b0)", "e[c] = b0[c] - h(k-1)[c]",
                 "neighbour order 0..7", "Qin < 0 ? +0 : Qin", "a NaN passes", "(G * Qin[c]) / A[c]", "where A[c] > 0",
                 "taken with d > m", "hK >= h0", "nz_fluvial_implicit's plane bit for bit", "contraction", "stalls",
                 "INCOMING heights", "lift a cell above a donor", "DepressionFillStage", "no lake trapping",
                 "nz_fluvial_implicit_mfd) has no sediment form", "ALL OR NOTHING", "`flux` is untouched",
                 "{passes that did work over all series, converged 0/1, residual as float bits}",
                 "Neither an _rw pair form nor a row-stripe form exists", "deposition negative or not finite",
                 "iterations < 0", "flux overlapping", "deposition 0.5, sedimentIterations 4"):
        assert must in words, must


def test_the_documents_name_the_stage_and_the_tool_exists():
    readme = read("README.md")
    assert "SedimentFluvialStage(" in readme and "nz_fluvial_sediment" in readme and "tools/bench_fluvial_sediment.py" in readme
    integ = read("INTEGRATION.md")
    assert "nz_fluvial_sediment(" in integ and "nz_fluvial_sediment_batch(" in integ and "NzFluvialSedimentDesc" in integ
    design = " ".join(read("DESIGN.md").split())
    assert "nz_fluvial_sediment.hip" in design and "| f14 " in design and "sedimentIterations = 4" in design
    for limit in ("contraction", "No lake trapping", "frozen per step", "multiple-flow solve is not covered", "unmeasured"):
        assert limit in design, limit
    assert "SedimentFluvialStage" in read("host-cs", "README.md")
    assert "SedimentFluvialStage" in read("HISTORY.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_fluvial_sediment.py"))
    mk = read("noize_job_amd", "csrc", "Makefile")
    assert "nz_fluvial_sediment.hip" in mk
    for hdr in ("nz_receiver.hpp", "nz_donor_front.hpp", "nz_tile64.hpp", "nz_relax_pass.hpp"):
        assert re.search(r"build/nz_fluvial_sediment\.o[^\n]*: %s" % re.escape(hdr), mk), hdr
    # the parent's translation unit does not know about this one
    assert "sediment" not in read("noize_job_amd", "csrc", "nz_fluvial_implicit.hip")
