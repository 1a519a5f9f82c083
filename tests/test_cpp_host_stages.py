"""host_demo's `stage` mode without a device: the scenario list, the guard that every stage class of the C++ host is run by
a compiled program somewhere (or is on a list that says why not), and the two refusals that need no context."""
import os
import re
import subprocess

import numpy as np

import test_gpu_cpp_host_stages as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "noize_job_amd", "host")
EXE = os.path.join(HOST, "host_demo")

# stage classes another mode of host_demo runs on a device, and the test that starts it
RUN_BY_OTHER_MODES = {
    "NoiseStage": "the default mode (test_gpu_parity.test_cpp_host_mirror_runs_the_metric_pipeline)",
    "KernelFilterStage": "the default mode",
    "FlowMapStage": "the default mode",
    "ErosionStage": "the default mode",
    "ReduceStage": "reduce",
    "ReadGeneratorContextStage": "context",
    "WriteGeneratorContextStage": "context",
    "DepressionFillStage": "fill (test_gpu_fill)",
}
# stage classes no compiled program runs, each with its reason
NOT_RUN = {
    "MeshTileReferenceDataStage": "MeshTileStage::Schedule on a context buffer: the mesh call is run by the MeshTileStage "
                                  "scenario, the buffer look-up by the context mode's two stages",
}


def demo(*args):
    assert os.path.exists(EXE), "host_demo not built (run __graft_entry__.build())"
    return subprocess.run([EXE] + list(args), timeout=120, capture_output=True, text=True)


def stage_classes():
    """Every class of noize_pipeline.hpp that derives from PipelineStage, directly or through another stage class, and
    schedules work itself (TmpStage and ResampleStage only hold what their subclasses share)."""
    text = open(os.path.join(HOST, "noize_pipeline.hpp")).read()
    found = [(m.group(1), m.group(2), m.start()) for m in re.finditer(r"\nclass (\w+) : public (\w+) \{", text)]
    stages, grew = {"PipelineStage"}, True
    while grew:
        grew = False
        for name, base, _ in found:
            if base in stages and name not in stages:
                stages.add(name)
                grew = True
    out = []
    for name, base, at in found:
        body = text[at:text.index("\n};", at)]
        if name in stages and "void Schedule(" in body:
            out.append(name)
    return out


def test_list_runs_without_a_device_and_names_the_scenarios_of_the_gpu_tests():
    p = demo("0", "-", "stage", "--list")
    assert p.returncode == 0, p.stderr
    names = p.stdout.split()
    assert names == G.SCENARIOS and len(set(names)) == len(names)
    tests = [n for n in dir(G) if n.startswith("test_")]
    assert len(tests) == len(names)  # one test per scenario


def test_every_stage_class_is_run_or_listed():
    classes = stage_classes()
    assert len(classes) >= 29 and "HydraulicErosionStage" in classes and "WarpedNoiseStage" in classes
    assert "TmpStage" not in classes and "ResampleStage" not in classes
    sets = (set(G.SCENARIOS), set(RUN_BY_OTHER_MODES), set(NOT_RUN))
    for name in classes:
        assert sum(name in s for s in sets) == 1, "%s is in %d of the three sets" % (name, sum(name in s for s in sets))
    for s in sets:
        assert s <= set(classes), "not a stage class: %s" % sorted(s - set(classes))
    assert all(reason.strip() for reason in NOT_RUN.values())
    # a mode named as the one that runs a class is a mode host_demo has
    source = open(os.path.join(HOST, "host_demo.cpp")).read()
    for name, mode in RUN_BY_OTHER_MODES.items():
        word = mode.split()[0]
        assert word == "the" or '"%s"' % word in source, (name, mode)
        if word == "the":
            assert re.search(r"\b%s \w+\(ctx\)" % name, source), name
    # ... and every scenario constructs the class it is named after
    stages = open(os.path.join(HOST, "host_demo_stages.hpp")).read()
    for name in G.SCENARIOS:
        assert re.search(r"\b%s st\(r\.ctx\)|<%s>\(r" % (name, name), stages), name


def test_an_unknown_stage_and_a_short_input_are_refused(tmp_path):
    out = str(tmp_path / "out.bin")
    p = demo("0", out, "stage", "NoSuchStage", str(tmp_path / "missing.f32"))
    assert p.returncode != 0 and "NoSuchStage" in p.stderr and p.stdout == ""
    assert not os.path.exists(out)
    short = str(tmp_path / "short.f32")
    np.zeros(100, np.float32).tofile(short)
    for name in ("WatershedStage", "CropStage"):
        p = demo("0", out, "stage", name, short)
        assert p.returncode != 0 and name in p.stderr and "100" in p.stderr and p.stdout == "", (name, p.stderr)
        assert not os.path.exists(out)  # refused before the output was opened and a context created
    p = demo("0", out, "stage", "WatershedStage")
    assert p.returncode != 0 and "input" in p.stderr
