"""noize_job_amd/csrc/nz_planes.hpp -- the stripe geometry and aliasing helpers of the terrain entry points -- checked on the
CPU: tests/planes_check.cpp is a stand-alone program that includes the header, built here with plain g++ under the address
and undefined-behaviour sanitizers and run directly.  It holds the stripe window against the two expressions the helper
replaced over every small stripe, the span and plane sizes, the overlap predicate, and nz_require_disjoint on the plane
layouts of nz_hydraulic_stripe and nz_fluvial_stripe with the refusal texts the GPU suites provoke."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planes_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "planes_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "planes_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("planes_check: ok"), run.stdout
