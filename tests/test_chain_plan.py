"""noize_job_amd/csrc/nz_chain_plan.hpp -- the host-built tile plan of the chained filter grid -- checked on the CPU:
tests/chain_plan_check.cpp is a stand-alone program that includes the header, built here with plain g++ under the address
and undefined-behaviour sanitizers and run directly.  For 5 and 9 taps, the three tile shapes, the grids 352 x 352,
1000 x 360, 301 x 263, 4096 x 4096 and a stripe window with or0 > 0, and the depth lists {4,4,4,5}, {4,4,5}, {9,8}, {1,1} it
compares every record with a brute-force restatement: origin and depth from the item number by the documented class rule,
the awaited set against every tile of the previous launch whose interior meets the widened window, every item once, and
the total nz_conv_chain_items reports (the same nz_chain_layout_of)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_plan_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chain_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "chain_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("chain_plan_check: ok"), run.stdout
