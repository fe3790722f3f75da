"""CPU: csrc/workspace.h (the workspace planner and ParamLayout every engine's context is laid out
with) checked by a stand-alone program under AddressSanitizer and UBSan: tests/host/
workspace_check.cc compares every offset with a running sum it computes itself.  Nothing is loaded
into Python and nothing is preloaded; the program is run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "workspace_check.cc")
CSRC = os.path.join(ROOT, "mujoco_reinforcement_learning_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ on PATH")
def test_workspace_planner_under_sanitizers(tmp_path):
    exe = str(tmp_path / "workspace_check")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
