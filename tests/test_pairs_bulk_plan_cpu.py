"""The host side of top_pairs_bulk's radix select (mmsbm_amd/csrc/pairs_bulk_plan.hpp) -- the order key, the digits, the
step between two passes, the early stop, the tie cut, the plan and the tile runs -- swept under AddressSanitizer + UBSan
(CPU build: the header is host arithmetic).  Compiles tests/native/pairs_bulk_check.cpp with g++ and runs it."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_select_step_and_plan_against_a_sorted_restatement(tmp_path):
    exe = tmp_path / "pairs_bulk_check"
    src = os.path.join(ROOT, "tests", "native", "pairs_bulk_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "pairs bulk check: ok" in run.stdout
