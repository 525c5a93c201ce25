"""The one launch plan the ensemble queries add to mmsbm_amd/csrc/serve_plan.hpp -- the pairs per launch of
recommend_pair_spread -- swept under AddressSanitizer + UBSan (CPU build: the header is host arithmetic).  Compiles
tests/native/ens_plan_check.cpp with g++ and runs it."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_pairs_per_launch_over_every_shape(tmp_path):
    exe = tmp_path / "ens_plan_check"
    src = os.path.join(ROOT, "tests", "native", "ens_plan_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "ens plan check: ok" in run.stdout
