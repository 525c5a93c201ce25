"""The form of an EM iteration (mmsbm_amd/csrc/step_plan.hpp) against the five predicates it replaced, over every padded
shape of K, L = 1 .. 80, every fact about the data, every ask and ratings on both sides of each size threshold, under
AddressSanitizer + UBSan (CPU build: the header is host arithmetic).  Compiles tests/native/step_plan_check.cpp with g++
and runs it."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_step_plan_answers_what_the_parents_predicates_answered(tmp_path):
    exe = tmp_path / "step_plan_check"
    src = os.path.join(ROOT, "tests", "native", "step_plan_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "step plan check: ok" in run.stdout
    reached = re.search(r"two launches (\d+), three (\d+), four (\d+)", run.stdout)
    assert reached and all(int(n) > 0 for n in reached.groups()), run.stdout


def test_the_removed_predicates_are_named_nowhere_but_in_the_transcription():
    names = ("fused_shape_ok", "fused_possible", "pass_dense_possible", "use_fused", "use_pass_dense")
    found = []
    for top in ("mmsbm_amd", "tests", "scripts", "include"):
        for folder, _, files in os.walk(os.path.join(ROOT, top)):
            for name in files:
                if not name.endswith((".hip", ".hpp", ".h", ".cpp", ".py")) or name == os.path.basename(__file__):
                    continue
                with open(os.path.join(folder, name), errors="replace") as fh:
                    text = fh.read()
                found += [(os.path.relpath(os.path.join(folder, name), ROOT), n) for n in names if n in text]
    assert found and {path for path, _ in found} == {os.path.join("tests", "native", "step_plan_check.cpp")}, found
