"""The request checks of the C ABI (mmsbm_amd/csrc/abi_request.hpp) on the CPU, under AddressSanitizer + UBSan: the
header is host arithmetic on plain arrays.  Compiles tests/native/abi_request_check.cpp with g++ and runs it; every
refusal it prints must be the one the library gave for the same request when tests/gpu_abi_requests_parent.json was
recorded, so the CPU run is tied to the recorded texts and not to the code under test."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

# what only the header's checkers say: a table row of a covered entry with one of these is a row the program must print
CHECKER_TEXTS = ("id out of range at row", "n must be at least 1", "a query returns at most", "[0] must be 0", " decrease at ",
                 "more than 2^31 - 1 ", "out of range at entry", "ascending and distinct", "n_cand outside", "negative n_cats",
                 "negative cap of", "is in two categories", "temperature", "depth must", "min_items must", "n_shelves must",
                 "negative per_shelf", "a query holds", "is twice in the list", "a list holds at most", "member repeated",
                 "theta entry", "is repeated", "asked twice", "must be the number of training users", "negative n_users")
# ... but for these: checks the entry makes itself or in an order of its own, before the header's
OWN = ("recommend_diverse: n = ", "recommend_diverse: pool", "recommend_diverse: n = 0 and",
       "recommend_allocate: n = ", "recommend_allocate: n_users = -1", "recommend_assign: n_users = -1",
       "recommend_query_groups: n = ", "recommend_query_groups: an unknown mode and", "recommend_query_groups: candidate",
       "recommend_query_groups: n_cand", "recommend_query_groups: a repeated member and",
       "recommend_query_ensemble: an unknown mode and", "recommend_top_pairs: n_users = -1",
       "recommend_top_pairs_bulk: n_users = -1", "recommend_pair_bar: n_users = -1",
       "recommend_top_pairs: m = ", "recommend_top_pairs_bulk: m = ", "recommend_pair_bar: m = ", "explain_query: 2^31 entries",
       "recommend_allocate: max_rounds = 0 and", "recommend_query_within: candidate n_items + 2 after add_items")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_request_checks_give_the_recorded_refusals(tmp_path):
    exe = tmp_path / "abi_request_check"
    src = os.path.join(ROOT, "tests", "native", "abi_request_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "abi request check: ok"
    printed = [line.split("\t") for line in lines[:-1]]
    assert all(len(row) == 3 for row in printed), [row for row in printed if len(row) != 3][:5]

    with open(os.path.join(ROOT, "tests", "gpu_abi_requests_parent.json")) as fh:
        table = {label: (code, text) for label, code, text in json.load(fh)}
    labels = [label for label, _, _ in printed]
    assert len(set(labels)) == len(labels)
    for label, code, text in printed:
        assert label in table, label
        assert (int(code), text) == table[label], (label, code, text, table[label])

    # every row the table holds for those checkers, in the entries the program covers, was printed
    entries = {label.split(":")[0] for label in labels}
    expected = [label for label, (code, text) in table.items()
                if label.split(":")[0] in entries and code != "ValueError" and not label.startswith(OWN)
                and any(t in text for t in CHECKER_TEXTS)]
    missing = sorted(set(expected) - set(labels))
    assert not missing, missing
    assert len(printed) >= len(expected) >= 250
