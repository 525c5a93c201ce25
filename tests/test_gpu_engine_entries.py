"""Every engine entry of the C ABI launches what it launched, and returns what it returned, before the engine moved out
of mmsbm_hip.hip into units of its own (tu_iterate.hip, tu_create.hip, tu_params.hip, tu_options.hip, and the host side
of prod_dist / predict / compute_omegas in tu_once.hip): per case of tests/engine_cases.py the launch count per kernel
name, the options that show the iteration's form, and step by step the SHA-256 of every array and every scalar the
sequence returns equal the table recorded from the parent commit (tests/gpu_engine_entries_parent.json, written by
tests/engine_cases.py).  The EM step has no atomics: the bits are comparable."""
import json
import os

import pytest

import engine_cases as cases
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mmsbm_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("-m gpu tests need a GPU: no HIP device visible (no CPU fallback exists)")
    if not os.environ.get("MMSBM_HIP_LAUNCH_LOG"):
        pytest.fail("the launch log is switched off (MMSBM_HIP_LAUNCH_LOG is empty): nothing to compare")
    import mmsbm_amd
    return mmsbm_amd


@pytest.fixture(scope="module")
def parent_table():
    with open(os.path.join(ROOT, "tests", "gpu_engine_entries_parent.json")) as fh:
        return json.load(fh)


def test_the_table_holds_these_cases(parent_table):
    assert sorted(parent_table) == sorted(cases.CASES)
    forms = {name: row["form"] for name, row in parent_table.items()}
    # every form the cases are named after is the one the parent really took
    assert forms["two-launch"]["launches"] == 2.0 and forms["two-launch"]["fused_split"] == 0.0
    assert forms["two-launch"]["splits_users"] == forms["two-launch"]["splits_pairs"] == 0.0
    assert forms["two-launch-lists"]["launches"] == 2.0 and forms["two-launch-lists"]["fused_split"] == 3.0
    assert forms["two-launch-swapped"]["launches"] == 2.0 and forms["two-launch-swapped"]["swapped"]
    assert forms["whole-segments"]["launches"] == 2.0 and forms["whole-segments"]["fused_split"] == 3.0
    assert forms["whole-segments"]["splits_users"] > 0 and forms["whole-segments"]["splits_pairs"] > 0
    assert forms["four-launch"]["launches"] == 4.0 and forms["four-launch"]["pass_dense"] == 0.0
    assert forms["four-launch"]["splits_users"] > 0 and forms["four-launch"]["splits_pairs"] > 0
    assert forms["pass-dense"]["launches"] == 4.0 and forms["pass-dense"]["pass_dense"] == 1.0
    assert forms["matrix-cores"]["mfma"] == 1.0 and forms["matrix-cores"]["a_units"] > 0
    assert forms["wide-rows"]["wide"] == 1.0
    for name, row in parent_table.items():
        labels = [step[0] for step in row["steps"]]
        assert len(set(labels)) == len(labels), name
        assert sum(lb.startswith("index_array") for lb in labels) == cases.N_INDEX_ARRAYS + 1
        assert ("compute_omegas" in labels) == (cases.CASES[name][1] * cases.CASES[name][2] <= cases.OMEGAS_MAX)
        assert ("iterate 2 a_units = 3" in labels) == (name == "matrix-cores")


@pytest.mark.parametrize("name", list(cases.CASES))
def test_launches_and_outputs_match_the_parent(hip, parent_table, name):
    got, want = cases.run_case(hip, name), parent_table[name]
    assert got["launches"] and got["steps"]
    assert got["form"] == want["form"], name
    assert [s[0] for s in got["steps"]] == [s[0] for s in want["steps"]], name
    for step, step_p in zip(got["steps"], want["steps"]):
        assert step == step_p, (name, step[0])
    assert got["launches"] == want["launches"], name
