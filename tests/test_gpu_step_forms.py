"""The iteration changes its form -- two, three or four launches -- where it changed it, and computes what it computed,
before the decision moved from the free predicates of tu_iterate.hip into StepPlan (mmsbm_amd/csrc/step_plan.hpp): per
case of tests/step_form_cases.py every recorded entry -- the options that show the form, the byte model, the launches
per iteration of every kernel id and the SHA-256 of the parameters, after every step -- equals the table recorded from
the parent commit (tests/gpu_step_forms_parent.json, written by tests/step_form_cases.py).  The EM step has no atomics:
the bits are comparable."""
import json
import os

import pytest

import step_form_cases as cases
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mmsbm_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("-m gpu tests need a GPU: no HIP device visible (no CPU fallback exists)")
    import mmsbm_amd
    return mmsbm_amd


@pytest.fixture(scope="module")
def parent_table():
    with open(os.path.join(ROOT, "tests", "gpu_step_forms_parent.json")) as fh:
        return json.load(fh)


def _options(table, name, label):
    """(launches, pass_dense, fused) the parent showed after a step."""
    row = next(step for step in table[name] if step[0] == label + ": options")
    return tuple(float.fromhex(v) for v in row[1:])


def _launches(table, name, label):
    row = next(step for step in table[name] if step[0] == label + ": launches per iteration")
    return json.loads(row[1])


def test_the_table_walks_every_transition(parent_table):
    assert sorted(parent_table) == sorted(cases.CASES)
    for name, steps in parent_table.items():
        labels = [step[0] for step in steps]
        assert len(set(labels)) == len(labels), name
    # the forms the cases are named after are the ones the parent really took
    assert _options(parent_table, "three", "created") == (2.0, 0.0, 1.0)
    assert _options(parent_table, "three", "1 pass_dense = 1") == (4.0, 1.0, 1.0)
    assert _launches(parent_table, "three", "1 pass_dense = 1")["pair_block_kernel(T+S)"] == 0
    assert _options(parent_table, "three", "1 pass_dense = 0") == (2.0, 0.0, 1.0)
    assert _options(parent_table, "three", "2 fused = 1") == (2.0, 0.0, 1.0)       # forced: wins over pass_dense = 1
    assert _options(parent_table, "three", "3 fused = 0") == (4.0, 1.0, 0.0)
    assert _options(parent_table, "three", "set_slots 2") == (4.0, 0.0, 0.0)     # three launches need one slot
    assert _options(parent_table, "three", "set_slots 1") == (4.0, 1.0, 0.0)
    for name in ("two", "lists"):                                               # rows of 10 groups: never three
        assert all(float.fromhex(step[2]) == 0.0 for step in parent_table[name] if step[0].endswith(": options"))
        assert _options(parent_table, name, "created") == (2.0, 0.0, 1.0)
    for name in cases.CASES:                                                    # "mfma" = 2 takes the two launches away
        assert _options(parent_table, name, "4a mfma = 2")[0] == 4.0
        refused = {step[0]: step[1] for step in parent_table[name] if len(step) == 2}
        assert "fused: not available" in refused["4b fused = 1"] and refused["4d fused = 1"] == "ran"
        assert _options(parent_table, name, "4b fused = 1")[0] == 4.0 and _options(parent_table, name, "4d fused = 1")[0] == 2.0


@pytest.mark.parametrize("name", list(cases.CASES))
def test_forms_and_outputs_match_the_parent(hip, parent_table, name):
    got, want = cases.run_case(hip, name), parent_table[name]
    assert [s[0] for s in got] == [s[0] for s in want], name
    for step, step_p in zip(got, want):
        assert step == step_p, (name, step[0])
