"""Every serving query launches what it launched, and returns what it returned, before its host side moved onto shared
helpers and the plans of serve_plan.hpp: per case of tests/serving_launch_cases.py the launch count per kernel name and
the SHA-256 of every output array equal the table recorded from the parent commit
(tests/gpu_serving_launches_parent.json, written by tests/serving_launch_cases.py)."""
import json
import os

import pytest

import exact_models as xm
import serving_launch_cases as cases
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
    with open(os.path.join(ROOT, "tests", "gpu_serving_launches_parent.json")) as fh:
        return json.load(fh)


def test_the_table_holds_these_cases(parent_table):
    assert cases.BASIC == xm.SPLIT[1]
    assert xm.batch_users(cases.WIDE[1], cases.WIDE[0]) == 128     # 129 rows: two batches, 128 + 1
    assert sorted(parent_table) == sorted(cases.CASES)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_launches_and_outputs_match_the_parent(hip, parent_table, name):
    got, want = cases.run_case(hip, name), parent_table[name]
    assert got["launches"] and got["outputs"]
    assert got["launches"] == want["launches"], name
    assert got["outputs"] == want["outputs"], name
