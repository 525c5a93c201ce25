"""The C ABI's request checks answer as they did before they moved to csrc/abi_request.hpp and before core.py's copies
of the argument runs were merged: every request of tests/abi_request_cases.py -- faulty, empty, or faulty twice -- gives
the code and text (or, where accepted, the output shapes) of the table recorded from the parent commit
(tests/gpu_abi_requests_parent.json, written by tests/abi_request_cases.py)."""
import json
import os

import pytest

import abi_request_cases as cases
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got():
    from mmsbm_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("-m gpu tests need a GPU: no HIP device visible (no CPU fallback exists)")
    import mmsbm_amd
    data, dims = cases.make_data()
    return cases.run(mmsbm_amd, cases.prototypes(ROOT), data, dims)


@pytest.fixture(scope="module")
def parent_table():
    with open(os.path.join(ROOT, "tests", "gpu_abi_requests_parent.json")) as fh:
        return json.load(fh)


def test_requests_match_the_parent(got, parent_table):
    assert [row[0] for row in got] == [row[0] for row in parent_table]
    moved = [(row, row_p) for row, row_p in zip(got, parent_table) if row != row_p]
    assert not moved, moved[:10]


def test_the_table_holds_what_it_is_for(parent_table):
    """The strings the merge is about are pinned many times over, accepted requests are the empty ones, and a faulty
    request is never accepted."""
    text = "\n".join(str(row[2]) for row in parent_table)
    for needle, at_least in (("asked twice", 2), ("is repeated", 3), ("null argument", 60), ("out of range at entry", 40),
                             ("ascending and distinct", 25), ("negative n_users", 20), ("out of range at row", 20),
                             ("must be the number of training users", 2), ("n_cand outside", 25), ("[0] must be 0", 20),
                             ("decrease at", 20), ("more than 2^31 - 1", 15), ("n must be at least 1", 15),
                             ("expected (slots, users,", 5), ("added slots", 6)):
        assert text.count(needle) >= at_least, (needle, text.count(needle))
    for label, code, message in parent_table:
        accepted = code == 0
        empty = any(word in label for word in ("no users", "no pairs", "no items", "no rows", "no groups", "two items"))
        assert accepted == empty, (label, code, message)
    assert sum(code == "ValueError" for _, code, _ in parent_table) >= 25
