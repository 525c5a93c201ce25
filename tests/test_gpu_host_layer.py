"""The host layer above the kernels answers as it did before its sessions, options and timers got one shape each: every
option value after create and after every step of tests/host_layer_cases.py, every refusal's code and text, and the
pairing of timed call to timer equal the table recorded from the parent commit (tests/gpu_host_layer_parent.json,
written by tests/host_layer_cases.py) -- and one predict session after the option steps returns what the same session
returned before them, so a moved predict session shows as a wrong answer and not only as a wrong flag."""
import json
import os

import numpy as np
import pytest

import host_layer_cases as cases
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
def problem():
    return cases.make_data()


@pytest.fixture(scope="module")
def parent_table():
    with open(os.path.join(ROOT, "tests", "gpu_host_layer_parent.json")) as fh:
        return json.load(fh)


def assert_rows_equal(got, expected, what):
    assert len(got) == len(expected), (what, len(got), len(expected))
    for row, row_p in zip(got, expected):
        assert row == row_p, (what, row, row_p)


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_options_match_the_parent(hip, problem, parent_table, shape):
    data, dims = problem
    predicted = []

    def predict(em):   # one whole predict session over the first 200 training rows
        em.predict_begin(data[:200], np.arange(dims[2], dtype=np.float64))
        per_slot = em.predict_add()
        predicted.append((per_slot, *em.predict_finish()))

    def start_and_predict(em):
        em.init_params(31)
        predict(em)

    first = shape == cases.SHAPES[0]
    got = cases.run_options(hip, shape, data, dims, created=start_and_predict if first else None,
                            stepped=predict if first else None)
    assert [row[0] for row in got] == ["created"] + [f"{name}={value}" for name, value in cases.STEPS]
    assert all(sorted(row[3]) == sorted(cases.OPTIONS) for row in got)
    assert_rows_equal(got, parent_table["options"][cases.shape_id(shape)], cases.shape_id(shape))
    if first:
        (slot_a, mean_a, stats_a), (slot_b, mean_b, stats_b) = predicted
        assert mean_a.shape == (200, dims[2]) and np.isfinite(mean_a).all() and mean_a.sum() > 0.0
        assert np.array_equal(slot_a, slot_b) and np.array_equal(mean_a, mean_b) and np.array_equal(stats_a, stats_b)


def test_refusals_match_the_parent(hip, problem, parent_table):
    data, dims = problem
    got = cases.run_refusals(hip, data, dims)
    assert_rows_equal(got, parent_table["refusals"], "refusals")
    by_label = {label: code for label, code, _ in got}
    assert by_label["no session: heldout_end"] != 0                     # heldout_end refuses without a session ...
    assert all(by_label[f"no session: {kind}_end"] == 0 for kind in ("recommend", "similar", "overlap"))   # ... the others accept
    assert all(code != 0 for label, code, _ in got if not label.endswith("_end")), got


def test_each_timed_call_feeds_its_own_timer(hip, problem, parent_table):
    data, dims = problem
    got = cases.run_timers(hip, data, dims)
    assert [row[0] for row in got] == ["created"] + [call for call, _ in cases.TIMED_CALLS]
    assert not any(got[0][1].values())
    for j, (call, timer) in enumerate(cases.TIMED_CALLS):
        after = got[j + 1][1]
        assert after[timer], (call, timer)                                # its own timer is > 0 ...
        still = {t for _, t in cases.TIMED_CALLS[j + 1:]} - {t for _, t in cases.TIMED_CALLS[:j + 1]}
        assert not any(after[t] for t in still), (call, after)           # ... and every timer not yet run reads 0.0
    assert_rows_equal(got, parent_table["timers"], "timers")
