"""The pair stage's launch plan, seen through the public API, is the one the library chose before the plan became one
value (mmsbm_amd/csrc/pair_plan.hpp): for the smallest shape that reaches each plan, under the creation knobs and after
every step of the option sequences, the options that show the plan equal the table recorded from the parent commit
(tests/gpu_pair_plan_parent.json, written by tests/pair_plan_cases.py) -- and after every sequence one
update_coefficients() equals the oracle's at the step tolerance, so a stale plan shows as a wrong result and not only as
a wrong flag."""
import json
import os

import pytest

import pair_plan_cases as cases
from conftest import ROOT, rel_err
from oracle import mmsbm_factorised as fact
from oracle import mmsbm_oracle as orc

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-12
DENSE_ORACLE_MAX = 4096   # K x L entries per rating up to which the dense oracle's (ratings x K x L) arrays stay small


@pytest.fixture(scope="module")
def hip():
    from mmsbm_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("-m gpu tests need a GPU: no HIP device visible (no CPU fallback exists)")
    import mmsbm_amd
    return mmsbm_amd


@pytest.fixture(scope="module")
def problem():
    data, dims = cases.make_data()
    return data, dims, orc.degrees(data, dims[0], dims[1])


@pytest.fixture(scope="module")
def parent_table():
    with open(os.path.join(ROOT, "tests", "gpu_pair_plan_parent.json")) as fh:
        return json.load(fh)


_steps = {}


def oracle_step(problem, k, l):
    """The start of a shape and the oracle's update_coefficients() of it: computed once per shape, never changed."""
    if (k, l) not in _steps:
        data, (n_u, n_i, n_r), (d_u, d_i) = problem
        start = orc.init_params(31, n_u, n_i, n_r, k, l, d_u, d_i)
        checker = orc if k * l <= DENSE_ORACLE_MAX else fact
        _steps[(k, l)] = (start, checker.update_coefficients(data, *start))
    return _steps[(k, l)]


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_plan_and_step_match_the_parent(hip, problem, parent_table, case):
    data, dims, _ = problem
    start, want = oracle_step(problem, case[0], case[1])

    def step_matches(em, sequence):
        for got, w, nm in zip(em.update_coefficients(), want, ("n_theta", "n_eta", "n_pr")):
            assert rel_err(got, w) < TOL_STEP, (cases.case_id(case), sequence, nm)

    got = cases.run_case(hip.HipEM, case, data, dims, prepare=lambda em: em.set_params(*start),
                         after_sequence=step_matches)
    expected = parent_table[cases.case_id(case)]
    assert sorted(got) == sorted(expected)
    for sequence, rows in got.items():
        assert len(rows) == len(expected[sequence]), sequence
        for (step, options), (step_p, options_p) in zip(rows, expected[sequence]):
            assert step == step_p and options == options_p, (cases.case_id(case), sequence, step, options, options_p)
