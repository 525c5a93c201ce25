"""The staged starts of staged_params.py are what they claim to be, and unambiguous in the reference alone.

test_gpu_staged.py holds the device to 1e-12 element-wise on these inputs.  That bar only means something if the inputs
reach the branches they are named after (clamped rows, clamped elements, exact zeros, subnormals) and if the expected
values do not depend on how a CPU evaluation associates its sums.  So, for every family at one shape with K L <= 1,024
and one beyond, three independent CPU evaluations of one M-step -- the dense oracle (the reference's order), the
factorised checker (the device's kind of order) and an np.longdouble restatement of the same formulas -- must agree
element-wise within 1e-13, with the same zero pattern, and hardly any expected entry may sit at or below ELEMENT_FLOOR,
where elem_rel_err compares absolutely only.  These are conditions on the inputs: a family that fails one gets other
inputs, never another bar.
"""
import numpy as np
import pytest

from border_tables import longdouble_step    # (the np.longdouble restatement of one M-step: shared with the border tables)
from conftest import ELEMENT_FLOOR, elem_rel_err
from oracle import mmsbm_factorised as fact
from oracle import mmsbm_oracle as orc
from staged_params import FAMILIES, clamped_elements, clamped_rows, staged, uniform_rows

SHAPES = [(7, 13), (36, 30)]          # K L = 91 and 1,080: either side of the 1,024 at which the pair stage changes family
N_U, N_I, N_R, N_ROWS = 120, 80, 5, 3000
AGREE = 1e-13


def below_floor_share(arrays):
    """Largest share, over the arrays, of the nonzero entries at or below ELEMENT_FLOOR."""
    return max(float(np.mean((np.abs(a) <= ELEMENT_FLOOR) & (a != 0))) for a in arrays)


@pytest.fixture(scope="module")
def cases():
    """(k, l, family) -> everything the tests below look at; each evaluation is made once."""
    out = {}
    for k, l in SHAPES:
        rng = np.random.default_rng(k * 131 + l)
        data = uniform_rows(rng, N_ROWS, N_U, N_I, N_R)
        d_u, d_i = orc.degrees(data, N_U, N_I)
        for name in FAMILIES + ("subcolumn",):
            theta, eta, pr = staged(name, rng, data, N_U, N_I, N_R, k, l)
            dense = orc.update_coefficients(data, theta, eta, pr)
            ld_num, ld_par = longdouble_step(data, theta, eta, pr, d_u, d_i)
            out[k, l, name] = dict(
                rows=clamped_rows(data, theta, eta, pr), elements=clamped_elements(data, theta, eta, pr),
                dense=dense, fact=fact.update_coefficients(data, theta, eta, pr), ld=ld_num,
                dense_par=orc.em_step(data, theta, eta, pr, d_u, d_i), fact_par=fact.em_step(data, theta, eta, pr, d_u, d_i),
                ld_par=ld_par)
    return out


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("k,l", SHAPES)
def test_clamped_rows_and_elements(cases, k, l, name):
    c = cases[k, l, name]
    if name == "rowborder":
        assert 0.15 <= c["rows"] <= 0.85, c["rows"]
    elif name == "tiny":
        assert c["rows"] == 1.0
    elif name in ("dead", "sub"):
        assert c["rows"] < 0.01, c["rows"]
    if name in ("late", "border"):
        assert c["elements"] > 0.05, c["elements"]


@pytest.mark.parametrize("name", FAMILIES + ("subcolumn",))
@pytest.mark.parametrize("k,l", SHAPES)
def test_the_three_references_agree_after_one_step(cases, k, l, name):
    """Numerators and normalised parameters; of `subcolumn` the numerators only (what it is used for: its p' is a ratio
    of subnormal sums and differs by 3e-8 between the evaluations, which is why `sub` leaves every other row normal)."""
    c = cases[k, l, name]
    for kind in ("",) if name == "subcolumn" else ("", "_par"):
        dense, fac, ld = c["dense" + kind], c["fact" + kind], c["ld" + kind]
        for a, b, what in ((fac, dense, "factorised vs dense"), (dense, ld, "dense vs long double"), (fac, ld, "factorised vs long double")):
            for x, y, nm in zip(a, b, ("theta", "eta", "pr")):
                err = elem_rel_err(x, y)
                assert err <= AGREE, (what, kind or "numerators", nm, err)


@pytest.mark.parametrize("name", ["dead", "border"])
@pytest.mark.parametrize("k,l", SHAPES)
def test_dense_and_factorised_have_the_same_zero_pattern(cases, k, l, name):
    c = cases[k, l, name]
    for kind in ("dense", "dense_par"):
        for x, y, nm in zip(c[kind], c[kind.replace("dense", "fact")], ("theta", "eta", "pr")):
            assert np.array_equal(x == 0, y == 0), (kind, nm)
            assert (x == 0).any(), (kind, nm)      # ... and there are zeros to speak of


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("k,l", SHAPES)
def test_hardly_any_expected_entry_is_below_the_floor(cases, k, l, name):
    """At or below ELEMENT_FLOOR an entry is compared absolutely only; the cap keeps the floor from hiding a failure."""
    c = cases[k, l, name]
    share = max(below_floor_share(c["dense"]), below_floor_share(c["dense_par"]))
    if name == "sub":
        assert 0.0 < share <= 0.25, share
    else:
        assert share == 0.0, share
