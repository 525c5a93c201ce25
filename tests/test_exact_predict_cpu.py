"""The exact predict / score reference of exact_predict.py against the oracle, its checker against the stand-in device,
and the conditions that make every case of test_gpu_exact_predict.py bite -- asserted here, on the CPU, for EVERY case
that file runs: a case that misses one is an error in the inputs, not something a GPU run could show.
"""
import numpy as np
import pytest

import exact_predict as xp
import fake_device as fake
from oracle import mmsbm_oracle as orc

CASE_NAMES = list(xp.CASES)
WRONG_RULES = {"last maximum": {"argmax": "last"}, "round half away": {"half": "away"},
               "one-off border < 1": {"border": "lt"}, "zero rows kept": {"zeros": "keep"}}


def power_of_two(S):
    return S & (S - 1) == 0


def loaded_fake(case, cls=fake.FakeHipEM):
    U, I, K, L, R, S = case["shape"]
    em = cls(case["data"], K, L, U, I, R, slots=S)
    for s, p in enumerate(case["params"]):
        em.select(s).set_params(*p)
    return em


# ---- the reference is the oracle's, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_reference_equals_the_oracle(name):
    case = xp.make_case(name)
    ref, rows, w, S = case["ref"], case["rows"], case["w"], len(case["params"])
    rats = [orc.prod_dist(rows, *p) for p in case["params"]]
    for s in range(S):
        xp.same_bits(ref["P"][s], rats[s], f"{name}: P of slot {s}")
        assert (ref["P"][s] <= 1.0).all() and (ref["nums"][s] >= 0).all()
    xp.same_bits(ref["mean"], np.array(rats).mean(axis=0), f"{name}: mean")
    scored = list(zip(rats, ref["slot_sums"])) + ([(ref["mean"], ref["mean_sums"])] if power_of_two(S) else [])
    for rat, sums in scored:
        want = orc.score_stats(rat, rows[:, 2], w)
        got = fake.FakeHipEM.final_stats(sums)
        assert sums[0] == (rat.sum(axis=1) != 0).sum()
        for key in ("accuracy", "one_off_accuracy", "mae", "s2", "s2pond"):
            assert got[key] == want[key], (name, key, got[key], want[key])
    if not power_of_two(S):                                  # the rounded mean: [0]..[3] exact all the same
        want = orc.score_stats(ref["mean"], rows[:, 2], w)
        got = fake.FakeHipEM.final_stats(ref["mean_sums"])
        for key in ("accuracy", "one_off_accuracy", "s2"):
            assert got[key] == want[key], (name, key)


def test_planted_rows_hold_what_they_are_named_for():
    for R in xp.RATING_RS:
        for kind in ("ties", "half"):
            pat = xp.planted(R, kind)
            assert (pat >= 0).all() and (pat.sum(axis=1) <= xp.P_DEN).all()
            if R == 1:
                continue
            top = (pat == pat.max(axis=1, keepdims=True)) & (pat.sum(axis=1, keepdims=True) > 0)
            spans = {tuple(np.flatnonzero(t).tolist()) for t in top if t.sum() > 1}
            assert {(r, r + 1) for r in range(R - 1)} <= spans                       # next to each other, even and odd r
            if R >= 3:
                assert {(r, r + 2) for r in range(R - 2)} <= spans                   # two apart
                assert {(r, r + 1, r + 2) for r in range(R - 2)} <= spans            # three in a row
            assert tuple(range(R)) in spans                                          # the flat row
            hw = xp.half_way(pat, xp.P_DEN, np.arange(R))
            floors = set(((pat @ np.arange(R)) // xp.P_DEN)[hw].tolist())
            assert {0} <= floors and (R < 3 or {0, 1} <= floors)


# ---- the checker, driven by the stand-in device ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_checker_passes_on_the_stand_in_device(name):
    case = xp.make_case(name)
    em = loaded_fake(case)
    xp.check_prod_dist(em, case, "stand-in")
    mean, raw = xp.check_session(em, case, "stand-in")
    assert mean.shape == (len(case["rows"]), case["shape"][4]) and raw[0] == case["ref"]["mean_sums"][0]
    for n in xp.ROW_COUNTS.get(name, ()):
        xp.check_session(em, xp.prefix(case, n), f"stand-in, {n} rows")


class HalfUpFake(fake.FakeHipEM):
    """A device that rounds the weighted mean half UP."""

    def _raw(self, rat):
        raw = super()._raw(rat)
        keep = rat.sum(axis=1) != 0
        raw[4] = (self._test[keep, 2] == np.floor(rat[keep] @ self._weights + 0.5)).sum()
        return raw


class LastMaximumFake(fake.FakeHipEM):
    """A device whose argmax is the LAST maximum."""

    def _raw(self, rat):
        keep = rat.sum(axis=1) != 0
        real = self._test[keep, 2]
        pred = rat.shape[1] - 1 - np.argmax(rat[keep][:, ::-1], axis=1)
        raw = super()._raw(rat)
        d = np.abs(pred - real)
        raw[1:4] = (d == 0).sum(), (d <= 1).sum(), d.sum()
        return raw


class StaleSumFake(fake.FakeHipEM):
    """A device whose second session starts from the first one's sum."""
    _kept = None

    def predict_finish(self, want_matrix=True):
        if StaleSumFake._kept is not None and StaleSumFake._kept.shape == self._rats[0].shape:
            self._rats[0] = self._rats[0] + StaleSumFake._kept
        StaleSumFake._kept = np.sum(self._rats, axis=0)
        return super().predict_finish(want_matrix)


@pytest.mark.parametrize("cls", [HalfUpFake, LastMaximumFake])
def test_checker_fails_on_a_device_with_a_wrong_rule(cls):
    case = xp.make_case("R5")
    with pytest.raises(AssertionError, match="sums of slot 0"):
        xp.check_session(loaded_fake(case, cls), case)


def test_checker_fails_on_a_stale_sum():
    case = xp.make_case("R4")
    StaleSumFake._kept = None
    em = loaded_fake(case, StaleSumFake)
    xp.check_session(em, case)
    with pytest.raises(AssertionError, match="mean"):
        xp.check_session(em, case)


# ---- every GPU case bites --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_conditions_hold_for_every_gpu_case(name):
    case = xp.make_case(name)
    U, I, K, L, R, S = case["shape"]
    ref, real, w = case["ref"], case["rows"][:, 2], case["w"]
    need = xp.required(case["family"], R)
    dists = [("slot 0", ref["nums"][0], xp.SCALE)] + ([("mean", ref["total"], xp.SCALE * S)] if power_of_two(S) else [])
    for what, num, den in dists:
        have = xp.conditions(num, den, real, w)
        short = {k: (have[k], v) for k, v in need.items() if have[k] < v}
        assert not short, (name, what, short, have)
        assert have["zero"] < have["rows"]
    assert len(case["rows"]) <= 4000 and set(real.tolist()) <= set(range(R))
    if not power_of_two(S):                                  # the cap on [4] of a rounded mean: at most 2 % of the rows
        assert ref["mean_half"].sum() <= 0.02 * len(real), (name, int(ref["mean_half"].sum()), len(real))
    for n in xp.ROW_COUNTS.get(name, ()):
        assert n <= len(case["rows"]), (name, n)
    if K > 1024:                                             # rows whose answer needs the columns past the first 1,024
        cut = [(t[:, :1024], e, p[:1024]) for t, e, p in case["params"]]
        short_num = xp.numerators(cut[0], case["rows"][:, 0], case["rows"][:, 1])
        assert ((short_num != ref["nums"][0]).any(axis=1)).sum() >= 50


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if xp.CASES[n][2][4] >= 2])
def test_inputs_tell_the_wrong_rules_apart(name):
    """Each wrong rule changes at least one sum the GPU test compares by equality.  (Rounding half away from zero can
    differ from half to even only on a pond of even + 1/2: the family without one is left out for that rule.)"""
    case = xp.make_case(name)
    ref, S = case["ref"], len(case["params"])
    upto = 6 if power_of_two(S) else 4
    for rule, kw in WRONG_RULES.items():
        if rule == "round half away" and "half_even" not in xp.required(case["family"], case["shape"][4]):
            continue
        alt = xp.exact_session(case["params"], case["rows"], case["w"], **kw)
        changed = [s for s in range(S) if not np.array_equal(alt["slot_sums"][s], ref["slot_sums"][s])]
        mean_changed = not np.array_equal(alt["mean_sums"][:upto], ref["mean_sums"][:upto])
        assert changed and (mean_changed or rule == "round half away" and not power_of_two(S)), (name, rule)


def test_constant_family_with_two_ratings_meets_a_half_way_pond():
    """... where the family can have one: the flat row (1/2, 1/2) under the rating indices."""
    case = xp.make_case("constantR2")
    alt = xp.exact_session(case["params"], case["rows"], case["w"], half="away")
    assert alt["slot_sums"][0][4] != case["ref"]["slot_sums"][0][4]


def test_signed_weights_give_negative_half_way_ponds():
    """-0.5 rounds to -0.0, which equals rating 0: rows with pond = -1/2 and real = 0 count as hits."""
    hits = 0
    for name in CASE_NAMES:
        case = xp.make_case(name)
        if case["w"].min() >= 0:
            continue
        pn = case["ref"]["nums"][0] @ case["w"].astype(np.int64)
        hits += int(((2 * pn == -xp.SCALE) & (case["rows"][:, 2] == 0)).sum())
    assert hits >= 20
    assert np.round(-0.5) == 0.0 and xp.six_sums(np.array([[4, 0, 0]]), 16, [0], np.array([-2.0, 0.0, 1.0]))[4] == 1.0
