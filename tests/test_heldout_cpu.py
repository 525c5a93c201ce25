"""Held-out log-likelihood and the validation-monitored fit without a GPU: the numpy restatement of
mmsbm_amd/csrc/heldout.hpp (what test_gpu_heldout.py holds the device to), and the host class's logic -- encoding, the
first-best rule, patience, the curve, the refusals -- against a stand-in device built on that restatement.

    t_s[k] = sum_l p_s[k, l, r] eta_s[i, l]      P_s(m) = sum_k theta_s[u, k] t_s[k]
    ll_s   = sum_m log(max(P_s(m), eps))         mean: (sum_s P_s(m)) / S, one division, and its ll
"""
import os
import re
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import exact_models as xm
import fake_device
from conftest import ROOT
from oracle import mmsbm_oracle as orc
from test_recommend_cpu import string_frame

EPS = np.finfo(np.float64).eps


# ---- the restatement ------------------------------------------------------------------------------------------------
def restate_p(params, rows):
    """(M,) P(observed rating | user, item) of every row [user, item, rating] under one parameter set."""
    theta, eta, p = params
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    t = np.einsum("klm,ml->mk", p[:, :, rows[:, 2]], eta[rows[:, 1]])
    return (theta[rows[:, 0]] * t).sum(axis=1) + 0.0


def restate_ll(prob):
    return float(np.log(np.maximum(prob, EPS)).sum()) if len(prob) else 0.0


def restate_heldout(params_list, rows):
    """{"p": (S, M), "ll": [S], "mean_p": (M,), "mean_ll"}: every slot alone, and the mean over the slots -- the sum
    over the slots in their order first, then ONE division."""
    ps = np.array([restate_p(prm, rows) for prm in params_list]).reshape(len(params_list), -1)
    tot = np.zeros(ps.shape[1])
    for row in ps:
        tot = tot + row
    mean = tot / float(len(params_list))
    return {"p": ps, "ll": [restate_ll(x) for x in ps], "mean_p": mean, "mean_ll": restate_ll(mean)}


def ll_bound(K, L, prob):
    """|device - restatement| allowed for the log-likelihood of rows with probabilities ``prob``: each P carries a
    chain of K L + K products and additions (relative error below (K L + 2) u once the second-order terms are left to
    the factor 2), which moves its log by as much absolutely; every log is rounded once and the M logs are summed, each
    addition rounding a partial sum no larger than sum |log|.  u = 2^-53; the factor 2 covers both sides."""
    logs = np.abs(np.log(np.maximum(prob, EPS)))
    m = len(prob)
    return 2.0 * 2.0 ** -53 * ((K * L + 2) * m + (m + 1) * float(logs.sum()))


def random_problem(rng, U, I, R, K, L, S, n_rows):
    params = [(rng.random((U, K)), rng.random((I, L)), orc.normalize_with_self(rng.random((K, L, R)))) for _ in range(S)]
    rows = np.stack([rng.integers(0, U, n_rows), rng.integers(0, I, n_rows), rng.integers(0, R, n_rows)], 1)
    return params, rows


def test_restatement_equals_the_triple_loop():
    rng = np.random.default_rng(0)
    params, rows = random_problem(rng, 6, 7, 3, 4, 5, 2, 40)
    got = restate_heldout(params, rows)
    for s, (theta, eta, p) in enumerate(params):
        for m, (u, i, r) in enumerate(rows.tolist()):
            want = 0.0
            for k in range(4):
                t = 0.0
                for l in range(5):
                    t += p[k, l, r] * eta[i, l]
                want += theta[u, k] * t
            assert abs(got["p"][s, m] - want) <= 1e-15 * max(want, 1.0)
        assert got["ll"][s] == pytest.approx(sum(np.log(max(x, EPS)) for x in got["p"][s]), rel=1e-14)
    assert np.allclose(got["mean_p"], got["p"].mean(axis=0), rtol=1e-15, atol=0)
    assert restate_heldout(params, rows[:0])["mean_ll"] == 0.0 and restate_ll(np.zeros(0)) == 0.0


def test_restatement_is_the_oracle_prod_dist_at_the_observed_rating():
    rng = np.random.default_rng(1)
    for U, I, R, K, L in ((9, 11, 5, 3, 4), (5, 4, 1, 6, 2), (30, 20, 4, 10, 10)):
        params, rows = random_problem(rng, U, I, R, K, L, 1, 200)
        theta, eta, p = params[0]
        theta, eta = theta / theta.sum(axis=1, keepdims=True), eta / eta.sum(axis=1, keepdims=True)   # memberships: P <= 1
        dist = orc.prod_dist(rows, theta, eta, p)
        want = dist[np.arange(len(rows)), rows[:, 2]]
        assert np.allclose(restate_p((theta, eta, p), rows), want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("S", [1, 3, 4])
def test_mean_p_is_exact_on_models_without_rounding(S):
    """Family `mixed`: theta and eta in eighths, p in sixteenths -- every product a multiple of 2^-10, every sum exact
    in any order, and the mean one correctly rounded division of an exact numerator."""
    case = xm.make_case("mixed", "stars", (12, 20, 4, 5, 3, S), n_random=60)
    rows = case["data"][:50]
    got = restate_heldout(case["params"], rows)
    for m, (u, i, r) in enumerate(rows.tolist()):
        num = Fraction(0)
        for theta, eta, p in case["params"]:
            for k in range(4):
                for l in range(5):
                    num += Fraction(theta[u, k]) * Fraction(p[k, l, r]) * Fraction(eta[i, l])
        assert num.denominator <= 1024 and float(num) == num
        assert xm.bits(got["mean_p"][m]) == xm.bits(float(num) / float(S))


def test_clamped_rows_and_the_bound_on_a_known_case():
    rng = np.random.default_rng(2)
    (theta, eta, p), rows, _ = xm.impossible_rating_case(rng, 8, 9, 4, 3, 4, [3, 6, 4])
    rows = np.stack([rows[:, 0] % 8, rows[:, 1], rows[:, 2]], 1)
    prob = restate_p((theta, eta, p), rows)
    dead = rows[:, 2] == 3
    assert dead.any() and (prob[dead] == 0.0).all() and (prob[~dead] > 0).all()
    assert restate_ll(prob) == pytest.approx(np.log(EPS) * dead.sum() + np.log(prob[~dead]).sum(), rel=1e-14)
    # two association orders of the same sum stay far inside the bound, one wrong row far outside it
    params, many = random_problem(rng, 300, 200, 5, 20, 20, 1, 100_000)
    pr = restate_p(params[0], many)
    logs = np.log(np.maximum(pr, EPS))
    bound = ll_bound(20, 20, pr)
    assert abs(float(logs.sum()) - float(np.cumsum(logs)[-1])) < 1e-2 * bound < 1e-7
    assert abs(np.log(pr[0] * 1.001) - logs[0]) > 100 * bound


# ---- the host class against a stand-in device -------------------------------------------------------------------------
class HeldoutFakeHipEM(fake_device.FakeHipEM):
    """FakeHipEM with the held-out session and the snapshots, answered by the restatement.  SCRIPT: when set, a list of
    per-check value lists that heldout_eval hands out in order instead (the tests of the monitor's rules)."""
    SCRIPT = None

    def heldout_begin(self, rows):
        self._ho = {"rows": np.asarray(rows, dtype=np.int64).reshape(-1, 3), "added": []}
        fake_device.LOG.append(("heldout_begin", len(self._ho["rows"])))

    def heldout_eval(self):
        assert getattr(self, "_ho", None) is not None, "no session"
        fake_device.LOG.append(("heldout_eval", self.slots))
        if HeldoutFakeHipEM.SCRIPT is not None:
            return np.asarray(HeldoutFakeHipEM.SCRIPT.pop(0), dtype=np.float64)
        return np.array([restate_ll(restate_p(prm, self._ho["rows"])) for prm in self._params])

    def heldout_add(self):
        self._ho["added"].append(self._params[self._sel])
        fake_device.LOG.append(("heldout_add", self._sel))
        return np.float64(restate_ll(restate_p(self._params[self._sel], self._ho["rows"])))

    def heldout_mean(self, want_rows=True):
        got = restate_heldout(self._ho["added"], self._ho["rows"])
        return (got["mean_p"] if want_rows else None), np.float64(got["mean_ll"])

    def heldout_end(self):
        self._ho = None
        fake_device.LOG.append(("heldout_end", None))

    def set_slots(self, n):
        super().set_slots(n)
        self._snap = [None] * self.slots

    def snapshot_save(self):
        self._snap[self._sel] = tuple(a.copy() for a in self._params[self._sel])
        fake_device.LOG.append(("snapshot_save", self._sel))

    def snapshot_get(self):
        assert self._snap[self._sel] is not None, "nothing saved"
        fake_device.LOG.append(("snapshot_get", self._sel))
        return tuple(a.copy() for a in self._snap[self._sel])


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", HeldoutFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(HeldoutFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    monkeypatch.setattr(HeldoutFakeHipEM, "SCRIPT", None)
    fake_device.LOG.clear()
    return host


def events(*names):
    return [(e, d) for e, d in fake_device.LOG if e in names]


def split_frame():
    df = string_frame(n_obs=160)
    return df.iloc[:120], df.iloc[120:]


def test_log_likelihood_encodes_drops_unseen_rows_and_leaves_predictions_alone(host, caplog):
    train, held = split_frame()
    m = host.MMSBM(2, 3, iterations=3, sampling=3, seed=7)
    m.fit(train, silent=True)
    m.predict(held)
    kept = (m.prediction_matrix.copy(), m.test.copy(), m.score(silent=True))
    extra = pd.DataFrame({"users": ["nobody", held.iloc[0, 0]], "items": [held.iloc[0, 1], "nothing"], "ratings": [3, 3]})
    fake_device.LOG.clear()
    with caplog.at_level("WARNING"):
        got = m.log_likelihood(pd.concat([held, extra], ignore_index=True))
    rows = m.data_handler.transform(held, m.logger)
    assert "nobody" in caplog.text and "nothing" in caplog.text
    want = restate_heldout([(r["theta"], r["eta"], r["pr"]) for r in m.results], rows)
    assert got["rows"] == len(rows) > 0
    assert got["log_likelihood"] == want["mean_ll"] and got["per_restart"] == want["ll"]
    assert got["perplexity"] == float(np.exp(-want["mean_ll"] / len(rows)))
    assert set(got) == {"rows", "log_likelihood", "per_restart", "perplexity"}
    assert [e for e, _ in events("heldout_begin", "heldout_add", "heldout_end")] == \
        ["heldout_begin"] + ["heldout_add"] * 3 + ["heldout_end"]
    assert np.array_equal(m.prediction_matrix, kept[0]) and np.array_equal(m.test, kept[1])
    assert m.score(silent=True)["stats"] == kept[2]["stats"]


def test_log_likelihood_refuses_a_share_of_a_model(host):
    train, held = split_frame()
    m = host.MMSBM(2, 3, iterations=2, sampling=3, seed=7)
    m.data_handler = host.Encoder()
    m.fit_encoded(m.data_handler.fit_transform(train), restarts=[0, 2])
    with pytest.raises(RuntimeError, match="2 of its 3 restarts"):
        m.log_likelihood(held)


def test_plain_fit_makes_no_heldout_or_snapshot_call(host):
    train, _ = split_frame()
    m = host.MMSBM(2, 3, iterations=5, sampling=2, seed=7, check_every=2)
    m.fit(train, silent=True)
    assert not [e for e, _ in fake_device.LOG if e.startswith(("heldout", "snapshot"))]
    assert m.validation_curve == {} and m.best_iteration == {}
    assert all(set(r) == {"likelihood", "pr", "theta", "eta"} for r in m.results)


def test_monitored_fit_checks_every_check_every_and_after_the_last_iteration(host):
    train, held = split_frame()
    m = host.MMSBM(2, 3, iterations=7, sampling=2, seed=7, check_every=3)
    m.fit(train, silent=True, validation=held)
    assert [d for e, d in events("iterate")] == [3, 3, 1]
    assert [d for e, d in events("heldout_eval")] == [2, 2, 2]           # one evaluation per check for the whole batch
    for i in range(2):
        assert [it for it, _ in m.validation_curve[i]] == [3, 6, 7]
        values = [v for _, v in m.validation_curve[i]]
        assert m.best_iteration[i] == [3, 6, 7][int(np.argmax(values))]
        assert m.results[i]["validation"] == max(values)
        assert m.iterations_run[i] == 7
    # the kept parameters are those of a plain fit stopped at the best check, with their own training likelihood
    for i in range(2):
        plain = host.MMSBM(2, 3, iterations=m.best_iteration[i], sampling=2, seed=7)
        plain.fit(train, silent=True)
        for key in ("theta", "eta", "pr"):
            assert np.array_equal(m.results[i][key], plain.results[i][key])
        assert m.results[i]["likelihood"] == plain.results[i]["likelihood"]
    assert fake_device.LOG.count(("heldout_end", None)) >= 1


def scripted(host, script, iterations, check_every, patience=None, sampling=2):
    train, held = split_frame()
    HeldoutFakeHipEM.SCRIPT = [list(v) for v in script]
    m = host.MMSBM(2, 3, iterations=iterations, sampling=sampling, seed=7, check_every=check_every,
                   restarts_per_launch=sampling)
    m.fit(train, silent=True, validation=held, patience=patience)
    return m


def test_first_best_rule_only_a_strictly_greater_value_replaces_the_best(host):
    m = scripted(host, [(-5.0, -9.0), (-5.0, -7.0), (-4.0, -7.0), (-4.0, -8.0)], iterations=8, check_every=2)
    assert m.best_iteration == {0: 6, 1: 4}
    assert [r["validation"] for r in m.results] == [-4.0, -7.0]
    assert events("snapshot_save") == [("snapshot_save", 0),                           # before any iteration: room for all
                                       ("snapshot_save", 0), ("snapshot_save", 1),     # first check: both
                                       ("snapshot_save", 1), ("snapshot_save", 0)]     # then only the new bests
    assert fake_device.LOG.index(("snapshot_save", 0)) < min(j for j, e in enumerate(fake_device.LOG) if e[0] == "iterate")
    assert m.validation_curve[1] == [(2, -9.0), (4, -7.0), (6, -7.0), (8, -8.0)]
    # restart 0's best is not the last state, restart 1's neither: both come back through the host, once each
    assert events("snapshot_get") == [("snapshot_get", 0), ("snapshot_get", 1)]


def test_patience_counts_per_restart_and_stops_per_batch(host):
    # restart 0 stalls from the second check, restart 1 improves until the third: with patience 2 the batch stops
    # after the check at which BOTH have gone two checks without a new best -- the fifth
    script = [(-5.0, -9.0), (-6.0, -8.0), (-6.0, -7.0), (-6.0, -7.5), (-6.0, -7.0), (0.0, 0.0), (0.0, 0.0)]
    m = scripted(host, script, iterations=14, check_every=2, patience=2)
    assert m.iterations_run == {0: 10, 1: 10}
    assert m.best_iteration == {0: 2, 1: 6}
    assert len(m.validation_curve[0]) == 5 and [d for _, d in events("iterate")] == [2] * 5
    # without patience every iteration runs
    m = scripted(host, script, iterations=14, check_every=2)
    assert m.iterations_run == {0: 14, 1: 14} and m.best_iteration == {0: 12, 1: 12}


def test_a_restart_whose_last_state_is_its_best_needs_no_round_trip(host):
    m = scripted(host, [(-5.0, -9.0), (-4.0, -9.5)], iterations=4, check_every=2)
    assert m.best_iteration == {0: 4, 1: 2}
    assert events("snapshot_get") == [("snapshot_get", 1)]


def test_queries_after_a_monitored_fit_use_the_kept_parameters(host):
    train, held = split_frame()
    m = scripted(host, [(-5.0, -9.0), (-6.0, -9.5), (-7.0, -9.9)], iterations=6, check_every=2)
    plain = host.MMSBM(2, 3, iterations=2, sampling=2, seed=7)
    plain.fit(train, silent=True)
    assert np.array_equal(m.predict(held), plain.predict(held))


def test_refusals_come_before_any_device_call(host):
    train, held = split_frame()
    m = host.MMSBM(2, 3, iterations=4, sampling=1, seed=7, tol=1e-3)
    with pytest.raises(ValueError, match="two stop rules"):
        m.fit(train, silent=True, validation=held)
    m = host.MMSBM(2, 3, iterations=4, sampling=1, seed=7)
    for bad in (0, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="positive integer"):
            m.fit(train, silent=True, validation=held, patience=bad)
    with pytest.raises(ValueError, match="needs a validation set"):
        m.fit(train, silent=True, patience=2)
    strangers = pd.DataFrame({"users": ["x", "y"], "items": ["a", "b"], "ratings": [1, 2]})
    with pytest.raises(ValueError, match="no row left"):
        m.fit(train, silent=True, validation=strangers)
    enc = host.Encoder().fit_transform(train)
    with pytest.raises(ValueError, match="no row left"):
        m.fit_encoded(enc, validation=np.array([[10 ** 6, 0, 0]]))
    with pytest.raises(ValueError, match="needs a validation set"):
        m.fit_encoded(enc, patience=1)
    assert not fake_device.LOG


def test_snapshots_that_do_not_fit_halve_the_batch_like_slots_that_do_not(host, monkeypatch):
    """The first snapshot_save allocates a further theta + eta + p per slot: made before any iteration, its refusal
    splits the batch as a refused set_slots does."""
    train, held = split_frame()

    def save(self):
        if self.slots > 1:
            raise host.HipLibraryError("mmsbm_hip_snapshot_save", 5, "snapshot: needs more device memory")
        HeldoutFakeHipEM.__dict__["_plain_save"](self)
    monkeypatch.setattr(HeldoutFakeHipEM, "_plain_save", HeldoutFakeHipEM.snapshot_save, raising=False)
    monkeypatch.setattr(HeldoutFakeHipEM, "snapshot_save", save)
    m = host.MMSBM(2, 3, iterations=4, sampling=2, seed=7, check_every=2, restarts_per_launch=2)
    m.fit(train, silent=True, validation=held)
    assert [d for e, d in events("set_slots")][-3:] == [2, 1, 1]
    assert not [1 for j, e in enumerate(fake_device.LOG) if e[0] == "iterate" and
                fake_device.LOG[:j].count(("set_slots", 1)) == 0]              # nothing iterated in the batch of two
    whole = host.MMSBM(2, 3, iterations=4, sampling=2, seed=7, check_every=2, restarts_per_launch=1)
    whole.fit(train, silent=True, validation=held)
    for a, b in zip(m.results, whole.results):
        assert all(np.array_equal(a[k], b[k]) for k in ("theta", "eta", "pr")) and a["validation"] == b["validation"]


def test_a_refused_monitored_fit_leaves_a_fitted_model_as_it_was(host):
    train, held = split_frame()
    m = host.MMSBM(2, 3, iterations=2, sampling=1, seed=7)
    m.fit(train, silent=True)
    encoder, results = m.data_handler, m.results
    strangers = pd.DataFrame({"users": ["x", "y"], "items": ["a", "b"], "ratings": [1, 2]})
    fake_device.LOG.clear()
    with pytest.raises(ValueError, match="no row left"):
        m.fit(held, silent=True, validation=strangers)
    assert m.data_handler is encoder and m.results is results and not fake_device.LOG


def test_fit_encoded_takes_encoded_validation_rows(host):
    train, held = split_frame()
    enc = host.Encoder()
    t = enc.fit_transform(train)
    v = enc.transform(held, None)
    m = host.MMSBM(2, 3, iterations=4, sampling=2, seed=7, check_every=2)
    m.fit_encoded(t, validation=np.concatenate([v, [[10 ** 6, 0, 0]]]), patience=3)
    assert events("heldout_begin") == [("heldout_begin", len(v))]
    assert sorted(m.best_iteration) == [0, 1] and all(r["validation"] == max(x for _, x in m.validation_curve[i])
                                                      for i, r in enumerate(m.results))


# ---- header, signatures and wrappers agree --------------------------------------------------------------------------
NEW_SYMBOLS = {"mmsbm_hip_heldout_begin": 5, "mmsbm_hip_heldout_eval": 2, "mmsbm_hip_heldout_add": 2,
               "mmsbm_hip_heldout_mean": 3, "mmsbm_hip_heldout_end": 1, "mmsbm_hip_snapshot_save": 1,
               "mmsbm_hip_snapshot_get": 4}


def test_header_signatures_and_wrappers_agree():
    from mmsbm_amd import _lib
    from mmsbm_amd.core import HipEM
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmsbm_hip.h")).read(), flags=re.S)
    assert "#define MMSBM_HIP_ABI_VERSION 1" in text
    for name, n_args in NEW_SYMBOLS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert decl, f"{name} is not declared in the header"
        assert len(decl.group(1).split(",")) == n_args
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n_args
        assert callable(getattr(HipEM, name[len("mmsbm_hip_"):]))
    src = open(os.path.join(ROOT, "mmsbm_amd", "core.py")).read()
    for name in NEW_SYMBOLS:
        assert f'"{name}"' in src, f"HipEM never calls {name}"
