"""MMSBM.recommend_robust() and MMSBM.score_spread() without a GPU: the numpy restatement of the ensemble aggregates
(ensemble_reference.py) pinned on its properties, and the host class's side -- labels, request order, candidates,
``exclude``, the ``mean`` / ``std`` columns, refusals -- through a CPU stand-in that answers the two new calls with the
restatement; and the header, the ctypes table and the wrappers agree on the two new symbols."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import ensemble_reference as ens
import exact_models as xm
import fake_device
from conftest import ROOT
from mmsbm_amd.core import HipEM
from test_recommend_cpu import RecommendFakeHipEM, fitted, restate_scores, seen_items, string_frame

assert tuple(HipEM.ENSEMBLE_MODES) == ens.MODES               # the restatement's modes are the wrapper's, in its order


def stack(S, rows=7, items=40, seed=0, scale=3.0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(S, rows, items)) * scale + 2.5


def same_bits(a, b):
    return np.array_equal(xm.bits(a), xm.bits(b))


# ---- the restatement, pinned -----------------------------------------------------------------------------------------------
def test_hand_made_values():
    a = np.array([[[5.0, 4.5]], [[5.0, 4.5]], [[5.0, 4.5]], [[3.0, 4.5]]])
    sp = ens.spread(a)
    assert sp["worst"].tolist() == [[3.0, 4.5]] and sp["best"].tolist() == [[5.0, 4.5]]
    assert sp["mean"].tolist() == [[4.5, 4.5]]                                   # the same mean ...
    assert sp["std"][0, 1] == 0.0 and sp["std"][0, 0] == np.sqrt(0.75)           # ... a safe pair and a guess
    items, vals, counts = ens.top_n(a, [0], 2, "lcb", 1.0)
    assert items.tolist() == [[1, 0]] and counts.tolist() == [2] and vals[0, 0] == 4.5
    assert ens.top_n(a, [0], 2, "lcb", -1.0)[0].tolist() == [[0, 1]]             # exploring
    assert ens.top_n(a, [0], 2, "lcb", 0.0)[0].tolist() == [[0, 1]]              # the mean: a tie, by item id


def test_one_restart_is_the_identity():
    a = stack(1)
    sp = ens.spread(a)
    for key in ("worst", "best", "mean"):
        assert same_bits(sp[key], a[0])
    assert same_bits(sp["std"], np.zeros_like(a[0]))
    for mode in ens.MODES:
        for risk in (0.0, 1.0, -1.0, 0.5):
            assert same_bits(ens.aggregate(a, mode, risk), a[0])


@pytest.mark.parametrize("S", [2, 3, 8])
def test_identical_restarts_have_no_spread(S):
    a = np.repeat(stack(1, seed=S), S, axis=0)
    sp = ens.spread(a)
    assert same_bits(sp["std"], np.zeros_like(a[0]))                             # +0.0, not -0.0
    for key in ("worst", "best", "mean"):
        assert same_bits(sp[key], a[0])


@pytest.mark.parametrize("S", [2, 3, 4, 8])
def test_order_of_the_summaries_and_permutations(S):
    a = stack(S, seed=10 + S)
    sp = ens.spread(a)
    slack = 4 * ens.ulp(np.abs(a).max(axis=0))                                   # (the mean is rounded; worst / best are not)
    assert (sp["worst"] <= sp["mean"] + slack).all() and (sp["mean"] <= sp["best"] + slack).all()
    assert (sp["std"] >= 0).all() and (sp["std"] <= sp["best"] - sp["worst"]).all()
    perm = np.concatenate([[0], 1 + np.random.default_rng(S).permutation(S - 1)])
    other = ens.spread(a[perm])
    assert same_bits(other["worst"], sp["worst"]) and same_bits(other["best"], sp["best"])
    assert same_bits(ens.aggregate(a, "lcb", 0.0), sp["mean"])                   # risk = 0 gives the mean
    assert same_bits(ens.aggregate(a, "min"), a.min(axis=0)) and same_bits(ens.aggregate(a, "max"), a.max(axis=0))


@pytest.mark.parametrize("shape", [(40, 61, 7, 9, 5, 2), (40, 61, 9, 5, 4, 4)], ids=["S2", "S4"])
@pytest.mark.parametrize("kind", ["stars", "signed"])
def test_the_mean_of_exact_models_is_exact(shape, kind):
    """No rounding in a_s, D, Q or S Q - D D on these models, and D / S is exact for a power of two: the mean has the bits
    of the exact score, var is one division and std one square root."""
    U, I, K, L, R, S = shape
    params, w = xm.model("mixed", np.random.default_rng(5), U, I, K, L, R, S, kind)
    users = np.arange(U)
    a = np.stack([xm.exact_scores([p], users, I, w) for p in params])
    sp = ens.spread(a)
    assert same_bits(sp["mean"], xm.exact_scores(params, users, I, w))
    var = ((a - a.mean(axis=0)) ** 2).sum(axis=0) / S                             # (exact too: dyadic values)
    assert same_bits(sp["std"], np.sqrt(var))
    if kind == "signed":
        assert a.min() < 0 < a.max()


def test_top_n_follows_the_candidates_and_exclusions():
    a = stack(3, rows=5, items=30, seed=3)
    users = np.array([4, 0, 4])
    seen = [set(range(u, 30, 5)) for u in range(5)]
    extra = [[1, 2], [], [29]]
    cand = np.arange(0, 30, 2)
    for mode in ens.MODES:
        items, vals, counts = ens.top_n(a, users, 4, mode, 0.5, cand, seen, extra)
        agg = ens.aggregate(a, mode, 0.5)
        for b, u in enumerate(users):
            keep = [i for i in cand if i not in seen[u] and i not in extra[b]]
            best, v = cat._row(agg[u], keep, 4)
            assert items[b, :counts[b]].tolist() == best.tolist() and same_bits(vals[b, :counts[b]], v)


# ---- the CPU stand-in ------------------------------------------------------------------------------------------------------
class EnsembleFakeHipEM(RecommendFakeHipEM):
    """RecommendFakeHipEM with the two ensemble calls, answered by the restatement over each added slot's own scores."""

    def _stack(self):
        assert self._rc["params"], "an ensemble query before recommend_add"
        users = np.arange(self.n_users)
        return np.stack([restate_scores([p], users, self.n_items, self._rc["w"]) for p in self._rc["params"]])

    def recommend_query_ensemble(self, users, n, mode, risk=0.0, candidates=None, exclude=None):
        assert 1 <= n <= 1024 and mode in ens.MODES and np.isfinite(risk)
        u = np.asarray(users)
        assert u.dtype == np.int32
        if candidates is not None:
            c = np.asarray(candidates)
            assert c.dtype == np.int32 and (np.diff(c) > 0).all()
        extra = None
        if exclude is not None:
            off, it = exclude
            assert off[0] == 0 and len(off) == len(u) + 1 and off[-1] == len(it)
            extra = [it[off[b]:off[b + 1]] for b in range(len(u))]
        fake_device.LOG.append(("recommend_query_ensemble", len(u), mode, float(risk)))
        return ens.top_n(self._stack(), u, n, mode, risk, candidates, self._rc["seen"], extra)

    def recommend_pair_spread(self, users, items, per_slot=False):
        u, i = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
        assert u.shape == i.shape
        fake_device.LOG.append(("recommend_pair_spread", len(u)))
        each = self._stack()[:, u, i]
        sp = ens.spread(each)
        stats = np.stack([sp["mean"], sp["std"], sp["worst"], sp["best"]], axis=1).reshape(len(u), 4)
        return (stats, each) if per_slot else stats


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", EnsembleFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(EnsembleFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


COLUMNS = ["users", "items", "score", "mean", "std", "rank"]
NAMES = {"lcb": "lcb", "worst": "min", "best": "max"}


def model_stack(model, weights=None):
    w = np.asarray(model.ratings if weights is None else weights, dtype=np.float64)
    users = np.arange(model.p + 1)
    return np.stack([restate_scores([(r["theta"], r["eta"], r["pr"])], users, model.m + 1, w) for r in model.results])


def expected(model, users, n, mode, risk=0.0, exclude_seen=True, candidates=None, exclude=None, weights=None):
    """The restatement in the host class's output format; users / candidates / exclude as labels."""
    ul, il = model.data_handler.user_labels(), model.data_handler.item_labels()
    a = model_stack(model, weights)
    ids = [ul.index(u) for u in users]
    seen = seen_items(model.train, model.p + 1) if exclude_seen else None
    cand = None if candidates is None else [il.index(i) for i in candidates]
    extra = None if exclude is None else [[il.index(i) for u2, i in exclude if u2 == u and i in il] for u in users]
    items, vals, counts = ens.top_n(a, ids, n, mode, risk, cand, seen, extra)
    sp = ens.spread(a)
    rows = [(ul[u], il[items[b, k]], vals[b, k], sp["mean"][u, items[b, k]], sp["std"][u, items[b, k]], k + 1)
            for b, u in enumerate(ids) for k in range(counts[b])]
    return pd.DataFrame(rows, columns=COLUMNS)


def same(got, want):
    assert list(got.columns) == list(want.columns)
    for c in got.columns:
        if got[c].dtype == np.float64:
            assert same_bits(got[c].to_numpy(), want[c].to_numpy(dtype=np.float64)), c
        else:
            assert got[c].tolist() == want[c].tolist(), c


@pytest.mark.parametrize("aggregate", list(NAMES))
def test_labels_request_order_and_the_spread_columns(host, aggregate):
    m = fitted(host, string_frame(), sampling=3)
    users = ["u7", "u1", "u7", "u3"]                                             # request order, a user asked twice
    want = expected(m, users, 4, NAMES[aggregate], 1.0 if aggregate == "lcb" else 0.0)
    assert want["users"].unique().tolist() == ["u7", "u1", "u3"] and want["rank"].max() == 4
    same(m.recommend_robust(users, n=4, aggregate=aggregate), want)
    assert (want["std"] > 0).any()
    kinds = [e[0] for e in fake_device.LOG]
    assert kinds.count("recommend_add") == 3 and kinds[-1] == "recommend_end"
    assert kinds.count("recommend_query_ensemble") == 1 and kinds.count("recommend_pair_spread") == 1   # one per batch
    everyone = m.recommend_robust(n=2, aggregate=aggregate)
    assert everyone["users"].unique().tolist() == m.data_handler.user_labels()


def test_risk_candidates_exclude_and_weights_reach_the_session(host):
    m = fitted(host, string_frame(), sampling=3)
    il = m.data_handler.item_labels()
    stock = [il[j] for j in (3, 17, 4, 9, 3, 0, 11)]                             # a duplicate counts once
    shown = [("u1", il[3]), ("u1", il[9]), ("u9", il[4]), ("nobody", il[0]), ("u2", "no-such-item")]
    w = [0.0, 0.0, 0.0, 1.0, 1.0]
    for risk in (0.5, 0.0, -1.0):
        same(m.recommend_robust(["u1", "u2"], n=3, risk=risk, candidates=stock, exclude=shown, exclude_seen=False, weights=w),
             expected(m, ["u1", "u2"], 3, "lcb", risk, False, set(stock), shown, w))
    assert [e[2:] for e in fake_device.LOG if e[0] == "recommend_query_ensemble"] == [("lcb", 0.5), ("lcb", 0.0), ("lcb", -1.0)]
    assert ("recommend_begin", False) in fake_device.LOG
    got = m.recommend_robust(["u1"], n=3, exclude=pd.DataFrame(shown, columns=["users", "items"]), aggregate="worst")
    same(got, expected(m, ["u1"], 3, "min", 0.0, True, None, shown))
    assert len(m.recommend_robust(["u1"], candidates=[])) == 0
    assert list(m.recommend_robust(["u1"], candidates=[]).columns) == COLUMNS


def test_users_are_batched(host, monkeypatch):
    m = fitted(host, string_frame(), sampling=2)
    whole = m.recommend_robust(n=3)
    monkeypatch.setattr(type(m), "RECOMMEND_BATCH_ROWS", 9)                      # three users per call
    fake_device.LOG.clear()
    same(m.recommend_robust(n=3), whole)
    calls = [e[1] for e in fake_device.LOG if e[0] == "recommend_query_ensemble"]
    assert calls == [3] * (len(calls) - 1) + [calls[-1]] and sum(calls) == m.p + 1
    assert [e[0] for e in fake_device.LOG].count("recommend_pair_spread") == len(calls)


def test_bad_arguments(host):
    m = fitted(host, string_frame(), sampling=2)
    with pytest.raises(ValueError, match="aggregate"):
        m.recommend_robust(aggregate="median")
    for aggregate in ("worst", "best"):
        with pytest.raises(ValueError, match="risk belongs"):
            m.recommend_robust(aggregate=aggregate, risk=0.5)
    for bad in (np.nan, np.inf, "1", None, True):
        with pytest.raises(ValueError, match="risk"):
            m.recommend_robust(risk=bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n must be"):
            m.recommend_robust(n=bad)
    with pytest.raises(KeyError, match="stranger"):
        m.recommend_robust(["u1", "stranger"])
    with pytest.raises(KeyError, match="no-such-item"):
        m.recommend_robust(["u1"], candidates=["no-such-item"])
    with pytest.raises(ValueError, match="weights"):
        m.recommend_robust(weights=[1.0, 2.0])
    assert not [e for e in fake_device.LOG if e[0] in ("recommend_query_ensemble", "recommend_pair_spread")]
    assert [e[0] for e in fake_device.LOG].count("recommend_begin") == [e[0] for e in fake_device.LOG].count("recommend_end")


def test_score_spread(host):
    m = fitted(host, string_frame(), sampling=3)
    ul, il = m.data_handler.user_labels(), m.data_handler.item_labels()
    pairs = [("u7", il[3]), ("u1", il[0]), ("u7", il[3]), ("u3", il[19])]
    a = model_stack(m)
    each = np.stack([a[:, ul.index(u), il.index(i)] for u, i in pairs], axis=1)
    sp = ens.spread(each)
    want = pd.DataFrame({"users": [u for u, _ in pairs], "items": [i for _, i in pairs], "mean": sp["mean"],
                         "std": sp["std"], "worst": sp["worst"], "best": sp["best"]})
    same(m.score_spread(pairs), want)
    for s in range(3):
        want[f"restart_{s}"] = each[s]
    same(m.score_spread(pd.DataFrame(pairs, columns=["users", "items"]).assign(note="x"), per_restart=True), want)
    robust = m.recommend_robust(["u7", "u3"], n=3)                               # a recommend-style frame goes in as it is
    spread = m.score_spread(robust)
    assert same_bits(spread["mean"].to_numpy(), robust["mean"].to_numpy()) and same_bits(spread["std"].to_numpy(), robust["std"].to_numpy())
    assert same_bits((spread["mean"] - 1.0 * spread["std"]).to_numpy(), robust["score"].to_numpy())
    empty = m.score_spread([], per_restart=True)
    assert len(empty) == 0 and list(empty.columns) == list(want.columns)
    with pytest.raises(KeyError, match="stranger"):
        m.score_spread([("stranger", il[0])])
    with pytest.raises(KeyError, match="no-such-item"):
        m.score_spread([("u1", "no-such-item")])
    with pytest.raises(ValueError, match="pairs"):
        m.score_spread([("u1", il[0], 3)])


def test_the_session_is_ended_on_error(host, monkeypatch):
    m = fitted(host, string_frame(), sampling=2)

    def broken(self, *a, **k):
        raise RuntimeError("device lost")
    monkeypatch.setattr(EnsembleFakeHipEM, "recommend_pair_spread", broken)
    for call in (lambda: m.recommend_robust(["u1"]), lambda: m.score_spread([("u1", m.data_handler.item_labels()[0])])):
        fake_device.LOG.clear()
        with pytest.raises(RuntimeError, match="device lost"):
            call()
        assert fake_device.LOG[-1][0] == "recommend_end"


def test_distributed_share_is_refused(host):
    m = fitted(host, string_frame(), sampling=2)
    m._restart_ids = [0]
    with pytest.raises(RuntimeError, match="gather=True"):
        m.recommend_robust()
    with pytest.raises(RuntimeError, match="gather=True"):
        m.score_spread([])


# ---- header, signatures and wrappers agree -------------------------------------------------------------------------------
NEW_SYMBOLS = {"mmsbm_hip_recommend_query_ensemble": 13, "mmsbm_hip_recommend_pair_spread": 6}


def test_header_signatures_and_wrappers_agree():
    from mmsbm_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmsbm_hip.h")).read(), flags=re.S)
    assert "#define MMSBM_HIP_ABI_VERSION 1" in text
    for name, n_args in NEW_SYMBOLS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert decl, f"{name} is not declared in the header"
        assert len(decl.group(1).split(",")) == n_args
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n_args
        assert callable(getattr(HipEM, name[len("mmsbm_hip_"):]))
    for mode, value in HipEM.ENSEMBLE_MODES.items():
        assert re.search(rf"#define MMSBM_HIP_ENSEMBLE_{mode.upper()} {value}\b", text), mode
    src = open(os.path.join(ROOT, "mmsbm_amd", "core.py")).read()
    for name in NEW_SYMBOLS:
        assert f'"{name}"' in src, f"HipEM never calls {name}"
    from mmsbm_amd.serving import Serving
    assert set(Serving._ROBUST_AGGREGATES.values()) == set(HipEM.ENSEMBLE_MODES)
