"""MMSBM.explain without a GPU: the restatement (tests/explain_reference.py) against the identity it stands for, and the
host class's orchestration -- labels, request order, ranks, shares, batches, every restart added, the session ended
however the call ends -- through a stand-in device answered by the restatement.  The device itself is checked in
test_gpu_explain.py."""
import numpy as np
import pandas as pd
import pytest

import explain_reference as xr
import fake_device
from test_fold_in_cpu import random_model, restate_fold
from test_recommend_cpu import RecommendFakeHipEM, string_frame

COLUMNS = ["users", "items", "because", "rating", "contribution", "share", "rank", "score", "explained"]


# ---- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,L,S", [(1, 4, 1), (3, 5, 2), (5, 3, 1), (6, 6, 3)])
def test_the_contributions_sum_to_the_score_under_one_more_theta_update(K, L, S):
    """sum_j a(u, t, j) = sum_k theta'_u[k] g_t[k], theta' from the fold-in restatement at one iteration from theta0 =
    theta_u on u's own rows, per slot; g from matrix products.  Both sides are sums of about S K d_u products of
    magnitude <= max|w|: 1e-13 max|w| is far above their rounding and far below any mistake in the formula."""
    U, I, R = 9, 14, 4
    rng = np.random.default_rng(K * 100 + L * 10 + S)
    params = []
    for s in range(S):
        th, eta, pr = random_model(U, I, R, K, L, seed=K + 7 * L + 31 * s)
        params.append((th / th.sum(axis=1, keepdims=True), eta / eta.sum(axis=1, keepdims=True), pr))
    data = np.stack([rng.integers(0, U, 120), rng.integers(0, I, 120), rng.integers(0, R, 120)], 1)
    data = np.concatenate([data, data[:10]])                              # duplicate triples are separate rows
    w = np.array([-1.0, 0.5, 2.0, 4.0])
    ref = xr.Restatement(data, params, w)
    for u in range(U):
        rows = ref.rows(u)
        assert len(rows) == (data[:, 0] == u).sum() > 0
        own = np.column_stack([np.zeros(len(rows), dtype=np.int64), rows])
        for t in (0, 5, I - 1):
            r = ref.pair(u, t)
            want = score = 0.0
            for th, eta, pr in params:
                g = (pr @ w) @ eta[t]
                nxt, iters = restate_fold(own, 1, eta, pr, 1, theta0=th[u:u + 1])
                assert iters[0] == 1
                want += float(nxt[0] @ g) / S
                score += float(th[u] @ g) / S
            assert abs(r["explained"] - want) <= 1e-13 * np.abs(w).max()
            assert abs(r["score"] - score) <= 1e-13 * np.abs(w).max()
            assert abs(r["a"].sum() - r["explained"]) <= 1e-13 * np.abs(w).max() and r["degree"] == len(rows)
            nxt = ref.theta_next(u)
            assert all(abs(x.sum() - 1.0) < 1e-12 for x in nxt)            # the shares of a row sum to 1


def test_a_fixed_point_of_the_theta_update_explains_its_whole_score():
    U, I, R, K, L = 4, 10, 3, 3, 4
    _, eta, pr = random_model(U, I, R, K, L, seed=5)
    rng = np.random.default_rng(6)
    data = np.stack([rng.integers(0, U, 200), rng.integers(0, I, 200), rng.integers(0, R, 200)], 1)
    theta, _ = restate_fold(data, U, eta, pr, 20000, tol=1e-16)
    ref = xr.Restatement(data, [(theta, eta, pr)], np.arange(1.0, R + 1))
    for u in range(U):
        r = ref.pair(u, 3)
        assert abs(r["explained"] - r["score"]) <= 1e-9 and r["score"] > 0


def test_query_orders_ties_by_item_then_rating_and_pads():
    rows = np.array([[0, 3, 1], [0, 1, 2], [0, 3, 0], [0, 1, 2], [1, 2, 0]])
    theta, eta, pr = np.array([[1.0, 0.0], [0.0, 1.0]]), np.full((4, 2), 0.5), np.full((2, 2, 3), 1.0 / 3)
    ref = xr.Restatement(rows, [(theta, eta, pr)], np.array([1.0, 2.0, 3.0]))
    hi, hr, co, counts, explained, score, degree = ref.query([0, 1], [0, 1, 2], [2, 2], 5)
    assert hi[0].tolist() == [1, 1, 3, 3, -1] and hr[0].tolist() == [2, 2, 0, 1, -1]      # every row ties
    assert len(set(co[0, :4].tolist())) == 1 and np.isneginf(co[0, 4])
    assert counts.tolist() == [4, 1] and degree.tolist() == [4, 1]
    assert explained[0] == score[0] == 2.0                                 # uniform p: the expected rating is 2


# ---- the host class through the stand-in -----------------------------------------------------------------------------
class ExplainFakeHipEM(RecommendFakeHipEM):
    """The recommend stand-in with the explain session, answered by the restatement."""
    FAIL_AT = None                       # explain_query call (counted from 0) that raises, for the clean-up test

    def explain_begin(self, rating_weights):
        w = np.ascontiguousarray(rating_weights, dtype=np.float64)
        if w.shape != (self.n_ratings,):
            raise ValueError("rating_weights")
        self._ex = {"w": w, "params": [], "calls": 0}
        fake_device.LOG.append(("explain_begin", w.tolist()))

    def explain_add(self):
        self._ex["params"].append(self.get_params())
        fake_device.LOG.append(("explain_add", self._sel))

    def explain_query(self, users, offsets, items, n):
        assert self._ex["params"], "explain_query before explain_add"
        assert 1 <= n <= 1024 and len(offsets) == len(users) + 1 and offsets[0] == 0 and offsets[-1] == len(items)
        assert (np.diff(offsets) >= 0).all()
        fake_device.LOG.append(("explain_query", (len(users), len(items))))
        if self.FAIL_AT is not None and self._ex["calls"] == self.FAIL_AT:
            raise RuntimeError("the device said no")
        self._ex["calls"] += 1
        return xr.Restatement(self.data, self._ex["params"], self._ex["w"]).query(users, offsets, items, n)

    def explain_end(self):
        self._ex = None
        fake_device.LOG.append(("explain_end", None))


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", ExplainFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(ExplainFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    monkeypatch.setattr(ExplainFakeHipEM, "FAIL_AT", None)
    fake_device.LOG.clear()
    return host


def fitted(host, df, sampling=2):
    m = host.MMSBM(2, 3, iterations=3, sampling=sampling, seed=7)
    m.fit(df, silent=True)
    return m


def expected_frame(m, pairs, n, weights=None):
    """The restatement in the host class's output format, for encoded (user, item) pairs."""
    enc = m.data_handler
    params = [(r["theta"], r["eta"], r["pr"]) for r in m.results]
    w = np.asarray(m.ratings if weights is None else weights, dtype=np.float64)
    ref = xr.Restatement(m.train, params, w)
    ul, il, rl = enc.user_labels(), enc.item_labels(), enc.rating_labels()
    rows = []
    for u, t in pairs:
        r = ref.pair(u, t)
        for k, j in enumerate(xr.top_rows(r["items"], r["ratings"], r["a"], n).tolist()):
            rows.append((ul[u], il[t], il[r["items"][j]], rl[r["ratings"][j]], r["a"][j], r["a"][j] / r["explained"], k + 1,
                         r["score"], r["explained"]))
    return pd.DataFrame(rows, columns=COLUMNS)


def same(got, want):
    assert list(got.columns) == COLUMNS
    for col in ("users", "items", "because", "rating", "rank"):
        assert got[col].tolist() == want[col].tolist(), col
    for col in ("contribution", "share", "score", "explained"):
        np.testing.assert_array_equal(got[col].to_numpy(dtype=np.float64), want[col].to_numpy(dtype=np.float64), err_msg=col)


def test_columns_labels_request_order_ranks_and_share(host):
    df = string_frame()
    m = fitted(host, df)
    ul, il = m.data_handler.user_labels(), m.data_handler.item_labels()
    pairs = [(3, 7), (3, 1), (0, 7), (3, 7), (5, 0)]                        # a user twice in a row, and again later
    ask = [(ul[u], il[t]) for u, t in pairs]
    got = m.explain(ask, n=3)
    same(got, expected_frame(m, pairs, 3))
    assert list(dict.fromkeys(zip(got["users"], got["items"]))) == list(dict.fromkeys(ask))
    history = {u: set(zip(g["items"], g["ratings"].astype(str))) for u, g in df.groupby("users")}  # (labels: str(value))
    assert all((b, r) in history[u] for u, b, r in zip(got["users"], got["because"], got["rating"]))
    at = 0
    for u, t in pairs:
        d = int((m.train[:, 0] == u).sum())
        g = got.iloc[at:at + min(3, d)]
        at += len(g)
        assert g["users"].tolist() == [ul[u]] * len(g) and g["items"].tolist() == [il[t]] * len(g)
        assert g["rank"].tolist() == list(range(1, len(g) + 1))
        assert (np.diff(g["contribution"].to_numpy()) <= 0).all()
        assert g["score"].nunique() == 1 and g["explained"].nunique() == 1
        np.testing.assert_array_equal(g["share"].to_numpy(), g["contribution"].to_numpy() / g["explained"].to_numpy())
    assert at == len(got)
    whole = m.explain([ask[0]], n=1024)                                     # all rows: the shares sum to 1
    assert len(whole) == int((m.train[:, 0] == 3).sum()) and abs(whole["share"].sum() - 1.0) < 1e-12
    assert abs(whole["contribution"].sum() - whole["explained"].iloc[0]) < 1e-12
    frame = pd.DataFrame({"who": [a for a, _ in ask], "what": [b for _, b in ask], "note": range(len(ask))})
    same(m.explain(frame, n=3), got)                                         # a frame: the first two columns, by place
    w = np.eye(len(m.ratings))[1]
    same(m.explain(ask, n=2, weights=w), expected_frame(m, pairs, 2, weights=w))
    assert ("explain_begin", w.tolist()) in fake_device.LOG
    assert len(m.explain([], n=3)) == 0 and list(m.explain([], n=3).columns) == COLUMNS
    m.predict(df.iloc[:40])
    before = m.score(silent=True)["stats"]
    m.explain(ask)
    assert m.score(silent=True)["stats"] == before


def test_recommends_frame_is_accepted_as_it_is(host):
    m = fitted(host, string_frame())
    ul, il = m.data_handler.user_labels(), m.data_handler.item_labels()
    rec = m.recommend(users=[ul[4], ul[1]], n=3)
    got = m.explain(rec)                                                     # (columns users, items, score, rank)
    uid, iid = {x: j for j, x in enumerate(ul)}, {x: j for j, x in enumerate(il)}
    pairs = [(uid[u], iid[i]) for u, i in zip(rec["users"], rec["items"])]
    same(got, expected_frame(m, pairs, 5))
    first = got.groupby(["users", "items"], sort=False)["score"].first().to_numpy()
    np.testing.assert_allclose(first, rec["score"].to_numpy(), rtol=0, atol=1e-12 * max(m.ratings))


def test_every_restart_is_added_and_the_session_ends_on_error(host, monkeypatch):
    m = fitted(host, string_frame(), sampling=3)
    ul, il = m.data_handler.user_labels(), m.data_handler.item_labels()
    ask = [(ul[u], il[t]) for u in range(4) for t in (0, 2)]
    fake_device.LOG.clear()
    m.explain(ask, n=2)
    names = [e for e, _ in fake_device.LOG]
    assert names.count("explain_begin") == 1 and names.count("explain_add") == 3 and names[-1] == "explain_end"
    assert names.index("explain_query") > max(j for j, e in enumerate(names) if e == "explain_add")
    monkeypatch.setattr(ExplainFakeHipEM, "FAIL_AT", 0)
    fake_device.LOG.clear()
    with pytest.raises(RuntimeError, match="the device said no"):
        m.explain(ask, n=2)
    assert [e for e, _ in fake_device.LOG][-1] == "explain_end"


def test_fetching_is_batched(host, monkeypatch):
    m = fitted(host, string_frame())
    ul, il = m.data_handler.user_labels(), m.data_handler.item_labels()
    pairs = [(u, t) for u in (2, 2, 6, 1) for t in (0, 4, 9)]
    ask = [(ul[u], il[t]) for u, t in pairs]
    want = m.explain(ask, n=3)
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 15)              # 5 pairs per call at n = 3
    fake_device.LOG.clear()
    same(m.explain(ask, n=3), want)
    calls = [d for e, d in fake_device.LOG if e == "explain_query"]
    assert [q for _, q in calls] == [5, 5, 2]
    assert [b for b, _ in calls] == [1, 3, 1]              # runs of one user are one occurrence: 2 2 2 2 2 | 2 6 6 6 1 | 1 1
    assert sum(1 for e, _ in fake_device.LOG if e == "explain_end") == 1


def test_unknown_labels_and_bad_arguments(host):
    m = fitted(host, string_frame(), sampling=3)
    ul, il = m.data_handler.user_labels(), m.data_handler.item_labels()
    fake_device.LOG.clear()
    with pytest.raises(KeyError, match="users not in the training data.*nobody"):
        m.explain([(ul[0], il[0]), ("nobody", il[1])])
    with pytest.raises(KeyError, match="items not in the training data.*no-such-item"):
        m.explain(pd.DataFrame({"users": [ul[0]], "items": ["no-such-item"]}))
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            m.explain([(ul[0], il[0])], n=bad)
    for bad in ([1.0, 2.0], [1.0, np.nan, 1.0, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0, 1.0]):
        with pytest.raises(ValueError):
            m.explain([(ul[0], il[0])], weights=bad)
    with pytest.raises(ValueError):
        m.explain([(ul[0], il[0], 3)])
    with pytest.raises(ValueError):
        m.explain(pd.DataFrame({"users": [ul[0]]}))
    assert not [e for e, _ in fake_device.LOG if e.startswith("explain_")]         # refused before any device call
    m._restart_ids = m._restart_ids[:1]
    m.results = m.results[:1]
    with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
        m.explain([(ul[0], il[0])])
