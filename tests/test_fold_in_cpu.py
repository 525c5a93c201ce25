"""MMSBM.fold_in() / recommend_new() without a GPU: a numpy restatement of the fold-in update, pinned to the oracle's
M-step, and the host class's side -- labels, dropped rows, restart order, argument checks, the refusal of a
distributed share -- through a CPU stand-in that answers fold_in / recommend_query_theta with the restatements.

The restatement is what the GPU tests (test_gpu_fold_in.py) compare the device against:
    v_j[k]      = sum_l p[k, l, r_j] eta[i_j, l]
    theta'_u[k] = (1/d_u) sum_{j in u} theta_u[k] v_j[k] / max(theta_u . v_j, eps)
"""
import logging

import numpy as np
import pandas as pd
import pytest

import fake_device
from oracle import mmsbm_oracle as orc
from test_recommend_cpu import RecommendFakeHipEM, restate, same, string_frame


# ---- the restatement ----------------------------------------------------------------------------------------------
def restate_v(rows, eta, pr):
    """(N, K): v_j = p[:, :, r_j] eta[i_j]"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    return np.einsum("klj,jl->jk", pr[:, :, rows[:, 2]], eta[rows[:, 1]]) if len(rows) else np.zeros((0, pr.shape[0]))


def restate_fold(rows, n_new, eta, pr, iterations, tol=None, theta0=None):
    """(theta (n_new, K), iterations used (n_new,)) -- what mmsbm_hip_fold_in returns."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    K = pr.shape[0]
    v = restate_v(rows, eta, pr)
    u = rows[:, 0]
    d = np.bincount(u, minlength=n_new).astype(np.float64)
    theta = np.full((n_new, K), 1.0 / K) if theta0 is None else np.array(theta0, dtype=np.float64)
    iters = np.zeros(n_new, dtype=np.int32)
    active = d > 0
    for _ in range(int(iterations)):
        if not active.any():
            break
        tu = theta[u]
        q = tu * v
        dot = np.maximum(q.sum(axis=1), orc.EPS)
        acc = np.zeros_like(theta)
        np.add.at(acc, u, q / dot[:, None])
        new = theta.copy()
        new[active] = acc[active] / d[active, None]
        delta = np.abs(new - theta).max(axis=1)
        theta = new
        iters[active] += 1
        if tol is not None and tol > 0:
            active &= ~(delta <= tol)
    return theta, iters


def log_likelihood(rows, n_new, theta, eta, pr):
    rows = np.asarray(rows, dtype=np.int64)
    v = restate_v(rows, eta, pr)
    per = np.log((theta[rows[:, 0]] * v).sum(axis=1))
    return np.bincount(rows[:, 0], weights=per, minlength=n_new)


def random_model(U, I, R, K, L, seed):
    rng = np.random.default_rng(seed)
    return rng.random((U, K)), rng.random((I, L)), orc.normalize_with_self(rng.random((K, L, R)))


def random_rows(n_new, I, R, n_rows, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, n_new, n_rows), rng.integers(0, I, n_rows), rng.integers(0, R, n_rows)], 1)


# ---- the restatement against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("K,L", [(1, 3), (4, 4), (7, 3), (3, 9)])
def test_one_iteration_is_the_oracle_theta_update(K, L):
    U, I, R = 30, 25, 4
    theta, eta, pr = random_model(U, I, R, K, L, seed=K * 10 + L)
    train = orc.synthetic_triples(600, U, I, R, seed=K)
    d_u, _ = orc.degrees(train, U, I)
    want = orc.normalize_with_d(orc.update_coefficients(train, theta, eta, pr)[0], d_u)
    got, iters = restate_fold(train, U, eta, pr, 1, theta0=theta)
    seen = d_u > 0
    np.testing.assert_allclose(got[seen], want[seen], rtol=1e-13, atol=0)
    assert (iters[seen] == 1).all()


def test_the_log_likelihood_never_decreases():
    theta, eta, pr = random_model(1, 40, 5, 6, 5, seed=3)
    rows = random_rows(20, 40, 5, 300, seed=4)
    th = np.random.default_rng(5).random((20, 6))
    th /= th.sum(axis=1, keepdims=True)                               # (a point of the simplex, where EM lives)
    last = log_likelihood(rows, 20, th, eta, pr)
    for _ in range(60):
        th, _ = restate_fold(rows, 20, eta, pr, 1, theta0=th)
        now = log_likelihood(rows, 20, th, eta, pr)
        assert (now >= last - 1e-12 * np.abs(last)).all()
        last = now


def test_uniform_and_random_starts_reach_the_same_theta():
    theta, eta, pr = random_model(1, 30, 3, 4, 3, seed=8)
    rows = random_rows(10, 30, 3, 400, seed=9)
    a, _ = restate_fold(rows, 10, eta, pr, 20000, tol=1e-15)
    t0 = np.random.default_rng(1).random((10, 4)) + 0.1
    t0 /= t0.sum(axis=1, keepdims=True)
    b, _ = restate_fold(rows, 10, eta, pr, 20000, tol=1e-15, theta0=t0)
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-8)


def test_tol_stops_each_user_on_its_own():
    _, eta, pr = random_model(1, 30, 3, 4, 3, seed=2)
    rows = random_rows(6, 30, 3, 120, seed=3)
    rows = rows[rows[:, 0] != 5]                                     # user 5 has no rows
    full, n_full = restate_fold(rows, 6, eta, pr, 500)
    th, it = restate_fold(rows, 6, eta, pr, 500, tol=1e-4)
    assert it[5] == 0 and n_full[5] == 0 and (th[5] == 0.25).all() and (n_full[:5] == 500).all()
    assert (it[:5] >= 1).all() and (it[:5] < 500).all() and len(set(it[:5].tolist())) > 1
    for u in range(5):                                                # a user stops where it alone says
        one, _ = restate_fold(rows, 6, eta, pr, int(it[u]))
        np.testing.assert_array_equal(th[u], one[u])


# ---- the host class through the stand-in -----------------------------------------------------------------------------
class FoldFakeHipEM(RecommendFakeHipEM):
    """The recommend stand-in with fold_in and recommend_query_theta, answered by the restatements."""

    def fold_in(self, rows, n_new, iterations, tol=None, theta0=None):
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        assert ((rows[:, 1] >= 0) & (rows[:, 1] < self.n_items)).all()
        assert ((rows[:, 2] >= 0) & (rows[:, 2] < self.n_ratings)).all()
        assert ((rows[:, 0] >= 0) & (rows[:, 0] < n_new)).all()
        _, eta, pr = self._params[self._sel]
        fake_device.LOG.append(("fold_in", self._sel))
        return restate_fold(rows, int(n_new), eta, pr, iterations, tol, theta0)

    def recommend_query_theta(self, theta, n, seen=None):
        fake_device.LOG.append(("recommend_query_theta", theta.shape[1]))
        params = [(t, e, p) for t, (_, e, p) in zip(theta, self._rc["params"])]
        assert len(params) == len(self._rc["params"]) == theta.shape[0]
        s = None
        if seen is not None:
            off, items = seen
            s = [set(items[off[b]:off[b + 1]].tolist()) for b in range(theta.shape[1])]
        return restate(params, np.arange(theta.shape[1]), self.n_items, self._rc["w"], n, s)


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", FoldFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(FoldFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def fitted(host, df, sampling=2):
    m = host.MMSBM(2, 3, iterations=3, sampling=sampling, seed=7)
    m.fit(df, silent=True)
    return m


def new_frame(model, seed=1):
    il = model.data_handler.item_labels()
    rng = np.random.default_rng(seed)
    users = ["new-b", "new-a", "u3", "new-b", "new-c", "new-a", "new-b", "u3"]
    return pd.DataFrame({"users": users, "items": [il[x] for x in rng.integers(0, len(il), len(users))],
                         "ratings": rng.integers(1, 6, len(users))})


def encoded(model, df):
    enc = model.data_handler
    labels = list(dict.fromkeys(str(x) for x in df["users"]))
    ids = enc.transform(df.assign(users=enc.user_labels()[0]))
    u = np.array([labels.index(str(x)) for x in df["users"]])
    return np.stack([u, ids[:, 1], ids[:, 2]], 1), labels


def test_labels_in_first_appearance_order_and_values(host):
    m = fitted(host, string_frame())
    df = new_frame(m)
    got = m.fold_in(df, iterations=7)
    rows, labels = encoded(m, df)
    assert len(got) == 2
    for t, res in zip(got, m.results):
        assert t.index.tolist() == ["new-b", "new-a", "u3", "new-c"] == labels
        assert t.shape == (4, 2)
        want, _ = restate_fold(rows, 4, res["eta"], res["pr"], 7)
        np.testing.assert_array_equal(t.to_numpy(), want)
    assert m.fold_in_iterations.shape == (4, 2) and (m.fold_in_iterations.to_numpy() == 7).all()
    assert m.fold_in_iterations.index.tolist() == labels


def test_training_theta_is_never_consulted(host):
    m = fitted(host, string_frame())
    df = new_frame(m)
    a = m.fold_in(df, iterations=5)
    for r in m.results:
        r["theta"] = r["theta"] * 0 + 123.0
    m._resident.clear()
    b = m.fold_in(df, iterations=5)
    for x, y in zip(a, b):
        pd.testing.assert_frame_equal(x, y)


def test_unseen_items_and_ratings_are_dropped_with_a_warning(host, caplog):
    m = fitted(host, string_frame())
    df = new_frame(m)
    extra = pd.DataFrame({"users": ["new-d", "new-a", "new-e"], "items": ["no-such-item", m.data_handler.item_labels()[0], "x"],
                          "ratings": [3, 99, 2]})
    with caplog.at_level(logging.WARNING, logger="MMSBM"):
        got = m.fold_in(pd.concat([df, extra], ignore_index=True), iterations=4)
    text = caplog.text
    assert "The items no-such-item, x are in the test set but weren't in the train set so I'll remove them." in text
    assert "The ratings 99 are in the test set but weren't in the train set so I'll remove them." in text
    assert got[0].index.tolist() == ["new-b", "new-a", "u3", "new-c", "new-d", "new-e"]
    assert (m.fold_in_iterations.loc[["new-d", "new-e"]].to_numpy() == 0).all()   # every row dropped: uniform, no step
    assert (got[0].loc["new-d"].to_numpy() == 0.5).all()
    same_users = m.fold_in(df, iterations=4)
    for a, b in zip(got, same_users):
        np.testing.assert_array_equal(a.iloc[:4].to_numpy(), b.to_numpy())


def test_restart_order_and_resident_slots(host):
    m = fitted(host, string_frame(), sampling=3)
    fake_device.LOG.clear()
    m.fold_in(new_frame(m), iterations=2)
    events = [(e, d) for e, d in fake_device.LOG if e in ("fold_in", "set_params", "set_slots")]
    assert events == [("fold_in", 0), ("fold_in", 1), ("fold_in", 2)]             # the fitted slots, no upload
    m.predict(string_frame().iloc[:20])
    m._resident.clear()
    fake_device.LOG.clear()
    m.recommend_new(new_frame(m), n=2, iterations=2)
    events = [e for e, _ in fake_device.LOG if e in ("fold_in", "set_params", "recommend_add", "recommend_begin",
                                                      "recommend_end", "recommend_query_theta")]
    assert events == ["recommend_begin"] + ["set_params", "fold_in", "recommend_add"] * 3 + [
        "recommend_query_theta", "recommend_end"]


def test_recommend_new_against_the_restatement(host):
    m = fitted(host, string_frame())
    df = new_frame(m)
    rows, labels = encoded(m, df)
    il = m.data_handler.item_labels()
    w = np.asarray(m.ratings, dtype=np.float64)
    for exclude in (True, False):
        got = m.recommend_new(df, n=3, exclude_seen=exclude, iterations=6)
        thetas = [restate_fold(rows, 4, r["eta"], r["pr"], 6)[0] for r in m.results]
        params = [(t, r["eta"], r["pr"]) for t, r in zip(thetas, m.results)]
        seen = [set(rows[rows[:, 0] == u, 1].tolist()) for u in range(4)] if exclude else None
        items, vals, counts = restate(params, np.arange(4), m.m + 1, w, 3, seen)
        want = pd.DataFrame([(labels[u], il[items[u, k]], vals[u, k], k + 1) for u in range(4) for k in range(counts[u])],
                            columns=["users", "items", "score", "rank"])
        same(got, want)
        if exclude:
            mine = set(zip(df["users"], df["items"]))
            assert not any((u, i) in mine for u, i in zip(got["users"], got["items"]))


def test_recommend_new_batches_users(host, monkeypatch):
    m = fitted(host, string_frame())
    want = m.recommend_new(new_frame(m), n=3)
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 7)        # two users per query call
    fake_device.LOG.clear()
    same(m.recommend_new(new_frame(m), n=3), want)
    assert [d for e, d in fake_device.LOG if e == "recommend_query_theta"] == [2, 2]


def test_after_fit_encoded_users_are_any_ids(host, caplog):
    df = string_frame()
    m = host.MMSBM(2, 3, iterations=3, sampling=2, seed=7)
    from mmsbm_amd.encode import Encoder
    m.fit_encoded(Encoder().fit_transform(df))
    data = np.array([[900, 1, 0], [5, 2, 1], [900, 3, 2], [77, m.m + 4, 0], [5, 0, len(m.ratings)]])
    with caplog.at_level(logging.WARNING, logger="MMSBM"):
        got = m.fold_in(data, iterations=3)
    assert got[0].index.tolist() == [900, 5, 77]
    assert f"The items {m.m + 4} are in the test set" in caplog.text
    assert f"The ratings {len(m.ratings)} are in the test set" in caplog.text
    rows = np.array([[0, 1, 0], [1, 2, 1], [0, 3, 2]])
    want, _ = restate_fold(rows, 3, m.results[1]["eta"], m.results[1]["pr"], 3)
    np.testing.assert_array_equal(got[1].to_numpy(), want)
    rec = m.recommend_new(data, n=2)
    assert rec["users"].tolist() == [900, 900, 5, 5, 77, 77] and rec["items"].dtype == np.int64


def test_bad_arguments_and_distributed_share(host):
    m = fitted(host, string_frame(), sampling=3)
    df = new_frame(m)
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError):
            m.fold_in(df, iterations=bad)
    for bad in (np.nan, "x", np.inf):
        with pytest.raises(ValueError):
            m.fold_in(df, tol=bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            m.recommend_new(df, n=bad)
    with pytest.raises(ValueError):
        m.recommend_new(df, weights=[1.0, 2.0])
    w = np.ones(len(m.ratings))
    w[0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        m.recommend_new(df, weights=w)
    m._restart_ids = m._restart_ids[:1]
    m.results = m.results[:1]
    for call in (lambda: m.fold_in(df), lambda: m.recommend_new(df)):
        with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
            call()


def test_unfitted_model_is_refused(host):
    m = host.MMSBM(2, 3)
    with pytest.raises(AssertionError):
        m.fold_in(pd.DataFrame({"users": [1], "items": [1], "ratings": [1]}))
