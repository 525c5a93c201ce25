"""MMSBM.fold_in_items() / recommend_with_new_items() without a GPU: a numpy restatement of the item fold-in update,
pinned to the oracle's M-step and to the user fold-in on the transposed model, and the host class's side -- labels,
dropped rows, restart order, training-label collisions, the extended catalogue, argument checks, the refusal of a
distributed share -- through a CPU stand-in that answers fold_in_items / recommend_add_items with the restatements.

The restatement is what the GPU tests (test_gpu_fold_in_items.py) compare the device against:
    v_j[l]    = sum_k p[k, l, r_j] theta[u_j, k]
    eta'_i[l] = (1/d_i) sum_{j in i} eta_i[l] v_j[l] / max(eta_i . v_j, eps)
"""
import logging

import numpy as np
import pandas as pd
import pytest

import fake_device
from oracle import mmsbm_oracle as orc
from test_fold_in_cpu import FoldFakeHipEM, random_model, restate_fold
from test_recommend_cpu import restate, same, seen_items, string_frame


# ---- the restatement ----------------------------------------------------------------------------------------------
def restate_v_items(rows, theta, pr):
    """(N, L): v_j = theta[u_j] p[:, :, r_j]"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    return np.einsum("klj,jk->jl", pr[:, :, rows[:, 2]], theta[rows[:, 0]]) if len(rows) else np.zeros((0, pr.shape[1]))


def restate_fold_items(rows, n_new, theta, pr, iterations, tol=None, eta0=None):
    """(eta (n_new, L), iterations used (n_new,)) -- what mmsbm_hip_fold_in_items returns.  rows: [user, item, rating]."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    L = pr.shape[1]
    v = restate_v_items(rows, theta, pr)
    i = rows[:, 1]
    d = np.bincount(i, minlength=n_new).astype(np.float64)
    eta = np.full((n_new, L), 1.0 / L) if eta0 is None else np.array(eta0, dtype=np.float64)
    iters = np.zeros(n_new, dtype=np.int32)
    active = d > 0
    for _ in range(int(iterations)):
        if not active.any():
            break
        q = eta[i] * v
        dot = np.maximum(q.sum(axis=1), orc.EPS)
        acc = np.zeros_like(eta)
        np.add.at(acc, i, q / dot[:, None])
        new = eta.copy()
        new[active] = acc[active] / d[active, None]
        delta = np.abs(new - eta).max(axis=1)
        eta = new
        iters[active] += 1
        if tol is not None and tol > 0:
            active &= ~(delta <= tol)
    return eta, iters


def log_likelihood_items(rows, n_new, theta, eta, pr):
    rows = np.asarray(rows, dtype=np.int64)
    per = np.log((eta[rows[:, 1]] * restate_v_items(rows, theta, pr)).sum(axis=1))
    return np.bincount(rows[:, 1], weights=per, minlength=n_new)


def item_rows(n_new, U, R, n_rows, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, U, n_rows), rng.integers(0, n_new, n_rows), rng.integers(0, R, n_rows)], 1)


def restate_extended(params, new_etas, users, weights, n, seen=None):
    """recommend_query over I + n_new items: each slot's eta table extended by its folded new rows."""
    ext = [(t, np.vstack([e, ne]), p) for (t, e, p), ne in zip(params, new_etas)]
    n_items = ext[0][1].shape[0]
    return restate(ext, users, n_items, weights, n, seen)


# ---- the restatement against the oracle and the user side -----------------------------------------------------------
@pytest.mark.parametrize("K,L", [(1, 3), (4, 4), (7, 3), (3, 9), (5, 1)])
def test_one_iteration_is_the_oracle_eta_update(K, L):
    U, I, R = 30, 25, 4
    theta, eta, pr = random_model(U, I, R, K, L, seed=K * 10 + L)
    train = orc.synthetic_triples(600, U, I, R, seed=K)
    _, d_i = orc.degrees(train, U, I)
    want = orc.normalize_with_d(orc.update_coefficients(train, theta, eta, pr)[1], d_i)
    got, iters = restate_fold_items(train, I, theta, pr, 1, eta0=eta)
    seen = d_i > 0
    np.testing.assert_allclose(got[seen], want[seen], rtol=1e-12, atol=0)
    assert (iters[seen] == 1).all() and (iters[~seen] == 0).all()


@pytest.mark.parametrize("K,L,tol", [(3, 5, None), (6, 2, 1e-6), (4, 4, 1e-3)])
def test_the_restatement_is_user_fold_in_on_the_transposed_model(K, L, tol):
    theta, _, pr = random_model(40, 1, 4, K, L, seed=K + L)
    rows = item_rows(9, 40, 4, 250, seed=L)
    rows = rows[rows[:, 1] != 4]                                      # item 4 has no rows
    e0 = np.random.default_rng(3).random((9, L)) + 0.1
    for start in (None, e0):
        got, it = restate_fold_items(rows, 9, theta, pr, 80, tol=tol, eta0=start)
        want, wit = restate_fold(rows[:, [1, 0, 2]], 9, theta, pr.transpose(1, 0, 2), 80, tol=tol, theta0=start)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(it, wit)


def test_the_log_likelihood_never_decreases():
    theta, _, pr = random_model(40, 1, 5, 5, 6, seed=3)
    rows = item_rows(20, 40, 5, 300, seed=4)
    e = np.random.default_rng(5).random((20, 6))
    e /= e.sum(axis=1, keepdims=True)
    last = log_likelihood_items(rows, 20, theta, e, pr)
    for _ in range(60):
        e, _ = restate_fold_items(rows, 20, theta, pr, 1, eta0=e)
        now = log_likelihood_items(rows, 20, theta, e, pr)
        assert (now >= last - 1e-12 * np.abs(last)).all()
        last = now


# ---- the host class through the stand-in -----------------------------------------------------------------------------
class ItemsFakeHipEM(FoldFakeHipEM):
    """The fold-in stand-in with fold_in_items and the extended catalogue, answered by the restatements."""

    def fold_in_items(self, rows, n_new, iterations, tol=None, eta0=None):
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        assert ((rows[:, 0] >= 0) & (rows[:, 0] < self.n_users)).all()
        assert ((rows[:, 1] >= 0) & (rows[:, 1] < n_new)).all()
        assert ((rows[:, 2] >= 0) & (rows[:, 2] < self.n_ratings)).all()
        theta, _, pr = self._params[self._sel]
        fake_device.LOG.append(("fold_in_items", self._sel))
        return restate_fold_items(rows, int(n_new), theta, pr, iterations, tol, eta0)

    def recommend_add(self):
        assert "new" not in self._rc, "recommend_add after recommend_add_items"
        super().recommend_add()

    def recommend_add_items(self, eta, seen=None):
        assert self._rc["params"] and "new" not in self._rc
        assert eta.shape[0] == len(self._rc["params"])
        fake_device.LOG.append(("recommend_add_items", eta.shape[1]))
        self._rc["new"] = eta
        if seen is not None:
            off, users = seen
            base = self._rc["seen"] or [set() for _ in range(self.n_users)]
            for j in range(eta.shape[1]):
                for u in users[off[j]:off[j + 1]].tolist():
                    base[u].add(self.n_items + j)
            self._rc["seen"] = base

    def recommend_query(self, users, n):
        if "new" not in self._rc:
            return super().recommend_query(users, n)
        fake_device.LOG.append(("recommend_query", len(users)))
        return restate_extended(self._rc["params"], self._rc["new"], users, self._rc["w"], n, self._rc["seen"])


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", ItemsFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(ItemsFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def fitted(host, df, sampling=2):
    m = host.MMSBM(2, 3, iterations=3, sampling=sampling, seed=7)
    m.fit(df, silent=True)
    return m


def new_frame(model, seed=1):
    ul = model.data_handler.user_labels()
    rng = np.random.default_rng(seed)
    items = ["film-b", "film-a", "f3", "film-b", "film-c", "film-a", "film-b", "f3"]
    return pd.DataFrame({"users": [ul[x] for x in rng.integers(0, len(ul), len(items))], "items": items,
                         "ratings": rng.integers(1, 6, len(items))})


def encoded(model, df):
    enc = model.data_handler
    labels = list(dict.fromkeys(str(x) for x in df["items"]))
    ids = enc.transform(df.assign(items=enc.item_labels()[0]))
    i = np.array([labels.index(str(x)) for x in df["items"]])
    return np.stack([ids[:, 0], i, ids[:, 2]], 1), labels


def test_labels_in_first_appearance_order_and_values(host):
    m = fitted(host, string_frame())
    df = new_frame(m)
    got = m.fold_in_items(df, iterations=7)
    rows, labels = encoded(m, df)
    assert len(got) == 2
    for e, res in zip(got, m.results):
        assert e.index.tolist() == ["film-b", "film-a", "f3", "film-c"] == labels
        assert e.index.name == "items" and e.shape == (4, 3)
        want, _ = restate_fold_items(rows, 4, res["theta"], res["pr"], 7)
        np.testing.assert_array_equal(e.to_numpy(), want)
    assert m.fold_in_items_iterations.shape == (4, 2) and (m.fold_in_items_iterations.to_numpy() == 7).all()
    assert m.fold_in_items_iterations.index.tolist() == labels


def test_training_eta_is_never_consulted(host):
    m = fitted(host, string_frame())
    df = new_frame(m)
    a = m.fold_in_items(df, iterations=5)
    for r in m.results:
        r["eta"] = r["eta"] * 0 + 123.0
    m._resident.clear()
    b = m.fold_in_items(df, iterations=5)
    for x, y in zip(a, b):
        pd.testing.assert_frame_equal(x, y)


def test_unseen_users_and_ratings_are_dropped_with_a_warning(host, caplog):
    m = fitted(host, string_frame())
    df = new_frame(m)
    extra = pd.DataFrame({"users": ["no-such-user", m.data_handler.user_labels()[0], "x"],
                          "items": ["film-d", "film-a", "film-e"], "ratings": [3, 99, 2]})
    with caplog.at_level(logging.WARNING, logger="MMSBM"):
        got = m.fold_in_items(pd.concat([df, extra], ignore_index=True), iterations=4)
    text = caplog.text
    assert "The users no-such-user, x are in the test set but weren't in the train set so I'll remove them." in text
    assert "The ratings 99 are in the test set but weren't in the train set so I'll remove them." in text
    assert got[0].index.tolist() == ["film-b", "film-a", "f3", "film-c", "film-d", "film-e"]
    assert (m.fold_in_items_iterations.loc[["film-d", "film-e"]].to_numpy() == 0).all()
    assert (got[0].loc["film-d"].to_numpy() == 1.0 / 3).all()
    same_items = m.fold_in_items(df, iterations=4)
    for a, b in zip(got, same_items):
        np.testing.assert_array_equal(a.iloc[:4].to_numpy(), b.to_numpy())


def test_transform_users_encodes_users_and_ratings():
    from mmsbm_amd.encode import Encoder
    df = string_frame()
    enc = Encoder()
    train = enc.fit_transform(df)
    test = pd.DataFrame({"users": [df["users"][0], "nobody", df["users"][5]], "items": ["never", "seen", "here"],
                         "ratings": [df["ratings"][0], df["ratings"][1], 77]})
    ids, keep = enc.transform_users(test)
    assert keep.tolist() == [True, False, False]
    assert ids.tolist() == [[train[0, 0], train[0, 2]]]


def test_restart_order_and_resident_slots(host):
    m = fitted(host, string_frame(), sampling=3)
    fake_device.LOG.clear()
    m.fold_in_items(new_frame(m), iterations=2)
    events = [(e, d) for e, d in fake_device.LOG if e in ("fold_in_items", "set_params", "set_slots")]
    assert events == [("fold_in_items", 0), ("fold_in_items", 1), ("fold_in_items", 2)]   # fitted slots, no upload
    m.predict(string_frame().iloc[:20])
    m._resident.clear()
    fake_device.LOG.clear()
    m.recommend_with_new_items(new_frame(m), n=2, iterations=2)
    events = [e for e, _ in fake_device.LOG if e in ("fold_in_items", "set_params", "recommend_add", "recommend_begin",
                                                      "recommend_end", "recommend_query", "recommend_add_items")]
    assert events == ["recommend_begin"] + ["set_params", "fold_in_items", "recommend_add"] * 3 + [
        "recommend_add_items", "recommend_query", "recommend_end"]


def expected_extended(m, df, n, exclude, iterations, users=None):
    rows, labels = encoded(m, df)
    enc = m.data_handler
    w = np.asarray(m.ratings, dtype=np.float64)
    params = [(r["theta"], r["eta"], r["pr"]) for r in m.results]
    new = [restate_fold_items(rows, len(labels), r["theta"], r["pr"], iterations)[0] for r in m.results]
    I = m.m + 1
    ids = np.arange(m.p + 1) if users is None else np.array([enc.user_labels().index(u) for u in users])
    seen = None
    if exclude:
        seen = seen_items(m.train, m.p + 1)
        for u, j in zip(rows[:, 0].tolist(), rows[:, 1].tolist()):
            seen[u].add(I + j)
    items, vals, counts = restate_extended(params, new, ids, w, n, seen)
    il = enc.item_labels() + labels
    ul = enc.user_labels()
    return pd.DataFrame([(ul[u], il[items[b, k]], vals[b, k], k + 1) for b, u in enumerate(ids) for k in range(counts[b])],
                        columns=["users", "items", "score", "rank"])


def test_recommend_with_new_items_against_the_restatement(host):
    m = fitted(host, string_frame())
    df = new_frame(m)
    for exclude in (True, False):
        got = m.recommend_with_new_items(df, n=6, exclude_seen=exclude, iterations=6)
        same(got, expected_extended(m, df, 6, exclude, 6))
        assert set(got["items"]) & {"film-a", "film-b", "film-c", "f3"}
        if exclude:
            mine = set(zip(df["users"], df["items"]))
            assert not any((u, i) in mine for u, i in zip(got["users"], got["items"]))
    want = m.recommend(n=6)                                          # the plain recommend is untouched
    assert not set(want["items"]) & {"film-a", "film-b", "film-c", "f3"}
    ul = m.data_handler.user_labels()
    some = [ul[3], ul[0]]
    same(m.recommend_with_new_items(df, users=some, n=4, iterations=6), expected_extended(m, df, 4, True, 6, some))


def test_recommend_with_new_items_batches_users(host, monkeypatch):
    m = fitted(host, string_frame())
    want = m.recommend_with_new_items(new_frame(m), n=3)
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 7)        # two users per query call
    fake_device.LOG.clear()
    same(m.recommend_with_new_items(new_frame(m), n=3), want)
    calls = [d for e, d in fake_device.LOG if e == "recommend_query"]
    assert calls == [2] * ((m.p + 1) // 2) + ([1] if (m.p + 1) % 2 else [])


def test_training_labels_are_refused(host):
    m = fitted(host, string_frame())
    df = new_frame(m)
    clash = pd.concat([df, pd.DataFrame({"users": [df["users"][0]], "items": [m.data_handler.item_labels()[2]],
                                         "ratings": [3]})], ignore_index=True)
    with pytest.raises(ValueError, match="training items"):
        m.recommend_with_new_items(clash)
    m.fold_in_items(clash, iterations=2)                              # fold_in_items treats every item as new


def test_after_fit_encoded_items_are_any_ids(host, caplog):
    df = string_frame()
    m = host.MMSBM(2, 3, iterations=3, sampling=2, seed=7)
    from mmsbm_amd.encode import Encoder
    m.fit_encoded(Encoder().fit_transform(df))
    big = m.m + 1
    data = np.array([[1, big + 900, 0], [2, big + 5, 1], [3, big + 900, 2], [m.p + 4, big + 77, 0],
                     [0, big + 5, len(m.ratings)]])
    with caplog.at_level(logging.WARNING, logger="MMSBM"):
        got = m.fold_in_items(data, iterations=3)
    assert got[0].index.tolist() == [big + 900, big + 5, big + 77]
    assert f"The users {m.p + 4} are in the test set" in caplog.text
    assert f"The ratings {len(m.ratings)} are in the test set" in caplog.text
    rows = np.array([[1, 0, 0], [2, 1, 1], [3, 0, 2]])
    want, _ = restate_fold_items(rows, 3, m.results[1]["theta"], m.results[1]["pr"], 3)
    np.testing.assert_array_equal(got[1].to_numpy(), want)
    rec = m.recommend_with_new_items(data, n=2)
    assert rec["items"].dtype == np.int64 and len(rec) == 2 * (m.p + 1)
    with pytest.raises(ValueError, match="training items"):
        m.recommend_with_new_items(np.array([[1, m.m, 0]]))
    with pytest.raises(ValueError, match="item column"):
        m.fold_in_items(np.array([[1, -3, 0]]))


def test_bad_arguments_and_distributed_share(host):
    m = fitted(host, string_frame(), sampling=3)
    df = new_frame(m)
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError):
            m.fold_in_items(df, iterations=bad)
    for bad in (np.nan, "x", np.inf):
        with pytest.raises(ValueError):
            m.fold_in_items(df, tol=bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            m.recommend_with_new_items(df, n=bad)
    with pytest.raises(ValueError):
        m.recommend_with_new_items(df, weights=[1.0, 2.0])
    with pytest.raises(KeyError):
        m.recommend_with_new_items(df, users=["nobody"])
    m._restart_ids = m._restart_ids[:1]
    m.results = m.results[:1]
    for call in (lambda: m.fold_in_items(df), lambda: m.recommend_with_new_items(df)):
        with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
            call()


def test_unfitted_model_is_refused(host):
    m = host.MMSBM(2, 3)
    with pytest.raises(AssertionError):
        m.fold_in_items(pd.DataFrame({"users": [1], "items": [1], "ratings": [1]}))
