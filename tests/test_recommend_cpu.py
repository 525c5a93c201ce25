"""MMSBM.recommend() without a GPU: the host class's side of top-N recommendation -- label mapping, request order,
batching, the argument checks and the refusal of a distributed share -- through a CPU stand-in that answers the
recommend_* calls with the numpy restatement below; and the restatement itself against a brute-force double loop.

The restatement is what the GPU tests (test_gpu_recommend.py) compare the device against:
    score(u, i) = mean over restarts of prod_dist(u, i) @ weights
(oracle.mmsbm_oracle.prod_dist per restart, src/kernels_numpy.py:86-96), candidates = every training item minus the
user's own training items when excluded, order = np.lexsort((item, -score)): score descending, ties by item id."""
import numpy as np
import pandas as pd
import pytest

import fake_device
from oracle import mmsbm_oracle as orc


# ---- the restatement ----------------------------------------------------------------------------------------------
def restate_scores(params, users, n_items, weights, chunk_pairs=200_000):
    """(len(users), n_items) scores: the mean over restarts of prod_dist, times the weights."""
    users = np.asarray(users, dtype=np.int64)
    out = np.empty((len(users), n_items), dtype=np.float64)
    per = max(1, chunk_pairs // max(n_items, 1))
    for b in range(0, len(users), per):
        uu = users[b:b + per]
        pairs = np.stack([np.repeat(uu, n_items), np.tile(np.arange(n_items), len(uu)), np.zeros(len(uu) * n_items, dtype=np.int64)], 1)
        dist = np.array([orc.prod_dist(pairs, t, e, p) for t, e, p in params]).mean(axis=0)
        out[b:b + len(uu)] = (dist @ np.asarray(weights, dtype=np.float64)).reshape(len(uu), n_items)
    return out


def seen_items(train, n_users):
    """Distinct training items of every user."""
    t = np.asarray(train)
    seen = [set() for _ in range(n_users)]
    for u, i in zip(t[:, 0].tolist(), t[:, 1].tolist()):
        seen[u].add(i)
    return seen


def restate(params, users, n_items, weights, n, seen=None, scores=None):
    """(items (M, n) padded with -1, scores (M, n) padded with -inf, counts (M,)) -- what recommend_query returns."""
    s = restate_scores(params, users, n_items, weights) if scores is None else scores
    items = np.full((len(users), n), -1, dtype=np.int32)
    vals = np.full((len(users), n), -np.inf)
    counts = np.zeros(len(users), dtype=np.int32)
    for b, u in enumerate(np.asarray(users).tolist()):
        cand = np.arange(n_items)
        if seen is not None:
            cand = cand[~np.isin(cand, np.fromiter(seen[u], dtype=np.int64, count=len(seen[u])))]
        order = cand[np.lexsort((cand, -s[b, cand]))][:n]
        counts[b] = len(order)
        items[b, :len(order)] = order
        vals[b, :len(order)] = s[b, order]
    return items, vals, counts


# ---- the CPU stand-in -----------------------------------------------------------------------------------------------
class RecommendFakeHipEM(fake_device.FakeHipEM):
    """FakeHipEM with the recommend session, answered by the restatement."""

    def recommend_begin(self, rating_weights, exclude_seen=True):
        w = np.ascontiguousarray(rating_weights, dtype=np.float64)
        if w.shape != (self.n_ratings,):
            raise ValueError("rating_weights")
        self._rc = {"w": w, "seen": seen_items(self.data, self.n_users) if exclude_seen else None, "params": []}
        fake_device.LOG.append(("recommend_begin", bool(exclude_seen)))

    def recommend_add(self):
        self._rc["params"].append(self.get_params())
        fake_device.LOG.append(("recommend_add", self._sel))

    def recommend_query(self, users, n):
        assert self._rc["params"], "recommend_query before recommend_add"
        assert 1 <= n <= 1024
        fake_device.LOG.append(("recommend_query", len(users)))
        return restate(self._rc["params"], users, self.n_items, self._rc["w"], n, self._rc["seen"])

    def recommend_end(self):
        self._rc = None
        fake_device.LOG.append(("recommend_end", None))


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", RecommendFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(RecommendFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def string_frame(n_obs=90, n_u=12, n_i=20, seed=3):
    rng = np.random.default_rng(seed)
    return pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                         "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                         "ratings": rng.integers(1, 6, n_obs)})


def fitted(host, df, sampling=2, **kw):
    m = host.MMSBM(2, 3, iterations=3, sampling=sampling, seed=7, **kw)
    m.fit(df, silent=True)
    return m


def expected_frame(model, users, n, exclude_seen=True, weights=None):
    """The restatement in the host class's output format, for encoded user ids `users`."""
    enc = model.data_handler
    params = [(r["theta"], r["eta"], r["pr"]) for r in model.results]
    w = np.asarray(model.ratings if weights is None else weights, dtype=np.float64)
    seen = seen_items(model.train, model.p + 1) if exclude_seen else None
    items, vals, counts = restate(params, users, model.m + 1, w, n, seen)
    ul, il = enc.user_labels(), enc.item_labels()
    rows = [(ul[u], il[items[b, k]], vals[b, k], k + 1) for b, u in enumerate(users) for k in range(counts[b])]
    return pd.DataFrame(rows, columns=["users", "items", "score", "rank"])


def same(got, want):
    assert list(got.columns) == ["users", "items", "score", "rank"]
    assert got["users"].tolist() == want["users"].tolist()
    assert got["items"].tolist() == want["items"].tolist()
    assert got["rank"].tolist() == want["rank"].tolist()
    np.testing.assert_array_equal(got["score"].to_numpy(dtype=np.float64), want["score"].to_numpy(dtype=np.float64))


# ---- the restatement against a brute-force double loop --------------------------------------------------------------
def test_restatement_matches_a_double_loop():
    rng = np.random.default_rng(0)
    U, I, R, K, L = 4, 6, 3, 2, 3
    params = [(rng.random((U, K)), rng.random((I, L)), orc.normalize_with_self(rng.random((K, L, R)))) for _ in range(2)]
    w = np.array([1.0, 2.5, -0.5])
    seen = [{0, 3}, set(), {0, 1, 2, 3, 4, 5}, {5}]
    items, vals, counts = restate(params, np.arange(U), I, w, 4, seen)
    for u in range(U):
        brute = []
        for i in range(I):
            if i in seen[u]:
                continue
            s = 0.0
            for t, e, p in params:
                s += sum(w[r] * sum(t[u, k] * e[i, l] * p[k, l, r] for k in range(K) for l in range(L)) for r in range(R))
            brute.append((-s / len(params), i))
        brute.sort()
        want = brute[:4]
        assert counts[u] == len(want)
        assert items[u, :counts[u]].tolist() == [i for _, i in want]
        np.testing.assert_allclose(vals[u, :counts[u]], [-s for s, _ in want], rtol=1e-13)
        assert (items[u, counts[u]:] == -1).all() and np.isneginf(vals[u, counts[u]:]).all()


def test_restatement_breaks_ties_by_item_id():
    rng = np.random.default_rng(1)
    eta = rng.random((5, 2))
    eta[3] = eta[1]                                   # items 1 and 3 score the same, bit for bit
    params = [(rng.random((1, 2)), eta, orc.normalize_with_self(rng.random((2, 2, 2))))]
    items, vals, _ = restate(params, [0], 5, [1.0, 2.0], 5)
    pos1, pos3 = items[0].tolist().index(1), items[0].tolist().index(3)
    assert pos3 == pos1 + 1 and vals[0, pos1] == vals[0, pos3]


# ---- the host class through the stand-in -----------------------------------------------------------------------------
def test_string_labels_after_fit_and_after_predict(host):
    df = string_frame()
    m = fitted(host, df)
    got = m.recommend(n=3)
    same(got, expected_frame(m, list(range(m.p + 1)), 3))
    assert set(got["users"]) <= set(df["users"]) and set(got["items"]) <= set(df["items"])
    train = set(zip(df["users"], df["items"]))
    assert not any((u, i) in train for u, i in zip(got["users"], got["items"]))   # no training pair comes back
    m.predict(df.iloc[:40])
    before = m.score(silent=True)["stats"]
    same(m.recommend(n=3), got)                       # after predict: the same
    assert m.score(silent=True)["stats"] == before    # and the stored predictions are untouched


def test_request_order_and_duplicate_users(host):
    df = string_frame()
    m = fitted(host, df)
    ask = ["u7", "u1", "u7", "u3"]
    got = m.recommend(users=ask, n=2)
    ids = [m.data_handler.user_labels().index(x) for x in ask]
    same(got, expected_frame(m, ids, 2))
    assert got["users"].tolist() == ["u7", "u7", "u1", "u1", "u7", "u7", "u3", "u3"]


def test_without_exclusion_and_with_one_hot_weights(host):
    df = string_frame()
    m = fitted(host, df)
    w = np.eye(len(m.ratings))[2]
    same(m.recommend(users=["u2"], n=4, exclude_seen=False, weights=w),
         expected_frame(m, [m.data_handler.user_labels().index("u2")], 4, exclude_seen=False, weights=w))


def test_user_with_every_item_seen_gets_no_rows(host):
    df = string_frame()
    items = sorted(set(df["items"]))
    full = pd.DataFrame({"users": ["all"] * len(items), "items": items, "ratings": [3] * len(items)})
    m = fitted(host, pd.concat([df, full], ignore_index=True))
    got = m.recommend(users=["all", "u1"], n=2)
    assert "all" not in set(got["users"]) and got["users"].tolist() == ["u1", "u1"]
    assert len(m.recommend(users=["all"], n=2)) == 0


def test_n_larger_than_the_catalogue(host):
    df = string_frame()
    m = fitted(host, df)
    n_items = m.m + 1
    got = m.recommend(users=["u0"], n=n_items + 5, exclude_seen=False)
    assert len(got) == n_items and got["rank"].tolist() == list(range(1, n_items + 1))
    same(got, expected_frame(m, [m.data_handler.user_labels().index("u0")], n_items + 5, exclude_seen=False))


def test_bad_arguments(host):
    m = fitted(host, string_frame())
    with pytest.raises(KeyError, match="nobody"):
        m.recommend(users=["u1", "nobody"])
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            m.recommend(n=bad)
    with pytest.raises(ValueError):
        m.recommend(weights=[1.0, 2.0])
    with pytest.raises(ValueError):
        m.recommend(weights=np.ones((len(m.ratings), 1)))
    for bad in (np.nan, np.inf):
        w = np.ones(len(m.ratings))
        w[1] = bad
        with pytest.raises(ValueError, match="finite"):
            m.recommend(weights=w)


def test_user_labels_are_the_encoders_whatever_the_request(host):
    rng = np.random.default_rng(5)
    df = pd.DataFrame({"users": rng.integers(0, 12, 90), "items": rng.integers(100, 120, 90), "ratings": rng.integers(1, 6, 90)})
    m = fitted(host, df)
    every = m.recommend(n=2)
    some = m.recommend(users=[7, "3"], n=2)           # an int and a str label of the same kind of id
    assert set(some["users"]) == {"7", "3"}
    joined = some.merge(every, on=["users", "rank"], suffixes=("", "_all"))
    assert len(joined) == len(some) and (joined["items"] == joined["items_all"]).all()


def test_distributed_share_is_refused(host):
    m = fitted(host, string_frame(), sampling=3)
    m._restart_ids = m._restart_ids[:1]               # what fit_distributed(gather=False) leaves on a rank
    m.results = m.results[:1]
    with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
        m.recommend()


def test_users_are_batched(host, monkeypatch):
    m = fitted(host, string_frame())
    want = m.recommend(n=3)
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 7)   # two users per query call
    fake_device.LOG.clear()
    same(m.recommend(n=3), want)
    queries = [d for e, d in fake_device.LOG if e == "recommend_query"]
    assert len(queries) == -(-(m.p + 1) // 2) and max(queries) == 2
    assert [e for e, _ in fake_device.LOG][-1] == "recommend_end"


def test_every_restart_is_added(host):
    m = fitted(host, string_frame(), sampling=3)
    fake_device.LOG.clear()
    m.recommend(n=1)
    assert sum(1 for e, _ in fake_device.LOG if e == "recommend_add") == 3
