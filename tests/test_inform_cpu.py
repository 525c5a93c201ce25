"""MMSBM.informative_items() / ask_next() / interview() without a GPU: the properties of the numpy restatement of the
information gain (inform_reference.py; test_gpu_inform.py compares the device against it), the host class's side --
labels, request order, candidates and exclusions, the shrinkage of a folded theta, argument checks -- through a CPU
stand-in that answers the inform_* calls with the restatement, and the precondition of the GPU test: on its seeds and
shapes no two gains of a user lie within 4 tolerances of each other, so the device's ITEMS must be equal."""
import numpy as np
import pandas as pd
import pytest

import exact_models as xm
import fake_device
import inform_reference as ir
from test_fold_in_cpu import FoldFakeHipEM, encoded, new_frame, restate_fold
from test_recommend_cpu import fitted, string_frame
from test_similar_cpu import random_params

# (shape (U, I, K, L, R, S), seed) of test_gpu_inform.test_general_models_agree_with_the_restatement: partial 64 x 64
# tiles on both sides with K below the staging depth of 16, and K = 17, 33 crossing it once and twice
GENERAL = [((300, 997, 7, 9, 5, 3), 0), ((260, 1021, 9, 5, 4, 4), 1), ((130, 200, 17, 6, 4, 2), 2),
           ((131, 203, 33, 5, 3, 2), 3)]
SPLIT = ((3, 5000, 4, 6, 5, 2), 4)        # few users over many items: the items split across selecting waves and merged
NS = (1, 10, 257)


def general_case(shape, seed):
    """(data, params) of a general model: rows of random_params, 4 U random training triples."""
    U, I, K, L, R, S = shape
    rng = np.random.default_rng(seed)
    params = random_params(rng, U, I, K, L, R, S)
    data = np.stack([rng.integers(0, U, 4 * U), rng.integers(0, I, 4 * U), rng.integers(0, R, 4 * U)], 1)
    return data, params


# ---- the restatement's properties -------------------------------------------------------------------------------------
def direct_kl(params, thetas):
    """gain as sum_k theta_k KL(q_k || m), one pair at a time."""
    M, I = thetas[0].shape[0], params[0][1].shape[0]
    out = np.zeros((M, I))
    for (_, eta, p), th in zip(params, thetas):
        q = np.einsum("il,klr->ikr", eta, p)
        for u in range(M):
            for i in range(I):
                m = th[u] @ q[i]
                for k in range(len(th[u])):
                    pos = q[i, k] > 0
                    out[u, i] += th[u, k] * np.sum(q[i, k, pos] * np.log(q[i, k, pos] / m[pos]))
    return out / len(params)


def test_gain_is_the_weighted_divergence_from_the_mixture():
    U, I, K, L, R, S = 6, 9, 3, 4, 5, 2
    params = random_params(np.random.default_rng(0), U, I, K, L, R, S)
    got = ir.gains_of_users(params, np.arange(U))
    np.testing.assert_allclose(got, direct_kl(params, [t for t, _, _ in params]), rtol=0, atol=1e-13)
    assert got.min() > 0.0


@pytest.mark.parametrize("shape", [(8, 11, 2, 3, 5, 1), (8, 11, 6, 3, 3, 2), (5, 7, 4, 4, 1, 2)])
def test_gain_lies_between_zero_and_log_min_k_r(shape):
    U, I, K, L, R, S = shape
    rng = np.random.default_rng(1)
    params = random_params(rng, U, I, K, L, R, S)
    for _, _, p in params:                                   # far apart groups: near-deterministic ratings
        p[:] = 1e-9
        for k in range(K):
            p[k, :, k % R] = 1.0
        p /= p.sum(axis=2, keepdims=True)
    g = ir.gains_of_users(params, np.arange(U))
    tol = ir.tolerance(K, L, R, S)
    assert (g >= 0.0).all() and (g <= np.log(min(K, R)) + tol).all()
    if R == 1:
        assert (g <= tol).all()                              # one rating value carries no information
    else:
        uniform = [np.full((1, K), 1.0 / K)] * S
        assert ir.gains(params, uniform).max() > 0.9 * np.log(min(K, R))   # the bound is reached


def test_zero_for_one_hot_theta_and_for_items_every_group_rates_alike():
    U, I, K, L, R, S = 5, 8, 4, 3, 5, 2
    params = random_params(np.random.default_rng(2), U, I, K, L, R, S)
    one_hot = [np.eye(K)[[1, 3, 0, 1, 2]] for _ in range(S)]
    g = ir.gains(params, one_hot)
    assert (xm.bits(g) == 0).all()                           # exactly +0.0
    for _, _, p in params:
        p[:, 1, :] = p[0, 1, :]                              # item group 1: every user group rates it alike
    for _, eta, _ in params:
        eta[[2, 6]] = np.eye(L)[1]
    g = ir.gains_of_users(params, np.arange(U))
    assert (g[:, [2, 6]] <= ir.tolerance(K, L, R, S)).all() and g[:, [0, 1, 3]].min() > 1e-6


def test_invariance_under_a_relabelling_of_the_groups_of_one_restart():
    U, I, K, L, R, S = 7, 10, 4, 3, 4, 3
    params = random_params(np.random.default_rng(3), U, I, K, L, R, S)
    want = ir.gains_of_users(params, np.arange(U))
    pk, pl = np.array([2, 0, 3, 1]), np.array([1, 2, 0])
    theta, eta, p = params[1]
    moved = list(params)
    moved[1] = (theta[:, pk], eta[:, pl], p[pk][:, pl])
    np.testing.assert_allclose(ir.gains_of_users(moved, np.arange(U)), want, rtol=0, atol=ir.tolerance(K, L, R, S))
    np.testing.assert_allclose(ir.mean_theta(moved)[1], ir.mean_theta(params)[1][pk], rtol=0, atol=0)


def test_mean_theta_and_the_order():
    rng = np.random.default_rng(4)
    theta = rng.integers(0, 17, (700, 3)) / 16.0             # dyadic: every order of the sum gives the same bits
    assert np.array_equal(xm.bits(ir.mass_fixed_order(theta)), xm.bits(theta.sum(axis=0)))
    g = np.array([[0.5, 0.25, 0.5, 0.0, 0.25], [0.0, 0.0, 0.0, 0.0, 0.0]])
    items, vals, counts = ir.top_n(g, 4, ir.allowed_mask(2, 5, lists=(np.array([0, 1, 4]), np.array([2, 0, 1, 2]))))
    assert items.tolist() == [[0, 1, 4, 3], [3, 4, -1, -1]] and counts.tolist() == [4, 2]
    assert vals[0].tolist() == [0.5, 0.25, 0.25, 0.0] and np.isneginf(vals[1, 2:]).all()
    items, _, counts = ir.top_n(g, 2, ir.allowed_mask(2, 5, candidates=[1, 3]))
    assert items.tolist() == [[1, 3], [1, 3]] and counts.tolist() == [2, 2]


# ---- the precondition of the GPU test: decided orders ----------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", GENERAL + [SPLIT], ids=lambda v: "U{}I{}K{}L{}R{}S{}".format(*v) if isinstance(v, tuple) else f"seed{v}")
def test_the_gpu_tests_models_are_well_separated(shape, seed):
    U, I, K, L, R, S = shape
    _, params = general_case(shape, seed)
    g = np.sort(ir.gains_of_users(params, np.arange(U)), axis=1)
    gaps = np.diff(g, axis=1)                                # of EVERY pair of neighbours in a user's order, so also of
    tol = ir.tolerance(K, L, R, S)                           # the best n + 1 of any filtered candidate list
    print(f"{shape}: smallest gap {gaps.min():.3e}, tolerance {tol:.3e}")
    assert gaps.min() > 4.0 * tol
    mean = ir.mean_theta(params)[:, None, :]
    gi = np.sort(ir.gains(params, list(mean)), axis=1)
    assert np.diff(gi, axis=1).min() > 4.0 * tol


# ---- the CPU stand-in ---------------------------------------------------------------------------------------------------
class InformFakeHipEM(FoldFakeHipEM):
    """The fold-in stand-in with the inform session, answered by the restatement."""
    _inf = None

    def inform_begin(self):
        self._inf = []
        fake_device.LOG.append(("inform_begin", None))

    def inform_add(self):
        self._inf.append(self.get_params())
        fake_device.LOG.append(("inform_add", self._sel))

    def _answer(self, g, n, candidates, lists):
        assert self._inf, "query before inform_add"
        assert 1 <= n <= 1024
        return ir.top_n(g, n, ir.allowed_mask(g.shape[0], self.n_items, candidates, lists))

    def inform_query(self, users, n, candidates=None, exclude=None, exclude_seen=True):
        fake_device.LOG.append(("inform_query", len(users)))
        assert self._inf, "query before inform_add"
        assert 1 <= n <= 1024
        mask = ir.allowed_mask(len(users), self.n_items, candidates, exclude)
        if exclude_seen:
            mask &= ir.allowed_mask(len(users), self.n_items, lists=ir.train_lists(self.data, users))
        return ir.top_n(ir.gains_of_users(self._inf, users), n, mask)

    def inform_query_theta(self, theta, n, seen=None, candidates=None):
        theta = np.asarray(theta, dtype=np.float64)
        assert theta.shape[0] == len(self._inf) and theta.shape[2] == self.k
        fake_device.LOG.append(("inform_query_theta", theta.copy()))
        return self._answer(ir.gains(self._inf, list(theta)), n, candidates, seen)

    def inform_mean_theta(self):
        return ir.mean_theta(self._inf)

    def inform_end(self):
        self._inf = None
        fake_device.LOG.append(("inform_end", None))


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", InformFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(InformFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def model_params(m):
    return [(r["theta"], r["eta"], r["pr"]) for r in m.results]


def frame_of(answer, row_labels, item_labels):
    items, vals, counts = answer
    rows = [(row_labels[b], item_labels[items[b, k]], vals[b, k], k + 1) for b in range(len(row_labels))
            for k in range(counts[b])]
    return pd.DataFrame(rows, columns=["users", "items", "gain", "rank"])


def same(got, want, columns=("users", "items", "gain", "rank")):
    assert list(got.columns) == list(columns)
    for col in columns:
        if col != "gain":
            assert got[col].tolist() == want[col].tolist(), col
    assert np.array_equal(xm.bits(got["gain"].to_numpy(dtype=np.float64)), xm.bits(want["gain"].to_numpy(dtype=np.float64)))


def events(prefix="inform"):
    return [e for e, _ in fake_device.LOG if e.startswith(prefix)]


# ---- informative_items ---------------------------------------------------------------------------------------------------
def test_labels_request_order_and_exclude_seen(host):
    df = string_frame()
    m = fitted(host, df)
    m.predict(df.iloc[:40])
    before = m.score(silent=True)["stats"]
    enc = m.data_handler
    ul, il = enc.user_labels(), enc.item_labels()
    ask = ["u7", "u1", "u7", "u3"]
    ids = [ul.index(x) for x in ask]
    g = ir.gains_of_users(model_params(m), ids)
    for exclude_seen in (True, False):
        got = m.informative_items(users=ask, n=4, exclude_seen=exclude_seen)
        mask = ir.allowed_mask(4, len(il), lists=ir.train_lists(m.train, ids) if exclude_seen else None)
        same(got, frame_of(ir.top_n(g, 4, mask), ask, il))
        assert got["users"].tolist() == [u for u in ask for _ in range(4)] and got["rank"].tolist() == [1, 2, 3, 4] * 4
        seen = set(zip(df["users"], df["items"]))
        if exclude_seen:
            assert not any((u, i) in seen for u, i in zip(got["users"], got["items"]))
        assert (got["gain"] >= 0).all()
    every = m.informative_items(n=2)
    assert every["users"].tolist() == [u for u in ul for _ in range(2)]
    assert m.score(silent=True)["stats"] == before                      # the stored predictions are untouched
    assert events()[0] == "inform_begin" and events()[-1] == "inform_end"


def test_candidates_and_exclude(host):
    m = fitted(host, string_frame())
    enc = m.data_handler
    ul, il = enc.user_labels(), enc.item_labels()
    ask = ["u2", "u5"]
    ids = [ul.index(x) for x in ask]
    g = ir.gains_of_users(model_params(m), ids)
    full = m.informative_items(users=ask, n=len(il), exclude_seen=False)
    stock = ["item-3", "item-11", "item-3", "item-0", "item-17", "item-8"]
    got = m.informative_items(users=ask, n=3, exclude_seen=False, candidates=stock)
    cand = sorted({il.index(x) for x in stock})
    same(got, frame_of(ir.top_n(g, 3, ir.allowed_mask(2, len(il), candidates=cand)), ask, il))
    filtered = full[full["items"].isin(stock)].groupby("users", sort=False).head(3)
    assert got["items"].tolist() == filtered["items"].tolist()           # the full list, filtered
    best = full.groupby("users", sort=False).head(1)
    pairs = [(u, i) for u, i in zip(best["users"], best["items"])] + [("u5", "no-such-item"), ("u9", il[0])]
    got = m.informative_items(users=ask, n=len(il), exclude_seen=False, exclude=pairs)
    assert len(got) == len(full) - 2 and not set(zip(got["users"], got["items"])) & set(pairs)
    assert got["items"].tolist() == [i for u, i in zip(full["users"], full["items"]) if (u, i) not in pairs]
    empty = m.informative_items(users=ask, n=3, candidates=[])
    assert len(empty) == 0 and list(empty.columns) == ["users", "items", "gain", "rank"]


def test_rows_are_batched_and_every_restart_is_added(host, monkeypatch):
    m = fitted(host, string_frame(), sampling=3)
    want = m.informative_items(n=3)
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 7)           # two users per query call
    fake_device.LOG.clear()
    same(m.informative_items(n=3), want)
    queries = [d for e, d in fake_device.LOG if e == "inform_query"]
    assert len(queries) == -(-(m.p + 1) // 2) and max(queries) == 2
    assert events().count("inform_add") == 3 and events()[-1] == "inform_end"


def test_the_session_ends_when_a_query_fails(host, monkeypatch):
    m = fitted(host, string_frame())

    def broken(self, *a, **kw):
        raise RuntimeError("device lost")
    monkeypatch.setattr(InformFakeHipEM, "inform_query", broken)
    monkeypatch.setattr(InformFakeHipEM, "inform_query_theta", broken)
    for call in (lambda: m.informative_items(n=2), lambda: m.interview(n=2), lambda: m.ask_next(new_frame(m), n=2)):
        fake_device.LOG.clear()
        with pytest.raises(RuntimeError, match="device lost"):
            call()
        assert events()[-1] == "inform_end"


# ---- ask_next --------------------------------------------------------------------------------------------------------------
def shrunk(m, rows, n_new, prior, iterations):
    """(S, n_new, K): the issue's formula, one entry at a time."""
    params = model_params(m)
    mean = ir.mean_theta(params)
    d = np.bincount(rows[:, 0], minlength=n_new)
    out = []
    for s, (_, eta, p) in enumerate(params):
        fold = restate_fold(rows, n_new, eta, p, iterations)[0]
        used = np.empty_like(fold)
        for u in range(n_new):
            for k in range(fold.shape[1]):
                used[u, k] = (float(d[u]) * fold[u, k] + prior * mean[s, k]) / (float(d[u]) + prior)
        out.append(fold if prior == 0 else used)
    return np.stack(out)


@pytest.mark.parametrize("prior", [1.0, 0.0, 2.5])
def test_ask_next_shrinks_the_folded_theta_bit_for_bit(host, prior):
    m = fitted(host, string_frame())
    df = new_frame(m)
    rows, labels = encoded(m, df)
    il = m.data_handler.item_labels()
    fake_device.LOG.clear()
    got = m.ask_next(df, n=3, prior=prior, iterations=6)
    want_theta = shrunk(m, rows, len(labels), prior, 6)
    sent = [d for e, d in fake_device.LOG if e == "inform_query_theta"]
    assert len(sent) == 1 and np.array_equal(xm.bits(sent[0]), xm.bits(want_theta))
    if prior == 0:                                                        # the folded theta itself
        folds = np.stack([restate_fold(rows, len(labels), r["eta"], r["pr"], 6)[0] for r in m.results])
        assert np.array_equal(xm.bits(sent[0]), xm.bits(folds))
    seen = ir.train_lists(rows, np.arange(len(labels)))
    g = ir.gains(model_params(m), list(want_theta))
    same(got, frame_of(ir.top_n(g, 3, ir.allowed_mask(len(labels), len(il), lists=seen)), labels, il))
    mine = set(zip(df["users"], df["items"]))
    assert not any((u, i) in mine for u, i in zip(got["users"], got["items"]))   # what a user rated is not asked again
    assert got["users"].tolist() == [u for u in labels for _ in range(3)]
    assert m.fold_in_iterations.index.tolist() == labels and (m.fold_in_iterations.to_numpy() == 6).all()
    order = [e for e in events() + [e for e, _ in fake_device.LOG if e == "fold_in"]]
    assert order.count("inform_add") == 2 and order.count("fold_in") == 2


def test_ask_next_candidates_and_a_user_without_known_rows(host):
    m = fitted(host, string_frame())
    il = m.data_handler.item_labels()
    df = pd.concat([new_frame(m), pd.DataFrame({"users": ["new-z"], "items": ["no-such-item"], "ratings": [3]})],
                   ignore_index=True)
    stock = il[2:9]
    got = m.ask_next(df, n=2, candidates=stock, iterations=4)
    assert set(got["items"]) <= set(stock) and got["users"].tolist()[-2:] == ["new-z", "new-z"]
    first = m.interview(n=2, candidates=stock)                            # no known row: theta-bar, the interview's list
    z = got[got["users"] == "new-z"]
    assert z["items"].tolist() == first["items"].tolist()
    # (the restatement's own sums depend on how many rows it is asked at once; the device's do not)
    np.testing.assert_allclose(z["gain"].to_numpy(), first["gain"].to_numpy(), rtol=0, atol=ir.tolerance(2, 3, 5, 2))
    sent = [d for e, d in fake_device.LOG if e == "inform_query_theta"]
    assert np.array_equal(xm.bits(sent[0][:, -1]), xm.bits(sent[1][:, 0]))   # ... the same theta rows were asked
    assert len(m.ask_next(df, n=2, candidates=[])) == 0


# ---- interview -------------------------------------------------------------------------------------------------------------
def test_interview_is_the_query_of_the_mean_theta(host):
    m = fitted(host, string_frame(), sampling=3)
    il = m.data_handler.item_labels()
    params = model_params(m)
    g = ir.gains(params, list(ir.mean_theta(params)[:, None, :]))
    got = m.interview(n=5)
    want = frame_of(ir.top_n(g, 5), ["x"], il).drop(columns="users")
    same(got, want, ("items", "gain", "rank"))
    got = m.interview(n=len(il) + 4, candidates=il[::2])
    assert len(got) == len(il[::2]) and got["rank"].tolist() == list(range(1, len(got) + 1))
    assert events().count("inform_add") == 6 and events()[-1] == "inform_end"
    assert list(m.interview(candidates=[]).columns) == ["items", "gain", "rank"]


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments(host):
    m = fitted(host, string_frame())
    df = new_frame(m)
    with pytest.raises(KeyError, match="nobody"):
        m.informative_items(users=["u1", "nobody"])
    for call in (lambda c: m.informative_items(candidates=c), lambda c: m.ask_next(df, candidates=c),
                 lambda c: m.interview(candidates=c)):
        with pytest.raises(KeyError, match="no-such-item"):
            call(["item-1", "no-such-item"])
    for bad in (0, -3, 2.5, True):
        for call in (lambda n: m.informative_items(n=n), lambda n: m.ask_next(df, n=n), lambda n: m.interview(n=n)):
            with pytest.raises(ValueError, match="n must be a positive integer"):
                call(bad)
    for bad in (-1, -0.5, np.nan, np.inf, True, "x", None):
        with pytest.raises(ValueError, match="prior must be a finite number >= 0"):
            m.ask_next(df, prior=bad)
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError, match="iterations must be a non-negative integer"):
            m.ask_next(df, iterations=bad)
    for bad in (np.nan, "x", np.inf):
        with pytest.raises(ValueError, match="tol must be None or a finite number"):
            m.ask_next(df, tol=bad)
    with pytest.raises(ValueError, match="pairs"):
        m.informative_items(exclude=[("u1", "item-1", 3)])
    assert not events()                                                   # refused before any device call


def test_distributed_share_and_unfitted_model_are_refused(host):
    m = fitted(host, string_frame(), sampling=3)
    df = new_frame(m)
    m._restart_ids = m._restart_ids[:1]                                   # what fit_distributed(gather=False) leaves on a rank
    m.results = m.results[:1]
    for call in (lambda: m.informative_items(), lambda: m.ask_next(df), lambda: m.interview()):
        with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
            call()
    fresh = host.MMSBM(2, 3)
    for call in (lambda: fresh.informative_items(), lambda: fresh.ask_next(df), lambda: fresh.interview()):
        with pytest.raises(AssertionError):
            call()


def test_ids_after_fit_encoded(host):
    rng = np.random.default_rng(2)
    train = np.stack([rng.integers(0, 9, 80), rng.integers(0, 11, 80), rng.integers(0, 4, 80)], 1)
    train[:9, 0], train[:11, 1], train[:4, 2] = np.arange(9), np.arange(11), np.arange(4)
    m = host.MMSBM(2, 3, iterations=3, sampling=2, seed=7)
    m.fit_encoded(train)
    got = m.informative_items(users=[4, 0], n=3, exclude_seen=False)
    assert got["users"].tolist() == [4, 4, 4, 0, 0, 0] and got["items"].dtype == np.int64
    want = ir.top_n(ir.gains_of_users(model_params(m), [4, 0]), 3)
    assert got["items"].tolist() == want[0].ravel().tolist()
    assert np.array_equal(xm.bits(got["gain"].to_numpy()), xm.bits(want[1].ravel()))
    new = m.ask_next(np.array([[900, 1, 0], [5, 2, 1], [900, 3, 2]]), n=2)
    assert new["users"].tolist() == [900, 900, 5, 5]
    with pytest.raises(KeyError, match="9"):
        m.informative_items(users=[9])
