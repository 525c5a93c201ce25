"""MMSBM.similar_items() / similar_users() without a GPU: the numpy restatement of the distance the device computes
(test_gpu_similar.py compares the device against it), the restatement against a brute-force loop, the exact reference
on the models of exact_models.py, and the host class's side -- labels, request order, batching, argument checks --
through a CPU stand-in that answers the similar_* calls with the restatement.

    items:  q_s[i, k, r] = sum_l eta_s[i, l] p_s[k, l, r],    m_s[k] = sum_u theta_s[u, k]
            D(i, j) = ( sum_s sum_k sum_r m_s[k] (q_s[i,k,r] - q_s[j,k,r])^2 ) / (S U)
    users:  the same with theta and eta, k and l, U and I exchanged.
Order: D ascending, equal D by ascending id (np.lexsort((id, D))), the query row itself left out."""
import numpy as np
import pandas as pd
import pytest

import exact_models as xm
import fake_device
from test_recommend_cpu import fitted, string_frame

SIDES = ("items", "users")


# ---- the restatement ----------------------------------------------------------------------------------------------
def profiles(params, side):
    """Per restart (q (rows, G, R), m (G,)): the rating profiles of the side's rows and the other side's group masses."""
    out = []
    for theta, eta, p in params:
        if side == "items":
            out.append((np.einsum("il,klr->ikr", eta, p), theta.sum(axis=0)))
        else:
            out.append((np.einsum("uk,klr->ulr", theta, p), eta.sum(axis=0)))
    return out


def n_others(params, side):
    return params[0][0].shape[0] if side == "items" else params[0][1].shape[0]


def restate_distances(params, side, ids, chunk=64):
    """(len(ids), rows): D of every (query row, row) pair -- the numerator first, one division by S x the other side."""
    ids = np.asarray(ids, dtype=np.int64)
    prof = profiles(params, side)
    rows = prof[0][0].shape[0]
    num = np.zeros((len(ids), rows))
    for b in range(0, len(ids), chunk):
        for q, m in prof:
            for g in range(q.shape[1]):
                d = q[ids[b:b + chunk], None, g, :] - q[None, :, g, :]
                num[b:b + chunk] += m[g] * (d * d).sum(axis=2)
    return num / float(len(params) * n_others(params, side))


def top_similar(dist, ids, n):
    """(ids (M, n) padded with -1, distance (M, n) padded with +inf, counts (M,)) from distances (row b = ids[b])."""
    rows = dist.shape[1]
    out = np.full((len(ids), n), -1, dtype=np.int32)
    vals = np.full((len(ids), n), np.inf)
    counts = np.zeros(len(ids), dtype=np.int32)
    for b, i in enumerate(np.asarray(ids).tolist()):
        cand = np.delete(np.arange(rows), i)
        order = cand[np.lexsort((cand, dist[b, cand]))][:n]
        counts[b] = len(order)
        out[b, :len(order)] = order
        vals[b, :len(order)] = dist[b, order]
    return out, vals, counts


def restate_similar(params, side, ids, n):
    """What similar_query returns."""
    return top_similar(restate_distances(params, side, ids), ids, n)


def exact_distances(params, side, ids, order=None):
    """D on the models of exact_models.py, the numerator accumulated one profile entry f = (s, g, r) at a time in the
    order given (None: ascending, the device's): every operation is exact, so the order cannot matter."""
    ids = np.asarray(ids, dtype=np.int64)
    prof = profiles(params, side)
    terms = [(s, g, r) for s, (q, _) in enumerate(prof) for g in range(q.shape[1]) for r in range(q.shape[2])]
    num = np.zeros((len(ids), prof[0][0].shape[0]))
    for t in (range(len(terms)) if order is None else order):
        s, g, r = terms[t]
        q, m = prof[s]
        d = q[ids, g, r][:, None] - q[None, :, g, r]
        num += (m[g] * d) * d
    return (num + 0.0) / float(len(params) * n_others(params, side))


def random_params(rng, U, I, K, L, R, S):
    def rows(shape):
        a = rng.random(shape) + 0.01
        return a / a.sum(axis=-1, keepdims=True)
    return [(rows((U, K)), rows((I, L)), rows((K, L, R))) for _ in range(S)]


# ---- the restatement against a brute-force loop ------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
def test_restatement_matches_a_triple_loop(side):
    U, I, K, L, R, S = 5, 7, 2, 3, 3, 2
    params = random_params(np.random.default_rng(0), U, I, K, L, R, S)
    rows, others = (I, U) if side == "items" else (U, I)
    ids = [3, 0, rows - 1, 3]
    got_ids, got_d, counts = restate_similar(params, side, ids, 4)
    for b, i in enumerate(ids):
        brute = []
        for j in range(rows):
            if j == i:
                continue
            acc = 0.0
            for theta, eta, p in params:
                G, T = (K, L) if side == "items" else (L, K)
                for g in range(G):
                    m = sum(theta[u, g] for u in range(U)) if side == "items" else sum(eta[x, g] for x in range(I))
                    for r in range(R):
                        if side == "items":
                            qi = sum(eta[i, t] * p[g, t, r] for t in range(T))
                            qj = sum(eta[j, t] * p[g, t, r] for t in range(T))
                        else:
                            qi = sum(theta[i, t] * p[t, g, r] for t in range(T))
                            qj = sum(theta[j, t] * p[t, g, r] for t in range(T))
                        acc += m * (qi - qj) ** 2
            brute.append((acc / (S * others), j))
        brute.sort()
        assert counts[b] == 4
        assert got_ids[b].tolist() == [j for _, j in brute[:4]]
        np.testing.assert_allclose(got_d[b], [d for d, _ in brute[:4]], rtol=1e-12)
        assert 0.0 <= got_d[b].min() and got_d[b].max() <= 2.0
    assert np.array_equal(got_ids[0], got_ids[3]) and np.array_equal(xm.bits(got_d[0]), xm.bits(got_d[3]))
    few = restate_similar(params, side, [1], rows + 3)                 # n beyond the side: rows - 1 answers, padded
    assert few[2][0] == rows - 1 and (few[0][0, rows - 1:] == -1).all() and np.isposinf(few[1][0, rows - 1:]).all()
    assert 1 not in few[0][0].tolist()


def test_restatement_puts_identical_rows_next_to_each_other_at_distance_zero():
    rng = np.random.default_rng(1)
    params = random_params(rng, 6, 8, 3, 2, 4, 2)
    for _, eta, _ in params:
        eta[5] = eta[2]                                                  # items 2 and 5: the same rows in every restart
    ids, d, _ = restate_similar(params, "items", [2, 5, 0], 7)
    assert ids[0, 0] == 5 and d[0, 0] == 0.0 and not np.signbit(d[0, 0])
    assert ids[1, 0] == 2 and d[1, 0] == 0.0
    row = ids[2].tolist()                                                # seen from a third item: adjacent, equal, 2 first
    assert row.index(5) == row.index(2) + 1
    assert xm.bits(d[2, row.index(2)]) == xm.bits(d[2, row.index(5)])


# ---- the exact reference on models without rounding -------------------------------------------------------------------
def tie_expected(family, side):
    """Whole groups of rows at distance exactly 0 from each other: theta is one-hot in every block family, eta in
    those with item groups."""
    return family in (xm.BLOCK_FAMILIES if side == "users" else xm.TIE_FAMILIES)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("shape", xm.MANY, ids=lambda s: "U{}I{}K{}L{}R{}S{}".format(*s))
@pytest.mark.parametrize("family", xm.FAMILIES)
def test_exact_reference_does_not_depend_on_the_accumulation_order(family, shape, side):
    U, I, K, L, R, S = shape
    params = xm.make_case(family, "stars", shape)["params"]
    rows = I if side == "items" else U
    ids = np.arange(rows)
    want = exact_distances(params, side, ids)
    n_terms = S * (K if side == "items" else L) * R
    perm = np.random.default_rng(xm.case_seed(family, "stars", shape)).permutation(n_terms)
    assert np.array_equal(xm.bits(exact_distances(params, side, ids, perm)), xm.bits(want))
    assert np.array_equal(xm.bits(restate_distances(params, side, ids)), xm.bits(want))
    assert (np.diag(want) == 0.0).all() and (want >= 0.0).all() and (want <= 2.0).all()
    # the cases bite: mass ties at the n = 10 boundary, or all-distinct distances
    others = np.sort(np.where(np.eye(rows, dtype=bool), np.inf, want), axis=1)
    if tie_expected(family, side):
        assert (others[:, 9] == others[:, 10]).all()
        assert ((want == 0.0).sum(axis=1) - 1).min() >= 6                # (the 7 items of the "rare" level)
    elif side == "items":
        assert family in ("mixed", "ascending", "descending")
        distinct = [len(np.unique(want[i])) for i in range(rows)]        # (ascending: |i - j| = |i - j'| on both sides of i)
        assert max(distinct) == rows and min(distinct) >= rows // 2


# ---- the CPU stand-in ---------------------------------------------------------------------------------------------------
class SimilarFakeHipEM(fake_device.FakeHipEM):
    """FakeHipEM with the similarity session, answered by the restatement."""
    _sm = None

    def similar_begin(self, side):
        side = {0: "items", 1: "users"}.get(side, side)
        assert side in SIDES
        self._sm = {"side": side, "params": []}
        fake_device.LOG.append(("similar_begin", side))

    def similar_add(self):
        self._sm["params"].append(self.get_params())
        fake_device.LOG.append(("similar_add", self._sel))

    def similar_query(self, ids, n):
        assert self._sm["params"], "similar_query before similar_add"
        assert 1 <= n <= 1024
        fake_device.LOG.append(("similar_query", len(ids)))
        return restate_similar(self._sm["params"], self._sm["side"], ids, n)

    def similar_end(self):
        self._sm = None
        fake_device.LOG.append(("similar_end", None))


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", SimilarFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(SimilarFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def side_labels(model, side):
    enc = model.data_handler
    return enc.item_labels() if side == "items" else enc.user_labels()


def call(model, side, wanted=None, **kw):
    return model.similar_items(items=wanted, **kw) if side == "items" else model.similar_users(users=wanted, **kw)


def expected_frame(model, side, ids, n):
    """The restatement in the host class's output format, for encoded ids."""
    params = [(r["theta"], r["eta"], r["pr"]) for r in model.results]
    out, vals, counts = restate_similar(params, side, ids, n)
    lab = side_labels(model, side)
    rows = [(lab[i], lab[out[b, k]], vals[b, k], k + 1) for b, i in enumerate(ids) for k in range(counts[b])]
    return pd.DataFrame(rows, columns=[side, "similar", "distance", "rank"])


def same(got, want, side):
    assert list(got.columns) == [side, "similar", "distance", "rank"]
    for col in (side, "similar", "rank"):
        assert got[col].tolist() == want[col].tolist(), col
    assert np.array_equal(xm.bits(got["distance"].to_numpy(dtype=np.float64)), xm.bits(want["distance"].to_numpy(dtype=np.float64)))


def n_rows(model, side):
    return (model.m if side == "items" else model.p) + 1


# ---- the host class through the stand-in -----------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
def test_string_labels_and_none_means_every_row(host, side):
    df = string_frame()
    m = fitted(host, df)
    m.predict(df.iloc[:40])
    before = m.score(silent=True)["stats"]
    got = call(m, side, n=3)
    same(got, expected_frame(m, side, list(range(n_rows(m, side))), 3), side)
    assert set(got[side]) == set(df[side]) and set(got["similar"]) <= set(df[side])
    assert (got[side] != got["similar"]).all()                          # a row is never its own neighbour
    assert got["rank"].tolist() == [1, 2, 3] * n_rows(m, side)
    assert m.score(silent=True)["stats"] == before                      # the stored predictions are untouched
    assert [e for e, _ in fake_device.LOG if e.startswith("similar")][0] == "similar_begin"
    assert ("similar_begin", side) in fake_device.LOG


def test_request_order_and_duplicates(host):
    m = fitted(host, string_frame())
    ask = ["item-7", "item-1", "item-7", "item-3"]
    got = m.similar_items(items=ask, n=2)
    ids = [m.data_handler.item_labels().index(x) for x in ask]
    same(got, expected_frame(m, "items", ids, 2), "items")
    assert got["items"].tolist() == ["item-7", "item-7", "item-1", "item-1", "item-7", "item-7", "item-3", "item-3"]
    ask = ["u3", "u0", "u3"]
    got = m.similar_users(users=ask, n=4)
    same(got, expected_frame(m, "users", [m.data_handler.user_labels().index(x) for x in ask], 4), "users")


@pytest.mark.parametrize("side", SIDES)
def test_n_beyond_the_side_returns_every_other_row(host, side):
    m = fitted(host, string_frame())
    rows = n_rows(m, side)
    first = side_labels(m, side)[0]
    got = call(m, side, [first], n=rows + 5)
    assert len(got) == rows - 1 and got["rank"].tolist() == list(range(1, rows))
    same(got, expected_frame(m, side, [0], rows + 5), side)


def test_labels_are_the_encoders_whatever_the_request(host):
    rng = np.random.default_rng(5)
    df = pd.DataFrame({"users": rng.integers(0, 12, 90), "items": rng.integers(100, 120, 90), "ratings": rng.integers(1, 6, 90)})
    m = fitted(host, df)
    every = m.similar_items(n=2)
    some = m.similar_items(items=[107, "103"], n=2)                      # an int and a str label of the same kind of id
    assert set(some["items"]) == {"107", "103"}
    joined = some.merge(every, on=["items", "rank"], suffixes=("", "_all"))
    assert len(joined) == len(some) and (joined["similar"] == joined["similar_all"]).all()


def test_ids_after_fit_encoded(host):
    rng = np.random.default_rng(2)
    train = np.stack([rng.integers(0, 9, 80), rng.integers(0, 11, 80), rng.integers(0, 4, 80)], 1)
    train[:9, 0], train[:11, 1], train[:4, 2] = np.arange(9), np.arange(11), np.arange(4)
    m = host.MMSBM(2, 3, iterations=3, sampling=2, seed=7)
    m.fit_encoded(train)
    got = m.similar_items(items=[4, 0], n=3)
    assert got["items"].tolist() == [4, 4, 4, 0, 0, 0]
    params = [(r["theta"], r["eta"], r["pr"]) for r in m.results]
    want = restate_similar(params, "items", [4, 0], 3)
    assert got["similar"].tolist() == want[0].ravel().tolist()
    assert np.array_equal(xm.bits(got["distance"].to_numpy()), xm.bits(want[1].ravel()))
    with pytest.raises(KeyError, match="11"):
        m.similar_items(items=[11])


def test_bad_arguments(host):
    m = fitted(host, string_frame())
    with pytest.raises(KeyError, match="no-such-item"):
        m.similar_items(items=["item-1", "no-such-item"])
    with pytest.raises(KeyError, match="nobody"):
        m.similar_users(users=["nobody"])
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            m.similar_items(n=bad)
        with pytest.raises(ValueError):
            m.similar_users(n=bad)
    assert not [e for e, _ in fake_device.LOG if e.startswith("similar")]   # refused before any device call


def test_distributed_share_is_refused(host):
    m = fitted(host, string_frame(), sampling=3)
    m._restart_ids = m._restart_ids[:1]                                  # what fit_distributed(gather=False) leaves on a rank
    m.results = m.results[:1]
    for side in SIDES:
        with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
            call(m, side)


@pytest.mark.parametrize("side", SIDES)
def test_rows_are_batched_and_every_restart_is_added(host, monkeypatch, side):
    m = fitted(host, string_frame(), sampling=3)
    want = call(m, side, n=3)
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 7)           # two rows per query call
    fake_device.LOG.clear()
    same(call(m, side, n=3), want, side)
    queries = [d for e, d in fake_device.LOG if e == "similar_query"]
    assert len(queries) == -(-n_rows(m, side) // 2) and max(queries) == 2
    assert sum(1 for e, _ in fake_device.LOG if e == "similar_add") == 3
    assert [e for e, _ in fake_device.LOG][-1] == "similar_end"


def test_the_session_ends_when_a_query_fails(host, monkeypatch):
    m = fitted(host, string_frame())

    def broken(self, ids, n):
        raise RuntimeError("device lost")
    monkeypatch.setattr(SimilarFakeHipEM, "similar_query", broken)
    fake_device.LOG.clear()
    with pytest.raises(RuntimeError, match="device lost"):
        m.similar_items(n=2)
    assert [e for e, _ in fake_device.LOG][-1] == "similar_end"


def test_a_one_item_model_returns_an_empty_frame(host):
    df = pd.DataFrame({"users": [f"u{x}" for x in range(6)], "items": ["only"] * 6, "ratings": [1, 2, 3, 4, 5, 3]})
    m = fitted(host, df)
    got = m.similar_items(n=5)
    assert len(got) == 0 and list(got.columns) == ["items", "similar", "distance", "rank"]
    assert len(m.similar_users(users=["u2"], n=10)) == 5
