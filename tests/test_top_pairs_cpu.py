"""MMSBM.top_pairs() without a GPU: the numpy restatement of the global query (what test_gpu_top_pairs.py compares the
device against), the conditions its tie cases rely on, asserted on the restatement alone, and the host class's side --
labels, request order, the refusals -- through a CPU stand-in that answers recommend_top_pairs with the restatement.

The restatement: the full score matrix of the request (test_recommend_cpu.restate_scores, or scores given), every
(user, item) pair a candidate except the seen ones, order = np.lexsort((item, user, -score)): score descending, equal
scores by ascending user id, then ascending item id; the first min(m, candidates) pairs."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import exact_models as xm
import fake_device
from conftest import ROOT
from test_recommend_cpu import RecommendFakeHipEM, fitted, restate_scores, seen_items, string_frame

TILE = 128                                  # users x items of one score tile (kRecTile)
MS = (1, 10, 300, 1024)                     # the m of the GPU cases


# ---- the restatement ------------------------------------------------------------------------------------------------
def candidate_mask(users, n_items, seen):
    """(len(users), n_items) bool: True where the pair is a candidate."""
    ok = np.ones((len(users), n_items), dtype=bool)
    if seen is not None:
        for b, u in enumerate(np.asarray(users).tolist()):
            if seen[u]:
                ok[b, np.fromiter(seen[u], dtype=np.int64, count=len(seen[u]))] = False
    return ok


def global_order(scores, users, seen):
    """(user ids, item ids, scores) of every candidate pair in the query's order; scores: row b = users[b]."""
    users = np.asarray(users, dtype=np.int64)
    ok = candidate_mask(users, scores.shape[1], seen)
    b, i = np.nonzero(ok)
    u, s = users[b], scores[b, i]
    order = np.lexsort((i, u, -s))
    return u[order], i[order], s[order]


def restate_top_pairs(params, weights, users, m, seen=None, scores=None, n_items=None):
    """(users (m,) int32, items (m,) int32, scores (m,), count) -- what recommend_top_pairs returns; padding -1 / -1 /
    -inf.  users: distinct ids in any order; scores: the request's score matrix when the caller has one."""
    users = np.asarray(users, dtype=np.int64)
    assert len(np.unique(users)) == len(users)
    if scores is None:
        scores = restate_scores(params, users, params[0][1].shape[0] if n_items is None else n_items, weights)
    u, i, s = global_order(scores, users, seen)
    count = min(m, len(u))
    ou, oi, os_ = np.full(m, -1, dtype=np.int32), np.full(m, -1, dtype=np.int32), np.full(m, -np.inf)
    ou[:count], oi[:count], os_[:count] = u[:count], i[:count], s[:count]
    return ou, oi, os_, count


def test_restatement_matches_a_triple_loop():
    rng = np.random.default_rng(0)
    U, I, K, L, R, S = 7, 9, 3, 2, 4, 2
    params = []
    for _ in range(S):
        p = rng.random((K, L, R))
        params.append((rng.random((U, K)), rng.random((I, L)), p / p.sum(axis=2, keepdims=True)))
    params[0][1][4] = params[0][1][1]                       # items 1 and 4 identical in every restart: exact ties
    params[1][1][4] = params[1][1][1]
    w = np.array([1.0, -2.0, 0.5, 3.0])
    seen = [set() for _ in range(U)]
    seen[2] = {0, 1, 8}
    seen[5] = set(range(I))
    users = [5, 2, 6, 0]
    rows = []
    for u in users:
        for i in range(I):
            if i in seen[u]:
                continue
            sc = 0.0
            for theta, eta, p in params:
                for k in range(K):
                    for l in range(L):
                        for r in range(R):
                            sc += theta[u, k] * eta[i, l] * p[k, l, r] * w[r] / S
            rows.append((sc, u, i))
    ref = restate_scores(params, users, I, w)
    got_u, got_i, got_s, count = restate_top_pairs(params, w, users, 12, seen)
    assert count == 12
    # the loop's sums round differently: the order is checked on the restatement's own scores, the scores within rounding
    by_pair = {(u, i): sc for sc, u, i in rows}
    assert len(rows) == 4 * I - 3 - I
    for k in range(count):
        assert abs(by_pair[(got_u[k], got_i[k])] - got_s[k]) <= 1e-13
        assert got_s[k] == ref[users.index(got_u[k]), got_i[k]]
    keys = [(-got_s[k], got_u[k], got_i[k]) for k in range(count)]
    assert keys == sorted(keys)
    everything = sorted((-ref[users.index(u), i], u, i) for _, u, i in rows)
    assert keys == everything[:12]
    for u in (0, 2, 6):                                      # the twins tie exactly and come in item order
        if 1 not in seen[u]:
            assert ref[users.index(u), 1] == ref[users.index(u), 4]
    # more than the candidates: padded
    got_u, got_i, got_s, count = restate_top_pairs(params, w, users, 40, seen)
    assert count == len(rows) and (got_u[count:] == -1).all() and (got_i[count:] == -1).all() and np.isneginf(got_s[count:]).all()
    # request order does not matter
    again = restate_top_pairs(params, w, users[::-1], 12, seen)
    assert np.array_equal(again[0], restate_top_pairs(params, w, users, 12, seen)[0])


@pytest.mark.parametrize("family", xm.FAMILIES)
def test_restatement_on_exact_scores(family):
    """On the models without rounding the order over exact_scores is the order of a plain sort of (-score, user, item),
    and with S a power of two restate_scores gives the same bits as exact_scores."""
    shape = (40, 150, 5, 4, 4, 4)
    U, I, K, L, R, S = shape
    case = xm.make_case(family, "signed", shape)
    ex = case["scores"]
    assert np.array_equal(xm.bits(ex), xm.bits(restate_scores(case["params"], case["users"], I, case["w"]) + 0.0))
    for seen in (None, case["seen"]):
        u, i, s, count = restate_top_pairs(case["params"], case["w"], case["users"], 500, seen, scores=ex)
        want = sorted((-ex[a, b], a, b) for a in range(U) for b in range(I) if seen is None or b not in seen[a])[:500]
        assert count == len(want) == 500
        assert [(-x, int(a), int(b)) for x, a, b in zip(s, u, i)] == want


# ---- the conditions the GPU cases rely on -------------------------------------------------------------------------------
def tie_group(case, exclude, m):
    """(tied, users, items): whether pair m and pair m + 1 of the global order score the same, and the user and item
    ids of the pairs that score exactly what pair m scores."""
    u, i, s = global_order(case["scores"], case["users"], case["seen"] if exclude else None)
    if len(u) <= m:
        return False, u[:0], i[:0]
    grp = s == s[m - 1]
    return bool(s[m - 1] == s[m]), u[grp], i[grp]


def tiles_of(ids):
    return len(np.unique(np.asarray(ids) // TILE))


# With nothing excluded: every block family.  With the training pairs excluded the groups shrink (the edge users of
# make_case have seen whole score levels), and the conditions are asserted for the families that tie by construction
# (exact_models.TIE_FAMILIES); the strictly monotone ones are still compared by equality on the device.
TIE_CASES = [(f, k, s, e) for f in xm.BLOCK_FAMILIES for k in xm.WEIGHT_KINDS for s in xm.MANY for e in (False, True)
             if not e or f in xm.TIE_FAMILIES]


@pytest.mark.parametrize("family,kind,shape,exclude", TIE_CASES,
                         ids=["{}-{}-U{}I{}-{}".format(f, k, s[0], s[1], "unseen_pairs" if e else "all_pairs") for f, k, s, e in TIE_CASES])
def test_tie_groups_sit_on_the_cut_and_cross_tiles(family, kind, shape, exclude):
    case = xm.make_case(family, kind, shape)
    for m in MS:
        tied, gu, gi = tie_group(case, exclude, m)
        assert tied, (family, kind, shape, m)
        assert tiles_of(gu) > 1, (family, kind, shape, m, len(gu))
        if family in ("interleaved", "constant", "rare"):
            assert tiles_of(gi) > 1, (family, kind, shape, m, len(gi))
    if family == "constant":
        u, i, s, count = restate_top_pairs(case["params"], case["w"], case["users"], max(MS),
                                           case["seen"] if exclude else None, scores=case["scores"])
        ok = candidate_mask(case["users"], shape[1], case["seen"] if exclude else None)
        fu, fi = np.nonzero(ok)                              # row-major: (user, item) order
        assert count == max(MS) and np.array_equal(u, fu[:count]) and np.array_equal(i, fi[:count])


# ---- the CPU stand-in -------------------------------------------------------------------------------------------------
class TopPairsFakeHipEM(RecommendFakeHipEM):
    """RecommendFakeHipEM with the global query, answered by the restatement."""
    MAX_TOP_PAIRS = 1024

    def recommend_top_pairs(self, m, users=None):
        assert self._rc["params"], "recommend_top_pairs before recommend_add"
        assert 1 <= m <= self.MAX_TOP_PAIRS
        ids = np.arange(self.n_users) if users is None else np.asarray(users)
        fake_device.LOG.append(("recommend_top_pairs", None if users is None else len(users)))
        return restate_top_pairs(self._rc["params"], self._rc["w"], ids, m, self._rc["seen"], n_items=self.n_items)


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", TopPairsFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(TopPairsFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def expected_frame(model, users, m, exclude_seen=True, weights=None):
    """The restatement in the host class's output format, for encoded user ids (None: all)."""
    enc = model.data_handler
    params = [(r["theta"], r["eta"], r["pr"]) for r in model.results]
    w = np.asarray(model.ratings if weights is None else weights, dtype=np.float64)
    seen = seen_items(model.train, model.p + 1) if exclude_seen else None
    ids = np.arange(model.p + 1) if users is None else np.asarray(users)
    u, i, s, count = restate_top_pairs(params, w, ids, m, seen, n_items=model.m + 1)
    ul, il = enc.user_labels(), enc.item_labels()
    rows = [(ul[u[k]], il[i[k]], s[k], k + 1) for k in range(count)]
    return pd.DataFrame(rows, columns=["users", "items", "score", "rank"])


def same(got, want):
    assert list(got.columns) == ["users", "items", "score", "rank"]
    for col in ("users", "items", "rank"):
        assert got[col].tolist() == want[col].tolist(), col
    assert np.array_equal(xm.bits(got["score"].to_numpy(dtype=np.float64)), xm.bits(want["score"].to_numpy(dtype=np.float64)))


def events(prefix="recommend"):
    return [e for e, _ in fake_device.LOG if e.startswith(prefix)]


def test_string_labels_and_none_means_every_user(host):
    df = string_frame()
    m = fitted(host, df)
    m.predict(df.iloc[:40])
    before = m.score(silent=True)["stats"]
    got = m.top_pairs(m=25)
    same(got, expected_frame(m, None, 25))
    assert len(got) == 25 and got["rank"].tolist() == list(range(1, 26))
    assert set(got["users"]) <= set(df["users"]) and set(got["items"]) <= set(df["items"])
    trained = set(zip(df["users"], df["items"]))
    assert not trained & set(zip(got["users"], got["items"]))            # exclude_seen: no training pair
    assert (np.diff(got["score"].to_numpy()) <= 0).all()
    assert m.score(silent=True)["stats"] == before                       # the stored predictions are untouched
    assert ("recommend_top_pairs", None) in fake_device.LOG              # users=None reaches the device as None
    assert events()[0] == "recommend_begin" and events()[-1] == "recommend_end"


def test_request_order_is_irrelevant_and_subsets_are_ranked_alone(host):
    m = fitted(host, string_frame())
    labels = m.data_handler.user_labels()
    ask = [labels[7], labels[1], labels[4]]
    got = m.top_pairs(m=10, users=ask)
    same(got, expected_frame(m, [7, 1, 4], 10))
    same(m.top_pairs(m=10, users=ask[::-1]), got)
    assert set(got["users"]) <= set(ask)


def test_without_exclusion_and_with_one_hot_weights(host):
    m = fitted(host, string_frame())
    same(m.top_pairs(m=30, exclude_seen=False), expected_frame(m, None, 30, exclude_seen=False))
    w = [0, 0, 0, 0, 1]
    same(m.top_pairs(m=30, weights=w), expected_frame(m, None, 30, weights=w))


def test_every_restart_is_added_and_the_session_ends(host, monkeypatch):
    m = fitted(host, string_frame(), sampling=3)
    fake_device.LOG.clear()
    m.top_pairs(m=5)
    assert sum(1 for e, _ in fake_device.LOG if e == "recommend_add") == 3
    assert events()[-1] == "recommend_end"

    def broken(self, m, users=None):
        raise RuntimeError("device lost")
    monkeypatch.setattr(TopPairsFakeHipEM, "recommend_top_pairs", broken)
    fake_device.LOG.clear()
    with pytest.raises(RuntimeError, match="device lost"):
        m.top_pairs(m=5)
    assert events()[-1] == "recommend_end"


def test_refusals_come_before_any_device_call(host):
    m = fitted(host, string_frame())
    labels = m.data_handler.user_labels()
    fake_device.LOG.clear()
    for bad in (0, -3, 2.5, True, None, "7"):
        with pytest.raises(ValueError, match="positive integer"):
            m.top_pairs(m=bad)
    with pytest.raises(ValueError, match="beyond the 1024"):
        m.top_pairs(m=1025)
    with pytest.raises(ValueError, match="more than once"):
        m.top_pairs(users=[labels[3], labels[0], labels[3]])
    with pytest.raises(KeyError, match="nobody"):
        m.top_pairs(users=[labels[0], "nobody"])
    with pytest.raises(ValueError, match="weights"):
        m.top_pairs(weights=[1.0, 2.0])
    assert not fake_device.LOG                                            # refused before any device call
    assert len(m.top_pairs(m=1024)) == min(1024, len(expected_frame(m, None, 1024)))


def test_everything_seen_gives_an_empty_frame(host):
    df = pd.DataFrame({"users": [f"u{x}" for x in range(6) for _ in range(2)], "items": ["a", "b"] * 6,
                       "ratings": [1, 2, 3, 4, 5, 3, 2, 2, 1, 5, 4, 4]})
    m = fitted(host, df)
    got = m.top_pairs(m=5)
    assert len(got) == 0 and list(got.columns) == ["users", "items", "score", "rank"]
    assert len(m.top_pairs(m=50, exclude_seen=False)) == 12              # fewer candidates than m: all of them


def test_distributed_share_is_refused(host):
    m = fitted(host, string_frame(), sampling=3)
    m._restart_ids = m._restart_ids[:1]                                  # what fit_distributed(gather=False) leaves on a rank
    m.results = m.results[:1]
    with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
        m.top_pairs()


def test_ids_after_fit_encoded(host):
    rng = np.random.default_rng(2)
    train = np.stack([rng.integers(0, 9, 80), rng.integers(0, 11, 80), rng.integers(0, 4, 80)], 1)
    train[:9, 0], train[:11, 1], train[:4, 2] = np.arange(9), np.arange(11), np.arange(4)
    m = host.MMSBM(2, 3, iterations=3, sampling=2, seed=7)
    m.fit_encoded(train)
    got = m.top_pairs(m=6, users=[4, 0])
    params = [(r["theta"], r["eta"], r["pr"]) for r in m.results]
    want = restate_top_pairs(params, np.asarray(m.ratings, dtype=np.float64), [4, 0], 6, seen_items(train, 9), n_items=11)
    assert got["users"].tolist() == want[0].tolist() and got["items"].tolist() == want[1].tolist()
    assert np.array_equal(xm.bits(got["score"].to_numpy()), xm.bits(want[2]))
    with pytest.raises(KeyError, match="9"):
        m.top_pairs(users=[9])


def test_the_bound_is_stated_once_per_layer_and_agrees():
    import mmsbm_amd.mmsbm as host
    from mmsbm_amd.core import HipEM
    with open(os.path.join(ROOT, "include", "mmsbm_hip.h")) as fh:
        bound = int(re.search(r"#define MMSBM_HIP_TOP_PAIRS_MAX_M (\d+)", fh.read()).group(1))
    assert bound >= 1024 and HipEM.MAX_TOP_PAIRS == bound and host.MMSBM.TOP_PAIRS_MAX == bound
    assert hasattr(HipEM, "recommend_top_pairs")


# ---- the kernels' decomposition, emulated ---------------------------------------------------------------------------------
CAP, FAN, BLOCK = 2048, 64, 256             # kTopCap, kTopFan, kBlock of top_pairs.hpp


def _better(s, k, thr):
    return thr is None or s > thr[0] or (s == thr[0] and k < thr[1])


def _sort_cut(lst, m):
    lst.sort(key=lambda e: (-e[0], e[1]))
    del lst[m:]
    return lst[m - 1] if len(lst) == m else None


def emulate_top_pairs(scores, users, seen, m, groups):
    """top_pairs.hpp step by step on the host: `groups` workgroups over contiguous runs of 128 x 128 tiles, per tile
    the pairs in thread order (16 x 16 threads, 8 x 8 pairs each: rows 8 in a row, columns 16 apart), judged against
    the workgroup's threshold, appended while the list of CAP entries has room, the list sorted and cut to m when it
    is full, the waiting pairs judged again; then the k-major merges of FAN lists."""
    users = np.asarray(users, dtype=np.int64)
    order = np.argsort(users)
    users, scores = users[order], scores[order]
    nb, ni = scores.shape
    n_it, n_ut = -(-ni // TILE), -(-nb // TILE)
    T = n_it * n_ut
    G = min(groups, T)
    lists = []
    tid = np.arange(BLOCK)
    e = np.arange(64)
    rows = ((tid // 16)[:, None] * 8 + (e // 8)[None, :]).ravel()          # thread-major, then e = a * 8 + c
    cols = ((tid % 16)[:, None] + 16 * (e % 8)[None, :]).ravel()
    for g in range(G):
        t0 = (T // G) * g + min(g, T % G)
        t1 = t0 + T // G + (1 if g < T % G else 0)
        lst, thr = [], None
        for t in range(t0, t1):
            b0, i0 = (t // n_it) * TILE, (t % n_it) * TILE
            b, i = b0 + rows, i0 + cols
            ok = (b < nb) & (i < ni)                                      # masked by index
            wait = [(float(scores[bb, ii]), (int(users[bb]) << 32) | int(ii)) for bb, ii in zip(b[ok].tolist(), i[ok].tolist())]
            first = True
            while True:
                surv = [x for x in wait if _better(x[0], x[1], thr)]
                if first and seen is not None:
                    surv = [x for x in surv if (x[1] & 0xffffffff) not in seen[x[1] >> 32]]
                first = False
                if not surv:
                    break
                room = CAP - len(lst)
                lst.extend(surv[:room])
                wait = surv[room:]
                if not wait:
                    break
                thr = _sort_cut(lst, m) or thr
            if thr is None and len(lst) >= m:
                thr = _sort_cut(lst, m)
        _sort_cut(lst, m)
        lists.append(lst)
    while True:
        out = []
        for l0 in range(0, len(lists), FAN):
            part = lists[l0:l0 + FAN]
            nl = len(part)
            lst, thr = [], None
            for base in range(0, nl * m, BLOCK):
                if len(lst) + BLOCK > CAP:
                    thr = _sort_cut(lst, m) or thr
                rnd = [part[p % nl][p // nl] for p in range(base, min(base + BLOCK, nl * m)) if p // nl < len(part[p % nl])]
                rnd = [x for x in rnd if _better(x[0], x[1], thr)]
                if not rnd:
                    break
                lst.extend(rnd)
            _sort_cut(lst, m)
            out.append(lst)
        lists = out
        if len(lists) == 1:
            break
    best = lists[0]
    ou, oi, os_ = np.full(m, -1, dtype=np.int32), np.full(m, -1, dtype=np.int32), np.full(m, -np.inf)
    for k, (s, key) in enumerate(best):
        ou[k], oi[k], os_[k] = key >> 32, key & 0xffffffff, s
    return ou, oi, os_, len(best)


@pytest.mark.parametrize("family,kind", [("constant", "stars"), ("interleaved", "signed"), ("rare", "indicator"), ("mixed", "stars")])
def test_the_decomposition_cannot_change_the_answer(family, kind):
    """The emulated kernels give the restatement's answer for 1, 2, 7 and 24 workgroups, m on both sides of the list's
    room, with and without exclusion, on mass ties: what top_pairs.hpp argues, executed."""
    shape = xm.MANY[0]
    case = xm.make_case(family, kind, shape)
    for exclude in (False, True):
        seen = case["seen"] if exclude else None
        for m in (10, 1024):
            want = restate_top_pairs(None, None, case["users"], m, seen, scores=case["scores"])
            for groups in (1, 2, 7, 24):
                got = emulate_top_pairs(case["scores"], case["users"], seen, m, groups)
                assert got[3] == want[3], (family, exclude, m, groups)
                for g, w in zip(got[:3], want[:3]):
                    assert np.array_equal(g, w), (family, exclude, m, groups)
