"""Recommendation within a part of the catalogue without a GPU: the numpy restatement (catalogue_reference.py) pinned
to test_recommend_cpu.restate, and the host class's side of MMSBM.recommend(candidates=, exclude=) and MMSBM.rerank --
label handling, the KeyErrors, the exclusions that are ignored, rerank's user order, de-duplication and n=None rule --
through a CPU stand-in that answers the new queries from the restatement."""
import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import fake_device
from test_recommend_cpu import RecommendFakeHipEM, expected_frame, fitted, restate, restate_scores, same, string_frame


# ---- the restatement ---------------------------------------------------------------------------------------------------
def random_scores(rng, M, I, ties=True):
    s = rng.integers(0, 6, (M, I)).astype(np.float64) if ties else rng.random((M, I))
    return s


@pytest.mark.parametrize("ties", [True, False])
def test_within_top_n_is_restate_with_the_complement_and_the_extras_seen(ties):
    rng = np.random.default_rng(4)
    U, I = 7, 40
    scores = random_scores(rng, U, I, ties)
    users = np.array([3, 0, 3, 6, 1])                       # user 3 twice, with different extra lists
    rows = scores[users]
    seen = [set(rng.choice(I, rng.integers(0, 9), replace=False).tolist()) for _ in range(U)]
    extra = [set(rng.choice(I, k, replace=False).tolist()) for k in (0, 1, 12, 40, 5)]
    for cand in (None, np.arange(I), np.arange(0, I, 2), np.array([5]), np.zeros(0, dtype=np.int64), np.array([0, I - 1])):
        for n in (1, 3, I + 2):
            for sn in (seen, None):
                for ex in (extra, None):
                    got = cat.within_top_n(rows, users, n, cand, sn, ex)
                    comp = set() if cand is None else set(range(I)) - set(np.asarray(cand).tolist())
                    for b, u in enumerate(users.tolist()):
                        out = comp | (set() if sn is None else sn[u]) | (set() if ex is None else ex[b])
                        want = restate(None, [0], I, None, n, [out], scores=rows[b:b + 1])
                        for g, w in zip(got, want):
                            assert np.array_equal(np.asarray(g)[b:b + 1], w), (cand, n, b)


def test_rank_lists_is_within_top_n_of_each_list():
    rng = np.random.default_rng(5)
    U, I = 6, 50
    scores = random_scores(rng, U, I)
    users = np.array([2, 2, 5, 0])
    rows = scores[users]
    seen = [set(rng.choice(I, 6, replace=False).tolist()) for _ in range(U)]
    lists = [np.sort(rng.choice(I, k, replace=False)) for k in (0, 1, 17, 50)]
    off, items = cat.csr(lists)
    for n in (1, 4, 60):
        for sn in (seen, None):
            got = cat.rank_lists(rows, users, off, items, n, sn)
            for b in range(len(users)):
                want = cat.within_top_n(rows[b:b + 1], users[b:b + 1], n, lists[b], sn, None)
                for g, w in zip(got, want):
                    assert np.array_equal(np.asarray(g)[b:b + 1], w), (n, b)


# ---- the CPU stand-in ----------------------------------------------------------------------------------------------------
class CatalogueFakeHipEM(RecommendFakeHipEM):
    """RecommendFakeHipEM with the queries within a part of the catalogue, answered by the restatement."""

    def _scores(self, users):
        return restate_scores(self._rc["params"], users, self.n_items, self._rc["w"])

    def recommend_query_within(self, users, n, candidates=None, exclude=None):
        assert self._rc["params"] and 1 <= n <= 1024
        users = np.asarray(users)
        if candidates is not None:
            c = np.asarray(candidates)
            assert c.dtype == np.int32 and (np.diff(c) > 0).all() and (len(c) == 0 or (c[0] >= 0 and c[-1] < self.n_items))
        extra = None
        if exclude is not None:
            off, it = exclude
            assert len(off) == len(users) + 1 and off[0] == 0 and off[-1] == len(it)
            extra = [it[off[b]:off[b + 1]] for b in range(len(users))]
        fake_device.LOG.append(("recommend_query_within", len(users)))
        return cat.within_top_n(self._scores(users), users, n, candidates, self._rc["seen"], extra)

    def recommend_rank(self, users, offsets, items, n):
        assert self._rc["params"] and 1 <= n <= 1024
        users, off, items = np.asarray(users), np.asarray(offsets), np.asarray(items)
        assert len(off) == len(users) + 1 and off[0] == 0 and off[-1] == len(items)
        for b in range(len(users)):                           # ascending and distinct, as the library requires
            assert (np.diff(items[off[b]:off[b + 1]]) > 0).all()
        fake_device.LOG.append(("recommend_rank", len(users)))
        return cat.rank_lists(self._scores(users), users, off, items, n, self._rc["seen"])


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", CatalogueFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(CatalogueFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def ids_of(model, side, labels):
    enc = model.data_handler
    index = (enc.user_labels() if side == "users" else enc.item_labels())
    return [index.index(x) for x in labels]


def filtered(model, users, n, keep, exclude_seen=True):
    """recommend()'s full list of each of `users` (labels, request order), the rows kept where keep(row, user, item),
    cut to n and ranked again: what the queries within a part of the catalogue must return."""
    parts = []
    for b, u in enumerate(users):
        full = model.recommend(users=[u], n=model.m + 1, exclude_seen=exclude_seen)
        block = full[np.array([keep(b, u, i) for i in full["items"]], dtype=bool)].head(n).copy()
        block["rank"] = np.arange(1, len(block) + 1)
        parts.append(block)
    return pd.concat(parts, ignore_index=True)


# ---- MMSBM.recommend(candidates=, exclude=) -----------------------------------------------------------------------------
def test_candidates_filter_the_plain_lists(host):
    df = string_frame()
    m = fitted(host, df)
    items = m.data_handler.item_labels()
    cand = [items[j] for j in (7, 2, 11, 2, 0, 15)]           # any order, a duplicate
    users = ["u7", "u1", "u7", "u3"]
    for exclude_seen in (True, False):
        got = m.recommend(users=users, n=3, exclude_seen=exclude_seen, candidates=cand)
        same(got, filtered(m, users, 3, lambda b, u, i: i in cand, exclude_seen))
    every = m.recommend(n=2, candidates=cand)                 # users=None: every training user
    same(every, filtered(m, m.data_handler.user_labels(), 2, lambda b, u, i: i in cand))
    assert set(every["items"]) <= set(cand)


def test_all_candidates_and_no_exclusions_equal_the_plain_call(host):
    m = fitted(host, string_frame())
    want = m.recommend(users=["u2", "u5"], n=4)
    same(m.recommend(users=["u2", "u5"], n=4, candidates=m.data_handler.item_labels()), want)
    same(m.recommend(users=["u2", "u5"], n=4, exclude=[]), want)


def test_empty_candidates_give_an_empty_frame_and_unknown_ones_a_key_error(host):
    m = fitted(host, string_frame())
    fake_device.LOG.clear()
    got = m.recommend(users=["u1"], n=3, candidates=[])
    assert len(got) == 0 and list(got.columns) == ["users", "items", "score", "rank"]
    assert not [e for e, _ in fake_device.LOG if e.startswith("recommend_query")]
    with pytest.raises(KeyError, match="no-such-item"):
        m.recommend(users=["u1"], candidates=["item-3", "no-such-item"])
    with pytest.raises(KeyError, match="nobody"):
        m.recommend(users=["nobody"], candidates=["item-3"])


def test_exclusions_as_tuples_and_as_a_frame_and_the_ones_that_are_ignored(host):
    df = string_frame()
    m = fitted(host, df)
    users = ["u4", "u9"]
    plain = m.recommend(users=users, n=3, exclude_seen=False)
    top = {u: plain[plain["users"] == u]["items"].tolist() for u in users}
    pairs = [("u4", top["u4"][0]), ("u4", top["u4"][2]), ("u9", top["u9"][1]), ("u4", top["u4"][0]),
             ("u2", top["u4"][1]),                            # a user that is not requested
             ("nobody", top["u9"][0]), ("u9", "no-such-item")]  # labels that are not in the training data
    gone = {("u4", top["u4"][0]), ("u4", top["u4"][2]), ("u9", top["u9"][1])}
    want = filtered(m, users, 3, lambda b, u, i: (u, i) not in gone, exclude_seen=False)
    same(m.recommend(users=users, n=3, exclude_seen=False, exclude=pairs), want)
    frame = pd.DataFrame(pairs, columns=["a", "b"]).assign(extra=1.0)     # first two columns, the rest ignored
    same(m.recommend(users=users, n=3, exclude_seen=False, exclude=frame), want)
    assert top["u4"][1] in want[want["users"] == "u4"]["items"].tolist()
    with pytest.raises(ValueError):
        m.recommend(users=users, exclude=[("u4",)])
    with pytest.raises(ValueError):
        m.recommend(users=users, exclude=pd.DataFrame({"only": ["u4"]}))


def test_candidates_and_exclusions_together_with_a_repeated_user(host):
    m = fitted(host, string_frame())
    items = m.data_handler.item_labels()
    cand = items[::2]
    users = ["u6", "u0", "u6"]
    gone = {("u6", cand[0]), ("u6", cand[3]), ("u0", cand[1]), ("u0", items[1])}   # (items[1]: not a candidate)
    got = m.recommend(users=users, n=5, candidates=cand, exclude=sorted(gone))
    same(got, filtered(m, users, 5, lambda b, u, i: i in cand and (u, i) not in gone))


def test_queries_are_batched_with_their_exclusion_lists(host, monkeypatch):
    m = fitted(host, string_frame())
    items = m.data_handler.item_labels()
    users = m.data_handler.user_labels()
    pairs = [(u, items[(3 * j) % len(items)]) for j, u in enumerate(users)] + [(users[0], items[5])]
    want = m.recommend(n=3, exclude_seen=False, exclude=pairs)
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 7)       # two users per query call
    fake_device.LOG.clear()
    same(m.recommend(n=3, exclude_seen=False, exclude=pairs), want)
    queries = [d for e, d in fake_device.LOG if e == "recommend_query_within"]
    assert len(queries) == -(-len(users) // 2) and max(queries) == 2
    assert [e for e, _ in fake_device.LOG][-1] == "recommend_end"


def test_the_plain_call_issues_the_calls_it_issued_before(host):
    m = fitted(host, string_frame(), sampling=2)
    fake_device.LOG.clear()
    m.recommend(users=["u1", "u2"], n=2)
    log = [(e, d) for e, d in fake_device.LOG if e.startswith("recommend")]
    assert [e for e, _ in log] == ["recommend_begin", "recommend_add", "recommend_add", "recommend_query", "recommend_end"]
    assert log[0] == ("recommend_begin", True) and log[3] == ("recommend_query", 2)
    same(m.recommend(users=["u1", "u2"], n=2), expected_frame(m, ids_of(m, "users", ["u1", "u2"]), 2))


# ---- MMSBM.rerank ---------------------------------------------------------------------------------------------------------
def test_rerank_orders_each_users_list_in_order_of_first_appearance(host):
    m = fitted(host, string_frame())
    items = m.data_handler.item_labels()
    pairs = [("u8", items[4]), ("u2", items[9]), ("u8", items[1]), ("u8", items[4]),     # a repeated pair
             ("u2", items[0]), ("u5", items[3]), ("u8", items[12]), ("u2", items[9]), ("u8", items[0])]
    lists = {}
    for u, i in pairs:
        lists.setdefault(u, set()).add(i)
    users = ["u8", "u2", "u5"]
    for exclude_seen in (True, False):
        got = m.rerank(pairs, exclude_seen=exclude_seen)                                  # n=None: the whole lists
        want = filtered(m, users, len(items), lambda b, u, i: i in lists[u], exclude_seen)
        same(got, want)
        same(m.rerank(pd.DataFrame(pairs, columns=["users", "items"]).assign(x=0), n=2, exclude_seen=exclude_seen),
             filtered(m, users, 2, lambda b, u, i: i in lists[u], exclude_seen))
    assert m.rerank(pairs, exclude_seen=False)["users"].drop_duplicates().tolist() == users
    assert len(m.rerank(pairs, exclude_seen=False)) == sum(len(v) for v in lists.values())


def test_rerank_scores_are_recommends_scores(host):
    m = fitted(host, string_frame())
    full = m.recommend(n=m.m + 1, exclude_seen=False)
    pairs = full.sample(25, random_state=1)[["users", "items"]]
    got = m.rerank(pairs, exclude_seen=False)
    joined = got.merge(full, on=["users", "items"], suffixes=("", "_full"))
    assert len(joined) == len(got) == 25
    assert np.array_equal(joined["score"].to_numpy().view(np.uint64), joined["score_full"].to_numpy().view(np.uint64))


def test_rerank_arguments(host, monkeypatch):
    m = fitted(host, string_frame())
    items = m.data_handler.item_labels()
    with pytest.raises(KeyError, match="nobody"):
        m.rerank([("nobody", items[0])])
    with pytest.raises(KeyError, match="no-such-item"):
        m.rerank([("u1", "no-such-item")])
    with pytest.raises(ValueError):
        m.rerank([("u1", items[0], 3)])
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            m.rerank([("u1", items[0])], n=bad)
    empty = m.rerank([])
    assert len(empty) == 0 and list(empty.columns) == ["users", "items", "score", "rank"]
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_MAX", 3)      # the longest list a query returns whole
    three = [("u1", items[j]) for j in range(3)]
    assert len(m.rerank(three, exclude_seen=False)) == 3
    with pytest.raises(ValueError, match="explicit n"):
        m.rerank(three + [("u1", items[3])], exclude_seen=False)
    assert len(m.rerank(three + [("u1", items[3])], n=2, exclude_seen=False)) == 2


def test_rerank_is_batched_and_ends_its_session(host, monkeypatch):
    m = fitted(host, string_frame())
    items = m.data_handler.item_labels()
    pairs = [(u, items[(j + k) % len(items)]) for j, u in enumerate(m.data_handler.user_labels()) for k in range(3)]
    want = m.rerank(pairs, n=3, exclude_seen=False)
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 7)       # two users per query call
    fake_device.LOG.clear()
    same(m.rerank(pairs, n=3, exclude_seen=False), want)
    queries = [d for e, d in fake_device.LOG if e == "recommend_rank"]
    assert len(queries) == -(-(m.p + 1) // 2) and max(queries) == 2
    assert [e for e, _ in fake_device.LOG][-1] == "recommend_end"
