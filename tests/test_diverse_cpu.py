"""MMSBM.recommend_diverse() / distances() / list_diversity() without a GPU: the greedy reference of
diverse_reference.py against brute force and a hand-worked example, the proof from the reference alone that the cases
of test_gpu_diverse.py bite (lists that move, steps decided by the tie rule and steps without a tie), and the host
class's side through a CPU stand-in that answers recommend_diverse / similar_pairs with the restatements."""
import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import diverse_reference as dr
import exact_models as xm
import fake_device
from test_catalogue_cpu import CatalogueFakeHipEM
from test_recommend_cpu import expected_frame, fitted, string_frame
from test_recommend_cpu import same as same_plain
from test_similar_cpu import SimilarFakeHipEM, exact_distances, restate_distances


# ---- the reference ---------------------------------------------------------------------------------------------------------
def random_pool(rng, M, levels=None):
    """A pool in recommend's order and a symmetric distance matrix with a zero diagonal; `levels`: so few distinct
    values that equal scores, equal distances and equal v are common."""
    draw = (lambda size: rng.integers(0, levels, size) / 4.0) if levels else (lambda size: rng.random(size))
    ids = np.sort(rng.choice(10 * M, M, replace=False))
    s = draw(M)
    order = np.lexsort((ids, -s))
    d = draw((M, M))
    d = np.triu(d, 1)
    return ids[order], s[order], d + d.T


def test_fma_many_is_the_fraction_fma():
    rng = np.random.default_rng(0)
    m, s = rng.random(400) * 2.0, rng.random(400) * 10.0 - 3.0
    m[:20], s[20:40] = 0.0, 0.0
    for lam in (0.0, 2.0 ** -3, 0.3, 1.0, 2.0 ** 10, 1e-7, 123456.789):
        want = np.array([dr.fma(lam, float(a), float(b)) for a, b in zip(m, s)])
        assert np.array_equal(xm.bits(dr.fma_many(lam, m, s) + 0.0), xm.bits(want + 0.0)), lam
    # one rounding, not two: 0.3 * m + s differs from the fma somewhere
    assert (0.3 * m + s != dr.fma_many(0.3, m, s)).any()


@pytest.mark.parametrize("levels", [None, 4])
def test_trade_off_zero_is_the_plain_top_n(levels):
    rng = np.random.default_rng(1)
    for M in (0, 1, 2, 7, 30):
        ids, s, d = random_pool(rng, M, levels)
        for n in (1, 3, M, M + 2):
            if n < 1:
                continue
            it, sc, dist, _ = dr.greedy(ids, s, d, n, 0.0)
            k = min(n, M)
            assert np.array_equal(it, ids[:k]) and np.array_equal(xm.bits(sc), xm.bits(s[:k]))
            assert len(dist) == k and (k == 0 or np.isposinf(dist[0]))


@pytest.mark.parametrize("levels", [None, 3])
@pytest.mark.parametrize("lam", [2.0 ** -3, 0.3, 1.0, 2.0 ** 10])
def test_every_step_is_an_arg_max_by_brute_force(lam, levels):
    rng = np.random.default_rng(2)
    any_tie = False
    for M in (2, 5, 9):
        ids, s, d = random_pool(rng, M, levels)
        place = {int(i): k for k, i in enumerate(ids)}
        for n in (2, M - 1, M):
            it, sc, dist, tied = dr.greedy(ids, s, d, n, lam)
            assert len(it) == min(n, M) and it[0] == ids[0] and np.isposinf(dist[0])
            picked = [place[int(it[0])]]
            for j in range(1, len(it)):
                best, best_at, ties = None, None, 0
                for i in range(M):                               # ascending places: strictly larger replaces
                    if i in picked:
                        continue
                    m = min(d[a][i] for a in picked)
                    v = dr.fma(lam, float(m), float(s[i]))
                    if best is None or v > best:
                        best, best_at, ties = v, i, 1
                    elif v == best:
                        ties += 1
                assert place[int(it[j])] == best_at, (M, n, j)
                assert dist[j] == min(d[a][best_at] for a in picked) and sc[j] == s[best_at]
                assert tied[j - 1] == (ties > 1)
                any_tie |= ties > 1
                picked.append(best_at)
    assert any_tie == (levels is not None)                       # the coarse values do produce tied steps


def test_n_equal_to_the_pool_returns_a_permutation_of_it():
    rng = np.random.default_rng(3)
    for M in (1, 6, 40):
        ids, s, d = random_pool(rng, M, 5)
        it, sc, dist, _ = dr.greedy(ids, s, d, M, 1.0)
        assert sorted(it.tolist()) == sorted(ids.tolist()) and sorted(sc.tolist()) == sorted(s.tolist())
        assert (dist[1:] >= 0.0).all()


def test_a_hand_worked_example():
    """Five items; trade_off 1.
        pick 1: 10 (the best score).
        pick 2: m = (0, 1, 2.5, 3) for 11 .. 14, v = 4.5, 5, 5.5, 4               -> 13, distance 2.5
        pick 3: m = (0, 0.5, 1) for 11, 12, 14, v = 4.5, 4.5, 2: a tie            -> 11 (the earlier place), distance 0
        pick 4: m = (0.5, 1) for 12, 14, v = 4.5, 2                              -> 12, distance 0.5
        pick 5: 14, distance min(3, 1, 3, 4) = 1"""
    ids = np.array([10, 11, 12, 13, 14])
    s = np.array([5.0, 4.5, 4.0, 3.0, 1.0])
    d = np.zeros((5, 5))
    for (a, b), v in {(0, 1): 0.0, (0, 2): 1.0, (0, 3): 2.5, (0, 4): 3.0, (1, 2): 1.0, (1, 3): 2.5, (1, 4): 3.0,
                      (2, 3): 0.5, (2, 4): 4.0, (3, 4): 1.0}.items():
        d[a, b] = d[b, a] = v
    it, sc, dist, tied = dr.greedy(ids, s, d, 5, 1.0)
    assert it.tolist() == [10, 13, 11, 12, 14] and sc.tolist() == [5.0, 3.0, 4.5, 4.0, 1.0]
    assert dist.tolist() == [np.inf, 2.5, 0.0, 0.5, 1.0] and tied == [False, True, False, False]
    assert dr.greedy(ids, s, d, 3, 1.0)[0].tolist() == [10, 13, 11]
    assert dr.greedy(ids, s, d, 5, 0.0)[0].tolist() == [10, 11, 12, 13, 14]
    far = dr.greedy(ids, s, d, 5, 2.0 ** 10)                     # the farthest-point order: 10, then 14 (3 away), ...
    assert far[0].tolist()[:2] == [10, 14]
    packed = dr.pack([dr.greedy(ids, s, d, 3, 1.0), dr.greedy(ids[:0], s[:0], d[:0, :0], 3, 1.0)], 4)
    assert packed[0].tolist() == [[10, 13, 11, -1], [-1] * 4] and packed[3].tolist() == [3, 0]
    assert np.isneginf(packed[1][0, 3]) and np.isposinf(packed[2][0, 3]) and np.isposinf(packed[2][1]).all()


# ---- the cases bite: from the reference alone ------------------------------------------------------------------------------
BITE_USERS = np.arange(12)                                       # twelve users, nothing excluded, stars weights, n = 10


def _bite(family, shape, pool, lam):
    """(lists that differ from the plain top-10, tied steps, steps) over BITE_USERS."""
    case = xm.make_case(family, "stars", shape)
    dist = exact_distances(case["params"], "items", np.arange(shape[1]))
    sc = case["scores"][BITE_USERS]
    ties = []
    args = (case["params"], BITE_USERS, case["w"], None, None, None, 10, pool)
    got = dr.exact_diverse(*args, lam, scores=sc, dist=dist, ties=ties)
    plain = dr.exact_diverse(*args, 0.0, scores=sc, dist=dist)
    assert np.array_equal(plain[0], xm.exact_top_n(sc, BITE_USERS, 10)[0])
    moved = int(sum((got[0][b] != plain[0][b]).any() for b in range(len(BITE_USERS))))
    return moved, sum(sum(t) for t in ties), sum(len(t) for t in ties)


@pytest.mark.parametrize("lam", [2.0 ** -3, 0.3, 1.0, 2.0 ** 10])
def test_mixed_lists_move_at_every_trade_off_without_a_tied_step(lam):
    """On xm.MANY[1] every one of the twelve lists differs from the plain top-10 at all four trade-offs; on xm.MANY[0]
    at 0.3, 1 and 2^10 (at 2^-3 nine of its twelve do: the reference's own figure, so that pair is not asserted)."""
    for shape in xm.MANY:
        moved, tied, steps = _bite("mixed", shape, 64, lam)
        assert steps == 108 and tied == 0
        if shape == xm.MANY[1] or lam > 2.0 ** -3:
            assert moved == 12, (shape, lam, moved)


@pytest.mark.parametrize("family", ["sorted", "interleaved"])
def test_block_families_move_only_once_the_pool_reaches_a_second_block(family):
    shape = xm.MANY[1]
    for lam in (0.3, 2.0 ** 10):                                 # pool 64: one block -- nothing can move at any trade-off
        assert _bite(family, shape, 64, lam) == (0, 108, 108)
    assert _bite(family, shape, 256, 2.0 ** 10) == (12, 108, 108)   # every list moves, every step decided by the tie rule


def test_rare_and_ascending_families():
    shape = xm.MANY[1]
    assert _bite("rare", shape, 64, 2.0 ** 10) == (12, 96, 108)
    assert _bite("ascending", shape, 256, 2.0 ** 10) == (12, 0, 108)


# ---- the CPU stand-in ---------------------------------------------------------------------------------------------------------
class DiverseFakeHipEM(CatalogueFakeHipEM, SimilarFakeHipEM):
    """The recommend and the similarity stand-ins with the two queries of this feature, answered by the restatements."""
    _rc = None

    def similar_pairs(self, a, b):
        assert self._sm["params"], "similar_pairs before similar_add"
        a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
        fake_device.LOG.append(("similar_pairs", len(a)))
        if len(a) == 0:
            return np.zeros(0)
        return restate_distances(self._sm["params"], self._sm["side"], a)[np.arange(len(a)), b]

    def recommend_diverse(self, users, n, pool, trade_off, candidates=None, exclude=None):
        assert self._rc["params"] and self._sm["params"] and self._sm["side"] == "items"
        assert len(self._rc["params"]) == len(self._sm["params"]) and 1 <= n <= pool <= 1024
        assert np.isfinite(trade_off) and trade_off >= 0
        users = np.asarray(users)
        extra = None
        if exclude is not None:
            off, it = exclude
            assert len(off) == len(users) + 1 and off[0] == 0 and off[-1] == len(it)
            extra = [it[off[b]:off[b + 1]] for b in range(len(users))]
        fake_device.LOG.append(("recommend_diverse", (len(users), n, pool, float(trade_off))))
        p_ids, p_sc, p_cnt = cat.within_top_n(self._scores(users), users, pool, candidates, self._rc["seen"], extra)
        dist = restate_distances(self._sm["params"], "items", np.arange(self.n_items))
        rows = []
        for b in range(len(users)):
            mine = p_ids[b, :p_cnt[b]].astype(np.int64)
            rows.append(dr.greedy(mine, p_sc[b, :p_cnt[b]], dist[np.ix_(mine, mine)], n, trade_off))
        return dr.pack(rows, n)


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", DiverseFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(DiverseFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def events(prefixes=("recommend", "similar")):
    return [e for e, _ in fake_device.LOG if e.startswith(prefixes)]


def params_of(model):
    return [(r["theta"], r["eta"], r["pr"]) for r in model.results]


# ---- the host class through the stand-in -----------------------------------------------------------------------------------
def test_string_labels_columns_and_both_sessions(host):
    df = string_frame()
    m = fitted(host, df)
    m.predict(df.iloc[:40])
    before = m.score(silent=True)["stats"]
    fake_device.LOG.clear()
    got = m.recommend_diverse(users=["u7", "u1", "u7"], n=3, diversity=0.5, pool=8)
    assert list(got.columns) == ["users", "items", "score", "distance", "rank"]
    assert got["users"].tolist() == ["u7"] * 3 + ["u1"] * 3 + ["u7"] * 3 and got["rank"].tolist() == [1, 2, 3] * 3
    assert set(got["items"]) <= set(df["items"])
    assert np.isposinf(got["distance"].to_numpy()[::3]).all() and np.isfinite(got["distance"].to_numpy()[1::3]).all()
    assert got.iloc[:3].equals(got.iloc[6:].reset_index(drop=True))
    # the sessions: both begun, every restart added to each in one pass, both ended
    assert events() == ["recommend_begin", "similar_begin", "recommend_add", "similar_add", "recommend_add", "similar_add",
                        "recommend_diverse", "similar_end", "recommend_end"]
    assert ("similar_begin", "items") in fake_device.LOG and ("recommend_begin", True) in fake_device.LOG
    # the numbers: the reference over the plain pool and the distances the model reports
    pool = m.recommend(users=["u1"], n=8)
    labels = pool["items"].tolist()
    d = m.distances([(x, y) for x in labels for y in labels])["distance"].to_numpy().reshape(8, 8)
    it, sc, dd, _ = dr.greedy(np.arange(8), pool["score"].to_numpy(), d, 3, 0.5)
    block = got.iloc[3:6]
    assert block["items"].tolist() == [labels[j] for j in it]
    assert np.array_equal(xm.bits(block["score"].to_numpy()), xm.bits(sc))
    assert np.array_equal(xm.bits(block["distance"].to_numpy()), xm.bits(dd))
    assert m.score(silent=True)["stats"] == before               # the stored predictions are untouched


def test_diversity_zero_is_recommend_and_none_means_every_user(host):
    m = fitted(host, string_frame())
    for kw in ({}, {"exclude_seen": False}, {"weights": [0, 0, 0, 0, 1.0]}):
        got = m.recommend_diverse(n=4, diversity=0, **kw)
        same_plain(got.drop(columns="distance"), m.recommend(n=4, **kw))
    got = m.recommend_diverse(n=2, diversity=0.0)
    same_plain(got.drop(columns="distance"), expected_frame(m, list(range(m.p + 1)), 2))


def test_the_default_pool_and_the_arguments_that_reach_the_device(host):
    m = fitted(host, string_frame())
    for n, pool, want in ((3, None, 30), (10, None, 100), (200, None, 1024), (3, 3, 3), (3, 1024, 1024), (5, np.int64(7), 7)):
        fake_device.LOG.clear()
        m.recommend_diverse(users=["u1", "u2"], n=n, diversity=np.float32(0.25), pool=pool)
        assert [d for e, d in fake_device.LOG if e == "recommend_diverse"] == [(2, n, want, 0.25)]


def test_candidates_and_exclusions_are_recommends(host):
    m = fitted(host, string_frame())
    items = m.data_handler.item_labels()
    cand = [items[j] for j in (7, 2, 11, 2, 0, 15, 9, 4)]
    users = ["u6", "u0", "u6"]
    gone = [("u6", items[7]), ("u0", items[2]), ("nobody", items[0]), ("u6", "no-such-item"), ("u3", items[9])]
    got = m.recommend_diverse(users=users, n=3, diversity=0, candidates=cand, exclude=gone)
    same_plain(got.drop(columns="distance"), m.recommend(users=users, n=3, candidates=cand, exclude=gone))
    spread = m.recommend_diverse(users=users, n=3, diversity=50.0, candidates=cand, exclude=gone)
    assert set(spread["items"]) <= set(cand) and not ((spread["users"] == "u6") & (spread["items"] == items[7])).any()
    fake_device.LOG.clear()
    none = m.recommend_diverse(users=users, n=3, diversity=1.0, candidates=[])
    assert len(none) == 0 and list(none.columns) == ["users", "items", "score", "distance", "rank"]
    assert not events()                                          # no device call for an empty candidate set


def test_bad_arguments_are_refused_before_any_device_call(host):
    m = fitted(host, string_frame())
    fake_device.LOG.clear()
    with pytest.raises(TypeError, match="diversity"):
        m.recommend_diverse(users=["u1"], n=3)
    for bad in (-0.1, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="diversity"):
            m.recommend_diverse(users=["u1"], n=3, diversity=bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            m.recommend_diverse(users=["u1"], n=bad, diversity=1.0)
    for n, pool in ((3, 2), (3, 0), (3, 1025), (3, 2.5), (3, True), (1025, None)):
        with pytest.raises(ValueError, match="pool"):
            m.recommend_diverse(users=["u1"], n=n, diversity=1.0, pool=pool)
    with pytest.raises(KeyError, match="nobody"):
        m.recommend_diverse(users=["u1", "nobody"], diversity=1.0)
    with pytest.raises(KeyError, match="no-such-item"):
        m.recommend_diverse(users=["u1"], diversity=1.0, candidates=["item-3", "no-such-item"])
    with pytest.raises(ValueError):
        m.recommend_diverse(users=["u1"], diversity=1.0, weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="side"):
        m.distances([("item-1", "item-2")], side="ratings")
    with pytest.raises(KeyError, match="no-such-item"):
        m.distances([("item-1", "no-such-item")])
    with pytest.raises(KeyError, match="item-1"):
        m.distances([("item-1", "item-2")], side="users")
    with pytest.raises(ValueError):
        m.distances([("item-1",)])
    with pytest.raises(KeyError, match="no-such-item"):
        m.list_diversity(pd.DataFrame({"users": ["u1"], "items": ["no-such-item"]}))
    assert not events()


def test_both_sessions_end_when_the_query_raises(host, monkeypatch):
    m = fitted(host, string_frame())

    def broken(self, *a, **kw):
        raise RuntimeError("device lost")
    monkeypatch.setattr(DiverseFakeHipEM, "recommend_diverse", broken)
    fake_device.LOG.clear()
    with pytest.raises(RuntimeError, match="device lost"):
        m.recommend_diverse(n=2, diversity=1.0)
    assert events()[-2:] == ["similar_end", "recommend_end"]
    # ... and when the second session cannot even begin, the first one is ended
    monkeypatch.setattr(DiverseFakeHipEM, "similar_begin", broken)
    fake_device.LOG.clear()
    with pytest.raises(RuntimeError, match="device lost"):
        m.recommend_diverse(n=2, diversity=1.0)
    assert events() == ["recommend_begin", "recommend_end"]


def test_rows_are_batched_with_their_exclusion_lists(host, monkeypatch):
    m = fitted(host, string_frame(), sampling=3)
    items, users = m.data_handler.item_labels(), m.data_handler.user_labels()
    pairs = [(u, items[(3 * j) % len(items)]) for j, u in enumerate(users)]
    want = m.recommend_diverse(n=3, diversity=2.0, pool=9, exclude=pairs)
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 7)   # two users per query call
    fake_device.LOG.clear()
    got = m.recommend_diverse(n=3, diversity=2.0, pool=9, exclude=pairs)
    assert got.equals(want)
    queries = [d[0] for e, d in fake_device.LOG if e == "recommend_diverse"]
    assert len(queries) == -(-len(users) // 2) and max(queries) == 2
    assert events().count("recommend_add") == 3 and events().count("similar_add") == 3


@pytest.mark.parametrize("side", ["items", "users"])
def test_distances_frame(host, side):
    m = fitted(host, string_frame())
    enc = m.data_handler
    labels = enc.item_labels() if side == "items" else enc.user_labels()
    pairs = [(labels[3], labels[0]), (labels[0], labels[3]), (labels[5], labels[5]), (labels[1], labels[7])]
    fake_device.LOG.clear()
    got = m.distances(pairs, side=side) if side == "users" else m.distances(pd.DataFrame(pairs, columns=["x", "y"]).assign(z=1))
    assert list(got.columns) == ["a", "b", "distance"]
    assert got["a"].tolist() == [p[0] for p in pairs] and got["b"].tolist() == [p[1] for p in pairs]
    ref = restate_distances(params_of(m), side, [3, 0, 5, 1])
    assert np.array_equal(xm.bits(got["distance"].to_numpy()), xm.bits(ref[np.arange(4), [0, 3, 5, 7]]))
    assert got["distance"].iloc[2] == 0.0 and got["distance"].iloc[0] == got["distance"].iloc[1]
    assert events() == ["similar_begin", "similar_add", "similar_add", "similar_pairs", "similar_end"]
    assert ("similar_begin", side) in fake_device.LOG
    fake_device.LOG.clear()
    none = m.distances([], side=side)
    assert len(none) == 0 and list(none.columns) == ["a", "b", "distance"] and not events()


def test_list_diversity_frame(host, monkeypatch):
    m = fitted(host, string_frame())
    recs = m.recommend(users=["u4", "u9", "u2"], n=4)
    recs = pd.concat([recs, pd.DataFrame({"users": ["solo"], "items": [recs["items"].iloc[0]], "score": [1.0], "rank": [1]})],
                     ignore_index=True)
    fake_device.LOG.clear()
    got = m.list_diversity(recs)
    assert list(got.columns) == ["users", "n", "diversity"]
    assert got["users"].tolist() == ["u4", "u9", "u2", "solo"] and got["n"].tolist() == [4, 4, 4, 1]
    assert np.isnan(got["diversity"].iloc[3])
    ids = {lab: j for j, lab in enumerate(m.data_handler.item_labels())}
    full = restate_distances(params_of(m), "items", np.arange(m.m + 1))
    for b, u in enumerate(["u4", "u9", "u2"]):
        mine = [ids[x] for x in recs[recs["users"] == u]["items"]]
        want = np.mean([full[x, y] for k, x in enumerate(mine) for y in mine[k + 1:]])
        assert got["diversity"].iloc[b] == pytest.approx(want, rel=1e-13)
    assert events() == ["similar_begin", "similar_add", "similar_add", "similar_pairs", "similar_end"]
    assert [d for e, d in fake_device.LOG if e == "similar_pairs"] == [18]
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 5)   # the pairs go to the device in calls of five
    again = m.list_diversity(recs)
    assert np.array_equal(xm.bits(again["diversity"].to_numpy()), xm.bits(got["diversity"].to_numpy()))
    # what diversity= buys, read from the summary: the spread list is at least as diverse where the pool allows it
    spread = m.list_diversity(m.recommend_diverse(users=["u4"], n=4, diversity=1000.0, pool=12))
    assert spread["diversity"].iloc[0] >= got["diversity"].iloc[0]
    empty = m.list_diversity(recs.iloc[:0])
    assert len(empty) == 0 and list(empty.columns) == ["users", "n", "diversity"]


def test_the_plain_recommend_issues_the_calls_it_issued_before(host):
    m = fitted(host, string_frame(), sampling=2)
    fake_device.LOG.clear()
    m.recommend(users=["u1", "u2"], n=2)
    log = [(e, d) for e, d in fake_device.LOG if e.startswith(("recommend", "similar"))]
    assert [e for e, _ in log] == ["recommend_begin", "recommend_add", "recommend_add", "recommend_query", "recommend_end"]
    assert log[0] == ("recommend_begin", True) and log[3] == ("recommend_query", 2)
    fake_device.LOG.clear()
    m.similar_items(items=["item-1"], n=2)
    assert events() == ["similar_begin", "similar_add", "similar_add", "similar_query", "similar_end"]


def test_distributed_share_is_refused(host):
    m = fitted(host, string_frame(), sampling=3)
    m._restart_ids = m._restart_ids[:1]
    m.results = m.results[:1]
    with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
        m.recommend_diverse(diversity=1.0)
    with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
        m.distances([("item-1", "item-2")])
    with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
        m.list_diversity(pd.DataFrame({"users": ["u1", "u1"], "items": ["item-1", "item-2"]}))
