"""MMSBM.recommend_group() without a GPU: the numpy restatement of the group query (group_reference.py) pinned on
hand-made matrices, and the host class's side -- the three forms of ``groups``, repeated and unknown users, the bar,
empty candidates, batching, the session's end -- through a CPU stand-in that answers recommend_query_groups with the
restatement."""
import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import fake_device
import group_reference as grp
from test_recommend_cpu import RecommendFakeHipEM, fitted, restate_scores, seen_items, string_frame


# ---- the restatement, pinned ---------------------------------------------------------------------------------------------
S = np.array([[3.0, 1.0, 2.0, 2.0, -1.0],
              [1.0, 4.0, 2.0, 0.0, -1.0],
              [2.0, 2.0, 2.0, 5.0, -3.0]])


def test_hand_made_values():
    off, mem = cat.csr([[0, 1, 2]])
    items, vals, counts = grp.group_top_n(S, off, mem, 5, "min")
    assert counts.tolist() == [5] and items[0].tolist() == [2, 0, 1, 3, 4]       # 2, then the tie 1 = 1 by id, 0, -3
    assert vals[0].tolist() == [2.0, 1.0, 1.0, 0.0, -3.0]
    items, vals, _ = grp.group_top_n(S, off, mem, 5, "max")
    assert items[0].tolist() == [3, 1, 0, 2, 4] and vals[0].tolist() == [5.0, 4.0, 3.0, 2.0, -1.0]
    items, vals, _ = grp.group_top_n(S, off, mem, 5, "count", bar=2.0)           # a bar equal to occurring scores
    assert items[0].tolist() == [2, 0, 1, 3, 4] and vals[0].tolist() == [3.0, 2.0, 2.0, 2.0, 0.0]
    items, vals, _ = grp.group_top_n(S, off, mem, 2, "mean")
    assert items[0].tolist() == [1, 3] and np.array_equal(vals[0], S[:, [1, 3]].mean(axis=0))


@pytest.mark.parametrize("mode", ["min", "max", "mean"])
def test_a_group_of_one_is_the_users_own_list(mode):
    rng = np.random.default_rng(0)
    s = rng.integers(0, 4, (6, 30)).astype(np.float64)                          # mass ties
    seen = [set(rng.choice(30, 5, replace=False).tolist()) for _ in range(6)]
    users = np.array([4, 0, 5, 2])
    off, mem = cat.csr([[u] for u in users])
    for cand in (None, np.arange(0, 30, 3)):
        got = grp.group_top_n(s, off, mem, 7, mode, cand=cand, seen=seen)
        want = cat.within_top_n(s[users], users, 7, cand=cand, seen=seen)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


def test_a_group_of_one_counts_zero_or_one():
    off, mem = cat.csr([[1]])
    items, vals, counts = grp.group_top_n(S, off, mem, 5, "count", bar=1.0)
    assert items[0].tolist() == [0, 1, 2, 3, 4] and vals[0].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0] and counts[0] == 5


def test_ties_go_to_the_smaller_id():
    s = np.ones((3, 8))
    off, mem = cat.csr([[0, 2], [1]])
    for mode in grp.MODES:
        items, _, counts = grp.group_top_n(s, off, mem, 4, mode, bar=1.0, cand=[7, 5, 1, 3, 6])
        assert items.tolist() == [[1, 3, 5, 6]] * 2 and counts.tolist() == [4, 4]


def test_seen_is_the_union_over_the_members_and_an_empty_group_is_empty():
    seen = [{0}, {1, 4}, set()]
    off, mem = cat.csr([[0, 1], [], [2], [1, 0, 2]])
    items, vals, counts = grp.group_top_n(S, off, mem, 5, "max", seen=seen)
    assert counts.tolist() == [2, 0, 5, 2]
    assert items[0, :2].tolist() == [2, 3] and items[3, :2].tolist() == [3, 2]
    assert (items[1] == -1).all() and np.isneginf(vals[1]).all()
    assert (items[0, 2:] == -1).all() and np.isneginf(vals[0, 2:]).all()


# ---- the CPU stand-in ----------------------------------------------------------------------------------------------------
class GroupFakeHipEM(RecommendFakeHipEM):
    """RecommendFakeHipEM with the group query, answered by the restatement."""

    def recommend_query_groups(self, offsets, members, n, mode, bar=0.0, candidates=None):
        assert self._rc["params"] and 1 <= n <= 1024 and mode in grp.MODES
        off, mem = np.asarray(offsets), np.asarray(members)
        assert off.dtype == np.int64 and mem.dtype == np.int32 and off[0] == 0 and off[-1] == len(mem)
        for g in range(len(off) - 1):
            assert len(set(mem[off[g]:off[g + 1]].tolist())) == off[g + 1] - off[g], "a repeated member"
        if candidates is not None:
            c = np.asarray(candidates)
            assert c.dtype == np.int32 and (np.diff(c) > 0).all()
        fake_device.LOG.append(("recommend_query_groups", len(off) - 1))
        scores = restate_scores(self._rc["params"], np.arange(self.n_users), self.n_items, self._rc["w"])
        return grp.group_top_n(scores, off, mem, n, mode, bar, candidates, self._rc["seen"])


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", GroupFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(GroupFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def expected(model, groups, n, mode, bar=0.0, exclude_seen=True, candidates=None, weights=None):
    """The restatement in the host class's output format; groups: {label: [user labels], distinct}."""
    ul, il = model.data_handler.user_labels(), model.data_handler.item_labels()
    params = [(r["theta"], r["eta"], r["pr"]) for r in model.results]
    w = np.asarray(model.ratings if weights is None else weights, dtype=np.float64)
    scores = restate_scores(params, np.arange(model.p + 1), model.m + 1, w)
    seen = seen_items(model.train, model.p + 1) if exclude_seen else None
    off, mem = cat.csr([[ul.index(u) for u in us] for us in groups.values()])
    cand = None if candidates is None else [il.index(i) for i in candidates]
    items, vals, counts = grp.group_top_n(scores, off, mem, n, mode, bar, cand, seen)
    rows = [(g, il[items[b, k]], vals[b, k], k + 1) for b, g in enumerate(groups) for k in range(counts[b])]
    return pd.DataFrame(rows, columns=["group", "items", "score", "rank"])


def same(got, want):
    assert list(got.columns) == ["group", "items", "score", "rank"]
    for c in ("group", "items", "rank"):
        assert got[c].tolist() == want[c].tolist(), c
    np.testing.assert_array_equal(got["score"].to_numpy(dtype=np.float64), want["score"].to_numpy(dtype=np.float64))


GROUPS = {"home": ["u7", "u1", "u3"], "solo": ["u2"], "table": ["u0", "u5", "u9", "u11", "u4"]}
NAMES = {"least_misery": "min", "most_pleasure": "max", "approval": "count", "mean": "mean"}


@pytest.mark.parametrize("aggregate", list(NAMES))
def test_the_three_forms_of_groups(host, aggregate):
    m = fitted(host, string_frame())
    bar = 3.0 if aggregate == "approval" else None
    want = expected(m, GROUPS, 3, NAMES[aggregate], bar or 0.0)
    assert want["group"].unique().tolist() == list(GROUPS) and want["rank"].max() == 3
    same(m.recommend_group(GROUPS, n=3, aggregate=aggregate, bar=bar), want)
    frame = pd.DataFrame([(g, u, "x") for g, us in GROUPS.items() for u in us], columns=["g", "who", "more"])
    same(m.recommend_group(frame, n=3, aggregate=aggregate, bar=bar), want)
    listed = m.recommend_group(list(GROUPS.values()), n=3, aggregate=aggregate, bar=bar)
    assert listed["group"].unique().tolist() == [0, 1, 2]
    same(listed.assign(group=listed["group"].map(dict(enumerate(GROUPS)))), want)


def test_options_reach_the_session(host):
    m = fitted(host, string_frame())
    stock = sorted(set(string_frame()["items"]))[::2]
    w = np.eye(len(m.ratings))[1]
    same(m.recommend_group(GROUPS, n=4, aggregate="most_pleasure", exclude_seen=False, weights=w, candidates=stock + stock[:2]),
         expected(m, GROUPS, 4, "max", exclude_seen=False, candidates=stock, weights=w))
    assert ("recommend_begin", False) in fake_device.LOG


def test_a_repeated_user_counts_once_and_the_first_appearance_fixes_the_order(host):
    m = fitted(host, string_frame())
    got = m.recommend_group({"a": ["u3", "u1", "u3", "u1", "u8"], "b": (x for x in ["u1", "u1"])}, n=5, aggregate="mean")
    same(got, expected(m, {"a": ["u3", "u1", "u8"], "b": ["u1"]}, 5, "mean"))
    labels, (off, mem) = m._group_lists({"a": ["u3", "u1", "u3", "u1", "u8"], "b": [], "c": ["u1"]})
    ul = m.data_handler.user_labels()
    assert labels.tolist() == ["a", "b", "c"] and off.tolist() == [0, 3, 3, 4]
    assert [ul[u] for u in mem] == ["u3", "u1", "u8", "u1"] and off.dtype == np.int64 and mem.dtype == np.int32


def test_an_empty_group_has_no_rows(host):
    m = fitted(host, string_frame())
    got = m.recommend_group({"a": ["u3"], "nobody": [], "c": ["u4"]}, n=2)
    assert got["group"].tolist() == ["a", "a", "c", "c"]
    assert len(m.recommend_group({}, n=2)) == 0 and len(m.recommend_group([], n=2)) == 0


def test_bad_arguments(host):
    m = fitted(host, string_frame())
    with pytest.raises(KeyError, match="stranger"):
        m.recommend_group({"a": ["u1", "stranger"]})
    with pytest.raises(ValueError, match="needs a bar"):
        m.recommend_group(GROUPS, aggregate="approval")
    for bad in (np.nan, np.inf, "3", True):
        with pytest.raises(ValueError, match="bar"):
            m.recommend_group(GROUPS, aggregate="approval", bar=bad)
    for aggregate in ("least_misery", "most_pleasure", "mean"):
        with pytest.raises(ValueError, match="bar belongs"):
            m.recommend_group(GROUPS, aggregate=aggregate, bar=1.0)
    with pytest.raises(ValueError, match="aggregate"):
        m.recommend_group(GROUPS, aggregate="median")
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            m.recommend_group(GROUPS, n=bad)
    with pytest.raises(ValueError):
        m.recommend_group(GROUPS, weights=[1.0, 2.0])
    with pytest.raises(KeyError, match="no-such-item"):
        m.recommend_group(GROUPS, candidates=["no-such-item"])
    with pytest.raises(ValueError, match="two columns"):
        m.recommend_group(pd.DataFrame({"g": [1, 2]}))
    assert not any(e == "recommend_query_groups" for e, _ in fake_device.LOG)


def test_empty_candidates_give_an_empty_frame(host):
    m = fitted(host, string_frame())
    fake_device.LOG.clear()
    got = m.recommend_group(GROUPS, n=3, candidates=[])
    assert len(got) == 0 and list(got.columns) == ["group", "items", "score", "rank"]
    assert not fake_device.LOG                             # no session for nothing


def test_groups_are_batched(host, monkeypatch):
    m = fitted(host, string_frame())
    groups = {f"g{j}": [f"u{j}", f"u{(j + 5) % 12}"] for j in range(7)}
    want = m.recommend_group(groups, n=3, aggregate="approval", bar=2.5)
    same(want, expected(m, groups, 3, "count", 2.5))
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 7)   # two groups per query call
    fake_device.LOG.clear()
    same(m.recommend_group(groups, n=3, aggregate="approval", bar=2.5), want)
    queries = [d for e, d in fake_device.LOG if e == "recommend_query_groups"]
    assert queries == [2, 2, 2, 1]
    assert [e for e, _ in fake_device.LOG][-1] == "recommend_end"


def test_the_session_is_ended_on_error(host, monkeypatch):
    m = fitted(host, string_frame(), sampling=3)

    def broken(self, *a, **k):
        raise RuntimeError("device lost")
    monkeypatch.setattr(GroupFakeHipEM, "recommend_query_groups", broken)
    fake_device.LOG.clear()
    with pytest.raises(RuntimeError, match="device lost"):
        m.recommend_group(GROUPS)
    events = [e for e, _ in fake_device.LOG]
    assert events.count("recommend_add") == 3 and events[-1] == "recommend_end"


def test_distributed_share_is_refused(host):
    m = fitted(host, string_frame(), sampling=3)
    m._restart_ids = m._restart_ids[:1]
    m.results = m.results[:1]
    with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
        m.recommend_group(GROUPS)
