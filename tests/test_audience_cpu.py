"""Item-side serving without a GPU: MMSBM.recommend_users() / recommend_users_new_items() / audience() through a CPU
stand-in that answers recommend_query_items / recommend_audience with the numpy restatements below; the restatements
against plain Python loops and against the user-side restatement of test_recommend_cpu.py (transposed); and the tie
and trap conditions of the exact cases test_gpu_audience.py runs, asserted here on the restatement so that a GPU case
cannot quietly lose its point.

    restate_item_query(scores_T, items, n, seen_by_item)      what recommend_query_items returns
    restate_audience(scores_T, items, min_score, seen_by_item) what recommend_audience returns

scores_T is (catalogue, U): row i the scores of item i for every user (the transpose of the user-side matrix);
seen_by_item[i]: the users left out for item i, or None."""
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import exact_models as xm
import fake_device
from test_fold_in_items_cpu import ItemsFakeHipEM, new_frame, restate_fold_items, encoded
from test_recommend_cpu import restate, restate_scores, seen_items, string_frame


# ---- the restatements -------------------------------------------------------------------------------------------------
def by_item(seen, n_items):
    """The transpose of per-user seen sets: per item the set of users that leave it out."""
    out = [set() for _ in range(n_items)]
    for u, s in enumerate(seen):
        for i in s:
            out[i].add(u)
    return out


def item_candidates(U, seen_i):
    cand = np.arange(U)
    return cand if not seen_i else cand[~np.isin(cand, np.fromiter(seen_i, dtype=np.int64, count=len(seen_i)))]


def restate_item_query(scores_T, items, n, seen_by_item=None):
    """(users (M, n) padded with -1, scores (M, n) padded with -inf, counts (M,)): score descending, ties by user id."""
    items = np.asarray(items, dtype=np.int64)
    U = scores_T.shape[1]
    users = np.full((len(items), n), -1, dtype=np.int32)
    vals = np.full((len(items), n), -np.inf)
    counts = np.zeros(len(items), dtype=np.int32)
    for b, i in enumerate(items.tolist()):
        cand = item_candidates(U, seen_by_item[i] if seen_by_item is not None else None)
        order = cand[np.lexsort((cand, -scores_T[i, cand]))][:n]
        counts[b] = len(order)
        users[b, :len(order)] = order
        vals[b, :len(order)] = scores_T[i, order]
    return users, vals, counts


def restate_audience(scores_T, items, min_score, seen_by_item=None):
    """(offsets (M + 1,) int64, users int32, scores): per item the candidates with score >= min_score, ascending id."""
    items = np.asarray(items, dtype=np.int64)
    U = scores_T.shape[1]
    offsets = np.zeros(len(items) + 1, dtype=np.int64)
    us, sc = [], []
    for b, i in enumerate(items.tolist()):
        cand = item_candidates(U, seen_by_item[i] if seen_by_item is not None else None)
        keep = cand[scores_T[i, cand] >= min_score]
        us.append(keep.astype(np.int32))
        sc.append(scores_T[i, keep])
        offsets[b + 1] = offsets[b] + len(keep)
    return (offsets, np.concatenate(us) if us else np.zeros(0, dtype=np.int32),
            np.concatenate(sc) if sc else np.zeros(0))


# ---- the restatements against plain loops and against the user side ---------------------------------------------------
def small_problem(seed=0, U=7, I=5):
    rng = np.random.default_rng(seed)
    s = np.round(rng.random((I, U)) * 4) / 4            # quarters: many exact ties
    seen = [set(rng.choice(U, rng.integers(0, U + 1), replace=False).tolist()) for _ in range(I)]
    seen[2] = set(range(U))                              # an item nobody may see
    seen[3] = set()
    return s, seen


def test_item_query_matches_a_double_loop():
    s, seen = small_problem()
    I, U = s.shape
    ask = [4, 0, 2, 0, 3]
    for sb in (seen, None):
        users, vals, counts = restate_item_query(s, ask, 4, sb)
        for b, i in enumerate(ask):
            brute = sorted((-s[i, u], u) for u in range(U) if sb is None or u not in sb[i])[:4]
            assert counts[b] == len(brute)
            assert users[b, :counts[b]].tolist() == [u for _, u in brute]
            assert vals[b, :counts[b]].tolist() == [-v for v, _ in brute]
            assert (users[b, counts[b]:] == -1).all() and np.isneginf(vals[b, counts[b]:]).all()
    assert np.array_equal(restate_item_query(s, ask, 4, seen)[0][1], restate_item_query(s, ask, 4, seen)[0][3])


def test_audience_matches_a_double_loop():
    s, seen = small_problem(1)
    I, U = s.shape
    ask = [1, 1, 4, 2, 0]
    for sb in (seen, None):
        for bar in (-1.0, 0.0, 0.25, 0.5, np.nextafter(0.5, 1), 1.0, 5.0):
            off, us, sc = restate_audience(s, ask, bar, sb)
            assert off[0] == 0 and off.dtype == np.int64 and us.dtype == np.int32
            for b, i in enumerate(ask):
                brute = [(u, s[i, u]) for u in range(U) if s[i, u] >= bar and (sb is None or u not in sb[i])]
                assert us[off[b]:off[b + 1]].tolist() == [u for u, _ in brute]
                assert sc[off[b]:off[b + 1]].tolist() == [v for _, v in brute]
            assert off[-1] == len(us) == len(sc)
    off, us, _ = restate_audience(s, ask, -1.0, seen)
    assert np.diff(off).tolist() == [U - len(seen[i]) for i in ask]       # below the minimum: candidates(i)
    assert restate_audience(s, ask, 5.0, seen)[0].tolist() == [0] * (len(ask) + 1)


def test_both_are_the_transposed_user_side_restatement():
    rng = np.random.default_rng(2)
    U, I = 9, 6
    s = np.round(rng.random((U, I)) * 8) / 8
    train = np.stack([rng.integers(0, U, 20), rng.integers(0, I, 20), np.zeros(20, dtype=np.int64)], 1)
    seen = seen_items(train, U)
    for sb in (seen, None):
        items, vals, counts = restate(None, np.arange(U), I, None, I, sb, scores=s)      # every candidate of every user
        full = np.full((U, I), -np.inf)
        for u in range(U):
            full[u, items[u, :counts[u]]] = vals[u, :counts[u]]
        bi = by_item(sb, I) if sb is not None else None
        users, v2, c2 = restate_item_query(s.T, np.arange(I), U, bi)
        back = np.full((U, I), -np.inf)
        for i in range(I):
            back[users[i, :c2[i]], i] = v2[i, :c2[i]]
        np.testing.assert_array_equal(back, full)
        off, us, sc = restate_audience(s.T, np.arange(I), -1.0, bi)
        back = np.full((U, I), -np.inf)
        back[us, np.repeat(np.arange(I), np.diff(off))] = sc
        np.testing.assert_array_equal(back, full)


# ---- the exact cases of the GPU file: their ties and traps ------------------------------------------------------------
# (family, weight kind, (U, I, K, L, R, S), seed): the seed is the first that gives the case what the tests below assert
EXACT_CASES = [
    ("sorted", "signed", (300, 129, 4, 9, 5, 3), 0),
    ("interleaved", "indicator", (257, 130, 9, 4, 4, 4), 1),
    ("constant", "signed", (300, 40, 5, 5, 4, 3), 1),
    ("rare", "stars", (5000, 2, 4, 6, 3, 1), 0),
    ("mixed", "signed", (129, 257, 17, 20, 4, 3), 0),
    ("mixed", "stars", (130, 3, 2, 3, 3, 1), 43),
]
CASE_ID = lambda c: "{}-{}-U{}I{}K{}L{}R{}S{}".format(c[0], c[1], *c[2])  # noqa: E731
_CASES = {}


def exact_case(case):
    """params, weights, training triples (random pairs, some of them twice), the per-item excluded users and scores_T
    of one exact case; computed once per process and left unchanged."""
    key = CASE_ID(case)
    if key not in _CASES:
        family, kind, shape, seed = case
        U, I, K, L, R, S = shape
        params, w = xm.model(family, np.random.default_rng(seed), U, I, K, L, R, S, kind)
        rng = np.random.default_rng([seed, 1])
        n_obs = 3 * U + 40
        data = np.stack([rng.integers(0, U, n_obs), rng.integers(0, I, n_obs), rng.integers(0, R, n_obs)], 1)
        data = np.concatenate([data, data[:25]])                                   # duplicate pairs count once
        scores_T = np.ascontiguousarray(xm.exact_scores(params, np.arange(U), I, w).T)
        scores_T.setflags(write=False)
        _CASES[key] = {"shape": shape, "params": params, "w": w, "data": data,
                       "seen": by_item(seen_items(data, U), I), "scores_T": scores_T}
    return _CASES[key]


def tie_group(row, value):
    return np.flatnonzero(row == value)


def tiles_of(users):
    return len(set((np.asarray(users) // 128).tolist()))


def median_group(c, item=1):
    row = c["scores_T"][item]
    med = np.sort(row)[len(row) // 2]
    return med, tie_group(row, med)


def is_rounded(x):
    """True when x is no dyadic rational of a small denominator: the quotient by S was rounded."""
    return Fraction(float(x)).denominator > 2 ** 40


def test_sorted_signed_has_a_rounded_median_a_wide_tie_group_and_many_scores_at_or_below_zero():
    c = exact_case(EXACT_CASES[0])
    med, g = median_group(c)
    assert is_rounded(med)                                   # 0.58333...: a rounded quotient of 3
    assert len(g) == 75 and tiles_of(g) == 3
    assert (c["scores_T"] <= 0).sum() > c["scores_T"].size * 2 // 5


def test_interleaved_indicator_fills_the_rank_stage_exactly_and_ties_across_tiles():
    c = exact_case(EXACT_CASES[1])
    U, I, K, L, R, S = c["shape"]
    assert min(K, L) * S == 16
    med, g = median_group(c)
    assert len(g) >= 29 and tiles_of(g) == 3


def test_constant_signed_scores_are_all_one_negative_value():
    c = exact_case(EXACT_CASES[2])
    vals = np.unique(c["scores_T"])
    assert len(vals) == 1 and vals[0] < 0 and is_rounded(vals[0])   # a padded lane's 0.0 would pass any bar <= 0
    assert c["shape"][0] % 128 != 0


def test_rare_stars_ties_over_forty_tiles():
    c = exact_case(EXACT_CASES[3])
    med, g = median_group(c)
    assert len(g) >= 1250 and tiles_of(g) == 40


def test_mixed_signed_crosses_three_rank_stages_with_thousands_of_distinct_scores():
    c = exact_case(EXACT_CASES[4])
    U, I, K, L, R, S = c["shape"]
    assert min(K, L) * S == 51                               # three 16-entry stages and a part of a fourth
    assert len(np.unique(c["scores_T"])) > 2000


def test_mixed_rank_two_ties_every_user_of_item_one():
    c = exact_case(EXACT_CASES[5])
    U, I, K, L, R, S = c["shape"]
    assert min(K, L) * S == 2
    med, g = median_group(c)
    assert len(g) == U == 130


@pytest.mark.parametrize("case", EXACT_CASES, ids=CASE_ID)
def test_the_bars_of_the_gpu_cases_do_what_they_are_there_for(case):
    c = exact_case(case)
    s, seen = c["scores_T"], c["seen"]
    U = s.shape[1]
    items = np.arange(s.shape[0])
    for sb in (seen, None):
        for i in (0, 1, s.shape[0] - 1):
            cand = item_candidates(U, sb[i] if sb else None)
            med = np.sort(s[i])[U // 2]
            in_group = np.isin(cand, tie_group(s[i], med))
            at = restate_audience(s, [i], med, sb)
            above = restate_audience(s, [i], np.nextafter(med, np.inf), sb)
            assert at[0][1] - above[0][1] == in_group.sum()                 # the whole tie group in, then out
        low = restate_audience(s, items, np.nextafter(s.min(), -np.inf), sb)
        assert np.diff(low[0]).tolist() == [U - (len(sb[i]) if sb else 0) for i in items]
        high = restate_audience(s, items, np.nextafter(s.max(), np.inf), sb)
        assert (high[0] == 0).all() and len(high[1]) == 0
    assert any(len(x) for x in seen) and len(c["data"]) > len({(u, i) for u, i, _ in c["data"].tolist()})


# ---- the host class through a stand-in ----------------------------------------------------------------------------------
class AudienceFakeHipEM(ItemsFakeHipEM):
    """The fold-in / extended-catalogue stand-in with the item-side queries, answered by the restatements."""

    def _item_side(self):
        assert self._rc["params"], "an item-side query before recommend_add"
        users = np.arange(self.n_users)
        s = restate_scores(self._rc["params"], users, self.n_items, self._rc["w"])
        n_cat = self.n_items
        if "new" in self._rc:                                   # the added items' columns, from their own eta
            ext = [(t, np.concatenate([e, self._rc["new"][j]]), p) for j, (t, e, p) in enumerate(self._rc["params"])]
            n_cat += self._rc["new"].shape[1]
            s = restate_scores(ext, users, n_cat, self._rc["w"])
        seen = by_item(self._rc["seen"], n_cat) if self._rc["seen"] is not None else None
        return np.ascontiguousarray(s.T), seen, n_cat

    def recommend_query_items(self, items, n):
        s, seen, n_cat = self._item_side()
        assert 1 <= n <= 1024 and all(0 <= i < n_cat for i in np.asarray(items).tolist())
        fake_device.LOG.append(("recommend_query_items", len(items)))
        return restate_item_query(s, items, n, seen)

    def recommend_audience(self, items, min_score, count_only=False, total=None):
        s, seen, n_cat = self._item_side()
        assert np.isfinite(min_score) and all(0 <= i < n_cat for i in np.asarray(items).tolist())
        fake_device.LOG.append(("recommend_audience", (len(items), bool(count_only))))
        off, us, sc = restate_audience(s, items, min_score, seen)
        assert total is None or total == off[-1]
        return (off, None, None) if count_only else (off, us, sc)


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", AudienceFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(AudienceFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def fitted(host, df, sampling=2):
    m = host.MMSBM(2, 3, iterations=3, sampling=sampling, seed=7)
    m.fit(df, silent=True)
    return m


def model_side(m, exclude_seen=True, weights=None):
    params = [(r["theta"], r["eta"], r["pr"]) for r in m.results]
    w = np.asarray(m.ratings if weights is None else weights, dtype=np.float64)
    s = restate_scores(params, np.arange(m.p + 1), m.m + 1, w).T
    seen = by_item(seen_items(m.train, m.p + 1), m.m + 1) if exclude_seen else None
    return s, seen


def expected_users_frame(m, ids, n, **kw):
    s, seen = model_side(m, **kw)
    users, vals, counts = restate_item_query(s, ids, n, seen)
    ul, il = m.data_handler.user_labels(), m.data_handler.item_labels()
    rows = [(il[i], ul[users[b, k]], vals[b, k], k + 1) for b, i in enumerate(ids) for k in range(counts[b])]
    return pd.DataFrame(rows, columns=["items", "users", "score", "rank"])


def expected_audience_frame(m, ids, bar, **kw):
    s, seen = model_side(m, **kw)
    off, us, sc = restate_audience(s, ids, bar, seen)
    ul, il = m.data_handler.user_labels(), m.data_handler.item_labels()
    rows = []
    for b, i in enumerate(ids):
        u, v = us[off[b]:off[b + 1]], sc[off[b]:off[b + 1]]
        for k, j in enumerate(np.lexsort((u, -v)).tolist()):
            rows.append((il[i], ul[u[j]], v[j], k + 1))
    return pd.DataFrame(rows, columns=["items", "users", "score", "rank"])


def same(got, want):
    assert list(got.columns) == ["items", "users", "score", "rank"]
    assert got["items"].tolist() == want["items"].tolist()
    assert got["users"].tolist() == want["users"].tolist()
    assert got["rank"].tolist() == want["rank"].tolist()
    np.testing.assert_array_equal(got["score"].to_numpy(dtype=np.float64), want["score"].to_numpy(dtype=np.float64))


def test_recommend_users_labels_request_order_and_none(host):
    df = string_frame()
    m = fitted(host, df)
    il = m.data_handler.item_labels()
    got = m.recommend_users(n=3)
    same(got, expected_users_frame(m, list(range(m.m + 1)), 3))
    train = set(zip(df["users"], df["items"]))
    assert not any((u, i) in train for u, i in zip(got["users"], got["items"]))
    ask = [il[5], il[0], il[5]]
    got = m.recommend_users(items=ask, n=2)
    same(got, expected_users_frame(m, [5, 0, 5], 2))
    assert got["items"].tolist() == [il[5]] * 2 + [il[0]] * 2 + [il[5]] * 2 and got["rank"].tolist() == [1, 2] * 3
    w = np.eye(len(m.ratings))[1]
    same(m.recommend_users(items=[il[2]], n=4, exclude_seen=False, weights=w),
         expected_users_frame(m, [2], 4, exclude_seen=False, weights=w))
    m.predict(df.iloc[:40])
    before = m.score(silent=True)["stats"]
    m.recommend_users(n=1)
    m.audience(min_score=0.0)
    assert m.score(silent=True)["stats"] == before


def test_recommend_users_is_batched_and_adds_every_restart(host, monkeypatch):
    m = fitted(host, string_frame(), sampling=3)
    want = m.recommend_users(n=3)
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 7)
    fake_device.LOG.clear()
    same(m.recommend_users(n=3), want)
    calls = [d for e, d in fake_device.LOG if e == "recommend_query_items"]
    assert len(calls) == -(-(m.m + 1) // 2) and max(calls) == 2
    assert sum(1 for e, _ in fake_device.LOG if e == "recommend_add") == 3
    assert [e for e, _ in fake_device.LOG][-1] == "recommend_end"


def test_audience_frame_rank_count_only_and_pieces(host, monkeypatch):
    m = fitted(host, string_frame())
    il = m.data_handler.item_labels()
    s, _ = model_side(m)
    bar = float(np.median(s))
    got = m.audience(min_score=bar)
    want = expected_audience_frame(m, list(range(m.m + 1)), bar)
    same(got, want)
    assert len(got) > 0
    for _, g in got.groupby("items", sort=False):
        assert g["rank"].tolist() == list(range(1, len(g) + 1))
        assert (np.diff(g["score"].to_numpy()) <= 0).all()
    counts = m.audience(min_score=bar, count_only=True)
    assert list(counts.columns) == ["items", "count"] and counts["items"].tolist() == il
    assert counts["count"].tolist() == [int((got["items"] == x).sum()) for x in il]
    ask = [il[3], il[1], il[3]]
    same(m.audience(items=ask, min_score=bar, exclude_seen=False), expected_audience_frame(m, [3, 1, 3], bar, exclude_seen=False))
    assert m.audience(items=ask, min_score=bar, count_only=True)["items"].tolist() == ask
    assert len(m.audience(min_score=float(s.max()) + 1.0)) == 0
    monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", 11)         # several filled calls
    fake_device.LOG.clear()
    same(m.audience(min_score=bar), want)
    filled = [d for e, d in fake_device.LOG if e == "recommend_audience" and not d[1]]
    assert len(filled) > 1 and sum(n for n, _ in filled) == m.m + 1


def test_audience_sorts_planted_ties_by_encoded_user_id(host):
    m = fitted(host, string_frame())
    for r in m.results:                       # users 2, 5, 9 become one user: their scores tie bit for bit
        r["theta"][5] = r["theta"][2]
        r["theta"][9] = r["theta"][2]
    m._resident.clear()
    ul = m.data_handler.user_labels()
    s, _ = model_side(m, exclude_seen=False)
    assert s[0, 2] == s[0, 5] == s[0, 9]
    got = m.audience(min_score=float(s.min()) - 1.0, exclude_seen=False)
    same(got, expected_audience_frame(m, list(range(m.m + 1)), float(s.min()) - 1.0, exclude_seen=False))
    first = got[got["items"] == m.data_handler.item_labels()[0]]["users"].tolist()
    at = first.index(ul[2])
    assert first[at:at + 3] == [ul[2], ul[5], ul[9]]
    top = m.recommend_users(n=m.p + 1, exclude_seen=False)
    assert top["users"].tolist() == got["users"].tolist()             # the same order as the top-n form at n = U


def test_bad_arguments(host):
    m = fitted(host, string_frame(), sampling=3)
    for call in (m.recommend_users, lambda **kw: m.audience(min_score=0.0, **kw)):
        with pytest.raises(KeyError, match="no-such-item"):
            call(items=[m.data_handler.item_labels()[0], "no-such-item"])
        with pytest.raises(ValueError):
            call(weights=[1.0, 2.0])
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            m.recommend_users(n=bad)
        with pytest.raises(ValueError):
            m.recommend_users_new_items(new_frame(m), n=bad)
    with pytest.raises(ValueError, match="min_score"):
        m.audience()
    for bad in (np.nan, np.inf, -np.inf, "x", None, True):
        with pytest.raises(ValueError, match="min_score"):
            m.audience(min_score=bad)
    assert not [e for e, _ in fake_device.LOG if e.startswith("recommend_")]      # refused before any device call
    m._restart_ids = m._restart_ids[:1]
    m.results = m.results[:1]
    for call in (m.recommend_users, lambda: m.audience(min_score=0.0), lambda: m.recommend_users_new_items(new_frame(m))):
        with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
            call()


def test_recommend_users_new_items(host):
    m = fitted(host, string_frame())
    df = new_frame(m)
    rows, labels = encoded(m, df)
    got = m.recommend_users_new_items(df, n=3, iterations=4)
    assert list(got.columns) == ["items", "users", "score", "rank"]
    assert list(dict.fromkeys(got["items"])) == labels                # order of first appearance
    assert m.fold_in_items_iterations.shape == (len(labels), 2)
    ul = m.data_handler.user_labels()
    rated = {(lab, ul[u]) for u, j in zip(rows[:, 0].tolist(), rows[:, 1].tolist()) for lab in [labels[j]]}
    assert not any((i, u) in rated for i, u in zip(got["items"], got["users"]))
    # the transposed columns of recommend_with_new_items at n = the whole catalogue
    n_all = m.m + 1 + len(labels)
    wide = m.recommend_with_new_items(df, n=n_all, iterations=4)
    for lab in labels:
        col = wide[wide["items"] == lab]
        order = np.lexsort((np.array([ul.index(u) for u in col["users"]]), -col["score"].to_numpy()))[:3]
        mine = got[got["items"] == lab]
        assert mine["users"].tolist() == col["users"].to_numpy()[order].tolist()
        np.testing.assert_array_equal(mine["score"].to_numpy(), col["score"].to_numpy()[order])
    free = m.recommend_users_new_items(df, n=len(ul), exclude_seen=False, iterations=4)
    assert len(free) == len(labels) * len(ul)
    events = [e for e, _ in fake_device.LOG if e in ("recommend_begin", "fold_in_items", "recommend_add",
                                                      "recommend_add_items", "recommend_query_items", "recommend_end")]
    assert events[-(4 + 2 * 2):] == ["recommend_begin"] + ["fold_in_items", "recommend_add"] * 2 + [
        "recommend_add_items", "recommend_query_items", "recommend_end"]
    clash = df.copy()
    clash.loc[0, "items"] = m.data_handler.item_labels()[0]
    with pytest.raises(ValueError, match="training items"):
        m.recommend_users_new_items(clash)
