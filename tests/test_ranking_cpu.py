"""MMSBM.heldout_positions() / ranking_score() without a GPU: the positions restated in numpy (against a brute-force
double loop, exact ties included), the metric formulas on hand-made position sets, and the host class's side --
encoding, dropped rows, input order, relevance through the encoder's labels, the session, the argument checks, the
refusal of a distributed share and the untouched model -- through a CPU stand-in that answers recommend_positions with
the restatement.

The restatement is what the GPU tests (test_gpu_ranking.py) compare the device against: scores as in
test_recommend_cpu.restate_scores, candidates = every training item minus the user's own training items when excluded,
position(u, t) = 1 + #{candidates j : s_j > s_t, or s_j == s_t and j < t}, 0 when t is not a candidate."""
import logging
import math

import numpy as np
import pandas as pd
import pytest

import fake_device
from oracle import mmsbm_oracle as orc
from test_recommend_cpu import RecommendFakeHipEM, restate_scores, seen_items, string_frame


# ---- the restatement ----------------------------------------------------------------------------------------------
def restate_positions(scores, offsets, items, users=None, seen=None):
    """(positions (offsets[-1],), candidates (len(offsets) - 1,)): scores[b] = the scores of request row b (all
    items); seen[users[b]] = the items left out, or seen None."""
    scores = np.asarray(scores, dtype=np.float64)
    n_rows, n_items = scores.shape
    positions = np.zeros(int(offsets[-1]), dtype=np.int64)
    candidates = np.zeros(n_rows, dtype=np.int64)
    for b in range(n_rows):
        cand = np.arange(n_items)
        if seen is not None:
            cand = cand[~np.isin(cand, np.fromiter(seen[users[b]], dtype=np.int64, count=len(seen[users[b]])))]
        order = cand[np.lexsort((cand, -scores[b, cand]))]         # score descending, ties by item id
        rank = np.zeros(n_items, dtype=np.int64)
        rank[order] = np.arange(1, len(order) + 1)
        positions[offsets[b]:offsets[b + 1]] = rank[np.asarray(items[offsets[b]:offsets[b + 1]], dtype=np.int64)]
        candidates[b] = len(cand)
    return positions, candidates


def brute_positions(scores, offsets, items, users=None, seen=None):
    positions, candidates = [], []
    for b in range(len(scores)):
        s = scores[b]
        cand = [j for j in range(len(s)) if seen is None or j not in seen[users[b]]]
        candidates.append(len(cand))
        for t in items[offsets[b]:offsets[b + 1]]:
            if t not in cand:
                positions.append(0)
                continue
            positions.append(1 + sum(1 for j in cand if s[j] > s[t] or (s[j] == s[t] and j < t)))
    return positions, candidates


def metrics_loop(rows, ks, relevant=None):
    """ranking_score's definition, one user at a time: rows = [(user, item, rating, position, candidates)]."""
    pairs = {}
    for u, i, r, p, c in rows:
        rel = relevant is None or r in relevant
        old = pairs.get((u, i))
        pairs[(u, i)] = (p, c, rel or (old is not None and old[2]))
    out = {"pairs": len(pairs), "not_candidates": sum(1 for p, _, _ in pairs.values() if p == 0)}
    per_user = {}
    for (u, _), (p, c, rel) in pairs.items():
        per_user.setdefault(u, [c, []])
        if rel and p > 0:
            per_user[u][1].append(p)
    vals = {"mrr": [], "auc": []}
    for k in ks:
        for name in ("precision", "recall", "ndcg", "hit_rate"):
            vals[f"{name}@{k}"] = []
    n_users = 0
    for u, (c, ps) in per_user.items():
        if not ps:
            continue
        n_users += 1
        ps = sorted(ps)
        m = len(ps)
        vals["mrr"].append(1.0 / ps[0])
        if c > m:
            vals["auc"].append(sum(c - m - (p - 1 - a) for a, p in enumerate(ps)) / (m * (c - m)))
        for k in ks:
            hits = sum(1 for p in ps if p <= k)
            vals[f"precision@{k}"].append(hits / k)
            vals[f"recall@{k}"].append(hits / m)
            vals[f"hit_rate@{k}"].append(1.0 if hits else 0.0)
            dcg = sum(1 / math.log2(p + 1) for p in ps if p <= k)
            vals[f"ndcg@{k}"].append(dcg / sum(1 / math.log2(j + 1) for j in range(1, min(k, m) + 1)))
    out["users"], out["skipped_users"] = n_users, len(per_user) - n_users
    for key, v in vals.items():
        out[key] = float(np.mean(v)) if v else float("nan")
    return out


def same_metrics(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for key, v in want.items():
        if isinstance(v, float) and math.isnan(v):
            assert math.isnan(got[key]), key
        else:
            assert got[key] == pytest.approx(v, rel=1e-12, abs=1e-15), (key, got[key], v)


# ---- the restatement against a brute-force double loop --------------------------------------------------------------
def test_positions_match_a_double_loop_with_exact_ties():
    rng = np.random.default_rng(0)
    U, I, R, K, L = 5, 9, 3, 2, 3
    params = [(rng.random((U, K)), rng.random((I, L)), orc.normalize_with_self(rng.random((K, L, R)))) for _ in range(2)]
    for _, e, _ in params:
        e[[2, 6, 7]] = e[4]                                      # items 2, 4, 6, 7 tie exactly
    w = np.array([1.0, 2.5, -0.5])
    users = [0, 3, 1, 4, 3]
    scores = restate_scores(params, users, I, w)
    assert scores[0, 2] == scores[0, 4] == scores[0, 6] == scores[0, 7]
    offsets = np.array([0, 4, 4, 9, 10, 12])
    items = np.array([4, 2, 7, 0, 8, 8, 6, 2, 1, 5, 7, 3])       # repeats, any order
    seen = [{0, 3}, set(), {0, 1, 2, 3, 4, 5, 6, 7, 8}, {6, 2}, {5}]
    for s in (None, seen):
        pos, cand = restate_positions(scores, offsets, items, users, s)
        bpos, bcand = brute_positions(scores, offsets, items, users, s)
        assert pos.tolist() == bpos and cand.tolist() == bcand
    pos, _ = restate_positions(scores, offsets, items, users)
    assert pos[1] + 1 == pos[0] and pos[2] == pos[0] + 2          # 2 < 4 < 7 among equals
    pos, cand = restate_positions(scores, offsets, items, users, seen)
    assert pos[3] == 0 and cand.tolist() == [7, 7, 9, 8, 7]       # item 0 is a training item of user 0


# ---- the metric formulas on hand-made positions ---------------------------------------------------------------------
L2 = math.log2


def hand_rows():
    """(user, item, rating, position, candidates); rating 1 = relevant, 0 = not."""
    return [
        # user 0: C = 10, relevant at 1 and 4 (item 13 twice: once irrelevant), irrelevant at 2
        (0, 10, 1, 1, 10), (0, 11, 0, 2, 10), (0, 13, 0, 4, 10), (0, 13, 1, 4, 10),
        # user 1: C = 3 = m -- no AUC
        (1, 20, 1, 1, 3), (1, 21, 1, 3, 3), (1, 22, 1, 2, 3),
        # user 2: no relevant pair -- skipped
        (2, 30, 0, 7, 50),
        # user 3: C = 6, a relevant pair that is not a candidate, one at 5
        (3, 40, 1, 0, 6), (3, 41, 1, 5, 6),
        # user 4: C = 100, m = 4 > k = 3
        (4, 50, 1, 7, 100), (4, 51, 1, 2, 100), (4, 52, 1, 50, 100), (4, 53, 1, 3, 100),
    ]


def hand_answer():
    """Worked out by hand, per user (0, 1, 3, 4), for k = 3 and k = 20."""
    ndcg3 = [1 / (1 + 1 / L2(3)), 1.0, 0.0, (1 / L2(3) + 1 / L2(4)) / (1 + 1 / L2(3) + 1 / L2(4))]
    ndcg20 = [(1 + 1 / L2(5)) / (1 + 1 / L2(3)), 1.0, 1 / L2(6),
              (1 / L2(3) + 1 / L2(4) + 1 / L2(8)) / (1 + 1 / L2(3) + 1 / L2(4) + 1 / L2(5))]   # (50 > 20)
    mean = lambda v: sum(v) / len(v)
    return {
        "users": 4, "skipped_users": 1, "pairs": 13, "not_candidates": 1,
        "mrr": mean([1, 1, 1 / 5, 1 / 2]),
        "auc": mean([(8 + 6) / 16, (5 - 4) / 5, (95 + 95 + 92 + 50) / (4 * 96)]),   # user 1 has none
        "precision@3": mean([1 / 3, 1, 0, 2 / 3]), "recall@3": mean([1 / 2, 1, 0, 2 / 4]),
        "hit_rate@3": mean([1, 1, 0, 1]), "ndcg@3": mean(ndcg3),
        "precision@20": mean([2 / 20, 3 / 20, 1 / 20, 3 / 20]), "recall@20": mean([1, 1, 1, 3 / 4]),
        "hit_rate@20": 1.0, "ndcg@20": mean(ndcg20),
    }


def test_metric_formulas_by_hand():
    from mmsbm_amd.mmsbm import ranking_metrics
    rows = np.array(hand_rows())
    got = ranking_metrics(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], [3, 20], {1})
    same_metrics(got, hand_answer())
    same_metrics(metrics_loop(hand_rows(), [3, 20], {1}), hand_answer())   # the loop the host tests compare with


def test_metric_edge_cases():
    from mmsbm_amd.mmsbm import ranking_metrics
    rows = np.array(hand_rows())
    shuffled = rows[np.random.default_rng(4).permutation(len(rows))]    # row order does not matter
    a = ranking_metrics(*shuffled.T, [3, 20], {1})
    same_metrics(a, hand_answer())
    every = ranking_metrics(*rows.T, [1], None)                         # every pair relevant
    same_metrics(every, metrics_loop(hand_rows(), [1], None))
    assert every["skipped_users"] == 0 and every["users"] == 5
    none = ranking_metrics(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], [5], {7})
    assert none["users"] == 0 and none["skipped_users"] == 5 and none["pairs"] == 13
    assert all(math.isnan(none[key]) for key in ("mrr", "auc", "precision@5", "recall@5", "ndcg@5", "hit_rate@5"))
    only_full = ranking_metrics(*np.array(hand_rows()[4:7]).T, [2], {1})  # C == m for every user: no AUC at all
    assert math.isnan(only_full["auc"]) and only_full["mrr"] == 1.0 and only_full["precision@2"] == 1.0


# ---- the host class through a CPU stand-in ----------------------------------------------------------------------------
class RankingFakeHipEM(RecommendFakeHipEM):
    """RecommendFakeHipEM with recommend_positions, answered by the restatement."""

    def recommend_positions(self, users, offsets, items):
        assert self._rc["params"], "recommend_positions before recommend_add"
        users = np.asarray(users, dtype=np.int64)
        offsets = np.asarray(offsets, dtype=np.int64)
        assert len(offsets) == len(users) + 1 and offsets[0] == 0 and (np.diff(offsets) >= 0).all()
        assert offsets[-1] == len(items)
        fake_device.LOG.append(("recommend_positions", len(users)))
        scores = restate_scores(self._rc["params"], users, self.n_items, self._rc["w"])
        pos, cand = restate_positions(scores, offsets, items, users.tolist(), self._rc["seen"])
        return pos.astype(np.int32), cand.astype(np.int32)


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", RankingFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(RankingFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def fitted(host, df, sampling=2):
    m = host.MMSBM(2, 3, iterations=3, sampling=sampling, seed=7)
    m.fit(df, silent=True)
    return m


def heldout_frame(df, n=40, seed=9):
    """Test rows: training users and items in new pairs and repeats, plus rows with an unseen user / item / rating."""
    rng = np.random.default_rng(seed)
    users, items = sorted(set(df["users"])), sorted(set(df["items"]))
    test = pd.DataFrame({"users": [users[j] for j in rng.integers(0, len(users), n)],
                         "items": [items[j] for j in rng.integers(0, len(items), n)],
                         "ratings": rng.integers(1, 6, n)})
    extra = pd.DataFrame({"users": ["nobody", users[0], users[1]], "items": [items[0], "no-film", items[2]],
                          "ratings": [3, 4, 9]})
    return pd.concat([test, df.iloc[:5], extra], ignore_index=True)   # df.iloc[:5]: training pairs


def expected_positions(model, test, exclude_seen=True, weights=None):
    """(encoded kept rows, position, candidates) of the test frame from the restatement."""
    enc = model.data_handler
    rows = enc.transform(test)
    params = [(r["theta"], r["eta"], r["pr"]) for r in model.results]
    w = np.asarray(model.ratings if weights is None else weights, dtype=np.float64)
    seen = seen_items(model.train, model.p + 1) if exclude_seen else None
    users = rows[:, 0].tolist()
    offsets = np.arange(len(rows) + 1)                              # one request row per test row
    scores = restate_scores(params, users, model.m + 1, w)
    pos, cand = restate_positions(scores, offsets, rows[:, 1], users, seen)
    return rows, pos, cand


def test_heldout_positions_with_string_labels(host, caplog):
    df = string_frame()
    m = fitted(host, df)
    test = heldout_frame(df)
    with caplog.at_level(logging.WARNING, logger="MMSBM"):
        got = m.heldout_positions(test)
    assert "weren't in the train set" in caplog.text
    assert "nobody" in caplog.text and "no-film" in caplog.text
    rows, pos, cand = expected_positions(m, test)
    assert list(got.columns) == ["users", "items", "ratings", "position", "candidates"]
    assert len(got) == len(test) - 3                                # the three unseen rows are dropped
    kept = test.iloc[:-3]
    assert got["users"].tolist() == kept["users"].tolist()          # input order, the encoder's labels
    assert got["items"].tolist() == kept["items"].tolist()
    assert got["ratings"].tolist() == [str(r) for r in kept["ratings"]]
    assert got["position"].tolist() == pos.tolist() and got["candidates"].tolist() == cand.tolist()
    assert (got["position"].iloc[-5:] == 0).all()                  # training pairs are not candidates
    assert (got["position"] <= got["candidates"]).all()


def test_without_exclusion_and_one_hot_weights(host):
    df = string_frame()
    m = fitted(host, df)
    test = heldout_frame(df)
    w = np.eye(len(m.ratings))[1]
    got = m.heldout_positions(test, exclude_seen=False, weights=w)
    _, pos, cand = expected_positions(m, test, exclude_seen=False, weights=w)
    assert got["position"].tolist() == pos.tolist() and got["candidates"].tolist() == cand.tolist()
    assert (got["position"] > 0).all() and (got["candidates"] == m.m + 1).all()


def test_ranking_score_several_k_and_relevant(host):
    df = string_frame()
    m = fitted(host, df)
    test = heldout_frame(df, n=60)
    rows, pos, cand = expected_positions(m, test)
    table = [(int(u), int(i), int(r), int(p), int(c)) for (u, i, r), p, c in zip(rows.tolist(), pos, cand)]
    got = m.ranking_score(test, k=[1, 5, 1000])
    same_metrics(got, metrics_loop(table, [1, 5, 1000]))
    assert got["users"] > 0 and got["not_candidates"] > 0
    labels = m.data_handler.rating_labels()
    rel = {4, 5}                                                    # rating values as in the data
    got = m.ranking_score(test, k=3, relevant=rel)
    same_metrics(got, metrics_loop(table, [3], {labels.index(str(v)) for v in rel}))
    assert "precision@3" in got and got["skipped_users"] > 0
    assert m.ranking_score(test, k=3, relevant=["4", 5])["mrr"] == got["mrr"]   # matched through str(value)


def test_every_restart_is_added_and_the_session_closed(host):
    m = fitted(host, string_frame(), sampling=3)
    fake_device.LOG.clear()
    m.ranking_score(heldout_frame(string_frame()))
    events = [e for e, _ in fake_device.LOG]
    assert events.count("recommend_add") == 3 and events.count("recommend_positions") == 1
    assert events[-1] == "recommend_end"


def test_model_state_is_unchanged(host):
    df = string_frame()
    m = fitted(host, df)
    m.predict(df.iloc[:30])
    before = {"test": m.test.copy(), "pm": m.prediction_matrix.copy(), "scored": m._scored,
              "theta": m.theta.copy(), "eta": m.eta.copy(), "pr": {k: v.copy() for k, v in m.pr.items()},
              "results": [{k: np.copy(v) for k, v in r.items()} for r in m.results]}
    stats = m.score(silent=True)["stats"]
    m.heldout_positions(heldout_frame(df))
    m.ranking_score(heldout_frame(df), k=[2, 4], relevant={5})
    np.testing.assert_array_equal(m.test, before["test"])
    np.testing.assert_array_equal(m.prediction_matrix, before["pm"])
    assert m._scored is before["scored"]
    pd.testing.assert_frame_equal(m.theta, before["theta"])
    pd.testing.assert_frame_equal(m.eta, before["eta"])
    for k, v in before["pr"].items():
        pd.testing.assert_frame_equal(m.pr[k], v)
    for r, b in zip(m.results, before["results"]):
        for k, v in b.items():
            np.testing.assert_array_equal(r[k], v)
    assert m.score(silent=True)["stats"] == stats


def test_bad_arguments(host):
    df = string_frame()
    m = fitted(host, df)
    test = heldout_frame(df)
    for bad in (0, -1, 2.5, True, [3, 0], [2, False], [], "5", None):
        with pytest.raises(ValueError, match="k must be"):
            m.ranking_score(test, k=bad)
    with pytest.raises(ValueError, match="not a rating"):
        m.ranking_score(test, relevant={5, 7})
    with pytest.raises(ValueError, match="relevant"):
        m.ranking_score(test, relevant=5)
    for fn in (m.heldout_positions, m.ranking_score):
        with pytest.raises(ValueError):
            fn(test, weights=[1.0, 2.0])
        w = np.ones(len(m.ratings))
        w[0] = np.nan
        with pytest.raises(ValueError, match="finite"):
            fn(test, weights=w)


def test_distributed_share_is_refused(host):
    m = fitted(host, string_frame(), sampling=3)
    m._restart_ids = m._restart_ids[:1]               # what fit_distributed(gather=False) leaves on a rank
    m.results = m.results[:1]
    for fn in (m.heldout_positions, m.ranking_score):
        with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
            fn(heldout_frame(string_frame()))


def test_after_fit_encoded(host, caplog):
    rng = np.random.default_rng(2)
    train = np.stack([rng.integers(0, 15, 120), rng.integers(0, 25, 120), rng.integers(0, 4, 120)], 1).astype(np.int32)
    m = host.MMSBM(2, 2, iterations=2, sampling=2, seed=1)
    m.fit_encoded(train)
    test = np.stack([rng.integers(0, 15, 30), rng.integers(0, 25, 30), rng.integers(0, 4, 30)], 1)
    test = np.concatenate([test, [[99, 0, 1], [0, 99, 1]]])
    with caplog.at_level(logging.WARNING, logger="MMSBM"):
        got = m.heldout_positions(test)
    assert "99" in caplog.text and len(got) == 30
    assert got["users"].tolist() == test[:30, 0].tolist() and got["ratings"].tolist() == test[:30, 2].tolist()
    params = [(r["theta"], r["eta"], r["pr"]) for r in m.results]
    scores = restate_scores(params, test[:30, 0], m.m + 1, np.asarray(m.ratings, dtype=np.float64))
    pos, cand = restate_positions(scores, np.arange(31), test[:30, 1], test[:30, 0].tolist(), seen_items(train, m.p + 1))
    assert got["position"].tolist() == pos.tolist() and got["candidates"].tolist() == cand.tolist()
    table = [(int(u), int(i), int(r), int(p), int(c)) for (u, i, r), p, c in zip(test[:30].tolist(), pos, cand)]
    same_metrics(m.ranking_score(test, k=[2, 5], relevant={3}), metrics_loop(table, [2, 5], {3}))
