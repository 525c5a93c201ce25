"""Positions of held-out items on the device (mmsbm_hip_recommend_positions, HipEM.recommend_positions,
MMSBM.heldout_positions / ranking_score) against the numpy restatement of test_ranking_cpu.py.

Positions and candidate counts are integers and are compared exactly.  The restatement's scores (oracle prod_dist) may
differ from the device's in the last bits, so an item whose restated score lies within TOL x max|score| of another
item's without being equal to it (a near tie, absent from these seeded problems in practice) may move by at most the
number of such neighbours; every other position must be equal.  What holds on the device alone -- consistency with
recommend_query, request independence, swapped contexts, no side effects -- is checked bit for bit.  Positions inside
large tie groups are compared without any band in test_gpu_serving_exact.py, on models whose scores carry no rounding.
"""
import numpy as np
import pandas as pd
import pytest

from oracle import mmsbm_oracle as orc
from test_gpu_recommend import LaunchWindow, context, problem
from test_ranking_cpu import metrics_loop, restate_positions, same_metrics
from test_recommend_cpu import restate_scores, seen_items

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope="module")
def hip():
    from mmsbm_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("-m gpu tests need a GPU: no HIP device visible (no CPU fallback exists)")
    import mmsbm_amd
    return mmsbm_amd


def request(data, U, I, seed, counts=(0, 1, 2, 5, 40)):
    """(users, offsets, items): every user 0..U-1 with a random number of test items from `counts` -- none, fewer
    and more than a chunk of keys -- some of them the user's own training items, some repeated."""
    rng = np.random.default_rng(seed)
    seen = seen_items(data, U)
    users = np.arange(U, dtype=np.int32)
    per, items = [], []
    for u in range(U):
        n = int(rng.choice(counts)) if U > 1 else 40
        it = rng.integers(0, I, n)
        if n >= 2 and seen[u]:
            it[0] = sorted(seen[u])[0]                        # an excluded item
        if n >= 5:
            it[1] = it[2]                                     # a repeat
        per.append(n)
        items.extend(it.tolist())
    offsets = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    return users, offsets, np.asarray(items, dtype=np.int32)


def session(em, n_slots, w, exclude):
    em.recommend_begin(w, exclude)
    for s in range(n_slots):
        em.select(s).recommend_add()


def check_positions(got, params, data, users, offsets, items, n_items, w, exclude, sample=None):
    """got = (positions, candidates) of the device; compared with the restatement for the request rows `sample`."""
    pos, cand = got
    U = int(max(np.max(users), np.max(data[:, 0]))) + 1
    seen = seen_items(data, U) if exclude else None
    rows = np.arange(len(users)) if sample is None else np.asarray(sample)
    scores = restate_scores(params, np.asarray(users)[rows], n_items, w)
    sub_off = np.concatenate([[0], np.cumsum(offsets[rows + 1] - offsets[rows])])
    sub_items = np.concatenate([items[offsets[b]:offsets[b + 1]] for b in rows]) if len(rows) else np.zeros(0, int)
    want_pos, want_cand = restate_positions(scores, sub_off, sub_items, np.asarray(users)[rows].tolist(), seen)
    assert cand[rows].tolist() == want_cand.tolist()
    got_pos = np.concatenate([pos[offsets[b]:offsets[b + 1]] for b in rows]) if len(rows) else np.zeros(0, int)
    exact = 0
    for j, b in enumerate(rows):
        s = scores[j]
        tau = TOL * max(np.abs(s).max(), 1e-300)
        for e in range(sub_off[j], sub_off[j + 1]):
            g, r = int(got_pos[e]), int(want_pos[e])
            if r == 0:
                assert g == 0, (b, e)
                exact += 1
                continue
            t = int(sub_items[e])
            d = np.abs(s - s[t])
            near = int(((d > 0) & (d <= tau)).sum())
            assert abs(g - r) <= near, (b, t, g, r, near)
            exact += g == r
    return exact, len(got_pos)


GRID = [  # (K, L, R, S, U, I, n_obs, duplicated eta rows)
    (2, 3, 2, 1, 300, 1021, 6000, False),          # K <= L
    (20, 20, 5, 3, 500, 997, 10000, True),         # S = 3, exact ties
    (33, 5, 10, 1, 200, 700, 3000, False),         # K > L
    (6, 9, 4, 3, 1, 9000, 600, True),              # one user: the items split across workgroups
]


@pytest.mark.parametrize("case", GRID, ids=[f"K{c[0]}L{c[1]}S{c[3]}U{c[4]}I{c[5]}" for c in GRID])
def test_positions_against_the_restatement(hip, case):
    K, L, R, S, U, I, n_obs, dup = case
    data, params = problem(U, I, R, K, L, S, n_obs, seed=K + 3 * L + S)
    if dup:
        for _, e, _ in params:
            e[[17, 300, I - 1]] = e[5]
    users, offsets, items = request(data, U, I, seed=K)
    if dup:                                            # the tied items in every test list of the first user
        items = np.concatenate([[5, 300, 17, I - 1], items]).astype(np.int32)
        offsets = offsets + 4
        offsets[0] = 0
    em = context(hip, data, params, U, I, R)
    try:
        for exclude in (True, False):
            for w in (np.arange(1.0, R + 1), np.eye(R)[R - 1]):
                session(em, S, w, exclude)
                got = em.recommend_positions(users, offsets, items)
                assert em.get_option("position_ms") > 0
                em.recommend_end()
                exact, total = check_positions(got, params, data, users, offsets, items, I, w, exclude)
                assert exact >= 0.95 * total
                if dup and not exclude:
                    p = got[0][:4]                     # items 5, 17, 300, I-1 in item order among equals
                    assert p[2] == p[0] + 1 and p[1] == p[0] + 2 and p[3] == p[0] + 3, p
                if exclude:                            # an excluded test item is not a candidate
                    seen = seen_items(data, U)
                    for b in range(U):
                        for e in range(offsets[b], offsets[b + 1]):
                            assert (got[0][e] == 0) == (int(items[e]) in seen[b])
    finally:
        em.close()


def test_consistency_with_recommend_query(hip):
    U, I, R = 400, 3000, 5
    data, params = problem(U, I, R, 12, 7, 2, 8000, seed=3)
    users, offsets, items = request(data, U, I, seed=4)
    em = context(hip, data, params, U, I, R)
    try:
        session(em, 2, np.arange(1.0, R + 1), True)
        pos, _ = em.recommend_positions(users, offsets, items)
        for n in (10, 1024):
            top, _, counts = em.recommend_query(users, n)
            for b in range(U):                          # position p <= n: item p - 1 of the query's row
                for e in range(offsets[b], offsets[b + 1]):
                    p = int(pos[e])
                    if 1 <= p <= n:
                        assert top[b, p - 1] == items[e], (b, e, p)
                    elif p > n:
                        assert items[e] not in top[b, :counts[b]]
            back = np.concatenate([top[b, :counts[b]] for b in range(U)])   # and the converse
            off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            bp, _ = em.recommend_positions(users, off, back)
            assert bp.tolist() == np.concatenate([np.arange(1, c + 1) for c in counts]).tolist()
        em.recommend_end()
    finally:
        em.close()


def test_request_independence_swaps_and_uploads(hip):
    U, I, R = 600, 5000, 5
    data, params = problem(U, I, R, 9, 14, 2, 12000, seed=8)
    users, offsets, items = request(data, U, I, seed=9)
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R)
    try:
        em.iterate(2)                                   # resident slots, moved by the EM loop
        fitted = [em.select(s).get_params() for s in range(2)]
        session(em, 2, w, True)
        every, cand = em.recommend_positions(users, offsets, items)
        again, cand2 = em.recommend_positions(users, offsets, items)
        rng = np.random.default_rng(1)
        for ask in (rng.permutation(U), rng.choice(U, 37, replace=False), np.array([5, 5, 77, 5]), np.array([77])):
            per = [items[offsets[b]:offsets[b + 1]] for b in ask]
            off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
            got, c = em.recommend_positions(users[ask], off, np.concatenate(per).astype(np.int32))
            want = np.concatenate([every[offsets[b]:offsets[b + 1]] for b in ask])
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(c, cand[ask])
        em.recommend_end()
    finally:
        em.close()
    np.testing.assert_array_equal(every, again)
    np.testing.assert_array_equal(cand, cand2)
    for swap in (0, 1):
        other = context(hip, data, fitted, U, I, R, swap=swap)
        try:
            assert other.swapped == bool(swap)
            session(other, 2, w, True)
            got, c = other.recommend_positions(users, offsets, items)
            other.recommend_end()
        finally:
            other.close()
        np.testing.assert_array_equal(got, every)
        np.testing.assert_array_equal(c, cand)


def test_no_side_effects(hip):
    U, I, R = 200, 900, 5
    data, params = problem(U, I, R, 10, 10, 3, 4000, seed=13)
    users, offsets, items = request(data, U, I, seed=14)
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(3)]
        test = data[:500]
        em.predict_begin(test, w)
        em.select(0).predict_add()
        session(em, 3, w, True)
        q0 = em.recommend_query(users, 50)
        em.recommend_positions(users, offsets, items)
        q1 = em.recommend_query(users, 50)              # the session answers as before
        p1 = em.recommend_positions(users, offsets, items)
        em.recommend_end()
        em.select(1).predict_add()
        mat, raw = em.predict_finish()
        after = [em.select(s).get_params() for s in range(3)]
        em.predict_begin(test, w)
        em.select(0).predict_add()
        em.select(1).predict_add()
        mat2, raw2 = em.predict_finish()
        session(em, 3, w, True)
        p2 = em.recommend_positions(users, offsets, items)
        em.recommend_end()
    finally:
        em.close()
    for a, b in zip(q0, q1):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(p1, p2):
        np.testing.assert_array_equal(a, b)
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(mat, mat2)
    np.testing.assert_array_equal(raw, raw2)


def test_end_to_end_with_string_ids(hip):
    rng = np.random.default_rng(21)
    n_obs = 5000
    df = pd.DataFrame({"users": [f"user{x}" for x in rng.integers(0, 150, n_obs)],
                       "items": [f"film-{x}" for x in rng.integers(0, 400, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    train, test = df.iloc[:4500], df.iloc[4500:].reset_index(drop=True)
    test = pd.concat([test, pd.DataFrame({"users": ["nobody"], "items": ["film-1"], "ratings": [3]})], ignore_index=True)
    model = hip.MMSBM(4, 5, iterations=30, sampling=3, seed=4)
    model.fit(train, silent=True)
    model.predict(test)
    stats = model.score(silent=True)["stats"]
    kept_test = model.test.copy()
    hp = model.heldout_positions(test)
    assert model.score(silent=True)["stats"] == stats
    np.testing.assert_array_equal(model.test, kept_test)
    enc = model.data_handler
    rows = enc.transform(test)
    assert len(hp) == len(rows) < len(test) and "nobody" not in set(hp["users"])
    assert hp["users"].tolist() == [enc.user_labels()[u] for u in rows[:, 0]]
    params = [(r["theta"], r["eta"], r["pr"]) for r in model.results]
    w = np.asarray(model.ratings, dtype=np.float64)
    users = rows[:, 0]
    off = np.arange(len(rows) + 1, dtype=np.int64)
    exact, total = check_positions((hp["position"].to_numpy(), hp["candidates"].to_numpy()), params, model.train,
                                   users, off, rows[:, 1], model.m + 1, w, True)
    assert exact >= 0.95 * total
    table = [(int(u), int(i), int(r), int(p), int(c))
             for (u, i, r), p, c in zip(rows.tolist(), hp["position"], hp["candidates"])]
    rel = {4, 5}
    got = model.ranking_score(test, k=[1, 10, 100], relevant=rel)
    same_metrics(got, metrics_loop(table, [1, 10, 100], {enc.rating_labels().index(str(v)) for v in rel}))
    assert got["users"] > 0 and 0 <= got["auc"] <= 1


def test_full_size_c3_heldout(hip):
    U, I, R, K = 100_000, 20_000, 5, 20
    data = orc.synthetic_triples(1_000_000, U, I, R, seed=0)
    rng = np.random.default_rng(0)
    held = rng.random(len(data)) < 0.1
    train, test = data[~held], data[held]
    U = int(train[:, 0].max()) + 1
    test = test[test[:, 0] < U]
    params = [(rng.random((U, K)), rng.random((I, K)), orc.normalize_with_self(rng.random((K, K, R))))]
    w = np.arange(1.0, R + 1)
    order = np.argsort(test[:, 0], kind="stable")
    users, counts = np.unique(test[order, 0], return_counts=True)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    items = test[order, 1].astype(np.int32)
    em = context(hip, train, params, U, I, R)
    try:
        session(em, 1, w, True)
        got = em.recommend_positions(users.astype(np.int32), offsets, items)
        assert em.get_option("position_ms") > 0
        em.recommend_end()
    finally:
        em.close()
    sample = np.random.default_rng(2).choice(len(users), 64, replace=False)
    # the sampled users' training rows only (seen_items over the whole train set would do, more slowly)
    mask = np.isin(train[:, 0], users[sample])
    exact, total = check_positions(got, params, train[mask], users, offsets, items, I, w, True, sample)
    assert exact >= 0.95 * total and total > 0
    assert (got[0] <= np.repeat(got[1], counts)).all() and (got[1] <= I).all()


def test_every_position_kernel_is_launched(hip):
    with LaunchWindow() as lw:
        for U, I in ((1, 9000), (300, 400)):           # items split across workgroups; no split
            data, params = problem(U, I, 3, 4, 6, 1, 2000, seed=U)
            users, offsets, items = request(data, U, I, seed=U)
            em = context(hip, data, params, U, I, 3)
            try:
                session(em, 1, np.ones(3), True)
                em.recommend_positions(users, offsets, items)
                em.recommend_end()
            finally:
                em.close()
        names = lw.names()
    for k in ("rec_score_kernel", "rec_exclude_kernel", "rec_position_kernel", "rec_position_sum_kernel"):
        assert k in names, (k, sorted(names))


def test_refusals(hip):
    data, params = problem(50, 60, 3, 4, 4, 1, 400, seed=2)
    em = context(hip, data, params, 50, 60, 3)
    E = hip._lib.HipLibraryError
    try:
        with pytest.raises(E, match="recommend_begin") as e:       # no session
            em.recommend_positions([0], [0, 1], [3])
        assert e.value.code == hip._lib.E_INVALID
        em.recommend_begin(np.ones(3))
        with pytest.raises(E, match="recommend_add") as e:         # no slot added
            em.recommend_positions([0], [0, 1], [3])
        assert e.value.code == hip._lib.E_INVALID
        em.recommend_add()
        for users, off, items in (([50], [0, 1], [3]), ([-1], [0, 1], [3]), ([0], [0, 1], [60]), ([0], [0, 1], [-2]),
                                  ([0, 1], [1, 1, 2], [3, 4]), ([0, 1, 2], [0, 2, 1, 3], [1, 2, 3])):
            with pytest.raises(E) as e:
                em.recommend_positions(users, off, items)
            assert e.value.code == hip._lib.E_INVALID, (users, off, items)
        pos, cand = em.recommend_positions([0, 1], [0, 0, 0], np.zeros(0, dtype=np.int32))   # nothing to rank
        assert len(pos) == 0 and len(cand) == 2
        em.recommend_end()
    finally:
        em.close()
