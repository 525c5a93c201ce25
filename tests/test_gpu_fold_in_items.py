"""Fold-in of new items on the device (mmsbm_hip_fold_in_items, mmsbm_hip_recommend_add_items, HipEM.fold_in_items /
recommend_add_items, MMSBM.fold_in_items / recommend_with_new_items) against the oracle's M-step and the numpy
restatement of test_fold_in_items_cpu.py.

One iteration from a given eta0 agrees with the oracle's eta update within 1e-12; 100 iterations agree with the
restatement element-wise within 1e-9.  What the device promises beyond that -- item fold-in bitwise equal to user
fold-in on the transposed problem, an item's eta bitwise the same whatever the other items of the request, the slot
count or the side layout, no change to any slot or session, training items' scores unchanged by an extended catalogue --
is checked bit for bit.
"""
import numpy as np
import pandas as pd
import pytest

from conftest import assert_elementwise
from oracle import mmsbm_oracle as orc
from test_fold_in_items_cpu import restate_fold_items
from test_gpu_recommend import check_rows, context, hip, problem  # noqa: F401  (hip: the fixture)
from test_recommend_cpu import restate_scores, seen_items

pytestmark = pytest.mark.gpu


def new_item_rows(degrees, U, R, seed):
    """Rows [user, new item, rating] of new items 0 .. len(degrees)-1, item j with degrees[j] rows, shuffled."""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(len(degrees)), degrees)
    rows = np.stack([rng.integers(0, U, len(i)), i, rng.integers(0, R, len(i))], 1)
    return rows[rng.permutation(len(rows))]


def rows_of(rows, items):
    """The rows of `items` (in that order, renumbered 0 ..), each item's rows in their order in `rows`."""
    out = []
    for b, j in enumerate(items):
        r = rows[rows[:, 1] == j].copy()
        r[:, 1] = b
        out.append(r)
    return np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)


GRID = [  # (K, L, R, S, U, I, degrees, swap) -- test_gpu_fold_in.GRID with the roles of K and L exchanged
    (3, 2, 2, 1, 60, 50, [1, 2, 3, 5, 8, 13, 40, 100], 0),
    (20, 20, 5, 2, 400, 300, [1, 3, 10, 30, 51, 52, 200, 1000], 0),      # both forms (the LDS one: d <= 51 at L = 20)
    (4, 1, 3, 1, 40, 30, [1, 2, 7, 300], 0),
    (3, 80, 5, 2, 50, 40, [1, 5, 12, 13, 60], 0),                        # L > 64, skinny K
    (33, 7, 10, 1, 70, 60, [0, 1, 4, 9, 200], 1),                        # swapped; an item without rows
    (10, 20, 5, 1, 500, 30, [20_000, 3, 1], 0),                          # one item with 20k rows: the streamed form
    (5, 200, 3, 1, 30, 20, [1, 5, 6, 30], 0),
]


@pytest.mark.parametrize("case", GRID, ids=[f"K{c[0]}L{c[1]}R{c[2]}S{c[3]}sw{c[7]}" for c in GRID])
def test_parity_grid(hip, case):
    K, L, R, S, U, I, degrees, swap = case
    data, params = problem(U, I, R, K, L, S, 20 * (U + I), seed=K + L + S)
    rows = new_item_rows(degrees, U, R, seed=L)
    n_new = len(degrees)
    e0 = np.random.default_rng(7).random((n_new, L)) + 0.05
    em = context(hip, data, params, U, I, R, swap=swap)
    try:
        assert em.swapped == bool(swap)
        got = []
        for s in range(S):
            em.select(s)
            one, it1 = em.fold_in_items(rows, n_new, 1, eta0=e0)
            hund, it100 = em.fold_in_items(rows, n_new, 100)
            tolled, it_tol = em.fold_in_items(rows, n_new, 300, tol=1e-7)
            got.append((one, it1, hund, it100, tolled, it_tol))
    finally:
        em.close()
    d = np.bincount(rows[:, 1], minlength=n_new)
    seen = d > 0
    for (one, it1, hund, it100, tolled, it_tol), (theta, _, pr) in zip(got, params):
        want = orc.normalize_with_d(orc.update_coefficients(rows, theta, e0, pr)[1][seen], d[seen])
        np.testing.assert_allclose(one[seen], want, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(one[~seen], e0[~seen])
        assert (it1 == seen).all() and (it100 == 100 * seen).all()
        ref, _ = restate_fold_items(rows, n_new, theta, pr, 100)
        assert_elementwise(hund, ref, "100 iterations")
        ref_t, ref_it = restate_fold_items(rows, n_new, theta, pr, 300, tol=1e-7)
        np.testing.assert_array_equal(it_tol, ref_it)
        assert_elementwise(tolled, ref_t, "tol")
        assert (hund[~seen] == 1.0 / L).all()


@pytest.mark.parametrize("K,L,swap", [(12, 7, 0), (5, 40, 0), (80, 3, 1), (20, 20, 0)])
def test_transposition_identity(hip, K, L, swap):
    U, I, R = 150, 200, 4
    data, params = problem(U, I, R, K, L, 1, 3000, seed=K + L)
    rows = new_item_rows([1, 2, 9, 40, 300, 0], U, R, seed=K)
    e0 = np.random.default_rng(3).random((6, L))
    theta, eta, pr = params[0]
    em = context(hip, data, params, U, I, R, swap=swap)
    try:
        items = [em.fold_in_items(rows, 6, 60), em.fold_in_items(rows, 6, 200, tol=1e-8, eta0=e0)]
    finally:
        em.close()
    tp = [(eta, theta, np.ascontiguousarray(pr.transpose(1, 0, 2)))]
    tr = context(hip, np.ascontiguousarray(data[:, [1, 0, 2]]), tp, I, U, R, swap=swap)
    try:
        t_rows = np.ascontiguousarray(rows[:, [1, 0, 2]])
        users = [tr.fold_in(t_rows, 6, 60), tr.fold_in(t_rows, 6, 200, tol=1e-8, theta0=e0)]
    finally:
        tr.close()
    for (a, ai), (b, bi) in zip(items, users):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(ai, bi)


def test_request_independence(hip):
    K, L, R, U, I = 12, 20, 5, 300, 200
    data, params = problem(U, I, R, K, L, 3, 5000, seed=3)
    degrees = np.random.default_rng(4).integers(1, 120, 90)
    degrees[7] = 3000
    rows = new_item_rows(degrees, U, R, seed=5)
    n = len(degrees)
    em = context(hip, data, params, U, I, R)
    try:
        em.select(1)
        every, it_every = em.fold_in_items(rows, n, 100, tol=1e-9)
        assert em.get_option("fold_in_ms") > 0
        perm = np.random.default_rng(6).permutation(n)
        p_t, p_it = em.fold_in_items(rows_of(rows, perm), n, 100, tol=1e-9)
        sub = np.array([7, 3, 50, 89])
        s_t, s_it = em.fold_in_items(rows_of(rows, sub), len(sub), 100, tol=1e-9)
        parts = [np.arange(0, 30), np.arange(30, 31), np.arange(31, n)]
        split = [em.fold_in_items(rows_of(rows, p), len(p), 100, tol=1e-9)[0] for p in parts]
    finally:
        em.close()
    one = context(hip, data, [params[1]], U, I, R)                      # one slot instead of three
    try:
        o_t, o_it = one.fold_in_items(rows, n, 100, tol=1e-9)
    finally:
        one.close()
    np.testing.assert_array_equal(p_t, every[perm])
    np.testing.assert_array_equal(p_it, it_every[perm])
    np.testing.assert_array_equal(s_t, every[sub])
    np.testing.assert_array_equal(s_it, it_every[sub])
    np.testing.assert_array_equal(np.concatenate(split), every)
    np.testing.assert_array_equal(o_t, every)
    np.testing.assert_array_equal(o_it, it_every)


def test_swapped_context_is_bitwise_equal(hip):
    for K, L in ((7, 12), (40, 5), (3, 80)):
        U, I, R = 200, 150, 4
        data, params = problem(U, I, R, K, L, 1, 3000, seed=L)
        rows = new_item_rows([1, 2, 9, 40, 300], U, R, seed=K)
        out = []
        for swap in (0, 1):
            em = context(hip, data, params, U, I, R, swap=swap)
            try:
                assert em.swapped == bool(swap)
                out.append(em.fold_in_items(rows, 5, 50))
            finally:
                em.close()
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1], out[1][1])


def test_no_side_effects(hip):
    U, I, R, K, L = 300, 200, 5, 8, 10
    data, params = problem(U, I, R, K, L, 2, 4000, seed=13)
    rows = new_item_rows([3, 30, 500], U, R, seed=1)
    w = np.arange(1.0, R + 1)
    test = data[:500]

    def session(em, fold):
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(2)]
        em.predict_begin(test, w)
        em.select(0).predict_add()
        em.recommend_begin(w, True)
        em.select(0).recommend_add()
        if fold:
            em.select(1).fold_in_items(rows, 3, 100)
            em.select(0).fold_in_items(rows, 3, 10, tol=1e-3)
        rec = em.recommend_query(np.arange(U), 5)
        em.recommend_end()
        em.select(1).predict_add()
        mat, raw = em.predict_finish()
        after = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(2)]
        em.iterate(3)
        moved = [em.select(s).get_params() for s in range(2)]
        return before, after, rec, mat, raw, moved

    runs = []
    for fold in (True, False):
        em = context(hip, data, params, U, I, R)
        try:
            runs.append(session(em, fold))
        finally:
            em.close()
    (b1, a1, rec1, mat1, raw1, mv1), (b2, a2, rec2, mat2, raw2, mv2) = runs
    for x, y in zip(b1, a1):
        for a, b in zip(x, y):
            np.testing.assert_array_equal(a, b)
    for a, b in zip(rec1, rec2):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(mat1, mat2)
    np.testing.assert_array_equal(raw1, raw2)
    for x, y in zip(mv1, mv2):
        for a, b in zip(x, y):
            np.testing.assert_array_equal(a, b)


# ---- the extended catalogue -----------------------------------------------------------------------------------------
def full_scores(got, n_items):
    """{item: score} of every row of a query that returned all its candidates."""
    items, scores, counts = got
    out = []
    for b in range(len(counts)):
        row = np.full(n_items, np.nan)
        row[items[b, :counts[b]]] = scores[b, :counts[b]]
        out.append(row)
    return np.array(out)


@pytest.mark.parametrize("K,L,swap", [(6, 9, 0), (12, 5, 0), (20, 20, 1)])   # y = eta W^T (K <= L) and y = eta (K > L)
def test_extended_catalogue(hip, K, L, swap):
    U, I, R, S, n_new = 120, 300, 5, 2, 25
    data, params = problem(U, I, R, K, L, S, 4000, seed=K * L)
    rng = np.random.default_rng(K)
    new_eta = rng.random((S, n_new, L))
    copies = {3: 17, 11: 17, 20: 250}                                 # new item j gets training item t's eta rows
    for j, t in copies.items():
        new_eta[:, j] = [params[s][1][t] for s in range(S)]
    seen_new = [rng.choice(U, rng.integers(0, 6), replace=True) for _ in range(n_new)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in seen_new])]).astype(np.int64)
    seen_users = np.concatenate(seen_new).astype(np.int32)
    w = np.arange(1.0, R + 1)
    users = np.arange(U, dtype=np.int32)
    NI = I + n_new
    em = context(hip, data, params, U, I, R, swap=swap)
    try:
        out = {}
        for excl in (False, True):
            em.recommend_begin(w, excl)
            for s in range(S):
                em.select(s).recommend_add()
            before = em.recommend_query(users, I)
            em.recommend_add_items(new_eta, (off, seen_users))
            after = em.recommend_query(users, NI)
            sample = np.array([0, 5, 77, 119], dtype=np.int32)
            thetas = np.stack([em.select(s).get_params()[0][sample] for s in range(S)])
            via_theta = em.recommend_query_theta(thetas, 40)
            pos_items = after[0][:, :30]
            n_pos = after[2].clip(max=30)
            p_off = np.concatenate([[0], np.cumsum(n_pos)]).astype(np.int64)
            p_items = np.concatenate([pos_items[b, :n_pos[b]] for b in range(U)])
            positions, cand = em.recommend_positions(users, p_off, p_items)
            assert em.get_option("recommend_ms") > 0
            em.recommend_end()
            out[excl] = (before, after, via_theta, positions, cand, p_off, n_pos, sample)
        em.recommend_begin(w, False)                                    # without seen lists nothing is left out
        for s in range(S):
            em.select(s).recommend_add()
        em.recommend_add_items(new_eta)
        plain = em.recommend_query(users, NI)
        em.recommend_end()
    finally:
        em.close()
    ext = [(t, np.vstack([e, new_eta[s]]), p) for s, (t, e, p) in enumerate(params)]
    ref = restate_scores(ext, users, NI, w)
    train_seen = seen_items(data, U)
    new_seen = [set() for _ in range(U)]
    for j, us in enumerate(seen_new):
        for u in us.tolist():
            new_seen[u].add(I + j)
    assert (plain[2] == NI).all()
    check_rows(plain, ref, np.arange(U), NI)
    for excl, (before, after, via_theta, positions, cand, p_off, n_pos, sample) in out.items():
        seen = [(train_seen[u] if excl else set()) | new_seen[u] for u in range(U)]
        check_rows(after, ref, np.arange(U), NI, seen, users)
        # training items' scores bitwise as before the call
        a, b = full_scores(before, NI), full_scores(after, NI)
        both = ~np.isnan(a[:, :I])
        np.testing.assert_array_equal(a[:, :I][both], b[:, :I][both])
        assert ((a[:, :I][both]) == b[:, :I][both]).all() and both.sum() > 0
        # a copy of training item t's eta scores bitwise like t; the tie goes to t (the smaller id)
        for j, t in copies.items():
            for u in range(U):
                if not np.isnan(b[u, t]) and not np.isnan(b[u, I + j]):
                    assert b[u, t] == b[u, I + j]
                    row = after[0][u].tolist()
                    assert row.index(t) < row.index(I + j)
        # positions and candidates agree with the query over the extended catalogue
        assert (cand == after[2]).all()
        want = np.concatenate([np.arange(1, k + 1) for k in n_pos]).astype(np.int32)
        np.testing.assert_array_equal(positions, want)
        # caller theta rows rank the extended catalogue as well (no exclusion for caller rows)
        check_rows(via_theta, ref[sample], np.arange(len(sample)), 40)
        assert (via_theta[0] >= I).any()


def test_extended_query_theta_is_bitwise_recommend_query(hip):
    U, I, R, K, L, S = 200, 400, 5, 10, 6, 2
    data, params = problem(U, I, R, K, L, S, 5000, seed=4)
    new_eta = np.random.default_rng(5).random((S, 30, L))
    w = np.arange(1.0, R + 1)
    users = np.array([3, 50, 199, 0], dtype=np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        em.recommend_begin(w, False)
        for s in range(S):
            em.select(s).recommend_add()
        em.recommend_add_items(new_eta)
        want = em.recommend_query(users, 50)
        thetas = np.stack([em.select(s).get_params()[0][users] for s in range(S)])
        got = em.recommend_query_theta(thetas, 50)
        seen = (np.array([0, 2, 2, 3, 3], dtype=np.int64), np.array([I + 4, 7, I + 29], dtype=np.int32))
        excl = em.recommend_query_theta(thetas, 50, seen)
        em.recommend_end()
    finally:
        em.close()
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)
    assert I + 4 not in excl[0][0] and 7 not in excl[0][2] and I + 29 not in excl[0][2]


# ---- the host class --------------------------------------------------------------------------------------------------
def test_end_to_end_with_string_labels(hip):
    rng = np.random.default_rng(21)
    n_obs = 4000
    df = pd.DataFrame({"users": [f"user{x}" for x in rng.integers(0, 150, n_obs)],
                       "items": [f"film-{x}" for x in rng.integers(0, 400, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 5, iterations=30, sampling=3, seed=4)
    model.fit(df, silent=True)
    people = sorted(set(df["users"]))
    new = pd.DataFrame({"users": [people[3], people[10], people[50], people[7], "nobody", people[3], people[99]],
                        "items": ["zoe", "al", "zoe", "new-3", "al", "al", "bo"],
                        "ratings": [5, 1, 4, 2, 3, 3, 5]})
    etas = model.fold_in_items(new, iterations=100)
    it = model.fold_in_items_iterations
    enc = model.data_handler
    ul, il = enc.user_labels(), enc.item_labels()
    labels = ["zoe", "al", "new-3", "bo"]
    kept = new[new["users"] != "nobody"]
    rows = np.stack([[ul.index(u) for u in kept["users"]], [labels.index(i) for i in kept["items"]],
                     [enc.rating_labels().index(str(r)) for r in kept["ratings"]]], 1)
    for e, res in zip(etas, model.results):
        assert e.index.tolist() == labels
        ref, _ = restate_fold_items(rows, 4, res["theta"], res["pr"], 100)
        assert_elementwise(e.to_numpy(), ref, "MMSBM.fold_in_items")
    assert it.shape == (4, 3) and (it.to_numpy() == 100).all()
    model.predict(df.iloc[:300])                                       # parameters uploaded again, not resident
    rec = model.recommend_with_new_items(new, n=8)
    assert rec["users"].tolist() == [u for u in ul for _ in range(8)]
    mine = set(zip(kept["users"], kept["items"])) | set(zip(df["users"], df["items"]))
    assert not any((u, i) in mine for u, i in zip(rec["users"], rec["items"]))
    assert set(rec["items"]) & set(labels)
    all_items = il + labels
    params = [(r["theta"], np.vstack([r["eta"], e.to_numpy()]), r["pr"]) for e, r in zip(etas, model.results)]
    ref = restate_scores(params, np.arange(len(ul)), len(all_items), np.asarray(model.ratings, dtype=np.float64))
    for b, u in enumerate(ul[:40]):
        sub = rec[rec["users"] == u]
        got = sub["score"].to_numpy(float)
        want = ref[b, [all_items.index(i) for i in sub["items"]]]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * np.abs(ref).max())
        assert (np.diff(got) <= 0).all()
    with pytest.raises(ValueError, match="training items"):
        model.recommend_with_new_items(pd.DataFrame({"users": [people[0]], "items": [il[0]], "ratings": [3]}))


def test_full_size_c3(hip):
    U, I, R, K = 100_000, 20_000, 5, 20
    data = orc.synthetic_triples(1_000_000, U, I, R, seed=0)
    U = int(data[:, 0].max()) + 1
    rng = np.random.default_rng(0)
    params = [(rng.random((U, K)), rng.random((I, K)), orc.normalize_with_self(rng.random((K, K, R))))]
    em = context(hip, data, params, U, I, R)
    try:
        eta, iters = em.fold_in_items(data, I, 100)
        w = np.arange(1.0, R + 1)
        em.recommend_begin(w, True)
        em.recommend_add()
        users = np.arange(U, dtype=np.int32)
        plain = em.recommend_query(users, 10)
        none = (np.zeros(U + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
        cand = em.recommend_positions(users, *none)[1]
        new_eta = rng.random((1, 2000, K))
        em.recommend_add_items(new_eta)
        wide = em.recommend_query(users, 10)
        cand_wide = em.recommend_positions(users, *none)[1]
        em.recommend_end()
    finally:
        em.close()
    d = np.bincount(data[:, 1], minlength=I)
    assert (iters == 100 * (d > 0)).all()
    pos = np.random.default_rng(2).choice(np.flatnonzero(d > 0), 256, replace=False)
    ref, _ = restate_fold_items(rows_of(data, pos), len(pos), params[0][0], params[0][2], 100)
    assert_elementwise(eta[pos], ref, "C3")
    assert (cand_wide == cand + 2000).all() and (wide[2] == 10).all()
    assert (wide[1][:, 0] >= plain[1][:, 0]).all()
    same = wide[0][:, 0] < I                                            # the best is still a training item
    assert (wide[0][same, 0] == plain[0][same, 0]).all() and (wide[1][same, 0] == plain[1][same, 0]).all()


def test_bad_arguments(hip):
    data, params = problem(50, 60, 3, 4, 4, 1, 400, seed=2)
    em = context(hip, data, params, 50, 60, 3)
    try:
        for rows, n_new in (([[50, 0, 0]], 2), ([[0, 2, 0]], 2), ([[0, 0, 3]], 2)):
            with pytest.raises(hip._lib.HipLibraryError):
                em.fold_in_items(np.array(rows), n_new, 5)
        with pytest.raises(hip._lib.HipLibraryError):
            em.fold_in_items(np.array([[0, 0, 0]]), 1, -1)
        with pytest.raises(hip._lib.HipLibraryError, match="negative n_new"):
            hip._lib.call("mmsbm_hip_fold_in_items", em._h, 0, None, None, None, -1, 5, -1.0, None, None, None)
        eta, iters = em.fold_in_items(np.zeros((0, 3), dtype=np.int64), 3, 5)
        assert (eta == 0.25).all() and (iters == 0).all()
        w = np.ones(3)
        em.recommend_begin(w, False)
        with pytest.raises(hip._lib.HipLibraryError, match="before any recommend_add"):
            em.recommend_add_items(np.ones((0, 1, 4)))                # (the host wrapper: no block per slot yet)
        em.recommend_add()
        with pytest.raises(hip._lib.HipLibraryError, match="negative"):
            hip._lib.call("mmsbm_hip_recommend_add_items", em._h, -1, None, None, None)
        with pytest.raises(hip._lib.HipLibraryError, match="decrease"):
            em.recommend_add_items(np.ones((1, 2, 4)), (np.array([0, 2, 1]), np.array([0])))
        with pytest.raises(hip._lib.HipLibraryError, match="out of range"):
            em.recommend_add_items(np.ones((1, 2, 4)), (np.array([0, 1, 1]), np.array([50])))
        em.recommend_add_items(np.ones((1, 0, 4)))                     # n_new == 0 changes nothing
        assert em.recommend_query(np.array([0]), 100)[2][0] == 60
        em.recommend_add_items(np.ones((1, 2, 4)), (np.array([0, 1, 1]), np.array([0])))
        assert em.recommend_query(np.array([0, 1]), 100)[2].tolist() == [61, 62]
        with pytest.raises(hip._lib.HipLibraryError, match="already"):
            em.recommend_add_items(np.ones((1, 2, 4)))
        with pytest.raises(hip._lib.HipLibraryError, match="after recommend_add_items"):
            em.recommend_add()
        with pytest.raises(hip._lib.HipLibraryError, match="out of range"):
            em.recommend_positions(np.array([0]), np.array([0, 1]), np.array([62]))
        pos, cand = em.recommend_positions(np.array([0, 1]), np.array([0, 1, 2]), np.array([60, 61]))
        assert pos[0] == 0 and pos[1] >= 1 and cand.tolist() == [61, 62]       # (user 0 has rated new item 0)
        em.recommend_end()
    finally:
        em.close()
    data, params = problem(20, 30, 3, 2, 1100, 1, 200, seed=3)         # L beyond MMSBM_HIP_FOLD_IN_MAX_K
    em = context(hip, data, params, 20, 30, 3)
    try:
        with pytest.raises(hip._lib.HipLibraryError, match="beyond"):
            em.fold_in_items(np.array([[0, 0, 0]]), 1, 5)
    finally:
        em.close()
