"""Fold-in on the device (mmsbm_hip_fold_in, mmsbm_hip_recommend_query_theta, HipEM.fold_in, MMSBM.fold_in /
recommend_new) against the oracle's M-step and the numpy restatement of test_fold_in_cpu.py.

One iteration from a given theta0 agrees with the oracle's theta update within 1e-12; 100 iterations agree with the
restatement element-wise within 1e-9.  What the kernels promise beyond that -- a user's theta bitwise the same whatever
the other users of the request, the slot count or the side layout, no change to any slot or session -- is checked bit
for bit.
"""
import numpy as np
import pandas as pd
import pytest

from conftest import assert_elementwise
from oracle import mmsbm_oracle as orc
from test_fold_in_cpu import restate_fold
from test_gpu_recommend import LaunchWindow, check_rows, context, hip, problem  # noqa: F401  (hip: the fixture)
from test_recommend_cpu import restate_scores

pytestmark = pytest.mark.gpu


def new_rows(degrees, I, R, seed):
    """Rows of new users 0 .. len(degrees)-1, user u with degrees[u] rows, in a shuffled order."""
    rng = np.random.default_rng(seed)
    u = np.repeat(np.arange(len(degrees)), degrees)
    rows = np.stack([u, rng.integers(0, I, len(u)), rng.integers(0, R, len(u))], 1)
    return rows[rng.permutation(len(rows))]


def rows_of(rows, users):
    """The rows of `users` (in that order, renumbered 0 ..), each user's rows in their order in `rows`."""
    out = []
    for b, u in enumerate(users):
        r = rows[rows[:, 0] == u].copy()
        r[:, 0] = b
        out.append(r)
    return np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)


GRID = [  # (K, L, R, S, U, I, degrees, swap)
    (2, 3, 2, 1, 50, 60, [1, 2, 3, 5, 8, 13, 40, 100], 0),
    (20, 20, 5, 2, 300, 400, [1, 3, 10, 30, 51, 52, 200, 1000], 0),      # both forms (the LDS one: d <= 51 at K = 20)
    (1, 4, 3, 1, 30, 40, [1, 2, 7, 300], 0),
    (80, 3, 5, 2, 40, 50, [1, 5, 12, 13, 60], 0),                        # K > 64, skinny L
    (7, 33, 10, 1, 60, 70, [0, 1, 4, 9, 200], 1),                        # swapped; a user without rows
    (20, 10, 5, 1, 30, 500, [20_000, 3, 1], 0),                          # one user with 20k rows: the streamed form
    (200, 5, 3, 1, 20, 30, [1, 5, 6, 30], 0),
]


@pytest.mark.parametrize("case", GRID, ids=[f"K{c[0]}L{c[1]}R{c[2]}S{c[3]}sw{c[7]}" for c in GRID])
def test_parity_grid(hip, case):
    K, L, R, S, U, I, degrees, swap = case
    data, params = problem(U, I, R, K, L, S, 20 * (U + I), seed=K + L + S)
    rows = new_rows(degrees, I, R, seed=K)
    n_new = len(degrees)
    t0 = np.random.default_rng(7).random((n_new, K)) + 0.05
    em = context(hip, data, params, U, I, R, swap=swap)
    try:
        assert em.swapped == bool(swap)
        got = []
        for s in range(S):
            em.select(s)
            one, it1 = em.fold_in(rows, n_new, 1, theta0=t0)
            hund, it100 = em.fold_in(rows, n_new, 100)
            tolled, it_tol = em.fold_in(rows, n_new, 300, tol=1e-7)
            got.append((one, it1, hund, it100, tolled, it_tol))
    finally:
        em.close()
    d = np.bincount(rows[:, 0], minlength=n_new)
    seen = d > 0
    for (one, it1, hund, it100, tolled, it_tol), (_, eta, pr) in zip(got, params):
        want = orc.normalize_with_d(orc.update_coefficients(rows, t0, eta, pr)[0][seen], d[seen])
        np.testing.assert_allclose(one[seen], want, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(one[~seen], t0[~seen])
        assert (it1 == seen).all() and (it100 == 100 * seen).all()
        ref, _ = restate_fold(rows, n_new, eta, pr, 100)
        assert_elementwise(hund, ref, "100 iterations")
        ref_t, ref_it = restate_fold(rows, n_new, eta, pr, 300, tol=1e-7)
        np.testing.assert_array_equal(it_tol, ref_it)
        assert_elementwise(tolled, ref_t, "tol")
        assert (hund[~seen] == 1.0 / K).all()


def test_request_independence(hip):
    K, L, R, U, I = 20, 12, 5, 200, 300
    data, params = problem(U, I, R, K, L, 3, 5000, seed=3)
    degrees = np.random.default_rng(4).integers(1, 120, 90)
    degrees[7] = 3000
    rows = new_rows(degrees, I, R, seed=5)
    n = len(degrees)
    em = context(hip, data, params, U, I, R)
    try:
        em.select(1)
        every, it_every = em.fold_in(rows, n, 100, tol=1e-9)
        assert em.get_option("fold_in_ms") > 0
        perm = np.random.default_rng(6).permutation(n)
        p_t, p_it = em.fold_in(rows_of(rows, perm), n, 100, tol=1e-9)
        sub = np.array([7, 3, 50, 89])
        s_t, s_it = em.fold_in(rows_of(rows, sub), len(sub), 100, tol=1e-9)
        parts = [np.arange(0, 30), np.arange(30, 31), np.arange(31, n)]
        split = [em.fold_in(rows_of(rows, p), len(p), 100, tol=1e-9)[0] for p in parts]
    finally:
        em.close()
    one = context(hip, data, [params[1]], U, I, R)                      # one slot instead of three
    try:
        o_t, o_it = one.fold_in(rows, n, 100, tol=1e-9)
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
    for K, L in ((12, 7), (5, 40), (80, 3)):
        U, I, R = 150, 200, 4
        data, params = problem(U, I, R, K, L, 1, 3000, seed=K)
        rows = new_rows([1, 2, 9, 40, 300], I, R, seed=L)
        out = []
        for swap in (0, 1):
            em = context(hip, data, params, U, I, R, swap=swap)
            try:
                assert em.swapped == bool(swap)
                out.append(em.fold_in(rows, 5, 50))
            finally:
                em.close()
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1], out[1][1])


def test_no_side_effects(hip):
    U, I, R, K, L = 200, 300, 5, 10, 8
    data, params = problem(U, I, R, K, L, 2, 4000, seed=13)
    rows = new_rows([3, 30, 500], I, R, seed=1)
    w = np.arange(1.0, R + 1)
    test = data[:500]

    def session(em, fold):
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(2)]
        em.predict_begin(test, w)
        em.select(0).predict_add()
        em.recommend_begin(w, True)
        em.select(0).recommend_add()
        if fold:
            em.select(1).fold_in(rows, 3, 100)
            em.select(0).fold_in(rows, 3, 10, tol=1e-3)
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
    for x, y in zip(mv1, mv2):                                        # the following iterate: bitwise the same
        for a, b in zip(x, y):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("K,L", [(6, 9), (20, 20), (12, 5)])         # x = theta (K <= L) and x = theta W (K > L)
def test_query_theta_is_bitwise_recommend_query(hip, K, L):
    U, I, R, S = 300, 700, 5, 2
    data, params = problem(U, I, R, K, L, S, 6000, seed=K * L)
    w = np.arange(1.0, R + 1)
    users = np.random.default_rng(2).choice(U, 120, replace=False)
    t = data[np.argsort(data[:, 0], kind="stable")]
    em = context(hip, data, params, U, I, R)
    try:
        em.iterate(2)
        thetas = np.stack([em.select(s).get_params()[0][users] for s in range(S)])
        em.recommend_begin(w, True)
        for s in range(S):
            em.select(s).recommend_add()
        want = em.recommend_query(users, 15)
        seen = [np.unique(t[t[:, 0] == u, 1]) for u in users]
        off = np.concatenate([[0], np.cumsum([len(x) for x in seen])]).astype(np.int64)
        got = em.recommend_query_theta(thetas, 15, (off, np.concatenate(seen)))
        em.recommend_begin(w, False)
        for s in range(S):
            em.select(s).recommend_add()
        want_all = em.recommend_query(users, 15)
        got_all = em.recommend_query_theta(thetas, 15)
        em.recommend_end()
    finally:
        em.close()
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(want_all, got_all):
        np.testing.assert_array_equal(a, b)


def test_end_to_end_with_string_labels(hip):
    rng = np.random.default_rng(21)
    n_obs = 4000
    df = pd.DataFrame({"users": [f"user{x}" for x in rng.integers(0, 150, n_obs)],
                       "items": [f"film-{x}" for x in rng.integers(0, 400, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 5, iterations=30, sampling=3, seed=4)
    model.fit(df, silent=True)
    films = sorted(set(df["items"]))
    new = pd.DataFrame({"users": ["zoe", "al", "zoe", "user3", "al", "zoe", "bo"],
                        "items": [films[3], films[10], films[50], films[7], "film-unknown", films[3], films[99]],
                        "ratings": [5, 1, 4, 2, 3, 3, 5]})
    thetas = model.fold_in(new, iterations=100)
    it = model.fold_in_iterations
    enc = model.data_handler
    il = enc.item_labels()
    labels = ["zoe", "al", "user3", "bo"]
    kept = new[new["items"] != "film-unknown"]
    rows = np.stack([[labels.index(u) for u in kept["users"]], [il.index(i) for i in kept["items"]],
                     [enc.rating_labels().index(str(r)) for r in kept["ratings"]]], 1)
    for t, res in zip(thetas, model.results):
        assert t.index.tolist() == labels
        ref, _ = restate_fold(rows, 4, res["eta"], res["pr"], 100)
        assert_elementwise(t.to_numpy(), ref, "MMSBM.fold_in")
    assert it.shape == (4, 3) and (it.to_numpy() == 100).all()
    model.predict(df.iloc[:300])                                       # parameters uploaded again, not resident
    rec = model.recommend_new(new, n=6)
    assert rec["users"].tolist() == [u for u in labels for _ in range(6)]
    mine = set(zip(kept["users"], kept["items"]))
    assert not any((u, i) in mine for u, i in zip(rec["users"], rec["items"]))
    params = [(np.asarray(t.to_numpy()), r["eta"], r["pr"]) for t, r in zip(thetas, model.results)]
    ref = restate_scores(params, np.arange(4), len(il), np.asarray(model.ratings, dtype=np.float64))
    for b, u in enumerate(labels):
        sub = rec[rec["users"] == u]
        got = sub["score"].to_numpy(float)
        want = ref[b, [il.index(i) for i in sub["items"]]]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * np.abs(ref).max())
        assert (np.diff(got) <= 0).all()


def test_full_size_c3(hip):
    U, I, R, K = 100_000, 20_000, 5, 20
    data = orc.synthetic_triples(1_000_000, U, I, R, seed=0)
    U = int(data[:, 0].max()) + 1
    rng = np.random.default_rng(0)
    params = [(rng.random((U, K)), rng.random((I, K)), orc.normalize_with_self(rng.random((K, K, R))))]
    em = context(hip, data, params, U, I, R)
    try:
        theta, iters = em.fold_in(data, U, 100)
    finally:
        em.close()
    d = np.bincount(data[:, 0], minlength=U)
    assert (iters == 100 * (d > 0)).all()
    pos = np.random.default_rng(2).choice(np.flatnonzero(d > 0), 256, replace=False)
    ref, _ = restate_fold(rows_of(data, pos), len(pos), params[0][1], params[0][2], 100)
    assert_elementwise(theta[pos], ref, "C3")


def test_every_fold_in_kernel_is_launched(hip):
    with LaunchWindow() as lw:
        for K in (3, 6, 12, 20, 40, 80, 200, 300, 600):               # every (G, NT); each with both forms
            data, params = problem(20, 30, 3, K, 2, 1, 200, seed=K)
            em = context(hip, data, params, 20, 30, 3)
            try:
                em.fold_in(new_rows([1, 1024 // K + 1], 30, 3, seed=K), 2, 3)
            finally:
                em.close()
        names = lw.names()
    assert "fold_v_kernel" in names, sorted(names)
    assert len({n for n in names if n.startswith("fold_kernel<")}) == 18, sorted(names)


def test_bad_arguments(hip):
    data, params = problem(50, 60, 3, 4, 4, 1, 400, seed=2)
    em = context(hip, data, params, 50, 60, 3)
    try:
        for rows, n_new in (([[2, 0, 0]], 2), ([[0, 60, 0]], 2), ([[0, 0, 3]], 2)):
            with pytest.raises(hip._lib.HipLibraryError):
                em.fold_in(np.array(rows), n_new, 5)
        with pytest.raises(hip._lib.HipLibraryError):
            em.fold_in(np.array([[0, 0, 0]]), 1, -1)
        theta, iters = em.fold_in(np.zeros((0, 3), dtype=np.int64), 3, 5)
        assert (theta == 0.25).all() and (iters == 0).all()
        em.recommend_begin(np.ones(3), False)
        em.recommend_add()
        with pytest.raises(hip._lib.HipLibraryError):
            em.recommend_query_theta(np.ones((1, 2, 4)), 3, (np.array([0, 1, 2]), np.array([0, 60])))
        with pytest.raises(ValueError):
            em.recommend_query_theta(np.ones((2, 2, 4)), 3)            # two theta blocks, one slot added
        em.recommend_end()
    finally:
        em.close()
