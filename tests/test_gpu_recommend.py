"""Top-N recommendation on the device (mmsbm_hip_recommend_*, HipEM.recommend_*, MMSBM.recommend) against the numpy
restatement of test_recommend_cpu.py: mean over restarts of oracle prod_dist, times the weights, lexsort on
(item, -score).

Scores agree within TOL x max|score|; the returned items agree outside the tie band: with tau = TOL x max|score| and
s* the restatement's n-th score, every item scoring above s* + tau is returned and none below s* - tau.  What the
kernels promise beyond that -- bitwise the same scores whatever the request, the launch shape or the side layout,
exact ties by item id, no change to any slot -- is checked bit for bit.  The band-free checks (mass ties, every
member of a tie group, scores compared by their bits) live in test_gpu_serving_exact.py, on models without rounding.
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
from oracle import mmsbm_oracle as orc
from test_recommend_cpu import restate_scores, seen_items

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402  (demangling + canonical kernel names, shared with the coverage report)

pytestmark = pytest.mark.gpu

TOL = 1e-12


class LaunchWindow:
    """Kernels this process launched between __enter__ and names(): the library appends its launch counts to the log
    whenever a context is destroyed, so read it after the contexts of the test are closed."""

    def __init__(self):
        self.path = os.environ.get("MMSBM_HIP_LAUNCH_LOG", "")

    def __enter__(self):
        self.pos = os.path.getsize(self.path) if self.path and os.path.exists(self.path) else 0
        return self

    def __exit__(self, *exc):
        return False

    def names(self):
        if not self.path:
            pytest.skip("launch log switched off (MMSBM_HIP_LAUNCH_LOG is empty)")
        with open(self.path) as fh:
            fh.seek(self.pos)
            rows = [ln.rstrip("\n").split("\t") for ln in fh]
        mine = [r[2] for r in rows if len(r) >= 4 and r[0] == str(os.getpid())]
        return {kernel_coverage.canon(n) for n in kernel_coverage.demangle(mine)} if mine else set()


@pytest.fixture(scope="module")
def hip():
    from mmsbm_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("-m gpu tests need a GPU: no HIP device visible (no CPU fallback exists)")
    import mmsbm_amd
    return mmsbm_amd


def problem(U, I, R, K, L, S, n_obs, seed):
    """Triples with every id inside (U, I, R) and S random parameter sets."""
    rng = np.random.default_rng(seed)
    data = np.stack([rng.integers(0, U, n_obs), rng.integers(0, I, n_obs), rng.integers(0, R, n_obs)], 1)
    params = [(rng.random((U, K)), rng.random((I, L)), orc.normalize_with_self(rng.random((K, L, R)))) for _ in range(S)]
    return data, params


def context(hip, data, params, U, I, R, swap=0):
    K, L = params[0][0].shape[1], params[0][1].shape[1]
    em = hip.HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=swap, slots=len(params))
    for s, p in enumerate(params):
        em.select(s).set_params(*p)
    return em


def run(em, n_slots, users, n, weights, exclude=True):
    em.recommend_begin(weights, exclude)
    for s in range(n_slots):
        em.select(s).recommend_add()
    out = em.recommend_query(users, n)
    em.recommend_end()
    return out


def check_rows(got, ref_scores, users_pos, n, seen=None, users=None):
    """got = (items, scores, counts) of the device for rows users_pos; ref_scores[j] = restatement scores of that row."""
    items, scores, counts = got
    for j, b in enumerate(users_pos):
        ref = ref_scores[j]
        tau = TOL * max(np.abs(ref).max(), 1e-300)
        cand = np.arange(len(ref))
        if seen is not None:
            cand = cand[~np.isin(cand, np.fromiter(seen[users[b]], dtype=np.int64, count=len(seen[users[b]])))]
        want = min(n, len(cand))
        assert counts[b] == want, (b, counts[b], want)
        it, sc = items[b, :want], scores[b, :want]
        assert (items[b, want:] == -1).all() and np.isneginf(scores[b, want:]).all()
        assert len(set(it.tolist())) == want and np.isin(it, cand).all()
        assert np.all(np.abs(sc - ref[it]) <= tau), np.abs(sc - ref[it]).max() / tau
        order = np.lexsort((it, -sc))                       # the device's own order: score desc, item asc
        assert (order == np.arange(want)).all()
        if want == 0:
            continue
        s_star = np.sort(ref[cand])[::-1][want - 1]
        above = cand[ref[cand] > s_star + tau]
        assert np.isin(above, it).all()
        assert (ref[it] >= s_star - tau).all()


GRID = [  # (K, L, R, S, U, I, n_obs, users checked against the restatement)
    (2, 3, 2, 1, 997, 1021, 20000, None),
    (20, 20, 5, 3, 1021, 997, 30000, 24),
    (50, 50, 10, 1, 3, 1021, 2000, None),
    (80, 80, 5, 3, 1, 997, 500, None),
    (5, 33, 10, 1, 997, 3, 1500, 40),
    (20, 20, 2, 1, 1, 5000, 3000, None),           # one user over 5,000 items: the items split across waves + merge
]


@pytest.mark.parametrize("case", GRID, ids=[f"K{c[0]}L{c[1]}R{c[2]}S{c[3]}U{c[4]}I{c[5]}" for c in GRID])
def test_parity_grid(hip, case):
    K, L, R, S, U, I, n_obs, sample = case
    data, params = problem(U, I, R, K, L, S, n_obs, seed=K * 7 + L + S)
    w = np.arange(1, R + 1, dtype=np.float64)
    users = np.arange(U, dtype=np.int32)
    pos = np.arange(U) if sample is None else np.random.default_rng(1).choice(U, sample, replace=False)
    ref = restate_scores(params, users[pos], I, w)
    seen = seen_items(data, U)
    em = context(hip, data, params, U, I, R)
    try:
        for exclude in (True, False):
            for n in sorted({1, 10, min(I, 1024), min(I + 5, 1024)}):
                got = run(em, S, users, n, w, exclude)
                check_rows(got, ref, pos, n, seen if exclude else None, users)
    finally:
        em.close()


def test_n_beyond_the_bound_is_refused(hip):
    data, params = problem(50, 60, 3, 4, 4, 1, 400, seed=2)
    em = context(hip, data, params, 50, 60, 3)
    try:
        em.recommend_begin(np.ones(3))
        em.recommend_add()
        with pytest.raises(hip._lib.HipLibraryError, match="1024") as e:
            em.recommend_query([0], 1025)
        assert e.value.code == hip._lib.E_UNSUPPORTED
        with pytest.raises(hip._lib.HipLibraryError):
            em.recommend_query([50], 3)                 # id out of range
        with pytest.raises(hip._lib.HipLibraryError, match="finite"):
            em.recommend_begin(np.array([1.0, np.nan, 2.0]))
        em.recommend_end()
    finally:
        em.close()


def test_exact_ties_come_in_item_order(hip):
    U, I, R = 40, 700, 4
    data, params = problem(U, I, R, 6, 9, 2, 3000, seed=5)
    for t, e, p in params:
        e[[17, 300, 699]] = e[5]
    em = context(hip, data, params, U, I, R)
    try:
        items, scores, counts = run(em, 2, np.arange(U), I, np.arange(1.0, R + 1), exclude=False)
    finally:
        em.close()
    for b in range(U):
        row = items[b].tolist()
        at = [row.index(i) for i in (5, 17, 300, 699)]
        assert at == list(range(at[0], at[0] + 4)), at
        assert len({scores[b, a] for a in at}) == 1


def test_request_independence_and_repeats(hip):
    U, I, R = 1021, 5000, 5                            # one user: the items split across waves; all users: no split
    data, params = problem(U, I, R, 20, 20, 2, 20000, seed=9)
    em = context(hip, data, params, U, I, R)
    try:
        w = np.arange(1.0, R + 1)
        em.recommend_begin(w, True)
        for s in range(2):
            em.select(s).recommend_add()
        every = em.recommend_query(np.arange(U), 10)
        again = em.recommend_query(np.arange(U), 10)
        sub = np.random.default_rng(3).choice(U, 77, replace=False)
        some = em.recommend_query(sub, 10)
        one = em.recommend_query([sub[5]], 10)
        assert em.get_option("recommend_ms") > 0        # device time of the last query
        em.recommend_end()
    finally:
        em.close()
    for a, b in zip(every, again):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(every, some):
        np.testing.assert_array_equal(a[sub], b)
    for a, b in zip(every, one):
        np.testing.assert_array_equal(a[sub[5:6]], b)


def test_swapped_context_and_uploaded_parameters_are_bitwise_equal(hip):
    U, I, R = 300, 800, 5
    data, params = problem(U, I, R, 12, 7, 2, 6000, seed=11)
    w = np.arange(1.0, R + 1)
    users = np.arange(U)
    em = context(hip, data, params, U, I, R, swap=0)
    try:
        em.iterate(3)                                   # resident slots, moved by the EM loop
        fitted = [em.select(s).get_params() for s in range(2)]
        resident = run(em, 2, users, 25, w)
    finally:
        em.close()
    for swap in (0, 1):
        other = context(hip, data, fitted, U, I, R, swap=swap)
        try:
            assert other.swapped == bool(swap)
            got = run(other, 2, users, 25, w)
        finally:
            other.close()
        for a, b in zip(resident, got):
            np.testing.assert_array_equal(a, b)


def test_no_side_effects(hip):
    U, I, R = 200, 300, 5
    data, params = problem(U, I, R, 10, 10, 3, 4000, seed=13)
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(3)]
        test = data[:500]
        em.predict_begin(test, np.arange(1.0, R + 1))
        em.select(0).predict_add()
        run(em, 3, np.arange(U), 10, np.arange(1.0, R + 1))   # a recommend session in the middle of a predict session
        em.select(1).predict_add()
        mat, raw = em.predict_finish()
        after = [em.select(s).get_params() for s in range(3)]
        em.predict_begin(test, np.arange(1.0, R + 1))
        em.select(0).predict_add()
        em.select(1).predict_add()
        mat2, raw2 = em.predict_finish()
    finally:
        em.close()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(mat, mat2)
    np.testing.assert_array_equal(raw, raw2)


def test_end_to_end_with_string_ids(hip):
    rng = np.random.default_rng(21)
    n_obs = 4000
    df = pd.DataFrame({"users": [f"user{x}" for x in rng.integers(0, 150, n_obs)],
                       "items": [f"film-{x}" for x in rng.integers(0, 400, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 5, iterations=30, sampling=3, seed=4)
    model.fit(df, silent=True)
    rec0 = model.recommend(n=8)                         # straight after fit: the resident slots
    model.predict(df.iloc[:300])
    stats = model.score(silent=True)["stats"]
    rec = model.recommend(n=8)                          # after predict: uploaded parameters
    assert model.score(silent=True)["stats"] == stats
    for col in ("users", "items", "rank"):
        assert rec[col].tolist() == rec0[col].tolist()
    np.testing.assert_allclose(rec["score"].to_numpy(float), rec0["score"].to_numpy(float), rtol=0, atol=TOL * rec["score"].abs().max())
    assert set(rec["users"]) <= set(df["users"]) and (rec.groupby("users", sort=False).size() <= 8).all()
    train = set(zip(df["users"], df["items"]))
    assert not any((u, i) in train for u, i in zip(rec["users"], rec["items"]))
    pairs = pd.DataFrame({"users": rec["users"], "items": rec["items"], "ratings": df["ratings"].iloc[0]})
    expect = model.predict(pairs) @ np.asarray(model.ratings, dtype=np.float64)   # the device predict path
    np.testing.assert_allclose(rec["score"].to_numpy(float), expect, rtol=0, atol=TOL * np.abs(expect).max())
    sub = model.recommend(users=["user7", "user3", "user7"], n=3)
    assert sub["users"].tolist()[:3] == ["user7"] * 3 and sub["users"].tolist()[-3:] == ["user7"] * 3
    with pytest.raises(KeyError):
        model.recommend(users=["user7", "nobody"])


def test_full_size_c3(hip):
    U, I, R, K = 100_000, 20_000, 5, 20
    data = orc.synthetic_triples(1_000_000, U, I, R, seed=0)
    U = int(data[:, 0].max()) + 1
    rng = np.random.default_rng(0)
    params = [(rng.random((U, K)), rng.random((I, K)), orc.normalize_with_self(rng.random((K, K, R))))]
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R)
    try:
        got = run(em, 1, np.arange(U, dtype=np.int32), 10, w)
    finally:
        em.close()
    pos = np.random.default_rng(2).choice(U, 256, replace=False)
    ref = restate_scores(params, pos, I, w)
    # seen items of the sampled users only
    mask = np.isin(data[:, 0], pos)
    seen = {int(u): set() for u in pos}
    for u, i in zip(data[mask, 0].tolist(), data[mask, 1].tolist()):
        seen[u].add(i)
    check_rows(got, ref, pos, 10, seen, np.arange(U))


def test_every_recommend_kernel_is_launched(hip):
    with LaunchWindow() as lw:
        for U, I in ((1, 5000), (300, 400)):           # items split across waves + merge; one wave per user
            data, params = problem(U, I, 3, 4, 6, 1, 2000, seed=U)
            em = context(hip, data, params, U, I, 3)
            try:
                run(em, 1, np.arange(U), 5, np.ones(3), exclude=True)
            finally:
                em.close()
        names = lw.names()
    for k in ("rec_w_kernel", "rec_fold_kernel", "rec_score_kernel", "rec_exclude_kernel"):
        assert k in names, (k, sorted(names))
    assert len({n for n in names if n.startswith("rec_select_kernel<")}) == 2, sorted(names)
