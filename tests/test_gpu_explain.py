"""Which of a user's training rows carry a recommendation, on the device (mmsbm_hip_explain_*, HipEM.explain_*;
explain.hpp) against the numpy restatement of tests/explain_reference.py.

Shapes: (K, L) in SHAPES (K <= L and K > L, K = 1, K beyond one wave's lanes), R = 5, 300 users x 1,500 items, about
6,300 random rows; users planted with 1, 63, 64 and 65 rows and one of 1,300 rows with duplicates (past the candidate
list's capacity at n = 5: its refill and re-sort path); S = 1 and 3; n in 1, 5, 300; both side layouts.

Tolerance: TOL x max|w| with TOL = 1e-12 of test_gpu_recommend.py.  With theta, eta rows and p on the simplex every
score, explained and contribution is at most max|w|, and the rounding of the chains is about (K L + S K + d_u) 2^-53
max|w| -- 2e-13 max|w| at these shapes.

1. against the restatement, 2. exact order on models without rounding, 3. the identity against fold_in, 4. independence
bit for bit, 5. no side effects, 6. refusals by status code, 7. the launch log.  MMSBM_E_TOOLARGE for missing device
memory is the one refusal not provoked here."""
import collections
import os
import sys

import numpy as np
import pytest

import exact_models as xm
import explain_reference as xr
from conftest import ROOT
from oracle import mmsbm_oracle as orc
from test_gpu_recommend import TOL, LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW = {}
NEW_KERNELS = ("exp_p_kernel", "exp_row_kernel", "exp_pair_kernel")
SHAPES = [(1, 4), (3, 5), (5, 3), (20, 20), (70, 3)]
SHAPE_ID = lambda s: f"K{s[0]}L{s[1]}"  # noqa: E731
U, I, R = 300, 1500, 5
PLANTED = {0: 1, 1: 63, 2: 64, 3: 65}
HEAVY, HEAVY_ROWS = 4, 1300
W = np.arange(1.0, R + 1)
NS = (1, 5, 300)
OUT = ("hist_items", "hist_ratings", "contribution", "counts", "explained", "score", "degree")


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


# ---- the data, the models and the request: built once ------------------------------------------------------------------
_CACHE = {}


def training_rows():
    if "data" not in _CACHE:
        rng = np.random.default_rng(17)
        free = np.arange(HEAVY + 1, U)
        parts = [np.stack([rng.choice(free, 6000), rng.integers(0, I, 6000), rng.integers(0, R, 6000)], 1),
                 np.stack([free, free % I, free % R], 1)]                       # every user holds a row
        for u, d in PLANTED.items():
            parts.append(np.stack([np.full(d, u), rng.integers(0, I, d), rng.integers(0, R, d)], 1))
        heavy = np.stack([np.full(1200, HEAVY), rng.integers(0, I, 1200), rng.integers(0, R, 1200)], 1)
        parts += [heavy, heavy[:HEAVY_ROWS - 1200]]                              # duplicate triples: separate rows
        data = np.concatenate(parts)
        data = data[rng.permutation(len(data))]                                  # a user's rows lie scattered
        deg = np.bincount(data[:, 0], minlength=U)
        assert all(deg[u] == d for u, d in PLANTED.items()) and deg[HEAVY] == HEAVY_ROWS and deg.min() >= 1
        _CACHE["data"] = data
    return _CACHE["data"]


def request():
    """(users, offsets, items): the planted users, the heavy one, others; a user twice, one without pairs, repeated
    items."""
    users = [0, 1, 2, 3, HEAVY, 7, 150, 299, 2, 88, 41, 7, 260]
    sizes = [2, 2, 3, 2, 2, 3, 1, 2, 1, 0, 2, 2, 1]
    rng = np.random.default_rng(3)
    items = rng.integers(0, I, sum(sizes)).astype(np.int32)
    items[1] = items[0]                                                         # a pair twice
    items[-1] = I - 1
    return np.asarray(users, dtype=np.int32), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), items


def pairs_of(users, offsets, items):
    return [(int(u), int(items[e])) for b, u in enumerate(users) for e in range(int(offsets[b]), int(offsets[b + 1]))]


def model(K, L, S):
    """(params, restatement): S random parameter sets with theta and eta rows and p on the simplex."""
    key = (K, L, S)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * K + 10 * L + S)
        params = []
        for _ in range(S):
            th, eta = rng.random((U, K)), rng.random((I, L))
            params.append((th / th.sum(axis=1, keepdims=True), eta / eta.sum(axis=1, keepdims=True),
                           orc.normalize_with_self(rng.random((K, L, R)))))
        _CACHE[key] = (params, xr.Restatement(training_rows(), params, W))
    return _CACHE[key]


def open_explain(em, n_slots, w=W):
    em.explain_begin(w)
    for s in range(n_slots):
        em.select(s).explain_add()


def same_bits(got, want, what):
    for g, h, nm in zip(got, want, OUT):
        gb, hb = (xm.bits(g), xm.bits(h)) if g.dtype == np.float64 else (g, h)
        assert gb.shape == hb.shape and np.array_equal(gb, hb), f"{what}: {nm} differ in {int((gb != hb).sum())} entries"


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------
def check_against(ref, got, pairs, n, what):
    hi, hr, co, counts, explained, score, degree = got
    tol = TOL * np.abs(ref.w).max()
    for q, (u, t) in enumerate(pairs):
        r = ref.pair(u, t)
        d, m = r["degree"], min(n, r["degree"])
        print(f"{what} pair {q} (u={u}, t={t}, d={d}): score {abs(score[q] - r['score']):.3e} explained "
              f"{abs(explained[q] - r['explained']):.3e} (tol {tol:.3e})")
        assert degree[q] == d and counts[q] == m, (what, q, degree[q], counts[q])
        assert abs(score[q] - r["score"]) <= tol and abs(explained[q] - r["explained"]) <= tol, (what, q)
        assert (hi[q, m:] == -1).all() and (hr[q, m:] == -1).all() and np.isneginf(co[q, m:]).all(), (what, q)
        # every returned row is a row of the user (as often as the user holds it), with that row's contribution
        a_of = {}
        for i, rt, a in zip(r["items"].tolist(), r["ratings"].tolist(), r["a"].tolist()):
            a_of.setdefault((i, rt), a)
        have = collections.Counter(zip(r["items"].tolist(), r["ratings"].tolist()))
        took = collections.Counter(zip(hi[q, :m].tolist(), hr[q, :m].tolist()))
        assert not took - have, (what, q, took - have)
        want = np.array([a_of[key] for key in zip(hi[q, :m].tolist(), hr[q, :m].tolist())])
        assert np.abs(co[q, :m] - want).max() <= tol, (what, q, np.abs(co[q, :m] - want).max())
        assert (np.diff(co[q, :m]) <= 0).all(), (what, q)
        left = have - took                                  # the rows not returned: none beats the n-th by more than tol
        assert sum(left.values()) == d - m
        if left:
            assert co[q, m - 1] >= max(a_of[key] for key in left) - tol, (what, q)


@pytest.mark.parametrize("swap", [0, 1], ids=["unswapped", "swapped"])
@pytest.mark.parametrize("S", [1, 3], ids=["S1", "S3"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
def test_against_the_restatement(hip, shape, S, swap):
    K, L = shape
    params, ref = model(K, L, S)
    users, offsets, items = request()
    pairs = pairs_of(users, offsets, items)
    em = context(hip, training_rows(), params, U, I, R, swap=swap)
    try:
        assert em.swapped == bool(swap)
        open_explain(em, S)
        for n in NS:
            check_against(ref, em.explain_query(users, offsets, items, n), pairs, n, f"{shape} S={S} swap={swap} n={n}")
        assert em.get_option("explain_ms") > 0
        em.explain_end()
    finally:
        em.close()


# ---- 2. exact order: pure users, dyadic eta, p and w ------------------------------------------------------------------------------
EXACT_DEGREES = (1, 2, 64, 256, 1024, 4, 512, 128)     # powers of two: dividing by S d_u is exact


def exact_case(K, L, S):
    """One-hot theta (user u in group (u + s) mod K of slot s); eta, p and w from exact_models' "mixed" generator.  A
    user's rows are drawn from the (item, rating) combinations whose v = p[k_u, :, r] . eta[i] is positive and has
    v * (1 / v) == 1.0 in every slot (true of nearly all of these few-bit values, asserted here): then the one division
    and the one multiply of the row kernel give c = one-hot exactly, every row of a user carries the same bits, and
    the order is decided by (item id, rating) alone."""
    rng = np.random.default_rng(97 * K + L + S)
    n_u, n_i = len(EXACT_DEGREES), 200
    mixed, w = xm.model("mixed", rng, n_u, n_i, K, L, R, S, "stars")
    params = [(np.eye(K)[(np.arange(n_u) + s) % K], eta, p) for s, (_, eta, p) in enumerate(mixed)]
    rows = []
    for u, d in enumerate(EXACT_DEGREES):
        ok = np.ones((n_i, R), dtype=bool)
        for s, (_, eta, p) in enumerate(params):
            v = eta @ p[(u + s) % K]                                             # (I, R), exact: few-bit dyadics
            with np.errstate(divide="ignore", invalid="ignore"):
                ok &= (v > 0) & (v * (1.0 / v) == 1.0)
        cand = np.argwhere(ok)
        assert len(cand) >= 20, (K, L, S, u, len(cand))
        pick = cand[rng.integers(0, len(cand), d)]                               # with repeats: duplicate triples
        rows.append(np.column_stack([np.full(d, u), pick]))
    data = np.concatenate(rows)
    return data[rng.permutation(len(data))], params, w, n_u, n_i


@pytest.mark.parametrize("S", [1, 2], ids=["S1", "S2"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
def test_exact_ties_come_in_item_then_rating_order(hip, shape, S):
    K, L = shape
    data, params, w, n_u, n_i = exact_case(K, L, S)
    users = np.arange(n_u, dtype=np.int32)
    ask = np.array([0, 7, n_i - 1, 7], dtype=np.int32)
    offsets = np.arange(n_u + 1, dtype=np.int64) * len(ask)
    items = np.tile(ask, n_u)
    em = context(hip, data, params, n_u, n_i, R)
    try:
        open_explain(em, S, w)
        em.recommend_begin(w, False)
        for s in range(S):
            em.select(s).recommend_add()
        rec_items, rec_scores, _ = em.recommend_query(users, n_i)
        by_item = np.empty((n_u, n_i))
        by_item[np.arange(n_u)[:, None], rec_items] = rec_scores
        for n in NS:
            hi, hr, co, counts, explained, score, degree = em.explain_query(users, offsets, items, n)
            for q, (u, t) in enumerate(pairs_of(users, offsets, items)):
                mine = data[data[:, 0] == u][:, 1:]
                first = mine[np.lexsort((mine[:, 1], mine[:, 0]))][:n]
                d, m = len(mine), len(first)
                total = 0.0
                for s, (_, eta, p) in enumerate(params):                         # exact: few-bit dyadics, integer weights
                    total += float((p[(u + s) % K] @ w) @ eta[t])
                assert counts[q] == m and degree[q] == d
                assert hi[q, :m].tolist() == first[:, 0].tolist() and hr[q, :m].tolist() == first[:, 1].tolist(), (shape, S, n, q)
                assert (xm.bits(co[q, :m]) == xm.bits(np.float64(total / (S * d)))).all(), (shape, S, n, q)
                assert explained[q] == score[q] == total / S, (shape, S, n, q, explained[q], score[q], total / S)
                if K <= L:
                    assert xm.bits(score[q]) == xm.bits(by_item[u, t]), (shape, S, q)
                else:
                    assert abs(score[q] - by_item[u, t]) <= TOL * np.abs(w).max()
        em.recommend_end()
        em.explain_end()
    finally:
        em.close()


# ---- 3. the identity on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
def test_explained_is_the_score_under_one_more_theta_update(hip, shape):
    """explained(u, t) against sum_k theta'_u[k] g_t[k], theta' from the device's own fold_in at one iteration from
    theta0 = theta_u on u's own training rows, per slot."""
    K, L = shape
    S = 3
    params, _ = model(K, L, S)
    data = training_rows()
    users, offsets, items = request()
    distinct = sorted(set(users.tolist()))
    own = np.concatenate([np.column_stack([np.full((data[:, 0] == u).sum(), b), data[data[:, 0] == u][:, 1:]])
                          for b, u in enumerate(distinct)])
    em = context(hip, data, params, U, I, R)
    try:
        nxt = [em.select(s).fold_in(own, len(distinct), 1, theta0=params[s][0][distinct])[0] for s in range(S)]
        open_explain(em, S)
        explained = em.explain_query(users, offsets, items, 1)[4]
        em.explain_end()
    finally:
        em.close()
    tol = TOL * np.abs(W).max()
    for q, (u, t) in enumerate(pairs_of(users, offsets, items)):
        want = sum(float(nxt[s][distinct.index(u)] @ ((params[s][2] @ W) @ params[s][1][t])) for s in range(S)) / S
        print(f"{shape} pair {q}: |explained - theta' . g| = {abs(explained[q] - want):.3e} (tol {tol:.3e})")
        assert abs(explained[q] - want) <= tol, (shape, q, explained[q], want)


# ---- 4. independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5), (20, 20), (70, 3)], ids=SHAPE_ID)
def test_a_pair_depends_on_its_user_its_item_and_the_added_slots_only(hip, shape):
    K, L = shape
    S, n = 3, 5
    params, _ = model(K, L, S)
    data = training_rows()
    users, offsets, items = request()
    n_pairs = len(items)
    at = np.repeat(np.arange(len(users)), np.diff(offsets))                      # the occurrence of every pair
    em = context(hip, data, params, U, I, R)
    try:
        open_explain(em, S)
        full = em.explain_query(users, offsets, items, n)
        for q in (0, 1, 2, 5, 9, 10, n_pairs - 1):                               # alone
            one = em.explain_query(users[at[q]:at[q] + 1], [0, 1], items[q:q + 1], n)
            same_bits(one, [a[q:q + 1] for a in full], f"{shape} pair {q} alone")
        rev_sizes = np.diff(offsets)[::-1]                                       # the request reversed
        rev_off = np.concatenate([[0], np.cumsum(rev_sizes)]).astype(np.int64)
        order = np.concatenate([np.arange(offsets[b], offsets[b + 1])[::-1] for b in range(len(users))][::-1]).astype(np.int64)
        rev = em.explain_query(users[::-1].copy(), rev_off, items[order], n)
        same_bits(rev, [a[order] for a in full], f"{shape} reversed")
        for rows in (1, 64, 100, 1400, 0):                                       # batches cut inside and between users
            em.set_option("explain_rows", rows)
            assert em.get_option("explain_rows") == rows
            same_bits(em.explain_query(users, offsets, items, n), full, f"{shape} explain_rows={rows}")
        em.explain_end()
    finally:
        em.close()
    em = context(hip, data, params, U, I, R, swap=1)                             # the other side layout
    try:
        assert em.swapped
        open_explain(em, S)
        same_bits(em.explain_query(users, offsets, items, n), full, f"{shape} swapped")
        em.explain_end()
    finally:
        em.close()
    extra = params + [model(K, L, 1)[0][0]]                                      # a further slot that is not added
    em = context(hip, data, extra, U, I, R)
    try:
        open_explain(em, S)
        same_bits(em.explain_query(users, offsets, items, n), full, f"{shape} with a slot beyond those added")
        em.explain_end()
    finally:
        em.close()


# ---- 5. it touches nothing ------------------------------------------------------------------------------------------------------------
def test_no_side_effects(hip):
    K, L, S = 6, 5, 3
    params, _ = model(K, L, S)
    data = training_rows()
    users, offsets, items = request()
    all_users = np.arange(U, dtype=np.int32)
    lib = hip._lib.load()
    kernels = lib.mmsbm_hip_kernel_count()
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
        em.recommend_begin(W, True)
        em.similar_begin("items")
        for s in range(S):
            em.select(s).recommend_add()
            em.select(s).similar_add()
        rec = em.recommend_query(all_users, 10)
        sim = em.similar_query(np.arange(50, dtype=np.int32), 10)
        open_explain(em, S)                                                      # inside the two open sessions
        first = em.explain_query(users, offsets, items, 5)
        same_bits(em.explain_query(users, offsets, items, 5), first, "a second query")
        rec2 = em.recommend_query(all_users, 10)
        sim2 = em.similar_query(np.arange(50, dtype=np.int32), 10)
        em.explain_end()
        em.recommend_end()
        em.similar_end()
        after = [em.select(s).get_params() for s in range(S)]
    finally:
        em.close()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(xm.bits(a), xm.bits(b))
    for g, h in zip(rec + sim, rec2 + sim2):
        assert np.array_equal(xm.bits(g) if g.dtype == np.float64 else g, xm.bits(h) if h.dtype == np.float64 else h)
    assert lib.mmsbm_hip_kernel_count() == kernels


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def refused(hip, code, fn, *args, **kw):
    with pytest.raises(hip._lib.HipLibraryError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.message)


def test_refusals_by_status_code(hip):
    K, L = 4, 3
    params, _ = model(K, L, 1)
    data = training_rows()
    lib = hip._lib
    em = hip.HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, slots=2)
    try:
        em.select(0).set_params(*params[0])                                      # slot 1 holds no parameters
        ask = ([3, 7], [0, 1, 3], [5, 6, 5])
        refused(hip, lib.E_INVALID, em.explain_query, *ask, 3)                   # no session
        refused(hip, lib.E_INVALID, em.explain_add)
        em.explain_begin(W)
        refused(hip, lib.E_INVALID, em.explain_query, *ask, 3)                   # before the first add
        refused(hip, lib.E_INVALID, em.select(1).explain_add)                    # a slot without parameters
        em.select(0).explain_add()
        want = em.explain_query(*ask, 3)
        for bad in (-1, U):
            refused(hip, lib.E_INVALID, em.explain_query, [3, bad], [0, 1, 3], [5, 6, 5], 3)
        for bad in (-1, I):
            refused(hip, lib.E_INVALID, em.explain_query, [3, 7], [0, 1, 3], [5, bad, 5], 3)
        refused(hip, lib.E_INVALID, em.explain_query, [3, 7], [1, 1, 3], [5, 6, 5], 3)       # offsets not from 0
        refused(hip, lib.E_INVALID, em.explain_query, [3, 7], [0, 4, 3], [5, 6, 5], 3)       # offsets decrease
        for bad in (0, -2):
            refused(hip, lib.E_INVALID, em.explain_query, *ask, bad)
        refused(hip, lib.E_UNSUPPORTED, em.explain_query, *ask, hip.HipEM.MAX_RECOMMEND + 1)
        for bad in (np.nan, np.inf, -np.inf):
            w = W.copy()
            w[2] = bad
            refused(hip, lib.E_INVALID, em.explain_begin, w)                     # (the open session stays as it is)
        for bad in (-1, 2.5):
            refused(hip, lib.E_INVALID, em.set_option, "explain_rows", bad)
        same_bits(em.explain_query(*ask, 3), want, "the session is still usable")
        em.explain_end()
        refused(hip, lib.E_INVALID, em.explain_query, *ask, 3)
    finally:
        em.close()
    wide = hip.HipEM(data[:50], 1025, 1, n_users=U, n_items=I, n_ratings=R)  # MMSBM_HIP_FOLD_IN_MAX_K + 1 user groups
    try:
        refused(hip, lib.E_UNSUPPORTED, wide.explain_begin, W)                   # K beyond the groups it is built for
    finally:
        wide.close()


# ---- 7. the launch log ------------------------------------------------------------------------------------------------------------------
def test_every_explain_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("exp_")]
    assert sorted(compiled) == sorted(NEW_KERNELS), compiled
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
