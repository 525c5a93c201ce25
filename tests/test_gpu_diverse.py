"""Diversified top-N and the distance of given pairs on the device (mmsbm_hip_recommend_diverse / _similar_pairs,
HipEM.recommend_diverse / similar_pairs, MMSBM.recommend_diverse, diverse.hpp) against diverse_reference.py.

Everything here is compared by EQUALITY -- items, counts, padding, and scores and distances by their bits:
  * on the models of exact_models.py the whole answer follows from the exact scores and the exact distances;
  * on random models the greedy reference is fed the device's own pool (recommend_query_within(n = pool)) and the
    device's own similar_pairs distances, so the kernel's chain, minimum, fma, arg-max and tie rule must be exact;
    similar_pairs itself is compared with similar_query by its bits, with itself (symmetry, zeros) and, within the
    tolerance test_gpu_similar.py derives, with the numpy restatement.

MMSBM_E_TOOLARGE is the one refusal not provoked here: it needs a device without free memory.
"""
import contextlib
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import diverse_reference as dr
import exact_models as xm
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)
from test_gpu_similar import MASS_BLOCK, tolerance
from test_similar_cpu import exact_distances, random_params, restate_distances

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = (6, 45, 2, 3, 2, 1)                                    # profile width K R S = 4: one piece, no tail
SHAPES = list(xm.MANY) + [TINY]                               # widths per slot 35 (8 pieces + 3), 36 (9 pieces), 4
FAMILIES = ("mixed", "sorted", "constant", "rare")
NS = (1, 2, 10, 64, 65)
LAMBDAS = (0.0, 2.0 ** -3, 0.3, 1.0, 2.0 ** 10)               # (0.3: the fma rounds)
SHAPE_ID = lambda s: "U{}I{}K{}L{}R{}S{}".format(*s)          # noqa: E731
WINDOW = {}


def pools_of(n):
    return sorted({p for p in (n, n + 1, 63, 64, 65, 256, 257, 1024) if p >= n})


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


@functools.lru_cache(maxsize=None)
def case_of(family, shape):
    """The session's inputs, exact scores and exact item distances: computed once, shared, never written to."""
    case = xm.make_case(family, "stars", shape)
    case["dist"] = exact_distances(case["params"], "items", np.arange(shape[1]))
    case["scores"].setflags(write=False)
    case["dist"].setflags(write=False)
    return case


@contextlib.contextmanager
def sessions(em, w, exclude, slots):
    """The recommend session and the similarity session over the items, the same slots added to both in one order."""
    em.recommend_begin(w, exclude)
    em.similar_begin("items")
    try:
        for s in slots:
            em.select(s).recommend_add()
            em.similar_add()
        yield em
    finally:
        em.similar_end()
        em.recommend_end()


def same_diverse(got, want, what):
    """(items, scores, distances, counts) equal in every entry, the padding included, the doubles by their bits."""
    for g, w, nm in zip(got, want, ("items", "scores", "distances", "counts")):
        real = nm in ("scores", "distances")
        gb, wb = (xm.bits(g), xm.bits(w)) if real else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        assert gb.shape == wb.shape, (what, nm, gb.shape, wb.shape)
        if not np.array_equal(gb, wb):
            row = int(np.argwhere(gb != wb)[0][0])
            raise AssertionError(f"{what}: {nm} differ in {int((gb != wb).sum())} entries, first in row {row}: "
                                 f"device {np.asarray(g)[row]}, reference {np.asarray(w)[row]}")


def same_as_plain(got, plain, what):
    """recommend_diverse at trade_off 0 against recommend_query_within(n): items, score bits, counts, padding."""
    same_diverse((got[0], got[1], np.zeros(0), got[3]), (plain[0], plain[1], np.zeros(0), plain[2]), what)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def request_rows(case, extra=6):
    """The edge users of xm.edge_triples (no candidate, LEFT = 9 candidates, the best level seen, nothing seen) and
    a few ordinary ones."""
    U = case["shape"][0]
    edge = sorted(case["roles"])
    rest = [u for u in range(U) if u not in case["roles"]][:extra]
    return i32(edge + rest)


# ---- 1. exact models, by equality; 3. lambda = 0 is the plain query -------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("family", FAMILIES)
def test_exact_models_by_equality(hip, family, shape, n):
    U, I, K, L, R, S = shape
    case = case_of(family, shape)
    users = request_rows(case)
    scores = case["scores"][users]
    assert "all" in case["roles"].values() and "all_but" in case["roles"].values() and xm.LEFT < 10
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        with sessions(em, case["w"], True, range(S)):
            for pool in pools_of(n):
                plain = em.recommend_query_within(users, n)
                for lam in LAMBDAS:
                    got = em.recommend_diverse(users, n, pool, lam)
                    want = dr.exact_diverse(case["params"], users, case["w"], case["seen"], None, None, n, pool, lam,
                                            scores=scores, dist=case["dist"])
                    same_diverse(got, want, f"{family} {shape} n={n} pool={pool} lambda={lam}")
                    if lam == 0.0:
                        same_as_plain(got, plain, f"lambda=0 n={n} pool={pool}")
            assert em.get_option("diverse_ms") > 0
    finally:
        em.close()
    counts = want[3].tolist()
    left = [I - len(case["seen"][u]) for u in users.tolist()]
    assert counts == [min(n, c) for c in left] and 0 in left and xm.LEFT in left


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("family", FAMILIES)
def test_a_candidate_subset_and_own_exclusion_lists(hip, family, shape):
    U, I, K, L, R, S = shape
    case = case_of(family, shape)
    rng = np.random.default_rng(xm.case_seed(family, "stars", shape))
    users = request_rows(case)
    users = i32(np.concatenate([users, users[-2:]]))            # two users asked twice, with two lists each
    scores = case["scores"][users]
    cand = i32(np.sort(rng.choice(I, (2 * I) // 5, replace=False)))
    lists = [rng.choice(I, int(k), replace=True) for k in rng.integers(0, 40, len(users))]
    lists[4] = np.zeros(0, dtype=np.int64)
    for b in (len(users) - 2, len(users) - 1):                  # the second list of a repeated user: its plain best items
        lists[b] = cat.within_top_n(scores[b:b + 1], users[b:b + 1], 5, cand, case["seen"])[0][0, :5]
        lists[b] = lists[b][lists[b] >= 0]
    extra = cat.csr(lists)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            seen = case["seen"] if exclude else None
            with sessions(em, case["w"], exclude, range(S)):
                for n, pool, lam in ((10, 10, 0.3), (10, 64, 2.0 ** 10), (10, 257, 0.3), (2, 65, 1.0), (65, 256, 2.0 ** -3)):
                    for c, x, xl in ((cand, None, None), (None, extra, lists), (cand, extra, lists)):
                        got = em.recommend_diverse(users, n, pool, lam, c, x)
                        want = dr.exact_diverse(case["params"], users, case["w"], seen, c, xl, n, pool, lam,
                                                scores=scores, dist=case["dist"])
                        what = f"{family} {shape} exclude={exclude} n={n} pool={pool} lambda={lam} cand={c is not None} own={x is not None}"
                        same_diverse(got, want, what)
                        zero = em.recommend_diverse(users, n, pool, 0.0, c, x)
                        plain = em.recommend_query_within(users, n, c, x)
                        same_as_plain(zero, plain, "lambda=0 " + what)
                one = i32([I // 2])                              # one candidate (none for a user that has seen it)
                for n, pool in ((1, 1), (2, 65), (10, 64)):
                    got = em.recommend_diverse(users, n, pool, 0.3, one)
                    same_diverse(got, dr.exact_diverse(case["params"], users, case["w"], seen, one, None, n, pool, 0.3,
                                                       scores=scores, dist=case["dist"]), f"one candidate n={n} pool={pool}")
                    assert set(got[3].tolist()) == ({0, 1} if exclude else {1})
    finally:
        em.close()
    both = want[0][-2:]                                          # the repeated users' second rows: their own lists bite
    first = want[0][len(users) - 4:len(users) - 2]
    assert (both != first).any()


# ---- 2. random models: the device's own pool and distances through the reference ------------------------------------------
RANDOM = [(200, 700, 5, 8, 4, 1), (150, 600, 8, 5, 3, 3)]       # (U, I, K, L, R, S): K != L both ways, S = 1 and 3


@functools.lru_cache(maxsize=None)
def random_problem(shape):
    U, I, K, L, R, S = shape
    rng = np.random.default_rng([7, *shape])
    params = random_params(rng, U, I, K, L, R, S)
    for _, eta, _ in params:
        eta[[17, 300]] = eta[5]                                 # identical item rows in every slot
    data = np.stack([rng.integers(0, U, 5 * U), rng.integers(0, I, 5 * U), rng.integers(0, R, 5 * U)], 1)
    return data, params


def pool_tables(em, users, pool, cand=None, extra=None):
    """Per request row: the ids of its `pool` best candidates and their pairwise similar_pairs distances, place a of
    the pool as the query row -- the device's own numbers."""
    p_ids, _, p_cnt = em.recommend_query_within(users, pool, cand, extra)
    out = []
    for b in range(len(users)):
        mine = p_ids[b, :int(p_cnt[b])]
        k = len(mine)
        d = em.similar_pairs(np.repeat(mine, k), np.tile(mine, k)).reshape(k, k) if k else np.zeros((0, 0))
        out.append((mine, d))
    return out


def device_greedy(em, users, n, pool, lam, tables, cand=None, extra=None):
    """greedy over the device's own recommend_query_within(n = pool) rows and the device's own distances (tables:
    pool_tables of a pool at least as large -- the order is total, so a smaller pool is its prefix)."""
    p_ids, p_sc, p_cnt = em.recommend_query_within(users, pool, cand, extra)
    rows = []
    for b in range(len(users)):
        k = int(p_cnt[b])
        ids, d = tables[b]
        assert np.array_equal(p_ids[b, :k], ids[:k])
        rows.append(dr.greedy(p_ids[b, :k], p_sc[b, :k], d[:k, :k], n, lam))
    return dr.pack(rows, n)


@pytest.mark.parametrize("shape", RANDOM, ids=SHAPE_ID)
def test_random_models_by_equality(hip, shape):
    U, I, K, L, R, S = shape
    data, params = random_problem(shape)
    w = np.arange(1.0, R + 1)
    rng = np.random.default_rng(3)
    users = i32(rng.choice(U, 6, replace=False))
    cand = i32(np.sort(rng.choice(I, 300, replace=False)))
    extra = cat.csr([rng.choice(I, 25, replace=False) for _ in users])
    em = context(hip, data, params, U, I, R)
    try:
        with sessions(em, w, True, range(S)):
            tables = pool_tables(em, users, 257)
            for n in (1, 2, 10, 65):
                for pool in sorted({n, 64, 65, 257} - set(range(n))):
                    for lam in LAMBDAS:
                        got = em.recommend_diverse(users, n, pool, lam)
                        same_diverse(got, device_greedy(em, users, n, pool, lam, tables), f"{shape} n={n} pool={pool} lambda={lam}")
                        if lam == 0.0:
                            plain = em.recommend_query_within(users, n)
                            same_as_plain(got, plain, f"lambda=0 n={n} pool={pool}")
            tables = pool_tables(em, users, 100, cand, extra)
            for lam in (0.3, 2.0 ** 10):
                got = em.recommend_diverse(users, 10, 100, lam, cand, extra)
                same_diverse(got, device_greedy(em, users, 10, 100, lam, tables, cand, extra), f"{shape} subset and own lists lambda={lam}")
                assert np.isin(got[0], cand).all()
    finally:
        em.close()


@pytest.mark.parametrize("side", ("items", "users"))
@pytest.mark.parametrize("shape", RANDOM, ids=SHAPE_ID)
def test_similar_pairs_three_ways(hip, shape, side):
    U, I, K, L, R, S = shape
    data, params = random_problem(shape)
    rows, others = (I, U) if side == "items" else (U, I)
    G, groups = (L, K) if side == "items" else (K, L)
    ids = np.arange(rows, dtype=np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        em.similar_begin(side)
        for s in range(S):
            em.select(s).similar_add()
        near, near_d, counts = em.similar_query(ids, rows - 1)
        a, b = np.repeat(ids, rows - 1), near.ravel()
        d_ab = em.similar_pairs(a, b)
        d_ba = em.similar_pairs(b, a)
        diag = em.similar_pairs(ids, ids)
        assert em.get_option("diverse_ms") > 0
        twins = em.similar_pairs([5, 17, 300, 5], [17, 300, 5, 300]) if side == "items" else None
        assert em.similar_pairs([], []).shape == (0,)
        em.similar_end()
    finally:
        em.close()
    assert (counts == rows - 1).all()
    # bits against similar_query, for every ordered pair of distinct rows
    assert np.array_equal(xm.bits(d_ab), xm.bits(near_d.ravel()))
    # bits of its own answers: symmetric; +0.0 on the diagonal and between identical rows
    assert np.array_equal(xm.bits(d_ab), xm.bits(d_ba))
    assert (xm.bits(diag) == 0).all()
    if twins is not None:
        assert (xm.bits(twins) == 0).all()
    # tolerance against the numpy restatement
    ref = restate_distances(params, side, ids)
    want = ref[a, b]
    tol = tolerance(want, G, R, S * groups * R, -(-others // MASS_BLOCK) + 8)
    err = np.abs(d_ab - want)
    print(f"{shape} {side}: largest error / tolerance {np.max(err / np.maximum(tol, 1e-300)):.3f}, largest error {err.max():.3e}")
    assert (err <= tol).all()


# ---- 4. a row depends on its user and the arguments only -------------------------------------------------------------------
ARGS = ((10, 100, 0.3), (65, 257, 2.0 ** 10), (2, 64, 1.0))


def test_a_row_depends_on_its_user_and_the_arguments_only(hip):
    shape = RANDOM[1]
    U, I, K, L, R, S = shape
    data, params = random_problem(shape)
    w = np.arange(1.0, R + 1)
    rng = np.random.default_rng(5)
    perm = rng.permutation(U)
    rep = np.array([perm[3], 0, perm[3], U - 1, perm[3]])
    em = context(hip, data, params, U, I, R)
    try:
        with sessions(em, w, True, range(S)):
            for n, pool, lam in ARGS:
                every = em.recommend_diverse(np.arange(U), n, pool, lam)
                for pick, what in ((np.arange(U), "again"), (perm, "shuffled"), (rep, "repeated"), (perm[:1], "one")):
                    same_diverse(em.recommend_diverse(pick, n, pool, lam), tuple(x[pick] for x in every), f"{what} {n} {pool} {lam}")
                for rows_per in (1, 7, U):                      # the request taken in parts: time and memory, never the answer
                    em.set_option("diverse_rows", rows_per)
                    same_diverse(em.recommend_diverse(perm, n, pool, lam), tuple(x[perm] for x in every), f"rows {rows_per}")
                em.set_option("diverse_rows", 0)
            extra = cat.csr([rng.choice(I, 20, replace=False) for _ in perm])
            whole = em.recommend_diverse(perm, 10, 64, 0.3, None, extra)
            em.set_option("diverse_rows", 7)                    # own lists follow their rows into the parts
            same_diverse(em.recommend_diverse(perm, 10, 64, 0.3, None, extra), whole, "own lists in parts")
            em.set_option("diverse_rows", 0)
    finally:
        em.close()


def test_swapped_contexts_are_bitwise_equal(hip):
    shape = RANDOM[0]
    U, I, K, L, R, S = shape
    data, params = random_problem(shape)
    w = np.arange(1.0, R + 1)
    answers = []
    for swap in (0, 1):
        em = context(hip, data, params, U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            with sessions(em, w, True, range(S)):
                answers.append([em.recommend_diverse(np.arange(U), *a) for a in ARGS])
        finally:
            em.close()
    for a, b, args in zip(answers[0], answers[1], ARGS):
        same_diverse(b, a, f"swap {args}")


def test_slots_beyond_those_added_do_not_matter(hip):
    U, I, K, L, R = 150, 400, 5, 6, 4
    rng = np.random.default_rng(4)
    params = random_params(rng, U, I, K, L, R, 3)
    data = np.stack([rng.integers(0, U, 5 * U), rng.integers(0, I, 5 * U), rng.integers(0, R, 5 * U)], 1)
    w = np.arange(1.0, R + 1)

    def ask(ps, slots):
        em = context(hip, data, ps, U, I, R)
        try:
            with sessions(em, w, True, slots):
                return [em.recommend_diverse(np.arange(U), *a) for a in ARGS]
        finally:
            em.close()
    alone, last = ask(params[:1], [0]), ask(params[2:], [0])
    for got, want, what in ((ask(params, [0]), alone, "slot 0 of 3"), (ask(params, [2]), last, "slot 2 of 3")):
        for g, x, args in zip(got, want, ARGS):
            same_diverse(g, x, f"{what} {args}")


def test_resident_and_uploaded_parameters_are_bitwise_equal(hip):
    shape = RANDOM[1]
    U, I, K, L, R, S = shape
    data, params = random_problem(shape)
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R)
    try:
        em.iterate(3)                                            # resident slots, moved by the EM loop
        fitted = [em.select(s).get_params() for s in range(S)]
        with sessions(em, w, True, range(S)):
            resident = [em.recommend_diverse(np.arange(U), *a) for a in ARGS]
    finally:
        em.close()
    other = context(hip, data, fitted, U, I, R)
    try:
        with sessions(other, w, True, range(S)):
            for want, args in zip(resident, ARGS):
                same_diverse(other.recommend_diverse(np.arange(U), *args), want, f"uploaded {args}")
    finally:
        other.close()


# ---- 5. refusals and side effects -------------------------------------------------------------------------------------------
def test_nothing_else_moves(hip):
    shape = RANDOM[1]
    U, I, K, L, R, S = shape
    data, params = random_problem(shape)
    w = np.arange(1.0, R + 1)
    users = np.arange(U)
    test = data[:400]
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
        em.predict_begin(test, w)
        em.select(0).predict_add()
        with sessions(em, w, True, range(S)):
            rec = em.recommend_query(users, 20)
            sim = em.similar_query(np.arange(I), 20)
            for a in ARGS:
                em.recommend_diverse(users, *a)
            em.recommend_diverse(users, 10, 50, 0.3, i32(np.arange(0, I, 3)), cat.csr([[1, 2, 3]] * U))
            em.similar_pairs(np.arange(I), np.arange(I)[::-1].copy())
            rec2 = em.recommend_query(users, 20)
            sim2 = em.similar_query(np.arange(I), 20)
        after = [em.select(s).get_params() for s in range(S)]
        for s in range(1, S):
            em.select(s).predict_add()
        mat, raw = em.predict_finish()
        em.predict_begin(test, w)
        for s in range(S):
            em.select(s).predict_add()
        mat2, raw2 = em.predict_finish()
    finally:
        em.close()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(xm.bits(a), xm.bits(b))
    for got, want in ((rec2, rec), (sim2, sim)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(xm.bits(got[1]), xm.bits(want[1])) and np.array_equal(got[2], want[2])
    assert np.array_equal(xm.bits(mat), xm.bits(mat2)) and np.array_equal(xm.bits(raw), xm.bits(raw2))


def test_refusals_by_status_code_before_any_launch(hip):
    U, I, K, L, R, S = 50, 60, 4, 3, 3, 2
    rng = np.random.default_rng(2)
    params = random_params(rng, U, I, K, L, R, S)
    data = np.stack([rng.integers(0, U, 5 * U), rng.integers(0, I, 5 * U), rng.integers(0, R, 5 * U)], 1)
    w = np.arange(1.0, R + 1)
    lib = hip._lib
    users = i32([0, 1])
    off = np.array([0, 2, 3], dtype=np.int64)

    def refused(call, code=lib.E_INVALID):
        with pytest.raises(lib.HipLibraryError) as e:
            call()
        assert e.value.code == code, (e.value.code, e.value.message)

    def ok(**kw):
        a = dict(users=users, n=3, pool=5, trade_off=0.5, candidates=None, exclude=None)
        a.update(kw)
        return lambda: em.recommend_diverse(a["users"], a["n"], a["pool"], a["trade_off"], a["candidates"], a["exclude"])

    with LaunchWindow() as lw:
        em = context(hip, data, params, U, I, R)
        try:
            refused(ok())                                        # no session at all
            refused(lambda: em.similar_pairs([0], [1]))
            em.recommend_begin(w, True)
            refused(ok())                                        # no slot added, no similarity session
            em.select(0).recommend_add()
            refused(ok())                                        # no similarity session
            em.similar_begin("users")
            em.similar_add()
            refused(ok())                                        # one of side users
            em.similar_begin("items")
            refused(ok())                                        # no slot added to it
            refused(lambda: em.similar_pairs([0], [1]))
            em.similar_add()
            em.select(1).recommend_add()
            refused(ok())                                        # slot counts differ: 2 and 1
            em.select(1).similar_add()
            for bad in (i32([0, U]), i32([-1, 0])):
                refused(ok(users=bad))
            for bad in (i32([5, 3, 8]), i32([3, 5, 5]), i32([-1, 3]), i32([3, I])):
                refused(ok(candidates=bad))
            refused(ok(exclude=(np.array([0, 2, 1], dtype=np.int64), i32([1]))))      # a bad CSR
            refused(ok(exclude=(np.array([1, 2, 3], dtype=np.int64), i32([1, 2, 3]))))
            refused(ok(exclude=(off, i32([1, 2, I]))))
            for bad in (0, -1):
                refused(ok(n=bad))
            refused(ok(n=6, pool=5))                             # pool < n
            for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
                refused(ok(trade_off=bad))
            refused(ok(pool=1025), lib.E_UNSUPPORTED)
            for bad in (-1, I):
                refused(lambda: em.similar_pairs([0, bad], [1, 2]))
                refused(lambda: em.similar_pairs([0, 1], [bad, 2]))
            em.recommend_add_items(np.stack([p[1][:2] for p in params]))
            refused(ok())                                        # the catalogue was grown
        finally:
            em.close()
        names = lw.names()                                       # (read once the context is closed)
    assert not [k for k in names if k.startswith(("div_", "cat_", "rec_score", "rec_select", "rec_exclude", "sim_dist"))], sorted(names)


def test_requests_beyond_the_candidates_and_empty_ones(hip):
    U, I, K, L, R, S = 50, 60, 4, 3, 3, 2
    rng = np.random.default_rng(2)
    params = random_params(rng, U, I, K, L, R, S)
    data = np.stack([rng.integers(0, U, 5 * U), rng.integers(0, I, 5 * U), rng.integers(0, R, 5 * U)], 1)
    users = i32([0, 1])
    em = context(hip, data, params, U, I, R)
    try:
        with sessions(em, np.arange(1.0, R + 1), True, range(S)):
            got = em.recommend_diverse(users, I + 5, I + 9, 0.5)  # n beyond the candidates: every one of them, padded
            assert (got[3] <= I).all() and (got[3] > 0).all()
            for b in range(2):
                k = got[3][b]
                assert sorted(got[0][b, :k].tolist()) == sorted(em.recommend_query_within(users[b:b + 1], I)[0][0, :k].tolist())
                assert (got[0][b, k:] == -1).all() and np.isposinf(got[2][b, k:]).all() and np.isneginf(got[1][b, k:]).all()
                assert np.isposinf(got[2][b, 0]) and np.isfinite(got[2][b, 1:k]).all()
            assert em.recommend_diverse([], 3, 5, 0.5)[0].shape == (0, 3)
            none = em.recommend_diverse(users, 3, 5, 0.5, i32([]))
            assert none[3].tolist() == [0, 0] and (none[0] == -1).all() and np.isposinf(none[2]).all()
    finally:
        em.close()


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_the_host_class_with_string_ids(hip):
    rng = np.random.default_rng(12)
    n_u, n_i, n_obs = 60, 150, 1500
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 6, iterations=8, sampling=2, seed=5)
    model.fit(df, silent=True)
    items = model.data_handler.item_labels()
    model.predict(df.iloc[:100])
    stats = model.score(silent=True)["stats"]
    ask = ["u7", "u1", "u7", "u30"]
    plain = model.recommend(users=ask, n=5)
    zero = model.recommend_diverse(users=ask, n=5, diversity=0)
    assert list(zero.columns) == ["users", "items", "score", "distance", "rank"]
    for col in ("users", "items", "rank"):
        assert zero[col].tolist() == plain[col].tolist()
    assert np.array_equal(xm.bits(zero["score"].to_numpy()), xm.bits(plain["score"].to_numpy()))
    # the frame against the reference fed with the library's own pool and distances
    lam, pool = 5.0, 30
    got = model.recommend_diverse(users=ask, n=5, diversity=lam, pool=pool)
    pools = model.recommend(users=ask, n=pool)
    row = 0
    for b, u in enumerate(ask):
        mine = pools.iloc[b * pool:(b + 1) * pool]
        assert (mine["users"] == u).all() and len(mine) == pool
        labels = mine["items"].tolist()
        pairs = [(x, y) for x in labels for y in labels]
        d = model.distances(pairs)["distance"].to_numpy().reshape(pool, pool)
        it, sc, dd, _ = dr.greedy(np.arange(pool), mine["score"].to_numpy(), d, 5, lam)
        block = got.iloc[row:row + 5]
        assert block["users"].tolist() == [u] * 5 and block["rank"].tolist() == [1, 2, 3, 4, 5]
        assert block["items"].tolist() == [labels[j] for j in it]
        assert np.array_equal(xm.bits(block["score"].to_numpy()), xm.bits(sc))
        assert np.array_equal(xm.bits(block["distance"].to_numpy()), xm.bits(dd))
        row += 5
    assert len(got) == row
    # the summary: what diversity= bought
    spread, base = model.list_diversity(got), model.list_diversity(plain)
    assert spread["users"].tolist() == ["u7", "u1", "u30"] and spread["n"].tolist() == [10, 5, 5]
    one = got[got["users"] == "u1"]["items"].tolist()
    want = model.distances([(x, y) for k, x in enumerate(one) for y in one[k + 1:]])["distance"].mean()
    assert spread["diversity"].iloc[1] == pytest.approx(want, rel=1e-12)
    print(pd.concat([base, spread["diversity"].rename("diverse")], axis=1))
    sub = model.recommend_diverse(users=ask, n=5, diversity=lam, candidates=items[::3], exclude=[("u7", items[0])])
    assert set(sub["items"]) <= set(items[::3]) and not ((sub["users"] == "u7") & (sub["items"] == items[0])).any()
    users_d = model.distances([("u7", "u1"), ("u1", "u7"), ("u7", "u7")], side="users")
    assert xm.bits(users_d["distance"].to_numpy())[0] == xm.bits(users_d["distance"].to_numpy())[1]
    assert users_d["distance"].iloc[2] == 0.0
    with pytest.raises(KeyError, match="no-such-item"):
        model.distances([("item-1", "no-such-item")])
    assert model.score(silent=True)["stats"] == stats


# ---- 7. coverage -----------------------------------------------------------------------------------------------------------------
def test_every_kernel_of_the_feature_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith(("div_", "sim_pairs"))]
    for k in ("div_greedy_kernel", "div_pairs_kernel", "div_ids_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
