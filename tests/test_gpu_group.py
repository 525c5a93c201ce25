"""Group recommendation on the device (mmsbm_hip_recommend_query_groups, HipEM.recommend_query_groups,
MMSBM.recommend_group; group.hpp) against the numpy restatement of group_reference.py:

1. by EQUALITY on models without rounding (exact_models): MIN / MAX / COUNT over groups of 1 .. U members laid out in two
   orders, n around the list sizes, with and without exclusions, bars on an occurring score, at 0 and below it (the
   padding trap); MEAN by bits where the model makes it exact (1, 2, 4, 8 members);
2. groups of one against recommend_query, bit for bit; 3. independence of the place in the request and of the side
   layout, and of how the member rows are dealt to workgroups (option "group_run_blocks": one run with a carry over
   every member tile, or groups cut into fragments that grp_combine_kernel joins); 4. exclusions that leave 9 and 0 candidates; 5. after recommend_add_items; 6. candidate subsets;
7. random models: the members' device scores aggregated in numpy, by bits (MIN / MAX / COUNT are selections) and within
   the derived bound (MEAN); 8. refusals by status code, 9. no side effects, 10. the launch log, 11. the host class
   end to end with string ids.

MMSBM_E_TOOLARGE for missing device memory is the one refusal not provoked here."""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import exact_models as xm
import group_reference as grp
from conftest import ROOT
from oracle import mmsbm_oracle as orc
from test_gpu_audience import DENSE, DENSE_ID, user_side_matrix
from test_gpu_catalogue import candidate_sets, i32, open_session, same_answer
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)
from test_recommend_cpu import seen_items

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW = {}
VARIANTS = [("mixed", "stars"), ("mixed", "signed"), ("sorted", "indicator"), ("constant", "indicator")]
SHAPES = list(xm.MANY) + [xm.SPLIT[1]]
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]
NS = (1, 10, 257)
SIZES = (1, 2, 7, 8, 9, 127, 128, 129)                     # around a block of 8 rows and a tile of 128
TILE_KERNELS = ("grp_tile_kernel<0>", "grp_tile_kernel<1>", "grp_tile_kernel<2>")
NEW_KERNELS = TILE_KERNELS + ("grp_combine_kernel", "grp_exclude_kernel", "grp_mean_kernel")


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


@functools.lru_cache(maxsize=None)
def case_of(variant, shape):
    """The session's inputs and exact scores: computed once, shared by the tests, never written to."""
    case = xm.make_case(*variant, shape)
    case["scores"].setflags(write=False)
    return case


def request(U, seed, order):
    """The groups of the issue -- SIZES and all U users, members drawn without repeats, in random member order -- as a
    list of id arrays: the SAME groups for a seed, laid out in two orders.  Order 0: ascending sizes, so the group of
    127 begins at block 6 of the request's first member tile and straddles its border; order 1: the groups of 128 and
    127 first, each exactly one tile, then the rest."""
    rng = np.random.default_rng(seed)
    sizes = [s for s in SIZES if s < U] + [U]
    groups = {s: rng.permutation(U)[:s].astype(np.int32) for s in sizes}
    if order == 1:
        sizes = [s for s in (128, 127) if s in groups] + [s for s in sizes if s not in (127, 128)]
    return [groups[s] for s in sizes]


def bars_of(scores):
    """An occurring score (the median: `>=` must take its whole tie group), 0 and a negative bar (the padding trap)."""
    return (float(np.sort(scores, axis=None)[scores.size // 2]), 0.0, -1.0)


def modes_and_bars(scores):
    return [("min", 0.0), ("max", 0.0)] + [("count", b) for b in bars_of(scores)]


def random_model(U, I, R, K, L, S, n_obs, seed):
    """Triples inside (U, I, R) and S random parameter sets whose theta and eta rows sum to 1, as a fitted model's do:
    a term of a score's sum is then bounded by max|w| (the premise of mean_bound)."""
    rng = np.random.default_rng(seed)
    data = np.stack([rng.integers(0, U, n_obs), rng.integers(0, I, n_obs), rng.integers(0, R, n_obs)], 1)
    rows = lambda n, d: (lambda a: a / a.sum(axis=1, keepdims=True))(rng.random((n, d)) + 0.01)  # noqa: E731
    return data, [(rows(U, K), rows(I, L), orc.normalize_with_self(rng.random((K, L, R)))) for _ in range(S)]


def mean_bound(F, size, w):
    """|device MEAN - numpy mean of the members' device scores| per item.  Both sides are fma / add chains of at most
    F = rank x S and `size` terms of magnitude <= max|w|, followed by one or two divisions: 4 (F + size) 2^-53 max|w|."""
    return 4.0 * (F + size) * 2.0 ** -53 * float(np.abs(w).max())


def check_mean(got, D, groups, n, F, w, seen=None, cand=None, what=""):
    """The MEAN answer against the members' device scores D (users x items): per returned item within mean_bound of
    numpy's mean, no item left out beats the n-th returned by more than the bound, the device's own order, the counts."""
    items, vals, counts = got
    base = np.arange(D.shape[1]) if cand is None else np.asarray(cand, dtype=np.int64)
    for g, mem in enumerate(groups):
        out = set() if seen is None else set().union(*(seen[m] for m in mem.tolist()))
        keep = base[~np.isin(base, np.fromiter(out, dtype=np.int64, count=len(out)))]
        want = min(n, len(keep)) if len(mem) else 0
        assert counts[g] == want, (what, g, counts[g], want)
        assert (items[g, want:] == -1).all() and np.isneginf(vals[g, want:]).all()
        if want == 0:
            continue
        it, sc = items[g, :want].astype(np.int64), vals[g, :want]
        ref = D[mem].mean(axis=0)
        tau = mean_bound(F, len(mem), w)
        assert len(set(it.tolist())) == want and np.isin(it, keep).all()
        assert np.abs(sc - ref[it]).max() <= tau, (what, g, np.abs(sc - ref[it]).max(), tau)
        assert np.array_equal(np.lexsort((it, -sc)), np.arange(want)), (what, g)
        left = np.setdiff1d(keep, it)
        if len(left):
            assert ref[left].max() <= sc[-1] + tau, (what, g, ref[left].max() - sc[-1], tau)


# ---- 1. exact models, by equality ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_selections_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    scores = case["scores"]
    if variant[1] == "signed":
        assert scores.min() < 0 < scores.max()             # MIN / MAX over scores of both signs
    requests = [cat.csr(request(U, xm.case_seed(*variant, shape), order)) for order in (0, 1)]
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)
            for order, (off, mem) in enumerate(requests):
                for mode, bar in modes_and_bars(scores):
                    for n in NS:
                        got = em.recommend_query_groups(off, mem, n, mode, bar)
                        same_answer(got, grp.group_top_n(scores, off, mem, n, mode, bar, None, seen),
                                    f"{mode} bar={bar!r} n={n} order={order} exclude={exclude}")
            assert em.get_option("group_ms") > 0
            em.recommend_end()
    finally:
        em.close()


@pytest.mark.parametrize("variant,shape", [c for c in CASES if c[1] in xm.MANY], ids=[i for i, c in zip(CASE_IDS, CASES) if c[1] in xm.MANY])
def test_mean_is_exact_on_dyadic_models(hip, variant, shape):
    """Every theta entry is a multiple of 1/8 (of 1 in the one-hot families), so the sum of 1, 2, 4 or 8 rows and its
    division are exact: the device's mean row is (mean theta) folded, and the score that of a user with that theta."""
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    cuts = np.cumsum([0, 8, 1, 4, 2, 8, 1])               # disjoint groups: every first member stands for one group
    perm = rng.permutation(U).astype(np.int32)
    groups = [perm[b:e] for b, e in zip(cuts[:-1], cuts[1:])]
    off, mem = cat.csr(groups)
    mean_params = [(np.stack([t[g].mean(axis=0) for g in groups]), e, p) for t, e, p in case["params"]]
    scores = np.zeros((U, I))                              # the groups' exact scores at their FIRST member's row
    firsts = [int(g[0]) for g in groups]
    scores[firsts] = xm.exact_scores(mean_params, np.arange(len(groups)), I, case["w"])
    one_off, one_mem = cat.csr([[f] for f in firsts])
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], False)
        for n in NS:
            same_answer(em.recommend_query_groups(off, mem, n, "mean"),
                        grp.group_top_n(scores, one_off, one_mem, n, "min"), f"mean n={n}")
        em.recommend_end()
    finally:
        em.close()


# ---- 2. groups of one ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude", [True, False], ids=["unseen", "all"])
def test_groups_of_one_are_recommend_query(hip, exclude):
    K, L, R, S, U, I = DENSE[1]
    data, params = random_model(U, I, R, K, L, S, 5 * U, seed=5)
    users = np.random.default_rng(6).permutation(U).astype(np.int32)
    off = np.arange(U + 1, dtype=np.int64)
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, np.arange(1.0, R + 1), exclude)
        for n in (1, 10, 257):
            want = em.recommend_query(users, n)
            for mode in ("min", "max", "mean"):
                same_answer(em.recommend_query_groups(off, users, n, mode), want, f"{mode} n={n}")
        full = em.recommend_query(users, I)
        bar = float(np.median(full[1][np.isfinite(full[1])]))
        D = np.full((U, I), -np.inf)
        keep = np.arange(I)[None, :] < full[2][:, None]
        D[np.repeat(users, full[2]), full[0][keep]] = full[1][keep]
        seen = [set(np.flatnonzero(np.isneginf(D[u])).tolist()) for u in range(U)]
        got = em.recommend_query_groups(off, users, 257, "count", bar)
        same_answer(got, grp.group_top_n(D, off, users, 257, "count", bar, None, seen), "count")
        assert set(np.unique(got[1][np.isfinite(got[1])]).tolist()) == {0.0, 1.0}   # (the bar is the median)
        em.recommend_end()
    finally:
        em.close()


# ---- 3. independence -------------------------------------------------------------------------------------------------------------
def test_a_group_does_not_depend_on_its_place_or_the_side_layout(hip):
    K, L, R, S, U, I = DENSE[1]
    data, params = random_model(U, I, R, K, L, S, 5 * U, seed=7)
    rng = np.random.default_rng(8)
    mine = rng.permutation(U)[:130].astype(np.int32)
    others = [rng.permutation(U)[:s].astype(np.int32) for s in (3, 128, 61, 9, 200)]
    alone = cat.csr([mine])
    answers = {}
    for swap in (0, 1):
        em = context(hip, data, params, U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            open_session(em, S, np.arange(1.0, R + 1), True)
            if swap == 0:
                sample = em.recommend_query(np.arange(0, U, 7, dtype=np.int32), I)[1]
                bar = float(np.median(sample[np.isfinite(sample)]))
            for mode in grp.MODES:
                want = em.recommend_query_groups(*alone, 10, mode, bar)
                assert want[2][0] == 10
                answers.setdefault(mode, want)
                same_answer(want, answers[mode], f"{mode}: swapped / unswapped")
                for name, place in (("first", 0), ("among", 3), ("last", len(others))):
                    groups = others[:place] + [mine] + others[place:]
                    got = em.recommend_query_groups(*cat.csr(groups), 10, mode, bar)
                    same_answer(tuple(a[place:place + 1] for a in got), want, f"{mode}: {name}, swap={swap}")
            em.recommend_end()
        finally:
            em.close()


@pytest.mark.parametrize("variant", VARIANTS[:2], ids=["stars", "signed"])
def test_the_answer_does_not_depend_on_the_runs(hip, variant):
    """One run for the whole request (the carry crosses every member tile: the group of all users spans three), runs of
    3 tiles, and runs of one tile with every longer group cut into fragments -- the same bits, and the reference's."""
    shape = xm.MANY[0]
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    scores = case["scores"]
    off, mem = cat.csr(request(U, xm.case_seed(*variant, shape), 0))
    for blocks, combined in ((1 << 20, False), (48, False), (16, True), (1, True), (0, None)):
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            with LaunchWindow() as lw:
                em.set_option("group_run_blocks", blocks)
                assert em.get_option("group_run_blocks") == blocks
                for exclude in (True, False):
                    seen = case["seen"] if exclude else None
                    open_session(em, S, case["w"], exclude)
                    for mode, bar in modes_and_bars(scores):
                        same_answer(em.recommend_query_groups(off, mem, 10, mode, bar),
                                    grp.group_top_n(scores, off, mem, 10, mode, bar, None, seen), f"{mode} {bar!r} blocks={blocks}")
                    em.recommend_end()
                em.close()                                 # (the log is written when the context goes)
                names = lw.names()
        finally:
            em.close()
        if combined is not None:
            assert ("grp_combine_kernel" in names) == combined, (blocks, sorted(names))
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for bad in (-1, 2.5, 2.0 ** 31):
            with pytest.raises(hip._lib.HipLibraryError) as e:
                em.set_option("group_run_blocks", bad)
            assert e.value.code == hip._lib.E_INVALID
    finally:
        em.close()


# ---- 4. exclusions that bite -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.MANY, ids=["U300", "U260"])
def test_exclusions_leave_nine_and_no_candidates(hip, shape):
    U, I, K, L, R, S = shape
    case = case_of(("mixed", "stars"), shape)
    assert case["roles"] == {0: "all", 1: "all_but", 2: "best", 3: "none"}
    seen = case["seen"]
    assert len(seen[0]) == I and len(seen[1]) == I - xm.LEFT and not seen[3]
    off, mem = cat.csr([[1, 3], [3, 0, 5], [3], []])       # all but 9 items; all of them; nothing; nobody
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        for mode in grp.MODES:
            items, vals, counts = em.recommend_query_groups(off, mem, 10, mode, 2.0)
            assert counts.tolist() == [xm.LEFT, 0, 10, 0], (mode, counts)
            assert set(items[0, :xm.LEFT].tolist()) == set(range(I)) - seen[1]
            assert (items[0, xm.LEFT:] == -1).all() and np.isneginf(vals[0, xm.LEFT:]).all()
            assert (items[[1, 3]] == -1).all() and np.isneginf(vals[[1, 3]]).all()
            if mode != "mean":
                same_answer((items, vals, counts), grp.group_top_n(case["scores"], off, mem, 10, mode, 2.0, None, seen), mode)
        em.recommend_end()
    finally:
        em.close()


# ---- 5. after recommend_add_items ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude", [True, False], ids=["train_and_new_pairs", "new_pairs_only"])
def test_after_added_items(hip, exclude):
    K, L, R, S, U, I, n_new = 6, 9, 4, 2, 300, 200, 5
    data, params = random_model(U, I, R, K, L, S, 2000, seed=21)
    rng = np.random.default_rng(22)
    eta_new = rng.random((S, n_new, L)) + 0.01
    eta_new /= eta_new.sum(axis=2, keepdims=True)           # (rows that sum to 1: random_model)
    off_new = np.concatenate([[0], np.cumsum(rng.integers(1, 40, n_new))]).astype(np.int64)
    seen_users = rng.integers(0, U, off_new[-1]).astype(np.int32)
    w = np.arange(1.0, R + 1)
    seen = seen_items(data, U) if exclude else [set() for _ in range(U)]
    for j in range(n_new):
        for u in seen_users[off_new[j]:off_new[j + 1]].tolist():
            seen[u].add(I + j)
    groups = [rng.permutation(U)[:s].astype(np.int32) for s in (1, 2, 9, 40)] + [seen_users[:1], seen_users[-1:]]
    off, mem = cat.csr(groups)
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, w, False)
        em.recommend_add_items(eta_new)
        D = user_side_matrix(em, U, I + n_new)             # every pair's device score
        em.recommend_end()
        assert np.isfinite(D).all()
        open_session(em, S, w, exclude)
        em.recommend_add_items(eta_new, (off_new, seen_users))
        bar = float(np.median(D))
        for mode, b in (("min", 0.0), ("max", 0.0), ("count", bar)):
            for n in (10, I + n_new):
                got = em.recommend_query_groups(off, mem, n, mode, b)
                same_answer(got, grp.group_top_n(D, off, mem, n, mode, b, None, seen), f"{mode} n={n}")
        whole = em.recommend_query_groups(off, mem, I + n_new, "max")
        assert (whole[0] >= I).any()                       # the added items are candidates
        assert I not in whole[0][4].tolist() and I + n_new - 1 not in whole[0][5].tolist()   # ... but not a seen one
        cand = i32([3, 50, I, I + 2, I + n_new - 1])
        same_answer(em.recommend_query_groups(off, mem, 3, "min", 0.0, cand),
                    grp.group_top_n(D, off, mem, 3, "min", 0.0, cand, seen), "candidates among the added items")
        check_mean(em.recommend_query_groups(off, mem, 10, "mean"), D, groups, 10, min(K, L) * S, w, seen, what="mean")
        em.recommend_end()
    finally:
        em.close()


# ---- 6. candidates -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(VARIANTS[0], xm.MANY[0]), (VARIANTS[1], xm.MANY[1]), (VARIANTS[2], xm.SPLIT[1])],
                         ids=["mixed-stars-U300", "mixed-signed-U260", "sorted-indicator-I5000"])
def test_candidate_subsets_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    scores = case["scores"]
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    off, mem = cat.csr(request(U, xm.case_seed(*variant, shape), 0))
    n = 10
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)
            for name, cand in candidate_sets(I, n, rng).items():
                for mode, bar in modes_and_bars(scores)[:3]:
                    got = em.recommend_query_groups(off, mem, n, mode, bar, cand)
                    same_answer(got, grp.group_top_n(scores, off, mem, n, mode, bar, cand, seen),
                                f"{name} {mode} exclude={exclude}")
            em.recommend_end()
    finally:
        em.close()


# ---- 7. random models: the members' device scores as the yardstick ---------------------------------------------------------------------
@pytest.mark.parametrize("swap", [0, 1], ids=["unswapped", "swapped"])
@pytest.mark.parametrize("shape", DENSE, ids=DENSE_ID)
def test_random_models_equal_the_aggregated_member_scores(hip, shape, swap):
    K, L, R, S, U, I = shape
    data, params = random_model(U, I, R, K, L, S, 5 * U + 50, seed=K + U)
    w = np.arange(1.0, R + 1) - (2.0 if K == 20 else 0.0)  # (one shape with weights of both signs)
    groups = request(U, U, swap)
    off, mem = cat.csr(groups)
    F = min(K, L) * S
    em = context(hip, data, params, U, I, R, swap=swap)
    try:
        open_session(em, S, w, False)
        D = user_side_matrix(em, U, I)                     # recommend_query(n = I), I <= 1,024: every pair's score
        em.recommend_end()
        assert np.isfinite(D).all()
        for exclude in (True, False):
            seen = seen_items(data, U) if exclude else None
            open_session(em, S, w, exclude)
            for mode, bar in modes_and_bars(D):
                for n in (10, min(I, 257)):
                    got = em.recommend_query_groups(off, mem, n, mode, bar)
                    same_answer(got, grp.group_top_n(D, off, mem, n, mode, bar, None, seen),
                                f"{mode} bar={bar!r} n={n} exclude={exclude}")
            check_mean(em.recommend_query_groups(off, mem, 10, "mean"), D, groups, 10, F, w, seen, what=f"exclude={exclude}")
            cand = i32(np.arange(0, I, 2))
            check_mean(em.recommend_query_groups(off, mem, 5, "mean", 0.0, cand), D, groups, 5, F, w, seen, cand, "candidates")
            em.recommend_end()
    finally:
        em.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_bad_requests_are_refused_before_any_launch(hip):
    U, I, K, L, R, S = xm.MANY[0]
    case = case_of(("mixed", "stars"), xm.MANY[0])
    lib = hip._lib
    off, mem = np.array([0, 2, 3], dtype=np.int64), i32([4, 7, 9])
    good = i32([3, 5, 8])

    def refused(call, code=lib.E_INVALID):
        with pytest.raises(lib.HipLibraryError) as e:
            call()
        assert e.value.code == code, e.value

    with LaunchWindow() as lw:
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            refused(lambda: em.recommend_query_groups(off, mem, 3, "min"))                 # no session
            em.recommend_begin(case["w"], True)
            refused(lambda: em.recommend_query_groups(off, mem, 3, "min"))                 # a session without a slot
            for s in range(S):
                em.select(s).recommend_add()
            refused(lambda: em.recommend_query_groups(np.array([1, 2, 3], dtype=np.int64), mem, 3, "min"))   # a bad CSR
            refused(lambda: em.recommend_query_groups(np.array([0, 3, 2], dtype=np.int64), mem[:2], 3, "min"))
            for bad in (-1, U):                                                            # an id out of range
                refused(lambda: em.recommend_query_groups(off, i32([4, bad, 9]), 3, "max"))
            refused(lambda: em.recommend_query_groups(off, i32([4, 4, 9]), 3, "min"))      # a repeated member
            refused(lambda: em.recommend_query_groups(np.array([0, 3], dtype=np.int64), i32([9, 4, 9]), 3, "mean"))
            for bad in (-1, 4, 17):                                                        # an unknown mode
                refused(lambda: em.recommend_query_groups(off, mem, 3, bad))
            for bad in (np.nan, np.inf, -np.inf):                                          # the bar, in COUNT mode only
                refused(lambda: em.recommend_query_groups(off, mem, 3, "count", bad))
            for bad in (i32([5, 3, 8]), i32([3, 5, 5]), i32([-1, 3, 5]), i32([3, 5, I])):  # the candidate list
                refused(lambda: em.recommend_query_groups(off, mem, 3, "min", 0.0, bad))
            refused(lambda: em.recommend_query_groups(off, mem, 0, "min"))
            refused(lambda: em.recommend_query_groups(off, mem, -2, "count", 1.0))
            refused(lambda: em.recommend_query_groups(off, mem, hip.HipEM.MAX_RECOMMEND + 1, "min"), lib.E_UNSUPPORTED)
            em.recommend_end()
            refused(lambda: em.recommend_query_groups(off, mem, 3, "min"))
        finally:
            em.close()
        names = lw.names()
        assert not [k for k in names if k.startswith(("grp_", "cat_", "rec_score", "rec_select", "rec_exclude"))], names


def test_what_is_not_refused(hip):
    """A user in two groups, no group at all, an empty group among others, a bar that is not finite outside COUNT."""
    U, I, K, L, R, S = xm.MANY[0]
    case = case_of(("mixed", "stars"), xm.MANY[0])
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], False)
        off, mem = cat.csr([[4, 7], [], [7, 4, 9], []])
        for mode in grp.MODES:
            got = em.recommend_query_groups(off, mem, 5, mode, 2.0 if mode == "count" else np.nan)
            assert got[2].tolist() == [5, 0, 5, 0]
            if mode != "mean":
                same_answer(got, grp.group_top_n(case["scores"], off, mem, 5, mode, 2.0), mode)
            none = em.recommend_query_groups(np.zeros(1, dtype=np.int64), i32([]), 5, mode, 2.0)
            assert none[0].shape == (0, 5) and none[2].shape == (0,)
        em.recommend_end()
    finally:
        em.close()


# ---- 9. no side effects -----------------------------------------------------------------------------------------------------------------
def test_queries_leave_the_context_as_it_was(hip):
    K, L, R, S, U, I = DENSE[1]
    data, params = random_model(U, I, R, K, L, S, 3000, seed=13)
    w = np.arange(1.0, R + 1)
    users, items = np.arange(U, dtype=np.int32), np.arange(I, dtype=np.int32)
    off, mem = cat.csr(request(U, 14, 0))
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
        em.similar_begin("items")
        for s in range(S):
            em.select(s).similar_add()
        near = em.similar_query(items, 5)
        open_session(em, S, w, True)
        rec = em.recommend_query(users, 10)
        for mode in grp.MODES:
            em.recommend_query_groups(off, mem, 10, mode, 3.0)
            em.recommend_query_groups(off, mem, 10, mode, 3.0, i32(np.arange(0, I, 3)))
        same_answer(em.recommend_query(users, 10), rec, "recommend_query afterwards")
        same_answer(em.similar_query(items, 5), near, "the open similar session")
        em.recommend_end()
        em.similar_end()
        after = [em.select(s).get_params() for s in range(S)]
    finally:
        em.close()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(xm.bits(a), xm.bits(b))


# ---- 10. the launch log -------------------------------------------------------------------------------------------------------------------
def test_what_each_query_launches(hip):
    U, I, K, L, R, S = xm.SPLIT[1]                         # 5,000 items: the selection is split across waves and merged
    case = case_of(("mixed", "stars"), xm.SPLIT[1])
    off, mem = cat.csr([[0, 2], [1]])
    select = ("rec_select_kernel<false>", "rec_select_kernel<true>")
    for mode, exclude, must, must_not in (
            ("min", True, (TILE_KERNELS[0], "grp_exclude_kernel") + select, ("rec_score", "rec_exclude", "cat_", "grp_mean", "grp_combine") + TILE_KERNELS[1:]),
            ("max", False, (TILE_KERNELS[1],) + select, ("rec_score", "rec_exclude", "cat_", "grp_mean", "grp_exclude") + TILE_KERNELS[::2]),
            ("count", True, (TILE_KERNELS[2], "grp_exclude_kernel") + select, ("rec_score", "rec_exclude", "cat_", "grp_mean") + TILE_KERNELS[:2]),
            ("mean", True, ("grp_mean_kernel", "rec_score_kernel", "grp_exclude_kernel") + select, ("grp_tile", "rec_exclude", "cat_")),
            ("mean", False, ("grp_mean_kernel", "rec_score_kernel") + select, ("grp_tile", "grp_exclude", "rec_exclude", "cat_"))):
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            open_session(em, S, case["w"], exclude)
            with LaunchWindow() as lw:
                em.recommend_query_groups(off, mem, 5, mode, 1.0)
                em.recommend_end()
                em.close()                                 # (the log is written when the context goes)
                names = lw.names()
        finally:
            em.close()
        assert all(k in names for k in must), (mode, must, sorted(names))
        assert not [n for n in names if n.startswith(tuple(must_not))], (mode, sorted(names))


# ---- 11. the host class, end to end -----------------------------------------------------------------------------------------------------------
def test_the_host_class_with_string_ids(hip):
    rng = np.random.default_rng(12)
    n_u, n_i, n_obs = 60, 150, 1500
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 6, iterations=8, sampling=2, seed=5)
    model.fit(df, silent=True)
    ul, il = model.data_handler.user_labels(), model.data_handler.item_labels()
    model.predict(df.iloc[:100])
    stats = model.score(silent=True)["stats"]
    groups = {"home": ["u7", "u1", "u30", "u7"], "solo": ["u2"], "nobody": [],
              "table": [f"u{j}" for j in (3, 9, 12, 40, 41, 42, 50, 51, 52, 8, 5)]}
    members = list(dict.fromkeys(u for us in groups.values() for u in us))
    # the per-member scores behind every line: rerank of the (member, item) pairs
    pairs = model.rerank([(u, i) for u in members for i in il], exclude_seen=False)
    D = pairs.pivot(index="users", columns="items", values="score").loc[members, il].to_numpy()
    assert np.isfinite(D).all()
    train = {u: set(df.loc[df["users"] == u, "items"]) for u in members}
    row = {u: j for j, u in enumerate(members)}
    w = np.asarray(model.ratings, dtype=np.float64)

    def expect(mode, bar, n, cand=None, exclude_seen=True):
        out = []
        for g, us in groups.items():
            us = list(dict.fromkeys(us))
            if not us:
                continue
            agg = grp.aggregate(D[[row[u] for u in us]], mode, bar)
            gone = set().union(*(train[u] for u in us)) if exclude_seen else set()
            keep = np.array([j for j, i in enumerate(il) if i not in gone and (cand is None or i in cand)], dtype=np.int64)
            best, vals = cat._row(agg, keep, n)
            out += [(g, il[j], v, k + 1) for k, (j, v) in enumerate(zip(best.tolist(), vals.tolist()))]
        return pd.DataFrame(out, columns=["group", "items", "score", "rank"])

    def same(got, want, exact=True, size=1):
        assert list(got.columns) == ["group", "items", "score", "rank"]
        a, b = got["score"].to_numpy(float), want["score"].to_numpy(float)
        if exact:
            for col in ("group", "items", "rank"):
                assert got[col].tolist() == want[col].tolist(), col
            assert np.array_equal(xm.bits(a), xm.bits(b))
        else:                                              # MEAN: the values within the bound, the lines' groups and ranks
            assert got["group"].tolist() == want["group"].tolist() and got["rank"].tolist() == want["rank"].tolist()
            assert np.abs(a - b).max() <= mean_bound(4 * 2, size, w)

    stock = [il[j] for j in rng.choice(len(il), 60, replace=False)]
    for aggregate, mode, bar in (("least_misery", "min", None), ("most_pleasure", "max", None),
                                 ("approval", "count", float(np.median(D)))):
        same(model.recommend_group(groups, n=5, aggregate=aggregate, bar=bar), expect(mode, bar, 5))
        same(model.recommend_group(groups, n=4, aggregate=aggregate, bar=bar, candidates=stock, exclude_seen=False),
             expect(mode, bar, 4, set(stock), False))
    frame = pd.DataFrame([(g, u) for g, us in groups.items() for u in us], columns=["group", "user"])
    same(model.recommend_group(frame, n=5), expect("min", None, 5))
    got = model.recommend_group(list(groups.values()), n=3, aggregate="most_pleasure")
    assert got["group"].unique().tolist() == [0, 1, 3]
    same(model.recommend_group(groups, n=5, aggregate="mean"), expect("mean", None, 5), exact=False, size=11)
    with pytest.raises(KeyError, match="stranger"):
        model.recommend_group({"a": ["u1", "stranger"]})
    assert len(model.recommend_group(groups, candidates=[])) == 0
    assert model.score(silent=True)["stats"] == stats


def test_every_group_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("grp_")]
    assert sorted(compiled) == sorted(NEW_KERNELS), compiled
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
