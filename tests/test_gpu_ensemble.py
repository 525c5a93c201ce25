"""Ensemble-aware queries on the device (mmsbm_hip_recommend_query_ensemble / _pair_spread, HipEM.recommend_query_ensemble
/ recommend_pair_spread, MMSBM.recommend_robust / score_spread; ensemble.hpp) against the numpy restatement of
ensemble_reference.py.  The reference INPUT is the device's own per-restart scores, obtained with existing code only:
for each slot s a recommend session that holds s alone (exclude_train = 0) answers recommend_query(n = I) -- by
candidate blocks of 1,024 items where I is larger -- scattered into a [S][U][I].

1. exact models (no rounding anywhere): MIN / MAX lists, pair_spread's worst / best / mean / per-slot values by bits, the
   mean against exact_scores where S is 2 or 4; 2. LCB and std on the same cases and on random models, against the
   restatement fed the device's a_s, within  std: 1 ulp(std),  lcb: |risk| ulp(std) + ulp(lcb)  (everything but the
   square root is restated by bits; the bound allows a one-ulp square root); 3. the restart border inside the staging
   (ranks 5 .. 33 x S 1 .. 8, 1 .. 129 rows x 1 .. 1,000 columns); 4. S = 1 and identical slots; 5. independence of
   the request, the side layout, spare slots and the batches; 6. candidates, per-row exclusions, added items;
7. pair_spread against the query; 8. refusals, side effects, the host class, the launch log.

MMSBM_E_TOOLARGE for missing device memory is the one refusal not provoked here.  The largest std / lcb errors seen are
printed by the last test (DESIGN 7r records them: 0 and 0 over 2,667,650 std values and every LCB list on an MI355X --
there the comparison is in fact by bits)."""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import ensemble_reference as ens
import exact_models as xm
from conftest import ROOT
from test_gpu_catalogue import candidate_sets, extra_lists, i32, open_session, same_answer
from test_gpu_group import random_model
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)
from test_recommend_cpu import seen_items

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW = {}
SEEN_ERR = {"std_ulps": 0.0, "lcb_over_bound": 0.0, "lcb_abs": 0.0, "values": 0}
VARIANTS = [("mixed", "stars"), ("mixed", "signed"), ("sorted", "indicator"), ("constant", "indicator")]
SHAPES = list(xm.MANY) + [xm.SPLIT[1]]
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]
NS = (1, 10, 257)
RISKS = (0.0, 1.0, -1.0, 0.5)
TILE_KERNELS = ("ens_tile_kernel<0>", "ens_tile_kernel<1>", "ens_tile_kernel<2>")
NEW_KERNELS = TILE_KERNELS + ("ens_pairs_kernel",)
BLOCK = 1024                                               # the largest n of recommend_query


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


def slot_scores(em, S, w, U, n_cat, added=None):
    """a [S][U][n_cat]: the score each slot ALONE gives every pair, from existing queries only (added: eta rows
    [S][n_new][L] appended to every one-slot session's catalogue)."""
    users = np.arange(U, dtype=np.int32)
    a = np.full((S, U, n_cat), np.nan)
    for s in range(S):
        em.recommend_begin(w, False)
        em.select(s).recommend_add()
        if added is not None:
            em.recommend_add_items(added[s:s + 1])
        for c0 in range(0, n_cat, BLOCK):
            cand = i32(np.arange(c0, min(n_cat, c0 + BLOCK)))
            if n_cat <= BLOCK:
                items, scores, counts = em.recommend_query(users, n_cat)
            else:
                items, scores, counts = em.recommend_query_within(users, len(cand), cand)
            assert (counts == len(cand)).all()
            a[s][np.repeat(users, counts), items.ravel()] = scores.ravel()
        em.recommend_end()
    assert np.isfinite(a).all()
    a.setflags(write=False)
    return a


def all_pairs(U, I):
    return i32(np.repeat(np.arange(U), I)), i32(np.tile(np.arange(I), U))


def check_spread(em, a, what=""):
    """pair_spread of every pair against the restatement: mean, worst, best and the per-slot values by bits, std within
    one ulp of the reference's.  Returns the device's stats [U][I][4]."""
    S, U, I = a.shape
    stats, each = em.recommend_pair_spread(*all_pairs(U, I), per_slot=True)
    stats, each = stats.reshape(U, I, 4), each.reshape(S, U, I)
    sp = ens.spread(a)
    assert np.array_equal(xm.bits(each), xm.bits(a)), (what, "per-slot values")
    for j, key in ((0, "mean"), (2, "worst"), (3, "best")):
        assert np.array_equal(xm.bits(stats[:, :, j]), xm.bits(sp[key])), (what, key)
    err = np.abs(stats[:, :, 1] - sp["std"]) / ens.ulp(sp["std"])
    SEEN_ERR["std_ulps"] = max(SEEN_ERR["std_ulps"], float(err.max()))
    SEEN_ERR["values"] += err.size
    assert err.max() <= 1.0, (what, "std", float(err.max()))
    assert not np.signbit(stats[:, :, 1]).any()
    return stats


def kept(I, u, b, cand, seen, extra):
    base = np.arange(I) if cand is None else np.asarray(cand, dtype=np.int64)
    out = set() if seen is None else set(seen[u])
    if extra is not None:
        out |= set(int(i) for i in extra[b])
    return base[~np.isin(base, np.fromiter(out, dtype=np.int64, count=len(out)))]


def check_lcb(got, a, users, n, risk, cand=None, seen=None, extra=None, what=""):
    """An LCB answer against the restatement fed the device's a [S][U][I]: counts, the padding, the device's own order,
    every returned value within the bound of the reference's value at the returned item, and no item left out beats the
    n-th returned by more than the bound.  risk = 0: the mean's bits."""
    items, vals, counts = got
    users = np.asarray(users, dtype=np.int64)
    sp = ens.spread(a[:, users])
    ref = ens.lcb(sp["mean"], sp["std"], risk)
    tau = abs(risk) * ens.ulp(sp["std"]) + ens.ulp(ref)
    for b, u in enumerate(users.tolist()):
        keep = kept(a.shape[2], u, b, cand, seen, extra)
        want = min(n, len(keep))
        assert counts[b] == want, (what, b, counts[b], want)
        assert (items[b, want:] == -1).all() and np.isneginf(vals[b, want:]).all()
        if want == 0:
            continue
        it, sc = items[b, :want].astype(np.int64), vals[b, :want]
        assert len(set(it.tolist())) == want and np.isin(it, keep).all(), (what, b)
        err = np.abs(sc - ref[b, it])
        SEEN_ERR["lcb_abs"] = max(SEEN_ERR["lcb_abs"], float(err.max()))
        SEEN_ERR["lcb_over_bound"] = max(SEEN_ERR["lcb_over_bound"], float((err / tau[b, it]).max()))
        assert (err <= tau[b, it]).all(), (what, b, float(err.max()))
        if risk == 0.0:
            assert np.array_equal(xm.bits(sc), xm.bits(sp["mean"][b, it])), (what, b, "risk = 0 is the mean")
        assert np.array_equal(np.lexsort((it, -sc)), np.arange(want)), (what, b)
        left = np.setdiff1d(keep, it)
        if len(left):
            assert (ref[b, left] <= sc[-1] + tau[b, left]).all(), (what, b)


def check_all_modes(em, a, users, n, cand=None, seen=None, extra=None, what="", risks=RISKS):
    """MIN and MAX by bits, LCB within the bound, for one request."""
    lists = None if extra is None else cat.csr(extra)
    for mode in ("min", "max"):
        same_answer(em.recommend_query_ensemble(users, n, mode, 0.0, cand, lists),
                    ens.top_n(a, users, n, mode, 0.0, cand, seen, extra), f"{what} {mode} n={n}")
    for risk in risks:
        check_lcb(em.recommend_query_ensemble(users, n, "lcb", risk, cand, lists), a, users, n, risk, cand, seen, extra,
                  f"{what} lcb risk={risk} n={n}")


# ---- 1. + 2. exact models: MIN / MAX / the spread by bits, LCB within the bound -----------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_exact_models(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    w = case["w"]
    exact = np.stack([xm.exact_scores([p], case["users"], I, w) for p in case["params"]])
    if variant[1] == "signed":
        assert exact.min() < 0 < exact.max()               # a maximum over negative scores: the padding trap
    few = i32([U - 1, 0, U // 2, 0][:min(U, 4)])
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        a = slot_scores(em, S, w, U, I)
        assert np.array_equal(xm.bits(a), xm.bits(exact))  # (the device's per-restart scores ARE the exact ones here)
        for exclude in (True, False):
            seen = case["seen"] if exclude else None
            open_session(em, S, w, exclude)
            for users in (case["users"], few):
                for n in NS:
                    check_all_modes(em, a, users, n, seen=seen, what=f"exclude={exclude} users={len(users)}",
                                    risks=RISKS if n == 10 else RISKS[1:2])
            if not exclude:
                stats = check_spread(em, a)
                if S in (2, 4):
                    assert np.array_equal(xm.bits(stats[:, :, 0]), xm.bits(case["scores"]))   # the mean: recommend's bits
            assert em.get_option("ensemble_ms") > 0
            em.recommend_end()
    finally:
        em.close()


# ---- 2. random models ---------------------------------------------------------------------------------------------------------
RANDOM = [(20, 20, 5, 3, 300, 300, 0), (20, 20, 5, 3, 300, 300, 1), (5, 33, 10, 2, 130, 257, 0), (50, 50, 10, 4, 65, 200, 0)]


@pytest.mark.parametrize("shape", RANDOM, ids=lambda c: "K{}L{}R{}S{}U{}I{}swap{}".format(*c))
def test_random_models(hip, shape):
    K, L, R, S, U, I, swap = shape
    data, params = random_model(U, I, R, K, L, S, 5 * U + 50, seed=K + U)
    w = np.arange(1.0, R + 1) - (2.0 if K == 20 else 0.0)  # (one shape with weights of both signs)
    users = i32(np.random.default_rng(U).permutation(U))
    em = context(hip, data, params, U, I, R, swap=swap)
    try:
        assert em.swapped == bool(swap)
        a = slot_scores(em, S, w, U, I)
        for exclude in (True, False):
            seen = seen_items(data, U) if exclude else None
            open_session(em, S, w, exclude)
            for n in (10, min(I, 257)):
                check_all_modes(em, a, users, n, seen=seen, what=f"exclude={exclude}")
            check_all_modes(em, a, users[:70], 5, i32(np.arange(0, I, 2)), seen, what="candidates")
            if not exclude:
                stats = check_spread(em, a)
                assert (stats[:, :, 1] > 0).any()
            em.recommend_end()
    finally:
        em.close()


# ---- 3. the restart border inside the staging ---------------------------------------------------------------------------------
ROWS_BY_COLUMNS = [(1, 1), (63, 127), (64, 128), (65, 129), (129, 1000), (1, 1000), (129, 1), (64, 129), (65, 127)]


@pytest.mark.parametrize("rank", [5, 7, 16, 17, 33])
def test_ranks_and_slots_around_a_staging_step(hip, rank):
    """K = L = rank, so a restart's chain is `rank` long: below a step of 16, exactly one, one and a short one, two and a
    short one.  With S restarts one after the other a step that ran on into the next restart, a short last step that was
    padded with the next restart's entries, or a padded row / column that entered a minimum or a maximum shows here.
    The rows are the request's, the columns those of the candidates' compact table (and of the whole catalogue of 1,000)."""
    U, I, R = 129, 1000, 3
    w = np.array([-1.0, 0.5, 2.0])                          # scores of both signs
    for S in (1, 2, 3, 8):
        data, params = random_model(U, I, R, rank, rank, S, 400, seed=100 * rank + S)
        em = context(hip, data, params, U, I, R)
        try:
            a = slot_scores(em, S, w, U, I)
            open_session(em, S, w, False)
            for rows, cols in ROWS_BY_COLUMNS:
                users = i32(np.arange(U - rows, U))
                cand = None if cols == I else i32(np.arange(I - cols, I))
                check_all_modes(em, a, users, 10, cand, what=f"rank={rank} S={S} {rows}x{cols}", risks=(1.0, -0.5))
            em.recommend_end()
        finally:
            em.close()


# ---- 4. one slot; identical slots ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude", [True, False], ids=["unseen", "all"])
def test_one_slot_is_recommend_query(hip, exclude):
    K, L, R, U, I = 20, 20, 5, 300, 997
    data, params = random_model(U, I, R, K, L, 1, 5 * U, seed=5)
    users = i32(np.random.default_rng(6).permutation(U))
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, 1, np.arange(1.0, R + 1), exclude)
        for n in NS:
            want = em.recommend_query(users, n)
            for mode, risk in (("min", 0.0), ("max", 0.0), ("lcb", 0.0), ("lcb", 1.0), ("lcb", -1.0), ("lcb", 0.5)):
                same_answer(em.recommend_query_ensemble(users, n, mode, risk), want, f"{mode} {risk} n={n}")
        em.recommend_end()
    finally:
        em.close()


@pytest.mark.parametrize("S", [2, 3])
def test_identical_slots_have_no_spread(hip, S):
    U, I, K, L, R, _ = xm.MANY[0]
    case = case_of(("mixed", "signed"), xm.MANY[0])
    params = [case["params"][0]] * S
    scores = xm.exact_scores(params, case["users"], I, case["w"])
    em = context(hip, case["data"], params, U, I, R)
    try:
        open_session(em, S, case["w"], True)
        stats = em.recommend_pair_spread(*all_pairs(U, I)).reshape(U, I, 4)
        assert np.array_equal(xm.bits(stats[:, :, 1]), xm.bits(np.zeros((U, I))))          # +0.0
        for j in (0, 2, 3):
            assert np.array_equal(xm.bits(stats[:, :, j]), xm.bits(scores))
        for n in NS:
            want = em.recommend_query(case["users"], n)
            for mode, risk in (("min", 0.0), ("max", 0.0), ("lcb", 1.0), ("lcb", -3.0)):
                same_answer(em.recommend_query_ensemble(case["users"], n, mode, risk), want, f"{mode} n={n}")
        em.recommend_end()
    finally:
        em.close()


# ---- 5. independence ----------------------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_the_request_the_side_layout_or_spare_slots(hip):
    K, L, R, S, U, I = 20, 20, 5, 3, 700, 300
    data, params = random_model(U, I, R, K, L, S, 5 * U, seed=7)
    _, spare = random_model(U, I, R, K, L, 2, 10, seed=8)
    rng = np.random.default_rng(9)
    mine, others = 431, i32(rng.permutation(U)[:200])
    w = np.arange(1.0, R + 1)
    answers = {}
    for name, swap, held in (("unswapped", 0, params), ("swapped", 1, params), ("spare slots", 0, params + spare)):
        em = context(hip, data, held, U, I, R, swap=swap)
        try:
            open_session(em, S, w, True)                   # (the first S slots only)
            for mode, risk in (("min", 0.0), ("max", 0.0), ("lcb", 1.0)):
                want = em.recommend_query_ensemble(i32([mine]), 10, mode, risk)
                assert want[2][0] == 10
                answers.setdefault(mode, want)
                same_answer(want, answers[mode], f"{mode}: {name}")
                for where, place in (("first", 0), ("among", 77), ("last", len(others))):
                    users = i32(np.concatenate([others[:place], [mine], others[place:]]))
                    got = em.recommend_query_ensemble(users, 10, mode, risk)
                    same_answer(tuple(x[place:place + 1] for x in got), want, f"{mode}: {where}, {name}")
            spread = em.recommend_pair_spread(i32([mine] * 10), answers["lcb"][0][0], per_slot=True)
            answers.setdefault("spread", spread)
            for x, y in zip(spread, answers["spread"]):
                assert np.array_equal(xm.bits(x), xm.bits(y)), name
            em.recommend_end()
        finally:
            em.close()


def test_three_hundred_users_over_a_hundred_thousand_items(hip):
    """Batches of 128, 128 and 44 rows, the items of a row split across waves and merged."""
    U, I, K, L, R, _ = xm.BATCHES
    S = 2
    assert xm.batch_users(I, U) == 128
    data, params = random_model(U, I, R, K, L, S, 3000, seed=12)
    w = np.array([-1.0, 0.0, 2.0])
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, w, True)
        for mode, risk in (("min", 0.0), ("max", 0.0), ("lcb", 1.0)):
            every = em.recommend_query_ensemble(np.arange(U), 10, mode, risk)
            assert (every[2] == 10).all()
            same_answer(em.recommend_query_ensemble([130], 10, mode, risk), tuple(x[130:131] for x in every), "alone")
            same_answer(em.recommend_query_ensemble(np.arange(120, 140), 10, mode, risk),
                        tuple(x[120:140] for x in every), "across the border")
            same_answer(em.recommend_query_ensemble(np.arange(U)[::-1], 10, mode, risk),
                        tuple(x[::-1] for x in every), "reversed")
            stats = em.recommend_pair_spread(np.repeat(np.arange(U), 10), every[0].ravel())
            ref = {"min": stats[:, 2], "max": stats[:, 3], "lcb": ens.lcb(stats[:, 0], stats[:, 1], risk)}[mode]
            assert np.array_equal(xm.bits(every[1].ravel()), xm.bits(ref)), mode
        em.recommend_end()
    finally:
        em.close()


# ---- 6. other routes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(VARIANTS[0], xm.MANY[0]), (VARIANTS[1], xm.MANY[1]), (VARIANTS[2], xm.SPLIT[1])],
                         ids=["mixed-stars-U300", "mixed-signed-U260", "sorted-indicator-I5000"])
def test_candidate_subsets_and_per_row_exclusions(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    again = np.arange(min(U, 7))[::-1]
    users = i32(np.concatenate([case["users"], again]))   # a user asked twice carries two lists
    n = 10
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        a = slot_scores(em, S, case["w"], U, I)
        for exclude in (True, False):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)
            for name, cand in candidate_sets(I, n, rng).items():
                check_all_modes(em, a, case["users"], n, cand, seen, what=f"{name} exclude={exclude}", risks=(1.0,))
            for cname, cand in (("null", None), ("every_other", i32(np.arange(0, I, 2))), ("block129", i32(np.arange(70, 199)))):
                lists = extra_lists(rng, users, case["scores"][users], cand, case["seen"], I)
                check_all_modes(em, a, users, n, cand, seen, lists, f"own lists {cname} exclude={exclude}", risks=(0.5,))
            em.recommend_end()
    finally:
        em.close()


@pytest.mark.parametrize("shape", xm.MANY, ids=["U300", "U260"])
def test_exclusions_leave_nine_and_no_candidates(hip, shape):
    U, I, K, L, R, S = shape
    case = case_of(("mixed", "stars"), shape)
    assert case["roles"] == {0: "all", 1: "all_but", 2: "best", 3: "none"}
    seen = case["seen"]
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        for mode in ens.MODES:
            items, vals, counts = em.recommend_query_ensemble(i32([1, 0, 3]), 10, mode, 1.0)
            assert counts.tolist() == [xm.LEFT, 0, 10], (mode, counts)
            assert set(items[0, :xm.LEFT].tolist()) == set(range(I)) - seen[1]
            assert (items[0, xm.LEFT:] == -1).all() and np.isneginf(vals[0, xm.LEFT:]).all()
            assert (items[1] == -1).all() and np.isneginf(vals[1]).all()
            none = em.recommend_query_ensemble(i32([]), 5, mode, 1.0)
            assert none[0].shape == (0, 5) and none[2].shape == (0,)
            empty = em.recommend_query_ensemble(i32([3, 4]), 5, mode, 1.0, i32([]))
            assert empty[2].tolist() == [0, 0] and (empty[0] == -1).all()
        assert em.recommend_pair_spread(i32([]), i32([])).shape == (0, 4)
        em.recommend_end()
    finally:
        em.close()


@pytest.mark.parametrize("exclude", [True, False], ids=["train_and_new_pairs", "new_pairs_only"])
def test_after_added_items(hip, exclude):
    K, L, R, S, U, I, n_new = 6, 9, 4, 2, 300, 200, 5
    data, params = random_model(U, I, R, K, L, S, 2000, seed=21)
    rng = np.random.default_rng(22)
    eta_new = rng.random((S, n_new, L)) + 0.01
    eta_new /= eta_new.sum(axis=2, keepdims=True)
    off_new = np.concatenate([[0], np.cumsum(rng.integers(1, 40, n_new))]).astype(np.int64)
    seen_users = rng.integers(0, U, off_new[-1]).astype(np.int32)
    w = np.arange(1.0, R + 1)
    seen = seen_items(data, U) if exclude else [set() for _ in range(U)]
    for j in range(n_new):
        for u in seen_users[off_new[j]:off_new[j + 1]].tolist():
            seen[u].add(I + j)
    users = i32(np.concatenate([rng.permutation(U)[:40], seen_users[:1], seen_users[-1:]]))
    em = context(hip, data, params, U, I, R)
    try:
        a = slot_scores(em, S, w, U, I + n_new, added=eta_new)
        open_session(em, S, w, exclude)
        em.recommend_add_items(eta_new, (off_new, seen_users))
        for n in (10, I + n_new):
            check_all_modes(em, a, users, n, seen=seen, what=f"n={n}", risks=(1.0,))
        whole = em.recommend_query_ensemble(users, I + n_new, "max")
        assert (whole[0] >= I).any()                       # the added items are candidates
        assert I not in whole[0][40].tolist() and I + n_new - 1 not in whole[0][41].tolist()   # ... but not a seen one
        check_all_modes(em, a, users, 3, i32([3, 50, I, I + 2, I + n_new - 1]), seen, what="candidates among the added items")
        check_spread(em, a)                                # (pairs of the added items included)
        em.recommend_end()
    finally:
        em.close()


# ---- 7. the two kernels against each other ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RANDOM[1:], ids=lambda c: "K{}L{}R{}S{}U{}I{}swap{}".format(*c))
def test_pair_spread_has_the_querys_bits(hip, shape):
    K, L, R, S, U, I, swap = shape
    data, params = random_model(U, I, R, K, L, S, 5 * U + 50, seed=K + U + 1)
    w = np.arange(1.0, R + 1) - 2.5
    users = i32(np.random.default_rng(3).permutation(U)[:100])
    em = context(hip, data, params, U, I, R, swap=swap)
    try:
        open_session(em, S, w, True)
        for cand in (None, i32(np.arange(1, I, 3))):
            for mode, risk in (("min", 0.0), ("max", 0.0)) + tuple(("lcb", r) for r in RISKS):
                items, vals, counts = em.recommend_query_ensemble(users, 10, mode, risk, cand)
                keep = np.arange(10)[None, :] < counts[:, None]
                stats = em.recommend_pair_spread(np.repeat(users, counts), items[keep])
                ref = {"min": stats[:, 2], "max": stats[:, 3], "lcb": ens.lcb(stats[:, 0], stats[:, 1], risk)}[mode]
                assert np.array_equal(xm.bits(vals[keep]), xm.bits(ref)), (mode, risk)
        em.recommend_end()
    finally:
        em.close()


# ---- 8. refusals, side effects, the host class, coverage ----------------------------------------------------------------------
def test_bad_requests_are_refused_before_any_launch(hip):
    U, I, K, L, R, S = xm.MANY[0]
    case = case_of(("mixed", "stars"), xm.MANY[0])
    lib = hip._lib
    users, good = i32([4, 7, 9]), i32([3, 5, 8])
    off = np.array([0, 1, 1, 2], dtype=np.int64)

    def refused(call, code=lib.E_INVALID):
        with pytest.raises(lib.HipLibraryError) as e:
            call()
        assert e.value.code == code, e.value

    with LaunchWindow() as lw:
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            refused(lambda: em.recommend_query_ensemble(users, 3, "min"))                  # no session
            refused(lambda: em.recommend_pair_spread(users, good))
            em.recommend_begin(case["w"], True)
            refused(lambda: em.recommend_query_ensemble(users, 3, "min"))                  # a session without a slot
            refused(lambda: em.recommend_pair_spread(users, good))
            for s in range(S):
                em.select(s).recommend_add()
            for bad in (-1, U):                                                            # an id out of range
                refused(lambda: em.recommend_query_ensemble(i32([4, bad, 9]), 3, "max"))
                refused(lambda: em.recommend_pair_spread(i32([4, bad, 9]), good))
            for bad in (-1, I):
                refused(lambda: em.recommend_pair_spread(users, i32([3, bad, 8])))
                refused(lambda: em.recommend_query_ensemble(users, 3, "min", 0.0, None, (off, i32([3, bad]))))
            for bad in (i32([5, 3, 8]), i32([3, 5, 5]), i32([-1, 3, 5]), i32([3, 5, I])):  # the candidate list
                refused(lambda: em.recommend_query_ensemble(users, 3, "min", 0.0, bad))
            refused(lambda: em.recommend_query_ensemble(users, 3, "lcb", 1.0, None, (np.array([1, 1, 1, 2], dtype=np.int64), good[:2])))
            refused(lambda: em.recommend_query_ensemble(users, 3, "lcb", 1.0, None, (np.array([0, 2, 1, 2], dtype=np.int64), good[:2])))
            for bad in (0, -2):
                refused(lambda: em.recommend_query_ensemble(users, bad, "min"))
            for bad in (-1, 3, 17):                                                        # an unknown mode
                refused(lambda: em.recommend_query_ensemble(users, 3, bad))
            for bad in (np.nan, np.inf, -np.inf):                                          # the risk, in LCB mode only
                refused(lambda: em.recommend_query_ensemble(users, 3, "lcb", bad))
            refused(lambda: em.recommend_query_ensemble(users, hip.HipEM.MAX_RECOMMEND + 1, "min"), lib.E_UNSUPPORTED)
            em.recommend_end()
            refused(lambda: em.recommend_query_ensemble(users, 3, "min"))
        finally:
            em.close()
        names = lw.names()
        assert not [k for k in names if k.startswith(("ens_", "cat_", "rec_score", "rec_select", "rec_exclude"))], names


def test_what_is_not_refused_and_what_each_query_launches(hip):
    U, I, K, L, R, S = xm.SPLIT[1]                         # 5,000 items: the selection is split across waves and merged
    case = case_of(("mixed", "stars"), xm.SPLIT[1])
    select = ("rec_select_kernel<false>", "rec_select_kernel<true>")
    lists = cat.csr([[5], []])
    for mode, exclude, cand, own, must, must_not in (
            ("min", True, None, None, (TILE_KERNELS[0], "rec_exclude_kernel") + select, ("rec_score", "cat_", "ens_pairs") + TILE_KERNELS[1:]),
            ("max", False, None, None, (TILE_KERNELS[1],) + select, ("rec_score", "rec_exclude", "cat_", "ens_pairs") + TILE_KERNELS[::2]),
            ("lcb", True, i32(np.arange(0, I, 2)), lists, (TILE_KERNELS[2], "cat_gather_kernel", "cat_cols_kernel", "cat_exclude_kernel") + select,
             ("rec_score", "rec_exclude", "ens_pairs") + TILE_KERNELS[:2])):
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            open_session(em, S, case["w"], exclude)
            with LaunchWindow() as lw:
                got = em.recommend_query_ensemble(i32([1, 2]), 5, mode, np.nan if mode != "lcb" else 1.0, cand, own)
                assert got[2].tolist() == [5, 5]           # (a risk that is not finite is read by LCB alone)
                em.recommend_end()
                em.close()                                 # (the log is written when the context goes)
                names = lw.names()
        finally:
            em.close()
        assert all(k in names for k in must), (mode, must, sorted(names))
        assert not [k for k in names if k.startswith(tuple(must_not))], (mode, sorted(names))
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        with LaunchWindow() as lw:
            em.recommend_pair_spread(i32([0, 2, 0]), i32([7, 7, I - 1]))
            assert em.get_option("ensemble_ms") > 0
            em.recommend_end()
            em.close()
            names = lw.names()
    finally:
        em.close()
    assert "ens_pairs_kernel" in names                     # ... and no row of scores is formed
    assert not [k for k in names if k.startswith(("ens_tile", "rec_score", "rec_select", "rec_exclude", "cat_"))], sorted(names)


def test_queries_leave_the_context_as_it_was(hip):
    K, L, R, S, U, I = 20, 20, 5, 3, 700, 300
    data, params = random_model(U, I, R, K, L, S, 3000, seed=13)
    w = np.arange(1.0, R + 1)
    users, items = np.arange(U, dtype=np.int32), np.arange(I, dtype=np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(x.copy() for x in em.select(s).get_params()) for s in range(S)]
        em.similar_begin("items")
        for s in range(S):
            em.select(s).similar_add()
        near = em.similar_query(items, 5)
        open_session(em, S, w, True)
        rec = em.recommend_query(users, 10)
        for mode in ens.MODES:
            em.recommend_query_ensemble(users, 10, mode, 1.0)
            em.recommend_query_ensemble(users, 10, mode, 1.0, i32(np.arange(0, I, 3)), cat.csr([[u % I] for u in users]))
        em.recommend_pair_spread(users[:I], items, per_slot=True)
        same_answer(em.recommend_query(users, 10), rec, "recommend_query afterwards")
        same_answer(em.similar_query(items, 5), near, "the open similar session")
        em.recommend_end()
        em.similar_end()
        after = [em.select(s).get_params() for s in range(S)]
    finally:
        em.close()
    for x, y in zip(before, after):
        for p, q in zip(x, y):
            assert np.array_equal(xm.bits(p), xm.bits(q))


def test_the_host_class_with_string_ids(hip):
    rng = np.random.default_rng(12)
    n_u, n_i, n_obs = 60, 150, 1500
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 6, iterations=8, sampling=3, seed=5)
    model.fit(df, silent=True)
    il = model.data_handler.item_labels()
    model.predict(df.iloc[:100])
    stats = model.score(silent=True)["stats"]
    users = ["u7", "u1", "u30", "u7"]
    people = list(dict.fromkeys(users))
    # the per-restart scores behind every line: score_spread of every (user, item) pair
    spread = model.score_spread([(u, i) for u in people for i in il], per_restart=True)
    assert list(spread.columns) == ["users", "items", "mean", "std", "worst", "best", "restart_0", "restart_1", "restart_2"]
    a = np.stack([spread[f"restart_{s}"].to_numpy().reshape(len(people), len(il)) for s in range(3)])
    sp = ens.spread(a)
    for key in ("mean", "worst", "best"):
        assert np.array_equal(xm.bits(spread[key].to_numpy()), xm.bits(sp[key].ravel())), key
    assert (np.abs(spread["std"].to_numpy() - sp["std"].ravel()) <= ens.ulp(sp["std"].ravel())).all()
    # one restart alone is what recommend's score is in a model of that restart: the mean is close to recommend's score
    plain = model.rerank([(u, i) for u in people for i in il], exclude_seen=False)
    mean = plain.pivot(index="users", columns="items", values="score").loc[people, il].to_numpy()
    assert np.abs(mean - sp["mean"]).max() <= 64 * 2.0 ** -53 * 5.0
    train = {u: set(df.loc[df["users"] == u, "items"]) for u in people}
    row = {u: j for j, u in enumerate(people)}
    stock = [il[j] for j in rng.choice(len(il), 60, replace=False)]
    shown = [("u7", stock[0]), ("u1", stock[1]), ("u55", stock[2])]
    for aggregate, mode, risk in (("lcb", "lcb", 1.0), ("lcb", "lcb", -0.5), ("worst", "min", 1.0), ("best", "max", 1.0)):
        for kw, cand, own, exclude_seen in (({}, None, (), True),
                                            ({"candidates": stock, "exclude": shown, "exclude_seen": False}, set(stock), shown, False)):
            got = model.recommend_robust(users, n=5, aggregate=aggregate, risk=risk, **kw)
            assert list(got.columns) == ["users", "items", "score", "mean", "std", "rank"]
            assert got["users"].tolist() == [u for u in users for _ in range(5)] and got["rank"].tolist() == [1, 2, 3, 4, 5] * 4
            value = ens.aggregate(a, mode, risk)
            for u, part in got.groupby("users", sort=False):
                gone = (train[u] if exclude_seen else set()) | {i for u2, i in own if u2 == u}
                keep = [j for j, i in enumerate(il) if i not in gone and (cand is None or i in cand)]
                it = [il.index(i) for i in part["items"].tolist()[:5]]
                assert set(it) <= set(keep)
                sc = part["score"].to_numpy()[:5]
                tau = abs(risk) * ens.ulp(sp["std"][row[u], it]) + ens.ulp(value[row[u], it])
                assert (np.abs(sc - value[row[u], it]) <= tau).all(), (aggregate, u)
                assert np.array_equal(np.lexsort((it, -sc)), np.arange(5))
                left = np.setdiff1d(keep, it)
                assert (value[row[u], left] <= sc[-1] + abs(risk) * ens.ulp(sp["std"][row[u], left]) + ens.ulp(value[row[u], left])).all()
                assert np.array_equal(xm.bits(part["mean"].to_numpy()[:5]), xm.bits(sp["mean"][row[u], it]))
    with pytest.raises(KeyError, match="stranger"):
        model.recommend_robust(["u1", "stranger"])
    with pytest.raises(ValueError, match="risk belongs"):
        model.recommend_robust(["u1"], aggregate="worst", risk=2.0)
    assert len(model.recommend_robust(users, candidates=[])) == 0
    assert model.score(silent=True)["stats"] == stats


def test_every_ensemble_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("ens_")]
    assert sorted(compiled) == sorted(NEW_KERNELS), compiled
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
    print("ensemble errors seen:", SEEN_ERR)
