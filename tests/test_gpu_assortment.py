"""Greedy assortment selection on the device (mmsbm_hip_recommend_assortment, HipEM.recommend_assortment,
MMSBM.assortment / assortment_value; assortment.hpp) against the numpy greedy of assortment_reference.py:

1. by EQUALITY on models without rounding (exact_models): both objectives, c in {0, 1, 12}, user subsets either side of a
   block and a step, with and without exclusions, with given items, candidate subsets, bars on an occurring score, below
   every score and above every score;
2. two forced run lengths and forced batches of item tiles: the same bits; 3. the edge users; 4. random models: the walk
   along the device's own picks over the device scores (reach by equality, best score within the derived bound);
5. cross-checks with assortment_value, audience and recommend; 6. refusals by status code, no side effects, the launch
   log, the host class end to end with string ids.

MMSBM_E_TOOLARGE for missing device memory is the one refusal not provoked here."""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

import assortment_reference as ar
import exact_models as xm
from conftest import ROOT
from test_assortment_cpu import numerators
from test_gpu_audience import user_side_matrix
from test_gpu_catalogue import candidate_sets, i32, open_session, same_answer
from test_gpu_group import random_model
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)
from test_recommend_cpu import seen_items

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW = {}
VARIANTS = [("mixed", "stars"), ("mixed", "signed"), ("sorted", "indicator"), ("constant", "indicator")]
CASES = [(v, s) for v in VARIANTS for s in xm.MANY]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]
SIZES = (1, 7, 8, 9, 127, 128, 129)                        # either side of a block of 8 rows and a step of 128
OBJECTIVES = ("best_score", "reach")
NEW_KERNELS = ("asrt_gain_kernel<0>", "asrt_gain_kernel<1>", "asrt_update_kernel<0>", "asrt_update_kernel<1>",
               "asrt_join_kernel", "asrt_pick_kernel", "asrt_given_kernel", "asrt_finish_kernel")


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


@functools.lru_cache(maxsize=None)
def case_of(variant, shape):
    """The session's inputs, exact scores and exact accumulators: computed once, shared by the tests, never written to."""
    case = xm.make_case(*variant, shape)
    case["A"] = numerators(case)
    for k in ("A", "scores"):
        case[k].setflags(write=False)
    return case


def levels_of(case, objective):
    """best_score: the default floor and one inside the scores; reach: an occurring score (`>=` takes its whole tie
    group), a bar below every score and one above every score (stops at once with "no_gain")."""
    sc = case["scores"]
    if objective == "best_score":
        return (float(np.min(case["w"])), float(np.sort(sc, axis=None)[sc.size // 2]))
    return (float(np.sort(sc, axis=None)[3 * sc.size // 4]), float(sc.min()) - 1.0, float(sc.max()) + 1.0)


def same_result(got, want, users, what):
    """The device's answer for the request `users` (any order) against the reference's over the sorted users."""
    items, gains, n, stop, s_items, s_scores, start = got
    assert n == len(items) == len(gains) == len(want["items"]) and stop == want["stop"], (what, n, stop, want["stop"], items, want["items"])
    assert items.tolist() == want["items"].tolist(), (what, items, want["items"])
    assert np.array_equal(xm.bits(gains), xm.bits(want["gains"])), (what, gains, want["gains"])
    assert xm.bits(start) == xm.bits(want["start"]), (what, start, want["start"])
    place = np.searchsorted(np.sort(users), users)
    ref_items, ref_scores = np.full(len(users), -1, dtype=np.int64), np.full(len(users), -np.inf)
    rows, it, sc = want["served"]
    ref_items[rows], ref_scores[rows] = it, sc
    assert s_items.tolist() == ref_items[place].tolist(), what
    assert np.array_equal(xm.bits(s_scores), xm.bits(ref_scores[place])), what


# ---- 1. exact models, by equality ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_exact_models_by_equality(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    A = case["A"]
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    everyone = rng.permutation(U).astype(np.int32)
    subsets = [rng.permutation(U)[:s].astype(np.int32) for s in SIZES] + [everyone]
    held = i32([I // 2, 3, I - 1])                          # the middle, the first tile and the last, partial tile
    cands = candidate_sets(I, 10, rng)
    stopped = set()
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)

            def check(users, c, objective, level, given=None, cand=None, what=""):
                got = em.recommend_assortment(users, c, objective, level, given, cand)
                want = ar.greedy(A, c, objective, level, S, np.sort(users), seen, [] if given is None else given.tolist(), cand)
                same_result(got, want, users, f"{objective} level={level!r} c={c} exclude={exclude} {what}")
                stopped.add(want["stop"])
                return got

            for objective in OBJECTIVES:
                levels = levels_of(case, objective)
                for level in levels:
                    for c in (0, 1, 12):
                        check(everyone, c, objective, level)
                    check(everyone, 12, objective, level, held, what="given")
                    check(everyone, 0, objective, level, held, what="given, c = 0")
                for users in subsets:
                    check(users, 12, objective, levels[0], what=f"{len(users)} users")
                for name, cand in cands.items():
                    got = check(everyone, 12, objective, levels[0], None, cand, name)
                    check(everyone, 3, objective, levels[0], held, cand, name + ", given")   # (given need not be candidates)
                    assert np.isin(got[0], cand).all()
                if objective == "reach":
                    assert check(everyone, 12, objective, levels[2])[3] == "no_gain"       # above every score: at once
            assert em.get_option("assortment_ms") > 0
            em.recommend_end()
    finally:
        em.close()
    assert stopped == {"c", "no_gain", "no_candidates"}, stopped


# ---- 2. the answer does not depend on the runs or the batches ------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS[:2], ids=["stars", "signed"])
def test_two_forced_run_lengths_and_forced_batches(hip, variant):
    """One run with a carry over every step (300 users: three steps), runs of one step each whose rows meet in
    asrt_join_kernel, and a partial buffer of two item tiles a run (four batches a round): the same bits on exact
    models, and the reference's."""
    shape = xm.MANY[0]
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users = np.arange(U, dtype=np.int32)
    held = i32([5, 600])
    answers = {}
    for blocks, part in ((1 << 20, 0), (16, 0), (16, 3 * 256 * 8), (0, 0)):
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            em.set_option("assortment_run_blocks", blocks)
            em.set_option("assortment_part_bytes", part)
            assert em.get_option("assortment_run_blocks") == blocks and em.get_option("assortment_part_bytes") == part
            open_session(em, S, case["w"], True)
            for objective in OBJECTIVES:
                level = levels_of(case, objective)[0]
                got = em.recommend_assortment(users, 12, objective, level, held)
                same_result(got, ar.greedy(case["A"], 12, objective, level, S, users, case["seen"], held.tolist()), users,
                            f"{objective} blocks={blocks} part={part}")
                first = answers.setdefault(objective, got)
                assert got[0].tolist() == first[0].tolist() and np.array_equal(xm.bits(got[1]), xm.bits(first[1]))
            em.recommend_end()
            for bad in (-1, 2.5, 2.0 ** 31):
                with pytest.raises(hip._lib.HipLibraryError) as e:
                    em.set_option("assortment_run_blocks", bad)
                assert e.value.code == hip._lib.E_INVALID
        finally:
            em.close()


# ---- 3. the edge users ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.MANY, ids=["U300", "U260"])
def test_a_user_without_an_unseen_candidate_contributes_nothing(hip, shape):
    U, I, K, L, R, S = shape
    case = case_of(("mixed", "stars"), shape)
    assert case["roles"] == {0: "all", 1: "all_but", 2: "best", 3: "none"}
    seen, A = case["seen"], case["A"]
    floor = float(np.min(case["w"]))
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        for objective, level in (("best_score", floor), ("reach", float(case["scores"].min()) - 1.0)):
            items, gains, n, stop, s_items, s_scores, start = em.recommend_assortment(i32([0]), 5, objective, level)
            assert (n, stop, s_items.tolist(), start) == (0, "no_gain", [-1], 0.0) and np.isneginf(s_scores).all()
            items, gains, n, stop, s_items, s_scores, _ = em.recommend_assortment(i32([1]), 12, objective, level)
            assert set(items.tolist()) <= set(range(I)) - seen[1] and 1 <= n <= xm.LEFT and stop == "no_gain"
            for users in (i32([0, 1, 2, 3]), i32([3, 7, 0])):
                same_result(em.recommend_assortment(users, 12, objective, level),
                            ar.greedy(A, 12, objective, level, S, np.sort(users), seen), users, objective)
                with_0 = em.recommend_assortment(users, 12, objective, level)
                without = em.recommend_assortment(users[users != 0], 12, objective, level)
                assert with_0[0].tolist() == without[0].tolist() and np.array_equal(xm.bits(with_0[1]), xm.bits(without[1]))
        em.recommend_end()
    finally:
        em.close()


# ---- 4. random models: the walk along the device's own picks ------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3], ids=["S1", "S3"])
def test_random_models_follow_the_device_scores(hip, S):
    U, I, R, K, L = 300, 500, 5, 7, 9
    data, params = random_model(U, I, R, K, L, S, 5 * U + 50, seed=40 + S)
    w = np.arange(1.0, R + 1)
    rng = np.random.default_rng(41 + S)
    requests = [np.arange(U, dtype=np.int32), rng.permutation(U)[:129].astype(np.int32)]
    held = i32([17, 400])
    cand = i32(np.arange(0, I, 3))
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, w, False)
        D = user_side_matrix(em, U, I)                     # recommend_query(n = I), I <= 1,024: every pair's score
        em.recommend_end()
        assert np.isfinite(D).all()
        bar = float(np.quantile(D, 0.98))
        for exclude in (True, False):
            seen = seen_items(data, U) if exclude else None
            open_session(em, S, w, exclude)
            for users in requests:
                rows = np.sort(users)
                place = np.searchsorted(rows, users)
                tau = ar.gain_bound(len(users), w)
                for objective, level in (("reach", bar), ("best_score", float(w.min()))):
                    for given, cd in (((), None), (held.tolist(), cand)):
                        c = 12
                        items, gains, n, stop, s_items, s_scores, start = em.recommend_assortment(
                            users, c, objective, level, i32(given) if given else None, cd)
                        st = ar.walk(D, objective, level, rows, seen, given, cd, items, gains, stop, c, tau)
                        assert n >= 2
                        # served: read from the device state -- the scores are D's, bit for bit
                        got = s_items >= 0
                        assert np.array_equal(xm.bits(s_scores[got]), xm.bits(D[users[got], s_items[got]]))
                        assert np.isneginf(s_scores[~got]).all()
                        if objective == "reach":
                            assert s_items.tolist() == st.served[place].tolist()
                            assert start == ar.greedy(D, 0, objective, level, 1, rows, seen, given)["start"]
                        else:
                            ref = st.served[place] >= 0    # (a user at the floor's rounding border may be on one side only)
                            assert (got | ~ref).all() and (s_scores[got & ~ref] == level).all()
                            assert np.array_equal(s_scores[got & ref], st.best[place][got & ref])
                            assert abs(start - ar.greedy(D, 0, objective, level, 1, rows, seen, given)["start"]) <= len(given) * tau
            em.recommend_end()
    finally:
        em.close()


# ---- 5. cross-checks -------------------------------------------------------------------------------------------------------------------
def test_cross_checks_with_value_audience_and_recommend(hip):
    U, I, R, K, L, S = 300, 500, 5, 7, 9, 3
    data, params = random_model(U, I, R, K, L, S, 5 * U + 50, seed=52)
    w = np.arange(1.0, R + 1)
    users = np.arange(U, dtype=np.int32)
    held = i32([9, 250])
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, w, True)
        sample = em.recommend_query(users[::7], I)[1]
        bar = float(np.quantile(sample[np.isfinite(sample)], 0.98))
        for objective, level in (("best_score", 1.0), ("reach", bar)):
            items, gains, n, stop, s_items, s_scores, start = em.recommend_assortment(users, 8, objective, level, held)
            assert n == 8 and stop == "c"
            # the chosen items valued as a set somebody else picked: the same state, the same total
            v = em.recommend_assortment(users, 0, objective, level, np.concatenate([held, items]))
            assert v[2] == 0 and v[3] == "c" and v[4].tolist() == s_items.tolist()
            assert np.array_equal(xm.bits(v[5]), xm.bits(s_scores))
            # ... and by bits: a column's sum is the same additions whether the item is given or chosen, and `start` is
            # the running sum in the same order (the host forms `value` from it as it does from the rounds' total)
            assert xm.bits(v[6]) == xm.bits(float(np.cumsum(np.concatenate([[start], gains]))[-1]))
            plain = em.recommend_assortment(users, 8, objective, level)
            valued = em.recommend_assortment(users, 0, objective, level, plain[0])
            assert xm.bits(valued[6]) == xm.bits(float(np.cumsum(plain[1])[-1])) and valued[4].tolist() == plain[4].tolist()
            whole = np.sort(np.concatenate([held, items])).astype(np.int32)
            got = s_items >= 0
            if objective == "reach":
                assert v[6] == start + gains.sum() == got.sum()
                off, au, _ = em.recommend_audience(whole, bar)
                assert sorted(set(au.tolist())) == users[got].tolist()
            else:
                top = em.recommend_query_within(users, 1, whole)
                assert np.array_equal(top[2] > 0, got)
                assert np.array_equal(xm.bits(top[1][got, 0]), xm.bits(s_scores[got]))
        em.recommend_end()
    finally:
        em.close()


# ---- 6. hygiene ------------------------------------------------------------------------------------------------------------------------
def test_bad_requests_are_refused_before_any_launch(hip):
    U, I, K, L, R, S = xm.MANY[0]
    case = case_of(("mixed", "stars"), xm.MANY[0])
    lib = hip._lib
    users = i32([4, 7, 9])

    def refused(call, code=lib.E_INVALID):
        with pytest.raises(lib.HipLibraryError) as e:
            call()
        assert e.value.code == code, e.value

    def raw(users, mode=0, level=1.0, given=(), cand=None, c=3):
        """The C entry itself (HipEM.recommend_assortment sorts the users before it calls)."""
        import ctypes as C
        u, g = i32(users), i32(given)
        cd = None if cand is None else i32(cand)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))    # noqa: E731
        out_i, out_g = np.zeros(max(c, 1), dtype=np.int32), np.zeros(max(c, 1))
        cnt, stop = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        gg, si, ss = np.zeros(max(len(g), 1)), np.zeros(max(len(u), 1), dtype=np.int32), np.zeros(max(len(u), 1))
        lib.call("mmsbm_hip_recommend_assortment", em._h, len(u), p(u, C.c_int32), mode, float(level), len(g), p(g, C.c_int32),
                 0 if cd is None else len(cd), None if cd is None else p(cd, C.c_int32), c, p(out_i, C.c_int32),
                 p(out_g, C.c_double), p(cnt, C.c_int32), p(stop, C.c_int32), p(gg, C.c_double), p(si, C.c_int32),
                 p(ss, C.c_double))

    with LaunchWindow() as lw:
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            refused(lambda: em.recommend_assortment(users, 3, "best_score", 1.0))          # no session
            em.recommend_begin(case["w"], True)
            refused(lambda: em.recommend_assortment(users, 3, "best_score", 1.0))          # a session without a slot
            for s in range(S):
                em.select(s).recommend_add()
            for bad in (-1, U):                                                            # an unknown user
                refused(lambda: em.recommend_assortment(i32([4, bad, 9]), 3, "reach", 1.0))
            refused(lambda: raw([7, 4, 9]))                                                # users not ascending / repeated
            refused(lambda: raw([4, 4, 9]))
            for bad in (-1, 2, 17):                                                        # an unknown mode
                refused(lambda: em.recommend_assortment(users, 3, bad, 1.0))
            for bad in (np.nan, np.inf, -np.inf):                                          # the floor and the bar
                for mode in OBJECTIVES:
                    refused(lambda: em.recommend_assortment(users, 3, mode, bad))
            for bad in (-1, I):                                                            # an unknown given item
                refused(lambda: em.recommend_assortment(users, 3, "best_score", 1.0, i32([3, bad])))
            for bad in (i32([5, 3, 8]), i32([3, 5, 5]), i32([-1, 3, 5]), i32([3, 5, I])):  # the candidate list
                refused(lambda: em.recommend_assortment(users, 3, "best_score", 1.0, None, bad))
            refused(lambda: em.recommend_assortment(users, -1, "best_score", 1.0))
            refused(lambda: em.recommend_assortment(users, hip.HipEM.MAX_ASSORT + 1, "reach", 1.0), lib.E_UNSUPPORTED)
            em.recommend_end()
            refused(lambda: em.recommend_assortment(users, 3, "best_score", 1.0))
        finally:
            em.close()
        names = lw.names()
        assert not [k for k in names if k.startswith(("asrt_", "cat_", "rec_score", "rec_select"))], names


def test_queries_leave_the_session_as_it_was(hip):
    U, I, R, K, L, S = 300, 500, 5, 7, 9, 3
    data, params = random_model(U, I, R, K, L, S, 3000, seed=13)
    w = np.arange(1.0, R + 1)
    users = np.arange(U, dtype=np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
        open_session(em, S, w, True)
        rec = em.recommend_query(users, 10)
        first = em.recommend_assortment(users, 10, "best_score", 1.0)
        em.recommend_assortment(users, 10, "reach", 3.0, i32([1, 2]), i32(np.arange(0, I, 3)))
        again = em.recommend_assortment(users, 10, "best_score", 1.0)          # the same bits from call to call
        assert first[0].tolist() == again[0].tolist() and np.array_equal(xm.bits(first[1]), xm.bits(again[1]))
        same_answer(em.recommend_query(users, 10), rec, "recommend_query afterwards")
        em.recommend_end()
        after = [em.select(s).get_params() for s in range(S)]
    finally:
        em.close()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(xm.bits(a), xm.bits(b))


def test_what_a_query_launches_and_that_nothing_works_behind_the_stop(hip):
    """c = 12 rounds are enqueued whatever happens; a query that stops after k rounds answers exactly as the same query
    asked for k rounds -- items, gains and the state read back at the end -- so the launches behind the stop flag did
    nothing.  With the split timing on, the phases' times are read."""
    U, I, K, L, R, S = xm.MANY[0]
    case = case_of(("sorted", "indicator"), xm.MANY[0])
    users = np.arange(U, dtype=np.int32)
    for objective, level in (("best_score", float(np.min(case["w"]))), ("reach", levels_of(case, "reach")[0])):
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            em.set_option("assortment_timing", 1)
            open_session(em, S, case["w"], True)
            with LaunchWindow() as lw:
                long = em.recommend_assortment(users, 12, objective, level, i32([4]))
                split = [em.get_option(f"assortment_{k}_ms") for k in ("gain", "pick", "update")]
                k = long[2]
                assert 1 <= k < 12 and long[3] == "no_gain"                    # (a block family: a few rounds, then ties at 0)
                short = em.recommend_assortment(users, k, objective, level, i32([4]))
                assert short[3] == "c" and short[0].tolist() == long[0].tolist()
                assert np.array_equal(xm.bits(short[1]), xm.bits(long[1])) and short[4].tolist() == long[4].tolist()
                assert np.array_equal(xm.bits(short[5]), xm.bits(long[5]))
                em.recommend_end()
                em.close()                                 # (the log is written when the context goes)
                names = lw.names()
        finally:
            em.close()
        assert all(t > 0 for t in split), split
        mode = OBJECTIVES.index(objective)
        must = (f"asrt_gain_kernel<{mode}>", f"asrt_update_kernel<{mode}>", "asrt_join_kernel", "asrt_pick_kernel",
                "asrt_given_kernel", "asrt_finish_kernel")
        assert all(m in names for m in must), (objective, sorted(names))
        assert not [n for n in names if n.startswith(("rec_score", "rec_select", "cat_", "grp_", f"asrt_gain_kernel<{1 - mode}>"))], sorted(names)


def test_the_host_class_with_string_ids(hip):
    rng = np.random.default_rng(12)
    n_u, n_i, n_obs = 60, 150, 1500
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 6, iterations=8, sampling=2, seed=5)
    model.fit(df, silent=True)
    ul, il = list(model.data_handler.user_labels()), list(model.data_handler.item_labels())
    model.predict(df.iloc[:100])
    stats = model.score(silent=True)["stats"]
    pairs = model.rerank([(u, i) for u in ul for i in il], exclude_seen=False)
    D = pairs.pivot(index="users", columns="items", values="score").loc[ul, il].to_numpy()
    assert np.isfinite(D).all()
    seen = [set(il.index(i) for i in df.loc[df["users"] == u, "items"]) for u in ul]
    w = np.asarray(model.ratings, dtype=np.float64)
    bar = float(np.quantile(D, 0.9))
    # reach: equality with the numpy greedy over the device scores
    got = model.assortment(c=6, objective="reach", bar=bar, given=["item-3"])
    want = ar.greedy(D, 6, "reach", bar, 1, None, seen, [il.index("item-3")])
    assert list(got.columns) == ["items", "gain", "total", "rank"] and got["rank"].tolist() == list(range(1, len(got) + 1))
    assert got["items"].tolist() == [il[i] for i in want["items"]] and got["gain"].tolist() == want["gains"].tolist()
    a = model.assortment_
    assert (a["rounds"], a["stopped"], a["users"], a["bar"], a["start"]) == (len(got), want["stop"], len(ul), bar, want["start"])
    assert a["value"] == want["value"] == len(a["served"]) / len(ul)
    rows, it, sc = want["served"]
    assert a["served"]["users"].tolist() == [ul[r] for r in rows] and a["served"]["items"].tolist() == [il[i] for i in it]
    assert np.array_equal(xm.bits(a["served"]["score"]), xm.bits(sc))
    chosen = ["item-3"] + got["items"].tolist()
    reached = model.audience(items=chosen, min_score=bar)
    assert sorted(set(reached["users"])) == sorted(a["served"]["users"])
    worth = model.assortment_value(chosen, objective="reach", bar=bar)
    assert worth["value"] == a["value"] and worth["served"].equals(a["served"])
    # best score: the walk over the device scores, and the cross-checks by bits
    some = [f"u{j}" for j in (7, 1, 30, 7, 2, 3, 9, 12, 40, 41)]
    stock = [il[j] for j in rng.choice(len(il), 60, replace=False)]
    got = model.assortment(c=5, users=some, candidates=stock)
    a = model.assortment_
    rows = np.asarray(sorted({ul.index(u) for u in some}))
    cand = np.asarray(sorted(il.index(i) for i in stock))
    tau = ar.gain_bound(len(rows), w)
    ar.walk(D, "best_score", float(w.min()), rows, seen, (), cand, [il.index(i) for i in got["items"]], got["gain"].to_numpy(),
            a["stopped"], 5, tau)
    assert set(got["items"]) <= set(stock) and a["users"] == 9 and a["floor"] == float(w.min())
    assert np.array_equal(xm.bits(got["total"]), xm.bits(np.cumsum(got["gain"].to_numpy())))
    assert xm.bits(a["value"]) == xm.bits(a["floor"] + (a["start"] + got["total"].iloc[-1]) / 9)
    worth = model.assortment_value(got["items"].tolist(), users=some)
    assert xm.bits(worth["value"]) == xm.bits(a["value"]) and worth["served"].equals(a["served"])
    top = model.recommend(users=a["served"]["users"].tolist(), n=1, candidates=got["items"].tolist())
    assert top["users"].tolist() == a["served"]["users"].tolist()
    assert np.array_equal(xm.bits(top["score"]), xm.bits(a["served"]["score"]))
    with pytest.raises(KeyError, match="stranger"):
        model.assortment(users=["u1", "stranger"])
    with pytest.raises(ValueError, match="bar"):
        model.assortment(objective="reach")
    assert model.score(silent=True)["stats"] == stats


def test_every_assortment_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("asrt_")]
    assert sorted(compiled) == sorted(NEW_KERNELS), compiled
    missing = [k for k in compiled if k not in names]
    assert not missing, missing
