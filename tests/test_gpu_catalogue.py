"""Recommendation within a part of the catalogue on the device (catalogue.hpp: mmsbm_hip_recommend_query_within,
_query_theta_within, _rank; MMSBM.recommend(candidates=, exclude=), recommend_new(candidates=), rerank) against the exact
reference: models whose scores carry no rounding (exact_models.py) and the numpy restatement of catalogue_reference.py.

Everything is compared by EQUALITY -- items, counts, the padding, and the scores by their bits -- with no tie band and
no case left out: the answer of a query within candidates is the row of recommend_query(n = all items) filtered to the
candidates and cut to n, whatever column a candidate gets in the compact table, whatever the split across waves.
"""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import exact_models as xm
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip, problem  # noqa: F401  (hip: the fixture)

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

SPLIT = (3, 5000, 4, 6, 5, 2)                                 # a subset of >= 2,048 columns is split across waves
assert SPLIT in xm.SPLIT
SHAPES = list(xm.MANY) + [SPLIT]
VARIANTS = [("mixed", "stars"), ("sorted", "indicator"), ("constant", "indicator")]
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]
NS = (1, 10, 257)
WINDOW = {}


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


def open_session(em, n_slots, w, exclude):
    em.recommend_begin(w, exclude)
    for s in range(n_slots):
        em.select(s).recommend_add()


def same_answer(got, want, what):
    """(items, scores, counts) equal in every entry, the padding included, scores by their bits."""
    for g, w, nm in zip(got, want, ("items", "scores", "counts")):
        gb, wb = (xm.bits(g), xm.bits(w)) if nm == "scores" else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        assert gb.shape == wb.shape, (what, nm, gb.shape, wb.shape)
        if not np.array_equal(gb, wb):
            row = int(np.argwhere(gb != wb)[0][0])
            raise AssertionError(f"{what}: {nm} differ in {int((gb != wb).sum())} entries, first in row {row}: "
                                 f"device {np.asarray(g)[row]}, exact {np.asarray(w)[row]}")


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def candidate_sets(I, n, rng):
    """name -> ascending distinct ids: the sets of the issue."""
    out = {"empty": [], "one": [I // 2], "first": [0], "last": [I - 1]}
    for k in (n - 1, n, n + 1):
        if 0 < k <= I:
            out[f"random{k}"] = np.sort(rng.choice(I, k, replace=False))
    out["every_other"] = np.arange(0, I, 2)
    for k in (127, 128, 129):                                 # consecutive ids across the tile border at id 128 (and,
        out[f"block{k}"] = np.arange(70, 70 + k)              # with 127 / 128 / 129 columns, around a full tile)
    out["all_but_one"] = np.delete(np.arange(I), I // 3)
    out["all"] = np.arange(I)
    return {k: i32(v) for k, v in out.items()}


# ---- 1. subsets, 2. the whole catalogue ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_subsets_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users, scores = case["users"], case["scores"]
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)
            for n in NS:
                for name, cand in candidate_sets(I, n, rng).items():
                    got = em.recommend_query_within(users, n, cand)
                    same_answer(got, cat.within_top_n(scores, users, n, cand, seen), f"{name} n={n} exclude={exclude}")
                    left = np.array([len(cand) - len(set(cand.tolist()) & seen[u]) if exclude else len(cand) for u in users.tolist()])
                    assert np.array_equal(got[2], np.minimum(left, n)), name
            em.recommend_end()
    finally:
        em.close()


@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_the_whole_catalogue_is_recommend_query(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users = case["users"]
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            for n in NS + (1024,):
                plain = em.recommend_query(users, n)
                same_answer(plain, xm.exact_top_n(case["scores"], users, n, case["seen"] if exclude else None), f"plain n={n}")
                same_answer(em.recommend_query_within(users, n), plain, f"null list n={n} exclude={exclude}")
                same_answer(em.recommend_query_within(users, n, i32(np.arange(I))), plain, f"named n={n} exclude={exclude}")
                same_answer(em.recommend_query_within(users, n, None, cat.csr([[]] * U)), plain, f"empty lists n={n}")
            em.recommend_end()
    finally:
        em.close()


# ---- 3. the query's own exclusions ------------------------------------------------------------------------------------------
def extra_lists(rng, users, scores, cand, seen, I):
    """One list per request row, by the row's place: empty; the row's best candidate; many items of the whole catalogue
    (outside the candidates and training items among them, shuffled, one repeated); all candidates but three; all."""
    pool = np.arange(I) if cand is None else np.asarray(cand)
    out = []
    for b, u in enumerate(users.tolist()):
        kind = b % 5
        if kind == 0:
            lst = []
        elif kind == 1:
            best = cat.within_top_n(scores[b:b + 1], [u], 1, cand, seen)[0][0, 0]
            lst = [int(best)] if best >= 0 else [int(pool[0])]
        elif kind == 2:
            lst = rng.choice(I, min(I, 200), replace=False).tolist() + sorted(seen[u])[:5]
            lst = lst + lst[:1]
            rng.shuffle(lst)
        elif kind == 3:
            lst = rng.permutation(pool)[3:].tolist()
        else:
            lst = pool.tolist()
        out.append(lst)
    return out


@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_extra_exclusions_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    # every user once, then some again: a user asked twice carries two different lists (they go by the row's place)
    again = np.arange(min(U, 7))[::-1]
    users = i32(np.concatenate([case["users"], again]))
    scores = case["scores"][users]
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)
            for cname, cand in (("null", None), ("every_other", i32(np.arange(0, I, 2))), ("block129", i32(np.arange(70, 199)))):
                lists = extra_lists(rng, users, scores, cand, case["seen"], I)
                assert lists[U] != lists[again[0]]
                for n in NS:
                    got = em.recommend_query_within(users, n, cand, cat.csr(lists))
                    want = cat.within_top_n(scores, users, n, cand, seen, lists)
                    same_answer(got, want, f"{cname} n={n} exclude={exclude}")
                    assert (got[2][np.arange(len(users)) % 5 == 4] == 0).all()            # a list that leaves none
                    if cand is not None and n >= 10 and not exclude:
                        assert (got[2][np.arange(len(users)) % 5 == 3] == 3).all()        # ... and fewer than n
            em.recommend_end()
    finally:
        em.close()


# ---- 4. caller theta rows, added items -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.MANY, ids=["K7L9", "K9L5"])
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_caller_theta_rows_and_added_items(hip, variant, shape):
    U, I, K, L, R, S = shape
    n_new = 40
    case = case_of(variant, shape)
    params, w = case["params"], case["w"]
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    sample = i32([0, 1, 2, 3, 5, 77, U - 1, 5])
    thetas = np.stack([params[s][0][sample] for s in range(S)])
    own = cat.csr([sorted(case["seen"][u]) for u in sample.tolist()])
    src = rng.integers(0, I, n_new)                          # added item j duplicates training item src[j]'s eta rows
    new_eta = np.stack([params[s][1][src] for s in range(S)])
    ext = [(t, np.vstack([e, new_eta[s]]), p) for s, (t, e, p) in enumerate(params)]
    NI = I + n_new
    ext_scores = xm.exact_scores(ext, case["users"], NI, w)
    subsets = {"every_third": i32(np.arange(1, I, 3)), "block128": i32(np.arange(70, 198))}
    ext_subsets = {"added_only": i32(np.arange(I, NI)), "mixed": i32(np.concatenate([np.arange(0, I, 5), np.arange(I, NI, 2)])),
                   "all": i32(np.arange(NI))}
    em = context(hip, case["data"], params, U, I, R)
    try:
        open_session(em, S, w, True)
        for n in NS:
            for name, cand in subsets.items():
                within = em.recommend_query_within(sample, n, cand)
                same_answer(within, cat.within_top_n(case["scores"][sample], sample, n, cand, case["seen"]), f"{name} n={n}")
                same_answer(em.recommend_query_theta(thetas, n, own, candidates=cand), within, f"theta {name} n={n}")
            same_answer(em.recommend_query_theta(thetas, n, own, candidates=None), em.recommend_query(sample, n), f"theta null n={n}")
        em.recommend_add_items(new_eta)
        for n in NS:
            for name, cand in ext_subsets.items():
                within = em.recommend_query_within(sample, n, cand)
                same_answer(within, cat.within_top_n(ext_scores[sample], sample, n, cand, case["seen"]), f"extended {name} n={n}")
                same_answer(em.recommend_query_theta(thetas, n, own, candidates=cand), within, f"theta extended {name} n={n}")
        lists = [np.sort(rng.choice(NI, k, replace=False)) for k in (0, 1, 33, 300, n_new, 257, 10, 11)]
        lists[4] = np.arange(I, NI)
        off, items = cat.csr(lists)
        same_answer(em.recommend_rank(sample, off, items, 300),
                    cat.rank_lists(ext_scores[sample], sample, off, items, 300, case["seen"]), "rank extended")
        em.recommend_end()
    finally:
        em.close()


# ---- 5. per-user lists ------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 9, 10, 11, 255, 256, 257, 300)


@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_per_user_lists_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    rows = max(U, 2 * len(LENGTHS))
    users = i32(np.arange(rows) % U)                          # (few users: each several times, with different lists)
    scores = case["scores"][users]
    lists = [np.sort(rng.choice(I, LENGTHS[b % len(LENGTHS)], replace=False)) for b in range(rows)]
    holder = min((u for u in range(U) if case["seen"][u]), key=lambda u: (len(case["seen"][u]), -u))
    own_row = int(np.flatnonzero(users == holder)[0])
    lists[own_row] = np.array(sorted(case["seen"][holder])[:300])   # a list made only of the user's training items
    off, items = cat.csr(lists)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)
            full = em.recommend_query(users, min(I, 1024)) if not exclude and I <= 1024 else None
            for n in (1, 10, 300):
                got = em.recommend_rank(users, off, items, n)
                same_answer(got, cat.rank_lists(scores, users, off, items, n, seen), f"n={n} exclude={exclude}")
                assert got[2][own_row] == (0 if exclude else min(n, len(lists[own_row])))
                if full is not None:                           # every returned score: recommend_query's bits for the pair
                    for b in range(rows):
                        at = {int(i): k for k, i in enumerate(full[0][b].tolist())}
                        mine = [at[int(i)] for i in got[0][b, :got[2][b]]]
                        assert np.array_equal(xm.bits(got[1][b, :got[2][b]]), xm.bits(full[1][b, mine])), (n, b)
            em.recommend_end()
    finally:
        em.close()


# ---- 6. random models: the filtered rows of recommend_query(n = I) -----------------------------------------------------------
RANDOM = [(200, 997, 5, 20, 20, 3), (130, 1021, 4, 33, 5, 2), (140, 300, 3, 5, 33, 1)]   # (U, I, R, K, L, S), I <= 1,024


def filter_rows(full, n, keep):
    """full = recommend_query(n = I); keep(b) -> the ids row b may return: the rows filtered and cut to n."""
    items, scores, counts = full
    rows = []
    for b in range(len(counts)):
        it, sc = items[b, :counts[b]], scores[b, :counts[b]]
        ok = np.isin(it, keep(b))
        rows.append((it[ok][:n], sc[ok][:n]))
    return cat.pack(rows, n)


@pytest.mark.parametrize("shape", RANDOM, ids=lambda s: "U{}I{}R{}K{}L{}S{}".format(*s))
def test_random_models_equal_the_filtered_rows_of_the_full_query(hip, shape):
    U, I, R, K, L, S = shape
    data, params = problem(U, I, R, K, L, S, 20 * U, seed=K + 3 * L + S)
    rng = np.random.default_rng(I)
    w = np.arange(1, R + 1, dtype=np.float64)
    users = i32(np.concatenate([np.arange(U), [3, 3, 0]]))
    cand = i32(np.sort(rng.choice(I, I // 3, replace=False)))
    extra = [rng.choice(I, (0, 1, 60)[b % 3], replace=False) for b in range(len(users))]
    lists = [np.sort(rng.choice(I, LENGTHS[b % len(LENGTHS)], replace=False)) for b in range(len(users))]
    off, items = cat.csr(lists)
    em = context(hip, data, params, U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, w, exclude)
            full = em.recommend_query(users, I)
            for n in (1, 10, 257):
                same_answer(em.recommend_query_within(users, n, cand), filter_rows(full, n, lambda b: cand), f"subset n={n}")
                same_answer(em.recommend_query_within(users, n, cand, cat.csr(extra)),
                            filter_rows(full, n, lambda b: np.setdiff1d(cand, extra[b])), f"subset + extra n={n}")
                same_answer(em.recommend_query_within(users, n, None, cat.csr(extra)),
                            filter_rows(full, n, lambda b: np.setdiff1d(np.arange(I), extra[b])), f"extra n={n}")
                same_answer(em.recommend_rank(users, off, items, n), filter_rows(full, n, lambda b: lists[b]), f"rank n={n}")
            em.recommend_end()
    finally:
        em.close()


# ---- 7. swapped sides ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(("mixed", "stars"), xm.MANY[1]), (("sorted", "indicator"), SPLIT)],
                         ids=["mixed-K9L5", "sorted-split"])
def test_swapped_contexts_answer_bitwise_the_same(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(7)
    users = i32(np.arange(max(U, 9)) % U)
    cand = i32(np.arange(0, I, 2))
    extra = cat.csr([rng.choice(I, 40, replace=False) for _ in users])
    lists = [np.sort(rng.choice(I, LENGTHS[b % len(LENGTHS)], replace=False)) for b in range(len(users))]
    off, items = cat.csr(lists)
    thetas = np.stack([p[0][users] for p in case["params"]])
    answers = []
    for swap in (0, 1):
        em = context(hip, case["data"], case["params"], U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            open_session(em, S, case["w"], True)
            answers.append({"within": em.recommend_query_within(users, 10, cand, extra),
                            "theta": em.recommend_query_theta(thetas, 10, None, candidates=cand),
                            "rank": em.recommend_rank(users, off, items, 300)})
            em.recommend_end()
        finally:
            em.close()
    scores = case["scores"][users]
    same_answer(answers[0]["within"], cat.within_top_n(scores, users, 10, cand, case["seen"],
                                                       [extra[1][extra[0][b]:extra[0][b + 1]] for b in range(len(users))]), "within")
    same_answer(answers[0]["theta"], cat.within_top_n(scores, users, 10, cand), "theta")
    same_answer(answers[0]["rank"], cat.rank_lists(scores, users, off, items, 300, case["seen"]), "rank")
    for what in answers[0]:
        same_answer(answers[1][what], answers[0][what], f"swapped {what}")


# ---- 8. refusals, 9. no side effects -----------------------------------------------------------------------------------------
def test_bad_requests_are_refused_before_any_launch(hip):
    U, I, K, L, R, S = xm.MANY[0]
    case = case_of(("mixed", "stars"), xm.MANY[0])
    E = hip._lib.HipLibraryError
    users = i32([0, 1])
    good = i32([3, 5, 8])
    off = np.array([0, 2, 3], dtype=np.int64)
    thetas = np.stack([p[0][users] for p in case["params"]])
    bad_lists = {"unsorted": i32([5, 3, 8]), "duplicate": i32([3, 5, 5]), "negative": i32([-1, 3, 5]), "beyond": i32([3, 5, I])}

    def refused(call, code=None):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == (hip._lib.E_INVALID if code is None else code), e.value

    with LaunchWindow() as lw:
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            refused(lambda: em.recommend_query_within(users, 3, good))            # no session
            refused(lambda: em.recommend_rank(users, off, good, 3))
            em.recommend_begin(case["w"], True)
            refused(lambda: em.recommend_query_within(users, 3, good))            # a session without a slot
            refused(lambda: em.recommend_query_theta(thetas[:0], 3, None, candidates=good))
            refused(lambda: em.recommend_rank(users, off, good, 3))
            for s in range(S):
                em.select(s).recommend_add()
            for name, lst in bad_lists.items():
                refused(lambda: em.recommend_query_within(users, 3, lst))
                refused(lambda: em.recommend_query_theta(thetas, 3, None, candidates=lst))
                refused(lambda: em.recommend_rank(users, np.array([0, 3, 3], dtype=np.int64), lst, 3))   # one row holds it all
                refused(lambda: em.recommend_rank(users, np.array([0, 0, 3], dtype=np.int64), lst, 3))
            refused(lambda: em.recommend_rank(users, np.array([0, 1, 3], dtype=np.int64), i32([5, 8, 3]), 3))   # row 1 unsorted
            refused(lambda: em.recommend_rank(users, np.array([1, 2, 3], dtype=np.int64), good, 3))             # a bad CSR
            refused(lambda: em.recommend_rank(users, np.array([0, 3, 2], dtype=np.int64), good[:2], 3))
            refused(lambda: em.recommend_query_within(users, 3, good, (np.array([0, 2, 1], dtype=np.int64), i32([1]))))
            refused(lambda: em.recommend_query_within(users, 3, good, (off, i32([1, 2, I]))))
            refused(lambda: em.recommend_query_within(i32([0, U]), 3, good))
            refused(lambda: em.recommend_rank(i32([0, -1]), off, good, 3))
            for call in (lambda n: em.recommend_query_within(users, n, good),
                         lambda n: em.recommend_query_theta(thetas, n, None, candidates=good),
                         lambda n: em.recommend_rank(users, off, good, n)):
                refused(lambda: call(0))
                refused(lambda: call(1025), hip._lib.E_UNSUPPORTED)
            em.recommend_end()
        finally:
            em.close()
        names = lw.names()
        assert not [k for k in names if k.startswith("cat_") or k.startswith(("rec_score", "rec_select", "rec_exclude"))], names


def test_queries_leave_the_context_as_it_was(hip):
    U, I, K, L, R, S = xm.MANY[1]
    case = case_of(("mixed", "stars"), xm.MANY[1])
    users = case["users"]
    rng = np.random.default_rng(9)
    cand = i32(np.arange(1, I, 3))
    extra = cat.csr([rng.choice(I, 30, replace=False) for _ in users])
    lists = cat.csr([np.sort(rng.choice(I, 50, replace=False)) for _ in users])
    test = np.stack([rng.integers(0, U, 500), rng.integers(0, I, 500), rng.integers(0, R, 500)], 1)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        em.predict_begin(test, case["w"])
        em.select(0).predict_add()
        open_session(em, S, case["w"], True)
        before = em.recommend_query(users, 257)
        params = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
        em.recommend_query_within(users, 10, cand, extra)
        em.recommend_query_within(users, 10, None, extra)
        em.recommend_query_theta(np.stack([p[0] for p in case["params"]]), 10, None, candidates=cand)
        em.recommend_rank(users, lists[0], lists[1], 10)
        same_answer(em.recommend_query(users, 257), before, "the plain query afterwards")
        for s in range(S):
            for a, b in zip(em.select(s).get_params(), params[s]):
                assert np.array_equal(xm.bits(a), xm.bits(b))
        em.recommend_end()
        for s in range(1, S):
            em.select(s).predict_add()
        got, _ = em.predict_finish()
    finally:
        em.close()
    ref = context(hip, case["data"], case["params"], U, I, R)
    try:
        ref.predict_begin(test, case["w"])
        for s in range(S):
            ref.select(s).predict_add()
        want, _ = ref.predict_finish()
    finally:
        ref.close()
    assert np.array_equal(xm.bits(got), xm.bits(want))


# ---- 10. end to end ------------------------------------------------------------------------------------------------------------
def test_the_host_class_with_string_ids(hip):
    rng = np.random.default_rng(12)
    n_u, n_i, n_obs = 60, 150, 1500
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 6, iterations=8, sampling=2, seed=5)
    model.fit(df, silent=True)
    items = model.data_handler.item_labels()
    full = model.recommend(n=len(items))
    model.predict(df.iloc[:100])
    stats = model.score(silent=True)["stats"]
    prediction = np.array(model.prediction_matrix, copy=True)

    def expect(users, keep, n):
        parts = []
        for b, u in enumerate(users):
            block = full[full["users"] == u]
            block = block[np.array([keep(b, u, i) for i in block["items"]], dtype=bool)].head(n).copy()
            block["rank"] = np.arange(1, len(block) + 1)
            parts.append(block)
        return pd.concat(parts, ignore_index=True)

    def same(got, want):
        assert list(got.columns) == ["users", "items", "score", "rank"]
        for col in ("users", "items", "rank"):
            assert got[col].tolist() == want[col].tolist(), col
        assert np.array_equal(xm.bits(got["score"].to_numpy()), xm.bits(want["score"].to_numpy()))

    cand = [items[j] for j in rng.choice(len(items), 40, replace=False)] + [items[0], items[0]]
    ask = ["u7", "u1", "u7", "u30"]
    plain = {u: full[full["users"] == u]["items"].tolist() for u in ask}
    in_cand = {u: [i for i in plain[u] if i in cand] for u in ask}
    gone = {("u7", in_cand["u7"][0]), ("u1", in_cand["u1"][1]), ("u30", in_cand["u30"][0]), ("u30", in_cand["u30"][2])}
    pairs = sorted(gone) + [("u2", items[3]), ("nobody", items[0]), ("u7", "no-such-item")]
    same(model.recommend(users=ask, n=5, candidates=cand), expect(ask, lambda b, u, i: i in cand, 5))
    same(model.recommend(users=ask, n=5, candidates=cand, exclude=pairs),
         expect(ask, lambda b, u, i: i in cand and (u, i) not in gone, 5))
    same(model.recommend(users=ask, n=5, exclude=pd.DataFrame(pairs, columns=["users", "items"])),
         expect(ask, lambda b, u, i: (u, i) not in gone, 5))
    assert len(model.recommend(users=ask, n=5, candidates=[])) == 0
    with pytest.raises(KeyError, match="no-such-item"):
        model.recommend(users=ask, candidates=["no-such-item"])

    re_pairs = [(u, i) for u in ("u9", "u3", "u12") for i in full[full["users"] == u]["items"].iloc[[0, 5, 2, 0, 9]]]
    re_pairs = [re_pairs[j] for j in rng.permutation(len(re_pairs))]
    order = list(dict.fromkeys(u for u, _ in re_pairs))
    named = {u: {i for v, i in re_pairs if v == u} for u in order}
    same(model.rerank(re_pairs), expect(order, lambda b, u, i: i in named[u], len(items)))
    same(model.rerank(pd.DataFrame(re_pairs), n=2), expect(order, lambda b, u, i: i in named[u], 2))
    with pytest.raises(KeyError):
        model.rerank([("u9", "no-such-item")])

    new = pd.DataFrame({"users": [f"new{x}" for x in rng.integers(0, 5, 60)],
                        "items": [f"item-{x}" for x in rng.integers(0, n_i, 60)], "ratings": rng.integers(1, 6, 60)})
    new = new[new["items"].isin(items)]
    everything = model.recommend_new(new, n=len(items))
    got = model.recommend_new(new, n=4, candidates=cand)
    parts = []
    for u in everything["users"].drop_duplicates():
        block = everything[(everything["users"] == u) & everything["items"].isin(cand)].head(4).copy()
        block["rank"] = np.arange(1, len(block) + 1)
        parts.append(block)
    same(got, pd.concat(parts, ignore_index=True))

    assert model.score(silent=True)["stats"] == stats
    assert np.array_equal(np.asarray(model.prediction_matrix), prediction)


# ---- 11. the launch log: these cases reach every kernel of catalogue.hpp ---------------------------------------------------------
def test_every_catalogue_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("cat_")]
    for k in ("cat_gather_kernel", "cat_cols_kernel", "cat_exclude_kernel", "cat_rank_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
    assert not [k for k in names if k.startswith("rec_position")], sorted(names)
