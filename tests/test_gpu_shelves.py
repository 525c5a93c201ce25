"""Category-level recommendation on the device (shelves.hpp: mmsbm_hip_recommend_query_shelves, _query_theta_shelves;
MMSBM.recommend_shelves, recommend_categories, recommend_new_shelves) against the exact reference: models whose scores
carry no rounding (exact_models.py) and the numpy restatement of the definition (shelves_reference.py, pinned in
test_shelves_cpu.py).

Everything is compared by EQUALITY -- categories, counts, the padding, `available`, and the values and scores by their
bits -- with no tie band and no case left out: a category's value is its best scores added left to right and divided
once, whatever form the category's size selects, whatever column an item gets under a candidate list, whatever the split
of the selection across waves.
"""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import exact_models as xm
import quota_reference as qr
import shelves_reference as sr
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

SPLIT = (3, 5000, 4, 6, 5, 2)                                 # the selection of 5,000 singletons is split at column 1,000
assert SPLIT in xm.SPLIT
SHAPES = list(xm.MANY) + [SPLIT]
VARIANTS = [("mixed", "stars"), ("sorted", "indicator"), ("constant", "indicator")]
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]
DEPTHS = (1, 2, 10, 64, 65, 257)
WINDOW = {}


def asks_of(depth):
    """(depth, min_items, n_shelves, per_shelf): with every depth, min_items in {1, 3, depth}, n_shelves in {1, 5, 257}
    and per_shelf in {0, 1, 10, 257} (257 x 257 runs once per layout, on a few rows: test 1)."""
    return [(depth, 1, 5, 10), (depth, 3, 1, 0), (depth, depth, 257, 1), (depth, 3, 5, 257)]


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
    """The seven arrays equal in every entry, the padding included, values and scores by their bits."""
    assert len(got) == len(want) == 7
    for g, w, nm in zip(got, want, sr.NAMES):
        gb, wb = (xm.bits(g), xm.bits(w)) if nm in ("values", "scores") else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        assert gb.shape == wb.shape, (what, nm, gb.shape, wb.shape)
        if not np.array_equal(gb, wb):
            row = int(np.argwhere(gb != wb)[0][0])
            raise AssertionError(f"{what}: {nm} differ in {int((gb != wb).sum())} entries, first in row {row}: "
                                 f"device {np.asarray(g)[row]}, exact {np.asarray(w)[row]}")


def same_triple(got, want, what):
    for g, w, nm in zip(got, want, ("items", "scores", "counts")):
        gb, wb = (xm.bits(g), xm.bits(w)) if nm == "scores" else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        assert gb.shape == wb.shape and np.array_equal(gb, wb), (what, nm)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ---- 1. every layout, depth, min_items, n_shelves and per_shelf ----------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_layouts_and_parameters_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users, scores = case["users"], case["scores"]
    lay = qr.layouts(I, np.random.default_rng(xm.case_seed(*variant, shape)))
    assert ("straddle" in lay) == (shape == SPLIT)
    few = users[:24]
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            walk = qr.Walk(scores, users, None, case["seen"] if exclude else None)
            open_session(em, S, case["w"], exclude)
            for name, (category_of, G) in lay.items():
                fast = sr.Shelves(scores, users, category_of, G, walk=walk)
                csr = qr.categories_csr(category_of, G)
                for depth in DEPTHS:
                    for ask in asks_of(depth):
                        same_answer(em.recommend_query_shelves(users, *csr, *ask), fast.answer(*ask), f"{name} {ask} exclude={exclude}")
                got = em.recommend_query_shelves(few, *csr, 10, 1, 257, 257)
                same_answer(got, fast.answer(10, 1, 257, 257, first=len(few)), f"{name} 257 x 257 exclude={exclude}")
            em.recommend_end()
    finally:
        em.close()


# ---- 2. candidate subsets and the query's own exclusions ------------------------------------------------------------------------
def own_lists(rng, users, I, pool):
    """One list per request row, by the row's place: empty; one candidate; many items of the whole catalogue, shuffled,
    one repeated; all candidates but three."""
    out = []
    for b in range(len(users)):
        kind = b % 4
        if kind == 0:
            lst = []
        elif kind == 1:
            lst = [int(pool[b % len(pool)])]
        elif kind == 2:
            lst = rng.choice(I, min(I, 200), replace=False).tolist()
            lst = lst + lst[:1]
        else:
            lst = rng.permutation(pool)[3:].tolist()
        out.append(lst)
    return out


@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_candidates_and_own_exclusions_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    again = np.arange(min(U, 7))[::-1]                        # a user asked twice carries two different lists
    users = i32(np.concatenate([case["users"], again]))
    scores = case["scores"][users]
    lay = qr.layouts(I, rng)
    # every other item; a block across column 128 of the compact table; a set that leaves most of mod64's categories empty
    subsets = {"every_other": np.arange(0, I, 2), "block": np.arange(70, 70 + 300),
               "sparse": np.unique(np.concatenate([rng.choice(I, 40, replace=False), np.arange(5, I, 64)[:6], np.arange(9, I, 128)[:4]]))}
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            for sname, cand in subsets.items():
                lists = own_lists(rng, users, I, cand)
                walk = qr.Walk(scores, users, cand, case["seen"] if exclude else None, lists)
                for name in ("mod7", "mod64", "blocks", "random", "all_but_three", f"mod{I}"):
                    category_of, G = lay[name]
                    fast = sr.Shelves(scores, users, category_of, G, walk=walk)
                    csr = qr.categories_csr(category_of, G)
                    if (sname, name) == ("sparse", "mod64"):
                        m = np.array([np.isin(csr[1][csr[0][g]:csr[0][g + 1]], cand).sum() for g in range(G)])
                        assert (m == 0).any() and (m == 1).any() and (m > 2).any()
                    for ask in ((1, 1, 5, 10), (2, 2, 1, 0), (10, 1, 5, 10), (10, 3, 257, 1), (65, 1, 5, 257)):
                        got = em.recommend_query_shelves(users, *csr, *ask, i32(cand), cat.csr(lists))
                        same_answer(got, fast.answer(*ask), f"{sname} {name} {ask} exclude={exclude}")
            em.recommend_end()
    finally:
        em.close()


# ---- 3. identities against the queries that exist ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(VARIANTS[0], xm.MANY[0]), (VARIANTS[2], xm.MANY[1]), (VARIANTS[1], SPLIT)],
                         ids=["mixed-K7L9", "constant-K9L5", "sorted-split"])
def test_identities(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users = case["users"]
    rng = np.random.default_rng(3)
    lay = qr.layouts(I, rng)
    cand = i32(np.arange(1, I, 3))
    sample = i32([0, 1, 2, U - 1, 2][:max(3, min(U, 5))])
    thetas = np.stack([case["params"][s][0][sample] for s in range(S)])
    own = cat.csr([sorted(case["seen"][u]) for u in sample.tolist()])
    runs = np.arange(I) // 13                                 # a full categorisation whose index ascends with the item id
    G13 = int(runs.max()) + 1
    csr13 = qr.categories_csr(runs, G13)
    singles = (np.arange(I + 1, dtype=np.int64), i32(np.arange(I)))
    whole = (np.array([0, I], dtype=np.int64), i32(np.arange(I)))
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            what = f"exclude={exclude}"
            for n in (1, 5, 257):
                # depth 1 on a full categorisation: the categories and score bits of the quota query with cap 1
                sc, sv, sa, cnt, it, s, ic = em.recommend_query_shelves(users, *csr13, 1, 1, n, 1)
                qi, qs, qc = em.recommend_query_quota(users, n, *csr13, i32(np.ones(G13)))
                same_triple((np.where(sc >= 0, it[:, :, 0], -1), sv, cnt), (qi, qs, qc), f"quota cap 1 n={n} " + what)
                assert np.array_equal(sc, np.where(qi >= 0, runs[np.maximum(qi, 0)], -1))
                # singletons: the plain query with categories <-> items, at any depth
                plain = em.recommend_query(users, n)
                for depth in (1, 10):
                    got = em.recommend_query_shelves(users, *singles, depth, 1, n, 0)
                    same_triple((got[0], got[1], got[3]), plain, f"singletons n={n} depth={depth} " + what)
                    assert np.array_equal(got[2], (plain[0] >= 0).astype(np.int32))
            # one category of everything: the first per_shelf of the plain list, its value their running mean
            plain = em.recommend_query(users, 257)
            for depth, per in ((1, 10), (10, 10), (65, 257), (257, 1)):
                sc, sv, sa, cnt, it, s, ic = em.recommend_query_shelves(users, *whole, depth, 1, 3, per)
                same_triple((it[:, 0, :], s[:, 0, :], ic[:, 0]), (plain[0][:, :per], plain[1][:, :per], np.minimum(plain[2], per)),
                            f"everything per={per} " + what)
                for b in range(len(users)):
                    if plain[2][b]:
                        t = min(depth, int(plain[2][b])) if plain[2][b] < 257 else depth
                        assert xm.bits(sv[b, :1]) == xm.bits(np.array([sr.sequential_mean(plain[1][b, :t])])), (b, depth)
                    assert cnt[b] == (plain[2][b] > 0) and (sc[b, 1:] == -1).all()
            # per_shelf >= depth: a shelf's value is the sequential mean of its returned scores
            for name, depth, per in (("blocks", 10, 10), ("mod7", 64, 257), ("random", 2, 10)):
                csr = qr.categories_csr(*lay[name])
                sc, sv, sa, cnt, it, s, ic = em.recommend_query_shelves(users, *csr, depth, 1, 5, per)
                for b, k in zip(*np.nonzero(sc >= 0)):
                    t = min(depth, int(sa[b, k]))
                    assert ic[b, k] == min(per, sa[b, k])
                    assert xm.bits(sv[b, k:k + 1]) == xm.bits(np.array([sr.sequential_mean(s[b, k, :t])])), (name, b, k)
            # each shelf's items: recommend_query_within over the category alone
            for name in ("blocks", "mod7"):
                category_of, G = lay[name]
                csr = qr.categories_csr(category_of, G)
                sc, sv, sa, cnt, it, s, ic = em.recommend_query_shelves(users, *csr, 10, 1, G, 10)
                for g in range(G):
                    wi, ws, wc = em.recommend_query_within(users, 10, csr[1][csr[0][g]:csr[0][g + 1]])
                    b, k = np.nonzero(sc == g)
                    assert set(b.tolist()) == set(np.flatnonzero(wc > 0).tolist()), (name, g)
                    same_triple((it[b, k], s[b, k], ic[b, k]), (wi[b], ws[b], wc[b]), f"within {name} {g} " + what)
            # a user alone: the same user inside the full request
            csr, ask = qr.categories_csr(*lay["random"]), (10, 3, 5, 10)
            full = em.recommend_query_shelves(users, *csr, *ask, cand)
            for b in sorted({0, 1, U // 2, U - 1}):
                same_answer(em.recommend_query_shelves(users[b:b + 1], *csr, *ask, cand), tuple(a[b:b + 1] for a in full), f"alone {b} " + what)
            # the theta entry with a slot's own theta: the user entry (the session's seen lists given as the rows' own)
            if exclude:
                for cd in (None, cand):
                    for ask in ((10, 3, 5, 10), (2, 1, 257, 0)):
                        same_answer(em.recommend_query_theta_shelves(thetas, *csr, *ask, own, cd),
                                    em.recommend_query_shelves(sample, *csr, *ask, cd), f"theta {cd is None} {ask} " + what)
            # no category, or none with a candidate: every row empty
            empty = sr.pack([[] for _ in users], 5, 10)
            same_answer(em.recommend_query_shelves(users, np.zeros(1, dtype=np.int64), i32([]), 10, 1, 5, 10), empty, "no categories")
            same_answer(em.recommend_query_shelves(users, np.array([0, 2, 2], dtype=np.int64), i32([0, 3]), 10, 1, 5, 10, cand), empty, "no column")
            em.recommend_end()
    finally:
        em.close()


def test_added_items_belong_to_the_catalogue(hip):
    """Categories may name the items of recommend_add_items; one category straddles the training and the added ids."""
    variant, shape = VARIANTS[0], xm.MANY[0]
    U, I, K, L, R, S = shape
    n_new = 70
    case = case_of(variant, shape)
    rng = np.random.default_rng(11)
    src = rng.integers(0, I, n_new)                          # added item j duplicates training item src[j]'s eta rows
    new_eta = np.stack([case["params"][s][1][src] for s in range(S)])
    ext = [(t, np.vstack([e, new_eta[s]]), p) for s, (t, e, p) in enumerate(case["params"])]
    NI = I + n_new
    scores = xm.exact_scores(ext, case["users"], NI, case["w"])
    category_of = np.full(NI, -1, dtype=np.int64)
    category_of[I - 30:I + 40] = 0                           # 70 columns: the long form
    category_of[I + 40:] = 1                                 # 30 columns: a short one
    category_of[np.arange(0, I - 30, 2)] = 2
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        em.recommend_add_items(new_eta)
        fast = sr.Shelves(scores, case["users"], category_of, 3, None, case["seen"])
        for ask in ((1, 1, 3, 10), (10, 1, 2, 10), (65, 3, 3, 257), (257, 1, 1, 0)):
            same_answer(em.recommend_query_shelves(case["users"], *qr.categories_csr(category_of, 3), *ask), fast.answer(*ask), f"added items {ask}")
        em.recommend_end()
    finally:
        em.close()


# ---- 4. swapped sides ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(("mixed", "stars"), xm.MANY[1]), (("sorted", "indicator"), SPLIT)],
                         ids=["mixed-K9L5", "sorted-split"])
def test_swapped_contexts_answer_bitwise_the_same(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(7)
    users = i32(np.arange(max(U, 9)) % U)
    cand = np.arange(0, I, 2)
    lists = [rng.choice(I, 40, replace=False) for _ in users]
    lay = qr.layouts(I, rng)
    thetas = np.stack([p[0][users] for p in case["params"]])
    ask = (10, 1, 5, 10)
    asked = {name: (lay[name], qr.categories_csr(*lay[name])) for name in ("mod7", "blocks", "random")}
    answers = []
    for swap in (0, 1):
        em = context(hip, case["data"], case["params"], U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            open_session(em, S, case["w"], True)
            got = {}
            for name, (_, csr) in asked.items():
                got[name] = em.recommend_query_shelves(users, *csr, *ask, i32(cand), cat.csr(lists))
                got["theta " + name] = em.recommend_query_theta_shelves(thetas, *csr, *ask, None, i32(cand))
            answers.append(got)
            em.recommend_end()
        finally:
            em.close()
    scores = case["scores"][users]
    for name, ((category_of, G), _) in asked.items():
        same_answer(answers[0][name], sr.shelves(scores, users, category_of, G, *ask, cand, case["seen"], lists), name)
        same_answer(answers[0]["theta " + name], sr.shelves(scores, users, category_of, G, *ask, cand), "theta " + name)
    for what in answers[0]:
        same_answer(answers[1][what], answers[0][what], f"swapped {what}")


# ---- 5. users beyond one batch of scores --------------------------------------------------------------------------------------------
def test_batches_of_users(hip):
    """300 users over 100,003 items: three batches (128 + 128 + 44 rows), so the value buffer, the selection and the
    shelves' items run at a row offset of the request; a layout of short categories and one of long ones."""
    U, I, K, L, R, S = xm.BATCHES
    case = xm.make_case("mixed", "stars", xm.BATCHES, n_random=3000)
    users = case["users"]
    assert xm.batch_users(I, U) == 128
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        for name, m, ask in (("short", 25, (10, 1, 5, 10)), ("long", 1000, (10, 3, 5, 10)), ("short", 25, (2, 1, 3, 0))):
            G = I // m                                        # (the last three items are on no shelf)
            csr = (np.arange(G + 1, dtype=np.int64) * m, i32(np.arange(G * m)))
            got = em.recommend_query_shelves(users, *csr, *ask)
            same_answer(got, sr.block_shelves(case["scores"], users, case["seen"], m, G, *ask), f"{name} {ask}")
            assert (got[3][:128] > 0).any() and (got[3][128:256] > 0).any() and (got[3][256:] > 0).any(), name
        em.recommend_end()
    finally:
        em.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_requests_are_refused_before_any_launch(hip):
    U, I, K, L, R, S = xm.MANY[0]
    case = case_of(("mixed", "stars"), xm.MANY[0])
    E = hip._lib.HipLibraryError
    users = i32([0, 1])
    off = np.array([0, 2, 3], dtype=np.int64)
    good = (off, i32([3, 5, 8]))
    ask = (10, 1, 5, 10)
    thetas = np.stack([p[0][users] for p in case["params"]])
    bad = {"unsorted": (off, i32([5, 3, 8])), "repeated": (off, i32([3, 3, 8])), "negative id": (off, i32([-1, 5, 8])),
           "beyond": (off, i32([3, I, 8])), "two categories": (off, i32([3, 5, 5])),
           "offsets from 1": (np.array([1, 2, 3], dtype=np.int64), i32([3, 5, 8])),
           "offsets decrease": (np.array([0, 3, 2], dtype=np.int64), i32([3, 5]))}
    bad_asks = [(0, 1, 5, 10), (10, 0, 5, 10), (10, 1, 0, 10), (10, 1, 5, -1), (-3, 1, 5, 10)]
    big_asks = [(1025, 1, 5, 10), (10, 1, 1025, 10), (10, 1, 5, 1025)]

    def refused(call, code=None):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == (hip._lib.E_INVALID if code is None else code), e.value

    def raw(symbol, head, nulls):
        """The C entry with given output pointers (None: null) for two rows."""
        import ctypes as C
        out, ptrs = em._shelves_out(2, 5, 10)
        for k in nulls:
            ptrs[k] = None
        coff, cit = good
        return hip._lib.call(symbol, em._h, 2, *head, 0, None, *([None, None] if symbol.endswith("query_shelves") else []),
                             2, coff.ctypes.data_as(C.POINTER(C.c_int64)), cit.ctypes.data_as(C.POINTER(C.c_int32)),
                             10, 1, 5, 10, *ptrs)

    with LaunchWindow() as lw:
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            refused(lambda: em.recommend_query_shelves(users, *good, *ask))                  # no session
            em.recommend_begin(case["w"], True)
            refused(lambda: em.recommend_query_shelves(users, *good, *ask))                  # a session without a slot
            refused(lambda: em.recommend_query_theta_shelves(thetas[:0], *good, *ask))
            for s in range(S):
                em.select(s).recommend_add()
            for name, cats in bad.items():
                refused(lambda: em.recommend_query_shelves(users, *cats, *ask))
                refused(lambda: em.recommend_query_theta_shelves(thetas, *cats, *ask))
            for call in (lambda a: em.recommend_query_shelves(users, *good, *a),
                         lambda a: em.recommend_query_theta_shelves(thetas, *good, *a)):
                for a in bad_asks:
                    refused(lambda: call(a))
                for a in big_asks:
                    refused(lambda: call(a), hip._lib.E_UNSUPPORTED)
            # a null output that is needed (with per_shelf > 0 the item arrays are)
            import ctypes as C
            up = users.ctypes.data_as(C.POINTER(C.c_int32))
            tp = thetas.ctypes.data_as(C.POINTER(C.c_double))
            for k in range(7):
                refused(lambda: raw("mmsbm_hip_recommend_query_shelves", (up,), [k]))
                refused(lambda: raw("mmsbm_hip_recommend_query_theta_shelves", (tp, None, None), [k]))
            # what recommend_query_within / _query_theta_within refuse
            refused(lambda: em.recommend_query_shelves(i32([0, U]), *good, *ask))
            refused(lambda: em.recommend_query_shelves(users, *good, *ask, i32([5, 3, 8])))
            refused(lambda: em.recommend_query_shelves(users, *good, *ask, i32([3, 5, I])))
            refused(lambda: em.recommend_query_shelves(users, *good, *ask, None, (np.array([0, 2, 1], dtype=np.int64), i32([1]))))
            refused(lambda: em.recommend_query_shelves(users, *good, *ask, None, (off, i32([1, 2, I]))))
            refused(lambda: em.recommend_query_theta_shelves(thetas, *good, *ask, None, i32([3, 3])))
            refused(lambda: em.recommend_query_theta_shelves(thetas, *good, *ask, (off, i32([1, 2, I]))))
            # nothing to show is no error, and launches nothing either
            none = em.recommend_query_shelves(users, np.zeros(1, dtype=np.int64), i32([]), *ask)
            same_answer(none, sr.pack([[], []], 5, 10), "no categories")
            same_answer(em.recommend_query_theta_shelves(thetas, *good, *ask, None, i32([0, 1])), sr.pack([[], []], 5, 10), "no column")
        finally:
            em.close()
        names = lw.names()
        assert not [k for k in names if k.startswith(("shelf_", "quota_", "cat_", "rec_score", "rec_select", "rec_exclude"))], names
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        before = em.recommend_query(case["users"], 10)
        for cats in bad.values():
            with pytest.raises(E):
                em.recommend_query_shelves(users, *cats, *ask)
        em.recommend_query_shelves(users, *good, *ask)
        same_triple(em.recommend_query(case["users"], 10), before, "the plain query afterwards")   # the session still answers
        em.recommend_end()
    finally:
        em.close()


# ---- 7. the host class ------------------------------------------------------------------------------------------------------------------
def test_the_host_class_with_string_ids(hip):
    rng = np.random.default_rng(12)
    n_u, n_i, n_obs = 60, 150, 1500
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 6, iterations=8, sampling=2, seed=5)
    model.fit(df, silent=True)
    items = list(model.data_handler.item_labels())
    code = {lab: j for j, lab in enumerate(items)}
    brands = {lab: f"brand-{int(lab.split('-')[1]) % 9}" for lab in items if int(lab.split("-")[1]) % 5}
    brands.update({"not-in-the-model": "brand-0", items[3]: None})
    first_seen = list(dict.fromkeys(b for lab, b in brands.items() if b is not None and lab in code))
    ask = ["u7", "u1", "u7", "u30"]
    pairs = [("u7", items[0]), ("u1", items[5]), ("u2", items[3]), ("nobody", items[0])]
    cand = [items[j] for j in rng.choice(len(items), 90, replace=False)]

    def emulated(call, who, shelves, per_shelf, depth, min_items, pool):
        """The composition of existing calls: call(users, candidates, n) per category, the mean and the sort here."""
        members, once = {}, list(dict.fromkeys(who))
        for lab in pool:
            if brands.get(lab) is not None:
                members.setdefault(brands[lab], []).append(lab)
        lists = {c: call(once, labs, max(depth, per_shelf, 1)) for c, labs in members.items()}
        avail = {c: call(once, labs, len(labs)).groupby("users").size() for c, labs in members.items()}
        rows = []
        for u in who:
            found = []
            for c in first_seen:
                if c not in lists:
                    continue
                mine = lists[c][lists[c]["users"] == u]
                a = int(avail[c].get(u, 0))
                if a >= min_items and a > 0:
                    found.append((c, sr.sequential_mean(mine["score"].to_numpy()[:min(depth, a)]), a, mine))
            found.sort(key=lambda x: -x[1])                                   # (stable: ties in order of first appearance)
            for k, (c, v, a, mine) in enumerate(found[:shelves]):
                if per_shelf == 0:
                    rows.append({"users": u, "category": c, "score": v, "available": a, "rank": k + 1})
                for j, (_, r) in enumerate(mine.head(per_shelf).iterrows()):
                    rows.append({"users": u, "category": c, "shelf": k + 1, "shelf_score": v, "available": a,
                                 "items": r["items"], "score": r["score"], "rank": j + 1})
        return pd.DataFrame(rows)

    def same(got, want, columns):
        assert list(got.columns) == columns and len(got) == len(want) > 0
        for col in columns:
            if col in ("score", "shelf_score"):
                assert np.array_equal(xm.bits(got[col].to_numpy()), xm.bits(want[col].to_numpy())), col
            else:
                assert got[col].tolist() == want[col].tolist(), col

    shelf_cols = ["users", "category", "shelf", "shelf_score", "available", "items", "score", "rank"]
    cat_cols = ["users", "category", "score", "available", "rank"]
    for kw, pool in (({}, items), ({"candidates": cand, "exclude": pairs}, cand)):
        call = lambda us, labs, n: model.recommend(users=us, n=n, candidates=labs, exclude=kw.get("exclude"))  # noqa: E731
        for shelves, per, depth, mn in ((3, 4, None, 1), (9, 2, 5, 3), (2, 12, 1, 1)):
            got = model.recommend_shelves(users=ask, shelves=shelves, per_shelf=per, categories=brands, depth=depth, min_items=mn, **kw)
            same(got, emulated(call, ask, shelves, per, per if depth is None else depth, mn, pool), shelf_cols)
        got = model.recommend_categories(users=ask, n=4, categories=brands, depth=3, **kw)
        same(got, emulated(call, ask, 4, 0, 3, 1, pool), cat_cols)
    shown = model.recommend_shelves(users=ask, shelves=3, per_shelf=4, categories=brands)
    assert shown.groupby(["users", "items"]).size().max() <= 2                # (u7 is asked twice; no item on two shelves)
    frame = pd.DataFrame({"sku": list(brands), "brand": list(brands.values())})
    for form in (pd.Series(brands), frame):
        assert model.recommend_shelves(users=ask, shelves=3, per_shelf=4, categories=form).equals(shown)
    empty = model.recommend_shelves(users=ask, categories=brands, candidates=[])
    assert len(empty) == 0 and list(empty.columns) == shelf_cols
    empty = model.recommend_categories(users=ask, categories={"nothing-known": "x"})
    assert len(empty) == 0 and list(empty.columns) == cat_cols

    new = pd.DataFrame({"users": [f"new{x}" for x in rng.integers(0, 5, 60)],
                        "items": [f"item-{x}" for x in rng.integers(0, n_i, 60)], "ratings": rng.integers(1, 6, 60)})
    new = new[new["items"].isin(items)]
    who = list(new["users"].drop_duplicates())
    for kw, pool in (({}, items), ({"candidates": cand}, cand)):
        got = model.recommend_new_shelves(new, shelves=3, per_shelf=4, categories=brands, depth=2, **kw)
        same(got, emulated(lambda us, labs, n: model.recommend_new(new, n=n, candidates=labs), who, 3, 4, 2, 1, pool), shelf_cols)


# ---- 8. the launch log: these cases reach every kernel of shelves.hpp -------------------------------------------------------------------
def test_every_shelf_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("shelf_")]
    for k in ("shelf_value_short_kernel", "shelf_value_long_kernel", "shelf_items_kernel", "shelf_avail_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
