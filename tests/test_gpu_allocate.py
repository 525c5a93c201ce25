"""Capacity-aware allocation on the device (allocate.hpp: mmsbm_hip_recommend_allocate, HipEM.recommend_allocate,
MMSBM.allocate) against the exact reference: models whose scores carry no rounding (exact_models.py) and the numpy walk
over all pairs (allocate_reference.greedy, pinned in test_allocate_cpu.py).

Everything is compared by EQUALITY -- items, counts, the padding, and the scores by their bits -- with no tie band and no
case left out: the answer is the one stable assignment, whatever the batches of either pass, the split of a selection
across waves or the order of the request.  The round count is the reference's (allocate_reference.threshold_rounds).
"""
import functools
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

import allocate_reference as ar
import exact_models as xm
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

WIDE = (2500, 40, 4, 6, 5, 2)      # 2,500 user columns under the item pass: its selection is split across waves and merged
SHAPES = list(xm.MANY) + [WIDE]    # 300 / 260 / 997 / 1,021: partial 128-tiles on both sides of both passes
VARIANTS = [("mixed", "stars"), ("sorted", "indicator"), ("constant", "indicator")]
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]
SETS = ("n1cap1", "n3cap2", "n10cap5", "n10drawn")
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


def demand_and_caps(name, variant, shape):
    """(n, caps) of the four sets: (1, 1), (3, 2), (10, 5) and 10 with caps drawn from {0, 1, 2, 5, unlimited}."""
    I = shape[1]
    if name == "n10drawn":
        rng = np.random.default_rng(xm.case_seed(*variant, shape))
        return 10, rng.choice(np.array([0, 1, 2, 5, -1]), I).astype(np.int32)
    n, q = {"n1cap1": (1, 1), "n3cap2": (3, 2), "n10cap5": (10, 5)}[name]
    return n, np.full(I, q, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def expected(variant, shape, exclude, name):
    """(the walk's answer, the rounds of the threshold algorithm), once per case."""
    case = case_of(variant, shape)
    n, caps = demand_and_caps(name, variant, shape)
    seen = case["seen"] if exclude else None
    want = ar.greedy(case["scores"], case["users"], n, caps, seen)
    _, rounds, converged, _ = ar.threshold_rounds(case["scores"], case["users"], n, caps, seen)
    assert converged
    return want, rounds


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


# ---- 1. every variant, shape and (n, cap) set, with and without the exclusions -----------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_the_walk_on_the_device(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            for name in SETS:
                n, caps = demand_and_caps(name, variant, shape)
                want, rounds = expected(variant, shape, exclude, name)
                *got, info = em.recommend_allocate(case["users"], n, caps)
                what = f"{name} exclude={exclude}"
                same_answer(got, want, what)
                assert info == {"rounds": rounds, "converged": True}, (what, info, rounds)
                assert em.get_option("allocate_rounds") == rounds and em.get_option("allocate_ms") > 0
                *again, _ = em.recommend_allocate(None, n, caps)               # NULL users: all of them
                same_answer(again, want, what + " users=None")
            em.recommend_end()
    finally:
        em.close()


def test_long_lists(hip):
    """n = 257 on (300, 997): caps 300 and 1,024 cannot bind for 300 users; cap 100 does (76,800 wanted, 99,700 there)."""
    variant, shape = VARIANTS[1], xm.MANY[0]
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)
            plain = em.recommend_query(case["users"], 257)
            for q in (300, 1024, 100):
                caps = np.full(I, q, dtype=np.int32)
                *got, info = em.recommend_allocate(case["users"], 257, caps)
                same_answer(got, ar.greedy(case["scores"], case["users"], 257, caps, seen), f"cap {q} exclude={exclude}")
                assert info["converged"]
                if q >= U:
                    same_answer(got, plain, f"cap {q}: the plain query")
                    assert info["rounds"] == 1
                else:
                    assert info["rounds"] == ar.threshold_rounds(case["scores"], case["users"], 257, caps, seen)[1]
                    assert not np.array_equal(got[0], plain[0])
            em.recommend_end()
    finally:
        em.close()


# ---- 2. nothing binds: recommend_query ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(VARIANTS[0], xm.MANY[0]), (VARIANTS[2], xm.MANY[1]), (VARIANTS[1], WIDE)],
                         ids=["mixed-K7L9", "constant-K9L5", "sorted-wide"])
def test_unlimited_caps_are_the_plain_query(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users = case["users"]
    rng = np.random.default_rng(2)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            for n in (1, 10, 257):
                plain = em.recommend_query(users, n)
                for cname, caps in (("negative", np.full(I, -1)), ("U", np.full(I, U)), ("beyond", np.full(I, 2 ** 31 - 1)),
                                    ("mixed", rng.choice(np.array([-1, -7, U, U + 1]), I))):
                    *got, info = em.recommend_allocate(users, n, i32(caps))
                    same_answer(got, plain, f"{cname} n={n} exclude={exclude}")
                    assert info == {"rounds": 1, "converged": True}
                # one user: no cap >= 1 can bind; its plain list without the items of cap 0
                caps = i32(rng.choice(np.array([0, 1, 2, -1]), I))
                left = i32(np.flatnonzero(caps != 0))
                for u in sorted({0, 1, 2, U // 2, U - 1}):
                    *got, info = em.recommend_allocate(i32([u]), n, caps)
                    same_answer(got, em.recommend_query_within(i32([u]), n, left), f"user {u} alone n={n} exclude={exclude}")
                    assert info == {"rounds": 1, "converged": True}
            em.recommend_end()
    finally:
        em.close()


# ---- 3. a round limit ----------------------------------------------------------------------------------------------------------------
def test_a_round_limit_leaves_a_feasible_answer(hip):
    variant, shape = VARIANTS[2], xm.MANY[0]                   # the constant family: hundreds of rounds at cap 1
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users, scores, seen = case["users"], case["scores"], case["seen"]
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        for name in ("n1cap1", "n10cap5", "n10drawn"):
            n, caps = demand_and_caps(name, variant, shape)
            full = expected(variant, shape, True, name)[1]
            for limit in (1, 3):
                assert limit < full
                want, rounds, converged, _ = ar.threshold_rounds(scores, users, n, caps, seen, max_rounds=limit)
                *got, info = em.recommend_allocate(users, n, caps, max_rounds=limit)
                what = f"{name} max_rounds={limit}"
                assert info == {"rounds": limit, "converged": False} and (rounds, converged) == (limit, False), (what, info)
                ar.check_feasible(got, scores, users, n, caps, seen)
                same_answer(got, want, what)
            *got, info = em.recommend_allocate(users, n, caps, max_rounds=full)     # exactly enough: converged
            same_answer(got, expected(variant, shape, True, name)[0], f"{name} max_rounds={full}")
            assert info == {"rounds": full, "converged": True}
        em.recommend_end()
    finally:
        em.close()


# ---- 4. a subset of the users, in any order ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(VARIANTS[0], xm.MANY[1]), (VARIANTS[1], xm.MANY[0]), (VARIANTS[2], WIDE)],
                         ids=["mixed-K9L5", "sorted-K7L9", "constant-wide"])
def test_a_user_subset_in_any_order(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(4)
    subset = rng.choice(U, min(U, 150), replace=False)         # 150 rows: a full and a partial tile, not the ids' order
    other = rng.permutation(subset)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        for name in SETS:
            n, caps = demand_and_caps(name, variant, shape)
            *got, info = em.recommend_allocate(i32(subset), n, caps)
            same_answer(got, ar.greedy(case["scores"][subset], subset, n, caps, case["seen"]), f"{name} subset")
            assert info["rounds"] == ar.threshold_rounds(case["scores"][subset], subset, n, caps, case["seen"])[1]
            *again, info2 = em.recommend_allocate(i32(other), n, caps)
            row_of = {u: b for b, u in enumerate(other.tolist())}
            back = np.array([row_of[u] for u in subset.tolist()])
            same_answer(tuple(a[back] for a in again), got, f"{name} the same users in another order")
            assert info2 == info
        em.recommend_end()
    finally:
        em.close()


# ---- 5. added items ------------------------------------------------------------------------------------------------------------------------
def test_added_items_carry_caps(hip):
    """Items of recommend_add_items take part, with their caps and their seen lists."""
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
    raters = [np.sort(rng.choice(U, (0, 3, 40)[j % 3], replace=False)) for j in range(n_new)]
    seen = [set(s) for s in case["seen"]]
    for j, us in enumerate(raters):
        for u in us.tolist():
            seen[u].add(I + j)
    lists = (np.concatenate([[0], np.cumsum([len(r) for r in raters])]).astype(np.int64), i32(np.concatenate(raters)))
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        em.recommend_add_items(new_eta, lists)
        for n, caps in ((1, np.full(NI, 1)), (10, np.full(NI, 5)), (10, rng.choice(np.array([0, 1, 2, 5, -1]), NI)),
                        (3, np.concatenate([np.full(I, -1), np.full(n_new, 2)]))):
            *got, info = em.recommend_allocate(case["users"], n, i32(caps))
            same_answer(got, ar.greedy(scores, case["users"], n, caps, seen), f"added items n={n}")
            assert info["converged"] and (got[0] >= I).any()
        em.recommend_end()
    finally:
        em.close()


# ---- 6. swapped sides ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(("mixed", "stars"), xm.MANY[1]), (("sorted", "indicator"), WIDE)],
                         ids=["mixed-K9L5", "sorted-wide"])
def test_swapped_contexts_answer_bitwise_the_same(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    answers = []
    for swap in (0, 1):
        em = context(hip, case["data"], case["params"], U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            open_session(em, S, case["w"], True)
            answers.append({name: em.recommend_allocate(case["users"], *demand_and_caps(name, variant, shape)) for name in SETS})
            em.recommend_end()
        finally:
            em.close()
    for name in SETS:
        same_answer(answers[0][name][:3], expected(variant, shape, True, name)[0], name)
        same_answer(answers[1][name][:3], answers[0][name][:3], f"swapped {name}")
        assert answers[1][name][3] == answers[0][name][3]


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_bad_requests_are_refused_before_any_launch(hip):
    import ctypes as C
    shape = (1100, 60, 4, 6, 5, 2)                           # more users than a list holds: a cap of 1,025 could bind
    U, I, K, L, R, S = shape
    case = case_of(("mixed", "stars"), shape)
    lib = hip._lib
    E = lib.HipLibraryError
    users = i32([4, 0, 9])
    caps = np.full(I, 2, dtype=np.int32)

    def refused(call, code=None):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == (lib.E_INVALID if code is None else code), e.value

    def raw(em, users, n, caps, max_rounds, n_users=None):
        """The C entry itself: null pointers and an n_users of its own."""
        m = len(users) if n_users is None else n_users
        items, scores, counts = em._query_out(max(m, 0), max(n, 1))
        rounds, conv = C.c_int32(0), C.c_int32(0)
        p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))                    # noqa: E731
        lib.call("mmsbm_hip_recommend_allocate", em._h, m, p(users, C.c_int32), n, p(caps, C.c_int32), max_rounds,
                 p(items, C.c_int32), p(scores, C.c_double), p(counts, C.c_int32), C.byref(rounds), C.byref(conv))

    with LaunchWindow() as lw:
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            refused(lambda: em.recommend_allocate(users, 3, caps))                           # no session
            em.recommend_begin(case["w"], True)
            refused(lambda: em.recommend_allocate(users, 3, caps))                           # a session without a slot
            for s in range(S):
                em.select(s).recommend_add()
            for bad in (i32([4, U, 9]), i32([-1, 0, 9])):                                    # an id out of range
                refused(lambda: em.recommend_allocate(bad, 3, caps))
            refused(lambda: em.recommend_allocate(i32([4, 0, 4]), 3, caps))                  # a repeated user id
            for n in (0, -1):
                refused(lambda: em.recommend_allocate(users, n, caps))
            for limit in (0, -5):
                refused(lambda: em.recommend_allocate(users, 3, caps, max_rounds=limit))
            refused(lambda: raw(em, users, 3, None, 10))                                     # null caps
            refused(lambda: raw(em, None, 3, caps, 10, n_users=U - 1))                       # all users are U rows
            refused(lambda: raw(em, users, 3, caps, 10, n_users=-1))
            refused(lambda: em.recommend_allocate(users, hip.HipEM.MAX_RECOMMEND + 1, caps), lib.E_UNSUPPORTED)
            binding = caps.copy()
            binding[7] = hip.HipEM.MAX_RECOMMEND + 1                                         # 1,025 < 1,100 users
            refused(lambda: em.recommend_allocate(None, 3, binding), lib.E_UNSUPPORTED)
            refused(lambda: em.recommend_allocate(np.arange(1027), 3, binding), lib.E_UNSUPPORTED)
        finally:
            em.close()
        names = lw.names()
        assert not [k for k in names if k.startswith(("alloc_", "rec_score", "rec_select", "rec_exclude"))], names
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        before = em.recommend_query(case["users"], 10)
        with pytest.raises(E):
            em.recommend_allocate(i32([4, 0, 4]), 3, caps)
        binding = caps.copy()
        binding[7] = hip.HipEM.MAX_RECOMMEND + 1
        *got, info = em.recommend_allocate(np.arange(1025), 3, binding)                      # 1,025 users: it cannot bind
        same_answer(got, ar.greedy(case["scores"][:1025], np.arange(1025), 3, binding, case["seen"]), "a cap of all users")
        same_answer(em.recommend_query(case["users"], 10), before, "the plain query afterwards")   # the session still answers
        em.recommend_end()
        # the longest list an item can hold: caps of 1,024 that bind (1,100 users want 58 of the 60 items each)
        open_session(em, S, case["w"], False)
        full = np.full(I, hip.HipEM.MAX_RECOMMEND, dtype=np.int32)
        *got, info = em.recommend_allocate(None, 58, full)
        same_answer(got, ar.greedy(case["scores"], case["users"], 58, full), "caps of 1,024")
        assert ar.loads(got, I).max() == 1024 and info["converged"]
        assert info["rounds"] == ar.threshold_rounds(case["scores"], case["users"], 58, full)[1] > 1
        em.recommend_end()
    finally:
        em.close()


# ---- 8. the host class ---------------------------------------------------------------------------------------------------------------------------
def test_the_host_class_with_string_ids(hip):
    rng = np.random.default_rng(12)
    n_u, n_i, n_obs = 60, 150, 1500
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 6, iterations=8, sampling=2, seed=5)
    model.fit(df, silent=True)
    items = list(model.data_handler.item_labels())
    users = list(model.data_handler.user_labels())
    code = {lab: j for j, lab in enumerate(items)}
    ucode = {lab: j for j, lab in enumerate(users)}

    def walk(who, n, cap_of, pool=None, exclude_seen=True):
        """The definition over recommend()'s own frame for n = all items: its scores, sorted as top_pairs sorts."""
        every = model.recommend(users=who, n=len(items), candidates=pool, exclude_seen=exclude_seen)
        every = every.assign(u=[ucode[u] for u in every["users"]], i=[code[i] for i in every["items"]])
        every = every.sort_values(["score", "u", "i"], ascending=[False, True, True], kind="stable")
        held, left, rows = dict.fromkeys(who, 0), {}, []
        for u, i, s in zip(every["users"], every["items"], every["score"]):
            q = left.setdefault(i, cap_of(i))
            if held[u] < n and q != 0:
                rows.append((u, i, s))
                held[u] += 1
                left[i] = q - 1
        out = pd.DataFrame(rows, columns=["users", "items", "score"])
        parts = []
        for u in who:
            block = out[out["users"] == u].copy()
            block["rank"] = np.arange(1, len(block) + 1)
            parts.append(block)
        return pd.concat(parts, ignore_index=True)

    def same(got, want):
        assert list(got.columns) == ["users", "items", "score", "rank"]
        for col in ("users", "items", "rank"):
            assert got[col].tolist() == want[col].tolist(), col
        assert np.array_equal(xm.bits(got["score"].to_numpy()), xm.bits(want["score"].to_numpy()))

    ask = ["u7", "u1", "u30", "u2", "u11"]
    everyone = list(users)
    per_item = {lab: int(q) for lab, q in zip(items, rng.choice([0, 1, 2, 3], len(items)))}
    per_item["not-in-the-model"] = 1
    named = {lab: per_item[lab] for lab in items[::2]}                        # the others: unlimited
    cand = [items[j] for j in rng.choice(len(items), 90, replace=False)]
    for who in (ask, everyone):
        for n in (1, 4):
            for capacity, cap_of in ((1, lambda i: 1), (per_item, per_item.get), (named, lambda i: named.get(i, -1)),
                                     (pd.Series(named), lambda i: named.get(i, -1))):
                got = model.allocate(n=n, capacity=capacity, users=who)
                same(got, walk(who, n, cap_of))
                a = model.allocation_
                assert a["converged"] and a["rounds"] >= 1 and a["filled"] == len(got) and a["requested"] == len(who) * n
                load = model.item_load(got)
                assert list(load.columns) == ["items", "count"] and load["count"].sum() == len(got)
                assert all(cap_of(i) < 0 or c <= cap_of(i) for i, c in zip(load["items"], load["count"]))
                assert load["count"].is_monotonic_decreasing
            got = model.allocate(n=n, capacity=2, users=who, candidates=cand)
            same(got, walk(who, n, lambda i: 2, cand))
            same(got, model.allocate(n=n, capacity={lab: (2 if lab in cand else 0) for lab in items}, users=who))
    # what it is for: recommend() sends everybody to the same few items, allocate() does not
    plain = model.recommend(n=3)
    assert model.item_load(plain)["count"].max() > 2
    spread = model.allocate(n=3, capacity=2)
    assert model.item_load(spread)["count"].max() <= 2 and len(spread) <= len(plain)
    assert model.allocate(n=3, capacity=len(users)).equals(plain)                 # nothing binds: recommend's frame
    same(model.allocate(n=3, capacity=2, exclude_seen=False), walk(everyone, 3, lambda i: 2, exclude_seen=False))
    empty = model.allocate(n=2, capacity=1, users=[])
    assert len(empty) == 0 and list(empty.columns) == list(plain.columns)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                           # converged: no warning
        model.allocate(n=3, capacity=2)
    with pytest.warns(RuntimeWarning, match="max_rounds"):
        cut = model.allocate(n=3, capacity=1, max_rounds=1)
    assert model.allocation_["converged"] is False and model.allocation_["rounds"] == 1
    assert model.item_load(cut)["count"].max() <= 1 and cut.groupby("users").size().max() <= 3
    with pytest.raises(ValueError, match="distinct"):
        model.allocate(n=1, capacity=1, users=["u7", "u1", "u7"])
    with pytest.raises(ValueError, match="capacity"):
        model.allocate(n=1, capacity=True)
    with pytest.raises(KeyError):
        model.allocate(n=1, capacity=1, users=["nobody"])


# ---- 9. the launch log: these cases reach every kernel of allocate.hpp ---------------------------------------------------------------------
def test_every_alloc_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("alloc_")]
    for k in ("alloc_score_kernel", "alloc_sigma_kernel", "alloc_tau_kernel", "alloc_changed_kernel", "alloc_cut_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
