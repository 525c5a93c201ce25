"""Welfare-maximising assignment on the device (assign.hpp: mmsbm_hip_recommend_assign, HipEM.recommend_assign,
MMSBM.assign) against the numpy restatement of the auction (assign_reference.auction, pinned in test_assign_cpu.py) on
models whose scores carry no rounding (exact_models.py).

Everything is compared by EQUALITY, with no tolerance and no case left out: items, loads, rounds, bids and the flag as
integers; scores, what was paid, the items' prices and price sums and every user's pi by their bits.  The auction only
adds, subtracts and compares doubles in a fixed order, so fed the same score bits the device must give the same bits.

The session offers no option for the size of a score batch, so the "batch forced small" form of a request is not among
the forms of test 2; the batch loop is the one recommend_query's tests cover.
"""
import ctypes as C
import functools
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

import assign_cases as ac
import assign_reference as ar
import exact_models as xm
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW = {}
INT_KEYS = ("items", "load")
BIT_KEYS = ("scores", "paid", "pi", "price", "price_sum")


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


def open_session(em, n_slots, w, exclude):
    em.recommend_begin(w, exclude)
    for s in range(n_slots):
        em.select(s).recommend_add()


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def as_device(res):
    """The reference's answer under the names HipEM.recommend_assign returns."""
    return {"items": res["items"], "scores": res["score"], "paid": res["paid"], "pi": res["pi"], "price": res["p1"],
            "price_sum": res["price_sum"], "load": res["load"], "rounds": res["rounds"], "bids": res["bids"],
            "converged": res["converged"]}


def same_answer(got, want, what, rows=None):
    """Every array equal in every entry (doubles by their bits), and the three numbers; rows: the request rows of `want`
    that `got` holds, in got's order."""
    for k in INT_KEYS + BIT_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if rows is not None and k in ("items", "scores", "paid", "pi"):
            w = w[rows]
        gb, wb = (xm.bits(g), xm.bits(w)) if k in BIT_KEYS else (g.astype(np.int64), w.astype(np.int64))
        assert gb.shape == wb.shape, (what, k, gb.shape, wb.shape)
        if not np.array_equal(gb, wb):
            at = int(np.flatnonzero(gb != wb)[0])
            raise AssertionError(f"{what}: {k} differ in {int((gb != wb).sum())} entries, first at {at}: device {g[at]!r}, "
                                 f"reference {w[at]!r}")
    for k in ("rounds", "bids", "converged"):
        assert got[k] == want[k], (what, k, got[k], want[k])


# ---- 1. every variant, shape, capacity set, reserve, with and without the exclusions ----------------------------------------
@pytest.mark.parametrize("variant,shape", ac.CASES, ids=ac.CASE_IDS)
def test_the_auction_on_the_device(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = ac.case_of(variant, shape)
    eps = ac.epsilon_of(variant)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            for name in ac.SETS:
                caps = ac.caps_of(name, variant, shape)
                for kind in ac.RESERVES:
                    reserve = ac.reserve_of(kind, variant, shape)
                    want = as_device(ac.expected(variant, shape, name, exclude, kind))
                    got = em.recommend_assign(case["users"], caps, reserve, eps, ac.MAX_ROUNDS)
                    what = f"{name} exclude={exclude} reserve={kind}"
                    same_answer(got, want, what)
                    assert em.get_option("assign_rounds") == want["rounds"] and em.get_option("assign_bids") == want["bids"]
                    assert em.get_option("assign_ms") > 0
                again = em.recommend_assign(None, caps, reserve, eps, ac.MAX_ROUNDS)      # NULL users: all of them
                same_answer(again, want, what + " users=None")
            em.recommend_end()
    finally:
        em.close()


# ---- 2. the same request in other forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(ac.VARIANTS[0], xm.MANY[1]), (ac.VARIANTS[1], xm.MANY[0]), (ac.VARIANTS[2], xm.MANY[0])],
                         ids=["mixed-K9L5", "sorted-K7L9", "constant-K7L9"])
def test_the_form_of_the_request_does_not_matter(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = ac.case_of(variant, shape)
    eps, reserve = ac.epsilon_of(variant), ac.reserve_of("default", variant, shape)
    rng = np.random.default_rng(4)
    order = rng.permutation(U)
    subset = rng.choice(U, 150, replace=False)               # a full and a partial tile, not in id order
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        for name in ac.SETS:
            caps = ac.caps_of(name, variant, shape)
            want = as_device(ac.expected(variant, shape, name, True, "default"))
            got = em.recommend_assign(i32(case["users"][order]), caps, reserve, eps, ac.MAX_ROUNDS)
            same_answer(got, want, f"{name} permuted", rows=order)
            part = as_device(ar.auction(case["scores"][subset], subset, caps, reserve, eps, case["seen"], ac.MAX_ROUNDS))
            got = em.recommend_assign(i32(subset), caps, reserve, eps, ac.MAX_ROUNDS)
            same_answer(got, part, f"{name} subset")
            again = em.recommend_assign(i32(subset[::-1]), caps, reserve, eps, ac.MAX_ROUNDS)
            same_answer(again, part, f"{name} subset reversed", rows=np.arange(len(subset))[::-1])
        em.recommend_end()
        # one slot in the session instead of S: the reference over that slot's scores alone
        open_session(em, 1, case["w"], True)
        one = xm.exact_scores(case["params"][:1], case["users"], I, case["w"])
        for name in ac.SETS:
            caps = ac.caps_of(name, variant, shape)
            want = as_device(ar.auction(one, case["users"], caps, reserve, eps, case["seen"], ac.MAX_ROUNDS))
            assert want["converged"]
            same_answer(em.recommend_assign(case["users"], caps, reserve, eps, ac.MAX_ROUNDS), want, f"{name} one slot")
        em.recommend_end()
    finally:
        em.close()


# ---- 3. nothing binds: recommend_query(n = 1) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(ac.VARIANTS[0], xm.MANY[0]), (ac.VARIANTS[2], xm.MANY[1]), (ac.VARIANTS[1], ac.SMALL)],
                         ids=["mixed-K7L9", "constant-K9L5", "sorted-small"])
def test_unlimited_caps_are_the_plain_query(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = ac.case_of(variant, shape)
    users, eps = case["users"], ac.epsilon_of(variant)
    rng = np.random.default_rng(2)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            items, scores, counts = em.recommend_query(users, 1)
            for kind in ac.RESERVES:
                reserve = ac.reserve_of(kind, variant, shape)
                stays = (counts > 0) & (scores[:, 0] > reserve)
                for cname, caps in (("negative", np.full(I, -1)), ("U", np.full(I, U)), ("beyond", np.full(I, 2 ** 31 - 1)),
                                    ("mixed", rng.choice(np.array([-1, -7, U, U + 1]), I))):
                    got = em.recommend_assign(users, i32(caps), reserve, eps)
                    what = f"{cname} exclude={exclude} reserve={kind}"
                    assert np.array_equal(got["items"], np.where(stays, items[:, 0], -1)), what
                    assert np.array_equal(xm.bits(got["scores"]), xm.bits(np.where(stays, scores[:, 0], -np.inf))), what
                    best = np.where(counts > 0, scores[:, 0], -np.inf)
                    assert np.array_equal(xm.bits(got["pi"]), xm.bits(np.maximum(best, reserve))), what
                    assert not got["paid"].any() and not got["price"].any() and not got["price_sum"].any(), what
                    assert (got["rounds"], got["converged"], got["bids"]) == (1, True, int(stays.sum())), what
                    assert np.array_equal(got["load"], np.bincount(items[stays, 0], minlength=I)), what
            em.recommend_end()
    finally:
        em.close()


# ---- 4. a round limit -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def optimum_of(variant, shape, name):
    case = ac.case_of(variant, shape)
    return ar.optimum(case["scores"], case["users"], ac.caps_of(name, variant, shape),
                      ac.reserve_of("default", variant, shape), case["seen"])[0]


def test_a_round_limit_leaves_a_feasible_answer_and_a_bound(hip):
    variant, shape = ac.VARIANTS[1], xm.MANY[0]
    U, I, K, L, R, S = shape
    case = ac.case_of(variant, shape)
    eps, reserve = ac.epsilon_of(variant), ac.reserve_of("default", variant, shape)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        for name in ("cap1", "cap2of40"):
            caps = ac.caps_of(name, variant, shape)
            full = ac.expected(variant, shape, name, True, "default")
            assert full["rounds"] > 3
            want = ar.auction(case["scores"], case["users"], caps, reserve, eps, case["seen"], max_rounds=3)
            got = em.recommend_assign(case["users"], caps, reserve, eps, max_rounds=3)
            assert (got["rounds"], got["converged"]) == (3, False) and not want["converged"]
            same_answer(got, as_device(want), f"{name} max_rounds=3")
            ar.check_feasible({"items": got["items"], "score": got["scores"], "paid": got["paid"], "load": got["load"]},
                              case["scores"], case["users"], caps, case["seen"])
            bound = ar.summary({"items": got["items"], "score": got["scores"], "pi": got["pi"],
                                "price_sum": got["price_sum"]}, reserve, eps)["bound"]
            best = optimum_of(variant, shape, name)
            print(f"{name}: bound after 3 rounds {bound!r}, optimum {best!r}")
            assert bound >= best
            # exactly enough rounds: converged, and within the guarantee of the optimum
            got = em.recommend_assign(case["users"], caps, reserve, eps, max_rounds=full["rounds"])
            same_answer(got, as_device(full), f"{name} max_rounds={full['rounds']}")
            sm = ar.summary({"items": got["items"], "score": got["scores"], "pi": got["pi"],
                             "price_sum": got["price_sum"]}, reserve, eps)
            print(f"{name}: value {sm['value']!r}, optimum {best!r}, bound {sm['bound']!r}, gap limit {sm['gap_limit']!r}")
            slack = 2.0 ** -40 * U                      # (sums of U terms of size <= 8: their rounding)
            assert sm["value"] <= best + slack and best <= sm["bound"] + slack
            assert sm["bound"] - sm["value"] <= sm["gap_limit"] + slack
        em.recommend_end()
    finally:
        em.close()


# ---- 5. the session afterwards, and the refusals -----------------------------------------------------------------------------------------
def test_bad_requests_are_refused_and_the_session_answers_as_before(hip):
    shape = (1100, 60, 4, 6, 5, 2)                           # more users than a slot list holds: a cap of 1,025 could bind
    U, I, K, L, R, S = shape
    variant = ("mixed", "stars")
    case = ac.case_of(variant, shape)
    lib = hip._lib
    E = lib.HipLibraryError
    users = i32([4, 0, 9])
    caps = np.full(I, 2, dtype=np.int32)
    eps = 2.0 ** -4

    def refused(call, code=None):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == (lib.E_INVALID if code is None else code), e.value

    def raw(em, users, caps, n_users=None, null=None, reserve=-3.0, epsilon=eps, max_rounds=10):
        """The C entry itself: null pointers and an n_users of its own."""
        m = len(users) if n_users is None else n_users
        out = {"items": np.zeros(max(m, 1), dtype=np.int32), "load": np.zeros(I, dtype=np.int32)}
        out.update({k: np.zeros(max(m, 1)) for k in ("scores", "paid", "pi")})
        out.update({k: np.zeros(I) for k in ("price", "price_sum")})
        rounds, conv = C.c_int32(0), C.c_int32(0)
        p = lambda k, t: None if k == null else out[k].ctypes.data_as(C.POINTER(t))                     # noqa: E731
        q = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))                     # noqa: E731
        lib.call("mmsbm_hip_recommend_assign", em._h, m, q(users), q(caps), reserve, epsilon, max_rounds,
                 p("items", C.c_int32), p("scores", C.c_double), p("paid", C.c_double), p("pi", C.c_double),
                 p("price", C.c_double), p("price_sum", C.c_double), p("load", C.c_int32),
                 None if null == "rounds" else C.byref(rounds), None if null == "converged" else C.byref(conv))

    with LaunchWindow() as lw:
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            refused(lambda: em.recommend_assign(users, caps, -3.0, eps))                      # no session
            em.recommend_begin(case["w"], True)
            refused(lambda: em.recommend_assign(users, caps, -3.0, eps))                      # a session without a slot
            for s in range(S):
                em.select(s).recommend_add()
            for bad in (i32([4, U, 9]), i32([-1, 0, 9])):                                     # an id out of range
                refused(lambda: em.recommend_assign(bad, caps, -3.0, eps))
            refused(lambda: em.recommend_assign(i32([4, 0, 4]), caps, -3.0, eps))             # a repeated user id
            for e in (0.0, -1.0, np.inf, np.nan, 4.0 * 2.0 ** -41):                           # (stars: span 4)
                refused(lambda: em.recommend_assign(users, caps, -3.0, e))
            for r in (np.nan, np.inf):
                refused(lambda: em.recommend_assign(users, caps, r, eps))
            for limit in (0, -5):
                refused(lambda: em.recommend_assign(users, caps, -3.0, eps, max_rounds=limit))
            refused(lambda: raw(em, users, None))                                             # null caps
            for k in ("items", "scores", "paid", "pi", "price", "price_sum", "load", "rounds", "converged"):
                refused(lambda: raw(em, users, caps, null=k))
            refused(lambda: raw(em, None, caps, n_users=U - 1))                               # all users are U rows
            refused(lambda: raw(em, users, caps, n_users=-1))
            binding = caps.copy()
            binding[7] = hip.HipEM.MAX_RECOMMEND + 1                                          # 1,025 < 1,100 users
            refused(lambda: em.recommend_assign(None, binding, -3.0, eps), lib.E_UNSUPPORTED)
            refused(lambda: em.recommend_assign(np.arange(1027), binding, -3.0, eps), lib.E_UNSUPPORTED)
        finally:
            em.close()
        names = lw.names()
        assert not [k for k in names if k.startswith(("assign_", "rec_score", "rec_select", "rec_exclude"))], names
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        before = em.recommend_query(case["users"], 10)
        with pytest.raises(E):
            em.recommend_assign(i32([4, 0, 4]), caps, -3.0, eps)
        some = np.arange(1025)
        binding = caps.copy()
        binding[7] = hip.HipEM.MAX_RECOMMEND + 1
        got = em.recommend_assign(some, binding, -3.0, eps)                                   # 1,025 users: it cannot bind
        same_answer(got, as_device(ar.auction(case["scores"][:1025], some, binding, -3.0, eps, case["seen"])), "a cap of all users")
        after = em.recommend_query(case["users"], 10)                                         # the session still answers
        for a, b in zip(after, before):
            assert np.array_equal(xm.bits(a) if a.dtype == np.float64 else a, xm.bits(b) if b.dtype == np.float64 else b)
        em.recommend_end()
        # the longest slot list: a cap of 1,024 that binds (1,100 users want item 0 or 1, which hold 1,024 + 5)
        open_session(em, S, case["w"], False)
        full = np.zeros(I, dtype=np.int32)
        full[0], full[1] = hip.HipEM.MAX_RECOMMEND, 5
        got = em.recommend_assign(None, full, -3.0, 0.25, max_rounds=4000)
        want = ar.auction(case["scores"], case["users"], full, -3.0, 0.25, None, 4000)
        same_answer(got, as_device(want), "a cap of 1,024")
        assert want["converged"] and want["load"][0] == 1024 and (want["items"] < 0).sum() == U - 1029
        em.recommend_end()
    finally:
        em.close()


# ---- 6. the host class ---------------------------------------------------------------------------------------------------------------------
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
    eps = 2.0 ** -6
    w = np.asarray(model.ratings, dtype=np.float64)
    reserve = float(w.min() - (w.max() - w.min()))           # the default

    def problem(who, cap_of, pool=None, exclude_seen=True):
        """(scores by request row, caps) out of recommend()'s own frame for n = all items."""
        every = model.recommend(users=who, n=len(items), candidates=pool, exclude_seen=exclude_seen)
        S = np.full((len(who), len(items)), -np.inf)
        row = {u: b for b, u in enumerate(who)}
        S[[row[u] for u in every["users"]], [code[i] for i in every["items"]]] = every["score"].to_numpy()
        caps = np.array([cap_of(i) for i in items])
        if pool is not None:
            caps[~np.isin(np.arange(len(items)), [code[i] for i in pool])] = 0
        return S, caps

    ask = ["u7", "u1", "u30", "u2", "u11"]
    named = {lab: int(q) for lab, q in zip(items[::2], rng.choice([0, 1, 2], len(items[::2])))}
    cand = [items[j] for j in rng.choice(len(items), 30, replace=False)]
    for who in (ask, list(users)):
        ids = np.array([ucode[u] for u in who])
        for capacity, cap_of, pool in ((1, lambda i: 1, None), (named, lambda i: named.get(i, -1), None),
                                       (pd.Series(named), lambda i: named.get(i, -1), None), (1, lambda i: 1, cand)):
            got = model.assign(capacity=capacity, epsilon=eps, users=who, candidates=pool)
            S, caps = problem(who, cap_of, pool)
            want = ar.auction(S, ids, caps, reserve, eps)
            has = want["items"] >= 0
            assert list(got.columns) == ["users", "items", "score", "rank", "price"]
            assert got["users"].tolist() == [u for u, h in zip(who, has) if h] and (got["rank"] == 1).all()
            assert got["items"].tolist() == [items[j] for j in want["items"][has]]
            assert np.array_equal(xm.bits(got["score"].to_numpy()), xm.bits(want["score"][has]))
            assert np.array_equal(xm.bits(got["price"].to_numpy()), xm.bits(want["paid"][has]))
            a, sm = model.assignment_, ar.summary(want, reserve, eps)
            assert (a["rounds"], a["bids"], a["converged"]) == (want["rounds"], want["bids"], True)
            assert (a["assigned"], a["dropped"]) == (int(has.sum()), int((~has).sum()))
            assert (a["total"], a["value"], a["bound"], a["gap_limit"]) == (sm["total"], sm["value"], sm["bound"], sm["gap_limit"])
            best = ar.optimum(S, ids, caps, reserve)[0]
            assert a["value"] <= best + 1e-9 and best <= a["bound"] + 1e-9 and a["bound"] - a["value"] <= a["gap_limit"] + 1e-9
            prices = a["prices"]
            bind = np.flatnonzero((caps >= 0) & (caps < len(who)))
            assert prices["items"].tolist() == [items[j] for j in bind] and prices["capacity"].tolist() == caps[bind].tolist()
            assert prices["load"].tolist() == want["load"][bind].tolist() and (prices["load"] <= prices["capacity"]).all()
            assert np.array_equal(xm.bits(prices["price"].to_numpy()), xm.bits(want["p1"][bind]))
    # what it is for: the total beats the stable walk's under the same capacities
    walk = model.allocate(n=1, capacity=1)
    best = model.assign(capacity=1, epsilon=eps)
    assert len(walk) == len(best) == len(users) and best["score"].sum() >= walk["score"].sum() - len(users) * eps
    # nothing binds: recommend(n=1)'s frame, price 0; the exclusions switched off
    plain = model.recommend(n=1)
    free = model.assign(capacity=len(users), epsilon=eps)
    assert free.drop(columns="price").equals(plain) and (free["price"] == 0).all()
    got = model.assign(capacity=2, epsilon=eps, exclude_seen=False)
    S, caps = problem(list(users), lambda i: 2, exclude_seen=False)
    want = ar.auction(S, np.arange(len(users)), caps, reserve, eps)
    assert got["items"].tolist() == [items[j] for j in want["items"][want["items"] >= 0]]
    empty = model.assign(capacity=1, epsilon=eps, users=[])
    assert len(empty) == 0 and list(empty.columns) == list(got.columns)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                           # converged: no warning
        model.assign(capacity=2, epsilon=eps)
    with pytest.warns(RuntimeWarning, match="max_rounds"):
        cut = model.assign(capacity=1, epsilon=eps, max_rounds=1)
    assert model.assignment_["converged"] is False and model.assignment_["rounds"] == 1
    assert cut["items"].value_counts().max() <= 1 and model.assignment_["bound"] >= model.assignment_["value"]
    with pytest.raises(ValueError, match="distinct"):
        model.assign(capacity=1, epsilon=eps, users=["u7", "u1", "u7"])
    with pytest.raises(ValueError, match="epsilon"):
        model.assign(capacity=1, epsilon=0.0)
    with pytest.raises(KeyError):
        model.assign(capacity=1, epsilon=eps, users=["nobody"])


# ---- 7. the launch log: these cases reach every kernel of assign.hpp, on the compacted path too ---------------------------------------------
def test_every_assign_kernel_was_launched_by_this_file(hip):
    # the compacted path: a converged request of several rounds whose rounds held fewer active rows than the request
    variant, shape = ac.VARIANTS[0], xm.MANY[0]
    U, I, K, L, R, S = shape
    case = ac.case_of(variant, shape)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        got = em.recommend_assign(case["users"], ac.caps_of("cap1", variant, shape), ac.reserve_of("default", variant, shape),
                                  ac.epsilon_of(variant))
        em.recommend_end()
    finally:
        em.close()
    dropped = int((got["items"] < 0).sum())
    active_rows = got["bids"] + dropped                      # every active row of a round bids, or drops out once
    assert got["rounds"] > 2 and got["converged"] and U < active_rows < got["rounds"] * U / 2, (got["rounds"], active_rows)
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("assign_")]
    for k in ("assign_value_kernel", "assign_bid_kernel", "assign_accept_kernel", "assign_count_kernel",
              "assign_scan_kernel", "assign_list_kernel", "assign_price_sum_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
    for k in ("rec_select_kernel", "rec_exclude_kernel"):    # recommend's own exclusion and selection, unchanged
        assert any(n.startswith(k) for n in names), (k, sorted(names))
