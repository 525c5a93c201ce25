"""The most informative items on the device (mmsbm_hip_inform_*, HipEM.inform_*, inform.hpp) against
inform_reference.py: gains within the tolerance derived there and ITEMS by equality (test_inform_cpu.py asserts, on the
restatement alone, that no two gains of a user on these seeds lie within 4 tolerances), the zeros of the exactly
representable models, and what the kernels promise bit for bit: +0.0 for a one-hot theta, identical items tied and in id
order, the same bits whatever the side layout, the batch, the other users of the call and the slots held.

MMSBM_E_TOOLARGE is the one refusal not provoked here: it needs a device without free memory.
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

import exact_models as xm
import inform_reference as ir
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)
from test_gpu_serving_exact import same_answer
from test_inform_cpu import GENERAL, NS, SPLIT, general_case
from test_similar_cpu import random_params

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE_ID = lambda s: "U{}I{}K{}L{}R{}S{}".format(*s)  # noqa: E731
TINY = (6, 45, 2, 3, 2, 1)
WINDOW = {}


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


class Session:
    """An inform session over slots 0 .. n_slots-1 (or `slots`) of a context, ended however the block ends."""

    def __init__(self, em, n_slots, slots=None):
        self.em, self.slots = em, range(n_slots) if slots is None else slots

    def __enter__(self):
        self.em.inform_begin()
        for s in self.slots:
            self.em.select(s).inform_add()
        return self.em

    def __exit__(self, *exc):
        self.em.inform_end()
        return False


def dense(answer, I):
    """(M, I) gains of an answer that holds every item (n >= I, nothing left out), by item id."""
    items, vals, counts = answer
    assert (counts == I).all()
    out = np.empty((len(items), I))
    np.put_along_axis(out, items[:, :I].astype(np.int64), vals[:, :I], axis=1)
    return out


def check(got, g, n, mask, tol, what):
    """An answer against the restatement's gains g (M, I): items and counts EQUAL, gains within tol, padding."""
    want_items, want_vals, want_counts = ir.top_n(g, n, mask)
    items, vals, counts = got
    assert np.array_equal(counts, want_counts), what
    assert np.array_equal(items, want_items), (what, np.argwhere(items != want_items)[:3])
    held = np.arange(n)[None, :] < counts[:, None]
    err = np.abs(np.where(held, vals - np.where(held, want_vals, 0.0), 0.0))
    print(f"{what}: largest error / tolerance {err.max() / tol:.4f}")
    assert (err <= tol).all(), (what, err.max() / tol)
    assert np.isneginf(vals[~held]).all() and (vals[held] >= 0.0).all() and not np.signbit(vals[held]).any()


# ---- 1. general models against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", GENERAL + [SPLIT], ids=lambda v: SHAPE_ID(v) if isinstance(v, tuple) else f"seed{v}")
def test_general_models_agree_with_the_restatement(hip, shape, seed):
    U, I, K, L, R, S = shape
    data, params = general_case(shape, seed)
    tol = ir.tolerance(K, L, R, S)
    users = np.arange(U, dtype=np.int32)
    g = ir.gains_of_users(params, users)
    seen = ir.allowed_mask(U, I, lists=ir.train_lists(data, users))
    mean = ir.mean_theta(params)[:, None, :]
    gm = ir.gains(params, list(mean))
    if (shape, seed) == SPLIT:
        assert xm.select_split(I, U, hip._lib.device_identity(0)["compute_units"])[0] > 1, "split across waves and merged"
    em = context(hip, data, params, U, I, R)
    try:
        with Session(em, S):
            for n in NS:
                check(em.inform_query(users, n), g, n, seen, tol, f"{shape} n={n}")
                assert em.get_option("inform_ms") > 0
            check(em.inform_query(users, 10, exclude_seen=False), g, 10, None, tol, f"{shape} nothing left out")
            check(em.inform_query_theta(mean, 257), gm, 257, None, tol, f"{shape} the mean theta")
    finally:
        em.close()


# ---- 2. zeros: exactly representable models ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.MANY + [TINY], ids=SHAPE_ID)
@pytest.mark.parametrize("family", xm.FAMILIES)
def test_models_full_of_exact_zeros(hip, family, shape):
    U, I, K, L, R, S = shape
    rng = np.random.default_rng(xm.case_seed(family, "stars", shape))
    params, _ = xm.model(family, rng, U, I, K, L, R, S)
    data = np.stack([rng.integers(0, U, 3 * U), rng.integers(0, I, 3 * U), rng.integers(0, R, 3 * U)], 1)
    mixed = np.stack([xm.dyadic_simplex(rng, (67, K), 16) for _ in range(S)])   # rows with exact zeros, not one-hot
    tol = ir.tolerance(K, L, R, S)
    em = context(hip, data, params, U, I, R)
    try:
        with Session(em, S):
            own = dense(em.inform_query(np.arange(U), 1024, exclude_seen=False), I)
            given = dense(em.inform_query_theta(mixed, 1024), I)
    finally:
        em.close()
    for got, want, what in ((own, ir.gains_of_users(params, np.arange(U)), "own"), (given, ir.gains(params, list(mixed)), "given")):
        assert np.isfinite(got).all() and (got >= 0.0).all() and not np.signbit(got).any(), (family, what)
        assert np.abs(got - want).max() <= tol, (family, what, np.abs(got - want).max() / tol)
    if family in xm.BLOCK_FAMILIES:                          # one-hot theta: nothing to learn about the user's group
        assert (xm.bits(own) == 0).all()


# ---- 3. exact structure, by bits ----------------------------------------------------------------------------------------
def test_one_hot_theta_gains_exactly_zero_for_every_item(hip):
    shape, seed = GENERAL[0]
    U, I, K, L, R, S = shape
    data, params = general_case(shape, seed)
    rng = np.random.default_rng(7)
    M = 70                                                   # (two tiles of query rows)
    theta = np.stack([np.eye(K)[rng.integers(0, K, M)] for _ in range(S)])   # a group of its own in every slot
    lists = [np.sort(rng.choice(I, size, replace=False)) for size in rng.integers(0, 40, M)]
    lists[3] = np.arange(0, 300)                             # ... the first ids left out
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    seen = (off, np.concatenate(lists).astype(np.int32))
    em = context(hip, data, params, U, I, R)
    try:
        with Session(em, S):
            got = {n: em.inform_query_theta(theta, n, seen) for n in NS}
            everything = em.inform_query_theta(theta, 1024)
    finally:
        em.close()
    assert (xm.bits(dense(everything, I)) == 0).all()        # +0.0, every item
    for n in NS:
        items, vals, counts = got[n]
        assert (counts == n).all() and (xm.bits(vals) == 0).all()
        for b in range(M):
            assert items[b].tolist() == np.setdiff1d(np.arange(I), lists[b])[:n].tolist(), (n, b)


def test_identical_items_tie_exactly_and_come_in_id_order(hip):
    U, I, K, L, R, S = 40, 700, 6, 9, 4, 2
    rng = np.random.default_rng(5)
    params = random_params(rng, U, I, K, L, R, S)
    data = np.stack([rng.integers(0, U, 5 * U), rng.integers(0, I, 5 * U), rng.integers(0, R, 5 * U)], 1)
    twins = (5, 17, 300, 699)
    for _, e, _ in params:
        e[list(twins[1:])] = e[5]
    em = context(hip, data, params, U, I, R)
    try:
        with Session(em, S):
            items, vals, counts = em.inform_query(np.arange(U), I, exclude_seen=False)
    finally:
        em.close()
    assert (counts == I).all()
    for b in range(U):
        row = items[b].tolist()
        at = [row.index(i) for i in twins]
        assert at == list(range(at[0], at[0] + 4)), (b, at)
        assert len(set(xm.bits(vals[b, at]).tolist())) == 1


def test_one_rating_value_carries_no_information(hip):
    U, I, K, L, R, S = 70, 90, 5, 4, 1, 2
    data, params = general_case((U, I, K, L, R, S), 8)
    em = context(hip, data, params, U, I, R)
    try:
        with Session(em, S):
            got = dense(em.inform_query(np.arange(U), I, exclude_seen=False), I)
    finally:
        em.close()
    assert (got >= 0.0).all() and got.max() <= ir.tolerance(K, L, R, S)


# ---- 4. invariances, by bits ---------------------------------------------------------------------------------------------
def test_swapped_contexts_are_bitwise_equal(hip):
    U, I, K, L, R, S = 300, 800, 12, 7, 5, 2
    data, params = general_case((U, I, K, L, R, S), 11)
    theta = np.stack([p[0][::3] for p in params])
    answers = []
    for swap in (0, 1):
        em = context(hip, data, params, U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            with Session(em, S):
                answers.append((em.inform_query(np.arange(U), 10), em.inform_query(np.arange(U), 257, exclude_seen=False),
                                em.inform_query_theta(theta, 10), em.inform_mean_theta()))
        finally:
            em.close()
    for k, what in enumerate(("n=10", "n=257", "theta rows")):
        same_answer(answers[1][k], answers[0][k], f"swap {what}")
    assert np.array_equal(xm.bits(answers[1][3]), xm.bits(answers[0][3]))


def test_a_user_alone_in_a_crowd_and_across_a_batch_border(hip):
    """300 users over 100,003 items: batches of 128, 128 and 44 rows."""
    U, I, K, L, R, S = xm.BATCHES
    assert xm.batch_users(I, U) == 128
    data, params = general_case(xm.BATCHES, 12)
    em = context(hip, data, params, U, I, R)
    try:
        with Session(em, S):
            every = em.inform_query(np.arange(U), 10)
            alone = em.inform_query([130], 10)
            border = em.inform_query(np.arange(120, 140), 10)             # one batch here, two batches above
            back = em.inform_query(np.arange(U)[::-1], 10)
            own = em.inform_query_theta(params[0][0][None, 250:], 10, ir.train_lists(data, np.arange(250, U)))
    finally:
        em.close()
    same_answer(alone, tuple(a[130:131] for a in every), "alone")
    same_answer(border, tuple(a[120:140] for a in every), "across the border")
    same_answer(back, tuple(a[::-1] for a in every), "reversed")
    same_answer(own, tuple(a[250:] for a in every), "the slot's own theta rows")
    assert (every[2] == 10).all()


def test_query_theta_of_the_slots_own_rows_is_query(hip):
    shape, seed = GENERAL[1]
    U, I, K, L, R, S = shape
    data, params = general_case(shape, seed)
    users = np.random.default_rng(1).permutation(U)[:150]
    theta = np.stack([p[0][users] for p in params])
    cand = np.arange(3, I, 7, dtype=np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        with Session(em, S):
            for n in (10, 257):
                same_answer(em.inform_query_theta(theta, n, ir.train_lists(data, users)), em.inform_query(users, n), f"n={n}")
            same_answer(em.inform_query_theta(theta, 10, None, cand), em.inform_query(users, 10, cand, None, False), "within")
    finally:
        em.close()


def test_slots_beyond_those_added_do_not_matter(hip):
    U, I, K, L, R = 200, 300, 5, 6, 4
    data, params = general_case((U, I, K, L, R, 3), 4)
    ids = np.arange(U)
    one = context(hip, data, params[2:], U, I, R)
    try:
        with Session(one, 1):
            alone = one.inform_query(ids, 10), one.inform_mean_theta()
    finally:
        one.close()
    three = context(hip, data, params, U, I, R)
    try:
        with Session(three, 3, slots=[2]):
            among = three.inform_query(ids, 10), three.inform_mean_theta()
    finally:
        three.close()
    same_answer(among[0], alone[0], "slot 2 of 3")
    assert np.array_equal(xm.bits(among[1]), xm.bits(alone[1]))


# ---- 5. the mask and the exclusions -----------------------------------------------------------------------------------------
def test_candidates_and_exclusions_filter_the_full_list(hip):
    shape, seed = GENERAL[0]
    U, I, K, L, R, S = shape
    data, params = general_case(shape, seed)
    rng = np.random.default_rng(3)
    users = np.array([5, 0, 299, 5, 64, 63, 128], dtype=np.int32)         # (a user asked twice carries two lists)
    cand = np.sort(rng.choice(I, 400, replace=False)).astype(np.int32)
    own = [rng.choice(I, size, replace=True) for size in (0, 30, 5, 200, 1, 0, 60)]
    own[2] = cand.copy()                                                  # every candidate left out: no answer
    off = np.concatenate([[0], np.cumsum([len(x) for x in own])]).astype(np.int64)
    lists = (off, np.concatenate(own).astype(np.int32))
    em = context(hip, data, params, U, I, R)
    try:
        with Session(em, S):
            full = em.inform_query(users, 1024, exclude_seen=False)
            got = {(c, x, t): em.inform_query(users, 25, cand if c else None, lists if x else None, t)
                   for c in (0, 1) for x in (0, 1) for t in (False, True)}
            none = em.inform_query(users, 5, np.zeros(0, dtype=np.int32))
    finally:
        em.close()
    g = np.full((len(users), I), -np.inf)
    np.put_along_axis(g, full[0][:, :I].astype(np.int64), full[1][:, :I], axis=1)   # the device's own gains
    train = ir.allowed_mask(len(users), I, lists=ir.train_lists(data, users))
    for (c, x, t), answer in got.items():
        mask = ir.allowed_mask(len(users), I, cand if c else None, lists if x else None) & (train if t else True)
        same_answer(answer, ir.top_n(g, 25, mask), f"candidates={c} lists={x} train={t}")
    assert got[(1, 1, False)][2][2] == 0 and (got[(1, 1, False)][0][2] == -1).all()
    assert np.isneginf(got[(1, 1, True)][1][2]).all()
    assert (none[2] == 0).all() and (none[0] == -1).all() and np.isneginf(none[1]).all()


# ---- 6. the population's mean membership -----------------------------------------------------------------------------------
@pytest.mark.parametrize("U", [1, 255, 700])
def test_mean_theta_in_the_fixed_order(hip, U):
    I, K, L, R, S = 50, 5, 4, 3, 2
    rng = np.random.default_rng(U)
    data, params = general_case((U, I, K, L, R, S), 6)
    exact, _ = xm.model("mixed", rng, U, I, K, L, R, S)
    answers = []
    for p in (exact, params):
        em = context(hip, data, p, U, I, R)
        try:
            with Session(em, S):
                answers.append(em.inform_mean_theta())
        finally:
            em.close()
    assert np.array_equal(xm.bits(answers[0]), xm.bits(ir.mean_theta(exact)))          # dyadic: by bits
    bound = (-(-U // ir.MASS_BLOCK) + 9) * 2.0 ** -52
    assert np.abs(answers[1] - ir.mean_theta(params)).max() <= bound
    assert np.abs(answers[1] - np.stack([t.mean(axis=0) for t, _, _ in params])).max() <= bound


# ---- 7. the ABI's refusals ----------------------------------------------------------------------------------------------
def refused(hip, code, fn, *args, **kw):
    with pytest.raises(hip._lib.HipLibraryError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.message)


def test_refusals_by_status_code_and_the_other_sessions_are_left_alone(hip):
    U, I, K, L, R = 50, 60, 4, 3, 3
    data, params = general_case((U, I, K, L, R, 1), 2)
    lib = hip._lib
    w = np.arange(1.0, R + 1)
    ok_theta = params[0][0][None, :2]
    em = context(hip, data, params, U, I, R)
    try:
        em.recommend_begin(w, True)
        em.recommend_add()
        em.similar_begin(0)
        em.similar_add()
        before = em.recommend_query(np.arange(U), 10), em.similar_query(np.arange(I), 10)
        refused(hip, lib.E_INVALID, em.inform_add)                       # without begin
        refused(hip, lib.E_INVALID, em.inform_query, [0], 3)
        refused(hip, lib.E_INVALID, em.inform_mean_theta)
        em.inform_begin()
        refused(hip, lib.E_INVALID, em.inform_query, [0], 3)             # before the first add
        refused(hip, lib.E_INVALID, em.inform_mean_theta)
        em.inform_add()
        for bad in (-1, U):
            refused(hip, lib.E_INVALID, em.inform_query, [0, bad], 3)
        for bad in (0, -2):
            refused(hip, lib.E_INVALID, em.inform_query, [0], bad)
            refused(hip, lib.E_INVALID, em.inform_query_theta, ok_theta, bad)
        refused(hip, lib.E_UNSUPPORTED, em.inform_query, [0], 1025)
        refused(hip, lib.E_UNSUPPORTED, em.inform_query_theta, ok_theta, 1025)
        for bad in ([3, 3], [4, 2], [0, I], [-1, 2]):                    # not strictly ascending, out of range
            refused(hip, lib.E_INVALID, em.inform_query, [0], 3, np.array(bad, dtype=np.int32))
            refused(hip, lib.E_INVALID, em.inform_query_theta, ok_theta, 3, None, np.array(bad, dtype=np.int32))
        bad_csr = [(np.array([1, 2, 2]), np.array([0, 1])), (np.array([0, 2, 1]), np.array([0])),
                   (np.array([0, 1, 2]), np.array([0, I])), (np.array([0, 1, 2]), np.array([-1, 0]))]
        for off, it in bad_csr:
            lists = (off.astype(np.int64), it.astype(np.int32))
            refused(hip, lib.E_INVALID, em.inform_query, [0, 1], 3, None, lists)
            refused(hip, lib.E_INVALID, em.inform_query_theta, ok_theta, 3, lists)
        for bad in (np.nan, np.inf, -np.inf, -0.25):
            theta = ok_theta.copy()
            theta[0, 1, 2] = bad
            refused(hip, lib.E_INVALID, em.inform_query_theta, theta, 3)
        assert em.inform_query([U - 1], 1024, exclude_seen=False)[2].tolist() == [I]
        assert em.inform_query([], 5)[0].shape == (0, 5)
        assert em.inform_query_theta(ok_theta[:, :0], 5)[0].shape == (0, 5)
        em.inform_begin()                                                # the next begin ends the session
        refused(hip, lib.E_INVALID, em.inform_query, [0], 3)
        em.inform_end()
        refused(hip, lib.E_INVALID, em.inform_add)
        em.inform_end()                                                  # ending twice is no error
        same_answer(em.recommend_query(np.arange(U), 10), before[0], "the open recommend session")
        same_answer(em.similar_query(np.arange(I), 10), before[1], "the open similarity session")
        em.similar_end()
        em.recommend_end()
    finally:
        em.close()
    fresh = hip.HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R)     # no parameters yet
    try:
        fresh.inform_begin()
        refused(hip, lib.E_INVALID, fresh.inform_add)
    finally:
        fresh.close()                                                    # (destroy ends the open session)


# ---- 8. the front door ------------------------------------------------------------------------------------------------------
def frame_of(answer, row_labels, item_labels):
    items, vals, counts = answer
    rows = [(row_labels[b], item_labels[items[b, k]], vals[b, k], k + 1) for b in range(len(row_labels))
            for k in range(counts[b])]
    return pd.DataFrame(rows, columns=["users", "items", "gain", "rank"])


def same_frame(got, want, columns=("users", "items", "gain", "rank")):
    assert list(got.columns) == list(columns)
    for col in columns:
        if col != "gain":
            assert got[col].tolist() == want[col].tolist(), col
    assert np.array_equal(xm.bits(got["gain"].to_numpy(dtype=np.float64)), xm.bits(want["gain"].to_numpy(dtype=np.float64)))


def test_the_host_class_with_string_ids(hip):
    rng = np.random.default_rng(12)
    n_u, n_i, n_obs = 60, 150, 1500
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 6, iterations=8, sampling=2, seed=5)
    model.fit(df, silent=True)
    enc = model.data_handler
    ul, il = list(enc.user_labels()), list(enc.item_labels())
    ask = ["u7", "u1", "u7", "u30"]
    stock = il[10:90]
    copycat = df[df["users"] == "u7"].assign(users="u7-again")            # a new user with a training user's rows
    new = pd.concat([copycat, pd.DataFrame({"users": ["zoe", "al", "zoe"], "items": [il[3], il[10], il[50]],
                                            "ratings": [5, 1, 4]})], ignore_index=True)
    got_items = model.informative_items(users=ask, n=5)
    got_within = model.informative_items(users=ask, n=5, exclude_seen=False, candidates=stock, exclude=[("u1", il[12])])
    got_first = model.interview(n=7, candidates=stock)
    got_new = model.ask_next(new, n=4, prior=1.0, iterations=20)
    got_fold = model.ask_next(new, n=4, prior=0, iterations=20)
    folds = np.stack([t.to_numpy() for t in model.fold_in(new, iterations=20)])
    new_labels = list(dict.fromkeys(new["users"]))
    rows = np.stack([[new_labels.index(u) for u in new["users"]], [il.index(i) for i in new["items"]]], 1)
    params = [(r["theta"], r["eta"], r["pr"]) for r in model.results]
    K, R = params[0][0].shape[1], params[0][2].shape[2]
    ids = np.array([ul.index(u) for u in ask], dtype=np.int32)
    cand = np.array(sorted(il.index(i) for i in stock), dtype=np.int32)
    em = context(hip, np.asarray(model.train), params, len(ul), len(il), R)
    try:
        with Session(em, 2):
            mean = em.inform_mean_theta()
            seen = ir.train_lists(rows, np.arange(len(new_labels)))
            d = np.bincount(rows[:, 0], minlength=len(new_labels)).astype(np.float64)[None, :, None]
            want_items = em.inform_query(ids, 5)
            own = (np.array([0, 0, 1, 1, 1], dtype=np.int64), np.array([il.index(il[12])], dtype=np.int32))
            want_within = em.inform_query(ids, 5, cand, own, False)
            want_first = em.inform_query_theta(mean[:, None, :], 7, None, cand)
            want_new = em.inform_query_theta((d * folds + 1.0 * mean[:, None, :]) / (d + 1.0), 4, seen)
            want_fold = em.inform_query_theta(folds, 4, seen)
    finally:
        em.close()
    same_frame(got_items, frame_of(want_items, ask, il))
    same_frame(got_within, frame_of(want_within, ask, il))
    same_frame(got_first, frame_of(want_first, ["x"], il).drop(columns="users"), ("items", "gain", "rank"))
    same_frame(got_new, frame_of(want_new, new_labels, il))
    same_frame(got_fold, frame_of(want_fold, new_labels, il))
    assert folds.shape == (2, 3, K) and got_fold["users"].tolist()[:4] == ["u7-again"] * 4
    assert not set(zip(got_new["users"], got_new["items"])) & set(zip(new["users"], new["items"]))


# ---- 9. coverage --------------------------------------------------------------------------------------------------------------
def test_every_inform_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("inf_")]
    for k in ("inf_entropy_kernel", "inf_score_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
    for k in ("sim_mass_kernel", "sim_profile_kernel", "rec_exclude_kernel", "cat_exclude_kernel"):
        assert k in names, (k, sorted(names))
    assert len({n for n in names if n.startswith("rec_select_kernel<")}) == 2, sorted(names)
