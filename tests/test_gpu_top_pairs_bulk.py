"""The m best (user, item) pairs beyond 1,024 on the device (mmsbm_hip_recommend_top_pairs_bulk,
mmsbm_hip_recommend_pair_bar, pairs_bulk.hpp).  Every comparison is by EQUALITY: ids, counts and padding as integers,
scores and the bar by their bits; there is no tolerance.

1. the exact models of exact_models.py against the restatement (test_top_pairs_cpu.restate_top_pairs), with the m of
   test_top_pairs_bulk_cpu.bulk_ms -- among them the tie-derived m, which that file shows to sit inside a tie group that
   spans three user tiles -- and the bar, the counts above and at it;
2. the two paths meet: m in {1, 10, 300, 1,024} against recommend_top_pairs, entry for entry;
3. random dense models against the host-sorted rows of recommend_query(all users, n = I), also after
   recommend_add_items, on a shuffled subset and on a swapped context;
4. the options change nothing: workgroups, digit width, early-stop size -- and the passes they force are read back;
5. 120,000 x 20,000: more than 2^31 pairs, and a constant model that puts 2.4e9 pairs into one bin;
6. recommend_pair_bar and recommend_audience at the bar; refusals by status code; no side effects; the launch log.

MMSBM_E_TOOLARGE is the one refusal not provoked here: it needs a device without free memory.
"""
import os
import sys

import numpy as np
import pytest

import exact_models as xm
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip, problem  # noqa: F401  (hip: the fixture)
from test_gpu_serving_exact import open_session
from test_recommend_cpu import seen_items
from test_top_pairs_bulk_cpu import bulk_ms, case_order, restate_info, tie_m
from test_top_pairs_cpu import MS, restate_top_pairs

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

VARIANT_IDS = [f"{f}-{k}" for f, k in xm.VARIANTS]
SHAPE_ID = lambda s: "U{}I{}K{}L{}R{}S{}".format(*s)  # noqa: E731
WINDOW = {}
SCORE_BUFFER_KERNELS = ("rec_score_kernel", "rec_exclude_kernel", "rec_select_kernel<")
NEW_KERNELS = ("pbulk_tile_kernel<false>", "pbulk_tile_kernel<true>", "pbulk_seen_kernel", "pbulk_count_kernel",
               "pbulk_cut_kernel", "pbulk_emit_kernel<false>", "pbulk_emit_kernel<true>", "pbulk_sortkey_kernel",
               "pbulk_gather_kernel")
# (five of test_gpu_top_pairs.py: U < 128, S = 1 and 3, K <= L and K > L, one user, a tile border at 128 + 1 and 128 - 1)
SMALL = [(100, 300, 4, 6, 3, 1), (100, 300, 6, 4, 3, 3), (129, 130, 3, 3, 4, 1), (1, 700, 5, 3, 4, 3), (127, 128, 2, 5, 2, 1)]


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


def same_pairs(got, want, what):
    """(users, items, scores, count) equal in every entry, the padding included, scores by their bits."""
    assert got[3] == want[3], f"{what}: count {got[3]}, expected {want[3]}"
    for g, w, nm in zip(got[:3], want[:3], ("users", "items", "scores")):
        gb, wb = (xm.bits(g), xm.bits(w)) if nm == "scores" else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        assert gb.shape == wb.shape, (what, nm, gb.shape, wb.shape)
        if not np.array_equal(gb, wb):
            at = int(np.flatnonzero(gb != wb)[0])
            raise AssertionError(f"{what}: {nm} differ in {int((gb != wb).sum())} entries, first at {at}: "
                                 f"device {np.asarray(g)[at]}, expected {np.asarray(w)[at]}")


def same_info(got, want, what):
    assert xm.bits(got["bar"]) == xm.bits(want["bar"]), f"{what}: bar {got['bar']!r}, expected {want['bar']!r}"
    for k in ("above", "ties", "candidates"):
        assert got[k] == want[k], f"{what}: {k} {got[k]}, expected {want[k]}"


def check_bulk(em, m, users, scores, seen, what, ask=None):
    """One bulk query and the bar alone against the restatement."""
    want = restate_top_pairs(None, None, users, m, seen, scores=scores)
    info = restate_info(scores, users, seen, m)
    *got, got_info = em.recommend_top_pairs_bulk(m, ask)
    same_pairs(got, want, what)
    same_info(got_info, info, what)
    return got, got_info


def sorted_query(em, users, n_items, m):
    """The first m of the host-sorted rows of recommend_query(users, n = I): the parent's exact answer for any m (I <=
    1,024 here, so a row holds every candidate of its user)."""
    users = np.sort(np.asarray(users, dtype=np.int32))
    items, scores, counts = em.recommend_query(users, n_items)
    keep = np.arange(n_items)[None, :] < counts[:, None]
    u = np.repeat(users.astype(np.int64), counts)
    i, s = items[keep].astype(np.int64), scores[keep]
    order = np.lexsort((i, u, -s))
    count = min(m, len(order))
    cut = order[:count]
    ou, oi, os_ = np.full(m, -1, dtype=np.int32), np.full(m, -1, dtype=np.int32), np.full(m, -np.inf)
    ou[:count], oi[:count], os_[:count] = u[cut], i[cut], s[cut]
    bar = (s[cut[-1]] + 0.0) if count else -np.inf
    return (ou, oi, os_, count), {"bar": float(bar), "above": int((s > bar).sum()), "ties": int((s == bar).sum()),
                                  "candidates": int(len(s))}


# ---- 1. exact, by equality ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.MANY, ids=SHAPE_ID)
@pytest.mark.parametrize("variant", xm.VARIANTS, ids=VARIANT_IDS)
def test_every_pair_is_exact(hip, variant, shape):
    """300 x 997 (K < L, S = 3) and 260 x 1,021 (K > L, S = 4): 299,100 and 265,460 pairs, three user tiles, partial
    tiles on both sides; m = 1,025; 4,096; the tie-derived m; candidates - 1; candidates; candidates + 7."""
    U, I, K, L, R, S = shape
    case = case_order(*variant, shape, False)[0]
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (False, True):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)
            for m in bulk_ms(*variant, shape, exclude):
                check_bulk(em, m, case["users"], case["scores"], seen, f"{variant} {shape} exclude={exclude} m={m}")
            em.recommend_end()
    finally:
        em.close()


@pytest.mark.parametrize("shape", SMALL, ids=SHAPE_ID)
@pytest.mark.parametrize("variant", xm.VARIANTS, ids=VARIANT_IDS)
def test_small_shapes_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    family, kind = variant
    rng = np.random.default_rng(xm.case_seed(family, kind, shape))
    params, w = xm.model(family, rng, U, I, K, L, R, S, kind)
    data = np.stack([rng.integers(0, U, 5 * U + 20), rng.integers(0, I, 5 * U + 20), rng.integers(0, R, 5 * U + 20)], 1)
    users = np.arange(U, dtype=np.int32)
    scores = xm.exact_scores(params, users, I, w)
    seen = seen_items(data, U)
    em = context(hip, data, params, U, I, R)
    try:
        for exclude in (False, True):
            open_session(em, S, w, exclude)
            sn = seen if exclude else None
            candidates = restate_info(scores, users, sn, 1)["candidates"]
            for m in (1025, candidates):
                check_bulk(em, m, users, scores, sn, f"{variant} {shape} exclude={exclude} m={m}")
            em.recommend_end()
    finally:
        em.close()


# ---- 2. the two paths meet ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", xm.FAMILIES)
def test_the_bulk_entry_equals_top_pairs_up_to_1024(hip, family):
    shape = xm.MANY[xm.FAMILIES.index(family) % 2]
    U, I, K, L, R, S = shape
    case = case_order(family, "signed", shape, True)[0]
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (False, True):
            open_session(em, S, case["w"], exclude)
            for m in MS:
                same_pairs(em.recommend_top_pairs_bulk(m)[:4], em.recommend_top_pairs(m), f"{family} exclude={exclude} m={m}")
            em.recommend_end()
    finally:
        em.close()


# ---- 3. random dense models: recommend_query as the yardstick -----------------------------------------------------------
@pytest.mark.parametrize("shape", [(300, 997, 7, 9, 5, 3), (1021, 700, 20, 20, 5, 2), (260, 1000, 12, 5, 4, 1)], ids=SHAPE_ID)
def test_random_models_equal_the_sorted_recommend_query(hip, shape):
    U, I, K, L, R, S = shape
    m = 5000
    data, params = problem(U, I, R, K, L, S, 6 * U, seed=U + I)
    w = np.arange(1.0, R + 1)
    rng = np.random.default_rng(5)
    subset = rng.permutation(rng.choice(U, 77, replace=False)).astype(np.int32)   # shuffled: not in id order
    em = context(hip, data, params, U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, w, exclude)
            for ask, ids in ((None, np.arange(U)), (subset, subset)):
                want, info = sorted_query(em, ids, I, m)
                *got, got_info = em.recommend_top_pairs_bulk(m, ask)
                same_pairs(got, want, f"{shape} exclude={exclude} subset={ask is not None}")
                same_info(got_info, info, f"{shape} exclude={exclude} subset={ask is not None}")
            assert em.get_option("pairs_bulk_ms") > 0
            em.recommend_end()
    finally:
        em.close()


def test_after_added_items(hip):
    U, I, K, L, R, S, n_new, m = 300, 500, 6, 9, 4, 2, 45, 5000
    data, params = problem(U, I, R, K, L, S, 2000, seed=21)
    rng = np.random.default_rng(22)
    eta_new = rng.random((S, n_new, L))
    off = np.concatenate([[0], np.cumsum(rng.integers(0, 40, n_new))]).astype(np.int64)
    seen_users = rng.integers(0, U, off[-1]).astype(np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, np.arange(1.0, R + 1), exclude)
            em.recommend_add_items(eta_new, (off, seen_users))
            want, info = sorted_query(em, np.arange(U), I + n_new, m)
            *got, got_info = em.recommend_top_pairs_bulk(m)
            same_pairs(got, want, f"added items exclude={exclude}")
            same_info(got_info, info, f"added items exclude={exclude}")
            assert (got[1][:got[3]] >= I).any()                              # new items are among the best
            named = set(zip(np.repeat(np.arange(n_new), np.diff(off)).tolist(), seen_users.tolist()))
            assert not [(j, u) for u, j in zip(got[0].tolist(), got[1].tolist()) if (j - I, u) in named]
            everything, _ = sorted_query(em, np.arange(U), I + n_new, U * (I + n_new))
            same_pairs(em.recommend_top_pairs_bulk(info["candidates"] + 3)[:4],
                       tuple(a[:info["candidates"] + 3] for a in everything[:3]) + (info["candidates"],), "every candidate")
            em.recommend_end()
    finally:
        em.close()


def test_a_swapped_context_gives_the_same_bits(hip):
    U, I, K, L, R, S, m = 300, 800, 12, 7, 5, 2, 5000
    data, params = problem(U, I, R, K, L, S, 3000, seed=11)
    w = np.arange(1.0, R + 1)
    answers = []
    for swap in (0, 1):
        em = context(hip, data, params, U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            open_session(em, S, w, True)
            answers.append(em.recommend_top_pairs_bulk(m))
            want, info = sorted_query(em, np.arange(U), I, m)
            same_pairs(answers[-1][:4], want, f"swap={swap}")
            same_info(answers[-1][4], info, f"swap={swap}")
            em.recommend_end()
        finally:
            em.close()
    same_pairs(answers[1][:4], answers[0][:4], "swapped / unswapped")
    same_info(answers[1][4], answers[0][4], "swapped / unswapped")


# ---- 4. the options change the route, not the answer ---------------------------------------------------------------------
@pytest.mark.parametrize("variant", [("interleaved", "stars"), ("mixed", "signed"), ("constant", "signed")], ids=lambda v: "-".join(v))
def test_the_answer_does_not_depend_on_groups_bits_or_the_early_stop(hip, variant):
    """A tie case (test_top_pairs_bulk_cpu.py: m inside a tie group that spans every user tile, so the cut by (user,
    item) crosses the borders between the workgroups' runs of the 24 tiles), a signed case with both signs and exact
    zeros, and the constant model.  pairs_bulk_collect = 0 runs every pass of the select; 5,000 stops after some; the
    default collects the 300,000 pairs outright."""
    shape = xm.MANY[0]
    U, I, K, L, R, S = shape
    case = case_order(*variant, shape, False)[0]
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        default_collect = em.get_option("pairs_bulk_collect")
        assert default_collect == 2.0 ** 20 and em.get_option("pairs_bulk_groups") == 0 and em.get_option("pairs_bulk_bits") == 0
        for exclude in (False, True):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)
            for m in (tie_m(*variant, shape, exclude)[0], 4096):
                want = restate_top_pairs(None, None, case["users"], m, seen, scores=case["scores"])
                info = restate_info(case["scores"], case["users"], seen, m)
                routes = set()
                for groups in (1, 2, 7, 0):
                    for bits in (4, 8, 0):
                        for collect in (0, 5000, default_collect):
                            for name, v in (("pairs_bulk_groups", groups), ("pairs_bulk_bits", bits), ("pairs_bulk_collect", collect)):
                                em.set_option(name, v)
                                assert em.get_option(name) == v
                            what = f"{variant} exclude={exclude} m={m} groups={groups} bits={bits} collect={collect}"
                            *got, got_info = em.recommend_top_pairs_bulk(m)
                            same_pairs(got, want, what)
                            same_info(got_info, info, what)
                            same_info(em.recommend_pair_bar(m), info, what + " (bar alone)")
                            passes, collected = em.get_option("pairs_bulk_passes"), em.get_option("pairs_bulk_collected")
                            if collect == 0:
                                assert passes == -(-64 // (bits or 12)) and collected == 0, what   # every digit
                            elif collect == default_collect:
                                assert passes == 0 and collected == info["candidates"], what        # no pass at all
                            else:
                                assert collected <= collect, what
                            routes.add((passes, collected > 0))
                assert len(routes) >= 4, routes                                  # several passes, early and late collection
            em.recommend_end()
    finally:
        em.close()


# ---- 5. more than 2^31 pairs ---------------------------------------------------------------------------------------------
def test_more_than_2_to_the_31_pairs_on_a_random_model(hip):
    """120,000 x 20,000 = 2.4e9 pairs: 64-bit tile, pair and bin counts.  The first 1,024 of m = 3,000 are
    recommend_top_pairs' answer, the list is in the query's order, nothing in it scores below the bar."""
    U, I, K, L, R, S, m = 120_000, 20_000, 4, 4, 3, 1, 3000
    assert U * I > 2 ** 31
    data, params = problem(U, I, R, K, L, S, 400_000, seed=31)
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, np.arange(1.0, R + 1), True)
        gu, gi, gs, count, info = em.recommend_top_pairs_bulk(m)
        print(f"pairs_bulk_ms {em.get_option('pairs_bulk_ms'):.2f}, passes {em.get_option('pairs_bulk_passes'):.0f}, "
              f"collected {em.get_option('pairs_bulk_collected'):.0f}")
        first = em.recommend_top_pairs(1024)
        em.recommend_end()
    finally:
        em.close()
    assert count == m and info["candidates"] == U * I - len(np.unique(data[:, 0] * I + data[:, 1]))
    same_pairs((gu[:1024], gi[:1024], gs[:1024], 1024), first, "the prefix of 1,024")
    assert np.array_equal(np.lexsort((gi, gu, -gs)), np.arange(m))             # sorted, no pair twice
    assert len(set(zip(gu.tolist(), gi.tolist()))) == m
    assert (gs >= info["bar"]).all() and xm.bits(gs[-1] + 0.0) == xm.bits(info["bar"])
    assert info["above"] < m <= info["above"] + info["ties"]
    seen = set(zip(data[:, 0].tolist(), data[:, 1].tolist()))
    assert not [1 for u, i in zip(gu.tolist(), gi.tolist()) if (u, i) in seen]


def test_more_than_2_to_the_31_pairs_in_one_bin(hip):
    """The constant model over 120,000 x 20,000: every pair ties, one bin of the histogram holds 2.4e9 pairs; m = 2,000
    returns user 0's first 2,000 candidate items."""
    U, I, K, L, R, S, m = 120_000, 20_000, 4, 3, 3, 1, 2000
    rng = np.random.default_rng(8)
    params, w = xm.model("constant", rng, U, I, K, L, R, S, "stars")
    data = np.stack([rng.integers(0, U, 300_000), rng.integers(0, I, 300_000), rng.integers(0, R, 300_000)], 1)
    data[:50, 0], data[:50, 1] = 0, np.arange(0, 100, 2)                       # user 0 has seen items 0, 2, .., 98
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, w, True)
        gu, gi, gs, count, info = em.recommend_top_pairs_bulk(m)
        print(f"pairs_bulk_ms {em.get_option('pairs_bulk_ms'):.2f}, passes {em.get_option('pairs_bulk_passes'):.0f}")
        assert em.get_option("pairs_bulk_passes") == 6 and em.get_option("pairs_bulk_collected") == 0
        em.recommend_end()
    finally:
        em.close()
    candidates = U * I - len(np.unique(data[:, 0] * I + data[:, 1]))
    assert candidates > 2 ** 31
    seen0 = set(data[data[:, 0] == 0, 1].tolist())
    want = np.array([i for i in range(I) if i not in seen0][:m])
    score = xm.exact_scores(params, [0], I, w)[0, 0]
    assert count == m and (gu == 0).all() and np.array_equal(gi, want)
    assert np.array_equal(xm.bits(gs), xm.bits(np.full(m, score)))
    assert info == {"bar": float(score), "above": 0, "ties": candidates, "candidates": candidates}


# ---- 6. the bar, refusals, side effects, launches ------------------------------------------------------------------------
def test_the_bar_alone_and_the_audience_at_the_bar(hip):
    U, I, K, L, R, S = 300, 997, 7, 9, 5, 3
    data, params = problem(U, I, R, K, L, S, 2000, seed=17)
    case = case_order("rare", "stars", xm.MANY[0], True)[0]
    rng = np.random.default_rng(2)
    subset = rng.permutation(U)[:130].astype(np.int32)
    for what, dt, pr, w in (("random", data, params, np.arange(1.0, R + 1)), ("rare", case["data"], case["params"], case["w"])):
        em = context(hip, dt, pr, U, I, R)
        try:
            for exclude in (True, False):
                open_session(em, S, w, exclude)
                for m in (1, 1025, 40_000, U * I):
                    for ask in (None, subset):
                        info = em.recommend_top_pairs_bulk(m, ask)[4]
                        same_info(em.recommend_pair_bar(m, ask), info, f"{what} exclude={exclude} m={m}")
                        assert info["above"] < min(m, info["candidates"]) <= info["above"] + info["ties"]
                    info = em.recommend_pair_bar(m)                  # (every user: the audience has no user filter)
                    sizes = np.diff(em.recommend_audience(np.arange(I), info["bar"], count_only=True)[0])
                    assert int(sizes.sum()) == info["above"] + info["ties"], (what, exclude, m)
                em.recommend_end()
        finally:
            em.close()


def refused(hip, code, fn, *args):
    with pytest.raises(hip._lib.HipLibraryError) as e:
        fn(*args)
    assert e.value.code == code, (e.value.code, e.value.message)


def test_refusals_by_status_code(hip):
    U, I, K, L, R = 50, 60, 4, 3, 3
    data, params = problem(U, I, R, K, L, 1, 300, seed=2)
    lib = hip._lib
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R)
    try:
        for fn in (em.recommend_top_pairs_bulk, em.recommend_pair_bar):
            refused(hip, lib.E_INVALID, fn, 3)                                   # no session
        em.recommend_begin(w, True)
        for fn in (em.recommend_top_pairs_bulk, em.recommend_pair_bar):
            refused(hip, lib.E_INVALID, fn, 3)                                   # before the first add
        em.recommend_add()
        for fn in (em.recommend_top_pairs_bulk, em.recommend_pair_bar):
            for bad in (-1, U):
                refused(hip, lib.E_INVALID, fn, 3, [0, bad])
            refused(hip, lib.E_INVALID, fn, 3, [7, 2, 7])                        # a repeated id
            for bad in (0, -2):
                refused(hip, lib.E_INVALID, fn, bad)
        refused(hip, lib.E_UNSUPPORTED, em.recommend_pair_bar, hip.HipEM.MAX_TOP_PAIRS_BULK + 1)
        refused(hip, lib.E_UNSUPPORTED, em.recommend_top_pairs, hip.HipEM.MAX_TOP_PAIRS + 1)   # top_pairs keeps its bound
        for name, bad in (("pairs_bulk_groups", -1), ("pairs_bulk_groups", 4097), ("pairs_bulk_groups", 2.5),
                          ("pairs_bulk_bits", 13), ("pairs_bulk_bits", -1), ("pairs_bulk_bits", 1.5),
                          ("pairs_bulk_collect", -1), ("pairs_bulk_collect", 2.0 ** 24 + 1), ("pairs_bulk_ms", 1)):
            refused(hip, lib.E_INVALID, em.set_option, name, bad)
        info = em.recommend_pair_bar(hip.HipEM.MAX_TOP_PAIRS_BULK)              # the bound itself: every candidate
        assert info["above"] + info["ties"] == info["candidates"] == U * I - len(np.unique(data[:, 0] * I + data[:, 1]))
        gu, gi, gs, count, info = em.recommend_top_pairs_bulk(5, [])            # nobody asked for: nothing
        assert count == 0 and (gu == -1).all() and (gi == -1).all() and np.isneginf(gs).all()
        assert info == {"bar": -np.inf, "above": 0, "ties": 0, "candidates": 0}
        want, info = sorted_query(em, np.arange(U), I, 2000)
        same_pairs(em.recommend_top_pairs_bulk(2000)[:4], want, "the session is still usable")
        em.recommend_end()
        refused(hip, lib.E_INVALID, em.recommend_top_pairs_bulk, 3)
    finally:
        em.close()


def test_no_side_effects(hip):
    U, I, K, L, R, S = 200, 300, 6, 5, 5, 3
    data, params = problem(U, I, R, K, L, S, 1500, seed=13)
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
        open_session(em, S, w, True)
        rec = em.recommend_query(np.arange(U), 10)
        top = em.recommend_top_pairs(300)
        first = em.recommend_top_pairs_bulk(3000)
        em.recommend_pair_bar(3000)
        same_pairs(em.recommend_top_pairs_bulk(3000)[:4], first[:4], "a second query")
        rec2 = em.recommend_query(np.arange(U), 10)
        top2 = em.recommend_top_pairs(300)
        em.recommend_end()
        after = [em.select(s).get_params() for s in range(S)]
    finally:
        em.close()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(xm.bits(a), xm.bits(b))
    for g, h in zip(rec + top[:3], rec2 + top2[:3]):
        assert np.array_equal(xm.bits(g) if g.dtype == np.float64 else g, xm.bits(h) if h.dtype == np.float64 else h)


def test_a_query_launches_no_score_buffer_kernel(hip):
    U, I, K, L, R, S = 300, 997, 7, 9, 5, 2
    data, params = problem(U, I, R, K, L, S, 2000, seed=17)
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, np.arange(1.0, R + 1), True)
        with LaunchWindow() as lw:
            em.recommend_top_pairs_bulk(3000)
            em.set_option("pairs_bulk_collect", 0)
            em.recommend_top_pairs_bulk(3000, np.arange(5))
            em.recommend_pair_bar(10)
            em.recommend_end()
            em.close()                                     # (the log is written when the context goes)
            names = lw.names()
    finally:
        em.close()
    for k in ("pbulk_tile_kernel<false>", "pbulk_tile_kernel<true>", "pbulk_seen_kernel", "pbulk_count_kernel",
              "pbulk_emit_kernel<true>", "pbulk_sortkey_kernel", "pbulk_gather_kernel"):
        assert k in names, (k, sorted(names))
    assert not [n for n in names if n.startswith(SCORE_BUFFER_KERNELS) or n.startswith("gtop_")], sorted(names)


def test_every_new_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("pbulk_")]
    for k in NEW_KERNELS:
        assert k in compiled, (k, compiled)
    assert sorted(compiled) == sorted(NEW_KERNELS)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
