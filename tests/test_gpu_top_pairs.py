"""The m best (user, item) pairs of the whole model on the device (mmsbm_hip_recommend_top_pairs,
HipEM.recommend_top_pairs, top_pairs.hpp):

1. by EQUALITY with the exact reference on the models of exact_models.py -- ids, count, padding, scores by their bits;
   test_top_pairs_cpu.py asserts on the restatement that pair m and pair m + 1 tie in these cases and that the tie
   group spans several tiles, so the tie-break by (user id, item id) decides every answer;
2. by EQUALITY with the existing path on general models: the first m of the host-sorted rows of
   recommend_query(all users, n = m) -- the same fma chain, so no tolerance;
3. against the numpy restatement (another association order) within TOL x max |restated score|, the tolerance of
   test_gpu_recommend.py, with no pair left out of the comparison;
4. the identities: the answer does not depend on the number of workgroups, on the order of the request, on the side
   layout or on where the parameters came from; more than 2^31 pairs; fewer candidates than m; none at all;
5. refusals by status code, no side effects, and the launch log: every gtop_ kernel launched here, and a query launches
   none of the score-buffer kernels.

MMSBM_E_TOOLARGE is the one refusal not provoked here: it needs a device without free memory.
"""
import os
import sys

import numpy as np
import pytest

import exact_models as xm
from conftest import ROOT
from test_gpu_recommend import TOL, LaunchWindow, context, hip, problem  # noqa: F401  (hip: the fixture)
from test_gpu_serving_exact import open_session
from test_recommend_cpu import restate_scores, seen_items
from test_top_pairs_cpu import MS, global_order, restate_top_pairs

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

VARIANT_IDS = [f"{f}-{k}" for f, k in xm.VARIANTS]
SHAPE_ID = lambda s: "U{}I{}K{}L{}R{}S{}".format(*s)  # noqa: E731
WINDOW = {}
SCORE_BUFFER_KERNELS = ("rec_score_kernel", "rec_exclude_kernel", "rec_select_kernel<")


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
        if not np.array_equal(gb, wb):
            at = int(np.flatnonzero(gb != wb)[0])
            raise AssertionError(f"{what}: {nm} differ in {int((gb != wb).sum())} entries, first at {at}: "
                                 f"device {np.asarray(g)[at]}, expected {np.asarray(w)[at]}")


def merged_query(em, users, m):
    """The global first m out of recommend_query(users, n = m): every row of the per-user answer, sorted on the host by
    (-score, user, item).  The global m best are among the per-user m best, so this is the parent's exact answer."""
    users = np.sort(np.asarray(users, dtype=np.int32))
    items, scores, counts = em.recommend_query(users, m)
    keep = np.arange(m)[None, :] < counts[:, None]
    u = np.repeat(users.astype(np.int64), counts)
    i, s = items[keep].astype(np.int64), scores[keep]
    order = np.lexsort((i, u, -s))[:m]
    count = len(order)
    ou, oi, os_ = np.full(m, -1, dtype=np.int32), np.full(m, -1, dtype=np.int32), np.full(m, -np.inf)
    ou[:count], oi[:count], os_[:count] = u[order], i[order], s[order]
    return ou, oi, os_, count


# ---- 1. exact, by equality ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.MANY, ids=SHAPE_ID)
@pytest.mark.parametrize("variant", xm.VARIANTS, ids=VARIANT_IDS)
def test_every_pair_is_exact(hip, variant, shape):
    """300 x 997 (K < L, S = 3) and 260 x 1,021 (K > L, S = 4): partial tiles on both sides, three user tiles."""
    U, I, K, L, R, S = shape
    case = xm.make_case(*variant, shape)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (False, True):
            seen = case["seen"] if exclude else None
            open_session(em, S, case["w"], exclude)
            for m in MS:
                want = restate_top_pairs(None, None, case["users"], m, seen, scores=case["scores"])
                same_pairs(em.recommend_top_pairs(m), want, f"{variant} {shape} exclude={exclude} m={m}")
            em.recommend_end()
    finally:
        em.close()


SMALL = [(100, 300, 4, 6, 3, 1), (100, 300, 6, 4, 3, 3), (129, 130, 3, 3, 4, 1), (1, 700, 5, 3, 4, 3), (127, 128, 2, 5, 2, 1)]


@pytest.mark.parametrize("shape", SMALL, ids=SHAPE_ID)
@pytest.mark.parametrize("variant", xm.VARIANTS, ids=VARIANT_IDS)
def test_small_shapes_are_exact(hip, variant, shape):
    """U < 128, S = 1 and 3, K <= L and K > L, one user, a tile border at 128 + 1 and 128 - 1."""
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
            for m in MS:
                want = restate_top_pairs(None, None, users, m, seen if exclude else None, scores=scores)
                same_pairs(em.recommend_top_pairs(m), want, f"{variant} {shape} exclude={exclude} m={m}")
            em.recommend_end()
    finally:
        em.close()


@pytest.mark.parametrize("variant", [("mixed", "signed"), ("constant", "stars"), ("constant", "signed")], ids=lambda v: "-".join(v))
def test_one_item_is_exact(hip, variant):
    U, I, K, L, R, S = 300, 1, 4, 3, 3, 3
    family, kind = variant
    rng = np.random.default_rng(7)
    params, w = xm.model(family, rng, U, I, K, L, R, S, kind)
    data = np.stack([np.arange(0, U, 3), np.zeros(U // 3, dtype=np.int64), rng.integers(0, R, U // 3)], 1)
    users = np.arange(U, dtype=np.int32)
    scores = xm.exact_scores(params, users, I, w)
    em = context(hip, data, params, U, I, R)
    try:
        for exclude in (False, True):
            open_session(em, S, w, exclude)
            for m in MS:
                want = restate_top_pairs(None, None, users, m, seen_items(data, U) if exclude else None, scores=scores)
                same_pairs(em.recommend_top_pairs(m), want, f"{variant} exclude={exclude} m={m}")
            em.recommend_end()
    finally:
        em.close()


# ---- 2. general models: the existing path as the yardstick ---------------------------------------------------------------
GENERAL = [(300, 997, 7, 9, 5, 3), (1021, 700, 20, 20, 5, 2), (260, 1500, 12, 5, 4, 1)]


@pytest.mark.parametrize("shape", GENERAL, ids=SHAPE_ID)
def test_general_models_equal_the_merged_recommend_query(hip, shape):
    U, I, K, L, R, S = shape
    data, params = problem(U, I, R, K, L, S, 6 * U, seed=U + I)
    w = np.arange(1.0, R + 1)
    rng = np.random.default_rng(5)
    subset = rng.choice(U, 77, replace=False).astype(np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, w, exclude)
            for m in MS:
                same_pairs(em.recommend_top_pairs(m), merged_query(em, np.arange(U), m), f"{shape} exclude={exclude} m={m}")
                same_pairs(em.recommend_top_pairs(m, subset), merged_query(em, subset, m), f"{shape} subset m={m}")
            assert em.get_option("top_pairs_ms") > 0
            em.recommend_end()
    finally:
        em.close()


def test_after_added_items(hip):
    U, I, K, L, R, S, n_new = 300, 500, 6, 9, 4, 2, 45
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
            for m in (10, 1024):
                got = em.recommend_top_pairs(m)
                same_pairs(got, merged_query(em, np.arange(U), m), f"added items exclude={exclude} m={m}")
            named = set(zip(np.repeat(np.arange(n_new), np.diff(off)).tolist(), seen_users.tolist()))
            assert not [(j, u) for u, j in zip(got[0].tolist(), got[1].tolist()) if (j - I, u) in named]
            em.recommend_end()
    finally:
        em.close()


def test_swapped_contexts_resident_and_uploaded_parameters_are_bitwise_equal(hip):
    U, I, K, L, R, S = 300, 800, 12, 7, 5, 2
    data, params = problem(U, I, R, K, L, S, 3000, seed=11)
    w = np.arange(1.0, R + 1)
    answers = []
    for swap in (0, 1):
        em = context(hip, data, params, U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            open_session(em, S, w, True)
            answers.append({m: em.recommend_top_pairs(m) for m in (10, 300)})
            for m in (10, 300):
                same_pairs(answers[-1][m], merged_query(em, np.arange(U), m), f"swap={swap} m={m}")
            em.recommend_end()
        finally:
            em.close()
    for m in (10, 300):
        same_pairs(answers[1][m], answers[0][m], f"swap m={m}")
    em = context(hip, data, params, U, I, R)
    try:
        em.iterate(3)                                      # resident slots, moved by the EM loop
        fitted = [em.select(s).get_params() for s in range(S)]
        open_session(em, S, w, True)
        resident = em.recommend_top_pairs(300)
        same_pairs(resident, merged_query(em, np.arange(U), 300), "resident")
        em.recommend_end()
    finally:
        em.close()
    other = context(hip, data, fitted, U, I, R)
    try:
        open_session(other, S, w, True)
        same_pairs(other.recommend_top_pairs(300), resident, "uploaded / resident")
        other.recommend_end()
    finally:
        other.close()


# ---- 3. general models against the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", [((300, 997, 7, 9, 5, 3), 0), ((260, 1021, 9, 5, 4, 4), 1), ((700, 900, 20, 20, 5, 2), 2)],
                         ids=lambda v: SHAPE_ID(v) if isinstance(v, tuple) else f"seed{v}")
@pytest.mark.parametrize("exclude", [True, False], ids=["unseen_pairs", "all_pairs"])
def test_general_models_agree_with_the_restatement(hip, shape, seed, exclude):
    U, I, K, L, R, S = shape
    data, params = problem(U, I, R, K, L, S, 8 * U, seed=seed)
    w = np.arange(1.0, R + 1)
    users = np.arange(U)
    ref = restate_scores(params, users, I, w)
    tol = TOL * np.abs(ref).max()
    seen = seen_items(data, U)
    ru, ri, rs = global_order(ref, users, seen if exclude else None)
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, w, exclude)
        got = {m: em.recommend_top_pairs(m) for m in MS}
        em.recommend_end()
    finally:
        em.close()
    for m in MS:
        gu, gi, gs, count = got[m]
        assert count == m and len(set(zip(gu.tolist(), gi.tolist()))) == m
        if exclude:
            assert not [1 for u, i in zip(gu.tolist(), gi.tolist()) if i in seen[u]]
        err = np.abs(gs - ref[gu, gi])
        s_star = rs[m - 1]
        print(f"{shape} exclude={exclude} m={m}: largest score error {err.max():.3e} (tol {tol:.3e}), "
              f"lowest returned restated score - m-th best {np.min(ref[gu, gi]) - s_star:.3e}")
        assert (err <= tol).all(), err.max() / tol                              # every returned score
        assert (ref[gu, gi] >= s_star - tol).all()                              # every returned pair belongs there
        above = rs > s_star + tol                                               # every pair clearly above is returned
        returned = set(zip(gu.tolist(), gi.tolist()))
        assert all((u, i) in returned for u, i in zip(ru[above].tolist(), ri[above].tolist()))
        order = np.lexsort((gi, gu, -gs))                                       # the device's own order
        assert np.array_equal(order, np.arange(m))


# ---- 4. identities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [("constant", "stars"), ("interleaved", "signed"), ("rare", "indicator")], ids=lambda v: "-".join(v))
def test_the_answer_does_not_depend_on_the_number_of_workgroups(hip, variant):
    """`constant`: every pair scores the same, so the tie group of pair m crosses every border between two workgroups'
    runs of tiles, whatever their number (24 tiles: 1, 2, 7 workgroups and the library's choice, one per tile);
    `interleaved` / `rare`: the tie groups test_top_pairs_cpu.py shows to span several user and item tiles."""
    shape = xm.MANY[0]
    U, I, K, L, R, S = shape
    case = xm.make_case(*variant, shape)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (False, True):
            open_session(em, S, case["w"], exclude)
            for m in MS:
                want = restate_top_pairs(None, None, case["users"], m, case["seen"] if exclude else None, scores=case["scores"])
                for groups in (1, 2, 7, 0):
                    em.set_option("top_pairs_groups", groups)
                    assert em.get_option("top_pairs_groups") == groups
                    same_pairs(em.recommend_top_pairs(m), want, f"{variant} exclude={exclude} m={m} groups={groups}")
            em.recommend_end()
    finally:
        em.close()


def test_groups_and_request_order_on_a_general_model(hip):
    U, I, K, L, R, S = 1021, 1500, 8, 8, 5, 2
    data, params = problem(U, I, R, K, L, S, 6000, seed=9)
    rng = np.random.default_rng(3)
    sub = rng.choice(U, 400, replace=False).astype(np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, np.arange(1.0, R + 1), True)
        want = {m: em.recommend_top_pairs(m) for m in MS}
        want_sub = em.recommend_top_pairs(300, sub)
        for groups in (1, 2, 7, 100, 4096):
            em.set_option("top_pairs_groups", groups)
            for m in MS:
                same_pairs(em.recommend_top_pairs(m), want[m], f"groups={groups} m={m}")
            same_pairs(em.recommend_top_pairs(300, sub[::-1]), want_sub, f"groups={groups} reversed subset")
            same_pairs(em.recommend_top_pairs(300, rng.permutation(sub)), want_sub, f"groups={groups} permuted subset")
        em.set_option("top_pairs_groups", 0)
        same_pairs(em.recommend_top_pairs(300, np.arange(U)), want[300], "all users named")
        em.recommend_end()
    finally:
        em.close()


def test_more_than_2_to_the_31_pairs(hip):
    """120,000 x 20,000 = 2.4e9 pairs: 64-bit tile and pair counts; equal to the merged recommend_query answer."""
    U, I, K, L, R, S, m = 120_000, 20_000, 4, 4, 3, 1, 10
    assert U * I > 2 ** 31
    data, params = problem(U, I, R, K, L, S, 400_000, seed=31)
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, np.arange(1.0, R + 1), True)
        got = em.recommend_top_pairs(m)
        print(f"top_pairs_ms {em.get_option('top_pairs_ms'):.2f}")
        want = merged_query(em, np.arange(U), m)
        print(f"recommend_ms {em.get_option('recommend_ms'):.2f}")
        same_pairs(got, want, "120,000 x 20,000")
        assert got[3] == m
        em.recommend_end()
    finally:
        em.close()


def test_fewer_candidates_than_m_and_none_at_all(hip):
    U, I, K, L, R = 9, 20, 3, 4, 3
    rng = np.random.default_rng(4)
    _, params = problem(U, I, R, K, L, 2, 10, seed=4)
    every = np.stack([np.repeat(np.arange(U), I), np.tile(np.arange(I), U), rng.integers(0, R, U * I)], 1)
    w = np.arange(1.0, R + 1)
    em = context(hip, every, params, U, I, R)              # every pair is a training pair
    try:
        open_session(em, 2, w, True)
        for m in (1, 10, 1024):
            gu, gi, gs, count = em.recommend_top_pairs(m)
            assert count == 0 and (gu == -1).all() and (gi == -1).all() and np.isneginf(gs).all()
        em.recommend_end()
        open_session(em, 2, w, False)                     # 180 candidates
        got = em.recommend_top_pairs(1024)
        assert got[3] == U * I and (got[0][U * I:] == -1).all() and (got[1][U * I:] == -1).all() and np.isneginf(got[2][U * I:]).all()
        same_pairs(got, merged_query(em, np.arange(U), 1024), "180 candidates, m = 1024")
        same_pairs(em.recommend_top_pairs(1024, [4]), merged_query(em, [4], 1024), "one user")
        em.recommend_end()
    finally:
        em.close()
    some = every[(every[:, 0] != 5) | (every[:, 1] % 7 != 3)]          # user 5 keeps items 3, 10, 17
    em = context(hip, some, params, U, I, R)
    try:
        open_session(em, 2, w, True)
        gu, gi, gs, count = em.recommend_top_pairs(10)
        assert count == 3 and gu[:3].tolist() == [5, 5, 5] and sorted(gi[:3].tolist()) == [3, 10, 17]
        assert (gu[3:] == -1).all() and (gi[3:] == -1).all() and np.isneginf(gs[3:]).all()
        same_pairs((gu, gi, gs, count), merged_query(em, np.arange(U), 10), "three candidates")
        em.recommend_end()
    finally:
        em.close()


# ---- 5. refusals, side effects, launches ---------------------------------------------------------------------------------
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
        refused(hip, lib.E_INVALID, em.recommend_top_pairs, 3)                 # no session
        em.recommend_begin(w, True)
        refused(hip, lib.E_INVALID, em.recommend_top_pairs, 3)                 # before the first add
        em.recommend_add()
        for bad in (-1, U):
            refused(hip, lib.E_INVALID, em.recommend_top_pairs, 3, [0, bad])
        refused(hip, lib.E_INVALID, em.recommend_top_pairs, 3, [7, 2, 7])      # a repeated id
        for bad in (0, -2):
            refused(hip, lib.E_INVALID, em.recommend_top_pairs, bad)
        refused(hip, lib.E_UNSUPPORTED, em.recommend_top_pairs, hip.HipEM.MAX_TOP_PAIRS + 1)
        for bad in (-1, 4097, 2.5):
            refused(hip, lib.E_INVALID, em.set_option, "top_pairs_groups", bad)
        assert em.recommend_top_pairs(hip.HipEM.MAX_TOP_PAIRS)[3] == hip.HipEM.MAX_TOP_PAIRS
        gu, gi, gs, count = em.recommend_top_pairs(5, [])                       # nobody asked for: nothing
        assert count == 0 and (gu == -1).all() and np.isneginf(gs).all()
        same_pairs(em.recommend_top_pairs(5), merged_query(em, np.arange(U), 5), "the session is still usable")
        em.recommend_end()
        refused(hip, lib.E_INVALID, em.recommend_top_pairs, 3)
    finally:
        em.close()


def test_no_side_effects(hip):
    U, I, K, L, R, S = 200, 300, 6, 5, 5, 3
    data, params = problem(U, I, R, K, L, S, 1500, seed=13)
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
        test = data[:500]
        open_session(em, S, w, True)
        rec = em.recommend_query(np.arange(U), 10)
        pos = em.recommend_positions(np.arange(U), np.arange(U + 1, dtype=np.int64), np.arange(U, dtype=np.int32) % I)
        em.predict_begin(test, w)
        em.select(0).predict_add()
        first = em.recommend_top_pairs(300)                # inside an open predict session
        em.select(1).predict_add()
        mat, raw = em.predict_finish()
        same_pairs(em.recommend_top_pairs(300), first, "a second query")
        rec2 = em.recommend_query(np.arange(U), 10)
        pos2 = em.recommend_positions(np.arange(U), np.arange(U + 1, dtype=np.int64), np.arange(U, dtype=np.int32) % I)
        em.recommend_end()
        after = [em.select(s).get_params() for s in range(S)]
        em.predict_begin(test, w)
        em.select(0).predict_add()
        em.select(1).predict_add()
        mat2, raw2 = em.predict_finish()
    finally:
        em.close()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(xm.bits(a), xm.bits(b))
    for g, h in zip(rec + pos, rec2 + pos2):
        assert np.array_equal(xm.bits(g) if g.dtype == np.float64 else g, xm.bits(h) if h.dtype == np.float64 else h)
    assert np.array_equal(xm.bits(mat), xm.bits(mat2)) and np.array_equal(xm.bits(raw), xm.bits(raw2))


def test_a_query_launches_no_score_buffer_kernel(hip):
    U, I, K, L, R, S = 300, 997, 7, 9, 5, 2
    data, params = problem(U, I, R, K, L, S, 2000, seed=17)
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, np.arange(1.0, R + 1), True)
        with LaunchWindow() as lw:
            em.recommend_top_pairs(300)
            em.recommend_top_pairs(10, np.arange(5))
            em.recommend_end()
            em.close()                                     # (the log is written when the context goes)
            names = lw.names()
    finally:
        em.close()
    assert "gtop_fused_kernel" in names and "gtop_merge_kernel" in names, sorted(names)
    assert not [n for n in names if n.startswith(SCORE_BUFFER_KERNELS)], sorted(names)


def test_every_top_pairs_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("gtop_")]
    for k in ("gtop_fused_kernel", "gtop_merge_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
    assert len({k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("rec_select_kernel<")}) == 2
