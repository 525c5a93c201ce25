"""The serving kernels (recommend.hpp, fold_in.hpp and their launch code) on models whose scores carry no rounding
(exact_models.py), where whole blocks of items tie exactly -- what a fitted model looks like, and what the random,
all-distinct scores of test_gpu_recommend.py / test_gpu_ranking.py / test_gpu_fold_in*.py never produce.

Recommendation and positions are compared with the exact reference by EQUALITY: items, counts, positions, the padding
and the scores bit for bit (viewed as uint64).  No tolerance, no share of cases left out: one wrong member of a tie
group, a count off by one inside a tie group or a merge that drops a candidate equal to the threshold fails.  The
conditions that make the cases bite (a tie at every N boundary, a tie group across a range boundary, scores that
always / never pass the threshold filter) are asserted on the inputs in test_serving_exact_cpu.py.

Fold-in divides, so after the first iteration it is inexact; it is checked by what must hold exactly (zeros stay zero,
power-of-two dot products, bitwise equality of the two sides) and by the restatement at the tolerances of
test_gpu_fold_in.py, on inputs that grid lacks: rows of probability zero (the clamp 1 / max(dot, eps)), theta0 with
exact zeros, and every group-size border of fold_code with degrees on both sides of the on-chip border.
"""
import os
import sys

import numpy as np
import pytest

import exact_models as xm
from conftest import ROOT, assert_elementwise
from oracle import mmsbm_oracle as orc
from test_fold_in_cpu import log_likelihood, restate_fold
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)
from test_serving_exact_cpu import DEGREES, row_sum_bound

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

VARIANT_IDS = [f"{f}-{k}" for f, k in xm.VARIANTS]
WINDOW = {}


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


def open_session(em, n_slots, w, exclude):
    em.recommend_begin(w, exclude)
    for s in range(n_slots):
        em.select(s).recommend_add()


def same_answer(got, want, what):
    """(items, scores, counts) equal in every entry, the padding included, scores by their bits."""
    for g, w, nm in zip(got, want, ("items", "scores", "counts")):
        gb, wb = (xm.bits(g), xm.bits(w)) if nm == "scores" else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        if not np.array_equal(gb, wb):
            row = int(np.argwhere(gb != wb)[0][0])
            raise AssertionError(f"{what}: {nm} differ in {int((gb != wb).sum())} entries, first in row {row}: "
                                 f"device {np.asarray(g)[row]}, exact {np.asarray(w)[row]}")


def covered_split(hip, I, U):
    """The split this device's CU count chooses is one the CPU conditions were asserted for."""
    cus = hip._lib.device_identity(0)["compute_units"]
    assert xm.select_split(I, U, cus) in {xm.select_split(I, U, c) for c in xm.CU_COUNTS}, cus
    assert xm.position_split(I, U, cus) in {xm.position_split(I, U, c) for c in xm.CU_COUNTS}, cus


def check_session(em, case, exclude, ns, rng, what, lengths=None):
    """Every n of `ns` against the exact top-N, the positions of built test lists against the exact positions, and the
    cross-check that needs no reference: the item returned at rank k has position k + 1."""
    U, I = case["shape"][:2]
    users, scores = case["users"], case["scores"]
    seen = case["seen"] if exclude else None
    top = xm.exact_top_n(scores, users, max(ns), seen)
    for n in ns:
        same_answer(em.recommend_query(users, n), xm.first_n(top, n), f"{what} n={n}")
    off, items = xm.position_lists(rng, scores, seen, **({} if lengths is None else {"lengths": lengths}))
    pos, cand = em.recommend_positions(users, off, items)
    want_pos, want_cand = xm.exact_positions(scores, off, items, users.tolist(), seen)
    assert np.array_equal(cand, want_cand), what
    assert np.array_equal(pos, want_pos), (what, np.flatnonzero(pos != want_pos)[:5], pos[pos != want_pos][:5], want_pos[pos != want_pos][:5])
    got_items, _, counts = em.recommend_query(users, max(ns))
    back = np.concatenate([got_items[b, :counts[b]] for b in range(U)]).astype(np.int32)
    b_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    b_pos, b_cand = em.recommend_positions(users, b_off, back)
    assert np.array_equal(b_pos, np.concatenate([np.arange(1, c + 1) for c in counts])), what
    assert np.array_equal(np.minimum(b_cand, max(ns)), counts), what


def list_lengths(U):
    return {1: (200,), 3: (33, 200, 17)}.get(U)


# ---- recommend_query and recommend_positions ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.MANY + xm.SPLIT, ids=lambda s: "U{}I{}K{}L{}R{}S{}".format(*s))
@pytest.mark.parametrize("variant", xm.VARIANTS, ids=VARIANT_IDS)
def test_query_and_positions_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    covered_split(hip, I, U)
    case = xm.make_case(*variant, shape)
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            check_session(em, case, exclude, xm.NS, rng, f"{variant} {shape} exclude={exclude}", list_lengths(U))
            em.recommend_end()
    finally:
        em.close()


@pytest.mark.parametrize("family", ["interleaved", "ascending"])
def test_users_beyond_one_batch(hip, family):
    """300 users over 100,003 items: batches of 128, 128 and 44 users, each a score buffer of about 100 MB."""
    U, I, K, L, R, S = xm.BATCHES
    case = xm.make_case(family, "stars", xm.BATCHES, n_random=3000)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            seen = case["seen"] if exclude else None
            top = xm.exact_top_n(case["scores"], case["users"], 257, seen)
            for n in (10, 257):
                same_answer(em.recommend_query(case["users"], n), xm.first_n(top, n), f"{family} exclude={exclude} n={n}")
            off = np.arange(U + 1, dtype=np.int64) * 5                   # five test items per user, across the batches
            items = np.concatenate([top[0][b, [0, 1, 9, 100, 256]] if top[2][b] == 257 else np.array([0, 1, 2, I - 2, I - 1])
                                    for b in range(U)]).astype(np.int32)
            pos, cand = em.recommend_positions(case["users"], off, items)
            want_pos, want_cand = xm.exact_positions(case["scores"], off, items, case["users"].tolist(), seen)
            assert np.array_equal(pos, want_pos) and np.array_equal(cand, want_cand)
            em.recommend_end()
    finally:
        em.close()


# ---- caller theta rows and added items (the paths fold-in feeds) -------------------------------------------------------
@pytest.mark.parametrize("K,L", [(4, 6), (6, 4)], ids=["K4L6", "K6L4"])
@pytest.mark.parametrize("family", xm.BLOCK_FAMILIES)
def test_caller_theta_rows_and_added_items_are_exact(hip, family, K, L):
    U, I, R, S, n_new = 120, 1500, 5, 3, 40
    shape = (U, I, K, L, R, S)
    case = xm.make_case(family, "stars", shape)
    rng = np.random.default_rng(xm.case_seed(family, "stars", shape))
    params, w, users = case["params"], case["w"], case["users"]
    src = rng.integers(0, I, n_new)                          # added item j duplicates training item src[j]'s eta rows
    src[:3] = (0, I - 1, 17)
    new_eta = np.stack([params[s][1][src] for s in range(S)])
    seen_new = [rng.choice(U, rng.integers(0, 6)) for _ in range(n_new)]
    n_off = np.concatenate([[0], np.cumsum([len(x) for x in seen_new])]).astype(np.int64)
    ext = [(t, np.vstack([e, new_eta[s]]), p) for s, (t, e, p) in enumerate(params)]
    NI = I + n_new
    ext_scores = xm.exact_scores(ext, users, NI, w)
    sample = np.array([0, 1, 2, 3, 5, 77, 119])
    thetas = np.stack([params[s][0][sample] for s in range(S)])
    t_seen = [set(rng.choice(I, 30, replace=False).tolist()) | {I + 1} for _ in sample]
    t_lists = [np.array(sorted(x)) for x in t_seen]
    t_off = np.concatenate([[0], np.cumsum([len(x) for x in t_lists])]).astype(np.int64)
    em = context(hip, case["data"], params, U, I, R)
    try:
        for exclude in (True, False):
            what = f"{family} K={K} L={L} exclude={exclude}"
            open_session(em, S, w, exclude)
            rows = np.arange(len(sample))
            for n in (1, 10, 257, 1024):                     # caller rows against the training catalogue
                same_answer(em.recommend_query_theta(thetas, n),
                            xm.exact_top_n(case["scores"][sample], rows, n), f"{what} theta n={n}")
            em.recommend_add_items(new_eta, (n_off, np.concatenate(seen_new).astype(np.int32)))
            seen = [set(case["seen"][u]) if exclude else set() for u in range(U)]
            for j, us in enumerate(seen_new):
                for u in us.tolist():
                    seen[u].add(I + j)
            ext_case = dict(case, shape=(U, NI, K, L, R, S), scores=ext_scores, seen=seen)
            check_session(em, ext_case, True, (1, 10, 257, 1024), rng, f"{what} extended")
            for n in (10, 1024):                             # caller rows, own seen lists, extended catalogue
                same_answer(em.recommend_query_theta(thetas, n, (t_off, np.concatenate(t_lists).astype(np.int32))),
                            xm.exact_top_n(ext_scores[sample], rows, n, t_seen), f"{what} theta extended n={n}")
            full = em.recommend_query(users, 1024)
            for u in range(U):                               # the duplicate ties with its source and comes after it
                row = full[0][u, :full[2][u]].tolist()
                for j in range(3):
                    if src[j] in row and I + j in row:
                        assert row.index(src[j]) < row.index(I + j)
                        assert full[1][u, row.index(src[j])] == full[1][u, row.index(I + j)]
            em.recommend_end()
    finally:
        em.close()


# ---- swapped context, slot order -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(("sorted", "stars"), xm.MANY[0]), (("mixed", "signed"), xm.MANY[1]),
                                           (("interleaved", "indicator"), xm.SPLIT[1])],
                         ids=["sorted", "mixed-signed", "interleaved-split"])
def test_swapped_contexts_and_slot_order_are_bitwise_equal_and_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = xm.make_case(*variant, shape)
    seen = case["seen"]
    off, items = xm.position_lists(np.random.default_rng(2), case["scores"], seen, **({} if U > 3 else {"lengths": list_lengths(U)}))
    want = {n: xm.exact_top_n(case["scores"], case["users"], n, seen) for n in (10, 1024)}
    want_pos = xm.exact_positions(case["scores"], off, items, case["users"].tolist(), seen)
    answers = []
    for swap, params in ((0, case["params"]), (1, case["params"]), (0, case["params"][::-1]), (1, case["params"][::-1])):
        em = context(hip, case["data"], params, U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            open_session(em, S, case["w"], True)
            got = {n: em.recommend_query(case["users"], n) for n in (10, 1024)}
            pos = em.recommend_positions(case["users"], off, items)
            em.recommend_end()
        finally:
            em.close()
        for n in got:
            same_answer(got[n], want[n], f"{variant} swap={swap} n={n}")
        assert np.array_equal(pos[0], want_pos[0]) and np.array_equal(pos[1], want_pos[1])
        answers.append(got)
    for other in answers[1:]:
        for n in other:
            same_answer(other[n], answers[0][n], f"{variant} layouts n={n}")


# ---- fold_in and fold_in_items ------------------------------------------------------------------------------------
GPU_DEGREES = DEGREES[:-1] + [400, DEGREES[-1]]              # (K = 6: 400 rows take the streamed form)


def both_sides(hip, model_params, rows, U, I, R, calls):
    """calls: [(iterations, tol, start)] -> the results of fold_in, after asserting that fold_in_items of the
    transposed problem gives bitwise the same (test_gpu_fold_in_items.test_transposition_identity)."""
    n_new = int(rows[:, 0].max()) + 1
    data = np.stack([np.arange(U) % U, np.arange(U) % I, np.arange(U) % R], 1)
    em = context(hip, data, [model_params], U, I, R)
    try:
        users = [em.fold_in(rows, n_new, n, tol=tol, theta0=start) for n, tol, start in calls]
    finally:
        em.close()
    t_params, t_rows = xm.transposed(model_params, rows)
    tr = context(hip, np.ascontiguousarray(data[:, [1, 0, 2]]), [t_params], I, U, R)
    try:
        items = [tr.fold_in_items(t_rows, n_new, n, tol=tol, eta0=start) for n, tol, start in calls]
    finally:
        tr.close()
    for (a, ai), (b, bi) in zip(users, items):
        assert np.array_equal(xm.bits(a), xm.bits(b)) and np.array_equal(ai, bi)
    return users


def test_rows_of_probability_zero_meet_the_clamp(hip):
    """A rating value the model never produces, a user all of whose rows are impossible, and a theta0 whose support
    misses the rows' v: 1 / max(dot, eps) is reached with dot = 0.  The result is finite, the restatement's, and a
    user's memberships sum to (d - z) / d (z impossible rows), as the reference's do: it divides by d."""
    U, I, K, L, R = 30, 40, 6, 5, 4
    d = np.asarray(GPU_DEGREES)
    iters = (1, 2, 7, 100)
    rng = np.random.default_rng(5)
    params, rows, z = xm.impossible_rating_case(rng, U, I, K, L, R, GPU_DEGREES)
    got = both_sides(hip, params, rows, U, I, R, [(n, None, None) for n in iters])
    for n, (t, it) in zip(iters, got):
        assert np.isfinite(t).all() and (it == n).all()
        assert_elementwise(t, restate_fold(rows, len(d), params[1], params[2], n)[0], f"impossible rating, {n} iterations")
        assert (np.abs(t.sum(axis=1) - (d - z) / d) <= row_sum_bound(K, d)).all(), n
        assert (t[-1] == 0.0).all()
    params, rows, t0, z = xm.disjoint_support_case(rng, U, I, K, L, R, GPU_DEGREES)
    assert z.sum() > 0
    got = both_sides(hip, params, rows, U, I, R, [(n, None, t0) for n in iters])
    for n, (t, it) in zip(iters, got):
        assert np.isfinite(t).all()
        assert (t[t0 == 0.0] == 0.0).all(), n                 # exact zeros of theta0 stay exactly zero
        assert_elementwise(t, restate_fold(rows, len(d), params[1], params[2], n, theta0=t0)[0], f"disjoint support, {n} iterations")
        assert (np.abs(t.sum(axis=1) - (d - z) / d) <= row_sum_bound(K, d)).all(), n
    want = orc.normalize_with_d(orc.update_coefficients(rows, t0, params[1], params[2])[0], d)
    np.testing.assert_allclose(got[0][0], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("K", [4, 8, 16])
def test_one_iteration_with_power_of_two_dot_products_is_exact(hip, K):
    top = 1024 // K
    degrees = [1, 3, top, top + 1, 2 * top + 5, 2, 1]        # both forms
    params, rows, want = xm.power_of_two_case(np.random.default_rng(K), 20, 30, K, 3, degrees)
    (got, it), = both_sides(hip, params, rows, 20, 30, K, [(1, None, None)])
    assert np.array_equal(xm.bits(got), xm.bits(want)), np.abs(got - want).max()
    assert (it == 1).all()


@pytest.mark.parametrize("K", xm.FOLD_KS)
def test_group_size_borders(hip, K):
    """Both sides of every border of fold_code, each with degrees on both sides of d * K = 1024, short users sharing a
    wave's LDS budget and a partly empty last wave."""
    U, I, L, R = 20, 30, 3, 4
    rng = np.random.default_rng(K)
    params = (rng.random((U, K)), rng.random((I, L)), orc.normalize_with_self(rng.random((K, L, R))))
    degrees = xm.border_degrees(K)
    rows = xm.rows_with_degrees(rng, degrees, I, R)
    t0 = rng.random((len(degrees), K)) + 0.05
    (one, _), (hund, it) = both_sides(hip, params, rows, U, I, R, [(1, None, t0), (100, None, None)])
    d = np.asarray(degrees)
    want = orc.normalize_with_d(orc.update_coefficients(rows, t0, params[1], params[2])[0], d)
    np.testing.assert_allclose(one, want, rtol=1e-12, atol=0)
    assert_elementwise(hund, restate_fold(rows, len(d), params[1], params[2], 100)[0], f"K={K}, 100 iterations")
    assert (it == 100).all()


def test_more_groups_than_the_kernels_cover_are_refused_before_any_launch(hip):
    K, U, I, L, R = 1025, 5, 6, 2, 3
    rng = np.random.default_rng(1)
    params = (rng.random((U, K)), rng.random((I, L)), orc.normalize_with_self(rng.random((K, L, R))))
    data = np.stack([np.arange(U), np.arange(U), np.arange(U) % R], 1)
    rows = np.array([[0, 1, 2], [1, 0, 0]])
    with LaunchWindow() as lw:
        em = context(hip, data, [params], U, I, R)
        try:
            with pytest.raises(hip._lib.HipLibraryError, match="1024") as e:
                em.fold_in(rows, 2, 5)
            assert e.value.code == hip._lib.E_UNSUPPORTED
        finally:
            em.close()
        tr = context(hip, data[:, [1, 0, 2]], [xm.transposed(params, rows)[0]], I, U, R)
        try:
            with pytest.raises(hip._lib.HipLibraryError, match="1024") as e:
                tr.fold_in_items(rows[:, [1, 0, 2]], 2, 5)
            assert e.value.code == hip._lib.E_UNSUPPORTED
        finally:
            tr.close()
        assert not [n for n in lw.names() if n.startswith("fold_")]


def test_the_likelihood_never_decreases(hip):
    """sum_j log(theta_u . v_j) of every new user from n to n + 1 iterations, n = 1 .. 30.  The floor is rounding alone
    (exact_models.likelihood_floor); on the restatement the smallest of the first ten steps on these inputs is above
    1e-6 (test_serving_exact_cpu.py), ten orders of magnitude above it."""
    U, I, K, L, R = 30, 40, 6, 5, 4
    params, rows, _ = xm.impossible_rating_case(np.random.default_rng(8), U, I, K, L, R, GPU_DEGREES)
    rows = rows[rows[:, 2] != R - 1]
    n_new = len(GPU_DEGREES) - 1
    d = np.bincount(rows[:, 0], minlength=n_new)
    got = both_sides(hip, params, rows, U, I, R, [(n, None, None) for n in range(1, 32)])
    liks = [log_likelihood(rows, n_new, t, params[1], params[2]) for t, _ in got]
    for n in range(1, 31):
        step = liks[n] - liks[n - 1]
        assert (step >= -xm.likelihood_floor(K, d, liks[n])).all(), (n, step.min())


# ---- the launch log: these cases reach every serving kernel the library compiles ----------------------------------------
def test_every_serving_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith(("rec_", "fold_"))]
    assert len([k for k in compiled if k.startswith("fold_kernel<")]) == 18
    assert len([k for k in compiled if k.startswith("rec_select_kernel<")]) == 2
    for k in ("rec_w_kernel", "rec_fold_kernel", "rec_score_kernel", "rec_exclude_kernel", "rec_position_kernel",
              "rec_position_sum_kernel", "fold_v_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
