"""The generators of exact_models.py under test, without a GPU: the exact reference against rational arithmetic, and
the CONDITIONS the cases of test_gpu_serving_exact.py rely on, asserted from the exact reference alone -- a tie at every
N boundary, a tie group across a range boundary in the split cases, scores that pass (or never pass) the selection's
threshold filter, the edge users' candidate counts, and the fold-in invariants on the CPU restatement.  These are
conditions on the inputs, not measurements: a generator change that breaks one fails here, instead of quietly
weakening the GPU test."""
from fractions import Fraction

import numpy as np
import pytest

import exact_models as xm
from oracle import mmsbm_oracle as orc
from test_fold_in_cpu import log_likelihood, restate_fold
from test_fold_in_items_cpu import restate_fold_items
from test_ranking_cpu import brute_positions
from test_recommend_cpu import restate_scores

VARIANT_IDS = [f"{f}-{k}" for f, k in xm.VARIANTS]


def fraction_score(params, u, i, w):
    num = Fraction(0)
    for theta, eta, p in params:
        K, L, R = p.shape
        for k in range(K):
            if theta[u, k] == 0.0:
                continue
            for l in range(L):
                if eta[i, l] == 0.0:
                    continue
                num += Fraction(theta[u, k]) * Fraction(eta[i, l]) * sum(Fraction(w[r]) * Fraction(p[k, l, r]) for r in range(R))
    return num / len(params)


# ---- the generators and the exact reference ---------------------------------------------------------------------------
def test_dyadic_simplex_rows():
    rng = np.random.default_rng(0)
    for shape, den in (((50, 7), 8), ((4, 6, 5), 16), ((3,), 16)):
        a = xm.dyadic_simplex(rng, shape, den)
        assert a.shape == shape and (a >= 0).all()
        assert np.array_equal(a * den, np.round(a * den)) and (a.sum(axis=-1) == 1.0).all()
    assert (xm.dyadic_simplex(rng, (200, 7), 8) == 0).mean() > 0.2          # zeros are common


@pytest.mark.parametrize("variant", xm.VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("K,L", [(4, 6), (7, 3)])
def test_exact_scores_equal_rational_arithmetic(variant, S, K, L):
    family, kind = variant
    U, I, R = 9, 70, 5
    rng = np.random.default_rng([S, K, L])
    params, w = xm.model(family, rng, U, I, K, L, R, S, kind)
    for theta, eta, p in params:                           # what the exactness argument assumes
        assert np.array_equal(p * xm.P_DEN, np.round(p * xm.P_DEN)) and np.array_equal(theta * 8, np.round(theta * 8))
        assert (p.sum(axis=2) == 1.0).all() and (theta.sum(axis=1) == 1.0).all() and (eta.sum(axis=1) == 1.0).all()
    assert np.array_equal(w, np.round(w))
    s = xm.exact_scores(params, np.arange(U), I, w)
    assert not np.signbit(s[s == 0.0]).any()               # a zero score is +0.0, as on the device
    for u, i in zip(rng.integers(0, U, 40).tolist(), rng.integers(0, I, 40).tolist()):
        assert Fraction(s[u, i]) == Fraction(float(fraction_score(params, u, i, w))), (u, i)
        if S in (1, 2, 4):
            assert fraction_score(params, u, i, w) == Fraction(s[u, i])      # not even the division rounds
    if S in (1, 2, 4):
        assert np.array_equal(xm.bits(s), xm.bits(restate_scores(params, np.arange(U), I, w) + 0.0))


def test_the_numerator_first_form_is_needed_at_three_slots():
    """restate_scores divides each probability by 3 before it weights them: not the device's bits."""
    rng = np.random.default_rng(3)
    params, w = xm.model("mixed", rng, 9, 70, 4, 6, 5, 3)
    s, r = xm.exact_scores(params, np.arange(9), 70, w), restate_scores(params, np.arange(9), 70, w)
    assert (xm.bits(s) != xm.bits(r)).any() and np.abs(s - r).max() < 1e-15


def test_launch_shapes_restated():
    assert xm.batch_users(100_003, 300) == 128 and xm.batch_users(997, 300) == 300 and xm.batch_users(20_000_000, 5) == 1
    assert xm.select_split(5000, 1, 256) == (5, 1000) and xm.select_split(40000, 3, 256) == (40, 1000)
    assert xm.select_split(997, 300, 256) == (1, 997) and xm.select_split(1021, 260, 256) == (1, 1021)
    assert xm.position_split(9000, 1, 256) == (5, 1800) and xm.position_split(40000, 1, 256) == (20, 2000)
    assert 256 in xm.CU_COUNTS
    U, I = xm.BATCHES[:2]
    assert xm.batch_users(I, U) < U and U % xm.batch_users(I, U) != 0 and xm.batch_users(I, U) * I * 8 <= 128 << 20


# ---- the conditions of the GPU cases ---------------------------------------------------------------------------------
def rows_cands(case, exclude):
    I = case["shape"][1]
    return [xm.candidates(I, case["seen"][u] if exclude else None) for u in range(case["shape"][0])]


@pytest.mark.parametrize("variant", [v for v in xm.VARIANTS if v[0] in xm.TIE_FAMILIES],
                         ids=[i for i, v in zip(VARIANT_IDS, xm.VARIANTS) if v[0] in xm.TIE_FAMILIES])
@pytest.mark.parametrize("shape", xm.MANY + xm.SPLIT, ids=str)
def test_candidates_n_and_n_plus_one_tie(variant, shape):
    case = xm.make_case(*variant, shape)
    for exclude in (True, False):
        cands = rows_cands(case, exclude)
        for n in xm.NS:
            if max(len(c) for c in cands) <= n:
                continue
            assert any(xm.ties_at(case["scores"][u], c, n) for u, c in enumerate(cands)), (exclude, n)


@pytest.mark.parametrize("variant", [v for v in xm.VARIANTS if v[0] in xm.TIE_FAMILIES],
                         ids=[i for i, v in zip(VARIANT_IDS, xm.VARIANTS) if v[0] in xm.TIE_FAMILIES])
@pytest.mark.parametrize("shape", xm.SPLIT, ids=str)
def test_a_tie_group_lies_across_a_range_boundary(variant, shape):
    """For every split the launch code can choose at this size: the tie group of the N-th candidate holds item ids on
    both sides of a boundary between two item ranges, for some checked (row, N); in the interleaved and the constant
    arrangement for every N that leaves candidates out."""
    U, I = shape[:2]
    case = xm.make_case(*variant, shape)
    splits = {xm.select_split(I, U, cus) for cus in xm.CU_COUNTS}
    assert all(parts > 1 for parts, _ in splits)
    for parts, per in splits:
        for exclude in (True, False):
            hits = {n: any(xm.threshold_group_spans(case["scores"][u], c, n, per) for u, c in enumerate(rows_cands(case, exclude)))
                    for n in xm.NS}
            assert any(hits.values()), (per, exclude)
            if variant[0] in ("interleaved", "constant"):
                assert all(hits.values()), (per, exclude, hits)


@pytest.mark.parametrize("shape", xm.MANY + xm.SPLIT, ids=str)
def test_strictly_monotone_families(shape):
    """Ascending: every item beats all items before it, so each passes the threshold filter when it is visited (64 of
    64 lanes every round, a re-sort at every fill).  Descending: no item after the first N beats the threshold."""
    up = xm.make_case("ascending", "stars", shape)["scores"]
    down = xm.make_case("descending", "stars", shape)["scores"]
    assert (np.diff(up, axis=1) > 0).all() and (np.diff(down, axis=1) < 0).all()


@pytest.mark.parametrize("shape", xm.MANY + [xm.SPLIT[1], xm.SPLIT[4]], ids=str)
def test_edge_users(shape):
    U, I = shape[:2]
    case = xm.make_case("rare", "stars", shape)
    by_role = {r: u for u, r in case["roles"].items()}
    if "all" in by_role:
        assert len(case["seen"][by_role["all"]]) == I
    left = xm.candidates(I, case["seen"][by_role["all_but"]])
    per = xm.select_split(I, U, xm.GEN_CUS)[1]
    assert len(left) == xm.LEFT < 10 and (per >= I or left.min() >= per)        # range 0 wholly seen
    s = case["scores"][by_role["best"]]
    assert case["seen"][by_role["best"]] == set(np.flatnonzero(s == s.max()).tolist())
    assert 0 < len(case["seen"][by_role["best"]]) <= xm.N_RARE
    assert not case["seen"][by_role["none"]]


def test_position_lists_hold_what_they_promise():
    case = xm.make_case("rare", "stars", xm.MANY[0])
    off, items = xm.position_lists(np.random.default_rng(1), case["scores"], case["seen"])
    lens = np.diff(off)
    assert set(lens.tolist()) == {0, 1, 4, 5, 16, 17, 33, 200}
    for b in np.flatnonzero(lens >= 33).tolist():
        mine = items[off[b]:off[b + 1]]
        assert mine[0] == 0 and mine[1] == case["shape"][1] - 1 and (mine[3] == mine[0] or mine[2] == mine[0])
        if case["seen"][b]:
            assert mine[2] in case["seen"][b]
        if b % 2:                                           # every member of the best level
            s = case["scores"][b]
            assert set(np.flatnonzero(s == s.max()).tolist()) <= set(mine.tolist())
    sub = np.arange(8)
    got = xm.exact_positions(case["scores"][sub], off[:9], items[:off[8]], sub.tolist(), case["seen"])
    want = brute_positions(case["scores"][sub], off[:9], items[:off[8]].tolist(), sub.tolist(), case["seen"])
    assert got[0].tolist() == want[0] and got[1].tolist() == want[1]


# ---- the fold-in invariants hold for the restatement (so a GPU failure is the kernel's) -------------------------------
DEGREES = [1, 2, 3, 7, 12, 40, 90, 6]


def row_sum_bound(K, d):
    """|row sum - (d - z) / d| <= this: per possible row sum_k q_k / dot = 1 within the rounding of K products, the
    K - 1 additions of dot, one reciprocal and K fmas; then d additions and one division (u = 2^-53)."""
    return (2 * K + d + 8) * 2.0 ** -53


def test_rows_of_probability_zero():
    rng = np.random.default_rng(5)
    (theta, eta, p), rows, z = xm.impossible_rating_case(rng, 30, 40, 6, 5, 4, DEGREES)
    d = np.asarray(DEGREES)
    assert z[-1] == d[-1] and (z[:-1] < d[:-1]).all() and z.sum() > z[-1]
    for n in (1, 2, 7, 100):
        t, _ = restate_fold(rows, len(d), eta, p, n)
        assert np.isfinite(t).all()
        assert (np.abs(t.sum(axis=1) - (d - z) / d) <= row_sum_bound(6, d)).all(), n
        assert (t[-1] == 0.0).all()
    (theta, eta, p), rows, t0, z = xm.disjoint_support_case(rng, 30, 40, 6, 5, 4, DEGREES)
    assert z[0::2].sum() > 0 and (z[1::2] == 0).all()
    for n in (1, 2, 7, 100):
        t, _ = restate_fold(rows, len(d), eta, p, n, theta0=t0)
        assert np.isfinite(t).all() and (t[t0 == 0.0] == 0.0).all()
        assert (np.abs(t.sum(axis=1) - (d - z) / d) <= row_sum_bound(6, d)).all(), n
    # the item side, by transposition
    (tt, te, tp), trows = xm.transposed((theta, eta, p), rows)
    e, _ = restate_fold_items(trows, len(d), tt, tp, 7, eta0=t0)
    assert np.array_equal(e, restate_fold(rows, len(d), eta, p, 7, theta0=t0)[0])


@pytest.mark.parametrize("K", [4, 8, 16])
def test_power_of_two_dot_products_are_exact(K):
    top = 1024 // K
    degrees = [1, 3, top, top + 1, 2 * top + 5]
    (theta, eta, p), rows, want = xm.power_of_two_case(np.random.default_rng(K), 20, 30, K, 3, degrees)
    assert (p.sum(axis=2) == 1.0).all() and (p.sum(axis=0) == 1.0).all()
    got, _ = restate_fold(rows, len(degrees), eta, p, 1)
    assert np.array_equal(xm.bits(got), xm.bits(want))
    ref = orc.normalize_with_d(orc.update_coefficients(rows, np.full((len(degrees), K), 1.0 / K), eta, p)[0], np.asarray(degrees))
    np.testing.assert_allclose(want, ref, rtol=1e-14)


def test_border_degrees_reach_both_forms_and_share_a_wave():
    for K in xm.FOLD_KS:
        deg = xm.border_degrees(K)
        G = xm.fold_lanes(K)
        gpw = 64 // G
        on = [d for d in deg if d * K <= 1024]
        assert any(d * K > 1024 for d in deg) and 1024 // K in on and 1024 // K + 1 in deg
        waves = xm.fold_waves(deg, K)
        assert sum(len(w) for w in waves) == len(on)
        if gpw > 1:
            assert len(waves[-1]) < gpw and any(len(w) > 1 for w in waves), K     # a partly empty wave; users sharing LDS
        if gpw >= 16:
            assert any(len(w) < gpw for w in waves[:-1]), K                       # a wave closed by its LDS budget
    assert [xm.fold_lanes(K) for K in (4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 1024)] == [1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 64]


def test_the_likelihood_never_decreases_on_these_inputs():
    rng = np.random.default_rng(8)
    (theta, eta, p), rows, z = xm.impossible_rating_case(rng, 30, 40, 6, 5, 4, DEGREES)
    rows = rows[rows[:, 2] != 3]                           # the possible rows: a finite likelihood
    n_new = len(DEGREES) - 1
    d = np.bincount(rows[:, 0], minlength=n_new)
    prev, steps = None, []
    for n in range(1, 32):
        t, _ = restate_fold(rows, n_new, eta, p, n)
        lik = log_likelihood(rows, n_new, t, eta, p)
        if prev is not None:
            steps.append(lik - prev)
            assert (lik - prev >= -xm.likelihood_floor(6, d, lik)).all(), n
        prev = lik
    assert np.min(steps[:10]) > 1e-6                       # (far above the floor while the iteration still moves)
