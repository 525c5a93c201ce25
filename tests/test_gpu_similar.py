"""Nearest items and users on the device (mmsbm_hip_similar_*, HipEM.similar_*, similar.hpp) against
test_similar_cpu.py: by EQUALITY with the exact reference on the models of exact_models.py (ids, counts, padding, and
distances by their bits: whole groups of rows tie at distance exactly 0), against the numpy restatement within a
tolerance derived from the operation counts on general models (returned ids equal, after asserting on the restatement
alone that no gap is near the tolerance), and the identities the kernels promise bit for bit.

MMSBM_E_TOOLARGE is the one refusal not provoked here: it needs a device without free memory.
"""
import os
import sys

import numpy as np
import pytest

import exact_models as xm
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)
from test_gpu_serving_exact import same_answer
from test_similar_cpu import SIDES, exact_distances, random_params, restate_distances, top_similar

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

VARIANT_IDS = [f"{f}-{k}" for f, k in xm.VARIANTS]
SHAPE_ID = lambda s: "U{}I{}K{}L{}R{}S{}".format(*s)  # noqa: E731
WINDOW = {}
MASS_BLOCK = 256                                          # sim_mass_kernel: threads that each add rows t, t + 256, ...


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


def ask(em, side, n_slots, ids, ns, slots=None):
    """{n: similar_query(ids, n)} of a session over `side` with slots 0 .. n_slots-1 (or `slots`) added."""
    em.similar_begin(side)
    try:
        for s in (range(n_slots) if slots is None else slots):
            em.select(s).similar_add()
        return {n: em.similar_query(ids, n) for n in ns}
    finally:
        em.similar_end()


def same_similar(got, want, what):
    """(ids, distance, counts) equal in every entry, the padding included, distances by their bits."""
    same_answer(got, want, what)


def first_n(top, n):
    out, dist, counts = top
    return out[:, :n], dist[:, :n], np.minimum(counts, n)


def exact_reference(params, side, ids, seed, chunk=64):
    """exact_distances of the query ids, after asserting that a permuted accumulation order gives the same bits (the
    model carries no rounding at this shape either)."""
    ids = np.asarray(ids, dtype=np.int64)
    theta, eta, p = params[0]
    n_terms = len(params) * (theta.shape[1] if side == "items" else eta.shape[1]) * p.shape[2]
    perm = np.random.default_rng(seed).permutation(n_terms)
    out = []
    for b in range(0, len(ids), chunk):
        d = exact_distances(params, side, ids[b:b + chunk])
        if b == 0:
            assert np.array_equal(xm.bits(d), xm.bits(exact_distances(params, side, ids[:chunk], perm)))
        out.append(d)
    return np.concatenate(out)


def n_rows(shape, side):
    return shape[1] if side == "items" else shape[0]


# ---- 1. exact, by equality ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("shape", xm.MANY, ids=SHAPE_ID)
@pytest.mark.parametrize("variant", xm.VARIANTS, ids=VARIANT_IDS)
def test_every_row_is_exact(hip, variant, shape, side):
    U, I, K, L, R, S = shape
    case = xm.make_case(*variant, shape)
    ids = np.arange(n_rows(shape, side), dtype=np.int32)
    top = top_similar(exact_reference(case["params"], side, ids, xm.case_seed(*variant, shape)), ids, max(xm.NS))
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        got = ask(em, side, S, ids, xm.NS)
    finally:
        em.close()
    for n in xm.NS:
        same_similar(got[n], first_n(top, n), f"{variant} {shape} {side} n={n}")


@pytest.mark.parametrize("n_ids", [1, 3])
@pytest.mark.parametrize("shape", [(3, 40000, 6, 4, 5, 3), (1, 9000, 4, 6, 5, 2)], ids=SHAPE_ID)
@pytest.mark.parametrize("family", xm.FAMILIES)
def test_few_rows_over_many_split_and_merged_are_exact(hip, family, shape, n_ids):
    U, I, K, L, R, S = shape
    assert shape in xm.SPLIT
    case = xm.make_case(family, "stars", shape)
    ids = np.array([I - 1, 0, I // 2][:n_ids], dtype=np.int32)
    cus = hip._lib.device_identity(0)["compute_units"]
    assert xm.select_split(I, n_ids, cus)[0] > 1, "the rows are split across waves and merged"
    top = top_similar(exact_reference(case["params"], "items", ids, xm.case_seed(family, "stars", shape)), ids, max(xm.NS))
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        got = ask(em, "items", S, ids, xm.NS)
    finally:
        em.close()
    for n in xm.NS:
        same_similar(got[n], first_n(top, n), f"{family} {shape} ids={ids.tolist()} n={n}")


@pytest.mark.parametrize("family", ["interleaved", "mixed"])
def test_query_rows_beyond_one_batch_are_exact(hip, family):
    """300 query items over 100,003: batches of 128, 128 and 44 rows, each a buffer of about 100 MB."""
    U, I, K, L, R, S = xm.BATCHES
    assert xm.batch_users(I, 300) == 128
    case = xm.make_case(family, "stars", xm.BATCHES, n_random=3000)
    rng = np.random.default_rng(xm.case_seed(family, "stars", xm.BATCHES))
    ids = rng.choice(I, 300, replace=False).astype(np.int32)
    ids[:2] = (I - 1, 0)
    top = top_similar(exact_reference(case["params"], "items", ids, 1), ids, 257)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        got = ask(em, "items", S, ids, (10, 257))
    finally:
        em.close()
    for n in (10, 257):
        same_similar(got[n], first_n(top, n), f"{family} n={n}")


# ---- 2. general models against the restatement ------------------------------------------------------------------------
def tolerance(D, G, R, rank, c_m):
    """2 x 2^-52 x (4 G sqrt(R D) + (rank + c_m + 8) D): the cancellation in q_i - q_j (each q carries <= G roundings
    of values <= 1, and sum m |d| / U <= sqrt(R D) by Cauchy-Schwarz), then the chain of `rank` terms and the mass
    reduction (c_m dependent additions); the factor 2 is the restatement's own rounding."""
    return 2.0 * 2.0 ** -52 * (4.0 * G * np.sqrt(R * D) + (rank + c_m + 8) * D)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("shape,seed", [((300, 997, 7, 9, 5, 3), 0), ((260, 1021, 9, 5, 4, 4), 1), ((2000, 3000, 20, 20, 5, 2), 2)],
                         ids=lambda v: SHAPE_ID(v) if isinstance(v, tuple) else f"seed{v}")
def test_general_models_agree_with_the_restatement(hip, shape, seed, side):
    U, I, K, L, R, S = shape
    n = 257
    rng = np.random.default_rng(seed)
    params = random_params(rng, U, I, K, L, R, S)
    data = np.stack([rng.integers(0, U, 4 * U), rng.integers(0, I, 4 * U), rng.integers(0, R, 4 * U)], 1)
    rows, others = (I, U) if side == "items" else (U, I)
    G, groups = (L, K) if side == "items" else (K, L)         # G: summed over in q; groups: the profile's
    c_m = -(-others // MASS_BLOCK) + 8                        # similar.hpp: ceil(rows / 256) + 8
    ids = np.arange(rows, dtype=np.int32)
    ref = restate_distances(params, side, ids)
    want_ids, want_d, want_c = top_similar(ref, ids, n + 1)
    assert (want_c == n + 1).all()
    tol = tolerance(want_d, G, R, S * groups * R, c_m)
    # the precondition, from the restatement alone: every gap between consecutive candidates at ranks 1 .. n + 1 is
    # wider than both tolerances, so the order is decided and the returned ids must be EQUAL
    gaps = np.diff(want_d, axis=1)
    print(f"{shape} {side}: smallest gap {gaps.min():.3e}, largest tolerance {tol.max():.3e}")
    assert (gaps > 2.0 * np.maximum(tol[:, :-1], tol[:, 1:])).all(), (gaps.min(), tol.max())
    em = context(hip, data, params, U, I, R)
    try:
        got_ids, got_d, got_c = ask(em, side, S, ids, (n,))[n]
        assert em.get_option("similar_ms") > 0
    finally:
        em.close()
    err = np.abs(got_d - want_d[:, :n])
    print(f"{shape} {side}: largest error / tolerance {np.max(err / tol[:, :n]):.3f}, largest error {err.max():.3e}")
    assert np.array_equal(got_c, np.full(rows, n))
    assert np.array_equal(got_ids, want_ids[:, :n])
    assert (err <= tol[:, :n]).all(), np.max(err / tol[:, :n])
    assert (got_d >= 0.0).all() and (np.diff(got_d, axis=1) >= 0.0).all()


# ---- 3. identities, bit for bit ---------------------------------------------------------------------------------------
def general_problem(U, I, K, L, R, S, seed):
    rng = np.random.default_rng(seed)
    params = random_params(rng, U, I, K, L, R, S)
    data = np.stack([rng.integers(0, U, 5 * U), rng.integers(0, I, 5 * U), rng.integers(0, R, 5 * U)], 1)
    return data, params


def test_users_are_items_of_the_transposed_problem(hip):
    U, I, K, L, R, S = 310, 530, 6, 9, 4, 2
    data, params = general_problem(U, I, K, L, R, S, seed=3)
    ns = (1, 10, 300)
    em = context(hip, data, params, U, I, R)
    try:
        users = ask(em, "users", S, np.arange(U), ns)
        items = ask(em, "items", S, np.arange(I), ns)
    finally:
        em.close()
    t_params = [xm.transposed(p, data)[0] for p in params]
    tr = context(hip, np.ascontiguousarray(data[:, [1, 0, 2]]), t_params, I, U, R)
    try:
        t_items = ask(tr, "items", S, np.arange(U), ns)
        t_users = ask(tr, "users", S, np.arange(I), ns)
    finally:
        tr.close()
    for n in ns:
        same_similar(users[n], t_items[n], f"users / transposed items n={n}")
        same_similar(items[n], t_users[n], f"items / transposed users n={n}")


@pytest.mark.parametrize("side", SIDES)
def test_swapped_contexts_are_bitwise_equal(hip, side):
    U, I, K, L, R, S = 300, 800, 12, 7, 5, 2
    data, params = general_problem(U, I, K, L, R, S, seed=11)
    ids = np.arange(n_rows((U, I), side))
    answers = []
    for swap in (0, 1):
        em = context(hip, data, params, U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            answers.append(ask(em, side, S, ids, (10, 257)))
        finally:
            em.close()
    for n in (10, 257):
        same_similar(answers[1][n], answers[0][n], f"{side} swap n={n}")


@pytest.mark.parametrize("side", SIDES)
def test_a_row_depends_on_its_id_only(hip, side):
    """A permuted, a subset and a repeated request; one row over many (the selection split and merged) and all rows."""
    U, I, K, L, R, S = 1021, 5000, 8, 8, 5, 2
    data, params = general_problem(U, I, K, L, R, S, seed=9)
    rows = n_rows((U, I), side)
    rng = np.random.default_rng(3)
    perm = rng.permutation(rows)
    sub = rng.choice(rows, 77, replace=False)
    rep = np.array([sub[5], 0, sub[5], rows - 1, sub[5]])
    em = context(hip, data, params, U, I, R)
    try:
        em.similar_begin(side)
        for s in range(S):
            em.select(s).similar_add()
        every = em.similar_query(np.arange(rows), 10)
        again = em.similar_query(np.arange(rows), 10)
        shuffled = em.similar_query(perm, 10)
        some = em.similar_query(sub, 10)
        one = em.similar_query([sub[5]], 10)
        repeated = em.similar_query(rep, 10)
        em.similar_end()
    finally:
        em.close()
    for pick, got, what in ((np.arange(rows), again, "again"), (perm, shuffled, "permuted"), (sub, some, "subset"),
                            (sub[5:6], one, "one"), (rep, repeated, "repeated")):
        same_similar(got, tuple(a[pick] for a in every), f"{side} {what}")


@pytest.mark.parametrize("side", SIDES)
def test_slots_beyond_those_added_do_not_matter(hip, side):
    U, I, K, L, R = 200, 300, 5, 6, 4
    data, params = general_problem(U, I, K, L, R, 3, seed=4)
    ids = np.arange(n_rows((U, I), side))
    one = context(hip, data, params[:1], U, I, R)
    try:
        alone = ask(one, side, 1, ids, (10,))
    finally:
        one.close()
    three = context(hip, data, params, U, I, R)
    try:
        among = ask(three, side, 3, ids, (10,), slots=[0])
        last = ask(three, side, 3, ids, (10,), slots=[2])
    finally:
        three.close()
    same_similar(among[10], alone[10], f"{side}: slot 0 of 3")
    other = context(hip, data, params[2:], U, I, R)
    try:
        same_similar(ask(other, side, 1, ids, (10,))[10], last[10], f"{side}: slot 2 of 3")
    finally:
        other.close()


@pytest.mark.parametrize("side", SIDES)
def test_resident_and_uploaded_parameters_are_bitwise_equal(hip, side):
    U, I, K, L, R, S = 300, 800, 12, 7, 5, 2
    data, params = general_problem(U, I, K, L, R, S, seed=12)
    ids = np.arange(n_rows((U, I), side))
    em = context(hip, data, params, U, I, R)
    try:
        em.iterate(3)                                      # resident slots, moved by the EM loop
        fitted = [em.select(s).get_params() for s in range(S)]
        resident = ask(em, side, S, ids, (25,))
    finally:
        em.close()
    other = context(hip, data, fitted, U, I, R)
    try:
        same_similar(ask(other, side, S, ids, (25,))[25], resident[25], side)
    finally:
        other.close()


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------
def test_no_side_effects(hip):
    U, I, K, L, R, S = 200, 300, 6, 5, 5, 3
    data, params = general_problem(U, I, K, L, R, S, seed=13)
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
        test = data[:500]
        em.recommend_begin(w, True)
        for s in range(S):
            em.select(s).recommend_add()
        rec = em.recommend_query(np.arange(U), 10)
        em.predict_begin(test, w)
        em.select(0).predict_add()
        for side in SIDES:                                 # similarity sessions inside an open predict and recommend session
            ask(em, side, S, np.arange(n_rows((U, I), side)), (10,))
            assert em.get_option("similar_ms") > 0
        em.select(1).predict_add()
        mat, raw = em.predict_finish()
        rec2 = em.recommend_query(np.arange(U), 10)
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
    same_answer(rec2, rec, "the open recommend session")
    assert np.array_equal(xm.bits(mat), xm.bits(mat2)) and np.array_equal(xm.bits(raw), xm.bits(raw2))


# ---- 5. the ABI's refusals ----------------------------------------------------------------------------------------------
def refused(hip, code, fn, *args):
    with pytest.raises(hip._lib.HipLibraryError) as e:
        fn(*args)
    assert e.value.code == code, (e.value.code, e.value.message)


def test_refusals_by_status_code(hip):
    U, I, K, L, R = 50, 60, 4, 3, 3
    data, params = general_problem(U, I, K, L, R, 1, seed=2)
    lib = hip._lib
    em = context(hip, data, params, U, I, R)
    try:
        for side in (2, -1):
            refused(hip, lib.E_INVALID, em.similar_begin, side)
        refused(hip, lib.E_INVALID, em.similar_add)                      # without begin
        refused(hip, lib.E_INVALID, em.similar_query, [0], 3)
        for side, rows in ((0, I), (1, U)):
            em.similar_begin(side)
            refused(hip, lib.E_INVALID, em.similar_query, [0], 3)        # before the first add
            em.similar_add()
            for bad in (-1, rows):
                refused(hip, lib.E_INVALID, em.similar_query, [0, bad], 3)
            for bad in (0, -2):
                refused(hip, lib.E_INVALID, em.similar_query, [0], bad)
            refused(hip, lib.E_UNSUPPORTED, em.similar_query, [0], 1025)
            assert em.similar_query([rows - 1], 1024)[2].tolist() == [rows - 1]
            for n in (rows - 1, rows, rows + 7):                         # n >= rows: every other row, padded
                out, dist, counts = em.similar_query([3, 0], n)
                assert counts.tolist() == [rows - 1] * 2
                assert (out[:, rows - 1:] == -1).all() and np.isposinf(dist[:, rows - 1:]).all()
                assert sorted(out[0, :rows - 1].tolist()) == [j for j in range(rows) if j != 3]
            assert em.similar_query([], 5)[0].shape == (0, 5)
            em.similar_begin(side)                                       # the next begin ends the session
            refused(hip, lib.E_INVALID, em.similar_query, [0], 3)
            em.similar_end()
            refused(hip, lib.E_INVALID, em.similar_add)
        em.similar_end()                                                 # ending twice is no error
    finally:
        em.close()
    fresh = hip.HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R)     # no parameters yet
    try:
        fresh.similar_begin(0)
        refused(hip, lib.E_INVALID, fresh.similar_add)
    finally:
        fresh.close()                                                    # (destroy ends the open session)


def test_a_side_with_one_row_has_no_neighbours(hip):
    U, I, K, L, R = 1, 40, 3, 4, 3
    data, params = general_problem(U, I, K, L, R, 2, seed=6)
    em = context(hip, data, params, U, I, R)
    try:
        out, dist, counts = ask(em, "users", 2, [0, 0], (5,))[5]
        assert counts.tolist() == [0, 0] and (out == -1).all() and np.isposinf(dist).all()
        assert ask(em, "items", 2, [7], (5,))[5][2].tolist() == [5]
    finally:
        em.close()


def test_identical_rows_are_at_distance_zero_and_in_id_order(hip):
    U, I, K, L, R, S = 40, 700, 6, 9, 4, 2
    data, params = general_problem(U, I, K, L, R, S, seed=5)
    for _, e, _ in params:
        e[[17, 300, 699]] = e[5]
    em = context(hip, data, params, U, I, R)
    try:
        out, dist, counts = ask(em, "items", S, np.arange(I), (I,))[I]
    finally:
        em.close()
    for i, twins in ((5, [17, 300, 699]), (300, [5, 17, 699])):
        assert out[i, :3].tolist() == twins and (xm.bits(dist[i, :3]) == 0).all()   # +0.0
    for b in range(I):
        if b in (5, 17, 300, 699):
            continue
        row = out[b].tolist()
        at = [row.index(i) for i in (5, 17, 300, 699)]
        assert at == list(range(at[0], at[0] + 4)), (b, at)
        assert len({dist[b, a] for a in at}) == 1


# ---- 6. coverage -----------------------------------------------------------------------------------------------------------
def test_every_similarity_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("sim_")]
    for k in ("sim_mass_kernel", "sim_profile_kernel", "sim_dist_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
    assert len({n for n in names if n.startswith("rec_select_kernel<")}) == 2, sorted(names)
