"""The overlap session on the device (mmsbm_hip_overlap_*, HipEM.overlap_*, overlap.hpp) against test_align_cpu.py: by
EQUALITY with the integer Gram matrix on models whose tables are multiples of 1/8 (every product and partial sum is
exact in any order), against the extended-precision restatement within the bound of a sum of non-negative terms on
general models, the identities the header promises bit for bit, planted relabellings recovered end to end, and the ABI's
refusals.

The shapes are the smallest at which the kernels can go wrong: rows around the 16-row LDS step, the 256-thread
workgroup and the slab length B (one slab, two, an odd number, a short last one), columns around the tile edge T (half
a tile, one column more, one tile and a column) and slot counts that put a slot's columns across two tiles."""
import os
import sys

import numpy as np
import pytest

import exact_models as xm
from conftest import ROOT
from mmsbm_amd import align
from test_align_cpu import (MARGIN, PLANTED, SIDES, assert_decided, planted_params, random_params, restate_overlap,
                            side_tables)
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)
from test_gpu_serving_exact import same_answer

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

B, T = 2048, 64                                           # overlap.hpp: kOvlSlab, kOvlTile
ROWS = (1, 2, 15, 16, 17, 255, 256, 257, B - 1, B, B + 1, 2 * B + 1, 5 * B + 3)
GROUPS_SLOTS = ((1, 1), (7, 3), (9, 4), (20, 8), (T // 2, 2), (T // 2 + 1, 2), (T + 1, 1))
WINDOW = {}


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


def ask(em, side, slots, queries=1):
    """The Gram matrix of a session over `side` with the slots `slots` added in that order (queries > 1: a list)."""
    em.overlap_begin(side)
    try:
        for s in slots:
            em.select(s).overlap_add()
        out = [em.overlap_query() for _ in range(queries)]
        return out[0] if queries == 1 else out
    finally:
        em.overlap_end()


def same_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(xm.bits(a), xm.bits(b)), (what, int((xm.bits(a) != xm.bits(b)).sum()))


def triples(U, I, R, n=None, seed=0):
    rng = np.random.default_rng(seed)
    n = max(U, I) if n is None else n
    return np.stack([np.arange(n) % U, np.arange(n) % I, rng.integers(0, R, n)], 1)


# ---- 1. exact, by equality ---------------------------------------------------------------------------------------------
def one_hot_blocks(rng, rows, G, R, S):
    """One-hot tables: row r of slot s sits in group (r + s) % G on the user side, (3 r + s) % G on the item side."""
    r = np.arange(rows)
    return [(np.eye(G)[(r + s) % G], np.eye(G)[(3 * r + s) % G], xm.dyadic_simplex(rng, (G, G, R), 16)) for s in range(S)]


def integer_gram(params, side):
    X = np.concatenate(side_tables(params, side), axis=1)
    X8 = np.rint(X * 8).astype(np.int64)
    assert np.array_equal(X8 / 8.0, X), "the tables are multiples of 1/8"
    return (X8.T @ X8) / 64.0                             # (integers below 2^53: exact)


@pytest.mark.parametrize("G,S", GROUPS_SLOTS, ids=lambda v: str(v))
def test_exact_models_equal_the_integer_gram_matrix(hip, G, S):
    R = 2
    for rows in ROWS:
        rng = np.random.default_rng(rows * 1000 + G)
        mixed, _ = xm.model("mixed", rng, rows, rows, G, G, R, S)
        em = hip.HipEM(triples(rows, rows, R), G, G, n_users=rows, n_items=rows, n_ratings=R, slots=S)
        try:
            for family, params in (("mixed", mixed), ("one-hot", one_hot_blocks(rng, rows, G, R, S))):
                for s, p in enumerate(params):
                    em.select(s).set_params(*p)
                for side in SIDES:
                    got = ask(em, side, range(S))
                    same_bits(got, integer_gram(params, side), f"{family} rows={rows} G={G} S={S} {side}")
        finally:
            em.close()


# ---- 2. general models against the restatement ------------------------------------------------------------------------
GENERAL = [(17, 256, 1, T + 1, 1), (257, 2 * B + 1, 7, 9, 3), (B - 1, 15, T // 2 + 1, T // 2, 2), (4 * B + 1, B, 9, 20, 4),
           (5 * B + 3, 255, 20, 7, 8)]                    # (U, I, K, L, S)


@pytest.mark.parametrize("shape", GENERAL, ids=lambda s: "U{}I{}K{}L{}S{}".format(*s))
def test_general_models_agree_with_the_restatement(hip, shape):
    """Every term is non-negative, so whatever the order of the n - 1 additions and n products rounded once each (fma:
    one rounding per row of a slab, then the tree over the slabs: never more than `rows` roundings on a path),
    |out - exact| <= (rows + 2) 2^-53 exact; the restatement's own error is rows 2^-64."""
    U, I, K, L, S = shape
    R = 3
    rng = np.random.default_rng(U + I)
    params = random_params(rng, U, I, K, L, R, S)
    em = context(hip, triples(U, I, R), params, U, I, R)
    try:
        for side, rows in (("users", U), ("items", I)):
            got = ask(em, side, range(S))
            assert em.get_option("overlap_ms") > 0
            want = restate_overlap(params, side)
            err = np.abs(got.astype(np.longdouble) - want)
            bound = (rows + 2) * np.longdouble(2.0) ** -53 * want
            ok = want > 0
            print(f"{shape} {side}: largest error / bound {float((err[ok] / bound[ok]).max()):.4f}")
            assert (err <= bound).all(), float((err[ok] / bound[ok]).max())
    finally:
        em.close()


# ---- 3. the contract, bit for bit ---------------------------------------------------------------------------------------
CONTRACT = (2 * B + 77, 300, 20, 33, 3, 4)                # U, I, K, L, R, S: three slabs; item columns across tiles


def contract_problem(seed=7):
    U, I, K, L, R, S = CONTRACT
    rng = np.random.default_rng(seed)
    return triples(U, I, R, 5 * U, seed), random_params(rng, U, I, K, L, R, S)


def groups_of(side):
    return CONTRACT[2] if side == "users" else CONTRACT[3]


@pytest.fixture(scope="module")
def whole(hip):
    """{side: the Gram matrix of all four slots}, computed once (the tests below leave it unchanged)."""
    U, I, K, L, R, S = CONTRACT
    data, params = contract_problem()
    em = context(hip, data, params, U, I, R)
    try:
        return {side: ask(em, side, range(S)) for side in SIDES}
    finally:
        em.close()


@pytest.mark.parametrize("side", SIDES)
def test_symmetric_repeatable_and_independent_of_the_other_slots(hip, whole, side):
    U, I, K, L, R, S = CONTRACT
    data, params = contract_problem()
    G = groups_of(side)
    full = whole[side]
    same_bits(full, np.ascontiguousarray(full.T), f"{side}: out == out.T")
    em = context(hip, data, params, U, I, R)
    try:
        first, second = ask(em, side, range(S), queries=2)
        same_bits(first, full, f"{side}: another context")
        same_bits(second, first, f"{side}: two queries in a row")
        for s in range(S):                                 # the slot alone: its columns start a tile of their own
            same_bits(ask(em, side, [s]), align.block(full, G, s, s), f"{side}: slot {s} alone")
        pair = ask(em, side, [3, 1])                       # two slots in another order: other tiles, other neighbours
        same_bits(align.block(pair, G, 0, 1), align.block(full, G, 3, 1), f"{side}: block (3, 1)")
        same_bits(align.block(pair, G, 1, 1), align.block(full, G, 1, 1), f"{side}: block (1, 1)")
        twice = ask(em, side, [2, 2])                      # a slot may join twice
        for a in range(2):
            for b in range(2):
                same_bits(align.block(twice, G, a, b), align.block(full, G, 2, 2), f"{side}: slot 2 twice")
    finally:
        em.close()


@pytest.mark.parametrize("side", SIDES)
def test_swapped_contexts_are_bitwise_equal(hip, whole, side):
    U, I, K, L, R, S = CONTRACT
    data, params = contract_problem()
    for swap in (0, 1):
        em = context(hip, data, params, U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            same_bits(ask(em, side, range(S)), whole[side], f"{side} swap={swap}")
        finally:
            em.close()


def test_resident_and_uploaded_parameters_are_bitwise_equal(hip):
    U, I, K, L, R, S = 700, 300, 7, 9, 4, 3
    rng = np.random.default_rng(12)
    data, params = triples(U, I, R, 5 * U, 12), random_params(rng, U, I, K, L, R, S, alpha=1.0)
    em = context(hip, data, params, U, I, R)
    try:
        em.iterate(3)                                      # resident slots, moved by the EM loop
        fitted = [em.select(s).get_params() for s in range(S)]
        resident = {side: ask(em, side, range(S)) for side in SIDES}
    finally:
        em.close()
    other = context(hip, data, fitted, U, I, R)
    try:
        for side in SIDES:
            same_bits(ask(other, side, range(S)), resident[side], side)
    finally:
        other.close()


@pytest.mark.parametrize("side", SIDES)
def test_slots_beyond_those_added_do_not_matter(hip, whole, side):
    U, I, K, L, R, S = CONTRACT
    data, params = contract_problem()
    G = groups_of(side)
    one = context(hip, data, params[2:3], U, I, R)         # a context that holds slot 2 and nothing else
    try:
        same_bits(ask(one, side, [0]), align.block(whole[side], G, 2, 2), f"{side}: a one-slot context")
    finally:
        one.close()
    em = context(hip, data, params, U, I, R)
    try:
        em.overlap_begin(side)
        em.select(0).overlap_add()
        em.select(1).overlap_add()
        before = em.overlap_query()
        em.set_slots(1)                                    # the session keeps its tables
        em.select(0).set_params(*params[3])
        same_bits(em.overlap_query(), before, f"{side}: after set_slots")
        em.overlap_add()
        after = em.overlap_query()
        em.overlap_end()
    finally:
        em.close()
    same_bits(before, whole[side][:2 * G, :2 * G], f"{side}: slots 0 and 1 of 4")
    same_bits(align.block(after, G, 2, 2), align.block(whole[side], G, 3, 3), f"{side}: a slot added after set_slots")
    same_bits(align.block(after, G, 0, 2), align.block(whole[side], G, 0, 3), f"{side}: ... against an earlier one")


def test_no_side_effects(hip):
    U, I, K, L, R, S = 200, 300, 6, 5, 5, 3
    rng = np.random.default_rng(13)
    data, params = triples(U, I, R, 5 * U, 13), random_params(rng, U, I, K, L, R, S, alpha=1.0)
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
        held = data[:500]
        em.recommend_begin(w, True)
        em.similar_begin("items")
        em.heldout_begin(held)
        for s in range(S):
            em.select(s).recommend_add()
            em.select(s).similar_add()
        rec = em.recommend_query(np.arange(U), 10)
        sim = em.similar_query(np.arange(I), 10)
        ll = em.heldout_eval()
        first = em.select(0).heldout_add()
        grams = {side: ask(em, side, range(S)) for side in SIDES}     # inside the three open sessions
        for s in range(1, S):
            em.select(s).heldout_add()
        mean = em.heldout_mean()
        same_answer(em.recommend_query(np.arange(U), 10), rec, "the open recommend session")
        same_answer(em.similar_query(np.arange(I), 10), sim, "the open similar session")
        same_bits(em.heldout_eval(), ll, "the open held-out session")
        em.recommend_end()
        em.similar_end()
        em.heldout_end()
        after = [em.select(s).get_params() for s in range(S)]
        em.heldout_begin(held)                             # the same adds without an overlap session in between
        assert em.select(0).heldout_add() == first
        for s in range(1, S):
            em.select(s).heldout_add()
        mean2 = em.heldout_mean()
        em.heldout_end()
    finally:
        em.close()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            same_bits(a, b, "the EM parameters")
    same_bits(mean[0], mean2[0], "the held-out session's running sum")
    assert mean[1] == mean2[1]
    for side in SIDES:
        want = restate_overlap(params, side)
        assert np.allclose(grams[side], np.asarray(want, dtype=np.float64), rtol=1e-12, atol=0)


# ---- 4. end to end: planted relabellings ------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("rows,G,seed", PLANTED)
def test_planted_relabellings_are_recovered_through_the_device(hip, rows, G, seed, side):
    params, pi = planted_params(rows, G, seed, side)
    tabs = [t.astype(np.longdouble) for t in side_tables(params, side)]
    for t, name in ((1, "copy"), (2, "noisy")):            # the precondition, from the restatement alone
        assert_decided(tabs[0].T @ tabs[t], rows, f"{side} rows={rows} G={G} {name}")
    U, I = (rows, 3) if side == "users" else (3, rows)
    em = context(hip, triples(U, I, 2), params, U, I, 2)
    try:
        O = ask(em, side, range(3))
    finally:
        em.close()
    for t in (1, 2):
        assert np.array_equal(align.best_assignment(align.block(O, G, 0, t)), np.argsort(pi)), (side, t)
    assert (align.group_cosine(O, G, 0, 1, np.argsort(pi)) > 1 - 1e-12).all()
    assert MARGIN * rows > 256 * 2.0 ** -53 * rows         # the margin is far above the device's rounding


def test_align_restarts_through_the_model(hip):
    """MMSBM.align_restarts() / consensus() on fitted restarts: every row of the answer is the optimum of the device's
    own Gram block (brute force: K = 3, L = 4), and the resident slots are left as they are."""
    import itertools
    rng = np.random.default_rng(4)
    U, I, R, K, L, S = 150, 90, 4, 3, 4, 3
    train = np.stack([rng.integers(0, U, 3000), rng.integers(0, I, 3000), rng.integers(0, R, 3000)], 1)
    train[:U, 0], train[:I, 1], train[:R, 2] = np.arange(U), np.arange(I), np.arange(R)
    m = hip.MMSBM(K, L, iterations=20, sampling=S, seed=3)
    m.fit_encoded(train)
    params = [(r["theta"], r["eta"], r["pr"]) for r in m.results]
    out = m.align_restarts()
    ref = out["reference"]
    assert ref == int(np.argmax([r["likelihood"] for r in m.results]))
    for side, G, rows in (("user", K, U), ("item", L, I)):
        want = np.asarray(restate_overlap(params, side + "s"), dtype=np.float64)
        for s in range(S):
            blk = align.block(want, G, ref, s)
            best = max(sum(blk[k, p[k]] for k in range(G)) for p in itertools.permutations(range(G)))
            got = blk[np.arange(G), out[side + "_groups"][s]].sum()
            assert abs(got - best) <= 1e-9 * rows, (side, s)
        assert np.array_equal(out[side + "_agreement"], out[side + "_agreement"].T)
        assert (out[side + "_similarity"][ref] == 1.0).all()
    cons = m.consensus(reference=0)
    assert np.abs(cons["theta"].to_numpy().sum(axis=1) - 1).max() < 1e-12 and cons["eta"].shape == (I, L)
    assert np.array_equal(m.results[0]["theta"], params[0][0])


# ---- 5. the ABI's refusals ----------------------------------------------------------------------------------------------
def refused(hip, code, fn, *args):
    with pytest.raises(hip._lib.HipLibraryError) as e:
        fn(*args)
    assert e.value.code == code, (e.value.code, e.value.message)


def test_refusals_by_status_code(hip):
    U, I, K, L, R = 50, 60, 4, 3, 3
    rng = np.random.default_rng(2)
    data, params = triples(U, I, R), random_params(rng, U, I, K, L, R, 1)
    lib = hip._lib
    em = context(hip, data, params, U, I, R)
    try:
        for side in (2, -1):
            refused(hip, lib.E_INVALID, em.overlap_begin, side)                       # side not 0 / 1
        refused(hip, lib.E_INVALID, em.overlap_add)                                   # add without begin
        refused(hip, lib.E_INVALID, lib.call, "mmsbm_hip_overlap_query", em._h, np.zeros(K * K).ctypes.data_as(lib.c_f64p))
        for side, G in ((0, L), (1, K)):
            em.overlap_begin(side)
            refused(hip, lib.E_INVALID, lib.call, "mmsbm_hip_overlap_query", em._h,   # query before the first add
                    np.zeros(G * G).ctypes.data_as(lib.c_f64p))
            em.overlap_add()
            refused(hip, lib.E_INVALID, lib.call, "mmsbm_hip_overlap_query", em._h, None)   # out == NULL
            assert em.overlap_query().shape == (G, G)
            em.overlap_begin(side)                                                    # the next begin ends the session
            refused(hip, lib.E_INVALID, lib.call, "mmsbm_hip_overlap_query", em._h, np.zeros(G * G).ctypes.data_as(lib.c_f64p))
            em.overlap_end()
            refused(hip, lib.E_INVALID, em.overlap_add)
        em.overlap_end()                                                              # ending twice is no error
    finally:
        em.close()
    fresh = hip.HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R)                  # a slot without parameters
    try:
        fresh.overlap_begin(0)
        refused(hip, lib.E_INVALID, fresh.overlap_add)
    finally:
        fresh.close()                                                                 # (destroy ends the open session)


def test_a_result_beyond_the_device_memory_is_refused(hip):
    """2,200 adds of a one-row table of 129 groups: the F x F result alone, F = 283,800, is 644 GB -- more than the
    device has, let alone free -- and the partial tiles as much again.  Refused before anything is allocated."""
    G, S = 129, 2200
    lib = hip._lib
    assert (G * S) ** 2 * 8 > 600e9
    rng = np.random.default_rng(1)
    params = random_params(rng, 1, 1, G, 1, 2, 1)
    em = context(hip, triples(1, 1, 2), params, 1, 1, 2)
    try:
        em.overlap_begin("users")
        for _ in range(S):
            em.overlap_add()
        refused(hip, lib.E_TOOLARGE, lib.call, "mmsbm_hip_overlap_query", em._h, np.zeros(1).ctypes.data_as(lib.c_f64p))
        em.overlap_begin("users")                                                     # the context is as usable as before
        em.overlap_add()
        same_bits(em.overlap_query(), np.outer(params[0][0][0], params[0][0][0]), "one row: a single product each")
        em.overlap_end()
    finally:
        em.close()


# ---- 6. coverage -----------------------------------------------------------------------------------------------------------
def test_every_overlap_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("ovl_")]
    for k in ("ovl_gram_kernel", "ovl_combine_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
    assert "rec_fold_kernel" in names, sorted(names)       # the copy of a slot's rows
