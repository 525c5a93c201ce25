"""Randomised top-N with logged propensities on the device (explore.hpp: mmsbm_hip_recommend_query_explore,
_recommend_list_propensity, _explore_noise; MMSBM.recommend_explore, propensities) against the numpy restatement of the
definition (explore_reference.py, pinned in test_explore_cpu.py) on models whose scores carry no rounding
(exact_models.py).

With a temperature that is a power of two the keys are exact given the noise, and the noise is a public function of
(seed, user, item): the reference takes g from explore_noise, so the lists, the counts and the score bits compare by
EQUALITY.  Only the propensities carry a tolerance: 1e-11 relative, above (I + 1,000) ulps for every catalogue used here,
which covers any summation order of positive terms and the exp of an argument up to 700.
"""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import exact_models as xm
import explore_reference as er
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)
from test_gpu_shelves import own_lists

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

SPLIT = (3, 5000, 4, 6, 5, 2)                                 # the selection of 5,000 columns is split across waves
assert SPLIT in xm.SPLIT
SHAPES = list(xm.MANY) + [SPLIT]
VARIANTS = [("mixed", "stars"), ("constant", "stars")]        # constant: every score ties, the order is the noise alone
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]
TEMPERATURES = (0.25, 1.0, 4.0)
NS = (1, 10, 257)
RTOL = 1e-11
SEED = 20
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


def words(hip, seed):
    from mmsbm_amd.core import pcg64_words
    return pcg64_words(np.random.default_rng(seed).bit_generator)


def open_session(em, n_slots, w, exclude):
    em.recommend_begin(w, exclude)
    for s in range(n_slots):
        em.select(s).recommend_add()


def noise_of(hip, em, seed, users, I):
    """g (len(users), I) of the device for every pair of the users and the catalogue."""
    uu = np.repeat(np.asarray(users, dtype=np.int32), I)
    ii = np.tile(np.arange(I, dtype=np.int32), len(users))
    g = em.explore_noise(words(hip, seed), uu, ii)[1].reshape(len(users), I)
    g.setflags(write=False)
    return g


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def close(got, want):
    return np.allclose(got, want, rtol=RTOL, atol=0.0)


def same_answer(got, want, what, n=None):
    """items and counts equal, scores by their bits, propensity within RTOL; the padding -1 / -inf / 0 included."""
    gi, gs, gp, gc = got
    wi, ws, wp, wc = want if n is None else (want[0][:, :n], want[1][:, :n], want[2][:, :n], np.minimum(want[3], n))
    assert gi.shape == wi.shape and gp.shape == wp.shape, (what, gi.shape, wi.shape)
    assert np.array_equal(gc, wc), (what, "counts")
    if not np.array_equal(gi, wi):
        row = int(np.argwhere(gi != wi)[0][0])
        raise AssertionError(f"{what}: items differ in {int((gi != wi).sum())} entries, first in row {row}: "
                             f"device {gi[row][:12]}, reference {wi[row][:12]}")
    assert np.array_equal(xm.bits(gs), xm.bits(ws)), (what, "scores")
    assert close(gp, wp), (what, "propensity", float(np.max(np.abs(gp - wp) / np.maximum(wp, 1e-300))))
    assert (gp[gi < 0] == 0).all() and (gp[gi >= 0] > 0).all(), (what, "padding")


# ---- 1. the noise -------------------------------------------------------------------------------------------------------------------
def test_the_noise_is_numpys_stream_at_a_64_bit_offset(hip):
    """r: EQUAL to numpy's advance(u << 32 | i) + random().  g within 8 * 2^-53 * max(1, |g|), derived: both sides form
    E = -log(1 - r) from the same exact 1 - r with a log good to one ulp (relative error at most 2^-52 each), so
    log(E) differs between them by at most 2 * 2^-52 absolutely (d log E = dE / E), and each side's second log adds one
    ulp of its result, at most 2^-52 |g|: |g_dev - g_np| <= 2 * 2^-52 + 2 * 2^-52 |g| <= 4 * 2^-52 max(1, |g|), which
    is 8 * 2^-53 max(1, |g|) -- the constant of the issue."""
    data = np.array([[0, 0, 0], [1, 1, 1]], dtype=np.int64)
    uu, ii = np.meshgrid([0, 1, 2, 65_535, 2 ** 31 - 1], [0, 1, 63, 64, 996, 2 ** 31 - 1], indexing="ij")
    uu, ii = i32(uu.ravel()), i32(ii.ravel())
    em = hip.HipEM(data, 2, 2, n_users=2, n_items=2, n_ratings=2)
    try:
        for seed in (0, SEED):
            r, g = em.explore_noise(words(hip, seed), uu, ii)
            want_r = er.uniforms(seed, uu, ii)
            assert np.array_equal(xm.bits(r), xm.bits(want_r)), (seed, np.flatnonzero(r != want_r))
            want_g = er.gumbel(want_r)
            err = np.abs(g - want_g) / np.maximum(1.0, np.abs(want_g))
            print(f"seed {seed}: largest |g - numpy| / max(1, |g|) = {err.max() / 2.0 ** -53:.2f} x 2^-53")
            assert (err <= 8 * 2.0 ** -53).all(), err.max()
            # the bit generator itself is taken as well, and left where it stands
            bg = np.random.default_rng(seed).bit_generator
            assert np.array_equal(em.explore_noise(bg, uu, ii)[0], r) and bg.state == np.random.default_rng(seed).bit_generator.state
        assert len(em.explore_noise(words(hip, 0), i32([]), i32([]))[0]) == 0
    finally:
        em.close()


# ---- 2. the lists ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_lists_scores_and_propensities(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users, scores = case["users"], case["scores"]
    if variant[0] == "constant":
        assert (scores == scores[0, 0]).all()
    state = words(hip, SEED)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        g = noise_of(hip, em, SEED, users, I)
        short = 0
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            for T in TEMPERATURES:
                want = er.explore(scores, users, T, g, max(NS), seen=case["seen"] if exclude else None)
                for n in NS:
                    got = em.recommend_query_explore(users, n, T, state)
                    same_answer(got, want, f"T={T} n={n} exclude={exclude}", n)
                    for b in np.flatnonzero((got[3] > 0) & (got[3] < n)):         # fewer candidates than n: ends in 1.0
                        assert got[2][b, got[3][b] - 1] == 1.0, (T, n, b)
                        short += 1
            em.recommend_end()
        assert short > 0 or U < 3
    finally:
        em.close()


# ---- 3. filtering ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(VARIANTS[0], xm.MANY[0]), (VARIANTS[1], xm.MANY[1])], ids=["mixed-K7L9", "constant-K9L5"])
def test_a_candidate_list_filters_the_full_perturbed_order(hip, variant, shape):
    """The noise of a pair does not depend on the candidates: query_explore(cand_items = C, own exclusions) is the
    user's full perturbed order (n = I) filtered and cut to n, its propensities those of the smaller candidate set."""
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    again = np.arange(min(U, 7))[::-1]                        # a user asked twice carries two different lists
    users = i32(np.concatenate([case["users"], again]))
    scores = case["scores"][users]
    state = words(hip, SEED)
    subsets = {"every_other": np.arange(0, I, 2), "block": np.arange(70, 70 + 300),
               "sparse": np.unique(np.concatenate([rng.choice(I, 40, replace=False), np.arange(5, I, 64)[:6]]))}
    T = 1.0
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        g = noise_of(hip, em, SEED, users, I)
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            full = em.recommend_query_explore(users, I, T, state)
            assert np.array_equal(full[3], (scores > -np.inf).sum(axis=1) - np.array(
                [len(case["seen"][u]) if exclude else 0 for u in users.tolist()]))
            for sname, cand in subsets.items():
                lists = own_lists(rng, users, I, cand)
                ok = er.candidate_mask(len(users), I, users, cand, case["seen"] if exclude else None, lists)
                for n in (1, 10, 257):
                    got = em.recommend_query_explore(users, n, T, state, i32(cand), cat.csr(lists))
                    for b in range(len(users)):
                        order = full[0][b, :full[3][b]]
                        kept = order[ok[b, order]][:n]
                        assert got[3][b] == len(kept) == min(n, ok[b].sum()), (sname, n, b)
                        assert np.array_equal(got[0][b, :len(kept)], kept), (sname, n, b)
                    same_answer(got, er.explore(scores, users, T, g, n, cand, case["seen"] if exclude else None, lists),
                                f"{sname} n={n} exclude={exclude}")
            em.recommend_end()
    finally:
        em.close()


# ---- 4. independence ------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return all(np.array_equal(x, y) if x.dtype.kind == "i" else np.array_equal(xm.bits(x), xm.bits(y)) for x, y in zip(a, b))


def test_a_row_depends_on_its_user_and_the_arguments_alone(hip):
    variant, shape = VARIANTS[0], xm.MANY[0]
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users = case["users"]
    state = words(hip, SEED)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        for n, T in ((10, 1.0), (257, 0.25)):
            full = em.recommend_query_explore(users, n, T, state)
            assert same_bits(em.recommend_query_explore(users, n, T, words(hip, SEED)), full)          # the same seed again
            other = em.recommend_query_explore(users, n, T, words(hip, SEED + 1))
            assert not np.array_equal(other[0], full[0]) and np.array_equal(other[3], full[3])         # another seed
            for b in (0, 1, 2, 3, 127, 128, U - 1):                                                       # one at a time
                assert same_bits(em.recommend_query_explore(users[b:b + 1], n, T, state), [a[b:b + 1] for a in full]), (n, b)
            assert same_bits(em.recommend_query_explore(users[::-1], n, T, state), [a[::-1] for a in full])    # reversed
            twice = i32(np.concatenate([users[:40], users[:40]]))                                      # twice in one request
            got = em.recommend_query_explore(twice, n, T, state)
            assert same_bits(got, [np.concatenate([a[:40], a[:40]]) for a in full])
        em.recommend_end()
    finally:
        em.close()


def test_batches_of_users(hip):
    """300 users over 100,003 items: three batches (128 + 128 + 44 rows), so the second buffer, the row states and the
    finish run at a row offset of the request; rows either side of every batch border against single-user calls."""
    U, I, K, L, R, S = xm.BATCHES
    case = xm.make_case("mixed", "stars", xm.BATCHES, n_random=3000)
    users = case["users"]
    assert xm.batch_users(I, U) == 128
    state = words(hip, SEED)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        full = em.recommend_query_explore(users, 10, 1.0, state)
        assert (full[3] == 10).sum() >= U - 2
        for b in (0, 127, 128, 255, 256, 299):
            one = em.recommend_query_explore(users[b:b + 1], 10, 1.0, state)
            assert same_bits(one, [a[b:b + 1] for a in full]), b
        # ... and the lists' propensities, three batches too, are the call's own
        keep = np.arange(10)[None, :] < full[3][:, None]
        lists = (np.concatenate([[0], np.cumsum(full[3])]).astype(np.int64), i32(full[0][keep]))
        sc, pr = em.recommend_list_propensity(users, lists, 1.0)
        assert np.array_equal(xm.bits(pr), xm.bits(full[2][keep])) and np.array_equal(xm.bits(sc), xm.bits(full[1][keep]))
        em.recommend_end()
    finally:
        em.close()


# ---- 5. concentrated mass -------------------------------------------------------------------------------------------------------------
def test_concentrated_mass_is_summed_from_what_remains(hip):
    """Family "rare": seven items on the better level.  At T = 2^-7 (above the floor 4 / 700) they carry all of the mass
    but 1e-40 of it; positions 8 .. 10 are drawn from the rest, and R_t formed as full-row sum minus head is 0 there."""
    variant, shape = ("rare", "stars"), xm.MANY[0]
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users, scores = case["users"], case["scores"]
    T, n = 2.0 ** -7, 10
    assert 4.0 / T <= er.FLOOR
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        g = noise_of(hip, em, SEED, users, I)
        open_session(em, S, case["w"], False)
        got = em.recommend_query_explore(users, n, T, words(hip, SEED))
        same_answer(got, er.explore(scores, users, T, g, n), "rare")
        broken = 0
        for b in range(U):
            order = er.row_order(scores[b], g[b], T, np.ones(I, dtype=bool))
            wide = er.row_propensities(scores[b], order, T, np.longdouble)[:n]
            assert close(got[2][b, 1:], wide[1:]), (b, got[2][b], wide)
            broken += not close(er.row_propensities_by_difference(scores[b], order, T)[1:n], wide[1:])
        assert broken == U                                     # the difference fails on every row of this case
        em.recommend_end()
    finally:
        em.close()


# ---- 6. the statistics of the device's lists ----------------------------------------------------------------------------------------------
def test_the_devices_lists_are_plackett_luce(hip):
    """test_explore_cpu's case on the device: 4,096 users with identical theta rows, eight items scoring
    5, 4.5, 4, 4, 3, 2, 1.5, 1 -- an item's score is its group's expected rating.  The same 4 standard errors."""
    U, I, K, L, R = er.PL_ROWS, len(er.PL_SCORES), 2, len(er.PL_SCORES), 5
    theta, eta, p = np.full((U, K), 0.5), np.eye(L), np.zeros((K, L, R))
    for l, s in enumerate(er.PL_SCORES):
        lo = int(np.floor(s)) - 1
        p[:, l, lo] = 1.0 - (s - np.floor(s))
        if s > np.floor(s):
            p[:, l, lo + 1] = s - np.floor(s)
    data = np.array([[0, 0, 0]], dtype=np.int64)
    users = np.arange(U, dtype=np.int32)
    em = context(hip, data, [(theta, eta, p)], U, I, R)
    try:
        open_session(em, 1, np.arange(1.0, R + 1), False)
        plain = em.recommend_query(users[:3], I)
        assert np.array_equal(np.sort(plain[1], axis=1)[:, ::-1], np.tile(np.sort(er.PL_SCORES)[::-1], (3, 1)))
        items, sc, prop, counts = em.recommend_query_explore(users, er.PL_N, er.PL_T, words(hip, er.PL_SEED))
        em.recommend_end()
    finally:
        em.close()
    assert (counts == er.PL_N).all() and np.array_equal(sc, er.PL_SCORES[items])
    d_first, d_incl = er.pl_deviations(items, er.PL_SCORES, er.PL_T, er.PL_N)
    print(f"largest deviations: first place {d_first:.2f}, top-3 inclusion {d_incl:.2f} standard errors")
    assert d_first <= 4.0 and d_incl <= 4.0, (d_first, d_incl)
    first = er.pl_exact(er.PL_SCORES, er.PL_T, er.PL_N)[0]
    assert close(prop[:, 0], first[items[:, 0]])


# ---- 7. the propensities of given lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(VARIANTS[0], xm.MANY[0]), (VARIANTS[0], SPLIT)], ids=["mixed-K7L9", "mixed-split"])
def test_list_propensity(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users, scores = case["users"], case["scores"]
    rng = np.random.default_rng(5)
    state = words(hip, SEED)
    cand = np.arange(0, I, 2)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            seen = case["seen"] if exclude else None
            for T, n, cd in ((1.0, 10, None), (0.25, 257, None), (4.0, 1024, None), (1.0, 10, cand)):
                # query_explore's own output, with the same arguments: the same bits
                own = own_lists(rng, users, I, np.arange(I) if cd is None else cd)
                gi, gs, gp, gc = em.recommend_query_explore(users, n, T, state, None if cd is None else i32(cd), cat.csr(own))
                lists = (np.concatenate([[0], np.cumsum(gc)]).astype(np.int64), i32(gi[gi >= 0]))
                keep = np.arange(n)[None, :] < gc[:, None]
                sc, pr = em.recommend_list_propensity(users, lists, T, None if cd is None else i32(cd), cat.csr(own))
                assert np.array_equal(xm.bits(pr), xm.bits(gp[keep])), (T, n, exclude)
                assert np.array_equal(xm.bits(sc), xm.bits(gs[keep])), (T, n, exclude)
            # arbitrary shuffled lists, some of their items no candidates, an empty list, one of 1,024 items
            ok = er.candidate_mask(U, I, users, cand, seen)
            given = []
            for b in range(U):
                given.append(rng.choice(I, min((0, 1024, 7, 1, 40)[b % 5], I), replace=False).tolist())
            if U >= 4:
                given[3] = rng.permutation(np.flatnonzero(ok[3])).tolist()[:1024]       # every candidate of a row (up to 1,024)
            assert any(len(x) == 0 for x in given) and any(len(x) == min(1024, I) for x in given)
            for T in (0.25, 4.0):
                sc, pr = em.recommend_list_propensity(users, cat.csr(given), T, i32(cand))
                at = 0
                for b in range(U):
                    ws, wp = er.list_propensity(scores[b], ok[b], T, given[b])
                    e = at + len(given[b])
                    assert np.array_equal(xm.bits(sc[at:e]), xm.bits(ws)), (T, b)
                    assert close(pr[at:e], wp) and np.array_equal(pr[at:e] == 0, wp == 0), (T, b)
                    # the non-candidates taken out of the list: the rest is unchanged, bit for bit
                    if b < 12 and len(given[b]):
                        inside = [i for i in given[b] if ok[b, i]]
                        s2, p2 = em.recommend_list_propensity(users[b:b + 1], cat.csr([inside]), T, i32(cand))
                        mask = ok[b, np.asarray(given[b])]
                        assert np.array_equal(xm.bits(p2), xm.bits(pr[at:e][mask])) and (pr[at:e][~mask] == 0).all()
                        assert np.isneginf(sc[at:e][~mask]).all()
                    at = e
                if U >= 4 and len(given[3]) == ok[3].sum() > 0:
                    assert pr[sum(len(x) for x in given[:3]) + len(given[3]) - 1] == 1.0
            em.recommend_end()
    finally:
        em.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_requests_are_refused_before_any_launch(hip):
    import ctypes as C
    U, I, K, L, R, S = xm.MANY[0]
    case = case_of(("mixed", "stars"), xm.MANY[0])
    E = hip._lib.HipLibraryError
    users = i32([0, 1])
    state = words(hip, SEED)
    off = np.array([0, 2, 3], dtype=np.int64)
    good = (off, i32([3, 5, 8]))

    def refused(call, code=None):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == (hip._lib.E_INVALID if code is None else code), e.value

    with LaunchWindow() as lw:
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            refused(lambda: em.recommend_query_explore(users, 10, 1.0, state))                   # no session
            refused(lambda: em.recommend_list_propensity(users, good, 1.0))
            em.recommend_begin(case["w"], True)
            refused(lambda: em.recommend_query_explore(users, 10, 1.0, state))                   # a session without a slot
            refused(lambda: em.recommend_list_propensity(users, good, 1.0))
            for s in range(S):
                em.select(s).recommend_add()
            floor = (case["w"].max() - case["w"].min()) / er.FLOOR
            for T in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), floor * 0.99, 1e-300):
                refused(lambda: em.recommend_query_explore(users, 10, T, state))
                refused(lambda: em.recommend_list_propensity(users, good, T))
            refused(lambda: em.recommend_query_explore(users, 0, 1.0, state))                     # n < 1
            refused(lambda: em.recommend_query_explore(users, -3, 1.0, state))
            refused(lambda: em.recommend_query_explore(users, 1025, 1.0, state), hip._lib.E_UNSUPPORTED)
            refused(lambda: em.recommend_query_explore(users, 10, 1.0, None))                     # a null state
            refused(lambda: em.explore_noise(None, i32([0]), i32([0])))
            refused(lambda: em.explore_noise(state, i32([0, -1]), i32([0, 0])))                   # a negative id
            for call in (lambda u=users, c=None, x=None: em.recommend_query_explore(u, 10, 1.0, state, c, x),
                         lambda u=users, c=None, x=None: em.recommend_list_propensity(u, good, 1.0, c, x)):
                refused(lambda: call(u=i32([0, U])))                                              # an id out of range
                refused(lambda: call(u=i32([-1, 0])))
                refused(lambda: call(c=i32([5, 3, 8])))                                           # not strictly ascending
                refused(lambda: call(c=i32([3, 3, 8])))
                refused(lambda: call(c=i32([3, 5, I])))
                refused(lambda: call(x=(np.array([0, 2, 1], dtype=np.int64), i32([1]))))          # a bad CSR
                refused(lambda: call(x=(off, i32([1, 2, I]))))
            refused(lambda: em.recommend_list_propensity(users, (off, i32([3, 3, 8])), 1.0))      # an item twice in a list
            refused(lambda: em.recommend_list_propensity(users, (off, i32([3, 5, I])), 1.0))
            refused(lambda: em.recommend_list_propensity(users, (np.array([1, 2, 3], dtype=np.int64), i32([3, 5, 8])), 1.0))
            long = (np.array([0, 1025, 1025], dtype=np.int64), i32(np.arange(1025) % I))
            refused(lambda: em.recommend_list_propensity(users, long, 1.0), hip._lib.E_UNSUPPORTED)
            # null outputs that are needed
            up = users.ctypes.data_as(C.POINTER(C.c_int32))
            refused(lambda: hip._lib.call("mmsbm_hip_recommend_query_explore", em._h, 2, up, 0, None, None, None, 10, 1.0,
                                          state, None, None, None, None))
            # nothing to show is no error, and launches nothing either
            none = em.recommend_query_explore(users, 10, 1.0, state, i32([]))
            assert (none[0] == -1).all() and np.isneginf(none[1]).all() and (none[2] == 0).all() and (none[3] == 0).all()
            assert len(em.recommend_query_explore(users[:0], 10, 1.0, state)[3]) == 0
            sc, pr = em.recommend_list_propensity(users, (np.zeros(3, dtype=np.int64), i32([])), 1.0)
            assert len(sc) == len(pr) == 0
        finally:
            em.close()
        names = lw.names()
        assert not [k for k in names if k.startswith(("explore_", "cat_", "rec_score", "rec_select", "rec_exclude"))], names
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        before = em.recommend_query(case["users"], 10)
        em.recommend_query_explore(case["users"], 10, 1.0, state)
        after = em.recommend_query(case["users"], 10)                                             # the session still answers
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert em.get_option("recommend_ms") > 0
        em.recommend_end()
    finally:
        em.close()


# ---- 9. the host class ----------------------------------------------------------------------------------------------------------------
def test_the_host_class_with_string_ids(hip):
    rng = np.random.default_rng(12)
    n_u, n_i, n_obs = 60, 150, 1500
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 6, iterations=8, sampling=2, seed=5)
    model.fit(df, silent=True)
    items = list(model.data_handler.item_labels())
    ask = ["u7", "u1", "u30"]
    pairs = [("u7", items[0]), ("u1", items[5]), ("nobody", items[0])]
    cand = [items[j] for j in rng.choice(len(items), 90, replace=False)]
    columns = ["users", "items", "score", "propensity", "rank"]
    for kw in ({}, {"candidates": cand, "exclude": pairs}, {"exclude_seen": False, "weights": [0, 0, 1, 2, 5]}):
        plain = model.recommend(users=ask, n=7, **kw)
        zero = model.recommend_explore(users=ask, n=7, temperature=0, **kw)
        assert list(zero.columns) == columns and (zero["propensity"] == 1.0).all()
        assert zero.drop(columns="propensity").equals(plain)
        got = model.recommend_explore(users=ask, n=7, temperature=0.5, seed=3, **kw)
        assert list(got.columns) == columns and len(got) == len(plain)
        assert all(got[c].dtype == zero[c].dtype for c in columns)
        assert got.equals(model.recommend_explore(users=ask, n=7, temperature=0.5, seed=np.random.default_rng(3), **kw))
        assert not got["items"].equals(model.recommend_explore(users=ask, n=7, temperature=0.5, seed=4, **kw)["items"])
        assert ((got["propensity"] > 0) & (got["propensity"] <= 1)).all() and got["rank"].tolist() == plain["rank"].tolist()
        # a score is recommend's: the item's score in the user's full list
        everything = model.recommend(users=ask, n=len(items), **kw).set_index(["users", "items"])["score"]
        assert np.array_equal(xm.bits(got["score"].to_numpy()),
                              xm.bits(everything.loc[list(zip(got["users"], got["items"]))].to_numpy()))
        # propensities() of the frame reproduces the column, from the rank column or from the order of appearance
        back = model.propensities(got, temperature=0.5, **kw)
        assert list(back.columns) == ["users", "items", "rank", "score", "propensity"]
        for frame in (back, model.propensities(got.drop(columns="rank"), temperature=0.5, **kw)):
            assert frame["users"].tolist() == got["users"].tolist() and frame["items"].tolist() == got["items"].tolist()
            assert frame["rank"].tolist() == got["rank"].tolist()
            assert np.array_equal(xm.bits(frame["propensity"].to_numpy()), xm.bits(got["propensity"].to_numpy()))
            assert np.array_equal(xm.bits(frame["score"].to_numpy()), xm.bits(got["score"].to_numpy()))
        upside = model.propensities(got.iloc[::-1], temperature=0.5, **kw)        # the rank column decides, not the row order
        key = list(zip(got["users"], got["items"]))
        assert np.array_equal(xm.bits(upside.set_index(["users", "items"])["propensity"].loc[key].to_numpy()),
                              xm.bits(got["propensity"].to_numpy()))
        # another policy's view of the same lists: other numbers, the same shape
        other = model.propensities(got, temperature=2.0, **kw)
        assert len(other) == len(got) and not np.array_equal(other["propensity"].to_numpy(), got["propensity"].to_numpy())
    # an item the policy could not have shown: 0 and -inf
    seen = df[df["users"] == "u7"]["items"].iloc[0]
    logged = pd.DataFrame({"users": ["u7", "u7"], "items": [seen, model.recommend(users=["u7"], n=1)["items"].iloc[0]]})
    back = model.propensities(logged, temperature=0.5)
    assert back["propensity"].iloc[0] == 0 and np.isneginf(back["score"].iloc[0]) and back["propensity"].iloc[1] > 0
    with pytest.raises(KeyError):
        model.propensities(pd.DataFrame({"users": ["nobody"], "items": [items[0]]}), temperature=0.5)
    with pytest.raises(ValueError, match="floor"):
        model.recommend_explore(users=ask, temperature=1e-4)
    empty = model.recommend_explore(users=ask, temperature=0.5, candidates=[])
    assert len(empty) == 0 and list(empty.columns) == columns


# ---- 10. the launch log: these cases reach every kernel of explore.hpp ------------------------------------------------------------------
def test_every_explore_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("explore_")]
    for k in ("explore_norm_kernel", "explore_perturb_kernel", "explore_finish_kernel", "explore_list_kernel",
              "explore_noise_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
