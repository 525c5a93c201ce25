"""Item-side serving on the device (mmsbm_hip_recommend_query_items / mmsbm_hip_recommend_audience, HipEM.*,
MMSBM.recommend_users / recommend_users_new_items / audience; audience.hpp):

1. by EQUALITY with the exact reference (exact_models.exact_scores, transposed) on the cases of test_audience_cpu.py,
   which asserts on the restatement that their tie groups span several user tiles and that their traps are set:
   ids, counts, padding, offsets, scores by their bits;
2. by EQUALITY with the user side on random dense models: recommend_query(all users, n = I) scattered into a U x I
   matrix is what both item-side queries give -- the same fma chain with the tables exchanged, so no tolerance --
   also in swapped contexts, with uploaded parameters, after recommend_add_items and on data with duplicate pairs;
3. split independence of the audience (rows per COUNT batch x entries per WRITE batch) and request independence;
4. wide rows: one item over 5,000 users (columns split across selecting waves), 200 items over 70,000 users (two
   batches of the score buffer);
5. refusals by status code, 6. no side effects, 7. the launch log, 8. the host class end to end with string ids.

MMSBM_E_TOOLARGE for missing device memory is the one refusal not provoked here."""
import ctypes as C
import os
import sys

import numpy as np
import pandas as pd
import pytest

import exact_models as xm
from conftest import ROOT
from test_audience_cpu import (CASE_ID, EXACT_CASES, by_item, exact_case, restate_audience, restate_item_query,
                               tie_group)
from test_gpu_recommend import TOL, LaunchWindow, context, hip, problem  # noqa: F401  (hip: the fixture)
from test_gpu_serving_exact import open_session, same_answer
from test_recommend_cpu import restate_scores, seen_items

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW = {}
SCORE_BUFFER_KERNELS = ("rec_score_kernel", "rec_exclude_kernel", "rec_select_kernel<")
NEW_KERNELS = ("aud_tile_kernel<false>", "aud_tile_kernel<true>", "aud_offsets_kernel")
TINY = ("mixed", "stars", (1, 5, 2, 3, 3, 2), 5)           # one user: U = 1 x I = 5


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


def same_csr(got, want, what):
    """(offsets, users, scores) equal in every entry, scores by their bits."""
    for g, w, nm in zip(got, want, ("offsets", "users", "scores")):
        gb, wb = (xm.bits(g), xm.bits(w)) if nm == "scores" else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        assert gb.shape == wb.shape, f"{what}: {nm} has shape {gb.shape}, expected {wb.shape}"
        if not np.array_equal(gb, wb):
            at = int(np.flatnonzero(gb != wb)[0])
            raise AssertionError(f"{what}: {nm} differ in {int((gb != wb).sum())} entries, first at {at}: "
                                 f"device {np.asarray(g)[at]}, expected {np.asarray(w)[at]}")


def below(x):
    return float(np.nextafter(x, -np.inf))


def above(x):
    return float(np.nextafter(x, np.inf))


# ---- 1. exact, by equality ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude", [True, False], ids=["unseen_pairs", "all_pairs"])
@pytest.mark.parametrize("case", EXACT_CASES + [TINY], ids=CASE_ID)
def test_exact_cases(hip, case, exclude):
    c = exact_case(case)
    U, I, K, L, R, S = c["shape"]
    s, seen = c["scores_T"], (c["seen"] if exclude else None)
    items = np.arange(I, dtype=np.int32)
    em = context(hip, c["data"], c["params"], U, I, R)
    try:
        open_session(em, S, c["w"], exclude)
        for n in (1, 10, 300, 1024):
            same_answer(em.recommend_query_items(items, n), restate_item_query(s, items, n, seen), f"{CASE_ID(case)} n={n}")
        bars = [below(s.min()), above(s.max())]
        for i in sorted({0, min(1, I - 1), I - 1}):
            med = np.sort(s[i])[U // 2]
            bars += [float(med), above(med)]               # item i's tie group at the median: all in, all out
        if case[1] == "signed":
            bars += [0.0, -0.0]
        for bar in bars:
            want = restate_audience(s, items, bar, seen)
            same_csr(em.recommend_audience(items, bar), want, f"{CASE_ID(case)} bar={bar!r}")
            sizes = em.recommend_audience(items, bar, count_only=True)
            assert sizes[1] is None and sizes[2] is None and np.array_equal(sizes[0], want[0])
        low = em.recommend_audience(items, bars[0], count_only=True)[0]   # candidates(i) exactly: no padded lane counted
        assert np.diff(low).tolist() == [U - (len(seen[i]) if seen else 0) for i in range(I)]
        assert (em.recommend_audience(items, bars[1])[0] == 0).all()
        assert em.get_option("audience_ms") > 0 and em.get_option("recommend_ms") > 0
        em.recommend_end()
    finally:
        em.close()


# ---- 2. the user side as the yardstick, bit for bit ------------------------------------------------------------------------
def user_side_matrix(em, U, n_cat):
    """recommend_query(all users, n = catalogue) scattered into U x catalogue; -inf where a pair is left out."""
    items, scores, counts = em.recommend_query(np.arange(U, dtype=np.int32), n_cat)
    keep = np.arange(n_cat)[None, :] < counts[:, None]
    m = np.full((U, n_cat), -np.inf)
    m[np.repeat(np.arange(U), counts), items[keep]] = scores[keep]
    return m


def query_items_matrix(em, U, n_cat, ids):
    n = min(U, 1024)
    users, scores, counts = em.recommend_query_items(ids, n)
    keep = np.arange(n)[None, :] < counts[:, None]
    m = np.full((U, n_cat), -np.inf)
    m[users[keep], np.repeat(np.asarray(ids), counts)] = scores[keep]
    for b in range(len(ids)):                               # the device's own order: score descending, user ascending
        u, v = users[b, :counts[b]], scores[b, :counts[b]]
        assert np.array_equal(np.lexsort((u, -v)), np.arange(counts[b]))
        assert (users[b, counts[b]:] == -1).all() and np.isneginf(scores[b, counts[b]:]).all()
    return m


def audience_matrix(em, U, n_cat, ids, bar):
    off, users, scores = em.recommend_audience(ids, bar)
    assert off[0] == 0 and off[-1] == len(users) == len(scores)
    at = np.repeat(np.arange(len(ids)), np.diff(off))
    assert all((np.diff(users[off[b]:off[b + 1]]) > 0).all() for b in range(len(ids)))     # ascending user ids
    m = np.full((U, n_cat), -np.inf)
    m[users, np.asarray(ids)[at]] = scores
    return m


def same_matrix(got, want, what):
    np.testing.assert_array_equal(xm.bits(got), xm.bits(want), err_msg=what)


def both_sides_agree(em, U, n_cat, what, ids=None):
    ids = np.arange(n_cat, dtype=np.int32) if ids is None else ids
    want = user_side_matrix(em, U, n_cat)
    finite = want[np.isfinite(want)]
    bar = below(finite.min()) if len(finite) else 0.0
    cols = np.asarray(ids)
    if U <= 1024:
        same_matrix(query_items_matrix(em, U, n_cat, ids)[:, cols], want[:, cols], f"{what}: query_items")
    same_matrix(audience_matrix(em, U, n_cat, ids, bar)[:, cols], want[:, cols], f"{what}: audience")
    return want


DENSE = [(2, 3, 2, 1, 997, 61), (20, 20, 5, 3, 700, 300), (5, 33, 10, 1, 130, 3), (50, 50, 10, 1, 3, 200)]
DENSE_ID = lambda c: "K{}L{}R{}S{}U{}I{}".format(*c)  # noqa: E731


@pytest.mark.parametrize("swap", [0, 1], ids=["unswapped", "swapped"])
@pytest.mark.parametrize("shape", DENSE, ids=DENSE_ID)
def test_random_models_equal_the_user_side(hip, shape, swap):
    K, L, R, S, U, I = shape
    data, params = problem(U, I, R, K, L, S, 5 * U + 50, seed=K + U)
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R, swap=swap)
    try:
        assert em.swapped == bool(swap)
        for exclude in (True, False):
            open_session(em, S, w, exclude)
            both_sides_agree(em, U, I, f"{shape} swap={swap} exclude={exclude}")
            em.recommend_end()
    finally:
        em.close()


def test_swapped_resident_and_uploaded_parameters_are_bitwise_equal(hip):
    K, L, R, S, U, I = 20, 20, 5, 3, 700, 300
    data, params = problem(U, I, R, K, L, S, 4000, seed=11)
    w = np.arange(1.0, R + 1)
    mats = []
    for swap in (0, 1):
        em = context(hip, data, params, U, I, R, swap=swap)
        try:
            open_session(em, S, w, True)
            mats.append(both_sides_agree(em, U, I, f"swap={swap}"))
            em.recommend_end()
        finally:
            em.close()
    same_matrix(mats[1], mats[0], "swapped / unswapped")
    em = context(hip, data, params, U, I, R)
    try:
        em.iterate(3)                                      # resident slots, moved by the EM loop
        fitted = [em.select(s).get_params() for s in range(S)]
        open_session(em, S, w, True)
        resident = both_sides_agree(em, U, I, "resident")
        em.recommend_end()
    finally:
        em.close()
    other = context(hip, data, fitted, U, I, R)
    try:
        open_session(other, S, w, True)
        same_matrix(both_sides_agree(other, U, I, "uploaded"), resident, "uploaded / resident")
        other.recommend_end()
    finally:
        other.close()


def test_after_added_items(hip):
    K, L, R, S, U, I, n_new = 6, 9, 4, 2, 300, 200, 5
    data, params = problem(U, I, R, K, L, S, 2000, seed=21)
    rng = np.random.default_rng(22)
    eta_new = rng.random((S, n_new, L))
    off = np.concatenate([[0], np.cumsum(rng.integers(1, 40, n_new))]).astype(np.int64)
    seen_users = rng.integers(0, U, off[-1]).astype(np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, np.arange(1.0, R + 1), exclude)
            before = both_sides_agree(em, U, I, "before add_items")           # (builds the item -> users lists)
            em.recommend_add_items(eta_new, (off, seen_users))
            new_ids = np.arange(I, I + n_new, dtype=np.int32)
            after = both_sides_agree(em, U, I + n_new, f"added items exclude={exclude}")
            both_sides_agree(em, U, I + n_new, "the new ids alone", ids=new_ids)
            same_matrix(after[:, :I], before, "training items' rows unchanged")
            for j in range(n_new):                                             # the new items' seen pairs are out
                assert np.isneginf(after[seen_users[off[j]:off[j + 1]], I + j]).all()
                assert np.isfinite(after[:, I + j]).sum() == U - len(set(seen_users[off[j]:off[j + 1]].tolist()))
            em.recommend_end()
    finally:
        em.close()


def test_duplicate_training_pairs_count_once(hip):
    K, L, R, S, U, I = 4, 5, 3, 2, 260, 150
    data, params = problem(U, I, R, K, L, S, 1500, seed=31)
    data = np.concatenate([data, data[:400], data[:100]])
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, np.arange(1.0, R + 1), True)
        want = both_sides_agree(em, U, I, "duplicate pairs")
        seen = by_item(seen_items(data, U), I)
        sizes = np.diff(em.recommend_audience(np.arange(I), below(want[np.isfinite(want)].min()), count_only=True)[0])
        assert sizes.tolist() == [U - len(seen[i]) for i in range(I)]
        em.recommend_end()
    finally:
        em.close()


# ---- 3. split and request independence -----------------------------------------------------------------------------------
def test_the_audience_does_not_depend_on_the_split_or_the_request(hip):
    K, L, R, S, U, I = 4, 4, 3, 2, 5000, 300
    data, params = problem(U, I, R, K, L, S, 20000, seed=41)
    items = np.arange(I, dtype=np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, np.arange(1.0, R + 1), True)
        sample = em.recommend_query(np.arange(0, U, 97, dtype=np.int32), I)[1]
        bar = float(np.percentile(sample[np.isfinite(sample)], 80))
        want = em.recommend_audience(items, bar)
        assert 0 < want[0][-1] < U * I and (np.diff(want[0]) > 1).any()
        for rows in (1, 7, 128, 0):
            for entries in (1, 1000, 0):
                em.set_option("audience_rows", rows)
                em.set_option("audience_entries", entries)
                assert em.get_option("audience_rows") == rows and em.get_option("audience_entries") == entries
                same_csr(em.recommend_audience(items, bar), want, f"rows={rows} entries={entries}")
        rng = np.random.default_rng(3)
        for name, ask in (("subset", rng.choice(I, 40, replace=False)), ("permutation", rng.permutation(I)),
                          ("repeats", np.array([7, 7, 250, 7, 0, 250]))):
            off, us, sc = em.recommend_audience(ask, bar)
            qu, qs, qc = em.recommend_query_items(ask, 10)
            one = em.recommend_query_items(items, 10)
            for b, i in enumerate(ask.tolist()):
                lo, hi = want[0][i], want[0][i + 1]
                assert np.array_equal(us[off[b]:off[b + 1]], want[1][lo:hi]), (name, b)
                assert np.array_equal(xm.bits(sc[off[b]:off[b + 1]]), xm.bits(want[2][lo:hi])), (name, b)
                assert np.array_equal(qu[b], one[0][i]) and np.array_equal(xm.bits(qs[b]), xm.bits(one[1][i])) and qc[b] == one[2][i]
        em.recommend_end()
    finally:
        em.close()


# ---- 4. wide rows ----------------------------------------------------------------------------------------------------------
def test_one_item_over_five_thousand_users(hip):
    """The 5,000 columns of one row split across selecting waves and are merged; the row's tie group spans 40 tiles."""
    c = exact_case(EXACT_CASES[3])
    U, I, K, L, R, S = c["shape"]
    em = context(hip, c["data"], c["params"], U, I, R)
    try:
        for exclude in (True, False):
            seen = c["seen"] if exclude else None
            open_session(em, S, c["w"], exclude)
            for ask in ([1], [0]):
                for n in (5, 1024):
                    same_answer(em.recommend_query_items(ask, n), restate_item_query(c["scores_T"], ask, n, seen), f"{ask} n={n}")
            em.recommend_end()
    finally:
        em.close()


def test_two_hundred_items_over_seventy_thousand_users(hip):
    """128 rows of 70,000 columns fill a batch of the score buffer: the query runs two batches."""
    U, I, K, L, R, S = 70_000, 200, 4, 9, 3, 2
    assert xm.batch_users(U, I) == 128
    rng = np.random.default_rng(51)
    params, w = xm.model("sorted", rng, U, I, K, L, R, S, "stars")
    data = np.stack([rng.integers(0, U, 60_000), rng.integers(0, I, 60_000), rng.integers(0, R, 60_000)], 1)
    s = np.ascontiguousarray(xm.exact_scores(params, np.arange(U), I, w).T)
    seen = by_item(seen_items(data, U), I)
    items = np.arange(I, dtype=np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        open_session(em, S, w, True)
        same_answer(em.recommend_query_items(items, 10), restate_item_query(s, items, 10, seen), "70,000 users")
        bar = float(np.sort(s[1])[U - 500])
        same_csr(em.recommend_audience(items, bar), restate_audience(s, items, bar, seen), "70,000 users, audience")
        em.recommend_end()
    finally:
        em.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def refused(hip, code, fn, *args, **kw):
    with pytest.raises(hip._lib.HipLibraryError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.message)


def test_refusals_by_status_code(hip):
    U, I, K, L, R = 50, 60, 4, 3, 3
    data, params = problem(U, I, R, K, L, 1, 300, seed=2)
    lib = hip._lib
    w = np.arange(1.0, R + 1)
    em = context(hip, data, params, U, I, R)
    try:
        refused(hip, lib.E_INVALID, em.recommend_query_items, [0], 3)             # no session
        refused(hip, lib.E_INVALID, em.recommend_audience, [0], 0.0)
        em.recommend_begin(w, True)
        refused(hip, lib.E_INVALID, em.recommend_query_items, [0], 3)             # before the first add
        refused(hip, lib.E_INVALID, em.recommend_audience, [0], 0.0)
        em.recommend_add()
        for bad in (-1, I):                                                       # an id = the catalogue's size; id -1
            refused(hip, lib.E_INVALID, em.recommend_query_items, [0, bad], 3)
            refused(hip, lib.E_INVALID, em.recommend_audience, [0, bad], 0.0)
        refused(hip, lib.E_INVALID, em.recommend_query_items, [0], 0)
        refused(hip, lib.E_UNSUPPORTED, em.recommend_query_items, [0], hip.HipEM.MAX_RECOMMEND + 1)
        for bad in (np.nan, np.inf, -np.inf):
            refused(hip, lib.E_INVALID, em.recommend_audience, [0], bad)
        for bad in (-1, 2.5):
            refused(hip, lib.E_INVALID, em.set_option, "audience_rows", bad)
            refused(hip, lib.E_INVALID, em.set_option, "audience_entries", bad)
        items = np.arange(I, dtype=np.int32)
        want = em.recommend_audience(items, 0.0)
        total = int(want[0][-1])
        assert total > 1
        off = np.full(I + 1, -7, dtype=np.int64)                                  # capacity one short
        us, sc = np.full(total, -7, dtype=np.int32), np.full(total, -7.0)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        with pytest.raises(lib.HipLibraryError) as e:
            lib.call("mmsbm_hip_recommend_audience", em._h, I, p(items, C.c_int32), 0.0, total - 1, p(off, C.c_int64),
                     p(us, C.c_int32), p(sc, C.c_double))
        assert e.value.code == lib.E_TOOLARGE
        assert np.array_equal(off, want[0]) and (us == -7).all() and (sc == -7.0).all()
        same_csr(em.recommend_audience(items, 0.0), want, "the session is still usable")
        seen = by_item(seen_items(data, U), I)
        assert np.array_equal(em.recommend_query_items(items, 3)[2], [min(3, U - len(seen[i])) for i in range(I)])
        em.recommend_end()
        refused(hip, lib.E_INVALID, em.recommend_audience, [0], 0.0)
    finally:
        em.close()


# ---- 6. no side effects --------------------------------------------------------------------------------------------------------
def test_no_side_effects(hip):
    U, I, K, L, R, S = 200, 300, 6, 5, 5, 3
    data, params = problem(U, I, R, K, L, S, 1500, seed=13)
    w = np.arange(1.0, R + 1)
    users, items = np.arange(U, dtype=np.int32), np.arange(I, dtype=np.int32)
    em = context(hip, data, params, U, I, R)
    try:
        before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
        test = data[:500]
        open_session(em, S, w, True)
        rec = em.recommend_query(users, 10)
        top = em.recommend_top_pairs(300)[:3]
        pos = em.recommend_positions(users, np.arange(U + 1, dtype=np.int64), users % I)
        em.predict_begin(test, w)
        em.select(0).predict_add()
        first = em.recommend_query_items(items, 10)        # inside an open predict session
        aud = em.recommend_audience(items, 3.0)
        em.select(1).predict_add()
        mat, raw = em.predict_finish()
        same_answer(em.recommend_query_items(items, 10), first, "a second query")
        same_csr(em.recommend_audience(items, 3.0), aud, "a second audience")
        rec2 = em.recommend_query(users, 10)
        top2 = em.recommend_top_pairs(300)[:3]
        pos2 = em.recommend_positions(users, np.arange(U + 1, dtype=np.int64), users % I)
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
    for g, h in zip(rec + top + pos, rec2 + top2 + pos2):
        assert np.array_equal(xm.bits(g) if g.dtype == np.float64 else g, xm.bits(h) if h.dtype == np.float64 else h)
    assert np.array_equal(xm.bits(mat), xm.bits(mat2)) and np.array_equal(xm.bits(raw), xm.bits(raw2))


# ---- 7. the launch log ---------------------------------------------------------------------------------------------------------
def test_what_each_query_launches(hip):
    c = exact_case(EXACT_CASES[3])                         # 5,000 users x 2 items
    U, I, K, L, R, S = c["shape"]
    for call, must, must_not in (
            (lambda em: em.recommend_audience([1, 0], 1.5), NEW_KERNELS, SCORE_BUFFER_KERNELS),
            (lambda em: em.recommend_audience([1], 1.5, count_only=True), NEW_KERNELS[::2], SCORE_BUFFER_KERNELS + NEW_KERNELS[1:2]),
            (lambda em: em.recommend_query_items([1], 5),
             ("rec_score_kernel", "rec_exclude_kernel", "rec_select_kernel<false>", "rec_select_kernel<true>"), ("aud_",))):
        em = context(hip, c["data"], c["params"], U, I, R)
        try:
            open_session(em, S, c["w"], True)
            with LaunchWindow() as lw:
                call(em)
                em.recommend_end()
                em.close()                                 # (the log is written when the context goes)
                names = lw.names()
        finally:
            em.close()
        assert all(k in names for k in must), (must, sorted(names))
        assert not [n for n in names if n.startswith(tuple(must_not))], sorted(names)


# ---- 8. the host class, end to end -----------------------------------------------------------------------------------------------
def test_end_to_end_with_string_ids(hip):
    rng = np.random.default_rng(21)
    n_obs = 4000
    df = pd.DataFrame({"users": [f"user{x}" for x in rng.integers(0, 150, n_obs)],
                       "items": [f"film-{x}" for x in rng.integers(0, 400, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 5, iterations=30, sampling=3, seed=4)
    model.fit(df, silent=True)
    enc = model.data_handler
    ul, il = np.asarray(enc.user_labels(), dtype=object), np.asarray(enc.item_labels(), dtype=object)
    U, I = len(ul), len(il)
    params = [(r["theta"], r["eta"], r["pr"]) for r in model.results]
    w = np.asarray(model.ratings, dtype=np.float64)
    s = restate_scores(params, np.arange(U), I, w).T
    tol = TOL * np.abs(s).max()
    seen = by_item(seen_items(model.train, U), I)
    train = set(zip(df["users"], df["items"]))
    uid = {x: j for j, x in enumerate(ul.tolist())}
    iid = {x: j for j, x in enumerate(il.tolist())}

    top = model.recommend_users(n=8)
    assert list(top.columns) == ["items", "users", "score", "rank"] and list(dict.fromkeys(top["items"])) == il.tolist()
    assert not any((u, i) in train for u, i in zip(top["users"], top["items"]))
    ref = s[[iid[i] for i in top["items"]], [uid[u] for u in top["users"]]]
    np.testing.assert_allclose(top["score"].to_numpy(float), ref, rtol=0, atol=tol)
    for i, g in top.groupby("items", sort=False):
        cand = np.setdiff1d(np.arange(U), np.fromiter(seen[iid[i]], dtype=np.int64, count=len(seen[iid[i]])))
        assert len(g) == min(8, len(cand)) and g["rank"].tolist() == list(range(1, len(g) + 1))
        s_star = np.sort(s[iid[i], cand])[::-1][len(g) - 1]
        assert (s[iid[i], [uid[u] for u in g["users"]]] >= s_star - tol).all()
        assert set(ul[cand[s[iid[i], cand] > s_star + tol]].tolist()) <= set(g["users"])
    sub = model.recommend_users(items=["film-7", "film-3", "film-7"], n=3)
    assert sub["items"].tolist()[:3] == ["film-7"] * 3 and sub["items"].tolist()[-3:] == ["film-7"] * 3

    bar = float(np.percentile(s, 90))
    aud = model.audience(min_score=bar)
    assert list(aud.columns) == ["items", "users", "score", "rank"]
    assert not any((u, i) in train for u, i in zip(aud["users"], aud["items"]))
    ref = s[[iid[i] for i in aud["items"]], [uid[u] for u in aud["users"]]]
    np.testing.assert_allclose(aud["score"].to_numpy(float), ref, rtol=0, atol=tol)
    assert (aud["score"] >= bar).all()
    got = set(zip(aud["items"], aud["users"]))
    off, us, _ = restate_audience(s, np.arange(I), bar + tol, seen)               # everything clearly above the bar is in
    sure = set(zip(il[np.repeat(np.arange(I), np.diff(off))].tolist(), ul[us].tolist()))
    assert sure <= got
    off, us, _ = restate_audience(s, np.arange(I), bar - tol, seen)               # and nothing clearly below
    maybe = set(zip(il[np.repeat(np.arange(I), np.diff(off))].tolist(), ul[us].tolist()))
    assert got <= maybe
    for _, g in aud.groupby("items", sort=False):
        assert g["rank"].tolist() == list(range(1, len(g) + 1)) and (np.diff(g["score"].to_numpy(float)) <= 0).all()
    counts = model.audience(min_score=bar, count_only=True)
    assert counts["items"].tolist() == il.tolist()
    assert counts["count"].tolist() == [int(n) for n in aud.groupby("items", sort=False).size().reindex(il, fill_value=0)]
    with pytest.raises(KeyError):
        model.audience(items=["film-7", "nothing"], min_score=bar)

    new = pd.DataFrame({"users": [f"user{x}" for x in rng.integers(0, 150, 300)],
                        "items": [f"new-{x}" for x in rng.integers(0, 6, 300)], "ratings": rng.integers(1, 6, 300)})
    cold = model.recommend_users_new_items(new, n=5, iterations=20)
    labels = list(dict.fromkeys(new["items"]))
    assert list(dict.fromkeys(cold["items"])) == labels and (cold.groupby("items").size() == 5).all()
    rated = set(zip(new["users"], new["items"]))
    assert not any((u, i) in rated for u, i in zip(cold["users"], cold["items"]))
    wide = model.recommend_with_new_items(new, n=I + len(labels), iterations=20)  # the user side, transposed
    for lab in labels:
        col = wide[wide["items"] == lab]
        order = np.lexsort((np.array([uid[u] for u in col["users"]]), -col["score"].to_numpy(float)))[:5]
        mine = cold[cold["items"] == lab]
        assert mine["users"].tolist() == col["users"].to_numpy()[order].tolist()
        assert np.array_equal(xm.bits(mine["score"].to_numpy(float)), xm.bits(col["score"].to_numpy(float)[order]))


def test_every_audience_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("aud_")]
    assert sorted(compiled) == sorted(NEW_KERNELS), compiled
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
