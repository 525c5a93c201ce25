"""Leave-one-out reliability of the training rows on the device (mmsbm_hip_loo_*, HipEM.loo_*; loo.hpp) against the
numpy restatement of tests/reliability_reference.py.

Shapes: (K, L) in reliability_reference.SHAPES (lane groups of 1, 2, 8 and 16 lanes, K = 70 walked in two pieces, L =
1; K = L = 40 in a test of its own: 16 lanes, and p too large for the on-chip copy), R = 5, 300 users x 1,500 items, about 8,700 rows in scattered order: users of 1, 2, 63, 64 and 65 rows (the chunk
border), one of 1,300 rows with 100 duplicated triples (21 chunks), one item of 900 rows, two items of one row, one row
whose user and item both hold nothing else.  Models per shape: soft, sharpened (late-stage), one-hot theta, an emptied
rating tile (fit = 0).  S = 1 and 3, both side layouts.

Tolerances: fitted and reliability TOL = 1e-12 absolute (probabilities <= 1; test_reliability_cpu.py measures what the
restatement itself moves by: below 1e-15).  A user's or item's surprise: TOL / P_min + 4 * 2^-52 * |surprise|, P_min the
reference's smallest reliability among its rows -- -log moves by at most TOL / P_min where the probability moves by
TOL, and the sum of d terms and the one division round by less than the second term; computed from the reference.

1. against the restatement, 2. fitted is heldout's row value bit for bit, 3. independence bit for bit, 4. the lowest m,
5. rows of degree 1, 6. no side effects, 7. refusals by status code, 8. the launch log, 9. end to end."""
import os
import sys

import numpy as np
import pytest

import exact_models as xm
import reliability_reference as rr
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the fixture)

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12
WINDOW = {}
NEW_KERNELS = ("loo_mean_kernel", "loo_fit_kernel<true>", "loo_fit_kernel<false>", "loo_sum_kernel<true>",
               "loo_sum_kernel<false>", "loo_comb_kernel", "loo_row_kernel<true>", "loo_row_kernel<false>",
               "loo_finish_kernel", "loo_agg_kernel", "loo_gather_kernel", "loo_low_kernel<false>", "loo_low_kernel<true>")
SHAPE_ID = lambda s: f"K{s[0]}L{s[1]}"  # noqa: E731
U, I, R = rr.U, rr.I, rr.R


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the launch-log test)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


def open_loo(em, slots):
    em.loo_begin()
    for s in slots:
        em.select(s).loo_add()


def everything(em):
    """(fitted, reliability, the four side columns) of the open session."""
    return em.loo_rows() + em.loo_sides()


def same_bits(got, want, what):
    assert len(got) == len(want)
    for n, (g, h) in enumerate(zip(got, want)):
        g, h = np.asarray(g), np.asarray(h)
        gb, hb = (xm.bits(g), xm.bits(h)) if g.dtype == np.float64 else (g, h)
        assert gb.shape == hb.shape and np.array_equal(gb, hb), f"{what}: output {n} differs in {int((gb != hb).sum())} entries"


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------
def side_bound(column, p_row, surprise):
    """TOL / P_min + 4 * 2^-52 * |surprise| per user (item), P_min over its rows of the reference's probabilities."""
    p_min = np.full(len(surprise), np.inf)
    np.minimum.at(p_min, column, p_row)
    with np.errstate(divide="ignore"):
        return TOL / p_min + 4 * 2.0 ** -52 * np.abs(surprise)


@pytest.mark.parametrize("kind", rr.KINDS)
@pytest.mark.parametrize("shape", rr.SHAPES, ids=SHAPE_ID)
def test_against_the_restatement(hip, shape, kind):
    K, L = shape
    data = rr.training_rows()
    for S, swap in ((1, 0), (3, 1)):
        params, ref = rr.model(K, L, S, kind), rr.restatement(K, L, S, kind)
        em = context(hip, data, params, U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            open_loo(em, range(S))
            assert em.get_option("loo_ms") > 0 and em.get_option("loo_sums_ms") > 0 and em.get_option("loo_rows_ms") > 0
            fitted, rel = em.loo_rows()
            sides = em.loo_sides()
            em.loo_end()
        finally:
            em.close()
        what = f"{shape} {kind} S={S} swap={swap}"
        print(f"{what}: fitted {np.abs(fitted - ref.fitted).max():.3e} reliability {np.abs(rel - ref.reliability).max():.3e} "
              f"(TOL {TOL:.0e})")
        assert np.abs(fitted - ref.fitted).max() <= TOL and np.abs(rel - ref.reliability).max() <= TOL, what
        assert (rel >= 0).all() and (fitted >= 0).all()
        want = ref.sides()
        for n, (got, col, prob) in enumerate(zip(sides, (0, 0, 1, 1), (ref.reliability, ref.fitted) * 2)):
            have = np.bincount(data[:, col], minlength=len(got)) > 0
            bound = side_bound(data[:, col], prob, want[n])
            err = np.abs(got[have] - want[n][have])
            print(f"{what}: side column {n} worst error {err.max():.3e}, worst error / bound {np.max(err / bound[have]):.3e}")
            assert (err <= bound[have]).all(), (what, n)
            assert np.isnan(got[~have]).all()
        if kind == "zero":                                  # the eps clamp: shares of 0, reliability 0, surprise -log eps
            gone = data[:, 2] == rr.ZERO_RATING
            assert (fitted[gone] == 0).all() and (rel[gone] == 0).all() and not np.signbit(rel[gone]).any(), what
            only = np.flatnonzero(np.bincount(data[gone, 1], minlength=I) == np.bincount(data[:, 1], minlength=I))
            only = only[np.bincount(data[:, 1], minlength=I)[only] > 0]             # items of that rating alone
            floor = -np.log(rr.EPS)                         # (the mean of d equal numbers, up to the sum's rounding)
            assert len(only) and (np.abs(sides[2][only] - floor) <= 4 * 2.0 ** -52 * floor).all(), what


def test_a_rating_tile_too_large_for_the_on_chip_copy(hip):
    """K = L = 40 at R = 5: 66 KB of p, past what the row kernels keep on chip -- they read the slot's own table then.
    The first 2,500 rows of the table (the restatement holds N x K x L numbers)."""
    K, L, S = 40, 40, 2
    data = rr.training_rows()[:2500]
    params = rr.model(K, L, S, "sharp")
    ref = rr.Restatement(data, params)
    for swap in (0, 1):
        em = context(hip, data, params, U, I, R, swap=swap)
        try:
            open_loo(em, range(S))
            fitted, rel = em.loo_rows()
            em.heldout_begin(data)
            for s in range(S):
                em.select(s).heldout_add()
            mean, _ = em.heldout_mean()
            em.heldout_end()
            em.loo_end()
        finally:
            em.close()
        print(f"(40, 40) swap={swap}: fitted {np.abs(fitted - ref.fitted).max():.3e} reliability "
              f"{np.abs(rel - ref.reliability).max():.3e} (TOL {TOL:.0e})")
        assert np.abs(fitted - ref.fitted).max() <= TOL and np.abs(rel - ref.reliability).max() <= TOL
        same_bits([fitted], [mean], f"(40, 40) swap={swap}: fitted against heldout")


# ---- 2. fitted is the held-out row value -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["soft", "sharp"])
@pytest.mark.parametrize("shape", rr.SHAPES, ids=SHAPE_ID)
def test_fitted_is_heldouts_row_value_bit_for_bit(hip, shape, kind):
    K, L = shape
    S = 3
    data = rr.training_rows()
    em = context(hip, data, rr.model(K, L, S, kind), U, I, R)
    try:
        em.heldout_begin(data)
        em.loo_begin()
        for s in range(S):
            em.select(s).heldout_add()
            em.select(s).loo_add()
        mean, _ = em.heldout_mean()
        fitted, _ = em.loo_rows()
        em.heldout_end()
        em.loo_end()
    finally:
        em.close()
    same_bits([fitted], [mean], f"{shape} {kind}")


# ---- 3. independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5), (20, 20), (70, 3)], ids=SHAPE_ID)
def test_a_row_depends_on_its_own_segments_and_the_added_slots_only(hip, shape):
    K, L = shape
    S = 3
    params = rr.model(K, L, S, "soft")
    data = rr.training_rows()
    n = len(data)
    subset = np.concatenate([np.flatnonzero(data[:, 0] == rr.HEAVY)[::7], [0, n - 1, 5, 5, 17], np.arange(n)[::-97]])
    em = context(hip, data, params, U, I, R)
    try:
        open_loo(em, range(S))
        full = everything(em)
        low = em.loo_lowest(5)
        same_bits(em.loo_rows(subset), [full[0][subset], full[1][subset]], f"{shape} a subset of the rows")
        same_bits(em.loo_rows(subset[:1]), [full[0][subset[:1]], full[1][subset[:1]]], f"{shape} one row")
        assert all(len(a) == 0 for a in em.loo_rows([]))
        same_bits(everything(em), full, f"{shape} a second query")
        open_loo(em, range(S))                                                       # the session again
        same_bits(everything(em), full, f"{shape} a second session")
        open_loo(em, [1])                                                            # slot 1 of the three alone
        alone = everything(em)
        em.loo_end()
    finally:
        em.close()
    em = context(hip, data, params[1:2], U, I, R)                                    # ... in a context of one slot
    try:
        open_loo(em, [0])
        same_bits(everything(em), alone, f"{shape} slot 1 alone against a one-slot context")
        em.loo_end()
    finally:
        em.close()
    em = context(hip, data, params, U, I, R, swap=1)                                 # the other side layout
    try:
        assert em.swapped
        open_loo(em, range(S))
        same_bits(everything(em), full, f"{shape} swapped")
        same_bits(em.loo_lowest(5)[:2], low[:2], f"{shape} swapped, lowest")
        em.loo_end()
    finally:
        em.close()
    extra = params + rr.model(K, L, 1, "sharp")                                      # a further slot that is not added
    em = context(hip, data, extra, U, I, R)
    try:
        open_loo(em, range(S))
        same_bits(everything(em), full, f"{shape} with a slot beyond those added")
        em.loo_end()
    finally:
        em.close()


# ---- 4. the lowest m ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5), (20, 20)], ids=SHAPE_ID)
def test_lowest_is_a_stable_sort_of_the_devices_own_column(hip, shape):
    K, L = shape
    data = rr.training_rows()
    rng = np.random.default_rng(9)
    some_users, some_items = rng.random(U) < 0.3, rng.random(I) < 0.5
    heavy = np.arange(U) == rr.HEAVY
    nobody = np.zeros(U, dtype=bool)
    for S, kind in ((1, "soft"), (3, "zero")):                                       # ("zero": 1,800 rows tie at 0.0)
        em = context(hip, data, rr.model(K, L, S, kind), U, I, R)
        try:
            open_loo(em, range(S))
            _, rel = em.loo_rows()
            for flags in ((None, None), (some_users, None), (None, some_items), (some_users, some_items), (heavy, None),
                          (nobody, None)):
                for m in (1, 5, 1024):
                    rows, vals, count = em.loo_lowest(m, *flags)
                    want = rr.lowest_of(data, rel, m, *flags)
                    what = f"{shape} {kind} m={m} flags={[None if f is None else int(f.sum()) for f in flags]}"
                    assert count == want[2] and np.array_equal(rows, want[0]), what
                    assert np.array_equal(xm.bits(vals), xm.bits(want[1])), what
            assert em.get_option("loo_ms") > 0
            rows, vals, count = em.loo_lowest(1024, heavy)                           # the planted ties, in position order
            dup = np.flatnonzero(np.diff(vals[:count]) == 0)
            assert len(dup) >= 50 and (np.diff(rows[:count])[dup] > 0).all(), (shape, kind, len(dup))
            em.loo_end()
        finally:
            em.close()


def test_lowest_of_fewer_rows_than_asked_for_is_padded(hip):
    K, L = 3, 5
    data = rr.training_rows()[:50]
    em = context(hip, data, rr.model(K, L, 1, "soft"), U, I, R)
    try:
        open_loo(em, [0])
        _, rel = em.loo_rows()
        rows, vals, count = em.loo_lowest(100)
        want = rr.lowest_of(data, rel, 100)
        assert count == 50 and np.array_equal(rows, want[0]) and np.array_equal(xm.bits(vals), xm.bits(want[1]))
        assert (rows[50:] == -1).all() and np.isposinf(vals[50:]).all()
        em.loo_end()
    finally:
        em.close()


# ---- 5. rows of degree 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3), (20, 20)], ids=SHAPE_ID)
def test_the_only_row_of_a_user_or_item_is_judged_from_the_mean_row(hip, shape):
    K, L = shape
    data = rr.training_rows()
    params = rr.model(K, L, 1, "sharp")
    theta, eta, pr = params[0]
    du, di = np.bincount(data[:, 0], minlength=U), np.bincount(data[:, 1], minlength=I)
    lone = np.flatnonzero((du[data[:, 0]] == 1) | (di[data[:, 1]] == 1))
    both = np.flatnonzero((du[data[:, 0]] == 1) & (di[data[:, 1]] == 1))
    assert len(both) == 1 and len(lone) >= 3
    em = context(hip, data, params, U, I, R)
    try:
        open_loo(em, [0])
        _, rel = em.loo_rows(lone)
        em.inform_begin()
        em.inform_add()
        tbar = em.inform_mean_theta()[0]
        em.inform_end()
        em.loo_end()
    finally:
        em.close()
    s = rr.slot_reliability(data, theta, eta, pr)
    assert np.abs(rel - s["rel"][lone]).max() <= TOL
    assert np.abs(tbar - theta.sum(axis=0) / U).max() <= TOL                         # inform_mean_theta's definition
    j = both[0]
    want = float(tbar @ pr[:, :, data[j, 2]] @ (eta.sum(axis=0) / I))                # both mean rows
    got = rel[lone.tolist().index(j)]
    print(f"{shape}: the row of degree (1, 1): {got:.6f} against theta-bar p eta-bar {want:.6f}, fitted {s['fit'][j]:.6f}")
    assert abs(got - want) <= TOL


# ---- 6. it touches nothing ---------------------------------------------------------------------------------------------------------------
def test_no_side_effects(hip):
    K, L, S = 6, 5, 3
    params = rr.model(K, L, S, "soft")
    data = rr.training_rows()
    all_users = np.arange(U, dtype=np.int32)
    ask = (np.array([3, 7], dtype=np.int32), np.array([0, 1, 3], dtype=np.int64), np.array([5, 6, 5], dtype=np.int32))
    w = np.arange(1.0, R + 1)

    def walk(with_session):
        em = context(hip, data, params, U, I, R)
        try:
            before = [tuple(a.copy() for a in em.select(s).get_params()) for s in range(S)]
            em.recommend_begin(w, True)
            em.explain_begin(w)
            for s in range(S):
                em.select(s).recommend_add()
                em.select(s).explain_add()
            first = em.recommend_query(all_users, 10) + em.explain_query(*ask, 3)
            if with_session:
                open_loo(em, range(S))
                everything(em)
                em.loo_lowest(10)
            again = em.recommend_query(all_users, 10) + em.explain_query(*ask, 3)
            if with_session:
                em.loo_end()
            em.recommend_end()
            em.explain_end()
            after = [em.select(s).get_params() for s in range(S)]
            em.iterate(2)
            moved = [em.select(s).get_params() for s in range(S)]
        finally:
            em.close()
        return before, after, first, again, moved

    before, after, first, again, moved = walk(True)
    for x, y in zip(before, after):
        same_bits(x, y, "get_params")
    same_bits(first, again, "the open recommend and explain sessions")
    plain = walk(False)[4]
    for x, y in zip(moved, plain):
        same_bits(x, y, "iterate(2) after the session")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(hip, code, fn, *args, **kw):
    with pytest.raises(hip._lib.HipLibraryError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.message)


def test_refusals_by_status_code(hip):
    K, L = 4, 3
    params = rr.model(K, L, 1, "soft")
    data = rr.training_rows()
    lib = hip._lib
    em = hip.HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, slots=2)
    try:
        em.select(0).set_params(*params[0])                                      # slot 1 holds no parameters
        for call in (em.loo_add, em.loo_rows, em.loo_sides, lambda: em.loo_lowest(3)):
            refused(hip, lib.E_INVALID, call)                                    # no session
        em.loo_begin()
        for call in (em.loo_rows, em.loo_sides, lambda: em.loo_lowest(3)):
            refused(hip, lib.E_INVALID, call)                                    # nothing added
        refused(hip, lib.E_INVALID, em.select(1).loo_add)                        # a slot without parameters
        em.select(0).loo_add()
        want = everything(em)
        for bad in (0, -2, hip.HipEM.MAX_LOO_M + 1):
            refused(hip, lib.E_INVALID, em.loo_lowest, bad)
        for bad in (-1, len(data)):
            refused(hip, lib.E_INVALID, em.loo_rows, [3, bad])
        with pytest.raises(ValueError):
            em.loo_lowest(3, np.ones(U + 1, dtype=bool))
        same_bits(everything(em), want, "the session is still usable")
        em.loo_end()
        refused(hip, lib.E_INVALID, em.loo_rows)
    finally:
        em.close()
    wide = hip.HipEM(data[:50], 1025, 1, n_users=U, n_items=I, n_ratings=R)     # MMSBM_HIP_FOLD_IN_MAX_K + 1 user groups
    try:
        refused(hip, lib.E_UNSUPPORTED, wide.loo_begin)
    finally:
        wide.close()


# ---- 8. the launch log ---------------------------------------------------------------------------------------------------------------------
def test_every_loo_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("loo_")]
    assert sorted(compiled) == sorted(NEW_KERNELS), compiled
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))


# ---- 9. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_the_four_methods_on_a_fitted_model(hip):
    import pandas as pd
    rng = np.random.default_rng(4)
    n_u, n_i, n = 40, 30, 900
    group_u, group_i = rng.integers(0, 2, n_u), rng.integers(0, 2, n_i)
    us, its = rng.integers(0, n_u, n), rng.integers(0, n_i, n)
    agree = group_u[us] == group_i[its]
    stars = np.where(agree, rng.integers(4, 6, n), rng.integers(1, 3, n))            # two planted blocks
    wrong = rng.choice(n, 12, replace=False)
    stars[wrong] = np.where(agree[wrong], 1, 5)                                       # twelve mistyped ratings
    df = pd.DataFrame({"users": [f"u{x}" for x in us], "items": [f"film-{x}" for x in its], "ratings": stars})
    m = hip.MMSBM(2, 2, iterations=60, sampling=2, seed=11)
    m.fit(df, silent=True)
    table = m.rating_reliability()
    assert list(table.columns) == ["users", "items", "rating", "fitted", "reliability", "surprise"] and len(table) == n
    assert table["users"].tolist() == df["users"].tolist() and table["items"].tolist() == df["items"].tolist()
    assert table["rating"].astype(str).tolist() == df["ratings"].astype(str).tolist()
    assert all(table[c].dtype == np.float64 for c in ("fitted", "reliability", "surprise"))
    assert ((table["reliability"] >= 0) & (table["reliability"] <= 1 + TOL)).all()
    np.testing.assert_array_equal(table["surprise"].to_numpy(),
                                  -np.log(np.maximum(table["reliability"].to_numpy(), rr.EPS)))
    order = np.argsort(table["reliability"].to_numpy(), kind="stable")
    for top in (1, 20):
        worst = m.spurious_ratings(top)
        assert list(worst.columns) == list(table.columns) + ["rank"] and worst["rank"].tolist() == list(range(1, top + 1))
        head = table.iloc[order[:top]].reset_index(drop=True)
        for col in table.columns:
            if head[col].dtype == np.float64:
                assert np.array_equal(xm.bits(worst[col].to_numpy()), xm.bits(head[col].to_numpy())), col
            else:
                assert worst[col].tolist() == head[col].tolist(), col
    found = set(order[:40].tolist()) & set(wrong.tolist())
    print(f"mistyped ratings among the 40 least reliable of {n}: {len(found)} of {len(wrong)}")
    assert len(found) >= 6                                                            # (chance: 0.5 of 12)
    one = m.rating_reliability([(df["users"][3], df["items"][3])])
    assert len(one) >= 1 and (one["users"] == df["users"][3]).all() and (one["items"] == df["items"][3]).all()
    mine = m.spurious_ratings(5, users=[df["users"][0]])
    assert (mine["users"] == df["users"][0]).all() and len(mine) == min(5, (df["users"] == df["users"][0]).sum())
    for side, frame in (("users", m.misfit_users(min_ratings=1)), ("items", m.misfit_items(min_ratings=1))):
        assert list(frame.columns) == [side, "ratings", "surprise", "fitted_surprise"]
        degree = df[side].value_counts()
        assert len(frame) == len(degree) and frame["ratings"].tolist() == [degree[x] for x in frame[side]]
        assert (np.diff(frame["surprise"].to_numpy()) <= 0).all() and frame["ratings"].dtype == np.int64
    assert len(m.misfit_users(m=3)) == 3
