"""The kernels that run AFTER the fit on the parameters a long run ends in (staged_params.py): the likelihood in every
device form, the held-out log-likelihood, the predict sums and the serving scores.

test_gpu_staged.py holds the M-step to the oracle on late, border, row-border, tiny, dead-group and subnormal starts;
everything behind the fit -- which by construction only ever sees such models -- used to be tested on rng.random
parameters or on a narrow slice of late ones.  Here:

  1. every likelihood form (lik_lane_kernel, lik_wave_kernel<1|2|3>, likelihood_fast_kernel at 1, 2, 4 and 8 lanes per
     triple, likelihood_units_kernel, likelihood_kernel; each asserted from the launch log) x every family x both side
     layouts: against the oracle at 1e-12 on the staged start, at 1e-11 after three device iterations (two-launch and
     four-launch form), finite and repeatable bit for bit; where the expected value is exactly 0.0 (`tiny`) within the
     bound derived in staged_after_fit.zero_likelihood_bound; restart slots holding another family each;
  2. heldout_* within the bounds of test_gpu_heldout.py and the predict sums by equality with the host formulas on the
     device's own prod_dist matrix, users with all-zero rows among them;
  3. the serving scores ELEMENT-WISE against an np.longdouble evaluation within score_bound (a sum of non-negative terms
     keeps a relative bound whatever the magnitudes: tau = 1e-12 max|row| sees nothing of a row that spans ten decades),
     zeroed rows and columns +0.0 by their bits, and every selection -- recommend_query, recommend_positions,
     recommend_top_pairs, similar_query -- against the lexsort of the device's OWN full rows, with no tolerance band.

The inputs are pinned, and every reference shown to sit inside its bar by itself, in test_staged_after_fit_cpu.py.
Each test records its worst error; the tables are printed when the module is done (-s shows them).
"""
import collections

import numpy as np
import pytest

import exact_models as xm
import staged_after_fit as saf
from conftest import ELEMENT_FLOOR
from oracle import mmsbm_oracle as orc
from staged_params import FAMILIES
from test_gpu_instantiations import LaunchWindow, hip  # noqa: F401  (hip: the fixture)
from test_gpu_recommend import context
from test_gpu_serving_exact import same_answer
from test_gpu_similar import MASS_BLOCK, tolerance
from test_gpu_staged import ran
from test_heldout_cpu import ll_bound, restate_heldout
from test_ranking_cpu import restate_positions
from test_recommend_cpu import restate, seen_items
from test_similar_cpu import SIDES, restate_distances, top_similar
from test_top_pairs_cpu import restate_top_pairs

pytestmark = pytest.mark.gpu

WORST = collections.defaultdict(float)     # (row, column, kind) -> worst figure seen
WINDOW = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    WINDOW["lw"] = LaunchWindow().__enter__()      # the launch log from the first test of this file on (read by the last one)
    yield
    for title, kinds in (("likelihood, relative error: staged start / after three iterations", ("start", "loop")),
                         ("likelihood where the expected value is 0.0, |value| / derived bound: start / after three iterations",
                          ("start / bound", "loop / bound")),
                         ("held-out log-likelihood, |delta| / ll_bound: slots / mean", ("ll / bound", "mean ll / bound")),
                         ("held-out mean_p, relative error / ((K L + 4) 2^-52)", ("mean_p / bound",)),
                         ("serving scores, element-wise relative error / score_bound: rating values / last rating one-hot",
                          ("values", "last")),
                         ("similar_query, |delta| / tolerance: items / users", ("items", "users"))):
        rows = sorted({k[0] for k in WORST if k[2] in kinds})
        if not rows:
            continue
        print("\n" + title)
        print(f"{'':30s}" + "".join(f"{s:>20s}" for s in FAMILIES))
        for row in rows:
            cells = (" / ".join(f"{WORST[row, s, kind]:.1e}" if (row, s, kind) in WORST else "-" for kind in kinds) for s in FAMILIES)
            print(f"{row:30s}" + "".join(f"{c:>20s}" for c in cells))


def record(row, stage, kind, figure):
    WORST[row, stage, kind] = max(WORST[row, stage, kind], figure)


def bits(a):
    return xm.bits(a)


# ---- 1. the likelihood: every form x every family ---------------------------------------------------------------------
def check_every_form(em, forms, want, rtol, cell, stage, kind, what):
    """em.likelihood() under every (lik_fast, lik_g) of `forms`: finite, the same bits on a second call, within the bar
    of `want`.  Leaves the options at their defaults."""
    ref = cell.ref
    n_obs = len(ref.data)
    zero_bound = saf.zero_likelihood_bound(n_obs, ref.k, ref.l)
    seen = []
    for (fast, g), kernel in forms.items():
        em.set_option("lik_fast", fast)
        em.set_option("lik_g", g)
        got = float(em.likelihood())
        assert np.isfinite(got), (what, kernel)
        assert bits(em.likelihood()) == bits(got), (what, kernel, "a second call")
        err = abs(got - want) / abs(want) if want != 0.0 else abs(got) / zero_bound
        record(kernel.split("<")[0], stage, kind if want != 0.0 else kind + " / bound", err)
        seen.append((kernel, got, err))
    print(f"{what} {stage} {kind}, expected {want!r}, {'relative error' if want != 0.0 else '|value| / bound'}: "
          + ", ".join(f"{kernel} {err:.1e}" for kernel, _, err in seen))
    for kernel, got, _ in seen:
        assert saf.lik_close(got, want, rtol, n_obs, ref.k, ref.l), (what, kind, kernel, got, want)
    em.set_option("lik_g", 0)
    em.set_option("lik_fast", 2)


def loop_modes(hip, em):
    """(1, 0) where the shape and the data allow the two-launch iteration, else (0,)."""
    try:
        em.set_option("fused", 1)
    except hip._lib.HipLibraryError:
        return (0,)
    assert em.get_option("launches") == 2.0
    return (1, 0)


@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("k,l", saf.LIK_SHAPES, ids=[f"{k}x{l}" for k, l in saf.LIK_SHAPES])
def test_likelihood_every_form_on_every_family(hip, k, l, stage):
    cell = saf.lik_cell(k, l, stage)
    ref = cell.ref
    if stage == "tiny":
        assert cell.want_start == 0.0 and cell.want_loop == 0.0      # every omega and every s_n below eps: eps (log eps - log eps)
    for swap in (0, 1):
        forms = saf.lik_forms(k, l, swap)
        what = f"K={k} L={l} swap={swap}"
        with LaunchWindow() as lw:
            with hip.HipEM(ref.data, k, l, *ref.dims, swap_sides=swap) as em:
                assert em.get_option("lik_fast") == 2.0 and em.get_option("lik_g") == 0.0
                em.set_params(*ref.start)
                check_every_form(em, forms, cell.want_start, saf.TOL_LIK, cell, stage, "start", what)
                for fused in loop_modes(hip, em):
                    # s_n comes from the iteration's own A table; the two-launch form leaves it stale (ensure_a)
                    em.set_option("fused", fused)
                    assert em.get_option("launches") == (2.0 if fused else 4.0)
                    em.set_params(*ref.start)
                    em.iterate(3)
                    check_every_form(em, forms, cell.want_loop, saf.TOL_LIK_LOOP, cell, stage, "loop", f"{what} fused={fused}")
            launched = lw.names()
        missing = sorted(set(forms.values()) - launched)
        assert not missing, (what, missing, sorted(n for n in launched if n.startswith("lik")))


@pytest.mark.parametrize("k,l,kernel", [(20, 20, "lik_lane_kernel"), (50, 50, "lik_wave_kernel")])
def test_likelihood_of_slots_holding_different_families(hip, k, l, kernel):
    """A clamp, a -inf table entry or a refilled table belongs to its slot: each slot's value is bitwise that of a
    one-slot context with the same parameters (and the oracle's at 1e-12)."""
    stages = ("init", "rowborder", "dead")
    cells = [saf.lik_cell(k, l, s) for s in stages]
    ref = cells[0].ref
    with LaunchWindow() as lw:
        with hip.HipEM(ref.data, k, l, *ref.dims, swap_sides=0, slots=3) as em:
            for s, c in enumerate(cells):
                em.select(s).set_params(*c.ref.start)
            got = [float(em.select(s).likelihood()) for s in (0, 1, 2)]
            back = [float(em.select(s).likelihood()) for s in (2, 1, 0)][::-1]
        for s, c in enumerate(cells):
            with hip.HipEM(ref.data, k, l, *ref.dims, swap_sides=0) as one:
                one.set_params(*c.ref.start)
                alone = float(one.likelihood())
            assert bits(got[s]) == bits(alone) == bits(back[s]), (stages[s], got[s], alone, back[s])
            assert saf.lik_close(got[s], c.want_start, saf.TOL_LIK, len(ref.data), k, l), (stages[s], got[s], c.want_start)
        ran(lw.names(), kernel)


# ---- 2. held-out log-likelihood and predict sums ----------------------------------------------------------------------
@pytest.mark.parametrize("family", saf.HELDOUT_FAMILIES)
@pytest.mark.parametrize("k,l", saf.HELDOUT_SHAPES, ids=[f"{k}x{l}" for k, l in saf.HELDOUT_SHAPES])
def test_heldout_on_staged_models(hip, k, l, family):
    data, dims, params, rows = saf.heldout_case(k, l, family)
    want = restate_heldout(params, rows)
    clamped = float(np.mean(want["p"][0] < saf.EPS))
    if family == "rowborder":
        assert 0.05 <= clamped <= 0.95, clamped
    if family == "tiny":
        assert clamped == 1.0
    for swap in (0, 1):
        em = context(hip, data, params, *dims, swap=swap)
        try:
            em.heldout_begin(rows)
            ev = em.heldout_eval()
            adds = [em.select(s).heldout_add() for s in range(2)]
            mean_p, mean_ll = em.heldout_mean()
            em.heldout_end()
        finally:
            em.close()
        for s in range(2):
            bound = ll_bound(k, l, want["p"][s])
            record(f"K={k} L={l}", family, "ll / bound", abs(ev[s] - want["ll"][s]) / bound)
            print(f"held-out K={k} L={l} {family} swap={swap} slot {s}: |delta| = {abs(ev[s] - want['ll'][s]):.3e}, bound {bound:.3e}")
            assert np.isfinite(ev[s]) and abs(ev[s] - want["ll"][s]) <= bound
            assert bits(adds[s]) == bits(ev[s])
        rtol = (k * l + 4) * 2.0 ** -52
        nz = want["mean_p"] != 0
        record(f"K={k} L={l}", family, "mean_p / bound", float(np.max(np.abs(mean_p[nz] - want["mean_p"][nz]) / want["mean_p"][nz])) / rtol)
        assert np.allclose(mean_p, want["mean_p"], rtol=rtol, atol=0)
        bound = ll_bound(k, l, want["mean_p"])
        record(f"K={k} L={l}", family, "mean ll / bound", abs(mean_ll - want["mean_ll"]) / bound)
        assert abs(mean_ll - want["mean_ll"]) <= bound


@pytest.mark.parametrize("family", saf.PREDICT_FAMILIES)
@pytest.mark.parametrize("k,l", saf.PREDICT_SHAPES, ids=[f"{k}x{l}" for k, l in saf.PREDICT_SHAPES])
def test_predict_sums_on_staged_models(hip, k, l, family):
    data, dims, params, test, zero_users = saf.predict_case(k, l, family)
    n_r = dims[2]
    weights = np.arange(n_r, dtype=np.float64)       # the reference's self.ratings (rating indices)
    zero_rows = np.isin(test[:, 0], zero_users)
    assert 2 <= zero_rows.sum() < len(test) // 10
    for swap in (0, 1):
        with hip.HipEM(data, k, l, *dims, slots=2, swap_sides=swap) as em:
            for s in range(2):
                em.select(s).set_params(*params[s])
            for fast in (0, 1):
                em.set_option("predict_fast", fast)
                assert em.get_option("predict_fast") == float(fast)
                rats = [em.select(s).prod_dist(test) for s in range(2)]
                em.predict_begin(test, weights)
                per = [em.select(s).predict_add() for s in range(2)]
                mean, raw = em.predict_finish()
                what = f"K={k} L={l} {family} swap={swap} predict_fast={fast}"
                assert np.array_equal(bits(mean), bits(np.array(rats).mean(axis=0))), what
                for rat, st in list(zip(rats, per)) + [(mean, raw)]:
                    assert np.all(np.isfinite(rat)) and (rat >= 0).all(), what
                    assert (bits(rat[zero_rows]) == 0).all(), what            # the zeroed users: +0.0 in every rating
                    if family == "tiny":                                      # ... and about 1e-220 is not zero
                        assert (rat[~zero_rows].max(axis=1) > ELEMENT_FLOOR).all() and rat.max() < 1e-200, what
                        assert st[0] == len(test) - zero_rows.sum(), what
                    want = orc.score_stats(rat, test[:, 2], list(range(n_r)))
                    got = hip.HipEM.final_stats(st)
                    assert st[0] == (rat.sum(1) != 0).sum(), what
                    for key in ("accuracy", "one_off_accuracy", "mae"):
                        assert got[key] == want[key], (what, key)
                    assert got["s2"] == want["s2"], what
                    assert abs(got["s2pond"] - want["s2pond"]) <= 1e-12 * want["s2pond"], what


# ---- 3. serving scores, element-wise; the order from the device's own scores ------------------------------------------
def csr(lists):
    return (np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64),
            np.concatenate([np.asarray(x, dtype=np.int32) for x in lists]) if lists else np.zeros(0, np.int32))


def full_rows(em, case, n_u, n_i):
    """(U, I) scores of the open session (nothing excluded) as the device returns them.  A query returns at most 1,024
    items of a row: longer rows are read in pages through recommend_query_theta with the slots' own theta rows, each
    page leaving out what the pages before it returned -- after asserting that its first page is recommend_query's."""
    users = np.arange(n_u, dtype=np.int32)
    dev = np.full((n_u, n_i), np.nan)
    if n_i <= saf.MAX_QUERY:
        items, scores, counts = em.recommend_query(users, n_i)
        assert (counts == n_i).all()
        pages = [(items, scores)]
    else:
        theta = np.stack([p[0] for p in case.params])
        pages, taken = [], [np.zeros(0, dtype=np.int32) for _ in range(n_u)]
        while len(taken[0]) < n_i:
            n = min(saf.MAX_QUERY, n_i - len(taken[0]))
            items, scores, counts = em.recommend_query_theta(theta, n, csr([np.sort(t) for t in taken]) if pages else None)
            assert (counts == n).all()
            if not pages:
                same_answer((items, scores, counts), em.recommend_query(users, n), "first page against recommend_query")
            pages.append((items, scores))
            taken = [np.concatenate([t, row]) for t, row in zip(taken, items)]
    for items, scores in pages:
        np.put_along_axis(dev, items.astype(np.int64), scores, axis=1)
    assert not np.isnan(dev).any()                    # every item of every row exactly once
    return dev


@pytest.mark.parametrize("family", saf.SERVE_FAMILIES)
@pytest.mark.parametrize("case", saf.SERVE_CASES, ids=saf.SERVE_IDS)
def test_serving_scores_and_order_on_staged_models(hip, case, family):
    k, l, swap, n_u, n_i = case
    sc = saf.serve_case(k, l, n_u, n_i, family)
    users = np.arange(n_u, dtype=np.int32)
    seen = seen_items(sc.data, n_u)
    bound = saf.score_bound(k, l, saf.SERVE_R, saf.SERVE_S)
    assert hip.HipEM.MAX_RECOMMEND == hip.HipEM.MAX_TOP_PAIRS == saf.MAX_QUERY
    if n_i > saf.MAX_QUERY:                           # the items of a row are split across waves and merged
        cus = hip._lib.device_identity(0)["compute_units"]
        parts, per = xm.select_split(n_i, n_u, cus)
        assert parts > 1 and sc.zero_items[0] // per != sc.zero_items[1] // per, (parts, per)
    rng = np.random.default_rng([k, l, n_u])
    held_users = np.unique(rng.integers(0, n_u, 300))
    held = [rng.integers(0, n_i, c) for c in np.bincount(rng.integers(0, len(held_users), 300), minlength=len(held_users))]
    for u, it in zip(held_users[:5], held):           # some of them the user's own training items
        if len(it) and seen[u]:
            it[0] = sorted(seen[u])[0]
    offsets, held_items = csr(held)
    em = context(hip, sc.data, sc.params, *sc.dims, swap=swap)
    try:
        for wname, w in saf.SERVE_WEIGHTS.items():
            what = f"{saf.SERVE_IDS[saf.SERVE_CASES.index(case)]} {family} weights={wname}"
            dev = None
            for exclude in (False, True):
                em.recommend_begin(w, exclude)
                for s in range(saf.SERVE_S):
                    em.select(s).recommend_add()
                if dev is None:
                    dev = full_rows(em, sc, n_u, n_i)
                    # -- the values, element-wise
                    exact = saf.longdouble_scores(sc.params, w)
                    frac, small_ok = saf.score_errors(dev, exact, bound, ELEMENT_FLOOR)
                    record(f"K={k} L={l} I={n_i}", family, wname, frac)
                    print(f"{what}: worst element-wise error {frac:.3f} of the bound {bound:.2e}; scores span "
                          f"{dev[dev > 0].min():.1e} .. {dev.max():.1e}")
                    assert small_ok and frac <= 1.0, (what, frac)
                    assert (bits(dev[list(sc.zero_users)]) == 0).all() and (bits(dev[:, list(sc.zero_items)]) == 0).all(), what
                # -- the order: every selection against the lexsort of the device's own full rows
                for n in (1, 10, min(n_i - 1, saf.MAX_QUERY)):
                    want = restate(None, users, n_i, w, n, seen if exclude else None, scores=dev)
                    same_answer(em.recommend_query(users, n), want, f"{what} exclude={exclude} n={n}")
                pos, cand = em.recommend_positions(held_users, offsets, held_items)
                want_pos, want_cand = restate_positions(dev[held_users], offsets, held_items, held_users, seen if exclude else None)
                assert np.array_equal(pos, want_pos) and np.array_equal(cand, want_cand), f"{what} exclude={exclude} positions"
                for m in (1, 100, saf.MAX_QUERY):
                    gu, gi, gs, count = em.recommend_top_pairs(m)
                    wu, wi, ws, wcount = restate_top_pairs(None, None, users, m, seen if exclude else None, scores=dev)
                    assert count == wcount and np.array_equal(gu, wu) and np.array_equal(gi, wi), f"{what} exclude={exclude} m={m}"
                    assert np.array_equal(bits(gs), bits(ws)), f"{what} exclude={exclude} m={m} scores"
                em.recommend_end()
    finally:
        em.close()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("family", ["late", "rowborder", "dead"])
@pytest.mark.parametrize("k,l", [(20, 20), (7, 33)])
def test_similar_on_staged_models(hip, k, l, family, side):
    """Distances within test_gpu_similar.tolerance of the restatement; the order against the lexsort of the device's own
    full distance rows (n = rows - 1), which needs no gap between neighbours."""
    n_u, n_i = 120, 300
    sc = saf.serve_case(k, l, n_u, n_i, family)
    n_r, n_s = saf.SERVE_R, saf.SERVE_S
    rows, others = (n_i, n_u) if side == "items" else (n_u, n_i)
    summed, groups = (l, k) if side == "items" else (k, l)
    c_m = -(-others // MASS_BLOCK) + 8
    ids = np.arange(rows, dtype=np.int32)
    ref = restate_distances(sc.params, side, ids)
    tol = tolerance(ref, summed, n_r, n_s * groups * n_r, c_m)
    em = context(hip, sc.data, sc.params, *sc.dims)
    try:
        em.similar_begin(side)
        for s in range(n_s):
            em.select(s).similar_add()
        got = {n: em.similar_query(ids, n) for n in (1, 10, rows - 1)}
        em.similar_end()
    finally:
        em.close()
    out, dist, counts = got[rows - 1]
    assert (counts == rows - 1).all()
    dev = np.full((rows, rows), np.nan)
    np.put_along_axis(dev, out.astype(np.int64), dist, axis=1)
    off = ~np.eye(rows, dtype=bool)
    assert np.isnan(dev[~off]).all() and not np.isnan(dev[off]).any()      # every other row exactly once
    assert (dev[off] >= 0.0).all()
    err = np.abs(dev - ref)[off]
    exact = tol[off] == 0
    assert (err[exact] == 0).all()                   # identical rows (the zeroed ones): distance exactly 0
    worst = float(np.max(err[~exact] / tol[off][~exact]))
    record(f"K={k} L={l}", family, side, worst)
    print(f"similar K={k} L={l} {family} {side}: largest error / tolerance {worst:.3f}")
    assert worst <= 1.0
    np.fill_diagonal(dev, 0.0)
    for n, answer in got.items():
        same_answer(answer, top_similar(dev, ids, n), f"K={k} L={l} {family} {side} n={n}")


# ---- the forms this file is about were launched by it -----------------------------------------------------------------
def test_every_likelihood_form_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    for kernel in ("lik_lane_kernel<", "lik_wave_kernel<1>", "lik_wave_kernel<2>", "lik_wave_kernel<3>",
                   "likelihood_units_kernel", "likelihood_kernel"):
        assert any(n == kernel or (kernel.endswith("<") and n.startswith(kernel)) for n in names), (kernel, sorted(names))
    lanes = {n.split(",")[1] for n in names if n.startswith("likelihood_fast_kernel<")}
    assert {"1", "2", "4", "8"} <= lanes, sorted(names)
