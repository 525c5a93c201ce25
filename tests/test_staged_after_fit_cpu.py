"""The inputs of test_gpu_staged_after_fit.py are what they claim to be, and every reference sits inside its bar alone.

With the GPU module's own shapes and seeds (staged_after_fit.py): the `rowborder` cells of the likelihood have both
outcomes of `log(max(s, eps))` in one launch, the `dead` cells have rows of omega that are clamped throughout (what the
wave kernel's dead-row skip keys on), the chosen shapes select every likelihood form, the dense oracle's likelihood
agrees with an np.longdouble evaluation three decades inside the 1e-12 the device is held to, the fp64 restatement of
the serving scores stays within the derived element-wise bound of the np.longdouble scores, and the held-out rows of
`rowborder` straddle eps.  Conditions on the inputs and the references: one that fails gets other inputs, never another bar.
"""
import numpy as np
import pytest

import staged_after_fit as saf
from conftest import ELEMENT_FLOOR
from staged_params import FAMILIES
from test_heldout_cpu import restate_p
from test_recommend_cpu import restate_scores

LIK_IDS = [f"{k}x{l}" for k, l in saf.LIK_SHAPES]
AGREE = 1e-13


# ---- the likelihood cells --------------------------------------------------------------------------------------------
def test_the_shapes_select_every_likelihood_form():
    kernels = {name for k, l in saf.LIK_SHAPES for swap in (0, 1) for name in saf.lik_forms(k, l, swap).values()}
    assert {"likelihood_units_kernel", "likelihood_kernel", "lik_wave_kernel<1>", "lik_wave_kernel<2>", "lik_wave_kernel<3>"} <= kernels
    assert {f"lik_lane_kernel<{kp},128>" for kp in (4, 8, 20, 32)} <= kernels
    lanes = {n.split(",")[1] for n in kernels if n.startswith("likelihood_fast_kernel<")}
    assert lanes == {"1", "2", "4", "8"}
    for k, l, swap, default, slow in ((20, 20, 0, "lik_lane_kernel<20,128>", "likelihood_units_kernel"),
                                      (50, 50, 1, "lik_wave_kernel<1>", "likelihood_units_kernel"),
                                      (70, 7, 1, "lik_wave_kernel<2>", "likelihood_units_kernel"),
                                      (12, 150, 0, "lik_wave_kernel<3>", "likelihood_kernel"),
                                      (5, 200, 0, "likelihood_kernel", "likelihood_kernel")):
        forms = saf.lik_forms(k, l, swap)
        assert forms[2, 0] == default and forms[0, 0] == slow, (k, l, swap, forms)
    assert saf.lik_forms(6, 88, 0)[1, 0] == "likelihood_fast_kernel<12,8,true>"     # test_gpu_instantiations.py's case


@pytest.mark.parametrize("k,l", saf.LIK_SHAPES, ids=LIK_IDS)
def test_rowborder_cells_hold_both_outcomes_of_the_row_clamp(k, l):
    ref = saf.lik_cell(k, l, "rowborder").ref
    assert 2 * len(ref.data) >= 5 * ref.dims[2] * max(ref.dims[0], ref.dims[1])     # lik_pairs_usable: a few triples per pair
    for params in (ref.start,):
        s = saf.row_sums(ref.data, *params)
        below = float(np.mean(s < saf.EPS))
        near = float(np.mean((s >= saf.EPS / 10) & (s < saf.EPS * 10)))
        assert 0.05 <= below <= 0.5, below
        assert near >= 0.05, near
        assert np.mean((s >= saf.EPS / 10) & (s < saf.EPS)) > 0 and np.mean((s >= saf.EPS) & (s < saf.EPS * 10)) > 0


@pytest.mark.parametrize("k,l", saf.LIK_SHAPES, ids=LIK_IDS)
def test_dead_cells_hold_rows_that_are_clamped_throughout(k, l):
    ref = saf.lik_cell(k, l, "dead").ref
    assert saf.dead_rows(ref.data, *ref.start) >= 1
    assert np.mean(saf.row_sums(ref.data, *ref.start) < saf.EPS) < 0.01           # ... in triples whose s_n is not clamped


@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("k,l", saf.LIK_SHAPES, ids=LIK_IDS)
def test_the_oracle_likelihood_agrees_with_long_double(k, l, stage):
    cell = saf.lik_cell(k, l, stage)
    ref = cell.ref
    for want, params, what in ((cell.want_start, ref.start, "start"), (cell.want_loop, ref.want_loop, "after three steps")):
        exact = saf.longdouble_likelihood(ref.data, *params)
        assert np.isfinite(want)
        if stage == "tiny":
            assert want == 0.0 and exact == 0.0, (what, want, exact)
        else:
            assert want < 0.0 and abs(want - exact) <= AGREE * abs(exact), (what, want, exact)


def test_the_zero_likelihood_bound_is_far_below_any_likelihood_of_the_cells():
    smallest = min(abs(saf.lik_cell(k, l, s).want_start) for k, l in [(3, 5), (20, 20)] for s in FAMILIES if s != "tiny")
    assert saf.zero_likelihood_bound(3000, 12, 150) < 1e-12 * smallest


# ---- held-out rows and predict rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k,l", saf.HELDOUT_SHAPES)
def test_heldout_rows_of_rowborder_straddle_eps_and_tiny_clamps_every_row(k, l):
    data, dims, params, rows = saf.heldout_case(k, l, "rowborder")
    assert len(rows) == saf.HELDOUT_ROWS and len(params) == 2
    clamped = float(np.mean(restate_p(params[0], rows) < saf.EPS))
    assert 0.05 <= clamped <= 0.95, clamped
    assert np.mean(restate_p(params[1], rows) < saf.EPS) == 0.0                   # the init slot next to it: nothing clamped
    data, dims, params, rows = saf.heldout_case(k, l, "tiny")
    assert np.mean(restate_p(params[0], rows) < saf.EPS) == 1.0
    data, dims, params, rows = saf.heldout_case(k, l, "dead")
    assert (restate_p(params[0], rows) > 0).all()


@pytest.mark.parametrize("family", saf.PREDICT_FAMILIES)
@pytest.mark.parametrize("k,l", saf.PREDICT_SHAPES)
def test_predict_rows_meet_the_zeroed_users_and_the_slots_differ(k, l, family):
    data, dims, params, test, zero_users = saf.predict_case(k, l, family)
    zero_rows = np.isin(test[:, 0], zero_users)
    assert 2 <= zero_rows.sum() < len(test) // 10
    for theta, eta, pr in params:
        assert not theta[list(zero_users)].any() and theta.any(axis=1).sum() == dims[0] - len(set(zero_users))
    assert not np.array_equal(params[0][0], params[1][0]) and not np.array_equal(params[0][1], params[1][1])


# ---- the serving scores -----------------------------------------------------------------------------------------------
SERVE_SHAPES = sorted({(c[0], c[1], c[3], c[4]) for c in saf.SERVE_CASES})


@pytest.mark.parametrize("family", saf.SERVE_FAMILIES)
@pytest.mark.parametrize("k,l,n_u,n_i", SERVE_SHAPES)
def test_the_fp64_restatement_stays_within_the_score_bound_of_long_double(k, l, n_u, n_i, family):
    sc = saf.serve_case(k, l, n_u, n_i, family)
    bound = saf.score_bound(k, l, saf.SERVE_R, saf.SERVE_S)
    assert len(sc.params) == saf.SERVE_S and not np.array_equal(sc.params[0][0], sc.params[1][0])
    for name, w in saf.SERVE_WEIGHTS.items():
        assert (w >= 0).all()
        exact = saf.longdouble_scores(sc.params, w)
        fp64 = restate_scores(sc.params, np.arange(n_u), n_i, w)
        frac, small_ok = saf.score_errors(fp64, exact, bound, ELEMENT_FLOOR)
        assert small_ok and frac <= 0.5, (name, frac)                             # the reference alone: half the bound at most
        assert not exact[list(sc.zero_users)].any() and not exact[:, list(sc.zero_items)].any()
        assert (exact >= 0).all() and np.mean(exact > ELEMENT_FLOOR) > 0.5
        if family == "tiny":
            assert ELEMENT_FLOOR < exact[exact > 0].min() and exact.max() < 1e-200
        if family == "rowborder":                                                  # what tau = 1e-12 max|row| cannot see
            live = np.delete(np.delete(exact, list(sc.zero_users), axis=0), list(sc.zero_items), axis=1).astype(np.float64)
            assert np.max(np.log10(live.max(axis=1) / live.min(axis=1))) >= 8.0
