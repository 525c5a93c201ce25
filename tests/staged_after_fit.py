"""Shapes, seeds, models and long-double references of the kernels that run AFTER the fit, on the late-stage parameters
of staged_params.py -- shared by test_gpu_staged_after_fit.py (the device) and test_staged_after_fit_cpu.py (which pins
these inputs and shows that every reference alone sits inside the bar the device is held to).  A plain module.

The likelihood cells reuse test_gpu_staged.reference(): the "uniform" data of a (K, L) cell, the staged start and the
oracle's parameters after three iterations, computed once and never changed.
"""
import collections

import numpy as np

from oracle import mmsbm_oracle as orc
from staged_params import staged, uniform_rows
from test_gpu_staged import reference

EPS = orc.EPS
U53 = 2.0 ** -53
LD = np.longdouble

TOL_LIK = 1e-12          # likelihood of given parameters against the oracle (the existing likelihood tests)
TOL_LIK_LOOP = 1e-11     # ... of the parameters three device iterations end in, against the oracle's three em_steps


# ---- the likelihood: which device form a shape selects (tu_once.hip, restated) -----------------------------------------
LIK_SHAPES = [(3, 5), (20, 20), (30, 32), (50, 50), (7, 70), (70, 7), (12, 150), (5, 200)]
LIK_G = (0, 1, 2, 4, 8)
LDS_MAX, SCALAR_TILE, LIK_THREADS = 160 * 1024, 8 * 1024, 128


def pad_dim(d):
    assert d <= 256
    return (d + 3) // 4 * 4


def lik_forms(k, l, swap):
    """{(lik_fast, lik_g): kernel name} for a context of K x L groups: the internal row widths are (lp, kp) =
    (padded side paired with the rating, padded other side); swap_sides = 1 pairs the users with the rating."""
    kp, lp = (pad_dim(l), pad_dim(k)) if swap else (pad_dim(k), pad_dim(l))

    def slow():
        return "likelihood_units_kernel" if (kp + lp) * LIK_THREADS * 8 <= LDS_MAX - 2048 else "likelihood_kernel"

    def table(g):
        tile_lds = lp > 20 or g > 1 or 2 * kp * lp * 8 > SCALAR_TILE
        if lp > 160 or (2 * kp * lp * 8 if tile_lds else 0) > LDS_MAX - 4096:
            return slow()
        lanes = g if g else (1 if lp <= 20 else 2 if lp <= 40 else 4)
        while lanes < 8 and -(-lp // lanes) > 20:
            lanes *= 2
        lw = (-(-lp // lanes) + 3) // 4 * 4
        return f"likelihood_fast_kernel<{lw if lw in (4, 8, 12, 16) else 20},{lanes},{'true' if tile_lds else 'false'}>"

    def default(g):
        if 32 < lp <= 192 and kp <= 192 and (2 * kp * lp + kp) * 8 <= LDS_MAX - 4096:
            return f"lik_wave_kernel<{1 if lp <= 64 else 2 if lp <= 128 else 3}>"
        if kp <= 32 and lp <= 32:
            return f"lik_lane_kernel<{kp},128>"
        return table(g)

    forms = {(0, 0): slow()}
    for g in LIK_G:
        forms[1, g] = table(g)
        if g == 0 or default(g) != default(0):      # (lik_g reaches the default form only where that is the table form)
            forms[2, g] = default(g)
    return forms


def longdouble_likelihood(data, theta, eta, pr):
    """The oracle's formula -- sum w (log w - log s~), w = max(omega, eps), s~ = max(sum omega, eps) -- in np.longdouble."""
    u, i, r = data[:, 0], data[:, 1], data[:, 2]
    om = theta.astype(LD)[u][:, :, None] * eta.astype(LD)[i][:, None, :] * np.moveaxis(pr.astype(LD), 2, 0)[r]
    w = np.maximum(om, LD(EPS))
    s = np.maximum(om.sum(axis=(1, 2)), LD(EPS))
    return float(np.sum(w * (np.log(w) - np.log(s)[:, None, None])))


def zero_likelihood_bound(n_obs, k, l):
    """Where the expected likelihood is exactly 0.0 (every omega and every s_n below eps): each of the n_obs K L
    elements is eps (log eps - log eps) with every logarithm rounded once on either side of the comparison."""
    return n_obs * k * l * EPS * 4 * U53 * abs(np.log(EPS))


def lik_close(got, want, rtol, n_obs, k, l):
    """|got - want| within rtol |want|, or, where want is exactly 0.0, within zero_likelihood_bound."""
    return abs(got - want) <= (rtol * abs(want) if want != 0.0 else zero_likelihood_bound(n_obs, k, l))


LikCell = collections.namedtuple("LikCell", "ref want_start want_loop")
_LIK = {}


def lik_cell(k, l, stage):
    """The cell's data and parameters (test_gpu_staged.reference) with the oracle's likelihood of the staged start and
    of the parameters its three em_steps end in: computed once."""
    if (k, l, stage) not in _LIK:
        ref = reference("uniform", k, l, stage)
        _LIK[k, l, stage] = LikCell(ref, float(orc.compute_likelihood(ref.data, *ref.start)),
                                    float(orc.compute_likelihood(ref.data, *ref.want_loop)))
    return _LIK[k, l, stage]


def row_sums(data, theta, eta, pr):
    return orc.compute_omegas(data, theta, eta, pr).sum(axis=(1, 2))


def dead_rows(data, theta, eta, pr):
    """Number of (triple, k) rows of omega that are clamped throughout: max_l omega[n, k, l] < eps."""
    return int(np.sum(orc.compute_omegas(data, theta, eta, pr).max(axis=2) < EPS))


# ---- models with several slots of one family (held-out, predict, serving) ----------------------------------------------
def family_slots(family, data, dims, k, l, n_slots, zero_users=(), zero_items=()):
    """n_slots parameter sets of one family over `data`: each slot with its own family seed, and with its rows dealt to
    other users and items (the families without random draws would otherwise give every slot the same model);
    the rows `zero_users` of theta and `zero_items` of eta are exact zeros in every slot."""
    n_u, n_i, n_r = dims
    out = []
    for s in range(n_slots):
        rng = np.random.default_rng([k, l, s, len(family), ord(family[0])])
        theta, eta, pr = staged(family, rng, data, n_u, n_i, n_r, k, l)
        if s:
            theta, eta = theta[rng.permutation(n_u)], eta[rng.permutation(n_i)]
        theta, eta = np.ascontiguousarray(theta), np.ascontiguousarray(eta)
        theta[list(zero_users)] = 0.0
        eta[list(zero_items)] = 0.0
        for a in (theta, eta, pr):
            a.setflags(write=False)
        out.append((theta, eta, pr))
    return out


# ---- held-out rows ------------------------------------------------------------------------------------------------
HELDOUT_SHAPES = [(20, 20), (70, 3)]
HELDOUT_FAMILIES = ("late", "rowborder", "tiny", "dead")
HELDOUT_ROWS = 1001


def heldout_case(k, l, family):
    """(data, dims, [family model, init model], held-out rows)."""
    ref = reference("uniform", k, l, family)
    init = reference("uniform", k, l, "init")
    rows = uniform_rows(np.random.default_rng([k, l, 7]), HELDOUT_ROWS, *ref.dims)
    return ref.data, ref.dims, [ref.start, init.start], rows


# ---- predict sums -------------------------------------------------------------------------------------------------
PREDICT_SHAPES = [(20, 20), (7, 33)]
PREDICT_FAMILIES = ("late", "tiny", "dead")


def predict_case(k, l, family):
    """(data, dims, two slots of the family with two users' theta rows at zero, test rows that meet those users)."""
    ref = reference("uniform", k, l, family)
    test = uniform_rows(np.random.default_rng([k, l, 11]), HELDOUT_ROWS, *ref.dims)
    zero_users = (int(test[0, 0]), int(test[500, 0]))
    return ref.data, ref.dims, family_slots(family, ref.data, ref.dims, k, l, 2, zero_users=zero_users), test, zero_users


# ---- serving scores -----------------------------------------------------------------------------------------------
SERVE_FAMILIES = ("late", "border", "rowborder", "tiny", "dead", "sub")
SERVE_R, SERVE_S = 5, 2
#             K   L  swap  U    I
SERVE_CASES = [(20, 20, 0, 120, 300), (20, 20, 1, 120, 300), (7, 33, 0, 120, 300), (7, 33, 1, 120, 300),
               (33, 7, 0, 120, 300), (33, 7, 1, 120, 300), (20, 20, 0, 40, 2100)]
SERVE_IDS = [f"K{c[0]}L{c[1]}swap{c[2]}U{c[3]}I{c[4]}" for c in SERVE_CASES]
SERVE_WEIGHTS = {"values": np.arange(1.0, SERVE_R + 1), "last": np.eye(SERVE_R)[SERVE_R - 1]}
MAX_QUERY = 1024                                      # HipEM.MAX_RECOMMEND and MAX_TOP_PAIRS: the largest n and m of a query

ServeCase = collections.namedtuple("ServeCase", "data dims params zero_users zero_items")
_SERVE = {}


def serve_zero_rows(n_u, n_i):
    """Two users and three items whose rows are exact zeros.  Items I // 3 - 1 and I // 3 sit either side of the first
    boundary when a row of 2,100 items is split into three ranges of 700."""
    return (3, n_u - 1), (n_i // 3 - 1, n_i // 3, n_i - 1)


def serve_case(k, l, n_u, n_i, family):
    if (k, l, n_u, n_i, family) not in _SERVE:
        dims = (n_u, n_i, SERVE_R)
        data = uniform_rows(np.random.default_rng([n_u, n_i, k, l]), 3000, *dims)
        zu, zi = serve_zero_rows(n_u, n_i)
        params = family_slots(family, data, dims, k, l, SERVE_S, zero_users=zu, zero_items=zi)
        data.setflags(write=False)
        _SERVE[k, l, n_u, n_i, family] = ServeCase(data, dims, params, zu, zi)
    return _SERVE[k, l, n_u, n_i, family]


def longdouble_scores(params, weights):
    """(U, I) scores (1/S) sum_s theta_s W_s eta_s^T, W_s = sum_r w_r p_s[:, :, r], in np.longdouble."""
    tot = LD(0)
    for theta, eta, pr in params:
        w = (pr.astype(LD) * np.asarray(weights, dtype=LD)).sum(axis=2)
        tot = tot + theta.astype(LD) @ w @ eta.astype(LD).T
    return tot / LD(len(params))


def score_bound(k, l, n_r, n_slots):
    """Relative bound of one fp64 score against the exact one: the longest chain of roundings a term passes through --
    the W chain (R), the fold chain (K or L, K + L covers either), the rank chain over the slots (S min(K, L)), one
    division, and four for the products -- times 2^-52.  Every term is non-negative (weights included), so the bound
    holds relative to the score whatever the magnitudes of the terms."""
    return (n_r + k + l + n_slots * min(k, l) + 4) * 2.0 ** -52


def score_errors(got, exact, bound, floor):
    """(worst relative error over the entries with exact > floor, as a fraction of `bound`; whether every entry at or
    below the floor agrees within the floor itself)."""
    exact = np.asarray(exact)
    big = exact > floor
    rel = np.abs(np.asarray(got, dtype=LD)[big] - exact[big]) / exact[big]
    small_ok = bool(np.all(np.abs(np.asarray(got, dtype=LD)[~big] - exact[~big]) <= floor))
    return (float(rel.max() / bound) if big.any() else 0.0), small_ok
