"""Starting parameters of the kind a long EM run ends in -- shared by test_staged_params_cpu.py and test_gpu_staged.py.

Every parity case of the M-step used to start from orc.init_params or rng.random: memberships of one magnitude, nothing
zero, no row sum s_n near eps.  staged() starts from orc.init_params too and then moves the parameters to where the
kernels' `1 / max(s, eps)`, the zero-row guard of p and the padding of the tiles matter:

  late       memberships concentrated on a few groups, the others decayed over more than 100 decades
  border     products theta eta p a few decades either side of eps; about 10 % of theta, 5 % of eta and of p exact zeros
  rowborder  every theta row and every eta row scaled by its own 10 ** U(-10, 0): the ROW SUMS s_n straddle eps
  tiny       theta and eta x 1e-110: every s_n is below eps
  dead       whole groups dead: theta[:, ::3] = 0, eta[:, 1::4] = 0, one p[k, :, :] = 0
  sub        every other row of one theta column at 3e-310, of one eta column at 7e-315, one p entry at 5e-320:
             subnormal operands and subnormal results.  (Not the WHOLE column: then every numerator of p[0, l, :] and
             p[k, L-1, :] is a subnormal with a handful of significant bits, and the normalised p' -- a ratio of such
             sums, of order one -- differs by 3e-8 between the dense and the factorised CPU evaluation.  With the other
             rows normal those sums are normal and the step is unambiguous: test_staged_params_cpu.py.)
  subcolumn  the WHOLE theta column at 3e-310, the whole eta column at 7e-315, the p entry at 5e-320: for checks of the
             numerators of one step only (they are unambiguous; p' is not, see above).  Here whole rows of the C table
             are subnormal, so some results depend on subnormal operands of the pair stage alone.
  init       orc.init_params as it is (the friendly start, for a slot next to a staged one)

late, border and tiny are the recipes of test_gpu_parity.test_likelihood_a_wave_per_pair.  A plain module, no conftest.
"""
import numpy as np

from oracle import mmsbm_oracle as orc

FAMILIES = ("late", "border", "rowborder", "tiny", "dead", "sub")
START_SEED = 3


def staged(name, rng, data, n_u, n_i, n_r, K, L):
    """(theta, eta, pr) of family `name` for the triples `data`; `rng` supplies the family's own random draws."""
    d_u, d_i = orc.degrees(data, n_u, n_i)
    theta, eta, pr = orc.init_params(START_SEED, n_u, n_i, n_r, K, L, d_u, d_i)
    if name == "init":
        pass
    elif name == "late":
        theta = theta ** rng.integers(1, 40, theta.shape)
        eta = eta ** rng.integers(1, 40, eta.shape)
        theta /= theta.sum(1, keepdims=True)
        eta /= eta.sum(1, keepdims=True)
        pr = orc.normalize_with_self(pr ** rng.integers(1, 12, pr.shape))
    elif name == "border":
        theta = 10.0 ** rng.uniform(-9, -3, theta.shape)
        eta = 10.0 ** rng.uniform(-9, -3, eta.shape)
        theta[rng.random(theta.shape) < 0.1] = 0.0
        eta[rng.random(eta.shape) < 0.05] = 0.0
        pr[rng.random(pr.shape) < 0.05] = 0.0
    elif name == "rowborder":
        theta = theta * 10.0 ** rng.uniform(-10, 0, (n_u, 1))
        eta = eta * 10.0 ** rng.uniform(-10, 0, (n_i, 1))
    elif name == "tiny":
        theta, eta = theta * 1e-110, eta * 1e-110
    elif name == "dead":
        theta[:, ::3] = 0.0
        eta[:, 1::4] = 0.0
        pr[2 % K, :, :] = 0.0
    elif name == "sub":
        theta[::2, 0] = 3e-310
        eta[::2, -1] = 7e-315
        pr[0, 0, 0] = 5e-320
    elif name == "subcolumn":
        theta[:, 0] = 3e-310
        eta[:, -1] = 7e-315
        pr[0, 0, 0] = 5e-320
    else:
        raise ValueError(f"unknown family {name!r}")
    return np.ascontiguousarray(theta), np.ascontiguousarray(eta), np.ascontiguousarray(pr)


def uniform_rows(rng, n, n_u, n_i, n_r):
    """n triples with independent uniform columns, ids inside (n_u, n_i, n_r) -- not re-encoded: ids may be unused."""
    return np.stack([rng.integers(0, n_u, n), rng.integers(0, n_i, n), rng.integers(0, n_r, n)], axis=1).astype(np.int64)


def clamped_rows(data, theta, eta, pr):
    """Share of the triples whose s_n = sum_kl omega is below eps (the rows `max(s, eps)` changes)."""
    return float(np.mean(orc.compute_omegas(data, theta, eta, pr).sum(axis=(1, 2)) < orc.EPS))


def clamped_elements(data, theta, eta, pr):
    """Share of the omega elements below eps (what the likelihood's element clamp changes)."""
    return float(np.mean(orc.compute_omegas(data, theta, eta, pr) < orc.EPS))
