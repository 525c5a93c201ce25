"""Ensemble-aware recommendation restated in numpy (no GPU, no library): what mmsbm_hip_recommend_query_ensemble and
mmsbm_hip_recommend_pair_spread answer, from the stack a [S][rows][items] of the score each restart ALONE gives a pair.
Shared by test_ensemble_cpu.py (which pins its properties) and test_gpu_ensemble.py (which feeds it the device's own
per-restart scores).

Every line below is ONE float64 operation on arrays: numpy rounds each of them, which is what the device does with
contraction off (ensemble.hpp), in the same order:
    worst = min_s a_s                       best = max_s a_s
    d_s = a_s - a_0   (s = 1 .. S - 1)      D = ((+0.0 + d_1) + d_2) + ...      Q = ((+0.0 + d_1 d_1) + d_2 d_2) + ...
    mean = a_0 + D / S
    var  = max(S Q - D D, +0.0) / (S S)     std = sqrt(var)
    lcb  = mean - risk std
Order of a list: value descending, equal values by ascending item id (catalogue_reference._row)."""
import numpy as np

import catalogue_reference as cat

MODES = ("min", "max", "lcb")


def spread(a):
    """{"worst", "best", "mean", "std"} of the stack a [S][...], each shaped like a[0]."""
    a = np.asarray(a, dtype=np.float64)
    S = float(a.shape[0])
    worst, best = a[0].copy(), a[0].copy()
    D, Q = np.zeros_like(a[0]), np.zeros_like(a[0])
    for s in range(1, a.shape[0]):
        worst = np.where(a[s] < worst, a[s], worst)
        best = np.where(a[s] > best, a[s], best)
        d = a[s] - a[0]
        dd = d * d
        D = D + d
        Q = Q + dd
    q = D / S
    mean = a[0] + q
    sq = S * Q
    dd = D * D
    t = sq - dd
    var = np.where(t > 0.0, t, 0.0) / (S * S)
    return {"worst": worst, "best": best, "mean": mean, "std": np.sqrt(var)}


def lcb(mean, std, risk):
    r = np.float64(risk) * std
    return mean - r


def aggregate(a, mode, risk=0.0):
    """The value the query ranks by, shaped like a[0]."""
    sp = spread(a)
    if mode == "min":
        return sp["worst"]
    if mode == "max":
        return sp["best"]
    assert mode == "lcb", mode
    return lcb(sp["mean"], sp["std"], risk)


def top_n(a, users, n, mode, risk=0.0, cand=None, seen=None, extra=None):
    """(items (M, n) padded with -1, values (M, n) padded with -inf, counts (M,)): row b = the n best candidates of user
    users[b] by aggregate(a[:, users[b]]); cand / seen / extra as in catalogue_reference.within_top_n."""
    users = np.asarray(users, dtype=np.int64)
    return cat.within_top_n(aggregate(np.asarray(a)[:, users], mode, risk), users, n, cand, seen, extra)


def ulp(x):
    """The unit in the last place of |x| (the spacing of the doubles at x)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))
