"""Matching the groups of the restarts (``MMSBM.align_restarts`` / ``MMSBM.consensus``): the host half.

The device hands over the Gram matrix O of the restarts' membership tables of one side (csrc/overlap.hpp): with G groups
per restart, block (s, t) of O is ``O[s*G:(s+1)*G, t*G:(t+1)*G][a, b] = sum_row x_s[row, a] x_t[row, b]`` -- how much
of the population group a of restart s and group b of restart t share.  What is left is small: S^2 assignment problems
of size G, then permuting and averaging.  Numpy only."""
from __future__ import annotations

import numpy as np


def _augment(cost, u, v, row_of, i):
    """One step of the Hungarian method in its shortest-augmenting-path form: row ``i`` (1-based) enters the matching
    ``row_of`` (the row matched to each column, 1-based, 0: none) by one Dijkstra-like search over the columns under
    the potentials ``u`` / ``v``, which stay feasible (u[i] + v[j] <= cost[i, j], with equality on matched pairs).  In
    place.  Among columns of equal reduced cost the search takes the first."""
    n = cost.shape[0]
    row_of[0] = i
    j0 = 0
    minv = np.full(n, np.inf)
    way = np.zeros(n + 1, dtype=np.int64)
    used = np.zeros(n + 1, dtype=bool)
    while True:
        used[j0] = True
        i0 = row_of[j0]
        free = ~used[1:]
        cur = cost[i0 - 1] - u[i0] - v[1:]
        better = free & (cur < minv)
        minv[better] = cur[better]
        way[1:][better] = j0
        cand = np.where(free, minv, np.inf)
        j1 = int(np.argmin(cand)) + 1            # (the first of the smallest)
        delta = cand[j1 - 1]
        u[row_of[used]] += delta
        v[used] -= delta
        minv[free] -= delta
        j0 = j1
        if row_of[j0] == 0:
            break
    while j0:                                    # the augmenting path, back to the dummy column
        j1 = way[j0]
        row_of[j0] = row_of[j1]
        j0 = j1


def _solve(M):
    """(cost, u, v, row_of) of the minimum-cost perfect matching of ``-M``: O(G^3), rows entering in ascending order."""
    M = np.asarray(M, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError(f"a square matrix is needed, got shape {M.shape}")
    if not np.isfinite(M).all():
        raise ValueError("finite entries are needed")
    n = M.shape[0]
    cost = -M
    u, v = np.zeros(n + 1), np.zeros(n + 1)      # potentials (index 0: the dummy row / column of the search)
    row_of = np.zeros(n + 1, dtype=np.int64)
    for i in range(1, n + 1):
        _augment(cost, u, v, row_of, i)
    return cost, u, v, row_of


def _columns(row_of):
    col = np.empty(len(row_of) - 1, dtype=np.int64)
    col[row_of[1:] - 1] = np.arange(len(col))
    return col


def best_assignment(M):
    """The maximum-weight perfect matching of the square matrix ``M``: ``col`` (G,) int64 with row k matched to column
    ``col[k]``, every column used once, ``sum_k M[k, col[k]]`` the largest any permutation reaches.

    Shortest augmenting paths with potentials (the Hungarian method in its O(G^3) form) on the cost ``-M``.
    Deterministic: the same matrix gives the same matching -- one of the optima where there are several."""
    return _columns(_solve(M)[3])


def assignment_margin(M):
    """How decisive ``best_assignment(M)`` is: its total minus the total of the best OTHER assignment (0.0 where a
    second optimum exists, +inf for G = 1).  Another assignment leaves out at least one optimal pair, so the second
    best is the best of G re-solved problems with one optimal pair forbidden each; a re-solve is one augmentation
    from the optimum's potentials (they stay feasible when a cost rises), O(G^2)."""
    cost, u, v, row_of = _solve(M)
    n = cost.shape[0]
    col = _columns(row_of)
    k = np.arange(n)
    best = -cost[k, col].sum()
    # (larger than any path of allowed pairs, and still finite: the forbidden pair is only taken when nothing else is left)
    big = 4.0 * (n + 1) * max(1.0, float(np.abs(cost).max()))
    second = -np.inf
    for row in range(n if n > 1 else 0):
        c2, u2, v2, r2 = cost.copy(), u.copy(), v.copy(), row_of.copy()
        c2[row, col[row]] = big
        r2[col[row] + 1] = 0
        _augment(c2, u2, v2, r2, row + 1)
        other = _columns(r2)
        if other[row] != col[row]:
            second = max(second, -cost[k, other].sum())
    return float(best - second)


def block(O, G, s, t):
    """Block (s, t) of the Gram matrix ``O`` of restarts with ``G`` groups each."""
    return O[s * G:(s + 1) * G, t * G:(t + 1) * G]


def group_cosine(O, G, s, t, col):
    """(G,) the cosine of column k of restart s and column ``col[k]`` of restart t:
    ``O_st[k, col[k]] / sqrt(O_ss[k, k] O_tt[col[k], col[k]])``, 0.0 where a norm is 0."""
    col = np.asarray(col, dtype=np.int64)
    k = np.arange(G)
    num = block(O, G, s, t)[k, col]
    den = np.sqrt(np.diagonal(block(O, G, s, s)) * np.diagonal(block(O, G, t, t))[col])
    out = np.zeros(G, dtype=np.float64)
    np.divide(num, den, out=out, where=den > 0)
    return np.clip(out, 0.0, 1.0)            # (Cauchy-Schwarz up to rounding)


def consensus_params(results, user_groups, item_groups):
    """(theta (U, K), eta (I, L), pr (K, L, R)): the mean over the restarts ``results`` (dicts with "theta", "eta",
    "pr") once their groups are matched -- ``user_groups[s, k]`` / ``item_groups[s, l]`` the group of restart s that
    is group k / l of the reference:

        theta[u, k] = mean_s theta_s[u, user_groups[s, k]],      eta likewise,
        pr[k, l, r] = mean_s pr_s[user_groups[s, k], item_groups[s, l], r].

    Summed over the restarts in ascending position, then divided once by S."""
    ug, ig = np.asarray(user_groups, dtype=np.int64), np.asarray(item_groups, dtype=np.int64)
    S = len(results)
    if ug.shape[0] != S or ig.shape[0] != S:
        raise ValueError(f"{S} restarts, but user_groups / item_groups hold {ug.shape[0]} / {ig.shape[0]} rows")
    theta = eta = pr = None
    for s, res in enumerate(results):
        t = np.asarray(res["theta"], dtype=np.float64)[:, ug[s]]
        e = np.asarray(res["eta"], dtype=np.float64)[:, ig[s]]
        p = np.asarray(res["pr"], dtype=np.float64)[ug[s]][:, ig[s]]
        theta, eta, pr = (t, e, p) if s == 0 else (theta + t, eta + e, pr + p)
    return theta / S, eta / S, pr / S


def align_side(O, G, n_rows, reference):
    """One side of ``MMSBM.align_restarts`` from its Gram matrix ``O`` (S G x S G): (groups (S, G) int64, similarity
    (S, G), agreement (S, S)).  ``groups[s]`` = ``best_assignment`` of block (reference, s); ``agreement[s, t]`` = the
    optimal assignment total of block (s, t) / ``n_rows``, computed for s <= t and mirrored (block (t, s) is its
    transpose: the same optimum)."""
    S = O.shape[0] // G
    groups = np.empty((S, G), dtype=np.int64)
    similarity = np.empty((S, G), dtype=np.float64)
    agreement = np.empty((S, S), dtype=np.float64)
    k = np.arange(G)
    for s in range(S):
        groups[s] = k if s == reference else best_assignment(block(O, G, reference, s))
        similarity[s] = 1.0 if s == reference else group_cosine(O, G, reference, s, groups[s])
    for s in range(S):
        for t in range(s, S):
            b = block(O, G, s, t)
            agreement[s, t] = agreement[t, s] = b[k, best_assignment(b)].sum() / n_rows
    return groups, similarity, agreement
