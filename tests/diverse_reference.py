"""Diversified top-N restated without the library (no GPU): what mmsbm_hip_recommend_diverse answers, from a pool in
recommend's order and the pairwise distances of its items.  Shared by test_diverse_cpu.py and test_gpu_diverse.py.

For one request row, with the pool P (ids, scores; score descending, equal scores by ascending id):
    pick 1   P[0];
    pick j   over the places i not picked yet: m_i = min over the earlier picks a of D(t_a, i),
             v_i = fma(lam, m_i, score_i) -- ONE rounding --, and the largest v_i wins, equal v_i the earlier place;
    output   the id, the pool's score and m at the moment of the pick (+inf for pick 1).
"""
from fractions import Fraction

import numpy as np

import catalogue_reference as cat
import exact_models as xm
from test_similar_cpu import exact_distances


def fma(a, b, c):
    """a * b + c with one rounding (Python 3.10 has no math.fma; Fraction.__float__ rounds correctly)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _fma_ratio(a, b, c):
    """fma through the integer ratios of the three doubles: the same rational number as fma(), divided once (int / int
    is correctly rounded)."""
    an, ad = a.as_integer_ratio()
    bn, bd = b.as_integer_ratio()
    cn, cd = c.as_integer_ratio()
    return (an * bn * cd + cn * ad * bd) / (ad * bd * cd)


_SPLIT = 134217729.0        # 2^27 + 1 (Veltkamp)


def fma_many(lam, m, s):
    """fma(lam, m[k], s[k]) for arrays of finite doubles.  Where the product lam * m[k] is exact in fp64 (Dekker's
    error term is zero: every power-of-two lam) the sum p + s[k] already rounds once; the other entries go through the
    exact integer form, equal inputs once."""
    m, s = np.asarray(m, dtype=np.float64), np.asarray(s, dtype=np.float64)
    p = lam * m
    t = _SPLIT * lam
    ah = t - (t - lam)
    al = lam - ah
    t = _SPLIT * m
    bh = t - (t - m)
    bl = m - bh
    err = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    out = p + s
    seen = {}
    for k in np.flatnonzero(err != 0.0).tolist():
        key = (float(m[k]), float(s[k]))
        if key not in seen:
            seen[key] = _fma_ratio(float(lam), key[0], key[1])
        out[k] = seen[key]
    return out


def greedy(ids, scores, dist, n, lam):
    """(items, scores, distances, tied): the picks of one row.  ids, scores: the pool (M,), in recommend's order;
    dist (M, M): dist[a, i] = D(ids[a], ids[i]), place a as the query row.  tied[j - 2]: the best value of pick j
    (j >= 2) was shared by two or more places."""
    ids, scores = np.asarray(ids), np.asarray(scores, dtype=np.float64)
    M = len(ids)
    picks = min(n, M)
    if picks == 0:
        return ids[:0], scores[:0], np.zeros(0), []
    order, dists, tied = [0], [np.inf], []
    open_ = np.ones(M, dtype=bool)
    open_[0] = False
    m = np.full(M, np.inf)
    for _ in range(1, picks):
        m = np.minimum(m, dist[order[-1]])
        places = np.flatnonzero(open_)
        v = fma_many(lam, m[places], scores[places])
        best = v.max()
        at = int(places[np.argmax(v == best)])                  # (argmax of a bool array: the first True)
        tied.append(int((v == best).sum()) > 1)
        order.append(at)
        dists.append(float(m[at]))
        open_[at] = False
    order = np.asarray(order)
    return ids[order], scores[order], np.asarray(dists), tied


def pack(rows, n):
    """(items (M, n) padded with -1, scores padded with -inf, distances padded with +inf, counts) of greedy rows."""
    items = np.full((len(rows), n), -1, dtype=np.int32)
    vals = np.full((len(rows), n), -np.inf)
    dists = np.full((len(rows), n), np.inf)
    counts = np.zeros(len(rows), dtype=np.int32)
    for b, (it, sc, d, _) in enumerate(rows):
        counts[b] = len(it)
        items[b, :len(it)], vals[b, :len(it)], dists[b, :len(it)] = it, sc, d
    return items, vals, dists, counts


def exact_diverse(params, users, weights, seen, cand, excl, n, pool, lam, scores=None, dist=None, ties=None):
    """What recommend_diverse returns on the models of exact_models.py: the pool from exact_scores (seen: sets by user
    id or None; cand: ids or None; excl: one iterable per request row or None), the distances from exact_distances.
    scores (len(users), I) and dist (I, I): the two tables when the caller has them already.  ties: a list that takes
    every row's `tied` flags."""
    n_items = params[0][1].shape[0]
    if scores is None:
        scores = xm.exact_scores(params, users, n_items, weights)
    if dist is None:
        dist = exact_distances(params, "items", np.arange(n_items))
    p_ids, p_sc, p_cnt = cat.within_top_n(scores, users, pool, cand, seen, excl)
    rows = []
    for b in range(len(users)):
        k = int(p_cnt[b])
        mine = p_ids[b, :k].astype(np.int64)
        rows.append(greedy(mine, p_sc[b, :k], dist[np.ix_(mine, mine)], n, lam))
        if ties is not None:
            ties.append(rows[-1][3])
    return pack(rows, n)
