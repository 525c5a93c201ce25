"""Greedy assortment selection restated in numpy (no GPU, no library): the reference of test_assortment_cpu.py and
test_gpu_assortment.py.

Everything works on a matrix A (users x items) of ACCUMULATORS -- the undivided sums of the device's score chain, score
= A / S -- or, with S = 1, of plain scores.  Two objectives over the eligible pairs (item not in the user's seen set):

    best_score   state best[u], start floor * S;  term(u, i) = max(0, A[u, i] - best[u])
    reach        state covered[u];                term(u, i) = 1.0 where u is not covered and A[u, i] / S >= bar

A round takes the candidate of largest gain = sum_u term(u, i), equal gains by the smaller item id, and stops when that
gain is not > 0 ("no_gain") or no candidate is left ("no_candidates"); after c rounds: "c".  Given items are applied to
the state first, in order, and are never chosen.
"""
import itertools

import numpy as np

STOPS = ("c", "no_gain", "no_candidates")


def eligible_mask(n_users, n_items, users, seen):
    """(len(users), n_items) bool: the pairs that count (seen: per user id a set of items, or None)."""
    ok = np.ones((len(users), n_items), dtype=bool)
    if seen is not None:
        for b, u in enumerate(np.asarray(users).tolist()):
            if seen[u]:
                ok[b, np.fromiter(seen[u], dtype=np.int64, count=len(seen[u]))] = False
    return ok


class State:
    """The per-user state of a query over the rows of A (already restricted to the request's users)."""

    def __init__(self, A, ok, objective, level, S=1):
        assert objective in ("best_score", "reach") and A.shape == ok.shape
        self.A, self.ok, self.objective, self.level, self.S = A, ok, objective, float(level), float(S)
        n = A.shape[0]
        self.best = np.full(n, self.level * self.S)            # (the product rounds as the device's does)
        self.served = np.full(n, -1, dtype=np.int64)
        self.hits = ok & (A / self.S >= self.level) if objective == "reach" else None

    def terms(self, items):
        """(users, len(items)) terms of the candidate columns `items` against the state."""
        items = np.asarray(items, dtype=np.int64)
        if self.objective == "reach":
            return (self.hits[:, items] & (self.served < 0)[:, None]).astype(np.float64)
        d = self.A[:, items] - self.best[:, None]
        return np.where(self.ok[:, items] & (d > 0), d, 0.0)

    def gains(self, items, order=None):
        """gain sums of the candidate columns, the users added in row order (or in `order`, a permutation)."""
        t = self.terms(items)
        if order is not None:
            t = t[np.asarray(order)]
        return np.add.reduce(t, axis=0) if t.shape[0] == 0 else np.cumsum(t, axis=0)[-1]

    def take(self, item):
        """The state after `item`: strictly better only, so the earliest item that reaches a user's best keeps them."""
        col = self.A[:, item]
        if self.objective == "reach":
            on = self.hits[:, item] & (self.served < 0)
        else:
            on = self.ok[:, item] & (col > self.best)
        self.best = np.where(on, col, self.best)
        self.served = np.where(on, item, self.served)

    def served_frame(self):
        """(row, item, score) of every served user."""
        rows = np.flatnonzero(self.served >= 0)
        return rows, self.served[rows], self.best[rows] / self.S


def greedy(A, c, objective, level, S=1, users=None, seen=None, given=(), candidates=None):
    """{"items", "gains" (sums / S; reach: counts), "stop", "start", "given_gains", "served" (rows, items, scores),
    "value"} of the greedy over the rows `users` of A (None: all, ascending)."""
    n_items = A.shape[1]
    users = np.arange(A.shape[0]) if users is None else np.asarray(users, dtype=np.int64)
    st = State(A[users], eligible_mask(A.shape[0], n_items, users, seen), objective, level, S)
    div = 1.0 if objective == "reach" else float(S)
    given_gains = []
    for g in given:
        given_gains.append(float(st.gains([g])[0]) / div)
        st.take(int(g))
    cand = np.arange(n_items) if candidates is None else np.asarray(candidates, dtype=np.int64)
    left = cand[~np.isin(cand, np.asarray(list(given), dtype=np.int64))]
    items, gains, stop = [], [], "c"
    for _ in range(c):
        if len(left) == 0:
            stop = "no_candidates"
            break
        g = st.gains(left)
        k = int(np.lexsort((left, -g))[0])                     # largest gain, equal gains by the smaller id
        if not g[k] > 0:
            stop = "no_gain"
            break
        items.append(int(left[k]))
        gains.append(float(g[k]) / div)
        st.take(int(left[k]))
        left = np.delete(left, k)
    start = float(np.cumsum(given_gains)[-1]) if given_gains else 0.0
    total = float(np.cumsum(gains)[-1]) if gains else 0.0
    n_u = len(users)
    if objective == "reach":
        value = (start + total) / n_u if n_u else 0.0
    else:
        value = float(level) + (start + total) / n_u if n_u else float(level)
    return {"items": np.asarray(items, dtype=np.int64), "gains": np.asarray(gains, dtype=np.float64), "stop": stop,
            "start": start, "given_gains": np.asarray(given_gains, dtype=np.float64), "served": st.served_frame(),
            "value": value}


def set_value(A, items, objective, level, S=1, users=None, seen=None):
    """F(items) - F(empty set), summed exactly as the definition reads (no greedy, no state): best_score in score
    units (sum over the users of max(floor, best eligible score) - floor), reach as a count."""
    users = np.arange(A.shape[0]) if users is None else np.asarray(users, dtype=np.int64)
    ok = eligible_mask(A.shape[0], A.shape[1], users, seen)
    items = np.asarray(list(items), dtype=np.int64)
    sc = np.where(ok[:, items], A[users][:, items] / float(S), -np.inf)
    if objective == "reach":
        return float((sc >= level).any(axis=1).sum()) if len(items) else 0.0
    best = np.maximum(sc.max(axis=1), level) if len(items) else np.full(len(users), float(level))
    return float((best - level).sum())


def best_set(A, c, objective, level, S=1, seen=None):
    """(value, items) of the best set of at most c items by brute force (small instances only)."""
    top = (0.0, ())
    for k in range(1, c + 1):
        for combo in itertools.combinations(range(A.shape[1]), k):
            v = set_value(A, combo, objective, level, S, None, seen)
            if v > top[0]:
                top = (v, combo)
    return top


# ---- random models: the walk along the device's own picks -------------------------------------------------------------
def gain_bound(n_users, w):
    """tau: |device best-score gain - numpy's gain on the device scores D| for one item, in score units.

    The device sums accumulator differences, numpy differences of D = accumulator / S.  Per user:
      * D[u, i] and best[u] / S each carry one rounding of the division: <= 2^-53 max|w| each (|score| <= max|w|), so
        the difference of the two quotients is off the exact (a - best) / S by <= 2 x 2^-53 max|w|, and forming it
        rounds once more, <= 2^-53 x 2 max|w| (|difference| <= 2 max|w|)                          -> 4 units
      * the device's own difference a - best rounds once: <= 2^-53 x 2 S max|w| in accumulator units, 2 units in score
        units                                                                                      -> 2 units
      * a term the one side counts and the other drops (a difference that rounds to 0, or the floor x S product's
        rounding) is itself within those bounds.
    So a term differs by <= 6 units of 2^-53 max|w|.  Each side then adds n_u non-negative terms in a chain: every
    partial sum is <= 2 n_u max|w| and every addition rounds by <= 2^-53 of it, n_u - 1 additions a side, both sides
    <= 2 x 2 n_u (n_u - 1) units; the device's final division by S adds one rounding of the total, <= 2 n_u units.
    Together <= (6 n_u + 4 n_u (n_u - 1) + 2 n_u) <= 4 n_u (n_u + 2) units: c0 = 4.
    """
    return 4.0 * n_users * (n_users + 2) * 2.0 ** -53 * float(np.abs(w).max())


def walk(D, objective, level, users, seen, given, candidates, dev_items, dev_gains, stop, c, tau=0.0):
    """Follow the device's own picks over the device scores D (S = 1 arithmetic on D): per round the device's gain for
    its pick is numpy's (reach: equal; best_score: within tau), no other candidate's numpy gain beats it (reach: by the
    (gain, id) order exactly; best_score: by more than tau), and the stop reason holds at the end.  Returns the state."""
    users = np.asarray(users, dtype=np.int64)
    st = State(D[users], eligible_mask(D.shape[0], D.shape[1], users, seen), objective, level, 1)
    for g in given:
        st.take(int(g))
    cand = np.arange(D.shape[1]) if candidates is None else np.asarray(candidates, dtype=np.int64)
    left = cand[~np.isin(cand, np.asarray(list(given), dtype=np.int64))]
    for k, (item, gain) in enumerate(zip(np.asarray(dev_items).tolist(), np.asarray(dev_gains).tolist())):
        g = st.gains(left)
        at = int(np.flatnonzero(left == item)[0])              # (the pick is a candidate that is left)
        if objective == "reach":
            assert gain == g[at], (k, item, gain, g[at])
            assert at == int(np.lexsort((left, -g))[0]), (k, item, left[np.lexsort((left, -g))[0]])
        else:
            assert abs(gain - g[at]) <= tau, (k, item, gain - g[at], tau)
            assert g.max() <= gain + tau, (k, item, g.max() - gain, tau)
        assert gain > 0
        st.take(item)
        left = np.delete(left, at)
    n = len(dev_items)
    if stop == "c":
        assert n == c
    elif stop == "no_candidates":
        assert n < c and len(left) == 0
    else:
        assert stop == "no_gain" and n < c and len(left) > 0
        assert st.gains(left).max() <= (0.0 if objective == "reach" else tau)
    return st
