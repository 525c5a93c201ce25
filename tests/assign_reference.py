"""Welfare-maximising assignment, restated in numpy (no GPU, no library): the reference of test_assign_cpu.py and
test_gpu_assign.py.

The problem: every user of a request gets at most one item, item i at most caps[i] users (0: none; negative or >= the
number of request users: unlimited); maximise the sum of the assigned scores plus `reserve` per unassigned user.  Pairs
a user has seen are no candidates.

  auction   the forward auction of mmsbm_amd/csrc/assign.hpp, round by round, in the device's operation order: additions,
            subtractions and comparisons of doubles only, so that fed the device's score bits it gives the device's
            price bits
  optimum   the exact optimum by the Hungarian method on the slot-expanded matrix with one private column per user (the
            reserve, or the user's best unlimited item: nobody competes for either)
  brute     every assignment of a tiny problem
"""
import itertools
import math

import numpy as np


def unlimited(caps, n_users):
    caps = np.asarray(caps, dtype=np.int64)
    return (caps < 0) | (caps >= n_users)


def masked(scores, users, seen):
    """The candidates' scores by request row, -inf where users[b] has seen the item."""
    s = np.array(scores, dtype=np.float64, copy=True)
    if seen is not None:
        for b, u in enumerate(np.asarray(users).tolist()):
            if seen[u]:
                s[b, np.fromiter(seen[u], dtype=np.int64, count=len(seen[u]))] = -np.inf
    return s


def auction(scores, users, caps, reserve, eps, seen=None, max_rounds=10000):
    """scores (len(users), I): row b is user users[b] (distinct ids).  Returns a dict: items, score, paid, pi (by request
    row; unassigned: -1, -inf, 0), p1, price_sum, load (by item), slots {item: (prices, holders)}, rounds, bids,
    converged, dropped (by request row)."""
    users = np.asarray(users, dtype=np.int64)
    n, I = len(users), scores.shape[1]
    caps = np.asarray(caps, dtype=np.int64)
    order = np.argsort(users, kind="stable")                 # the device works in id order: row r = users[order[r]]
    S = masked(scores, users, seen)[order]
    free = unlimited(caps, n)
    p1 = np.where(free, 0.0, np.where(caps == 0, np.inf, 0.0))
    p2 = np.where(free, 0.0, np.where(caps >= 2, 0.0, np.inf))
    price = {int(i): np.zeros(int(caps[i])) for i in np.flatnonzero(~free & (caps > 0))}
    holder = {i: np.full(len(p), -1, dtype=np.int64) for i, p in price.items()}
    item = np.full(n, -1, dtype=np.int64)
    paid = np.zeros(n)
    dropped = np.zeros(n, dtype=bool)
    rounds = bids = 0
    converged = True
    while True:
        act = np.flatnonzero((item < 0) & ~dropped)
        if len(act) == 0:
            break
        if rounds == max_rounds:
            converged = False
            break
        rounds += 1
        V = S[act] - p1[None, :]
        i1 = np.argmax(V, axis=1)                            # (the first of equal values: the smallest item id)
        rows = np.arange(len(act))
        v1 = V[rows, i1]
        V[rows, i1] = -np.inf
        v2p = V.max(axis=1)
        stay = v1 > reserve
        dropped[act[~stay]] = True
        s1 = S[act, i1]
        with np.errstate(invalid="ignore"):
            v2 = np.maximum(np.maximum(reserve, v2p), s1 - p2[i1])
            beta = (p1[i1] + (v1 - v2)) + eps
        bids += int(stay.sum())
        by_item = {}
        for r in np.flatnonzero(stay).tolist():              # ascending row = ascending user id
            by_item.setdefault(int(i1[r]), []).append(r)
        for i, rs in by_item.items():
            if free[i]:
                for r in rs:
                    item[act[r]], paid[act[r]] = i, 0.0
                continue
            rs = sorted(rs, key=lambda r: (-beta[r], r))     # bid descending, equal bids by ascending user
            pr, ho = price[i], holder[i]
            for k, r in enumerate(rs[:len(pr)]):
                if not beta[r] > pr[k]:
                    break
                if ho[k] >= 0:
                    item[ho[k]] = -1
                    paid[ho[k]] = 0.0
                pr[k], ho[k] = beta[r], act[r]
                item[act[r]], paid[act[r]] = i, beta[r]
            again = np.lexsort((ho, pr))                     # price ascending, then holder ascending
            price[i], holder[i] = pr[again], ho[again]
            p1[i] = price[i][0]
            if len(pr) >= 2:
                p2[i] = price[i][1]
    V = S - p1[None, :]
    pi = np.maximum(reserve, V.max(axis=1)) if I > 0 else np.full(n, float(reserve))
    got = item >= 0
    score = np.where(got, S[np.arange(n), np.maximum(item, 0)], -np.inf)
    back = np.empty(n, dtype=np.int64)
    back[order] = np.arange(n)                               # request row b is sorted row back[b]
    price_sum = np.zeros(I)
    for i, p in price.items():
        for x in p.tolist():                                 # (the device's order: the slots ascending, one addition each)
            price_sum[i] += x
    slots = {i: (price[i].copy(), np.where(holder[i] >= 0, users[order][np.maximum(holder[i], 0)], -1)) for i in price}
    return {"items": item[back].astype(np.int32), "score": score[back], "paid": paid[back], "pi": pi[back],
            "p1": p1, "price_sum": price_sum, "load": np.bincount(item[got], minlength=I).astype(np.int32),
            "slots": slots, "rounds": rounds, "bids": bids, "converged": converged, "dropped": dropped[back]}


def summary(res, reserve, eps):
    """What MMSBM.assign puts into assignment_: the sums, by math.fsum."""
    got = res["items"] >= 0
    assigned = int(got.sum())
    total = math.fsum(res["score"][got].tolist())
    value = math.fsum(res["score"][got].tolist() + [float(reserve)] * int((~got).sum()))
    bound = math.fsum(res["pi"].tolist() + res["price_sum"].tolist())
    return {"assigned": assigned, "total": total, "value": value, "bound": bound, "gap_limit": assigned * eps}


def check_feasible(res, scores, users, caps, seen=None):
    """One item per user at most, a candidate each, nobody beyond a cap, the scores the pairs' own."""
    S = masked(scores, users, seen)
    items = np.asarray(res["items"], dtype=np.int64)
    got = items >= 0
    assert (items[~got] == -1).all() and np.isneginf(np.asarray(res["score"])[~got]).all()
    assert (np.asarray(res["paid"])[~got] == 0).all()
    taken = S[np.flatnonzero(got), items[got]]
    assert np.isfinite(taken).all() and np.array_equal(taken.view(np.uint64), np.asarray(res["score"])[got].view(np.uint64))
    load = np.bincount(items[got], minlength=S.shape[1])
    caps = np.asarray(caps, dtype=np.int64)
    bind = ~unlimited(caps, len(users))
    assert (load[bind] <= caps[bind]).all()
    assert np.array_equal(load, np.asarray(res["load"], dtype=np.int64))


# ---- the exact optimum ---------------------------------------------------------------------------------------------------
def _expanded(scores, users, caps, reserve, seen):
    """The slot-expanded value matrix (n, columns) and every column's item (-1: the user's private column)."""
    S = masked(scores, users, seen)
    n, I = S.shape
    caps = np.asarray(caps, dtype=np.int64)
    free = unlimited(caps, n)
    own = np.full(n, float(reserve))
    own_item = np.full(n, -1, dtype=np.int64)
    if free.any():
        idx = np.flatnonzero(free)
        best = S[:, idx].max(axis=1)
        better = best > own
        own[better] = best[better]
        own_item[better] = idx[np.argmax(S[:, idx], axis=1)][better]
    cols = np.repeat(np.flatnonzero(~free), caps[~free])
    M = np.full((n, len(cols) + n), -np.inf)
    M[:, :len(cols)] = S[:, cols]
    M[np.arange(n), len(cols) + np.arange(n)] = own
    return M, np.concatenate([cols, np.full(n, -1, dtype=np.int64)]), own_item


def hungarian_max(M):
    """Column of every row of M (n rows <= columns) in a row-perfect matching of largest total value; -inf: no pair.
    The shortest-augmenting-path form with potentials, the inner step in numpy."""
    n, m = M.shape
    assert n <= m
    big = 1.0 + 4.0 * float(np.abs(M[np.isfinite(M)]).max(initial=1.0)) * max(n, 1)
    cost = np.where(np.isfinite(M), -M, big)
    u, v = np.zeros(n + 1), np.zeros(m + 1)
    match = np.zeros(m + 1, dtype=np.int64)                  # column j (1-based) holds row match[j] (1-based; 0: free)
    way = np.zeros(m + 1, dtype=np.int64)
    for r in range(1, n + 1):
        match[0] = r
        j0 = 0
        minv = np.full(m + 1, np.inf)
        used = np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = match[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            open_ = ~used[1:]
            upd = open_ & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            cand = np.where(open_, minv[1:], np.inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[match[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if match[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            match[j0] = match[j1]
            j0 = j1
    col = np.full(n, -1, dtype=np.int64)
    for j in range(1, m + 1):
        if match[j]:
            col[match[j] - 1] = j - 1
    return col


def optimum(scores, users, caps, reserve, seen=None):
    """(value, items by request row): the largest sum of assigned scores plus reserve per unassigned user."""
    users = np.asarray(users, dtype=np.int64)
    if len(users) == 0:
        return 0.0, np.zeros(0, dtype=np.int64)
    M, col_item, own_item = _expanded(scores, users, caps, reserve, seen)
    col = hungarian_max(M)
    vals = M[np.arange(len(users)), col]
    assert np.isfinite(vals).all() or np.isneginf(reserve)
    items = col_item[col]
    private = items < 0
    items[private] = own_item[private]
    return math.fsum(vals.tolist()), items


def brute(scores, users, caps, reserve, seen=None):
    """The optimum value of a tiny problem by trying everything."""
    S = masked(scores, users, seen)
    n, I = S.shape
    caps = np.asarray(caps, dtype=np.int64)
    free = unlimited(caps, n)
    best = -np.inf
    for pick in itertools.product(range(-1, I), repeat=n):
        load = np.bincount([i for i in pick if i >= 0], minlength=I)
        if (load[~free] > caps[~free]).any():
            continue
        vals = [float(reserve) if i < 0 else S[b, i] for b, i in enumerate(pick)]
        if any(np.isneginf(x) for x in vals) and not np.isneginf(reserve):
            continue
        best = max(best, math.fsum(vals))
    return best
