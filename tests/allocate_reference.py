"""Capacity-aware allocation restated in numpy (no GPU, no library): what mmsbm_hip_recommend_allocate and
MMSBM.allocate answer, for test_allocate_cpu.py and test_gpu_allocate.py.

``greedy`` is the definition: all candidate pairs (u, i) of the request walked in top_pairs' order -- score descending,
equal scores by ascending user id, then ascending item id --, a pair taken iff u holds fewer than n items and i was
given out fewer than cap[i] times.  ``threshold_rounds`` is the algorithm the device runs (allocate.hpp): rounds of
user-proposing deferred acceptance with one threshold per capped item; because every preference is read off one strict
order of the pairs, the stable matching is unique and both give the same answer.

Arguments of both: ``scores`` (len(users), n_items), row b the exact scores of user users[b] (exact_models.py);
``users`` distinct ids; ``caps`` one integer per item (0: the item is out, negative or >= len(users): unlimited);
``seen``: per user ID the set of items left out for it, or None.  Answers are (items, scores, counts) as recommend_query
pads them: -1 / -inf behind a row's count.
"""
import numpy as np


def _prepare(scores, users, caps, seen):
    """(users int64, caps int64, S): S = the scores with -inf over every pair that is no candidate."""
    users = np.asarray(users, dtype=np.int64)
    caps = np.asarray(caps, dtype=np.int64)
    S = np.array(scores, dtype=np.float64, copy=True)
    assert S.shape == (len(users), len(caps)) and len(set(users.tolist())) == len(users)
    assert np.isfinite(S).all()
    if seen is not None:
        for b, u in enumerate(users.tolist()):
            if seen[u]:
                S[b, np.fromiter(seen[u], dtype=np.int64, count=len(seen[u]))] = -np.inf
    S[:, caps == 0] = -np.inf
    return users, caps, S


def _padded(rows, S, n):
    """rows: per request row its items in order -> (items, scores, counts)."""
    B = len(rows)
    items = np.full((B, n), -1, dtype=np.int32)
    scores = np.full((B, n), -np.inf)
    counts = np.zeros(B, dtype=np.int32)
    for b, it in enumerate(rows):
        k = len(it)
        counts[b] = k
        items[b, :k] = it
        scores[b, :k] = S[b, it]
    return items, scores, counts


def greedy(scores, users, n, caps, seen=None):
    """The walk.  It is the definition."""
    users, caps, S = _prepare(scores, users, caps, seen)
    B, NI = S.shape
    bb, ii = np.nonzero(S != -np.inf)
    order = np.lexsort((ii, users[bb], -S[bb, ii]))
    left = np.where((caps < 0) | (caps >= B), B, caps).tolist()
    held = [0] * B
    rows = [[] for _ in range(B)]
    open_rows = B
    for b, i in zip(bb[order].tolist(), ii[order].tolist()):
        if held[b] < n and left[i] > 0:
            rows[b].append(i)
            left[i] -= 1
            held[b] += 1
            if held[b] == n:
                open_rows -= 1
                if open_rows == 0:
                    break
    return _padded(rows, S, n)


def threshold_rounds(scores, users, n, caps, seen=None, max_rounds=None):
    """The rounds of allocate.hpp -> (answer, rounds, converged, taus): taus[r] = (score, user id) per item after round
    r + 1, (-inf, -1) where no threshold was set.  After ``max_rounds`` rounds that still changed a threshold the lists
    are cut to what the last thresholds accept, and converged is False."""
    users, caps, S = _prepare(scores, users, caps, seen)
    B, NI = S.shape
    cand = S != -np.inf
    cols = np.arange(NI)
    uorder = np.argsort(-S, axis=1, kind="stable")                     # a user's order: score descending, item ascending
    by_id = np.argsort(users, kind="stable")
    iorder = by_id[np.argsort(-S[by_id], axis=0, kind="stable")]       # an item's order: score descending, user id ascending
    irank = np.empty((B, NI), dtype=np.int64)
    irank[iorder, cols[None, :]] = np.arange(B)[:, None]
    capped = (caps > 0) & (caps < B)
    thr = np.full(NI, B + 1, dtype=np.int64)                           # (u, i) is acceptable iff irank[u, i] < thr[i]
    taus, rounds, converged = [], 0, True
    while True:
        rounds += 1
        ok = np.take_along_axis(cand & (irank < thr[None, :]), uorder, axis=1)
        take = ok & (np.cumsum(ok, axis=1) <= n)                       # P_u, in the user's order
        if not capped.any():
            break
        prop = np.zeros((B, NI), dtype=bool)
        np.put_along_axis(prop, uorder, take, axis=1)
        full = np.flatnonzero(capped & (prop.sum(axis=0) >= caps))
        new = thr.copy()
        if len(full):
            r = np.where(prop[:, full], irank[:, full], B)
            kth = caps[full] - 1
            r = np.partition(r, sorted(set(kth.tolist())), axis=0)
            new[full] = r[kth, np.arange(len(full))] + 1               # the cap-th proposer stays acceptable
        changed = bool((new != thr).any())
        thr = new
        at = np.minimum(thr, B) - 1
        has = thr <= B
        taus.append((np.where(has, S[iorder[at, cols], cols], -np.inf), np.where(has, users[iorder[at, cols]], -1)))
        if not changed:
            break
        if max_rounds is not None and rounds == max_rounds:
            converged = False
            break
    keep = take & np.take_along_axis(irank < thr[None, :], uorder, axis=1)
    rows = [uorder[b][keep[b]] for b in range(B)]
    return _padded(rows, S, n), rounds, converged, taus


def loads(answer, n_items):
    """How often every item was given out."""
    items = answer[0]
    return np.bincount(items[items >= 0].astype(np.int64), minlength=n_items)


def check_feasible(answer, scores, users, n, caps, seen=None):
    """Rows of at most n distinct candidates in recommend's order, padded; no item beyond its cap."""
    users, caps, S = _prepare(scores, users, caps, seen)
    items, sc, counts = answer
    assert items.shape == sc.shape == (len(users), n) and counts.shape == (len(users),)
    for b in range(len(users)):
        k = int(counts[b])
        assert 0 <= k <= n and (items[b, k:] == -1).all() and np.isneginf(sc[b, k:]).all(), b
        it = items[b, :k].astype(np.int64)
        assert len(set(it.tolist())) == k and (S[b, it] != -np.inf).all(), b
        assert np.array_equal(sc[b, :k].view(np.uint64), S[b, it].view(np.uint64)), b
        assert (np.lexsort((it, -sc[b, :k])) == np.arange(k)).all(), b
    load = loads(answer, len(caps))
    finite = caps >= 0
    assert (load[finite] <= caps[finite]).all(), np.flatnonzero(finite & (load > caps))[:10]


def blocking_pairs(answer, scores, users, n, caps, seen=None):
    """The candidate pairs (row, item) outside the answer that both sides would rather hold: the user has room or holds
    something behind i in its order, and the item has room or is held by a user behind u in its order."""
    users, caps, S = _prepare(scores, users, caps, seen)
    B, NI = S.shape
    items, _, counts = answer
    held = np.zeros((B, NI), dtype=bool)
    for b in range(B):
        held[b, items[b, :counts[b]]] = True
    room = np.where((caps < 0) | (caps >= B), B, caps)
    cols = np.arange(NI)[None, :]
    # the worst key a side holds, or +inf / the largest id when it has room: (score, id) worse than it blocks nothing
    hs = np.where(held, S, np.inf)
    u_s = np.where(counts < n, -np.inf, hs.min(axis=1))
    u_i = np.where(counts < n, NI, np.where(held & (S == u_s[:, None]), cols, -1).max(axis=1))
    i_s = np.where(held.sum(axis=0) < room, -np.inf, hs.min(axis=0))
    i_u = np.where(held.sum(axis=0) < room, users.max() + 1, np.where(held & (S == i_s[None, :]), users[:, None], -1).max(axis=0))
    user_wants = (S > u_s[:, None]) | ((S == u_s[:, None]) & (cols < u_i[:, None]))
    item_wants = (S > i_s[None, :]) | ((S == i_s[None, :]) & (users[:, None] < i_u[None, :]))
    return np.argwhere((S != -np.inf) & ~held & user_wants & item_wants)
