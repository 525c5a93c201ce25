"""The numpy restatement of randomised top-N with propensities (mmsbm_amd/csrc/explore.hpp), operation by operation; no
GPU, no library.  Pinned to the Plackett-Luce distribution in test_explore_cpu.py, the reference of test_gpu_explore.py.

    r(u, i)  numpy's Generator.random() as draw number u * 2^32 + i of the PCG64 stream: bg.advance(u << 32 | i)
    g        E = -log(1 - r), E = 2^-54 where r = 0;  g = -log(E)
    key      s + T * g  (two roundings);  -inf stays -inf
    list     the n candidates of largest key, equal keys by ascending item id
    p_t      e_t / R_t,  e_i = exp((s_i - max s) / T),  R_t = the sum of e over the candidates not ranked above t
"""
import numpy as np

FLOOR = 700.0
E_AT_ZERO = 2.0 ** -54


def stream(seed):
    """A fresh PCG64 of ``np.random.default_rng(seed)``'s stream."""
    bg = np.random.PCG64()
    bg.state = np.random.default_rng(seed).bit_generator.state
    return bg


def uniform(seed, u, i):
    """r(u, i): the definition, one pair."""
    bg = stream(seed)
    bg.advance((int(u) << 32) | int(i))
    return np.random.Generator(bg).random()


def uniforms(seed, users, items):
    """r of each (user, item) pair."""
    return np.array([uniform(seed, u, i) for u, i in zip(np.asarray(users).tolist(), np.asarray(items).tolist())])


def uniform_rows(seed, users, n_items):
    """(len(users), n_items): r(u, 0 .. n_items - 1) -- consecutive draws from u * 2^32 on."""
    out = np.empty((len(users), n_items))
    for b, u in enumerate(np.asarray(users).tolist()):
        bg = stream(seed)
        bg.advance(int(u) << 32)
        out[b] = np.random.Generator(bg).random(n_items)
    return out


def gumbel(r):
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(divide="ignore"):
        E = np.where(r == 0.0, E_AT_ZERO, -np.log(1.0 - r))
    return -np.log(E)


def candidate_mask(n_rows, n_items, users, cand=None, seen=None, own=None):
    """(n_rows, n_items) bool: row b's candidates -- ``cand`` (ids; None: all), without seen[users[b]] and own[b]."""
    ok = np.zeros((n_rows, n_items), dtype=bool)
    ok[:, np.arange(n_items) if cand is None else np.asarray(cand, dtype=np.int64)] = True
    for b in range(n_rows):
        for lst in ((seen[int(users[b])] if seen is not None else ()), (own[b] if own is not None else ())):
            if len(lst):
                ok[b, np.fromiter(lst, dtype=np.int64, count=len(lst))] = False
    return ok


def row_order(s, g, T, ok):
    """The row's candidates in key order: key descending, equal keys by ascending item id."""
    idx = np.flatnonzero(ok)
    key = s[idx] + T * g[idx]                                  # (numpy rounds the product, then the sum)
    return idx[np.lexsort((idx, -key))]


def row_propensities(s, order, T, dtype=np.float64):
    """p_t of every position of ``order`` (the row's candidates in list order): R_t summed over what remains, from the
    end.  dtype longdouble: the direct form in extended precision."""
    if len(order) == 0:
        return np.zeros(0)
    sv = s[order].astype(dtype)
    e = np.exp((sv - sv.max()) / dtype(T))
    R = np.cumsum(e[::-1])[::-1]
    return (e / R).astype(np.float64)


def row_propensities_by_difference(s, order, T):
    """What explore.hpp must NOT do: R_t = the full-row sum minus the head."""
    sv = s[order]
    e = np.exp((sv - sv.max()) / T)
    with np.errstate(divide="ignore", invalid="ignore"):
        return e / (e.sum() - np.concatenate([[0.0], np.cumsum(e)[:-1]]))


def explore(scores, users, T, g, n, cand=None, seen=None, own=None):
    """(items, scores, propensity, counts) as recommend_query_explore returns them.  scores / g: (rows, items), row b
    belonging to users[b]."""
    n_rows, n_items = scores.shape
    ok = candidate_mask(n_rows, n_items, users, cand, seen, own)
    items = np.full((n_rows, n), -1, dtype=np.int32)
    out_s = np.full((n_rows, n), -np.inf)
    out_p = np.zeros((n_rows, n))
    counts = np.zeros(n_rows, dtype=np.int32)
    for b in range(n_rows):
        order = row_order(scores[b], g[b], T, ok[b])
        c = min(n, len(order))
        counts[b] = c
        items[b, :c] = order[:c]
        out_s[b, :c] = scores[b, order[:c]]
        out_p[b, :c] = row_propensities(scores[b], order, T)[:c]
    return items, out_s, out_p, counts


def list_propensity(s, ok, T, lst, dtype=np.float64):
    """(scores, propensity) of one row's given list ``lst`` (distinct ids, the order given): an item that is no
    candidate gets -inf / 0 and the rest is computed as if it were absent."""
    lst = np.asarray(lst, dtype=np.int64)
    valid = ok[lst] if len(lst) else np.zeros(0, dtype=bool)
    rest = ok.copy()
    rest[lst[valid]] = False
    order = np.concatenate([lst[valid], np.flatnonzero(rest)])     # the list, then what remains (any order: one sum)
    p = row_propensities(s, order, T, dtype)
    out_s, out_p = np.full(len(lst), -np.inf), np.zeros(len(lst))
    out_s[valid] = s[lst[valid]]
    out_p[valid] = p[:int(valid.sum())]
    return out_s, out_p


# ---- the Plackett-Luce distribution itself ------------------------------------------------------------------------------
PL_SCORES = np.array([5.0, 4.5, 4.0, 4.0, 3.0, 2.0, 1.5, 1.0])
PL_T, PL_SEED, PL_N, PL_ROWS = 0.5, 0, 3, 4096


def pl_exact(scores, T, n):
    """(first-place probability, top-n inclusion probability) of every item: the ordered n-tuples enumerated."""
    import itertools
    w = np.exp((scores - scores.max()) / T)
    first = w / w.sum()
    incl = np.zeros(len(scores))
    tuples = 0
    for tup in itertools.permutations(range(len(scores)), n):
        left, pr = w.sum(), 1.0
        for i in tup:
            pr *= w[i] / left
            left -= w[i]
        incl[list(tup)] += pr
        tuples += 1
    return first, incl, tuples


def pl_deviations(lists, scores, T, n):
    """The largest deviation of the lists' first-place and top-n inclusion frequencies from the exact probabilities, in
    standard errors of a frequency over len(lists) independent rows."""
    rows = len(lists)
    first, incl, _ = pl_exact(scores, T, n)
    f_first = np.bincount(lists[:, 0], minlength=len(scores)) / rows
    f_incl = np.bincount(lists.ravel(), minlength=len(scores)) / rows
    se = lambda p: np.sqrt(p * (1.0 - p) / rows)                                      # noqa: E731
    return float(np.max(np.abs(f_first - first) / se(first))), float(np.max(np.abs(f_incl - incl) / se(incl)))
