"""Recommendation within a part of the catalogue, restated in numpy (no GPU, no library): what
mmsbm_hip_recommend_query_within / _rank answer, from a matrix of scores.  Shared by test_catalogue_cpu.py (which pins
it to test_recommend_cpu.restate) and test_gpu_catalogue.py (which compares the device with it by equality).

Order: score descending, equal scores by ascending item id -- recommend_query's, cut to the candidates."""
import numpy as np


def _row(s, cand, n):
    """(items, scores) of the n best of candidate ids `cand` (any order, distinct) by the row of scores `s`."""
    cand = np.asarray(cand, dtype=np.int64)
    best = cand[np.lexsort((cand, -s[cand]))][:n]
    return best, s[best]


def pack(rows, n):
    items = np.full((len(rows), n), -1, dtype=np.int32)
    vals = np.full((len(rows), n), -np.inf)
    counts = np.zeros(len(rows), dtype=np.int32)
    for b, (it, sc) in enumerate(rows):
        counts[b] = len(it)
        items[b, :len(it)] = it
        vals[b, :len(it)] = sc
    return items, vals, counts


def within_top_n(scores, users, n, cand=None, seen=None, extra=None):
    """(items (M, n) padded with -1, scores (M, n) padded with -inf, counts (M,)): row b = the n best items of `cand`
    (ids, None: every column of `scores`) for user users[b] by scores[b], without seen[users[b]] (sets by user id, or
    None) and without extra[b] (one iterable per REQUEST ROW, or None)."""
    n_items = scores.shape[1]
    base = np.arange(n_items) if cand is None else np.unique(np.asarray(cand, dtype=np.int64))
    rows = []
    for b, u in enumerate(np.asarray(users).tolist()):
        out = set() if seen is None else set(seen[u])
        if extra is not None:
            out |= set(int(i) for i in extra[b])
        keep = base[~np.isin(base, np.fromiter(out, dtype=np.int64, count=len(out)))]
        rows.append(_row(scores[b], keep, n))
    return pack(rows, n)


def rank_lists(scores, users, offsets, items, n, seen=None):
    """The same triple for per-row candidate lists: row b's candidates are items[offsets[b]:offsets[b + 1]]."""
    rows = []
    for b, u in enumerate(np.asarray(users).tolist()):
        lst = np.asarray(items[offsets[b]:offsets[b + 1]], dtype=np.int64)
        if seen is not None:
            lst = lst[~np.isin(lst, np.fromiter(seen[u], dtype=np.int64, count=len(seen[u])))]
        rows.append(_row(scores[b], lst, n))
    return pack(rows, n)


def csr(lists):
    """(offsets int64, values int32) of a list of iterables."""
    lists = [np.asarray(list(x), dtype=np.int32) for x in lists]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return off, (np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, dtype=np.int32))
