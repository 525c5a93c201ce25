"""Group recommendation restated in numpy (no GPU, no library): what mmsbm_hip_recommend_query_groups answers, from a
matrix of scores.  Shared by test_group_cpu.py (which pins it on hand-made matrices and drives the host class with it)
and test_gpu_group.py (which compares the device with it by equality).

A group's value of an item aggregates the members' scores -- "min" (least misery), "max" (most pleasure), "count" (the
members whose score is >= bar, as a double) or "mean" (numpy's mean over the members: the device's MEAN is the score of
the mean row, equal to it up to rounding only).  Candidates: `cand` without every item ANY member has seen.  Order:
value descending, equal values by ascending item id (catalogue_reference._row)."""
import numpy as np

from catalogue_reference import _row, pack

MODES = ("min", "max", "count", "mean")


def aggregate(rows, mode, bar=0.0):
    """The group's value per item from its members' score rows (members x items), members >= 1."""
    rows = np.asarray(rows, dtype=np.float64)
    if mode == "min":
        return rows.min(axis=0)
    if mode == "max":
        return rows.max(axis=0)
    if mode == "count":
        return (rows >= bar).sum(axis=0).astype(np.float64)
    if mode == "mean":
        return rows.mean(axis=0)
    raise ValueError(mode)


def group_top_n(scores, offsets, members, n, mode, bar=0.0, cand=None, seen=None):
    """(items (G, n) padded with -1, values (G, n) padded with -inf, counts (G,)): row g = the n best items of `cand`
    (ids, None: every column of `scores`) by the aggregate of scores[members[offsets[g]:offsets[g + 1]]] -- `scores` has
    one row per USER ID --, without the union of seen[m] over the members (sets by user id, or None).  A group without
    members has no entry."""
    scores = np.asarray(scores, dtype=np.float64)
    base = np.arange(scores.shape[1]) if cand is None else np.unique(np.asarray(cand, dtype=np.int64))
    rows = []
    for g in range(len(offsets) - 1):
        mem = np.asarray(members[offsets[g]:offsets[g + 1]], dtype=np.int64)
        if len(mem) == 0:
            rows.append((np.zeros(0, dtype=np.int64), np.zeros(0)))
            continue
        out = set() if seen is None else set().union(*(seen[m] for m in mem.tolist()))
        keep = base[~np.isin(base, np.fromiter(out, dtype=np.int64, count=len(out)))]
        rows.append(_row(aggregate(scores[mem], mode, bar), keep, n))
    return pack(rows, n)
