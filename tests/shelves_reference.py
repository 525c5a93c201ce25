"""Category-level recommendation, restated in numpy (no GPU, no library): what mmsbm_hip_recommend_query_shelves
answers, from a matrix of scores.  Shared by test_shelves_cpu.py (which pins the forms below to each other and to the
composition of catalogue_reference.within_top_n) and test_gpu_shelves.py (which compares the device with it by equality).

The definition (literal_shelves): a row's candidates after seen / cand / extra; for category g its candidates' scores
s_1, s_2, ... in recommend_query's order (score descending, equal scores by ascending item id), a of them; a < min_items:
no candidate; else t = min(depth, a) and the value is ((s_1 + s_2) + ... + s_t) / t, added left to right in a Python loop
(never np.sum, which is pairwise) and divided once.  The row's shelves: the n_shelves largest values, equal values by
ascending category index; a shelf's items: the first min(per_shelf, a) of s_1, s_2, ...

Shelves (the class) is the same answer for many (depth, min_items, n_shelves, per_shelf) over one request and one
layout: the rows' full orders and every position's rank inside its category come from quota_reference.Walk, the values
are added one rank at a time -- step j adds every (row, category)'s j-th best score to its running sum, so each sum still
runs left to right."""
import numpy as np

import quota_reference as qr


def pack(rows, n_shelves, per_shelf):
    """rows: per request row a list of (category, value, available, items, scores) -> the device's seven arrays."""
    m = len(rows)
    cats = np.full((m, n_shelves), -1, dtype=np.int32)
    vals = np.full((m, n_shelves), -np.inf)
    avail = np.zeros((m, n_shelves), dtype=np.int32)
    counts = np.zeros(m, dtype=np.int32)
    items = np.full((m, n_shelves, per_shelf), -1, dtype=np.int32)
    scores = np.full((m, n_shelves, per_shelf), -np.inf)
    item_counts = np.zeros((m, n_shelves), dtype=np.int32)
    for b, shelves in enumerate(rows):
        counts[b] = len(shelves)
        for k, (g, v, a, it, sc) in enumerate(shelves):
            cats[b, k], vals[b, k], avail[b, k], item_counts[b, k] = g, v, a, len(it)
            items[b, k, :len(it)] = it
            scores[b, k, :len(it)] = sc
    return cats, vals, avail, counts, items, scores, item_counts


def sequential_mean(s):
    """((s[0] + s[1]) + ...) / len(s), one addition after the other."""
    acc = s[0]
    for x in s[1:]:
        acc = acc + x
    return acc / np.float64(len(s))


def literal_shelves(scores, users, category_of, n_cats, depth, min_items, n_shelves, per_shelf, cand=None, seen=None,
                    extra=None):
    """The definition, row by row and category by category.  category_of: one per item, its category or -1."""
    category_of = np.asarray(category_of, dtype=np.int64)
    rows = []
    for b, u in enumerate(np.asarray(users).tolist()):
        keep = qr._candidates(scores.shape[1], u, b, cand, seen, extra)
        found = []
        for g in range(n_cats):
            mine = keep[category_of[keep] == g]
            a = len(mine)
            if a < min_items or a == 0:
                continue
            mine = mine[np.lexsort((mine, -scores[b][mine]))]
            s = scores[b][mine]
            found.append((g, sequential_mean(s[:min(depth, a)]), a, mine[:per_shelf], s[:per_shelf]))
        found.sort(key=lambda x: (-x[1], x[0]))
        rows.append(found[:n_shelves])
    return pack(rows, n_shelves, per_shelf)


class Shelves:
    """One request (scores, users, cand, seen, extra as catalogue_reference.within_top_n) and one layout."""

    def __init__(self, scores, users, category_of, n_cats, cand=None, seen=None, extra=None, walk=None):
        self.walk = qr.Walk(scores, users, cand, seen, extra) if walk is None else walk
        self.G = int(n_cats)
        order, valid = self.walk.order, self.walk.valid
        c, rank = self.walk.ranks(category_of)
        r, p = np.nonzero(valid & (c >= 0))
        self.row, self.cat, self.rank = r, c[r, p], rank[r, p]
        self.item = order[r, p]
        self.score = self.walk.scores[r, self.item]
        m = len(order)
        self.avail = np.bincount(self.row * self.G + self.cat, minlength=m * self.G).reshape(m, self.G)
        by = np.lexsort((self.rank, self.row * self.G + self.cat))                 # (row, category) runs, best first
        self.by_item, self.by_score = self.item[by], self.score[by]
        self.start = np.concatenate([[0], np.cumsum(self.avail.ravel())])[:-1].reshape(m, self.G)
        self.steps = np.argsort(self.rank, kind="stable")                          # positions by rank
        self.step_at = np.searchsorted(self.rank[self.steps], np.arange(int(self.rank.max(initial=-1)) + 2))
        self._values = {}

    def values(self, depth):
        """(rows, G): the sequential sum of the min(depth, a) best scores divided by their number; nan where a = 0."""
        if depth not in self._values:
            acc = np.zeros(self.avail.shape)
            for j in range(min(depth, len(self.step_at) - 1)):                     # the j-th best of every (row, category)
                at = self.steps[self.step_at[j]:self.step_at[j + 1]]
                r, g, s = self.row[at], self.cat[at], self.score[at]
                acc[r, g] = s if j == 0 else acc[r, g] + s
            with np.errstate(invalid="ignore", divide="ignore"):
                self._values[depth] = acc / np.minimum(depth, self.avail).astype(np.float64)
        return self._values[depth]

    def answer(self, depth, min_items, n_shelves, per_shelf, first=None):
        """first: only the request's first `first` rows (a row's answer depends on that row alone)."""
        rows = slice(0, first)
        ok = self.avail[rows] >= max(min_items, 1)
        v = np.where(ok, self.values(depth)[rows], -np.inf)
        return pick(v, ok, self.avail[rows], self.start[rows], self.by_item, self.by_score, n_shelves, per_shelf)


def pick(v, ok, avail_of, start_of, by_item, by_score, n_shelves, per_shelf):
    """The seven arrays from the values v (rows, G; -inf where not ok), the categories' candidates avail_of and where
    each (row, category)'s candidates stand, best first, in by_item / by_score (start_of)."""
    m, G = v.shape
    top = np.argsort(-v, axis=1, kind="stable")[:, :n_shelves]                     # (equal values: ascending category)
    rows = np.arange(m)[:, None]
    counts = np.minimum(ok.sum(axis=1), n_shelves).astype(np.int32)
    width = top.shape[1]
    live = np.arange(width)[None, :] < counts[:, None]
    cats = np.full((m, n_shelves), -1, dtype=np.int32)
    vals = np.full((m, n_shelves), -np.inf)
    avail = np.zeros((m, n_shelves), dtype=np.int32)
    cats[:, :width] = np.where(live, top, -1)
    vals[:, :width] = np.where(live, v[rows, top], -np.inf)
    avail[:, :width] = np.where(live, avail_of[rows, top], 0)
    items = np.full((m, n_shelves, per_shelf), -1, dtype=np.int32)
    scores = np.full((m, n_shelves, per_shelf), -np.inf)
    item_counts = np.minimum(avail, per_shelf).astype(np.int32)
    if per_shelf > 0 and len(by_item):
        take = np.arange(per_shelf)[None, None, :] < item_counts[:, :, None]
        start = np.zeros((m, n_shelves), dtype=np.int64)
        start[:, :width] = np.where(live, start_of[rows, top], 0)
        at = np.minimum(start[:, :, None] + np.arange(per_shelf)[None, None, :], len(by_item) - 1)
        items[take] = by_item[at][take]
        scores[take] = by_score[at][take]
    return cats, vals, avail, counts, items, scores, item_counts


def block_shelves(scores, users, seen, m, G, depth, min_items, n_shelves, per_shelf):
    """The definition for the layout "category g = the items [g m, (g + 1) m)" over the whole catalogue, by one sort
    inside every block (a large catalogue: no full order of a row is formed).  seen: sets by user id, or None."""
    s = np.array(scores[:, :G * m])
    if seen is not None:
        for b, u in enumerate(np.asarray(users).tolist()):
            out = np.fromiter((i for i in seen[u] if i < G * m), dtype=np.int64)
            s[b, out] = -np.inf
    blk = s.reshape(len(s), G, m)
    order = np.argsort(-blk, axis=2, kind="stable")                                # (equal scores: ascending item)
    srt = np.take_along_axis(blk, order, 2)
    a = (srt > -np.inf).sum(axis=2)
    acc = srt[:, :, 0].copy()
    for j in range(1, min(depth, m)):
        acc = np.where(j < a, acc + srt[:, :, j], acc)
    ok = a >= max(min_items, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(ok, acc / np.minimum(depth, a), -np.inf)
    start = (np.arange(len(s))[:, None] * G + np.arange(G)[None, :]) * m
    return pick(v, ok, a, start, (order + (np.arange(G) * m)[None, :, None]).ravel(), srt.ravel(), n_shelves, per_shelf)


def shelves(scores, users, category_of, n_cats, depth, min_items, n_shelves, per_shelf, cand=None, seen=None, extra=None):
    """literal_shelves' answer through Shelves."""
    return Shelves(scores, users, category_of, n_cats, cand, seen, extra).answer(depth, min_items, n_shelves, per_shelf)


def composed_shelves(scores, users, category_of, n_cats, depth, min_items, n_shelves, per_shelf, cand=None, seen=None,
                     extra=None):
    """The independent statement, from catalogue_reference.within_top_n alone: per category one within_top_n(n = all of
    it) over the category's items (its counts are `available`, its rows the shelf's order), the mean of the first
    min(depth, a) returned scores, and the host's sort."""
    import catalogue_reference as cat
    category_of = np.asarray(category_of, dtype=np.int64)
    base = np.arange(scores.shape[1]) if cand is None else np.unique(np.asarray(cand, dtype=np.int64))
    found = [[] for _ in users]
    for g in range(n_cats):
        mine = base[category_of[base] == g]
        if len(mine) == 0:
            continue
        items, vals, counts = cat.within_top_n(scores, users, len(mine), mine, seen, extra)
        for b in range(len(found)):
            a = int(counts[b])
            if a >= max(min_items, 1):
                found[b].append((g, sequential_mean(vals[b, :min(depth, a)]), a, items[b, :min(per_shelf, a)],
                                 vals[b, :min(per_shelf, a)]))
    return pack([sorted(f, key=lambda x: (-x[1], x[0]))[:n_shelves] for f in found], n_shelves, per_shelf)


NAMES = ("categories", "values", "available", "counts", "items", "scores", "item_counts")
