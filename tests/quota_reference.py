"""Per-category caps on a top-N list, restated in numpy (no GPU, no library): what mmsbm_hip_recommend_query_quota
answers, from a matrix of scores.  Shared by test_quota_cpu.py (which pins the forms below to each other and to the
composition of catalogue_reference.within_top_n) and test_gpu_quota.py (which compares the device with it by equality).

The definition is the WALK (walk_top_n): a row's candidates in recommend_query's order -- score descending, equal
scores by ascending item id, after seen / cand / extra -- are walked and an item is taken unless caps[g] items of its
category g were taken before it; the walk stops after n.  An item in no category (category_of == -1) is uncapped.

Walk (the class) is the same answer for many (n, caps) over one request: the rows' full orders and every position's rank
inside its own category are computed once, then an item is kept when that rank is below the cap."""
import numpy as np

import catalogue_reference as cat


def _candidates(n_items, u, b, cand, seen, extra):
    base = np.arange(n_items) if cand is None else np.unique(np.asarray(cand, dtype=np.int64))
    out = set() if seen is None else set(seen[u])
    if extra is not None:
        out |= set(int(i) for i in extra[b])
    return base[~np.isin(base, np.fromiter(out, dtype=np.int64, count=len(out)))]


def walk_top_n(scores, users, n, category_of, caps, cand=None, seen=None, extra=None):
    """(items (M, n) padded with -1, scores (M, n) padded with -inf, counts (M,)) by the literal walk.  Arguments as
    catalogue_reference.within_top_n, plus category_of (one per item: its category or -1) and caps (one per category)."""
    category_of, caps = np.asarray(category_of, dtype=np.int64), np.asarray(caps, dtype=np.int64)
    rows = []
    for b, u in enumerate(np.asarray(users).tolist()):
        keep = _candidates(scores.shape[1], u, b, cand, seen, extra)
        order = keep[np.lexsort((keep, -scores[b][keep]))]
        taken, held = [], np.zeros(len(caps), dtype=np.int64)
        for i in order.tolist():
            if len(taken) == n:
                break
            g = category_of[i]
            if g >= 0:
                if held[g] >= caps[g]:
                    continue
                held[g] += 1
            taken.append(i)
        taken = np.asarray(taken, dtype=np.int64)
        rows.append((taken, scores[b][taken]))
    return cat.pack(rows, n)


class Walk:
    """The request rows' orders, once: rows users[b] by scores[b], candidates after cand / seen / extra as in
    within_top_n.  top: keep only the rows' best `top` candidates and everything tied with the last of them (None: all);
    an answer that would need more raises."""

    def __init__(self, scores, users, cand=None, seen=None, extra=None, top=None):
        self.scores = scores
        orders = []
        self.cut = []
        for b, u in enumerate(np.asarray(users).tolist()):
            keep = _candidates(scores.shape[1], u, b, cand, seen, extra)
            s = scores[b][keep]
            cut = top is not None and len(keep) > top
            if cut:
                keep = keep[s >= np.partition(s, len(s) - top)[len(s) - top]]
                s = scores[b][keep]
            self.cut.append(cut)
            orders.append(keep[np.lexsort((keep, -s))])
        width = max([len(o) for o in orders] + [1])
        self.order = np.full((len(orders), width), -1, dtype=np.int64)
        for b, o in enumerate(orders):
            self.order[b, :len(o)] = o
        self.valid = self.order >= 0
        self.cut = np.asarray(self.cut, dtype=bool)

    def ranks(self, category_of):
        """(category, rank inside it among the row's candidates) of every position of the orders; -1 where uncapped."""
        category_of = np.asarray(category_of, dtype=np.int64)
        c = np.where(self.valid, category_of[np.maximum(self.order, 0)], -1)
        n_rows, width = c.shape
        key = (np.arange(n_rows)[:, None] * (int(category_of.max(initial=-1)) + 2) + c + 1).ravel()
        by_key = np.argsort(key, kind="stable")                 # (positions of one (row, category) stay in order)
        sorted_key = key[by_key]
        start = np.flatnonzero(np.concatenate([[True], sorted_key[1:] != sorted_key[:-1]]))
        run = np.repeat(start, np.diff(np.concatenate([start, [len(key)]])))
        rank = np.empty(len(key), dtype=np.int64)
        rank[by_key] = np.arange(len(key)) - run
        return c, rank.reshape(n_rows, width)

    def top_n(self, n, category_of, caps, ranks=None):
        caps = np.asarray(caps, dtype=np.int64)
        c, rank = self.ranks(category_of) if ranks is None else ranks
        ok = self.valid & ((c < 0) | (rank < caps[np.maximum(c, 0)]))
        place = np.cumsum(ok, axis=1) - 1
        take = ok & (place < n)
        counts = take.sum(axis=1).astype(np.int32)
        assert not (self.cut & (counts < n)).any(), "the walk needs more than the rows' best `top` candidates"
        items = np.full((len(c), n), -1, dtype=np.int32)
        vals = np.full((len(c), n), -np.inf)
        r, p = np.nonzero(take)
        items[r, place[r, p]] = self.order[r, p]
        vals[r, place[r, p]] = self.scores[r, self.order[r, p]]
        return items, vals, counts


def quota_top_n(scores, users, n, category_of, caps, cand=None, seen=None, extra=None):
    """walk_top_n's answer through Walk."""
    return Walk(scores, users, cand, seen, extra).top_n(n, category_of, caps)


def composed_top_n(scores, users, n, category_of, caps, cand=None, seen=None, extra=None):
    """The independent statement: the n best (within_top_n) of the union of each category's own caps[g] best
    (within_top_n(n = caps[g]) over the category's items) and the uncapped items."""
    category_of, caps = np.asarray(category_of, dtype=np.int64), np.asarray(caps, dtype=np.int64)
    n_items = scores.shape[1]
    base = np.arange(n_items) if cand is None else np.unique(np.asarray(cand, dtype=np.int64))
    pools = [base[category_of[base] < 0].tolist() for _ in users]
    for g, q in enumerate(caps.tolist()):
        mine = base[category_of[base] == g]
        if q == 0 or len(mine) == 0:
            continue
        items, _, counts = cat.within_top_n(scores, users, q, mine, seen, extra)
        for b in range(len(pools)):
            pools[b].extend(items[b, :counts[b]].tolist())
    rows = [cat.within_top_n(scores[b:b + 1], [u], n, np.asarray(pools[b], dtype=np.int64), seen,
                             None if extra is None else [extra[b]]) for b, u in enumerate(np.asarray(users).tolist())]
    return tuple(np.concatenate([r[k] for r in rows]) for k in range(3))


def categories_csr(category_of, n_cats):
    """(offsets int64, items int32) of category_of: every category's items ascending."""
    category_of = np.asarray(category_of, dtype=np.int64)
    order = np.argsort(category_of, kind="stable")          # (stable: a category's items stay ascending)
    order = order[category_of[order] >= 0]
    counts = np.bincount(category_of[order], minlength=n_cats)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), order.astype(np.int32)


# ---- the category layouts both test files run ------------------------------------------------------------------------
BLOCK_SIZES = (1, 2, 63, 64, 65, 127, 128, 129)    # around the widths of a sub-wave group, a wave, two waves


def blocks(n_items, first, sizes):
    """Contiguous blocks of `sizes` items from item `first` on, one category each; the other items uncategorised."""
    c = np.full(n_items, -1, dtype=np.int64)
    at = first
    for g, m in enumerate(sizes):
        assert at + m <= n_items
        c[at:at + m] = g
        at += m
    return c


def layouts(n_items, rng):
    """name -> (category_of, number of categories)."""
    out = {}
    for G in (1, 2, 7, 64, n_items):                       # item % G; G = n_items: every category a singleton
        out[f"mod{G}"] = (np.arange(n_items) % G, G)
    out["blocks"] = (blocks(n_items, 3, BLOCK_SIZES), len(BLOCK_SIZES))
    if n_items > 1100:                                     # a block across column 1,000: the border of two selecting waves
        out["straddle"] = (blocks(n_items, 950, (100,)), 1)
    all_but = np.zeros(n_items, dtype=np.int64)
    all_but[[0, n_items // 2, n_items - 1]] = -1
    out["all_but_three"] = (all_but, 1)
    c = rng.integers(0, 23, n_items)
    c[rng.random(n_items) < 1 / 3] = -1                    # a third of the items uncategorised
    out["random"] = (c, 23)
    return out


def cap_sets(n, n_cats):
    """name -> caps: every uniform cap of the issue, and one mix of 0 / 1 / 3 per category."""
    out = {f"cap{q}": np.full(n_cats, q, dtype=np.int32) for q in sorted({0, 1, 2, n - 1, n, n + 1})}
    out["mix"] = np.asarray([(0, 1, 3)[g % 3] for g in range(n_cats)], dtype=np.int32)
    return out


def mix_absent(category_of, n_cats):
    """The mix's fourth kind: every fourth category taken out of the table (its items become uncategorised)."""
    c = np.asarray(category_of, dtype=np.int64).copy()
    c[(c >= 0) & (c % 4 == 3)] = -1
    return c
