"""What ``MMSBM`` offers beyond the reference's surface, as the base class it inherits: recommendation from the user's
and the item's side, nearest neighbours, diversified lists, explanations, the matching of the restarts' groups,
ranking evaluation, the fold-in of new users and items and the leave-one-out reliability of the training ratings.  Every method scores on the device, through sessions of the
model's context (``MMSBM._ctx`` / ``MMSBM._restarts``); this module holds what they share on the host: the label table
of a side (``_Side``), grouped lists (``grouped`` / ``group_slice``), the argument checks, the session holder and the
frame assembler.
"""
from __future__ import annotations

import contextlib
import math
import warnings

import numpy as np
import pandas as pd

from .encode import _columns


# ---------------------------------------------------------------------- argument checks
def check_integer(value, name, lo=None, must_be="a positive integer", got=...):
    """int(value) of an argument that has to be an integer (no bool) of at least ``lo``; otherwise the ValueError
    "<name> must be <must_be>, got <got>" (``got``: what the message shows, the value itself by default)."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or (lo is not None and value < lo):
        raise ValueError(f"{name} must be {must_be}, got {value if got is ... else got!r}")
    return int(value)


def check_finite(value, name, lo=None, must_be="a finite number", bool_too=False):
    """float(value) of an argument that has to be a finite number (no bool unless ``bool_too``) of at least ``lo``."""
    if (isinstance(value, bool) and not bool_too) or not isinstance(value, (int, float, np.integer, np.floating)) \
            or not np.isfinite(value) or (lo is not None and value < lo):
        raise ValueError(f"{name} must be {must_be}, got {value!r}")
    return float(value)


EXPLORE_FLOOR = 700.0   # (max w - min w) / temperature beyond this is refused (explore.hpp: no exp underflows below it)


def explore_temperature(temperature, weights):
    """float(temperature) of ``recommend_explore`` / ``propensities``: finite, >= 0 and, unless 0, not below the floor
    (max w - min w) / 700 of the rating ``weights`` -- the ValueError names the floor."""
    t = check_finite(temperature, "temperature", 0, "a finite number >= 0")
    spread = float(np.max(weights) - np.min(weights))
    if t > 0.0 and spread / t > EXPLORE_FLOOR:
        raise ValueError(f"temperature must be 0 or at least the floor {spread / EXPLORE_FLOOR!r} of these weights "
                         f"((max weight - min weight) / {EXPLORE_FLOOR:g}: below it the policy is recommend()'s list), "
                         f"got {t!r}")
    return t


def explore_stream(seed):
    """The four PCG64 state words (``core.pcg64_words``) of ``np.random.default_rng(seed)``: the stream that
    ``recommend_explore`` keys its noise on.  A generator is read where it stands, not advanced."""
    from .core import pcg64_words
    bg = np.random.default_rng(seed).bit_generator
    if not isinstance(bg, np.random.PCG64):
        raise ValueError(f"seed must give a PCG64 stream, got a generator on {type(bg).__name__}")
    return pcg64_words(bg)


# ---------------------------------------------------------------------- grouped lists
def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def grouped(keys, values, n_groups, sort=False, distinct=False):
    """(offsets (n_groups + 1,) int64, values int32): the ``values`` whose key is g are [offsets[g]:offsets[g + 1]], in
    input order, or ascending with ``sort``; ``distinct`` (with ``sort``) keeps one of equal values of a group."""
    keys, values = np.asarray(keys, dtype=np.int64), np.asarray(values)
    order = np.lexsort((values, keys)) if sort else np.argsort(keys, kind="stable")
    keys, values = keys[order], values[order]
    if distinct:
        new = np.ones(len(keys), dtype=bool)
        new[1:] = (keys[1:] != keys[:-1]) | (values[1:] != values[:-1])
        keys, values = keys[new], values[new]
    return _offsets(np.bincount(keys, minlength=n_groups)), values.astype(np.int32)


def group_slice(lists, b, e):
    """The groups [b, e) of ``lists`` = (offsets, values) as a list of their own (offsets from 0); None stays None."""
    if lists is None:
        return None
    off, values = lists
    return off[b:e + 1] - off[b], values[off[b]:off[e]]


# ---------------------------------------------------------------------- capped categories
class Quota:
    """The capped categories of ``recommend_quota`` in encoded terms: category g holds the items
    ``items[offsets[g]:offsets[g + 1]]`` (ascending) with cap ``caps[g]``; ``category_of`` (one per item of the side):
    the place of the item's category in ``labels`` (the caller's labels, capped or not), or -1."""

    def __init__(self, offsets, items, caps, category_of, labels):
        self.offsets, self.items, self.caps, self.category_of, self.labels = offsets, items, caps, category_of, labels

    def label(self, ids):
        """The caller's category label of each encoded item id, None where it has none."""
        table = np.empty(len(self.labels) + 1, dtype=object)
        table[:-1] = self.labels
        table[-1] = None
        return table[self.category_of[np.asarray(ids, dtype=np.int64)]]


def _category_columns(categories):
    """(item labels, categories) of a ``categories`` argument in one of its three forms; anything else: ValueError."""
    if isinstance(categories, dict):
        return list(categories.keys()), list(categories.values())
    if isinstance(categories, pd.DataFrame):
        if categories.shape[1] < 2:
            raise ValueError("categories needs two columns: items and categories")
        return categories.iloc[:, 0].tolist(), categories.iloc[:, 1].tolist()
    if isinstance(categories, pd.Series):
        return categories.index.tolist(), categories.tolist()
    raise ValueError("categories must be a dict {item: category}, a Series indexed by item or a DataFrame of "
                     f"(item, category) rows, got {type(categories).__name__}")


def category_table(categories, items):
    """A ``categories`` argument against the item table ``items`` (a ``_Side``) -> (ids, codes, labels, category_of):
    the items that have a category (encoded ids, ascending and distinct) and the place of each one's category in
    ``labels`` -- the caller's labels in order of first appearance --, and ``category_of``: one per item of the side,
    that place or -1.

    ``categories``: a dict {item label: category}, a Series indexed by item, or a DataFrame whose first two columns are
    item and category.  Items the side does not have are ignored, a missing category (None / NaN) leaves the item
    without one, an item given two different categories is a ValueError."""
    labs, cats = _category_columns(categories)
    ids = items.ids(labs)
    held = np.empty(len(cats), dtype=object)
    for j, c in enumerate(cats):
        held[j] = c
    keep = (ids >= 0) & ~np.fromiter((c is None or (isinstance(c, (float, np.floating)) and np.isnan(c)) or c is pd.NaT
                                      or c is pd.NA for c in cats), dtype=bool, count=len(cats))
    ids, (codes, labels) = ids[keep].astype(np.int64), pd.factorize(held[keep])
    order = np.lexsort((codes, ids))
    ids, codes = ids[order], codes[order]
    clash = np.flatnonzero((ids[1:] == ids[:-1]) & (codes[1:] != codes[:-1]))
    if len(clash):
        raise ValueError(f"items given two different categories: {list(dict.fromkeys(items.label(ids[clash]).tolist()))[:10]}")
    first = np.ones(len(ids), dtype=bool)
    first[1:] = ids[1:] != ids[:-1]
    ids, codes = ids[first], codes[first]
    category_of = np.full(len(items), -1, dtype=np.int64)
    category_of[ids] = codes
    return ids, codes, list(labels), category_of


def quota_categories(categories, max_per_category, items):
    """``recommend_quota``'s ``categories`` and ``max_per_category`` against the item table ``items`` (a ``_Side``; no
    context is needed) -> ``Quota``.

    ``categories``: a dict {item label: category}, a Series indexed by item, or a DataFrame whose first two columns are
    item and category.  Items the side does not have are ignored, a missing category (None / NaN) leaves the item
    uncapped, an item given two different categories is a ValueError.  ``max_per_category``: an integer >= 0 for every
    category, or a dict {category: integer >= 0} -- categories it does not name are uncapped."""
    _category_columns(categories)                                              # (its ValueError comes first)
    must_be = "an integer >= 0 or a dict {category: integer >= 0}"
    if isinstance(max_per_category, dict):
        per = {c: check_integer(v, f"max_per_category[{c!r}]", 0, "an integer >= 0") for c, v in max_per_category.items()}
        cap_of = lambda c: per.get(c, -1)                                      # noqa: E731  (-1: uncapped)
    else:
        every = check_integer(max_per_category, "max_per_category", 0, must_be)
        cap_of = lambda c: every                                               # noqa: E731
    ids, codes, labels, category_of = category_table(categories, items)
    cap = np.array([cap_of(c) for c in labels], dtype=np.int64)
    capped = np.flatnonzero(cap >= 0)
    place = np.full(len(labels), -1, dtype=np.int64)
    place[capped] = np.arange(len(capped))
    mine = place[codes] >= 0
    offsets, members = grouped(place[codes][mine], ids[mine], len(capped), sort=True)
    return Quota(offsets, members, cap[capped].astype(np.int32), category_of, labels)


def shelf_categories(categories, items):
    """``recommend_shelves``' ``categories`` (``category_table``'s forms and rules) against the item table ``items`` ->
    a ``Quota`` without caps: category g -- the g-th label in order of first appearance, which is the order that decides
    between equal shelf values -- holds the items ``items[offsets[g]:offsets[g + 1]]``."""
    ids, codes, labels, category_of = category_table(categories, items)
    offsets, members = grouped(codes, ids, len(labels), sort=True)
    return Quota(offsets, members, None, category_of, labels)


# ---------------------------------------------------------------------- capacities
def allocate_capacity(capacity, items):
    """``allocate``'s ``capacity`` against the item table ``items`` (a ``_Side``; no context is needed) -> one int32 per
    item: how often it can be given out, -1 for unlimited.

    ``capacity``: an integer >= 0 for every item, or a dict / Series {item label: integer >= 0} -- items it does not
    name are unlimited, labels the side does not have are ignored."""
    must_be = "an integer >= 0 or a dict {item: integer >= 0}"
    if isinstance(capacity, pd.Series):
        capacity = dict(zip(capacity.index.tolist(), capacity.tolist()))
    if not isinstance(capacity, dict):
        return np.full(len(items), check_integer(capacity, "capacity", 0, must_be), dtype=np.int32)
    caps = np.full(len(items), -1, dtype=np.int32)
    labs = list(capacity.keys())
    ids = items.ids(labs)
    for j, lab in zip(ids.tolist(), labs):
        q = check_integer(capacity[lab], f"capacity[{lab!r}]", 0, "an integer >= 0")
        if j >= 0:
            caps[j] = min(q, np.iinfo(np.int32).max)
    return caps


# ---------------------------------------------------------------------- labels of a side
class _Side:
    """The users, the items or the ratings of a fitted model: how many there are, the label of an id and the id of a
    label.  ``labels``: the encoder's (object array, id -> label); None after ``fit_encoded``, where an id is its own
    label (int64) and ``known`` may name the ids in use (default: all below ``size``)."""

    def __init__(self, name, size, labels=None, known=None):
        self.name, self.size, self.labels, self.known = name, size, labels, known
        self._index = None

    def __len__(self):
        return self.size

    def label(self, ids):
        """The label of each id."""
        ids = np.asarray(ids, dtype=np.int64)
        return ids if self.labels is None else self.labels[ids]

    def index(self):
        """id -> label as a pandas index takes it (None: the ids themselves)."""
        return None if self.labels is None else self.labels.tolist()

    def ids(self, labels):
        """The id (int32) of each label, -1 where the training data has none.  With an encoder a label is looked up as
        str(x) (7 and "7" are one user); without one only integers that are ids count."""
        if self.labels is not None:
            if self._index is None:
                self._index = {lab: j for j, lab in enumerate(self.labels.tolist())}
            found = [self._index.get(str(x), -1) for x in labels]
        else:
            inside = (lambda j: 0 <= j < self.size) if self.known is None else (lambda j: j in self.known)
            found = [int(x) if isinstance(x, (int, np.integer)) and inside(int(x)) else -1 for x in labels]
        return np.asarray(found, dtype=np.int32)

    def request(self, wanted):
        """(ids int32, labels) of a request for entries of the side (None: all of them).  A label the training data
        does not have: KeyError.  The labels are the encoder's, not the caller's spelling (the frames join on them)."""
        if wanted is None:
            ids = np.arange(self.size, dtype=np.int32)
            return ids, (ids if self.labels is None else self.labels)
        asked = np.asarray(list(wanted), dtype=object)
        ids = self.ids(asked)
        if (ids < 0).any():
            missing = list(dict.fromkeys(asked[ids < 0].tolist()))
            raise KeyError(f"{self.name} not in the training data: {missing}")
        return ids, (asked if self.labels is None else self.labels[ids])

    def extended(self, new_labels):
        """The side with ``new_labels`` behind it (ids size, size + 1, ...), for labelling only."""
        mine = np.arange(self.size, dtype=np.int64) if self.labels is None else self.labels
        return _Side(self.name, self.size + len(new_labels), np.concatenate([mine, new_labels]).astype(mine.dtype))


@contextlib.contextmanager
def session(ctx, kind, *begin_args):
    """ctx's ``kind`` session ("recommend", "similar", "overlap", "explain", "inform", "heldout", "loo") begun with
    ``begin_args`` around the block, ended however the block ends."""
    getattr(ctx, kind + "_begin")(*begin_args)
    try:
        yield ctx
    finally:
        getattr(ctx, kind + "_end")()


class Serving:
    """The serving methods of ``MMSBM`` (a plain base class: it relies on the model's ``_ctx``, ``_restarts``,
    ``_device_list``, ``results``, ``ratings``, ``p``, ``m``, ``data_handler`` and ``logger``)."""

    RECOMMEND_BATCH_ROWS = 1 << 22   # result rows (users x n) fetched from the device per query call
    RECOMMEND_MAX = 1024             # largest n of a top-N query (MMSBM_HIP_RECOMMEND_MAX_N)
    TOP_PAIRS_MAX = 1024             # largest m of top_pairs (MMSBM_HIP_TOP_PAIRS_MAX_M)
    DIVERSE_POOL_MAX = 1024          # largest pool of a diversified query (MMSBM_HIP_RECOMMEND_MAX_N)
    _sides = (None, {})              # (the encoder they were built from, {name: _Side})

    # ------------------------------------------------------------------ what the methods share
    def _side(self, name):
        """The label table of the model's "users", "items" or "ratings".  With an encoder it is built once and kept
        for as long as ``data_handler`` is that encoder."""
        enc = self.data_handler
        if not enc:  # (after fit_encoded: rows and ratings keep their integer ids)
            if name == "ratings":
                return _Side(name, len(self.ratings), known=self.ratings)
            return _Side(name, (self.p if name == "users" else self.m) + 1)
        if self._sides[0] is not enc:
            self._sides = (enc, {})
        if name not in self._sides[1]:
            labels = {"users": enc.user_labels, "items": enc.item_labels, "ratings": enc.rating_labels}[name]()
            self._sides[1][name] = _Side(name, len(labels), np.asarray(labels, dtype=object))
        return self._sides[1][name]

    def _check_whole_model(self):
        self._check_is_fitted()
        if len(self._restart_ids) != self.sampling:
            raise RuntimeError(
                f"this model holds {len(self._restart_ids)} of its {self.sampling} restarts (restarts.fit_distributed "
                "without gather=True): fit with gather=True to recommend from all of them")

    def _recommend_args(self, n, weights):
        return check_integer(n, "n", 1), self._rating_weights(weights)

    def _rating_weights(self, weights):
        w = np.asarray(self.ratings if weights is None else weights, dtype=np.float64)
        if w.shape != (len(self.ratings),):
            raise ValueError(f"weights has shape {w.shape}, expected ({len(self.ratings)},): one per rating value")
        if not np.isfinite(w).all():
            raise ValueError(f"weights must be finite, got {w.tolist()}")
        return w

    @staticmethod
    def _pair_columns(pairs):
        """(users, items) of a ``pairs`` argument: the first two columns of a DataFrame, or (user, item) tuples."""
        if hasattr(pairs, "iloc") and hasattr(pairs, "columns"):
            if pairs.shape[1] < 2:
                raise ValueError("pairs needs two columns: users and items")
            return pairs.iloc[:, 0].tolist(), pairs.iloc[:, 1].tolist()
        rows = [tuple(x) for x in pairs]
        if any(len(x) != 2 for x in rows):
            raise ValueError("pairs must be (user, item) tuples")
        return [x[0] for x in rows], [x[1] for x in rows]

    def _candidate_ids(self, candidates):
        """The encoded ids of ``candidates`` (item labels of the training data: KeyError otherwise), ascending and
        distinct, int32; None stays None."""
        if candidates is None:
            return None
        return np.unique(self._side("items").request(list(candidates))[0]).astype(np.int32)

    def _exclusion_lists(self, exclude, ids):
        """(offsets (len(ids) + 1,) int64, items int32): for every requested row (encoded user ``ids``) the distinct
        encoded items ``exclude`` names for that user, ascending; pairs of other users and unknown labels are dropped.
        None stays None."""
        if exclude is None:
            return None
        users = self._side("users")
        us, its = self._pair_columns(exclude)
        uid, iid = users.ids(us), self._side("items").ids(its)
        keep = (uid >= 0) & (iid >= 0)
        off, items = grouped(uid[keep], iid[keep], len(users), sort=True, distinct=True)      # every user's list ...
        counts = np.diff(off)[ids]
        mine = _offsets(counts)                                                               # ... and each row's copy
        return mine, items[np.repeat(off[ids] - mine[:-1], counts) + np.arange(mine[-1])]

    def _session_of_restarts(self, kind, *begin_args):
        """The context, with its ``kind`` session ("recommend", "similar", "overlap", "explain") begun with
        ``begin_args`` and every restart the model holds added to it, around the block; the session is ended however
        the block ends."""
        return self._sessions_of_restarts((kind, *begin_args))

    @contextlib.contextmanager
    def _sessions_of_restarts(self, *sessions):
        """_session_of_restarts for several kinds at once: ``sessions`` are (kind, *begin_args); every restart the model
        holds is selected ONCE and added to each of them in that order, so they hold the same slots in the same order.
        Every session begun is ended however the block ends."""
        ctx, restarts = self._restarts()
        with contextlib.ExitStack() as stack:
            for kind, *begin_args in sessions:
                stack.enter_context(session(ctx, kind, *begin_args))
            for _ in restarts:
                for kind, *_args in sessions:
                    getattr(ctx, kind + "_add")()
            yield ctx

    def _row_batches(self, n_rows, n):
        """[b, e) of request rows with at most RECOMMEND_BATCH_ROWS result rows (``n`` per request row) each."""
        step = max(1, self.RECOMMEND_BATCH_ROWS // n)
        return ((b, min(n_rows, b + step)) for b in range(0, n_rows, step))

    @staticmethod
    def _frame(rows, columns, batches, query, n=0):
        """The frame of a request answered batch by batch (bounded host memory at a million users), one line per entry
        of a request row.  ``rows``: {column: its label for every request row}, the leading columns.  ``columns``:
        {column: how it is made}, in frame order: a ``_Side`` (ids from ``query``, shown as that side's labels), None
        (numbers from ``query``; "rank": 1 = the row's first entry, numbered here unless ``query`` does) or a function
        of the batch's {column: entries from ``query``}.  ``query(*batch)`` for every batch (b, e, ...) of ``batches``
        -> (entries of each row (e - b,), {column: (e - b, n) padded behind a row's entries | (e - b, 1) one per row |
        (entries,) one per entry, rows in order; "row": each entry's row, from 0, where ``query`` has it anyway}).  No
        batch: the empty frame with the same columns."""
        parts = []
        for batch in batches:
            b, e = batch[:2]
            counts, got = query(*batch)
            at = got.pop("row") if "row" in got else np.repeat(np.arange(e - b), counts)
            keep = np.arange(n)[None, :] < counts[:, None]
            got = {c: v if v.ndim == 1 else np.broadcast_to(v, keep.shape)[keep] for c, v in got.items()}
            got.setdefault("rank", np.nonzero(keep)[1].astype(np.int64) + 1)
            part = {c: v[b:e][at] if len(at) else np.empty(0, dtype=object) for c, v in rows.items()}
            for c, how in columns.items():
                part[c] = how.label(got[c]) if isinstance(how, _Side) else got[c] if how is None else how(got)
            parts.append(pd.DataFrame(part))
        if parts:
            return pd.concat(parts, ignore_index=True)
        empty = {c: [] if isinstance(how, _Side) else np.zeros(0, dtype=np.int64 if c == "rank" else np.float64)
                 for c, how in columns.items()}
        return pd.DataFrame({**{c: [] for c in rows}, **empty})

    def _top_n_frame(self, query, n, row_labels, side, columns=("users", "items", "score"), derived=None):
        """The top-``n`` frame (users, items, score, rank) of rows [0, len(row_labels)), fetched in calls of at most
        RECOMMEND_BATCH_ROWS result rows: ``query(b, e)`` -> (ids, values, ..., counts) of rows [b, e), each (e - b, n)
        but the counts.  ``side``: the ``_Side`` of the returned ids.  ``columns``: the names of the row, the
        returned-id and the value columns (similar_items / similar_users; recommend_diverse has two value columns).
        ``derived``: {column: function of the returned ids} of columns behind ``rank`` (recommend_quota's category)."""
        def entries(b, e):
            *padded, counts = query(b, e)
            return counts, dict(zip(columns[1:], padded))
        made = {columns[1]: side, **dict.fromkeys(columns[2:]), "rank": None}
        for name, of_ids in (derived or {}).items():
            made[name] = lambda got, of_ids=of_ids: of_ids(got[columns[1]])
        frame = self._frame({columns[0]: row_labels}, made, self._row_batches(len(row_labels), n), entries, n)
        return frame.astype(dict.fromkeys(derived, object)) if derived and not len(frame) else frame

    # ------------------------------------------------------------------ recommendation (not in the reference)
    def recommend(self, users=None, n=10, exclude_seen=True, weights=None, candidates=None, exclude=None):
        """The ``n`` best items per user, scored on the device: score(u, i) = sum_r weights[r] P(r | u, i), mean over
        the restarts the model holds -- with the default weights (the rating values, ``self.ratings``) the expected
        rating that ``predict`` + ``score`` use.  Candidates are all training items, without the user's own training
        items when ``exclude_seen``.  Order: score descending, equal scores by ascending encoded item id.

        ``candidates``: an iterable of item labels -- the items in stock, of one category, released this week; only
        they are scored and ranked (duplicates count once; a label that is not in the training data: KeyError; an
        empty one: an empty frame).  ``exclude``: further (user, item) pairs to leave out -- shown, dismissed, bought
        elsewhere -- as a DataFrame whose first two columns are users and items or an iterable of (user, item) tuples;
        pairs of users that are not requested, and pairs with a user or an item that is not in the training data, are
        ignored.  Scores and order are those of the plain call: the answer is its list for n = all items, filtered.

        Returns a DataFrame with columns ``users``, ``items``, ``score``, ``rank`` (1 = best), users in request order
        (``users=None``: every training user), users and items as the encoder's labels (``theta`` / ``eta``'s index).  The model's stored predictions and
        ``score()`` are left as they are."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        ids, labels = self._side("users").request(users)
        items = self._side("items")
        if candidates is None and exclude is None:
            with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
                return self._top_n_frame(lambda b, e: ctx.recommend_query(ids[b:e], n), n, labels, items)
        cand = self._candidate_ids(candidates)
        if cand is not None and len(cand) == 0:
            return self._top_n_frame(None, n, labels[:0], items)
        extra = self._exclusion_lists(exclude, ids)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            return self._top_n_frame(
                lambda b, e: ctx.recommend_query_within(ids[b:e], n, cand, group_slice(extra, b, e)), n, labels, items)

    def recommend_quota(self, users=None, n=10, categories=..., max_per_category=..., exclude_seen=True, weights=None,
                        candidates=None, exclude=None):
        """``recommend`` with a hard cap per category: at most ``max_per_category`` items of one category in a user's
        list -- two per brand, one sponsored item, none of a category that is blocked (cap 0).  The definition: the
        user's full order of ``recommend`` (score descending, equal scores by ascending encoded item id; the user's own
        items, ``candidates`` and ``exclude`` applied first) is walked and an item taken unless its category is full,
        until ``n`` are taken.  Exact at any catalogue size and on the device: nothing is over-fetched or tuned.

        ``categories`` (required): a dict {item label: category}, a Series indexed by item, or a DataFrame whose first
        two columns are item and category.  Items that are not training items are ignored (a shop's table is larger
        than the model); an item it does not name, or whose category is None / NaN, is uncapped; an item given two
        different categories: ValueError.  ``max_per_category`` (required): an integer >= 0 for every category, or a
        dict {category: integer >= 0} -- categories it does not name are uncapped.  The other arguments are
        ``recommend``'s.

        Returns ``recommend``'s frame (``users``, ``items``, ``score``, ``rank``) plus ``category``: the caller's label
        of the item's category, or None.  Scores are ``recommend``'s, bit for bit; users in request order.  The
        model's stored predictions and ``score()`` are left as they are."""
        if categories is ... or max_per_category is ...:
            raise TypeError("recommend_quota needs categories= and max_per_category=")
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        ids, labels = self._side("users").request(users)
        items = self._side("items")
        quota = quota_categories(categories, max_per_category, items)
        cand = self._candidate_ids(candidates)
        derived = {"category": quota.label}
        if cand is not None and len(cand) == 0:
            return self._top_n_frame(None, n, labels[:0], items, derived=derived)
        extra = self._exclusion_lists(exclude, ids)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            return self._top_n_frame(
                lambda b, e: ctx.recommend_query_quota(ids[b:e], n, quota.offsets, quota.items, quota.caps, cand,
                                                       group_slice(extra, b, e)), n, labels, items, derived=derived)

    def recommend_explore(self, users=None, n=10, temperature=..., seed=0, exclude_seen=True, weights=None,
                          candidates=None, exclude=None):
        """``recommend`` drawn at random, with the probability of what was drawn: every other query returns the same
        list on every call, so the items just below the cut are never shown and nothing logged under it can evaluate
        another policy.  Each user's list is sampled WITHOUT replacement from the Plackett-Luce distribution over the
        user's candidates (``recommend``'s: ``exclude_seen``, ``candidates``, ``exclude``) with utilities
        score / ``temperature``: the first item with probability proportional to exp(score / temperature), the next
        one among the rest in the same way, and so on.  On the device: Gumbel noise keyed by (seed, user, item) alone
        is added to the scores and the n largest are taken, so a user's list does not depend on the other users of the
        call, the request order, ``n`` of a longer call's head, or the catalogue's size.

        ``temperature`` is required: it is in score units, so no default fits every weighting.  0 gives
        ``recommend``'s frame with propensity 1.0; it may not lie below (max weight - min weight) / 700 otherwise
        (ValueError naming that floor: below it the policy IS ``recommend`` to within 1e-300).  ``seed``: anything
        ``np.random.default_rng`` accepts (a PCG64 stream; a generator is read, not advanced).

        Returns ``recommend``'s frame plus ``propensity`` -- the probability the policy had of putting that item at
        that rank given the ranks above it; the product over a user's rows is the probability of the list: columns
        ``users``, ``items``, ``score``, ``propensity``, ``rank``.  ``score`` is ``recommend``'s, bit for bit.
        ``propensities`` re-derives the column for any logged frame.  The model's stored predictions and ``score()``
        are left as they are."""
        if temperature is ...:
            raise TypeError("recommend_explore() needs temperature=: score units (0: plain recommend)")
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        t = explore_temperature(temperature, w)
        columns = ("users", "items", "score", "propensity")
        if t == 0.0:
            frame = self.recommend(users, n, exclude_seen, weights, candidates, exclude)
            frame.insert(3, "propensity", np.ones(len(frame)))
            return frame
        words = explore_stream(seed)
        ids, labels = self._side("users").request(users)
        items = self._side("items")
        cand = self._candidate_ids(candidates)
        if cand is not None and len(cand) == 0:
            return self._top_n_frame(None, n, labels[:0], items, columns)
        extra = self._exclusion_lists(exclude, ids)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            return self._top_n_frame(
                lambda b, e: ctx.recommend_query_explore(ids[b:e], n, t, words, cand, group_slice(extra, b, e)),
                n, labels, items, columns)

    def propensities(self, recs, temperature=..., exclude_seen=True, weights=None, candidates=None, exclude=None):
        """What ``recommend_explore``'s policy at ``temperature`` WOULD have given lists that somebody else logged --
        another temperature, an older model, a deterministic list: the number inverse-propensity scoring divides by.
        ``recs``: any recommend-style frame, users and items in its first two columns (both must be in the training
        data: KeyError); a user's list is its rows in ``rank`` order when the frame has a ``rank`` column, in order of
        appearance otherwise (at most 1,024 items, none twice).  ``exclude_seen``, ``weights``, ``candidates`` and
        ``exclude`` describe the policy's candidates as in ``recommend_explore``.

        Returns ``users``, ``items``, ``rank`` (the place in the list as given, from 1), ``score``, ``propensity``,
        users in order of first appearance.  An item the policy could not have shown that user (seen, excluded, no
        candidate) has propensity 0 and score -inf, and the rest of the list is computed as if it were absent.  No
        noise is involved: applied to ``recommend_explore``'s own frame with the same arguments it returns that
        frame's ``propensity``, bit for bit."""
        if temperature is ...:
            raise TypeError("propensities() needs temperature=: the policy's, in score units")
        self._check_whole_model()
        w = self._rating_weights(weights)
        t = explore_temperature(temperature, w)
        if t == 0.0:
            raise ValueError("temperature must be > 0: at 0 the policy is recommend()'s list, with propensity 1 on it "
                             "and 0 elsewhere")
        if not (hasattr(recs, "iloc") and hasattr(recs, "columns")) or recs.shape[1] < 2:
            raise ValueError("recs must be a frame whose first two columns are users and items")
        users_side, items_side = self._side("users"), self._side("items")
        uid, _ = users_side.request(recs.iloc[:, 0].tolist())
        iid, _ = items_side.request(recs.iloc[:, 1].tolist())
        users, first = np.unique(uid, return_index=True)
        users = users[np.argsort(first, kind="stable")].astype(np.int32)          # order of first appearance
        place = np.empty(len(users_side), dtype=np.int64)
        place[users] = np.arange(len(users))
        row = place[uid]
        order = (np.lexsort((np.asarray(recs["rank"]), row)) if "rank" in recs.columns
                 else np.argsort(row, kind="stable"))
        row, listed = row[order], iid[order].astype(np.int32)
        offsets = _offsets(np.bincount(row, minlength=len(users)))
        if len(users) and int(np.diff(offsets).max()) > self.RECOMMEND_MAX:
            raise ValueError(f"a user's list holds {int(np.diff(offsets).max())} items: at most {self.RECOMMEND_MAX}")
        pair = np.sort(row * len(items_side) + listed)
        if (pair[1:] == pair[:-1]).any():
            raise ValueError("recs names an item twice for one user")
        rank = np.arange(len(row), dtype=np.int64) - offsets[row] + 1
        score, prop = np.full(len(row), -np.inf), np.zeros(len(row))
        cand = self._candidate_ids(candidates)
        if len(users) and (cand is None or len(cand)):
            extra = self._exclusion_lists(exclude, users)
            with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
                for b, e in self._row_batches(len(users), self.RECOMMEND_MAX):
                    at = slice(offsets[b], offsets[e])
                    score[at], prop[at] = ctx.recommend_list_propensity(
                        users[b:e], group_slice((offsets, listed), b, e), t, cand, group_slice(extra, b, e))
        return pd.DataFrame({"users": users_side.label(users)[row], "items": items_side.label(listed), "rank": rank,
                             "score": score, "propensity": prop})

    def _shelves_frame(self, query, shelves, per_shelf, row_labels, cats):
        """The frame of a shelves query of rows [0, len(row_labels)): ``query(b, e)`` -> HipEM.recommend_query_shelves'
        tuple for rows [b, e); ``cats``: the ``Quota`` whose labels name the returned category indices.  per_shelf 0:
        one line per shelf (users, category, score, available, rank), else one per item of a shelf (users, category,
        shelf, shelf_score, available, items, score, rank)."""
        table = np.empty(len(cats.labels) + 1, dtype=object)
        table[:-1] = cats.labels

        def entries(b, e):
            sc, sv, sa, cnt, it, s, ic = query(b, e)
            live = np.arange(shelves)[None, :] < cnt[:, None]                        # (rows, shelves)
            if per_shelf == 0:
                r, k = np.nonzero(live)
                return cnt, {"row": r, "category": table[sc[r, k]], "score": sv[r, k], "available": sa[r, k],
                             "rank": k.astype(np.int64) + 1}
            r, k, j = np.nonzero(live[:, :, None] & (np.arange(per_shelf)[None, None, :] < ic[:, :, None]))
            return cnt, {"row": r, "category": table[sc[r, k]], "shelf": k.astype(np.int64) + 1, "shelf_score": sv[r, k],
                         "available": sa[r, k], "items": it[r, k, j], "score": s[r, k, j], "rank": j.astype(np.int64) + 1}
        if per_shelf == 0:
            columns = dict.fromkeys(("category", "score", "available", "rank"))
        else:
            columns = {**dict.fromkeys(("category", "shelf", "shelf_score", "available")), "items": self._side("items"),
                       "score": None, "rank": None}
        frame = self._frame({"users": row_labels}, columns, self._row_batches(len(row_labels), shelves * max(per_shelf, 1)),
                            entries)
        if not len(frame):
            ints = [c for c in ("shelf", "available", "rank") if c in frame]
            frame = frame.astype({"category": object, **dict.fromkeys(ints, np.int64)})
        return frame

    @staticmethod
    def _shelves_args(shelves, per_shelf, depth, min_items, name="shelves"):
        """(shelves, per_shelf, depth, min_items) checked as integers >= 1; per_shelf None: no item lists (0 to the
        device); depth None: per_shelf."""
        shelves = check_integer(shelves, name, 1)
        per_shelf = 0 if per_shelf is None else check_integer(per_shelf, "per_shelf", 1)
        depth = per_shelf if depth is None and per_shelf else check_integer(depth, "depth", 1)
        return shelves, per_shelf, depth, check_integer(min_items, "min_items", 1)

    def recommend_shelves(self, users=None, shelves=5, per_shelf=10, categories=..., depth=None, min_items=1,
                          exclude_seen=True, weights=None, candidates=None, exclude=None):
        """Which categories to show each user, and what to put on them: the rows of a front page ("Thrillers", "Brand
        X", "New this week"), each holding that user's best items of one category.  Over ``recommend``'s candidates
        (the user's own items, ``candidates`` and ``exclude`` applied first) and scores, a category's value for a user
        is the mean of its ``depth`` best candidates' scores (of all of them when it has fewer; ``depth=None``:
        ``per_shelf``; ``depth=1``: its best item's score), added best first; a category with fewer than ``min_items``
        candidates is not shown.  The user's shelves are the ``shelves`` categories of largest value -- equal values in
        the order in which the categories first appear in ``categories`` -- and a shelf's items its ``per_shelf`` best.
        One query on the device: no users x categories x depth table is formed.

        ``categories`` (required): ``recommend_quota``'s three forms with its rules -- unknown items are ignored, an
        item it does not name or whose category is None / NaN is on no shelf, an item given two different categories:
        ValueError.  The other arguments are ``recommend``'s.

        Returns a DataFrame with columns ``users``, ``category``, ``shelf`` (1 = best), ``shelf_score``, ``available``
        (the category's candidates for the user), ``items``, ``score``, ``rank`` (1 = best inside the shelf): one line
        per item of a shelf, users in request order.  Scores are ``recommend``'s, bit for bit.  The model's stored
        predictions and ``score()`` are left as they are."""
        if categories is ...:
            raise TypeError("recommend_shelves needs categories=")
        per_shelf = check_integer(per_shelf, "per_shelf", 1)                   # (no item lists: recommend_categories)
        shelves, per_shelf, depth, min_items = self._shelves_args(shelves, per_shelf, depth, min_items)
        return self._recommend_shelves(users, shelves, per_shelf, categories, depth, min_items, exclude_seen, weights,
                                       candidates, exclude)

    def recommend_categories(self, users=None, n=5, categories=..., depth=10, min_items=1, exclude_seen=True,
                             weights=None, candidates=None, exclude=None):
        """The ``n`` best categories per user without their items: ``recommend_shelves`` with no item lists.  Returns a
        DataFrame with columns ``users``, ``category``, ``score`` (the category's value: the mean of the user's
        ``depth`` best candidates of it), ``available``, ``rank`` (1 = best)."""
        if categories is ...:
            raise TypeError("recommend_categories needs categories=")
        n, _, depth, min_items = self._shelves_args(n, None, depth, min_items, "n")
        return self._recommend_shelves(users, n, 0, categories, depth, min_items, exclude_seen, weights, candidates, exclude)

    def _recommend_shelves(self, users, shelves, per_shelf, categories, depth, min_items, exclude_seen, weights,
                           candidates, exclude):
        self._check_whole_model()
        w = self._rating_weights(weights)
        ids, labels = self._side("users").request(users)
        cats = shelf_categories(categories, self._side("items"))
        cand = self._candidate_ids(candidates)
        if cand is not None and len(cand) == 0:
            return self._shelves_frame(None, shelves, per_shelf, labels[:0], cats)
        extra = self._exclusion_lists(exclude, ids)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            return self._shelves_frame(
                lambda b, e: ctx.recommend_query_shelves(ids[b:e], cats.offsets, cats.items, depth, min_items, shelves,
                                                         per_shelf, cand, group_slice(extra, b, e)),
                shelves, per_shelf, labels, cats)

    def allocate(self, n=1, capacity=..., users=None, exclude_seen=True, weights=None, candidates=None,
                 max_rounds=10000):
        """``recommend`` when items run out: every requested user asks for ``n`` items and item i can be given out
        ``capacity[i]`` times -- units in stock, papers per reviewer, coupons per product, a tutor's free slots.  It is
        the one constraint that couples the users of a request, so no filter over ``recommend`` emulates it.  The
        definition: all candidate (user, item) pairs of the request are walked in ``top_pairs``' order (score
        descending, equal scores by ascending encoded user id, then item id) and a pair is taken iff its user holds fewer
        than ``n`` items and its item is not used up.  The result is the one stable assignment: no user and item left
        that would both rather have each other.  On the device it is reached by rounds of deferred acceptance over the
        user-side and the item-side top-N, without sorting the pairs.

        ``capacity`` (required): an integer >= 0 for every item, or a dict / Series {item label: integer >= 0} -- items
        it does not name are unlimited, labels that are not training items are ignored; 0 takes an item out.
        ``users``: distinct labels (None: every training user).  ``candidates``: only these items are given out (every
        other item gets capacity 0).  ``max_rounds``: the rounds after which the device stops; the answer is then
        feasible (nobody above ``n``, no item above its capacity) but not the walk's, and a RuntimeWarning says so.

        Returns ``recommend``'s frame (``users``, ``items``, ``score``, ``rank``), users in request order; a user may
        get fewer than ``n`` rows.  Scores are ``recommend``'s, bit for bit; with nothing capped the frame IS
        ``recommend``'s.  ``self.allocation_`` = {"rounds", "converged", "filled", "requested"}: the rounds taken,
        whether they reached the fixed point, the rows returned and users x n.  ``item_load`` counts a frame's items."""
        if capacity is ...:
            raise TypeError("allocate needs capacity=")
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        max_rounds = check_integer(max_rounds, "max_rounds", 1)
        ids, labels = self._side("users").request(users)
        if len(np.unique(ids)) != len(ids):
            raise ValueError("users must be distinct: capacity couples the users of a request, not its rows")
        items = self._side("items")
        caps = allocate_capacity(capacity, items)
        cand = self._candidate_ids(candidates)
        if cand is not None:
            inside = np.zeros(len(items), dtype=bool)
            inside[cand] = True
            caps[~inside] = 0
        self.allocation_ = {"rounds": 0, "converged": True, "filled": 0, "requested": len(ids) * n}
        if len(ids) == 0:
            return self._top_n_frame(None, n, labels[:0], items)

        def whole(b, e):   # (one call: the users of a request cannot be split)
            got_items, scores, counts, info = ctx.recommend_allocate(ids, n, caps, max_rounds)
            self.allocation_.update(info, filled=int(counts.sum()))
            return counts, {"items": got_items, "score": scores}
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            frame = self._frame({"users": labels}, {"items": items, "score": None, "rank": None}, [(0, len(ids))], whole, n)
        if not self.allocation_["converged"]:
            warnings.warn(f"allocate stopped after max_rounds = {max_rounds} rounds before the fixed point: the "
                          "assignment is feasible but not the stable one", RuntimeWarning, stacklevel=2)
        return frame

    @staticmethod
    def item_load(recs):
        """How often each item appears in a recommend-style frame (any frame with an ``items`` column): a DataFrame
        ``items``, ``count``, the most used first, equal counts in order of first appearance.  What to look at before
        and after ``allocate``."""
        codes, found = pd.factorize(np.asarray(recs["items"], dtype=object))
        count = np.bincount(codes, minlength=len(found)).astype(np.int64)
        order = np.argsort(-count, kind="stable")
        return pd.DataFrame({"items": np.asarray(found, dtype=object)[order], "count": count[order]})

    def assign(self, capacity=..., epsilon=None, reserve=None, users=None, exclude_seen=True, weights=None,
               candidates=None, max_rounds=10000):
        """The assignment of largest total score under ``allocate``'s capacities: every requested user gets at most one
        item, item i at most ``capacity[i]`` users, and  sum of the assigned scores + (unassigned users) x ``reserve``
        is the largest possible, within (assigned users) x ``epsilon``.  Papers to reviewers, coupons to customers,
        stock to a mailing.  ``allocate`` gives the one stable assignment (nobody envies anybody) and spends the good
        items on whoever comes first; this one maximises the sum, and prices every item: the price is what one more
        unit of it is worth in score units.  On the device it is a forward auction: users without an item bid for their
        best item at the current prices, an item keeps its highest bids, and who is outbid bids again.

        ``capacity`` (required) and ``candidates``: as ``allocate``'s.  ``epsilon`` (required): the bidding step, in
        score units -- smaller is closer to the optimum and takes more rounds.  ``reserve``: what an unassigned user
        counts; a user whose every candidate is worth less at the final prices stays out.  None: min(weights) - span
        (span = max(weights) - min(weights), or 1), below every score, so that any candidate beats staying out.
        ``users``: distinct labels (None: every training user).  ``max_rounds``: the rounds after which the device stops
        (RuntimeWarning); the assignment is then feasible and ``bound`` still holds.

        Returns ``recommend``'s frame (``users``, ``items``, ``score``, ``rank`` = 1) plus ``price``, what the user's
        slot costs; unassigned users have no row.  Scores are ``recommend``'s, bit for bit; with nothing capped the frame
        is ``recommend(n=1)``'s for every user whose best score exceeds ``reserve``.  ``self.assignment_``: ``rounds``,
        ``bids``, ``converged``, ``assigned``, ``dropped``, ``total`` (the sum of the scores), ``value`` (with the
        reserve), ``bound`` (no assignment is worth more), ``gap_limit`` = assigned x epsilon, and ``prices``: a frame
        ``items``, ``price``, ``load``, ``capacity`` of the capped items.  Not covered: more than one item per user,
        ``exclude=`` pairs, folded-in users, epsilon-scaling, capacities above 1,024 that bind."""
        if capacity is ...:
            raise TypeError("assign needs capacity=")
        if epsilon is None:
            raise TypeError("assign needs epsilon=")
        self._check_whole_model()
        _, w = self._recommend_args(1, weights)
        max_rounds = check_integer(max_rounds, "max_rounds", 1)
        span = float(w.max() - w.min())
        if isinstance(epsilon, (bool, np.bool_)) or not isinstance(epsilon, (int, float, np.integer, np.floating)) \
                or not np.isfinite(epsilon) or not epsilon > 0 or epsilon < span * 2.0 ** -40:
            raise ValueError(f"epsilon must be a finite number > 0 and >= (max - min weight) x 2^-40, got {epsilon!r}")
        if reserve is None:
            reserve = float(w.min()) - (span if span > 0 else 1.0)
        elif isinstance(reserve, (bool, np.bool_)) or not isinstance(reserve, (int, float, np.integer, np.floating)) \
                or np.isnan(reserve) or reserve == np.inf:
            raise ValueError(f"reserve must be a number below +inf, got {reserve!r}")
        epsilon, reserve = float(epsilon), float(reserve)
        ids, labels = self._side("users").request(users)
        if len(np.unique(ids)) != len(ids):
            raise ValueError("users must be distinct: capacity couples the users of a request, not its rows")
        items = self._side("items")
        caps = allocate_capacity(capacity, items)
        cand = self._candidate_ids(candidates)
        if cand is not None:
            inside = np.zeros(len(items), dtype=bool)
            inside[cand] = True
            caps[~inside] = 0
        binding = np.flatnonzero((caps >= 0) & (caps < len(ids)))
        self.assignment_ = {"rounds": 0, "bids": 0, "converged": True, "assigned": 0, "dropped": 0, "total": 0.0,
                            "value": math.fsum([reserve] * len(ids)) if len(ids) else 0.0,
                            "bound": math.fsum([reserve] * len(ids)) if len(ids) else 0.0, "gap_limit": 0.0,
                            "prices": pd.DataFrame({"items": items.label(binding), "price": np.zeros(len(binding)),
                                                    "load": np.zeros(len(binding), dtype=np.int64),
                                                    "capacity": caps[binding].astype(np.int64)})}
        columns = {"items": items, "score": None, "rank": None, "price": None}
        if len(ids) == 0:
            return self._frame({"users": labels[:0]}, columns, [], None, 1)

        def whole(b, e):   # (one call: the users of a request cannot be split)
            got = ctx.recommend_assign(ids, caps, reserve, epsilon, max_rounds)
            has = got["items"] >= 0
            scores = got["scores"][has].tolist()
            self.assignment_.update(
                rounds=got["rounds"], bids=got["bids"], converged=got["converged"], assigned=int(has.sum()),
                dropped=int((~has).sum()), total=math.fsum(scores),
                value=math.fsum(scores + [reserve] * int((~has).sum())),
                bound=math.fsum(got["pi"].tolist() + got["price_sum"][binding].tolist()),
                gap_limit=int(has.sum()) * epsilon)
            self.assignment_["prices"] = pd.DataFrame({
                "items": items.label(binding), "price": got["price"][binding],
                "load": got["load"][binding].astype(np.int64), "capacity": caps[binding].astype(np.int64)})
            return has.astype(np.int64), {"items": got["items"][:, None], "score": got["scores"][:, None],
                                          "price": got["paid"][:, None]}
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            frame = self._frame({"users": labels}, columns, [(0, len(ids))], whole, 1)
        if not self.assignment_["converged"]:
            warnings.warn(f"assign stopped after max_rounds = {max_rounds} rounds with users still bidding: the "
                          "assignment is feasible, and assignment_['bound'] holds, but the gap may exceed gap_limit",
                          RuntimeWarning, stacklevel=2)
        return frame

    def rerank(self, pairs, n=None, exclude_seen=True, weights=None):
        """The order of caller-given candidates per user -- the second stage of a two-stage system: a cheap retriever
        proposes a few hundred items per user, the model orders them.  ``pairs``: a DataFrame whose first two columns
        are users and items (further columns are ignored), or an iterable of (user, item) tuples; both must be in the
        training data (KeyError).  A user's candidates are the items of its pairs (a repeated pair counts once),
        without the user's own training items when ``exclude_seen``.  Scores and order are ``recommend``'s, bit for
        bit, and everything runs on the device.

        ``n``: the best ``n`` of each list; None: each user's whole list, provided the longest holds at most 1,024
        items (a longer one needs an explicit ``n``).  Returns ``recommend``'s frame (``users``, ``items``, ``score``,
        ``rank``), users in order of first appearance in ``pairs``.  The model's stored predictions and ``score()``
        are left as they are."""
        self._check_whole_model()
        w = self._rating_weights(weights)
        if n is not None:
            n, _ = self._recommend_args(n, weights)
        us, its = self._pair_columns(pairs)
        uid, _ = self._side("users").request(us)
        iid, _ = self._side("items").request(its)
        users, first = np.unique(uid, return_index=True)
        users = users[np.argsort(first, kind="stable")]                    # order of first appearance
        place = np.empty((self.p + 1), dtype=np.int64)
        place[users] = np.arange(len(users))
        lists = grouped(place[uid], iid, len(users), sort=True, distinct=True)   # per user ascending and distinct
        users = users.astype(np.int32)
        labels = self._side("users").request(None)[1][users]
        if n is None:
            longest = int(np.diff(lists[0]).max()) if len(users) else 1
            if longest > self.RECOMMEND_MAX:
                raise ValueError(f"the longest candidate list holds {longest} items: beyond {self.RECOMMEND_MAX} "
                                 "an explicit n is needed")
            n = max(longest, 1)
        if len(users) == 0:
            return self._top_n_frame(None, n, labels[:0], self._side("items"))
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            return self._top_n_frame(lambda b, e: ctx.recommend_rank(users[b:e], *group_slice(lists, b, e), n),
                                     n, labels, self._side("items"))

    def recommend_users(self, items=None, n=10, exclude_seen=True, weights=None):
        """The ``n`` best users per item -- who should see this item -- scored on the device: ``recommend`` from the
        item's side.  Scores as in ``recommend`` (the same numbers, bit for bit); candidates are all training users,
        without the users that have the item in the training data when ``exclude_seen``.  Order: score descending,
        equal scores by ascending encoded user id.

        Returns a DataFrame with columns ``items``, ``users``, ``score``, ``rank`` (1 = best), items in request order
        (``items=None``: every training item), labels as ``recommend`` returns them.  The model's stored predictions
        and ``score()`` are left as they are."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        ids, labels = self._side("items").request(items)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            return self._top_n_frame(lambda b, e: ctx.recommend_query_items(ids[b:e], n), n, labels,
                                     self._side("users"), columns=("items", "users", "score"))

    def audience(self, items=None, min_score=None, exclude_seen=True, weights=None, count_only=False):
        """Every user whose score for an item reaches ``min_score`` (required, finite) -- a mailing list, the reach of a
        campaign -- found on the device without a users x items score matrix.  Scores and candidates as in
        ``recommend_users``; the bar is compared with the final score.

        Returns a DataFrame with columns ``items``, ``users``, ``score``, ``rank`` (1 = the item's best user): items in
        request order (``items=None``: every training item), within an item score descending, equal scores by
        ascending encoded user id.  ``count_only=True``: columns ``items``, ``count``, one row per requested item.  The
        model's stored predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        min_score, w = check_finite(min_score, "min_score"), self._rating_weights(weights)
        ids, labels = self._side("items").request(items)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            sizes = np.diff(ctx.recommend_audience(ids, min_score, count_only=True)[0])
            if count_only:
                return pd.DataFrame({"items": labels, "count": sizes.astype(np.int64)})

            def pieces():  # of at most RECOMMEND_BATCH_ROWS entries (a larger item goes alone)
                b = 0
                while b < len(ids):
                    e, total = b + 1, int(sizes[b])
                    while e < len(ids) and total + int(sizes[e]) <= self.RECOMMEND_BATCH_ROWS:
                        total += int(sizes[e])
                        e += 1
                    yield b, e, total
                    b = e

            def query(b, e, total):
                off, us, sc = ctx.recommend_audience(ids[b:e], min_score, total=total)
                at = np.repeat(np.arange(e - b), np.diff(off))
                order = np.lexsort((us, -sc, at))
                return np.diff(off), {"row": at, "users": us[order], "score": sc[order],
                                      "rank": (np.arange(len(at)) - off[:-1][at] + 1).astype(np.int64)}
            return self._frame({"items": labels}, {"users": self._side("users"), "score": None, "rank": None},
                               pieces(), query)

    def top_pairs(self, m=100, users=None, exclude_seen=True, weights=None):
        """The ``m`` best (user, item) pairs of the whole model, ranked on the device in ONE order over all pairs of
        ``users`` (None: every training user) and the training items -- the most probable missing links of a network,
        the strongest matches of a catalogue.  Scores as in ``recommend`` (the same numbers, bit for bit); candidates
        are all pairs, without the training pairs when ``exclude_seen``.  Order: score descending, equal scores by
        ascending encoded user id, then encoded item id; the order in which ``users`` are named does not matter.

        Returns a DataFrame with columns ``users``, ``items``, ``score``, ``rank`` (1 = best of all), at most ``m``
        rows, labels as ``recommend`` returns them.  The model's stored predictions and ``score()`` are left as they
        are."""
        self._check_whole_model()
        m = check_integer(m, "m", 1)
        if m > self.TOP_PAIRS_MAX:
            raise ValueError(f"m = {m} is beyond the {self.TOP_PAIRS_MAX} pairs a query returns at most")
        w = self._rating_weights(weights)
        ids = None
        if users is not None:
            ids, labels = self._side("users").request(users)
            if len(np.unique(ids)) != len(ids):
                twice = list(dict.fromkeys(labels[np.isin(ids, ids[np.bincount(ids)[ids] > 1])].tolist()))
                raise ValueError(f"users named more than once: {twice}")
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            us, its, scores, count = ctx.recommend_top_pairs(m, ids)
        return pd.DataFrame({
            "users": self._side("users").label(us[:count]),
            "items": self._side("items").label(its[:count]),
            "score": scores[:count],
            "rank": np.arange(1, count + 1, dtype=np.int64)})

    TOP_PAIRS_BULK_MAX = 1 << 26     # largest m of top_pairs_bulk (MMSBM_HIP_TOP_PAIRS_BULK_MAX_M)

    def _pairs_bulk_args(self, m, users, weights):
        """(m, rating weights, encoded ids or None) of ``top_pairs_bulk`` / ``score_bar``, refused as ``top_pairs``
        refuses them."""
        self._check_whole_model()
        m = check_integer(m, "m", 1)
        if m > self.TOP_PAIRS_BULK_MAX:
            raise ValueError(f"m = {m} is beyond the {self.TOP_PAIRS_BULK_MAX} pairs a query returns at most")
        w = self._rating_weights(weights)
        ids = None
        if users is not None:
            ids, labels = self._side("users").request(users)
            if len(np.unique(ids)) != len(ids):
                twice = list(dict.fromkeys(labels[np.isin(ids, ids[np.bincount(ids)[ids] > 1])].tolist()))
                raise ValueError(f"users named more than once: {twice}")
        return m, w, ids

    def top_pairs_bulk(self, m, users=None, exclude_seen=True, weights=None):
        """``top_pairs`` for ``m`` far beyond 1,024 -- up to 2^26 -- : the links a reconstruction adds to a network,
        the sends of a campaign with a global budget.  Candidates, scores and order are ``top_pairs``'; the score of
        the ``m``-th pair is found exactly on the device by a radix select over the score tiles, the pairs above it
        and the ties the order admits are then written and sorted there.  No users x items matrix exists.

        Returns ``top_pairs``' DataFrame: columns ``users``, ``items``, ``score``, ``rank`` (1 = best of all), at most
        ``m`` rows.  ``self.pairs_bulk_`` then holds ``{"bar", "above", "ties", "candidates"}``: the score of the
        last returned pair, how many candidate pairs score strictly above it and exactly it, and the number of
        candidates (see ``score_bar``).  The model's stored predictions and ``score()`` are left as they are."""
        m, w, ids = self._pairs_bulk_args(m, users, weights)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            us, its, scores, count, info = ctx.recommend_top_pairs_bulk(m, ids)
        self.pairs_bulk_ = info
        step = self.RECOMMEND_BATCH_ROWS
        parts = [pd.DataFrame({
            "users": self._side("users").label(us[b:min(count, b + step)]),
            "items": self._side("items").label(its[b:min(count, b + step)]),
            "score": scores[b:min(count, b + step)],
            "rank": np.arange(b + 1, min(count, b + step) + 1, dtype=np.int64)}) for b in range(0, max(count, 1), step)]
        return pd.concat(parts, ignore_index=True) if len(parts) > 1 else parts[0]

    def score_bar(self, m, users=None, exclude_seen=True, weights=None):
        """The score of the ``m``-th best (user, item) pair without the pairs themselves: what a budget of ``m`` sends
        sets as the bar.  The request is ``top_pairs_bulk``'s.

        Returns ``{"bar", "above", "ties", "candidates"}``: the bar, the candidate pairs that score strictly above it,
        those that score exactly it, and all candidates.  ``audience(min_score=bar)`` over the same users returns
        ``above + ties`` pairs -- ``m`` or, when pairs tie at the bar, more; ``top_pairs_bulk`` cuts the ties by
        ascending user, then item."""
        m, w, ids = self._pairs_bulk_args(m, users, weights)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            return ctx.recommend_pair_bar(m, ids)

    def explain(self, pairs, n=5, weights=None):
        """Why an item is recommended to a user: the ``n`` training rows of the user that carry most of the pair's
        score -- the "because you rated ..." of a recommendation -- found on the device.

        With eta and p fixed, the theta half of the M-step writes a user's membership as an average over the user's
        d_u training rows j = (u, i_j, r_j): theta'_u[k] = (1/d_u) sum_j c_j[k], where c_j[k] = theta_u[k] v_j[k] /
        (theta_u . v_j) is the share of row j that group k takes and v_j[k] = sum_l p[k, l, r_j] eta[i_j, l].  The score
        is linear in theta, score(u, t) = sum_k theta_u[k] g_t[k] with g_t[k] = sum_l (sum_r weights[r] p[k, l, r])
        eta[t, l], so contribution(u, t, j) = (1/d_u) sum_k c_j[k] g_t[k] is the part of the score that row j carries
        (d_u times it: the score u would have for t if judged from row j alone).  The contributions of ALL the user's
        rows, not only the ``n`` returned, sum to ``explained``, the score under one more theta update; ``explained``
        equals ``score`` at a fixed point of EM, so ``score - explained`` is how far that user's theta is from one.
        Everything is the mean over the restarts the model holds.

        ``pairs``: a DataFrame whose first two columns are users and items (further columns are ignored, so
        ``model.explain(model.recommend(users=[...]))`` works as is), or an iterable of (user, item) tuples; both must
        be in the training data (KeyError).  Returns a DataFrame with columns ``users``, ``items``, ``because`` (the
        history item), ``rating`` (the rating the user gave it), ``contribution``, ``share`` (contribution /
        explained), ``rank`` (1 = the largest contribution), ``score``, ``explained`` (both repeated on a pair's rows):
        pairs in request order, labels as ``recommend`` returns them; within a pair contribution descending, equal
        ones by ascending encoded history item id, then rating id.  The model's stored predictions and ``score()`` are
        left as they are."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        us, its = self._pair_columns(pairs)
        uid, ulab = self._side("users").request(us)
        iid, ilab = self._side("items").request(its)
        made = {"because": self._side("items"), "rating": self._side("ratings"), "contribution": None,
                "share": lambda c: c["contribution"] / c["explained"], "rank": None, "score": None, "explained": None}
        with self._session_of_restarts("explain", w) as ctx:
            def query(b, e):
                u = uid[b:e]
                first = np.flatnonzero(np.concatenate([[True], u[1:] != u[:-1]]))   # runs of one user: one occurrence
                off = np.concatenate([first, [e - b]]).astype(np.int64)
                hi, hr, co, counts, explained, score, _ = ctx.explain_query(u[first], off, iid[b:e], n)
                return counts, {"because": hi, "rating": hr, "contribution": co, "score": score[:, None],
                                "explained": explained[:, None]}
            return self._frame({"users": ulab, "items": ilab}, made, self._row_batches(len(uid), n), query, n)

    # ------------------------------------------------------------------ which ratings look wrong (not in the reference)
    LOWEST_MAX = 1024                # largest m of spurious_ratings (MMSBM_HIP_LOO_MAX_M)

    def _reliability_frame(self, rows, fitted, reliability):
        """The frame of the training rows at positions ``rows``: labels, fitted, reliability, surprise."""
        train = np.asarray(self.train)[rows]
        return pd.DataFrame({
            "users": self._side("users").label(train[:, 0]),
            "items": self._side("items").label(train[:, 1]),
            "rating": self._side("ratings").label(train[:, 2]),
            "fitted": fitted,
            "reliability": reliability,
            "surprise": -np.log(np.maximum(reliability, np.finfo(np.float64).eps))})

    def _known_labels(self, side, labels):
        """The ids of ``labels`` on ``side`` ("users" / "items"), -1 where the training data has none: those are named
        in ``predict``'s warning."""
        ids = self._side(side).ids(labels)
        unseen = list(dict.fromkeys(str(x) for x, j in zip(labels, ids.tolist()) if j < 0))
        if unseen:
            self.logger.warning(f"The {side} {', '.join(unseen)} are in the test set but weren't in the train set so "
                                f"I'll remove them.")
        return ids

    def rating_reliability(self, pairs=None):
        """How far the model believes each training rating once that rating is taken away -- the other half of network
        reconstruction: ``top_pairs`` finds the missing links, this the spurious ones.  Computed on the device.

        The in-sample probability of a training row (``fitted``) is bent towards the row: a user with six ratings has
        a theta that was fitted to explain each of them, so a wrong rating largely vouches for itself.  ``reliability``
        is the probability of the row's rating under parameters that never saw the row: the M-step writes theta_u as
        the average of its rows' shares c_j (the identity ``explain`` rests on) and eta_i as that of its rows' shares
        e_j, so one EM step without row j is a downdate of two sums, theta-_u = (C_u - c_j) / (d_u - 1) and eta-_i =
        (E_i - e_j) / (d_i - 1), and reliability_j = sum_kl theta-_u[k] eta-_i[l] p[k, l, r_j].  The only row of a user
        (item) is judged from the mean theta (eta) row.  p stays the fitted p on purpose: a row is one of d_u rows of its
        user but one of very many soft counts of a block, and removing it from a block that only this row supports is
        ill-conditioned.  ``surprise`` = -log(max(reliability, eps)).  Everything is the mean over the restarts the
        model holds.

        ``pairs``: None for every training row in training order, or a DataFrame whose first two columns are users and
        items, or (user, item) tuples: the training rows of those pairs, in training order (a pair rated twice has two
        rows; users and items unseen in training are dropped with ``predict``'s warning).  Returns a DataFrame with
        columns ``users``, ``items``, ``rating``, ``fitted``, ``reliability``, ``surprise``.  The model's stored
        predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        rows = None
        if pairs is not None:
            us, its = self._pair_columns(pairs)
            uid, iid = self._known_labels("users", us), self._known_labels("items", its)
            keep = (uid >= 0) & (iid >= 0)
            train = np.asarray(self.train)
            width = np.int64(self.m + 1)
            asked = np.unique(uid[keep].astype(np.int64) * width + iid[keep])
            rows = np.flatnonzero(np.isin(train[:, 0].astype(np.int64) * width + train[:, 1], asked))
        with self._session_of_restarts("loo") as ctx:
            fitted, reliability = ctx.loo_rows(rows)
        return self._reliability_frame(slice(None) if rows is None else rows, fitted, reliability)

    def spurious_ratings(self, m=100, users=None, items=None):
        """The ``m`` training ratings the model believes least -- a mistyped 1 for a 5, a shared account, a bot, a
        mislabelled item -- selected on the device: the rows of smallest ``reliability`` (``rating_reliability``
        defines it), ascending, exactly equal ones in training order.  ``users`` / ``items`` (labels of the training
        data: KeyError otherwise) restrict the rows to those of the named users and, when both are given, of the named
        items as well.  ``m`` is at most 1,024: for more, sort ``rating_reliability()``.

        Returns a DataFrame with the columns of ``rating_reliability`` plus ``rank`` (1 = the least reliable), at most
        ``m`` rows.  The model's stored predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        m = check_integer(m, "m", 1)
        if m > self.LOWEST_MAX:
            raise ValueError(f"m = {m} is beyond the {self.LOWEST_MAX} rows a query returns at most: "
                             "sort rating_reliability() instead")
        flags = []
        for side, wanted in (("users", users), ("items", items)):
            if wanted is None:
                flags.append(None)
                continue
            mask = np.zeros(len(self._side(side)), dtype=bool)
            mask[self._side(side).request(wanted)[0]] = True
            flags.append(mask)
        with self._session_of_restarts("loo") as ctx:
            rows, reliability, count = ctx.loo_lowest(m, *flags)
            fitted, _ = ctx.loo_rows(rows[:count])
        frame = self._reliability_frame(rows[:count], fitted, reliability[:count])
        frame["rank"] = np.arange(1, count + 1, dtype=np.int64)
        return frame

    def _misfit(self, side, m, min_ratings):
        self._check_whole_model()
        if m is not None:
            m = check_integer(m, "m", 1)
        min_ratings = check_integer(min_ratings, "min_ratings", 1)
        with self._session_of_restarts("loo") as ctx:
            sides = ctx.loo_sides()
        surprise, fitted = sides[:2] if side == "users" else sides[2:]
        table = self._side(side)
        degree = np.bincount(np.asarray(self.train)[:, 0 if side == "users" else 1], minlength=len(table))[:len(table)]
        ids = np.flatnonzero(degree >= min_ratings)
        ids = ids[np.lexsort((ids, -surprise[ids]))][:m]
        return pd.DataFrame({side: table.label(ids), "ratings": degree[ids].astype(np.int64),
                             "surprise": surprise[ids], "fitted_surprise": fitted[ids]})

    def misfit_users(self, m=None, min_ratings=2):
        """The users the model explains worst: per user the mean ``surprise`` of its training rows
        (``rating_reliability``), summed on the device.  Users with fewer than ``min_ratings`` training rows are left
        out (the only row of a user is judged from the mean theta row, which says little about the user).

        Returns a DataFrame with columns ``users``, ``ratings`` (the user's training rows), ``surprise``,
        ``fitted_surprise`` (the same mean built from the in-sample ``fitted``), ``surprise`` descending, equal ones by
        encoded id; ``m``: the first ``m`` rows (None: all)."""
        return self._misfit("users", m, min_ratings)

    def misfit_items(self, m=None, min_ratings=2):
        """``misfit_users`` for the items: columns ``items``, ``ratings``, ``surprise``, ``fitted_surprise``."""
        return self._misfit("items", m, min_ratings)

    # ------------------------------------------------------------------ nearest items / users (not in the reference)
    def similar_items(self, items=None, n=10):
        """The ``n`` training items most similar to each of ``items`` (None: every training item), on the device.

        An item's rating profile is the rating distribution a member of each user group gives it,
        q[i, k, :] = sum_l eta[i, l] p[k, l, :]; the distance of two items is
        D(i, j) = sum_k m[k] |q[i, k, :] - q[j, k, :]|^2 / U with m[k] = sum_u theta[u, k] the users in group k: how
        differently a user drawn from the training population rates the two, in [0, 2], mean over the restarts the
        model holds.  It does not depend on how a restart happens to label its groups.

        Returns a DataFrame with columns ``items``, ``similar``, ``distance``, ``rank`` (1 = nearest), rows in request
        order, both id columns as the encoder's labels (``eta``'s index).  Order: distance ascending, equal distances
        by ascending encoded id; an item is never its own neighbour.  The model's stored predictions and ``score()``
        are left as they are."""
        return self._similar("items", items, n)

    def similar_users(self, users=None, n=10):
        """The ``n`` training users most similar to each of ``users`` (None: every training user): ``similar_items``
        with the sides exchanged -- q[u, l, :] = sum_k theta[u, k] p[k, l, :], weighted by the items in each item
        group.  Columns ``users``, ``similar``, ``distance``, ``rank``."""
        return self._similar("users", users, n)

    def _similar(self, side, wanted, n):
        self._check_whole_model()
        n, _ = self._recommend_args(n, None)
        ids, labels = self._side(side).request(wanted)
        with self._session_of_restarts("similar", side) as ctx:
            return self._top_n_frame(lambda b, e: ctx.similar_query(ids[b:e], n), n, labels, self._side(side),
                                     columns=(side, "similar", "distance"))

    # ------------------------------------------------------------------ diversified lists (not in the reference)
    def recommend_diverse(self, users=None, n=10, diversity=..., pool=None, exclude_seen=True, weights=None,
                          candidates=None, exclude=None):
        """``recommend`` re-ranked for diversity, on the device: a fitted model puts whole blocks of items on the same
        memberships, so a user's ``n`` best items are often near-copies of each other.  From the user's ``pool`` best
        candidates -- ``recommend(n=pool)``'s list, with the same ``exclude_seen``, ``weights``, ``candidates`` and
        ``exclude`` -- the best one is taken first; then, ``n - 1`` times, the candidate with the largest
        score + ``diversity`` x (distance to the nearest item taken so far), equal values to the better item of
        ``recommend``'s order.  The distance is ``similar_items``'s (``distances``).

        ``diversity`` is required: it is in score units per unit of distance, so no default fits every weighting.
        It must be finite and >= 0; 0 gives ``recommend(n)``'s list, and the larger it is the further apart the items
        of a list lie.  ``pool``: None means min(1024, 10 n); at least ``n`` and at most 1,024.

        Returns ``recommend``'s frame plus ``distance`` -- to the nearest item ranked above it in the list, +inf at
        rank 1: columns ``users``, ``items``, ``score``, ``distance``, ``rank``.  ``list_diversity`` summarises a
        list.  The model's stored predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        if diversity is ...:
            raise TypeError("recommend_diverse() needs diversity=: score units per unit of distance (0: plain recommend)")
        lam = check_finite(diversity, "diversity", 0, "a finite number >= 0")
        pool = check_integer(min(self.DIVERSE_POOL_MAX, 10 * n) if pool is None else pool, "pool", 1)
        if not n <= pool <= self.DIVERSE_POOL_MAX:
            raise ValueError(f"pool must lie in [n, {self.DIVERSE_POOL_MAX}], got pool={pool} with n={n}")
        ids, labels = self._side("users").request(users)
        cand = self._candidate_ids(candidates)
        columns = ("users", "items", "score", "distance")
        if cand is not None and len(cand) == 0:
            return self._top_n_frame(None, n, labels[:0], self._side("items"), columns)
        extra = self._exclusion_lists(exclude, ids)
        with self._sessions_of_restarts(("recommend", w, exclude_seen), ("similar", "items")) as ctx:
            return self._top_n_frame(
                lambda b, e: ctx.recommend_diverse(ids[b:e], n, pool, lam, cand, group_slice(extra, b, e)),
                n, labels, self._side("items"), columns)

    def distances(self, pairs, side="items"):
        """The distance of given pairs of training items (``side="users"``: of training users), on the device:
        ``similar_items``'s D, the number ``recommend_diverse`` trades against the score.  ``pairs``: a DataFrame whose
        first two columns hold the two labels of each pair, or an iterable of 2-tuples; a label that is not in the
        training data: KeyError.  D(a, b) = D(b, a) bit for bit and D(a, a) = 0.

        Returns a DataFrame with columns ``a``, ``b`` (the encoder's labels), ``distance``, rows in request order."""
        self._check_whole_model()
        if side not in ("items", "users"):
            raise ValueError(f"side must be 'items' or 'users', got {side!r}")
        left, right = self._pair_columns(pairs)
        a, a_labels = self._side(side).request(left)
        b, b_labels = self._side(side).request(right)
        if len(a) == 0:
            return pd.DataFrame({"a": [], "b": [], "distance": np.zeros(0)})
        with self._session_of_restarts("similar", side) as ctx:
            d = self._pair_distances(ctx, a, b)
        return pd.DataFrame({"a": a_labels, "b": b_labels, "distance": d})

    def _pair_distances(self, ctx, a, b):
        """ctx.similar_pairs in calls of at most RECOMMEND_BATCH_ROWS pairs."""
        step = self.RECOMMEND_BATCH_ROWS
        parts = [ctx.similar_pairs(a[s:s + step], b[s:s + step]) for s in range(0, len(a), step)]
        return np.concatenate(parts) if parts else np.zeros(0)

    def list_diversity(self, recs):
        """The intra-list distance of every user's list in a recommend-style frame (``recommend``,
        ``recommend_diverse``, ``rerank`` ...: the first two columns are users and items): the mean of ``distances``
        over the unordered pairs of the list's items, on the device -- what ``diversity=`` bought, to be read next to
        ``ranking_score``.  The items must be in the training data (KeyError); the users are only the lists' names.

        Returns a DataFrame with columns ``users`` (order of first appearance), ``n`` (items in the list) and
        ``diversity`` (NaN for a list of fewer than two items)."""
        self._check_whole_model()
        us, its = self._pair_columns(recs)
        iid, _ = self._side("items").request(its)
        names = list(dict.fromkeys(us))
        place = {u: j for j, u in enumerate(names)}
        start, listed = grouped([place[u] for u in us], iid, len(names))   # each list's items, in the frame's order
        sizes = np.diff(start)
        a, b, owner = [], [], []
        for j, k in enumerate(sizes.tolist()):
            if k >= 2:
                x, y = np.triu_indices(k, 1)
                mine = listed[start[j]:start[j + 1]]
                a.append(mine[x])
                b.append(mine[y])
                owner.append(np.full(len(x), j, dtype=np.int64))
        total = np.zeros(len(names))
        if a:
            with self._session_of_restarts("similar", "items") as ctx:
                d = self._pair_distances(ctx, np.concatenate(a), np.concatenate(b))
            total = np.bincount(np.concatenate(owner), weights=d, minlength=len(names))
        pairs = sizes * (sizes - 1) // 2
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(pairs > 0, total / np.maximum(pairs, 1), np.nan)
        return pd.DataFrame({"users": np.asarray(names, dtype=object) if names else [], "n": sizes.astype(np.int64),
                             "diversity": mean})

    # ------------------------------------------------------------------ matching the restarts' groups (not in the reference)
    def align_restarts(self, reference=None):
        """Which group of each restart is which group of restart ``reference``, and how well the restarts agree.

        Every restart labels its groups in an order of its own.  The overlap of two groups is the population they
        share, O[a, b] = sum_u theta_s[u, a] theta_t[u, b] (items: eta); the device computes it for all pairs of
        restarts at once, and each restart's groups are matched to the reference's by the assignment of the largest
        total overlap.  ``reference``: a position in ``self.results``; None: the restart of the highest training
        likelihood (the first of them).

        Returns a dict:
          ``reference``        the position used;
          ``user_groups``      (S, K) int64, ``[s, k]`` = the group of restart s matched to group k of the reference
                               (the identity for the reference itself);  ``item_groups`` (S, L) likewise;
          ``user_similarity``  (S, K), the cosine of each matched pair of theta columns, in [0, 1], 1 for the
                               reference; a column near 0 across the restarts is a group they do not reproduce -- the
                               usual sign of too large a K.  ``item_similarity`` (S, L) likewise;
          ``user_agreement``   (S, S), the largest assignment total of restarts s and t divided by the number of
                               users: the expected share of users the two put into matched groups; symmetric.
                               ``item_agreement`` likewise.
        ``self.results``, the stored predictions and ``score()`` are left as they are."""
        from . import align
        self._check_whole_model()
        S = len(self.results)
        if reference is None:
            reference = int(np.argmax([float(a["likelihood"]) for a in self.results]))   # (the first of the highest)
        else:
            reference = check_integer(reference, "reference", None, "a position in self.results (an int) or None")
            if not 0 <= reference < S:
                raise ValueError(f"reference = {reference} is not a position in self.results (0 .. {S - 1})")
        out = {"reference": reference}
        for side, groups, n_rows in (("user", self.user_groups, self.p + 1), ("item", self.item_groups, self.m + 1)):
            with self._session_of_restarts("overlap", side + "s") as ctx:
                gram = ctx.overlap_query()
            out[side + "_groups"], out[side + "_similarity"], out[side + "_agreement"] = align.align_side(
                gram, groups, n_rows, reference)
        return out

    def consensus(self, reference=None):
        """theta, eta and pr averaged over the restarts once their groups are matched (``align_restarts``).

        This is a DESCRIPTIVE summary, written in the group labels of restart ``reference`` (None: the restart of the
        highest training likelihood): what the restarts say about the groups on average, for reading memberships and
        judging which groups are reproducible.  It is not what the model predicts with: the predictive ensemble remains
        the mean over the restarts' own predictions that ``predict`` and ``recommend`` use, which needs no matching.

        Returns {"theta": DataFrame (user labels x K), "eta": DataFrame (item labels x L), "pr": {rating label: K x L
        DataFrame} (shaped as ``self.theta`` / ``self.eta`` / ``self.pr``), "alignment": the dict of
        ``align_restarts``}.  ``self.results`` and the stored objects are left as they are."""
        from . import align
        alignment = self.align_restarts(reference)
        theta, eta, pr = align.consensus_params(self.results, alignment["user_groups"], alignment["item_groups"])
        return {**self._labelled(theta, eta, pr), "alignment": alignment}

    def _labelled(self, theta, eta, pr):
        """{"theta", "eta", "pr"} as the model's stored objects are shaped: theta and eta as DataFrames indexed by the
        user and item labels, pr as {rating label: K x L DataFrame}."""
        ratings = self._side("ratings").label(np.arange(pr.shape[2])).tolist()
        return {"theta": pd.DataFrame(theta, index=self._side("users").index()),
                "eta": pd.DataFrame(eta, index=self._side("items").index()),
                "pr": {lab: pd.DataFrame(pr[:, :, j]) for j, lab in enumerate(ratings)}}

    # ------------------------------------------------------------------ ranking evaluation (not in the reference)
    def log_likelihood(self, data):
        """The held-out predictive log-likelihood of ``data`` (same columns as the training data), on the device:
        sum over the rows of log max(P(observed rating | user, item), eps) -- the quantity a probabilistic model is
        judged by, where ``score()`` reports the accuracy of the argmax.  Rows with a user, item or rating unseen in
        training are dropped with ``predict``'s warning.

        Returns {"rows": rows scored, "log_likelihood": that of the model's predictive distribution, the mean over the
        restarts as ``predict`` uses it, "per_restart": [that of each restart alone], "perplexity":
        exp(-log_likelihood / rows)}.  The model's stored predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        rows = self._encode_heldout(data)
        ctx, restarts = self._restarts()
        with session(ctx, "heldout", rows):
            per_restart = [float(ctx.heldout_add()) for _ in restarts]
            _, mean = ctx.heldout_mean(want_rows=False)
        n, mean = len(rows), float(mean)
        return {"rows": n, "log_likelihood": mean, "per_restart": per_restart,
                "perplexity": float(np.exp(-mean / n)) if n else float("nan")}

    def _encode_heldout(self, data):
        """Encoded (N, 3) int32 rows of ``data`` in input order, rows with a user, item or rating unseen in training
        dropped with ``Encoder.transform``'s warning (after ``fit_encoded``: ids outside the training ones)."""
        if self.data_handler:
            return self.data_handler.transform(data, self.logger)
        return self._known_rows(data, self.p + 1, self.m + 1, self.ratings)

    def _known_mask(self, columns):
        """The mask of the rows of encoded id ``columns`` -- (name, ids, known), ``known`` the number of training ids
        or the training ids themselves -- that hold a training id in every column; the ids the others hold are named
        in ``Encoder.transform``'s warning, column after column (a row counts for the first column that drops it)."""
        for name, col, _ in columns:
            if len(col) and not np.issubdtype(col.dtype, np.integer):
                raise ValueError(f"after fit_encoded the {name} column holds encoded integer ids")
        keep = np.ones(len(columns[0][1]), dtype=bool)
        for name, col, known in columns:
            hit = (col >= 0) & (col < known) if np.isscalar(known) else np.isin(col, known)
            unseen = np.unique(col[keep & ~hit])
            if len(unseen):
                self.logger.warning(f"The {name} {', '.join(str(v) for v in unseen.tolist())} are in the test set "
                                    f"but weren't in the train set so I'll remove them.")
            keep &= hit
        return keep

    def _known_rows(self, data, n_users, n_items, ratings):
        """The rows of encoded ``data`` whose ids are training ones (users below n_users, items below n_items, ratings
        among ``ratings``), (N, 3) int32 in input order; the others are dropped with ``Encoder.transform``'s warning."""
        cols = [np.asarray(c) for c in _columns(data)[0]]
        keep = self._known_mask([("users", cols[0], n_users), ("items", cols[1], n_items),
                                 ("ratings", cols[2], np.asarray(ratings))])
        return np.stack([c[keep] for c in cols], 1).astype(np.int32)

    def _heldout(self, data, exclude_seen, weights):
        """(encoded rows (N, 3), position (N,), candidates (N,)) of every row of ``data`` that survives encoding."""
        self._check_whole_model()
        w = self._rating_weights(weights)
        rows = self._encode_heldout(data)
        uniq, user = np.unique(rows[:, 0], return_inverse=True)      # one request entry per user holding rows
        offsets, order = grouped(user.reshape(-1), np.arange(len(rows)), len(uniq))
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            pos, cand = ctx.recommend_positions(uniq.astype(np.int32), offsets, rows[order, 1])
        position = np.empty(len(rows), dtype=np.int64)
        position[order] = pos
        candidates = np.empty(len(rows), dtype=np.int64)
        candidates[order] = np.repeat(cand.astype(np.int64), np.diff(offsets))
        return rows, position, candidates

    def heldout_positions(self, data, exclude_seen=True, weights=None):
        """Where each held-out row's item falls in its user's full recommendation order, on the device: one row per
        row of ``data`` that survives encoding (rows whose user, item or rating is not in the training data are dropped
        with ``predict``'s warning), in input order.  Scores and candidates are those of ``recommend(users, n,
        exclude_seen, weights)``; ``position`` = 1 + the candidates that come before the item (score descending, equal
        scores by ascending encoded item id), 0 when the item is not a candidate (a training item of the user while
        ``exclude_seen``); ``candidates`` = the user's number of candidates.

        Returns a DataFrame with columns ``users``, ``items``, ``ratings`` (the encoder's labels), ``position`` and
        ``candidates``.  The model's stored objects are left as they are."""
        rows, position, candidates = self._heldout(data, exclude_seen, weights)
        cols = {name: self._side(name).label(rows[:, j]) for j, name in enumerate(("users", "items", "ratings"))}
        return pd.DataFrame({**cols, "position": position, "candidates": candidates})

    def _ranking_args(self, k, relevant):
        ks = list(k) if hasattr(k, "__iter__") and not isinstance(k, (str, bytes)) else [k]
        for x in ks or [None]:
            check_integer(x, "k", 1, "a positive integer or a list of them", got=k)
        ks = list(dict.fromkeys(int(x) for x in ks))
        if relevant is None:
            return ks, None
        if isinstance(relevant, (str, bytes)) or not hasattr(relevant, "__iter__"):
            raise ValueError(f"relevant must be a collection of rating values, got {relevant!r}")
        relevant = list(relevant)
        ids = self._side("ratings").ids(relevant)   # (with an encoder str(value), whatever the order of the labels)
        if (ids < 0).any():
            raise ValueError(f"relevant rating {relevant[int(np.argmax(ids < 0))]!r} is not a rating of the training data")
        return ks, set(ids.tolist())

    def ranking_score(self, data, k=10, relevant=None, exclude_seen=True, weights=None):
        """Top-N ranking metrics of the held-out rows ``data`` (users, items, ratings like ``predict``'s), from
        ``heldout_positions(data, exclude_seen, weights)``.  Each distinct (user, item) pair counts once; it is
        relevant when any of its rows has a rating in ``relevant`` (rating values as in the data, e.g. ``{4, 5}``;
        None: every pair).  Pairs that are not candidates (position 0) are left out and counted.  Per user with m >= 1
        relevant candidate pairs at positions p_t among C candidates: hits(k) = #{p_t <= k}, precision@k = hits / k,
        recall@k = hits / m, hit_rate@k = [hits > 0], ndcg@k (binary gains), mrr = 1 / min p_t and
        auc = sum_t (C - m - (p_t - 1 - a_t)) / (m (C - m)) with a_t the relevant pairs before t (not defined for
        C == m).  Each metric is the mean over those users (NaN without any).  ``k``: an int or a list of ints >= 1.

        Returns a dict: ``users`` (evaluated), ``skipped_users`` (users with rows but no relevant candidate pair),
        ``pairs`` (distinct pairs), ``not_candidates`` (pairs at position 0), ``mrr``, ``auc`` and ``precision@k``,
        ``recall@k``, ``ndcg@k``, ``hit_rate@k`` for each k."""
        self._check_whole_model()
        ks, rel_ids = self._ranking_args(k, relevant)
        rows, position, candidates = self._heldout(data, exclude_seen, weights)
        return ranking_metrics(rows[:, 0], rows[:, 1], rows[:, 2], position, candidates, ks, rel_ids)

    # ------------------------------------------------------------------ fold-in of new users and items (not in the reference)
    def _encode_new(self, data, side):
        """(rows (N, 3) int32 in the training column order, labels of the new entities in order of first appearance).
        Column ``side`` (0: users, 1: items) of ``data`` holds new entities, numbered by first appearance (the training
        theta / eta is never consulted); the other two columns are encoded against the training dictionaries, and rows
        with an unseen entry are dropped with ``Encoder.transform``'s warning.  An entity whose rows are all dropped
        keeps its place (uniform start, no iterations)."""
        cols, _ = _columns(data)
        own = np.asarray(cols[side])
        fixed = 1 - side
        names = ("users", "items")
        enc = self.data_handler
        if enc:  # labels as the encoder makes them: str(value)
            if own.dtype.kind in "iu":
                codes, uniq = pd.factorize(own)
            else:
                if any(v is None or (isinstance(v, float) and v != v) for v in own.tolist()):
                    raise AssertionError("Data contains missing values. Aborting.")
                codes, uniq = pd.factorize(np.array([str(v) for v in own.tolist()], dtype=object))
            labels = np.array([str(v) for v in np.asarray(uniq).tolist()], dtype=object)
            rows, keep = (enc.transform_items if side == 0 else enc.transform_users)(data, self.logger)
        else:
            if len(own) and (not np.issubdtype(own.dtype, np.integer) or own.min() < 0):
                raise ValueError(f"after fit_encoded the {names[side][:-1]} column holds non-negative integer ids")
            codes, uniq = pd.factorize(own.astype(np.int64))
            labels = np.asarray(uniq, dtype=np.int64)
            other, rating = np.asarray(cols[fixed]), np.asarray(cols[2])
            keep = self._known_mask([(names[fixed], other, len(self._side(names[fixed]))),
                                     ("ratings", rating, len(self.ratings))])
            rows = np.stack([other[keep], rating[keep]], 1).astype(np.int32)
        out = np.empty((int(keep.sum()), 3), dtype=np.int32)
        out[:, side] = np.asarray(codes)[keep]
        out[:, fixed] = rows[:, 0]
        out[:, 2] = rows[:, 1]
        return out, labels

    def _fold_runs(self, rows, n_new, iterations, tol, each=None, items=False):
        """(thetas, iterations): theta (n_new, K) -- eta (n_new, L) with ``items`` -- and the iterations used of every
        restart, in ``self.results`` order; ``each(ctx)`` runs after each restart's fold-in while its parameters are
        selected (recommend_new adds the slot there)."""
        ctx, restarts = self._restarts()
        thetas, iters = [], []
        for _ in restarts:
            t, it = (ctx.fold_in_items if items else ctx.fold_in)(rows, n_new, iterations, tol)
            thetas.append(t)
            iters.append(it)
            if each is not None:
                each(ctx)
        return thetas, iters

    @staticmethod
    def _fold_args(iterations, tol):
        iterations = check_integer(iterations, "iterations", 0, "a non-negative integer")
        return iterations, (None if tol is None else check_finite(tol, "tol", None, "None or a finite number", bool_too=True))

    @staticmethod
    def _iterations_frame(iters, labels, name):
        """(new entities x restarts) the iterations each ran, and the index (the new labels, named ``name``)."""
        index = pd.Index(labels, name=name) if len(labels) else pd.Index([], name=name)
        return pd.DataFrame(np.stack(iters, 1) if iters else np.zeros((len(labels), 0)), index=index), index

    def fold_in(self, data, iterations=100, tol=None):
        """theta of users that were not in the training data, from their ratings: ``iterations`` steps of the theta
        half of the M-step with every restart's eta and p held fixed, from a uniform start (``tol``: a user stops once
        no entry of its theta moves by more than ``tol``).  ``data``: users, items, ratings like ``fit``'s (after
        ``fit_encoded``: integer triples, users as any non-negative ids, items and ratings encoded).

        Returns a list of DataFrames, one per restart in ``self.results`` order, each (new users x K) indexed by the
        user labels in order of first appearance in ``data``.  ``self.fold_in_iterations``: a DataFrame (new users x
        restarts) of the iterations each user ran.  The model itself is left as it is."""
        self._check_whole_model()
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._encode_new(data, 0)
        thetas, iters = self._fold_runs(rows, len(labels), iterations, tol)
        self.fold_in_iterations, index = self._iterations_frame(iters, labels, "users")
        return [pd.DataFrame(t, index=index) for t in thetas]

    def recommend_new(self, data, n=10, exclude_seen=True, weights=None, iterations=100, tol=None, candidates=None):
        """``recommend`` for users that were not in the training data: each restart scores with the theta its own
        ``fold_in`` gives them (same arguments as ``fold_in``), the scores are averaged over the restarts.  Returns
        the frame ``recommend`` returns (users, items, score, rank), users in order of first appearance in ``data``;
        ``exclude_seen`` leaves out the items a user has in ``data``; ``candidates`` as in ``recommend``: only these
        items are scored and ranked."""
        return self._recommend_new(data, n, exclude_seen, weights, iterations, tol, candidates, None)

    def recommend_new_quota(self, data, n=10, categories=..., max_per_category=..., exclude_seen=True, weights=None,
                            iterations=100, tol=None, candidates=None):
        """``recommend_new`` with ``recommend_quota``'s cap per category (``categories`` and ``max_per_category`` as
        there, both required): ``recommend_new``'s frame plus the ``category`` column."""
        if categories is ... or max_per_category is ...:
            raise TypeError("recommend_new_quota needs categories= and max_per_category=")
        self._check_whole_model()
        quota = quota_categories(categories, max_per_category, self._side("items"))
        return self._recommend_new(data, n, exclude_seen, weights, iterations, tol, candidates, quota)

    def recommend_new_shelves(self, data, shelves=5, per_shelf=10, categories=..., depth=None, min_items=1,
                              exclude_seen=True, weights=None, iterations=100, tol=None, candidates=None):
        """``recommend_shelves`` for users that were not in the training data, folded in as ``recommend_new`` folds
        them (``iterations``, ``tol``): ``recommend_shelves``' frame, users in order of first appearance in ``data``;
        ``per_shelf=0``: ``recommend_categories``' frame (then ``depth`` is required)."""
        if categories is ...:
            raise TypeError("recommend_new_shelves needs categories=")
        self._check_whole_model()
        per_shelf = check_integer(per_shelf, "per_shelf", 0, "a non-negative integer") or None
        shelves, per_shelf, depth, min_items = self._shelves_args(shelves, per_shelf, depth, min_items)
        w = self._rating_weights(weights)
        cats = shelf_categories(categories, self._side("items"))
        cand = self._candidate_ids(candidates)
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._encode_new(data, 0)
        with session(self._ctx(self._device_list()[0]), "recommend", w, False) as ctx:
            thetas, iters = self._fold_runs(rows, len(labels), iterations, tol, each=lambda c: c.recommend_add())
            self.fold_in_iterations = pd.DataFrame(np.stack(iters, 1), index=pd.Index(labels, name="users"))
            theta = np.stack(thetas)                                  # (restarts, new users, K)
            seen = grouped(rows[:, 0], rows[:, 1], len(labels), sort=True) if exclude_seen else None
            return self._shelves_frame(
                lambda b, e: ctx.recommend_query_theta_shelves(theta[:, b:e], cats.offsets, cats.items, depth, min_items,
                                                               shelves, per_shelf, group_slice(seen, b, e), cand),
                shelves, per_shelf, labels, cats)

    def _recommend_new(self, data, n, exclude_seen, weights, iterations, tol, candidates, quota):
        """recommend_new (``quota`` None) and recommend_new_quota (a ``Quota``)."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        cand = self._candidate_ids(candidates)
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._encode_new(data, 0)
        within = {} if cand is None else {"candidates": cand}
        with session(self._ctx(self._device_list()[0]), "recommend", w, False) as ctx:
            thetas, iters = self._fold_runs(rows, len(labels), iterations, tol, each=lambda c: c.recommend_add())
            self.fold_in_iterations = pd.DataFrame(np.stack(iters, 1), index=pd.Index(labels, name="users"))
            theta = np.stack(thetas)                                  # (restarts, new users, K)
            seen = grouped(rows[:, 0], rows[:, 1], len(labels), sort=True) if exclude_seen else None
            if quota is None:
                return self._top_n_frame(
                    lambda b, e: ctx.recommend_query_theta(theta[:, b:e], n, group_slice(seen, b, e), **within),
                    n, labels, self._side("items"))
            return self._top_n_frame(
                lambda b, e: ctx.recommend_query_theta_quota(theta[:, b:e], n, quota.offsets, quota.items, quota.caps,
                                                             group_slice(seen, b, e), **within),
                n, labels, self._side("items"), derived={"category": quota.label})

    def fold_in_items(self, data, iterations=100, tol=None):
        """eta of items that were not in the training data, from their ratings: ``iterations`` steps of the eta half of
        the M-step with every restart's theta and p held fixed, from a uniform start (``tol`` as in ``fold_in``).
        ``data``: users, items, ratings like ``fit``'s; every item of it is new (the training eta is never consulted),
        users and ratings are encoded against the training dictionaries and rows with an unseen user or rating are
        dropped with ``predict``'s warning (after ``fit_encoded``: integer triples, items as any non-negative ids, users
        and ratings encoded).

        Returns a list of DataFrames, one per restart in ``self.results`` order, each (new items x L) indexed by the
        item labels in order of first appearance in ``data``.  ``self.fold_in_items_iterations``: a DataFrame (new
        items x restarts) of the iterations each item ran.  The model itself is left as it is."""
        self._check_whole_model()
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._encode_new(data, 1)
        etas, iters = self._fold_runs(rows, len(labels), iterations, tol, items=True)
        self.fold_in_items_iterations, index = self._iterations_frame(iters, labels, "items")
        return [pd.DataFrame(e, index=index) for e in etas]

    def _new_items(self, data):
        """_encode_new for the items of ``data``, refused (ValueError) when one of them is a training item."""
        rows, labels = self._encode_new(data, 1)
        clash = [x for x, j in zip(labels.tolist(), self._side("items").ids(labels.tolist())) if j >= 0]
        if clash:
            raise ValueError(f"items of data are training items, so the frame would be ambiguous: {clash[:10]}")
        return rows, labels

    @contextlib.contextmanager
    def _session_with_new_items(self, rows, labels, weights, exclude_seen, iterations, tol):
        """The context, with a recommend session around the block whose catalogue is the training items plus the new
        ones (``rows``, ``labels`` of ``_new_items``): every restart folds them in and is added, then the etas go in
        with, when ``exclude_seen``, the training users that rated each new item."""
        with session(self._ctx(self._device_list()[0]), "recommend", weights, exclude_seen) as ctx:
            etas, iters = self._fold_runs(rows, len(labels), iterations, tol, each=lambda c: c.recommend_add(), items=True)
            self.fold_in_items_iterations = pd.DataFrame(np.stack(iters, 1), index=pd.Index(labels, name="items"))
            ctx.recommend_add_items(np.stack(etas), grouped(rows[:, 1], rows[:, 0], len(labels)) if exclude_seen else None)
            yield ctx

    def recommend_with_new_items(self, data, users=None, n=10, exclude_seen=True, weights=None, iterations=100,
                                 tol=None):
        """``recommend`` over the training items plus the new items of ``data``: each restart scores the new items with
        the eta its own ``fold_in_items`` gives them (same arguments), the scores are averaged over the restarts.
        Returns the frame ``recommend`` returns (users, items, score, rank) for training users (``users`` as in
        ``recommend``); ``exclude_seen`` leaves out a user's training items and the new items the user rated in
        ``data``.  An item label of ``data`` that is also a training item is refused (ValueError)."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._new_items(data)
        ids, user_labels = self._side("users").request(users)
        with self._session_with_new_items(rows, labels, w, exclude_seen, iterations, tol) as ctx:
            return self._top_n_frame(lambda b, e: ctx.recommend_query(ids[b:e], n), n, user_labels,
                                     self._side("items").extended(labels))

    def recommend_users_new_items(self, data, n=10, exclude_seen=True, weights=None, iterations=100, tol=None):
        """``recommend_users`` for items that were not in the training data -- the cold-start audience of new items:
        each restart scores with the eta its own ``fold_in_items`` gives them (same arguments), the scores are averaged
        over the restarts.  Returns the frame ``recommend_users`` returns (items, users, score, rank), items in order
        of first appearance in ``data``; ``exclude_seen`` leaves out the users that rated the item in ``data``.  An
        item label of ``data`` that is also a training item is refused (ValueError)."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._new_items(data)
        ids = np.arange(self.m + 1, self.m + 1 + len(labels), dtype=np.int32)
        with self._session_with_new_items(rows, labels, w, exclude_seen, iterations, tol) as ctx:
            return self._top_n_frame(lambda b, e: ctx.recommend_query_items(ids[b:e], n), n, labels,
                                     self._side("users"), columns=("items", "users", "score"))


    # ------------------------------------------------------------------ recommendation for groups (not in the reference)
    _GROUP_COLUMNS = ("group", "items", "score")
    _GROUP_AGGREGATES = {"least_misery": "min", "most_pleasure": "max", "approval": "count", "mean": "mean"}

    def _group_lists(self, groups):
        """(labels (G,) object, (offsets (G + 1,) int64, members int32)) of a ``groups`` argument: a dict {label:
        users}, a sequence of user iterables (labels 0, 1, ...) or a DataFrame whose first two columns are group and
        user (groups in order of first appearance).  A user that is not in the training data: KeyError.  A user
        repeated within a group counts once; the first appearance fixes the member order."""
        if hasattr(groups, "iloc") and hasattr(groups, "columns"):
            if groups.shape[1] < 2:
                raise ValueError("groups needs two columns: group and user")
            named = {}
            for g, u in zip(groups.iloc[:, 0].tolist(), groups.iloc[:, 1].tolist()):
                named.setdefault(g, []).append(u)
        elif isinstance(groups, dict):
            named = {g: list(us) for g, us in groups.items()}
        else:
            named = dict(enumerate(list(us) for us in groups))
        labels = np.empty(len(named), dtype=object)
        labels[:] = list(named)
        sizes = [len(us) for us in named.values()]
        flat = [u for us in named.values() for u in us]
        ids = self._side("users").request(flat)[0] if flat else np.zeros(0, dtype=np.int32)
        rows = pd.DataFrame({"g": np.repeat(np.arange(len(named)), sizes), "u": ids}).drop_duplicates()
        return labels, (_offsets(np.bincount(rows["g"].to_numpy(), minlength=len(named))),
                        rows["u"].to_numpy().astype(np.int32))

    def recommend_group(self, groups, n=10, aggregate="least_misery", bar=None, exclude_seen=True, weights=None,
                        candidates=None):
        """The ``n`` best items for each GROUP of users -- a household choosing a film, a table of friends choosing a
        restaurant, a campaign that picks one product for a segment -- aggregated on the device without a members x
        items score matrix.  With score(m, i) ``recommend``'s score of member m for item i (the same numbers, bit for
        bit), the group's value of an item is, by ``aggregate``:

        ``"least_misery"``   the LOWEST score any member gives it;
        ``"most_pleasure"``  the HIGHEST;
        ``"approval"``       how many members score it at or above ``bar`` (required for this aggregate, finite, compared
                             with the final score; refused for the others);
        ``"mean"``           the score of the group's mean membership row -- the members' mean score up to rounding.

        ``groups``: a dict {label: iterable of users}, a sequence of iterables (labels 0, 1, ...) or a DataFrame whose
        first two columns are group and user.  A user that is not in the training data: KeyError; a user repeated
        within a group counts once.  Candidates are all training items (``candidates`` as in ``recommend``), without
        every item ANY member has in the training data when ``exclude_seen``.  Order: value descending, equal values
        by ascending encoded item id.

        Returns a DataFrame with columns ``group``, ``items``, ``score``, ``rank`` (1 = best), groups in request order.
        The per-member scores behind a line are ``rerank`` of the (member, item) pairs, with ``exclude_seen=False``
        for the members that have the item.  The model's stored predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        if aggregate not in self._GROUP_AGGREGATES:
            raise ValueError(f"aggregate must be one of {list(self._GROUP_AGGREGATES)}, got {aggregate!r}")
        if aggregate == "approval":
            if bar is None:
                raise ValueError('aggregate="approval" needs a bar')
            bar = check_finite(bar, "bar")
        elif bar is not None:
            raise ValueError(f'bar belongs to aggregate="approval", not to {aggregate!r}')
        mode = self._GROUP_AGGREGATES[aggregate]
        labels, lists = self._group_lists(groups)
        items = self._side("items")
        cand = self._candidate_ids(candidates)
        if cand is not None and len(cand) == 0:
            return self._top_n_frame(None, n, labels[:0], items, self._GROUP_COLUMNS)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            return self._top_n_frame(
                lambda b, e: ctx.recommend_query_groups(*group_slice(lists, b, e), n, mode, bar or 0.0, cand),
                n, labels, items, self._GROUP_COLUMNS)

    # ------------------------------------------------------------------ which items to have at all (not in the reference)
    ASSORTMENT_MAX = 1024            # largest c of assortment (MMSBM_HIP_ASSORT_MAX_C)
    _ASSORTMENT_OBJECTIVES = ("best_score", "reach")

    def assortment(self, c=10, objective="best_score", bar=None, floor=None, given=None, users=None, candidates=None,
                   exclude_seen=True, weights=None):
        """The ``c`` items to HAVE for a set of users -- the titles a shop stocks, the ten items of a newsletter, the
        slots of a programme -- chosen greedily on the device.  The value of a set is not the sum of its items' values:
        a second item that pleases the same users as the first adds almost nothing, so the ``c`` items of highest mean
        score are ``c`` near-copies.  With score(u, i) ``recommend``'s score (the same numbers, bit for bit) and a pair
        counted only when it is eligible (``exclude_seen``: i is not a training item of u), the value of a set S is, by
        ``objective``:

        ``"best_score"``  sum over the users of max(``floor``, the best score an item of S gives them) -- ``floor``
                          (finite; default min(weights), the lowest value a score can take) is what a user is worth who
                          finds nothing; ``bar`` is refused;
        ``"reach"``       the number of users for whom S holds an item they score at or above ``bar`` (required, finite,
                          compared with the final score); ``floor`` is refused.

        Both are monotone submodular, so the greedy rule -- ``c`` times the item of largest marginal gain, equal gains
        to the smaller encoded item id -- is within 1 - 1/e of the best set of ``c``.  It stops early when no item gains
        anything (or none is left), and the frame then has fewer rows.

        ``given``: items already in the assortment ("we stock these, which ``c`` to add"): applied first, in the order
        given, never chosen; they need not be among ``candidates``.  ``users`` (None: every training user; a user named
        twice counts once), ``candidates`` and ``weights`` as in ``recommend``.  Unknown labels: KeyError.  0 <= ``c`` <=
        1,024.

        Returns a DataFrame ``items``, ``gain``, ``total``, ``rank``: each round's item, its gain (in score units; in
        reach mode a whole number of users), the running sum and 1 for the first item chosen.  ``self.assortment_`` =
        {"rounds", "stopped" ("c", "no_gain" or "no_candidates"), "users", "floor" or "bar", "start" (what the given
        items gained over the empty set), "value" (best score: floor + (start + total) / users, the mean best score a
        user finds; reach: the share of users reached), "served" (a frame ``users``, ``items``, ``score``: per served
        user the item of their best score -- reach: the item that covered them first -- read from the device state)}.
        Reach answers depend on the model and the arguments alone; best-score gains are sums of doubles in the launch
        plan's order -- the same bits from call to call, possibly other last bits on another device."""
        self._check_whole_model()
        c = check_integer(c, "c", 0, f"an integer from 0 to {self.ASSORTMENT_MAX}")
        if c > self.ASSORTMENT_MAX:
            raise ValueError(f"c must be an integer from 0 to {self.ASSORTMENT_MAX}, got {c}")
        w = self._rating_weights(weights)
        if objective not in self._ASSORTMENT_OBJECTIVES:
            raise ValueError(f"objective must be one of {list(self._ASSORTMENT_OBJECTIVES)}, got {objective!r}")
        if objective == "reach":
            if bar is None:
                raise ValueError('objective="reach" needs a bar')
            if floor is not None:
                raise ValueError('floor belongs to objective="best_score", not to "reach"')
            level = check_finite(bar, "bar")
        else:
            if bar is not None:
                raise ValueError('bar belongs to objective="reach", not to "best_score"')
            level = float(w.min()) if floor is None else check_finite(floor, "floor")
        users_side, items = self._side("users"), self._side("items")
        ids, labels = users_side.request(users)
        _, first = np.unique(ids, return_index=True)
        first.sort()
        ids, labels = ids[first], labels[first]                                # (a user named twice counts once)
        held = np.zeros(0, dtype=np.int32) if given is None else items.request(list(given))[0]
        held = held[np.sort(np.unique(held, return_index=True)[1])]
        cand = self._candidate_ids(candidates)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            chosen, gains, rounds, stopped, s_items, s_scores, start = ctx.recommend_assortment(
                ids, c, objective, level, held, cand)
        gains = np.asarray(gains, dtype=np.float64)
        total = np.cumsum(gains)
        reached = start + (float(total[-1]) if rounds else 0.0)
        if objective == "reach":
            value = reached / len(ids) if len(ids) else 0.0
        else:
            value = level + reached / len(ids) if len(ids) else level
        got = np.asarray(s_items) >= 0
        served = pd.DataFrame({"users": labels[got], "items": items.label(np.asarray(s_items)[got]),
                               "score": np.asarray(s_scores, dtype=np.float64)[got]})
        self.assortment_ = {"rounds": int(rounds), "stopped": stopped, "users": len(ids),
                            ("bar" if objective == "reach" else "floor"): level, "start": start, "value": value,
                            "served": served}
        return pd.DataFrame({"items": items.label(np.asarray(chosen, dtype=np.int64)), "gain": gains, "total": total,
                             "rank": np.arange(1, rounds + 1, dtype=np.int64)})

    def assortment_value(self, items, objective="best_score", bar=None, floor=None, users=None, exclude_seen=True,
                         weights=None):
        """What a set somebody else picked is worth, by ``assortment``'s arithmetic: ``assortment(c=0, given=items,
        ...)``.  Returns {"value", "start", "served"} of ``self.assortment_`` -- so a hand-made list and the greedy one
        are compared by the same kernels."""
        self.assortment(0, objective, bar, floor, items, users, None, exclude_seen, weights)
        return {k: self.assortment_[k] for k in ("value", "start", "served")}

    # ------------------------------------------------------------------ how far the restarts agree (not in the reference)
    _ROBUST_AGGREGATES = {"lcb": "lcb", "worst": "min", "best": "max"}   # -> HipEM.ENSEMBLE_MODES

    def recommend_robust(self, users=None, n=10, aggregate="lcb", risk=1.0, exclude_seen=True, weights=None,
                         candidates=None, exclude=None):
        """``recommend`` that knows the model is an ensemble: ``fit`` keeps every restart, and ``recommend`` ranks by the
        mean over them -- a pair every restart scores 4.6 and a pair three restarts score 5 and one 3.4 get the same
        number.  Here the value of a pair is formed on the device from the score each restart ALONE gives it
        (``recommend``'s score in a model of that one restart), by ``aggregate``:

        ``"lcb"``    mean - ``risk`` x std over the restarts (population std) -- a lower confidence bound: ``risk`` > 0
                     prefers the items the restarts agree on, 0 ranks by the mean, < 0 explores where they disagree;
        ``"worst"``  the LOWEST score any restart gives the pair;
        ``"best"``   the HIGHEST.

        ``risk`` (finite) belongs to ``"lcb"`` and is refused with the others unless left at its default.  Candidates,
        ``exclude_seen``, ``weights``, ``candidates`` and ``exclude`` as in ``recommend``.  Order: value descending,
        equal values by ascending encoded item id.  A model of one restart answers as ``recommend``.

        Returns ``recommend``'s frame -- ``score`` is the aggregate -- plus ``mean`` and ``std`` of every returned pair:
        columns ``users``, ``items``, ``score``, ``mean``, ``std``, ``rank``.  ``score_spread`` gives the same numbers
        for pairs of the caller's choice.  The model's stored predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        if aggregate not in self._ROBUST_AGGREGATES:
            raise ValueError(f"aggregate must be one of {list(self._ROBUST_AGGREGATES)}, got {aggregate!r}")
        risk = check_finite(risk, "risk")
        if aggregate != "lcb" and risk != 1.0:
            raise ValueError(f'risk belongs to aggregate="lcb", not to {aggregate!r}')
        mode = self._ROBUST_AGGREGATES[aggregate]
        ids, labels = self._side("users").request(users)
        items = self._side("items")
        columns = ("users", "items", "score", "mean", "std")
        cand = self._candidate_ids(candidates)
        if cand is not None and len(cand) == 0:
            return self._top_n_frame(None, n, labels[:0], items, columns)
        extra = self._exclusion_lists(exclude, ids)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            def query(b, e):
                its, scores, counts = ctx.recommend_query_ensemble(ids[b:e], n, mode, risk, cand, group_slice(extra, b, e))
                keep = np.arange(n)[None, :] < counts[:, None]
                stats = ctx.recommend_pair_spread(np.repeat(ids[b:e], counts), its[keep])   # the returned pairs
                mean, std = np.full(its.shape, np.nan), np.full(its.shape, np.nan)
                mean[keep], std[keep] = stats[:, 0], stats[:, 1]
                return its, scores, mean, std, counts
            return self._top_n_frame(query, n, labels, items, columns)

    def score_spread(self, pairs, weights=None, per_restart=False):
        """How far the restarts agree about given (user, item) pairs, on the device: the score each restart alone gives
        the pair (``recommend``'s score in a model of that one restart), summarised over the restarts.

        ``pairs``: a DataFrame whose first two columns are users and items (further columns are ignored, so
        ``model.score_spread(model.recommend(users=[...]))`` works as is), or an iterable of (user, item) tuples; both
        must be in the training data (KeyError).  Returns a DataFrame with columns ``users``, ``items``, ``mean``,
        ``std`` (population form), ``worst``, ``best`` -- the numbers ``recommend_robust`` ranks by, bit for bit -- and,
        with ``per_restart``, ``restart_0``, ``restart_1``, ... in ``self.results`` order; pairs in request order,
        labels as ``recommend`` returns them.  The model's stored predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        w = self._rating_weights(weights)
        us, its = self._pair_columns(pairs)
        uid, ulab = self._side("users").request(us)
        iid, ilab = self._side("items").request(its)
        step = self.RECOMMEND_BATCH_ROWS
        stats, each = [np.zeros((0, 4))], []
        with self._session_of_restarts("recommend", w, False) as ctx:
            for s in range(0, len(uid), step):
                got = ctx.recommend_pair_spread(uid[s:s + step], iid[s:s + step], per_restart)
                stats.append(got[0] if per_restart else got)
                if per_restart:
                    each.append(got[1])
        stats = np.concatenate(stats)
        out = {"users": ulab, "items": ilab, **{c: stats[:, j] for j, c in enumerate(("mean", "std", "worst", "best"))}}
        if per_restart:
            rows = np.concatenate(each, axis=1) if each else np.zeros((len(self.results), 0))
            out.update({f"restart_{s}": rows[s] for s in range(len(rows))})
        return pd.DataFrame(out)

    # ------------------------------------------------------------------ which items to ask about (not in the reference)
    _GAIN_COLUMNS = ("users", "items", "gain")

    def informative_items(self, users=None, n=10, exclude_seen=True, candidates=None, exclude=None):
        """The ``n`` items whose rating would tell most about each training user, on the device.

        A rating of item i by user u is generated as k ~ theta[u], l ~ eta[i], r ~ p[k, l, .].  With the item's rating
        profile q[i, k, :] = sum_l eta[i, l] p[k, l, :] the information the rating carries about the group k the user
        acts from is gain(u, i) = H(sum_k theta[u, k] q[i, k, :]) - sum_k theta[u, k] H(q[i, k, :]) in nats, between 0
        and log min(K, R), mean over the restarts the model holds: zero for an item every group rates alike and for a
        user whose theta is one-hot, largest where the groups the user may belong to disagree.  It does not depend on
        how a restart happens to label its groups.

        Candidates are all training items, without the user's own training items when ``exclude_seen``;
        ``candidates`` and ``exclude`` as in ``recommend``.  Order: gain descending, equal gains by ascending encoded
        item id.  Returns a DataFrame with columns ``users``, ``items``, ``gain``, ``rank`` (1 = most informative),
        users in request order (``users=None``: every training user), labels as ``recommend`` returns them.  The
        model's stored predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        n = check_integer(n, "n", 1)
        ids, labels = self._side("users").request(users)
        items = self._side("items")
        cand = self._candidate_ids(candidates)
        if cand is not None and len(cand) == 0:
            return self._top_n_frame(None, n, labels[:0], items, self._GAIN_COLUMNS)
        extra = self._exclusion_lists(exclude, ids)
        with self._session_of_restarts("inform") as ctx:
            return self._top_n_frame(
                lambda b, e: ctx.inform_query(ids[b:e], n, cand, group_slice(extra, b, e), exclude_seen),
                n, labels, items, self._GAIN_COLUMNS)

    def ask_next(self, data, n=10, candidates=None, prior=1.0, iterations=100, tol=None):
        """The ``n`` items to ask each NEW user about next: ``informative_items`` for users that were not in the
        training data, from the few ratings ``data`` holds of them (users, items, ratings like ``fold_in``'s).

        Each restart's theta comes from ``fold_in`` (same ``iterations`` and ``tol``) and is shrunk towards the
        population, theta_used = (d_u theta_fold + prior theta_bar) / (d_u + prior), where d_u is the user's number of
        known rows in ``data``, theta_bar the restart's mean training theta and ``prior`` a pseudo-count >= 0: a
        maximum-likelihood theta from one or two ratings is close to one-hot, and a one-hot theta has gain 0
        everywhere.  ``prior=0``: the folded theta itself.  The items a user rated in ``data`` are left out;
        ``candidates`` as in ``recommend`` -- the items people can be expected to know.

        Returns ``informative_items``'s frame, users in order of first appearance in ``data``.
        ``self.fold_in_iterations`` as ``fold_in`` leaves it.  The model itself is left as it is."""
        self._check_whole_model()
        n = check_integer(n, "n", 1)
        prior = check_finite(prior, "prior", 0, "a finite number >= 0")
        cand = self._candidate_ids(candidates)
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._encode_new(data, 0)
        if cand is not None and len(cand) == 0:
            return self._top_n_frame(None, n, labels[:0], self._side("items"), self._GAIN_COLUMNS)
        with session(self._ctx(self._device_list()[0]), "inform") as ctx:
            thetas, iters = self._fold_runs(rows, len(labels), iterations, tol, each=lambda c: c.inform_add())
            self.fold_in_iterations = pd.DataFrame(np.stack(iters, 1), index=pd.Index(labels, name="users"))
            theta = np.stack(thetas)                                  # (restarts, new users, K)
            if prior > 0:
                d = np.bincount(rows[:, 0], minlength=len(labels)).astype(np.float64)[None, :, None]
                theta = (d * theta + prior * ctx.inform_mean_theta()[:, None, :]) / (d + prior)
            seen = grouped(rows[:, 0], rows[:, 1], len(labels), sort=True)
            return self._top_n_frame(
                lambda b, e: ctx.inform_query_theta(theta[:, b:e], n, group_slice(seen, b, e), cand),
                n, labels, self._side("items"), self._GAIN_COLUMNS)

    def interview(self, n=10, candidates=None):
        """The ``n`` items to ask a user about whom nothing is known: ``informative_items`` under each restart's mean
        training theta.  ``candidates`` as in ``recommend``.  Returns a DataFrame with columns ``items``, ``gain``,
        ``rank`` (1 = most informative)."""
        self._check_whole_model()
        n = check_integer(n, "n", 1)
        cand = self._candidate_ids(candidates)
        if cand is not None and len(cand) == 0:
            return pd.DataFrame({"items": [], "gain": np.zeros(0), "rank": np.zeros(0, dtype=np.int64)})
        with self._session_of_restarts("inform") as ctx:
            items, gains, counts = ctx.inform_query_theta(ctx.inform_mean_theta()[:, None, :], n, None, cand)
        count = int(counts[0])
        return pd.DataFrame({"items": self._side("items").label(items[0, :count]), "gain": gains[0, :count],
                             "rank": np.arange(1, count + 1, dtype=np.int64)})


def ranking_metrics(users, items, ratings, position, candidates, ks, relevant=None):
    """The dict of ``MMSBM.ranking_score`` from per-row encoded ids, positions and candidate counts (work in
    proportion to the rows).  ``relevant``: a set of rating ids, or None (every pair relevant)."""
    users, items, ratings = (np.asarray(a, dtype=np.int64) for a in (users, items, ratings))
    position, candidates = np.asarray(position, dtype=np.int64), np.asarray(candidates, dtype=np.int64)
    rel_row = np.ones(len(users), dtype=bool) if relevant is None else np.isin(ratings, sorted(relevant))
    # distinct (user, item) pairs: relevant when any of their rows is (the position is the same for every row)
    order = np.lexsort((items, users))
    u, i = users[order], items[order]
    start = np.ones(len(u), dtype=bool)
    start[1:] = (u[1:] != u[:-1]) | (i[1:] != i[:-1])
    pair = np.cumsum(start) - 1
    n_pairs = int(start.sum())
    pu, pp, pc = u[start], position[order][start], candidates[order][start]
    prel = np.zeros(n_pairs, dtype=bool)
    np.logical_or.at(prel, pair, rel_row[order])
    out = {"users": 0, "skipped_users": 0, "pairs": n_pairs, "not_candidates": int((pp == 0).sum())}
    # per user: its relevant candidate pairs sorted by position
    keep = prel & (pp > 0)
    tu, tp, tc = pu[keep], pp[keep], pc[keep]
    o = np.lexsort((tp, tu))
    tu, tp, tc = tu[o], tp[o], tc[o]
    all_users = np.unique(pu)
    ev, first, m = np.unique(tu, return_index=True, return_counts=True)
    n_ev = len(ev)
    out["users"], out["skipped_users"] = n_ev, int(len(all_users) - n_ev)
    grp = np.repeat(np.arange(n_ev), m)
    a = np.arange(len(tu)) - np.repeat(first, m)                   # relevant pairs before each one
    C = tc[first]
    nan = float("nan")
    mean = (lambda v: float(np.mean(v))) if n_ev else (lambda v: nan)
    out["mrr"] = mean(1.0 / tp[first])
    neg = C - m
    ok = neg > 0
    above = np.bincount(grp, weights=(np.repeat(neg, m) - (tp - 1 - a)).astype(np.float64), minlength=n_ev)
    out["auc"] = float(np.mean(above[ok] / (m[ok] * neg[ok]).astype(np.float64))) if ok.any() else nan
    gain = 1.0 / np.log2(tp + 1.0)
    for k in ks:
        inside = tp <= k
        hits = np.bincount(grp, weights=inside.astype(np.float64), minlength=n_ev)
        dcg = np.bincount(grp, weights=np.where(inside, gain, 0.0), minlength=n_ev)
        ideal = np.cumsum(1.0 / np.log2(np.arange(1, max(int(m.max()) if n_ev else 0, 1) + 1) + 1.0))
        idcg = ideal[np.minimum(m, k) - 1] if n_ev else np.zeros(0)
        out[f"precision@{k}"] = mean(hits / k)
        out[f"recall@{k}"] = mean(hits / m)
        out[f"ndcg@{k}"] = mean(dcg / idcg)
        out[f"hit_rate@{k}"] = mean((hits > 0).astype(np.float64))
    return out
