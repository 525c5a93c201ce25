"""The index a context holds, restated in numpy (whole arrays, no samples): the sort stage that layout.hpp builds on
the host and tu_layout.hip on the device, and the properties of the XCD-local work lists (build_worklist_ranges).
Integer data: every comparison against these is plain equality."""
import numpy as np

SORT_ARRAYS = ("pair_off", "pair_user", "pair_item", "rating_off", "user_off", "user_pair", "item_off", "item_pairs",
               "item_deg")
XCDS = 8                   # layout.hpp: kXcds
SMALL_PARTS = 32           # layout.hpp: kSmallSplitParts


def sort_stage(data, n_users, n_items, n_ratings):
    """The nine arrays of the sort stage for (N, 3) triples (user, item, rating), as int64."""
    d = np.asarray(data, dtype=np.int64).reshape(-1, 3)
    u, i, r = d[:, 0], d[:, 1], d[:, 2]
    n = len(d)
    order = np.lexsort((u, i, r))                               # by (rating, item, user)
    pair_user = u[order]
    key = (r * np.int64(n_items) + i)[order]
    head = np.r_[True, key[1:] != key[:-1]] if n else np.zeros(0, dtype=bool)
    first = np.flatnonzero(head)
    pair_item, pair_rating = i[order][first], r[order][first]
    pair_id = np.cumsum(head) - 1                               # per sorted triple: the running count of heads
    by_user = np.argsort(pair_user, kind="stable")
    return {
        "pair_off": np.r_[first, n].astype(np.int64),
        "pair_user": pair_user,
        "pair_item": pair_item,
        "rating_off": np.searchsorted(pair_rating, np.arange(n_ratings + 1)).astype(np.int64),
        "user_off": np.r_[0, np.cumsum(np.bincount(u, minlength=n_users))].astype(np.int64),
        "user_pair": pair_id[by_user],
        "item_off": np.r_[0, np.cumsum(np.bincount(pair_item, minlength=n_items))].astype(np.int64),
        "item_pairs": np.argsort(pair_item, kind="stable").astype(np.int64),
        "item_deg": np.bincount(i, minlength=n_items).astype(np.int64),
    }


def differing(got, want, names=SORT_ARRAYS):
    """Names of the arrays of `got` that are not equal to `want`'s (length or content)."""
    return [nm for nm in names if not np.array_equal(np.asarray(got[nm]).astype(np.int64), np.asarray(want[nm]).astype(np.int64))]


def item_length(n_obs, nseg):
    """layout.hpp: item_length -- triples per work item at most."""
    if nseg <= 0:
        return 64
    mean = max(n_obs // nseg, 1)
    if nseg >= 65536:
        return min(max(64, 4 * mean), 1 << 20)
    if mean <= 16:
        return 64
    want, length = max(n_obs // 65536, 16), 16
    while length * 2 <= want:
        length *= 2
    return min(length, 1 << 20)


def check_work_lists(off, idx, table_rows, n_ranges, items, splits, item_len=None, per_block=None):
    """The properties of one side's XCD-local work list.  off: the segments' offsets; idx: the gathered row of every
    triple in the segments' order (pair_user for the pair segments, user_pair for the user segments); table_rows: rows
    of the gathered table; items / splits: the (m, 4) records (segment, begin, end, partial row or -1) and (segment,
    first partial row, pieces, 0).  item_len: the list's item length (default: item_length of the sizes); per_block:
    work items per workgroup -- given, the placement is checked too: every workgroup holds items of one range and
    lands on an XCD that serves that range.  Returns the number of cut segments."""
    off, idx = np.asarray(off, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    items, splits = np.asarray(items, dtype=np.int64).reshape(-1, 4), np.asarray(splits, dtype=np.int64).reshape(-1, 4)
    nseg, n_obs = len(off) - 1, int(off[-1])
    assert len(idx) == n_obs
    if item_len is None:
        item_len = item_length(n_obs, nseg)
    seg_len = np.diff(off)
    seg_of = np.repeat(np.arange(nseg), seg_len)
    if n_obs > 1:                                               # the rows of a segment ascend
        assert np.all((np.diff(idx) >= 0) | (np.diff(seg_of) != 0)), "gathered rows do not ascend inside a segment"
    range_of = idx * n_ranges // max(int(table_rows), 1)
    assert n_obs == 0 or (range_of.min() >= 0 and range_of.max() < n_ranges)

    null = items[:, 0] < 0
    assert np.all(items[null] == [-1, 0, 0, -1]), "a padding item is not (-1, 0, 0, -1)"
    real = items[~null]
    assert real[:, 0].max(initial=-1) < nseg
    by_seg = real[np.lexsort((real[:, 1], real[:, 0]))]
    seg, beg, end, part = by_seg.T
    count = np.bincount(seg, minlength=nseg)
    assert np.all(count >= 1), ("segments without a work item", np.flatnonzero(count == 0)[:10])
    assert np.all(count[seg_len == 0] == 1), "an empty segment has more than one item"
    start = np.r_[0, np.cumsum(count)]
    # the items of a segment tile it exactly, in order
    assert np.array_equal(beg[start[:-1]], off[:-1]) and np.array_equal(end[start[1:] - 1], off[1:])
    later = np.ones(len(seg), dtype=bool)
    later[start[:-1]] = False
    assert np.array_equal(beg[later], end[np.flatnonzero(later) - 1]), "the items of a segment leave a gap or overlap"
    length = end - beg
    assert np.all(length[seg_len[seg] > 0] > 0), "an empty item in a segment that has triples"
    assert length.max(initial=0) <= item_len, ("an item longer than the list's item length", int(length.max(initial=0)), item_len)
    # ranges
    full = length > 0
    lo, hi = np.zeros(len(seg), dtype=np.int64), np.zeros(len(seg), dtype=np.int64)
    lo[full], hi[full] = range_of[beg[full]], range_of[end[full] - 1]
    cut = count[seg] > 1
    assert np.all(lo[cut] == hi[cut]), "an item of a cut segment holds rows of more than one range"
    assert np.all(part[cut] >= 0) and np.all(part[~cut] == -1)
    short = (seg_len[seg] < 2 * n_ranges) & (seg_len[seg] <= item_len)
    assert np.all((lo == hi) | short | cut), "a segment of several ranges was left whole that is not a short one"
    # a short segment is never cut; any other segment of several ranges always is
    whole_range = np.ones(nseg, dtype=bool)
    if n_obs:
        nonempty = seg_len > 0
        whole_range[nonempty] = range_of[off[:-1][nonempty]] == range_of[off[1:][nonempty] - 1]
    is_short = (seg_len < 2 * n_ranges) & (seg_len <= item_len)
    must_cut = (seg_len > 0) & ~is_short & (~whole_range | (seg_len > item_len))
    assert np.array_equal(count > 1, must_cut), "the set of cut segments is not the rule's"
    # splits: exactly the cut segments; the partial rows are dealt in segment order; those of few pieces come first
    cut_segs = np.flatnonzero(count > 1)
    assert np.array_equal(np.sort(splits[:, 0]), cut_segs)
    sp = splits[np.argsort(splits[:, 0], kind="stable")]
    assert np.array_equal(sp[:, 2], count[cut_segs])
    assert np.array_equal(sp[:, 1], np.r_[0, np.cumsum(sp[:, 2])][:-1])
    assert np.all(splits[:, 3] == 0)
    small = splits[:, 2] <= SMALL_PARTS
    n_small = int(small.sum())
    assert small[:n_small].all() and not small[n_small:].any()
    assert np.all(np.diff(splits[:n_small, 0]) > 0) and np.all(np.diff(splits[n_small:, 0]) > 0)
    first_part = np.full(nseg, -1, dtype=np.int64)
    first_part[sp[:, 0]] = sp[:, 1]
    piece = np.arange(len(seg)) - start[seg]
    assert np.array_equal(part[cut], first_part[seg[cut]] + piece[cut]), "an item's partial row is not its split's"
    if per_block is not None:
        # an item's range: its rows'; a short segment left whole: its middle triple's; an empty segment: range 0
        placed = np.zeros(len(items), dtype=np.int64)
        b, e = items[:, 1], items[:, 2]
        has = ~null & (e > b)
        placed[has] = range_of[(b + (e - b) // 2)[has]]
        assert len(items) % (XCDS * per_block) == 0
        share = XCDS // n_ranges if n_ranges < XCDS else 1
        for blk in range(len(items) // per_block):
            sl = slice(blk * per_block, (blk + 1) * per_block)
            mine = placed[sl][~null[sl]]
            if not len(mine):
                continue
            assert np.all(mine == mine[0]), ("a workgroup holds items of several ranges", blk)
            assert blk % XCDS in {(int(mine[0]) + k * n_ranges) % XCDS for k in range(share)}, ("workgroup on the wrong XCD", blk, int(mine[0]))
    return len(cut_segs)
