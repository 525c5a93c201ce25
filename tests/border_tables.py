"""Designed triple tables: training data that sits on the borders of the EM kernels' index arithmetic.

Every other training table of the suite is a random draw, which reaches a given side of a border (a segment of exactly
one chunk of indices, of 32 or 33 pieces, a rating of 320 or 321 slabs, an (item, rating) grid that is exactly half
full ...) only by chance.  Duplicate triples are allowed, so ANY list of user degrees and ANY list of (item, rating)
pair sizes with the same sum can be realised: make_table() lists the pair slots, lists the user slots and matches them
through a seeded permutation.  The named tables below are built on it; test_border_tables_cpu.py asserts from
core.build_layout that each of them holds the borders it is named after on both sides, DESIGN section 6 lists the
borders by file and line.

"Users" and "pairs" are the INTERNAL sides of a context (layout.hpp): swap_sides = 1 makes the items the segment side
and (user, rating) the pairs, so every table comes in two forms -- Table.data for swap_sides = 0 and Table.swapped
(columns 0 and 1 exchanged) for swap_sides = 1 -- which give a context the same internal index.
"""
import collections

import numpy as np

from oracle import mmsbm_oracle as orc

ITEM_LEN = 64              # layout.hpp: kMaxItemLen
SMALL_PARTS = 32           # layout.hpp: kSmallSplitParts
UNIT = 64                  # layout.hpp: kMvChunkPairs / shapes.hpp: kUnitPairs
XCDS = 8                   # layout.hpp: kXcds -- a populated rating's units are padded to a multiple of it (R > 1)
SLAB_ROUND = 320           # eta_p.hpp: kRedRows * kRedBatch slabs of one rating per trip of p_update_block's `off` loop
RED_GROUP = 6              # eta_p.hpp: kRedGroup ratings per LDS pass
GRID_MAX_R = 16            # tu_create.hip: upload_item_grid
BLOCK = 256                # common.hpp: kBlock
FUSED_SPLIT_LDS = 96 * 1024   # shapes.hpp: kFusedSplitLds


class Table(collections.namedtuple("Table", "name data dims")):
    """data: (n, 3) int64 triples (user, item, rating) whose INTERNAL sides at swap_sides = 0 are the designed ones."""

    @property
    def swapped(self):
        """The same design on the other side layout: for a context created with swap_sides = 1."""
        return np.ascontiguousarray(self.data[:, [1, 0, 2]])

    @property
    def swapped_dims(self):
        return (self.dims[1], self.dims[0], self.dims[2])

    def form(self, swap):
        return (self.swapped, self.swapped_dims) if swap else (self.data, self.dims)


def make_table(name, user_degrees, pair_sizes, seed=0):
    """user_degrees[u] = triples of user u (0: the id never occurs); pair_sizes[r][i] = triples of the pair (item i,
    rating r) (0: no such pair; a short list leaves the items beyond it without that rating).  Both must have the same
    sum.  The pair slots in (rating, item) order meet the user slots through a seeded permutation; the rows are then
    shuffled, so nothing is pre-sorted."""
    deg = np.asarray(user_degrees, dtype=np.int64)
    n_items = max(len(s) for s in pair_sizes)
    n_ratings = len(pair_sizes)
    items, ratings = [], []
    for r, sizes in enumerate(pair_sizes):
        sizes = np.asarray(sizes, dtype=np.int64)
        items.append(np.repeat(np.arange(len(sizes)), sizes))
        ratings.append(np.full(int(sizes.sum()), r, dtype=np.int64))
    items, ratings = np.concatenate(items), np.concatenate(ratings)
    users = np.repeat(np.arange(len(deg)), deg)
    assert len(users) == len(items), (name, len(users), len(items))
    rng = np.random.default_rng([seed, len(users)])
    data = np.stack([users[rng.permutation(len(users))], items, ratings], axis=1)
    data = np.ascontiguousarray(data[rng.permutation(len(data))]).astype(np.int64)
    return Table(name, data, (len(deg), n_items, n_ratings))


def fill(lengths, total, unit=1):
    """`lengths` followed by as many segments of `unit` triples (the last one shorter) as bring the sum to `total`."""
    rest = total - int(np.sum(lengths))
    assert rest >= 0, rest
    return list(lengths) + [unit] * (rest // unit) + ([rest % unit] if rest % unit else [])


def place(sizes, n_ratings):
    """A flat list of pair sizes as pair_sizes[r][i]: entry j goes to rating j % R of the (j // R)-th USED item.  The
    first, the middle and the last item id stay without any triple."""
    n_real = -(-len(sizes) // n_ratings)
    width = n_real + 3
    real = [i for i in range(width) if i not in (0, width // 2, width - 1)]
    out = [[0] * width for _ in range(n_ratings)]
    for j, s in enumerate(sizes):
        out[j % n_ratings][real[j // n_ratings]] = s
    return out


def with_gaps(degrees):
    """User degrees with an id that never occurs at the start, in the middle and at the very end."""
    half = len(degrees) // 2
    return [0] + list(degrees[:half]) + [0] + list(degrees[half:]) + [0]


def even_degrees(n, per):
    """n triples over users of `per` triples each (the last one takes the rest)."""
    return [per] * (n // per) + ([n % per] if n % per else [])


# ---- `segments`: lengths around the chunk of indices, the work-item cut, 32 / 33 pieces, the second trip of the big combine ----
def odd_round_pieces(g):
    """The smallest piece count beyond 33 that ends INSIDE a round of seg_combine_big: its NG = 256 / g groups add four
    pieces each per trip (j0 + i NG, i = 0 .. 3), and 32, 33, 4 NG and 4 NG + 1 pieces all end on a round's border or
    one piece past it, where the first piece a group must NOT add is never reached by its i loop."""
    ng = BLOCK // g
    p = SMALL_PARTS + 2
    while not ((p // ng) % 4 == 1 and p % ng == 1):
        p += 1
    return p


def segment_lengths(item_len, g):
    """1 .. 130 (2 CH + 1 for every CH up to 64, and item_len - 1, item_len, item_len + 1 at both item lengths), then
    the lengths that give exactly 32 and 33 pieces, for the NG = 256 / g groups of seg_combine_big 4 NG and 4 NG + 1
    pieces (the longest and the shortest segment of that piece count respectively), and odd_round_pieces(g)."""
    ng4 = 4 * (BLOCK // g)
    longs = {SMALL_PARTS * item_len, SMALL_PARTS * item_len + 1, ng4 * item_len, ng4 * item_len + 1,
             odd_round_pieces(g) * item_len - 3}
    return list(range(1, 131)) + sorted(x for x in longs if x > 130)


def segments(item_len, g, n_ratings=3, seed=1):
    """Both sides hold every length of segment_lengths() and ids that never occur (length 0) at the start, in the
    middle and at the end.  item_length() (layout.hpp) gives 64 while a side's mean segment is at most 16 triples,
    else 16 at this size: the 64 form pads both sides with segments of one triple, the 16 form pads nothing."""
    assert item_len in (16, 64)
    core = segment_lengths(item_len, g)
    n = int(np.sum(core))
    total = n + n // 14 + 1 if item_len == 64 else n
    return make_table(f"segments{item_len}-g{g}", with_gaps(fill(core, total)), place(fill(core[::-1], total), n_ratings), seed)


def segments_short(n_ratings=3, seed=2):
    """The 0 .. 130 part alone (wide rows: the long-double reference of 600 x 5 costs 50 KB per triple)."""
    core = list(range(1, 131))
    return make_table("segments-short", with_gaps(core), place(core[::-1], n_ratings), seed)


# ---- `units`: pairs per rating around the 64-pair unit, the 8-unit padding, 320 slabs and the passes of six ratings ----
UNITS = {
    "r1": [513],
    "r5": [0, 1, 63, 64, 65],
    "r6": [130, 0, 513, 3, 20481, 0],
    "r7": [0, 511, 512, 20480, 65, 63, 1],
    "r12": [1, 63, 64, 65, 511, 512, 0, 513, 1, 64, 65, 0],
    "r13": [64, 1, 0, 65, 63, 512, 513, 511, 1, 0, 64, 65, 20481],
    "chunk": [1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025],   # big tiles: 256 / 512 / 1,024 pairs per workgroup
}


def units(kind, seed=3):
    """Rating r has UNITS[kind][r] pairs (items 0 .. c - 1), every seventh pair two triples, the others one; users of
    six triples each."""
    counts = UNITS[kind]
    sizes = [[2 if i % 7 == 3 else 1 for i in range(c)] for c in counts]
    n = sum(sum(s) for s in sizes)
    return make_table(f"units-{kind}", even_degrees(n, 6), sizes, seed)


# ---- `whole_segments`: the limits of the two-launch form's whole-segment lists (K = L = 20: rows of 20, 8 lanes, item_len 16) ----
def whole_segments(kind, kp=20, g=8, item_len=16, seed=4):
    """kind "fits": a pair of exactly 64 pieces and a user whose kFusedSplitLds / (8 kp) partial rows just fit, so both
    lists are built; "pair65": a pair of 65 pieces (build_mv_chunks_capped gives up); "user_over": one partial row too
    many.  All three hold, per side, a run of segments of two pieces that fills a workgroup's cap of work items exactly
    (64 per pair unit, 256 / g per user workgroup) followed by a run that would pass it by one."""
    rows_fit = FUSED_SPLIT_LDS // (8 * kp)
    user_big = (rows_fit + (kind == "user_over")) * item_len - (item_len - 1 if kind == "user_over" else 0)
    pair_big = (UNIT + (kind == "pair65")) * item_len - (item_len - 1 if kind == "pair65" else 0)
    two, three = item_len + 1, 2 * item_len + 1
    ucap = BLOCK // g
    users = [user_big] + [two] * (ucap // 2) + [two] * (ucap // 2 - 1) + [three] + [two] * 3 + [5, 1, item_len]
    # rating 0: the pair runs (item order = pair order inside a rating); rating 1: the big pair and the rest
    run = [two] * (UNIT // 2) + [two] * (UNIT // 2 - 1) + [three] + [two] * 3
    n_u = int(np.sum(users))
    rest = n_u - int(np.sum(run)) - pair_big
    assert rest > 0, rest
    other = [pair_big] + fill([], rest, 20)
    return make_table(f"whole-{kind}", users, [run, other], seed)


# ---- `grid`: the density rule of the dense item grid and its rounds of 8, 4, 2 and 1 ----
CSR_COUNTS = (0, 1, 7, 8, 9, 16, 17)


def grid(n_ratings, kind, n_items=72, seed=5):
    """kind "full": every (item, rating) combination.  "dense": every one but a hole at the first rating of item 1, at the last rating of
    item 2 and the whole of item 3.  "half" / "below": exactly half of the I x R combinations, or one fewer -- the
    items hold 0, 1, 7, 8, 9, 16, 17 ... pairs (cut to R) at rotating ratings.  "csr": the same counts, whatever their
    sum.  Every fifth pair has two triples."""
    occ = np.zeros((n_items, n_ratings), dtype=bool)
    if kind == "full":
        occ[:] = True
    elif kind == "dense":
        occ[:] = True
        occ[1, 0] = False
        occ[2, n_ratings - 1] = False
        occ[3, :] = False
    else:
        counts = [min(CSR_COUNTS[i % len(CSR_COUNTS)], n_ratings) for i in range(n_items)]
        if kind in ("half", "below"):
            assert n_items * n_ratings % 2 == 0
            want = n_items * n_ratings // 2 - (kind == "below")
            i = n_items - 1
            while sum(counts) != want:          # the later items give or take until the sum is exact
                step = 1 if sum(counts) < want else -1
                if 0 <= counts[i] + step <= n_ratings and (i % len(CSR_COUNTS)) not in (0, 1):
                    counts[i] += step
                i = i - 1 if i > len(CSR_COUNTS) else n_items - 1
        for i, c in enumerate(counts):
            occ[i, [(i + j) % n_ratings for j in range(c)]] = True
    sizes = [[(2 if (i + r) % 5 == 0 else 1) if occ[i, r] else 0 for i in range(n_items)] for r in range(n_ratings)]
    n = sum(sum(s) for s in sizes)
    return make_table(f"grid-{kind}-r{n_ratings}", even_degrees(n, 5), sizes, seed)


# ---- `sort_sizes`: the device-built index at sizes of 1, 2, 2^k and 2^k + 1 ----
def sort_sizes():
    """name -> Table; the ids are uniform draws inside the dims unless the name says otherwise."""
    out = {}
    rng = np.random.default_rng(6)

    def add(name, n, n_u, n_i, n_r, rows=None):
        if rows is None:
            rows = np.stack([rng.integers(0, n_u, n), rng.integers(0, n_i, n), rng.integers(0, n_r, n)], axis=1)
        out[name] = Table("sort-" + name, np.ascontiguousarray(rows, dtype=np.int64), (n_u, n_i, n_r))
    add("one-triple", 1, 1, 1, 1)
    add("one-triple-of-many-ids", 1, 5, 4, 3, np.array([[2, 1, 1]]))
    add("all-the-same-triple", 700, 5, 4, 3, np.tile(np.array([[3, 2, 1]]), (700, 1)))     # (the last rating has no row)
    add("one-user", 300, 1, 2, 2)
    add("one-item", 300, 2, 1, 2)
    add("u256-i257-r1", 3000, 256, 257, 1)
    add("u257-i256-r4", 3000, 257, 256, 4)                # R x I = 1,024
    add("u1024-i1025-r1", 5000, 1024, 1025, 1)
    add("u1025-i64-r16", 5000, 1025, 64, 16)              # R x I = 1,024
    add("u2-i2-r2", 64, 2, 2, 2)
    rows = np.stack([rng.integers(0, 64, 2000), rng.integers(0, 32, 2000), rng.integers(0, 4, 2000)], axis=1)
    add("empty-last-rating", 2000, 64, 32, 5, rows)       # rating 4 never occurs
    return out


# ---- `pairmean`: the likelihood's wave-per-pair form needs 2.5 triples per pair on average (tu_once.hip: lik_pairs_usable) ----
def pairmean(kind, seed=7):
    """400 pairs of 2 and 3 triples in turn: 2 n = 5 pairs exactly ("at"); one triple fewer ("below")."""
    sizes = [[2, 3] * 100, [3, 2] * 100]
    if kind == "below":
        sizes[1][0] = 2
    n = sum(sum(x) for x in sizes)
    return make_table(f"pairmean-{kind}", even_degrees(n, 9), sizes, seed)


# ---- what core.build_layout says about a table (CPU only) ----
def layout_of(table, fused_caps=None):
    from mmsbm_amd.core import build_layout
    return build_layout(table.data, *table.dims, fused_caps=fused_caps)


def side_facts(lay, side):
    """lengths: triples per segment; pieces: work items per segment (1: whole); item_len: the longest piece."""
    off = lay["user_off" if side == "users" else "pair_off"].astype(np.int64)
    lengths = np.diff(off)
    pieces = np.ones(len(lengths), dtype=np.int64)
    splits = lay["user_splits" if side == "users" else "pair_splits"]
    if len(splits):
        pieces[splits[:, 0]] = splits[:, 2]
    items = lay["user_items" if side == "users" else "pair_items"]
    cut = items[items[:, 3] >= 0] if len(items) else items
    item_len = int((cut[:, 2] - cut[:, 1]).max()) if len(cut) else None
    return dict(lengths=lengths, pieces=pieces, item_len=item_len, n_items=len(items))


def units_per_rating(lay, n_ratings):
    """(units, empty units, pairs) per rating of the 64-pair unit list."""
    mv = lay["mv_chunks"]
    out = []
    for r in range(n_ratings):
        mine = mv[mv[:, 0] == r]
        out.append((len(mine), int(np.sum(mine[:, 1] == mine[:, 2])), int(lay["rating_off"][r + 1] - lay["rating_off"][r])))
    return out


# ---- the reference: one M-step in np.longdouble ----
def longdouble_step(data, theta, eta, pr, d_u, d_i, rows=4096):
    """update_coefficients and the normalisations of em_step in np.longdouble: the same max(s, eps), the same zero-row
    guard of p.  Returns (numerators, parameters), rounded to float64.  (`rows` triples at a time: the (N, K, L)
    tensor of a wide shape would not fit; in long double the order of the slabs is far below a float64 ulp.)"""
    ld = np.longdouble
    th, et, p = theta.astype(ld), eta.astype(ld), pr.astype(ld)
    p_r = np.moveaxis(p, 2, 0)
    n_theta, n_eta, n_pr = np.zeros_like(th), np.zeros_like(et), np.zeros_like(p)
    for lo in range(0, len(data), rows):
        u, i, r = (data[lo:lo + rows, j] for j in range(3))
        om = th[u][:, :, None] * et[i][:, None, :] * p_r[r]
        inc = om / np.maximum(om.sum(axis=(1, 2)), ld(orc.EPS))[:, None, None]
        np.add.at(n_theta, u, inc.sum(axis=2))
        np.add.at(n_eta, i, inc.sum(axis=1))
        for rr in np.unique(r):
            n_pr[:, :, rr] += inc[r == rr].sum(axis=0)
    tot = n_pr.sum(axis=2, keepdims=True)
    params = (n_theta / d_u[:, None].astype(ld), n_eta / d_i[:, None].astype(ld), n_pr / np.where(tot == 0, ld(1), tot))
    return tuple(a.astype(np.float64) for a in (n_theta, n_eta, n_pr)), tuple(a.astype(np.float64) for a in params)


def longdouble_likelihood(data, theta, eta, pr, rows=4096):
    """compute_likelihood (sum of w log w - w log s, w = max(omega, eps), s = max(sum omega, eps)) in np.longdouble.
    The triples none of whose elements can be clamped (min theta_u min eta_i min p_r >= 2 eps, a lower bound of every
    omega) are summed in factorised form where the tensor is large -- sum_kl omega log omega = sum_k theta log theta A +
    sum_k theta D with A = P eta, D = P (eta log eta) + (P log P) eta (oracle/mmsbm_factorised.py), every term in long
    double --, all others element by element; test_border_tables_cpu.py holds the two forms together."""
    ld = np.longdouble
    th, et, p_r = theta.astype(ld), eta.astype(ld), np.moveaxis(pr.astype(ld), 2, 0)
    u, i, r = (data[:, j] for j in range(3))
    clear = theta.min(axis=1)[u] * eta.min(axis=1)[i] * pr.reshape(-1, pr.shape[2]).min(axis=0)[r] >= 2 * orc.EPS
    if len(data) * theta.shape[1] * eta.shape[1] <= 2_000_000:
        clear[:] = False
    total = longdouble_likelihood_factorised(data[clear], th, et, p_r) if clear.any() else ld(0)
    rest = data[~clear]
    for lo in range(0, len(rest), rows):
        u, i, r = (rest[lo:lo + rows, j] for j in range(3))
        om = th[u][:, :, None] * et[i][:, None, :] * p_r[r]
        w = np.maximum(om, ld(orc.EPS))
        s = np.maximum(om.sum(axis=(1, 2)), ld(orc.EPS))
        total += np.sum(w * np.log(w) - w * np.log(s)[:, None, None])
    return float(total)


def longdouble_likelihood_factorised(data, th, et, p_r):
    """(th, et: long double; p_r: (R, K, L) long double; no omega of these triples below eps)"""
    ld = np.longdouble
    u, i, r = (data[:, j] for j in range(3))
    key = r * et.shape[0] + i
    uniq, q = np.unique(key, return_inverse=True)
    q = q.reshape(-1)
    q_item, q_rating = uniq % et.shape[0], uniq // et.shape[0]

    def xlogx(x):
        return x * np.log(x)
    a_tab, d_tab = np.zeros((len(uniq), th.shape[1]), dtype=ld), np.zeros((len(uniq), th.shape[1]), dtype=ld)
    for rr in np.unique(q_rating):
        rows = q_rating == rr
        e = et[q_item[rows]]
        a_tab[rows] = e @ p_r[rr].T
        d_tab[rows] = xlogx(e) @ p_r[rr].T + e @ xlogx(p_r[rr]).T
    total, th_log = ld(0), xlogx(th)
    for lo in range(0, len(data), 8192):
        sl = slice(lo, lo + 8192)
        t, a, d = th[u[sl]], a_tab[q[sl]], d_tab[q[sl]]
        s = np.sum(t * a, axis=1)
        total += np.sum(np.sum(th_log[u[sl]] * a + t * d, axis=1) - s * np.log(s))
    return total


def friendly_start(table, k, l, seed=11):
    """orc.init_params on the table: memberships of one magnitude, nothing zero."""
    d_u, d_i = orc.degrees(table.data, table.dims[0], table.dims[1])
    return orc.init_params(seed, *table.dims, k, l, d_u, d_i), d_u, d_i


def swapped_params(arrays):
    """(theta, eta, p)-like triple of the other side layout: the sides exchanged, every rating tile transposed."""
    a, b, c = arrays
    return np.ascontiguousarray(b), np.ascontiguousarray(a), np.ascontiguousarray(np.transpose(c, (1, 0, 2)))


def segment_sum(values, ids, n):
    """out[j] = sum of the rows of `values` with ids == j, each sum taken in row order (np.add.at, only fast)."""
    out = np.zeros((n,) + values.shape[1:], dtype=values.dtype)
    if len(ids):
        order = np.argsort(ids, kind="stable")
        sorted_ids = ids[order]
        first = np.flatnonzero(np.r_[True, sorted_ids[1:] != sorted_ids[:-1]])
        out[sorted_ids[first]] = np.add.reduceat(values[order], first, axis=0)
    return out


def longdouble_factorised_step(data, theta, eta, pr, d_u, d_i):
    """The same M-step in np.longdouble WITHOUT the (N, K, L) tensor, for the shapes whose tensor is out of reach
    (600 x 5 on 8,515 triples is 400 MB of long doubles): the sums of oracle/mmsbm_factorised.py's docstring, every
    product and sum in long double.  With a 64-bit mantissa either association order is within a few 1e-19 of the
    exact sum per term, so after rounding to float64 the two restatements differ by an ulp or two at a few entries;
    test_border_tables_cpu.py holds them to 20,481 x 2^-64 + 2^-52 = 1.3e-15 of each other on every table."""
    ld = np.longdouble
    u, i, r = (data[:, j] for j in range(3))
    th, et, p = theta.astype(ld), eta.astype(ld), pr.astype(ld)
    key = r * eta.shape[0] + i
    uniq, q = np.unique(key, return_inverse=True)
    q = q.reshape(-1)
    q_item, q_rating = uniq % eta.shape[0], uniq // eta.shape[0]
    a_tab = np.zeros((len(uniq), theta.shape[1]), dtype=ld)
    for rr in np.unique(q_rating):
        rows = q_rating == rr
        a_tab[rows] = et[q_item[rows]] @ p[:, :, rr].T
    s = np.sum(th[u] * a_tab[q], axis=1)
    w = 1 / np.maximum(s, ld(orc.EPS))
    n_theta = th * segment_sum(w[:, None] * a_tab[q], u, len(th))
    c_tab = segment_sum(w[:, None] * th[u], q, len(uniq))
    n_pr, t_tab = np.zeros_like(p), np.zeros((len(uniq), et.shape[1]), dtype=ld)
    for rr in np.unique(q_rating):
        rows = q_rating == rr
        t_tab[rows] = c_tab[rows] @ p[:, :, rr]
        n_pr[:, :, rr] = p[:, :, rr] * (c_tab[rows].T @ et[q_item[rows]])
    n_eta = et * segment_sum(t_tab, q_item, len(et))
    tot = n_pr.sum(axis=2, keepdims=True)
    params = (n_theta / d_u[:, None].astype(ld), n_eta / d_i[:, None].astype(ld), n_pr / np.where(tot == 0, ld(1), tot))
    return tuple(a.astype(np.float64) for a in (n_theta, n_eta, n_pr)), tuple(a.astype(np.float64) for a in params)


DENSE_LD_MAX = 10_000_000      # N K L up to which the reference is the dense long-double restatement


def reference_step(data, theta, eta, pr, d_u, d_i):
    if len(data) * theta.shape[1] * eta.shape[1] <= DENSE_LD_MAX:
        return longdouble_step(data, theta, eta, pr, d_u, d_i)
    return longdouble_factorised_step(data, theta, eta, pr, d_u, d_i)


# ---- the registry the CPU and the GPU module share ----
# (item_len, g, K, L): the internal row length K (padded to a multiple of 4) selects the group of g lanes (shapes.hpp: group_code)
SEGMENT_CASES = [(64, 4, 10, 10), (16, 4, 10, 10), (64, 8, 20, 12), (16, 16, 50, 50), (16, 32, 80, 80)]
GRID_R = tuple(range(1, 18))
FULL_R = (1, 7, 11, 16)         # R of the tables with every (item, rating) combination: one round at B = 8, 8 + 2 + 1, two full rounds
DENSITY_R = (2, 4, 9, 16)      # R at which the tables with exactly half of the combinations, and one fewer, are built
_CACHE = {}


def table(name):
    """Every named table, built once: "segments64-g4", "segments-short", "units-r6", "whole-fits", "grid-dense-r9",
    "sort-one-triple" ..."""
    if name not in _CACHE:
        kind, _, rest = name.partition("-")
        if name == "segments-short":
            t = segments_short()
        elif kind.startswith("segments"):
            t = segments(int(kind[len("segments"):]), int(rest[1:]))
        elif kind == "units":
            t = units(rest)
        elif kind == "whole":
            t = whole_segments(rest)
        elif kind == "grid":
            what, _, r = rest.partition("-r")
            t = grid(int(r), what)
        elif kind == "pairmean":
            t = pairmean(rest)
        elif kind == "sort":
            t = sort_sizes()[rest]
        else:
            raise KeyError(name)
        assert t.name == name, (t.name, name)
        t.data.setflags(write=False)
        _CACHE[name] = t
    return _CACHE[name]


def all_names():
    names = [f"segments{il}-g{g}" for il, g, _, _ in SEGMENT_CASES] + ["segments-short"]
    names += [f"units-{k}" for k in UNITS] + [f"whole-{k}" for k in ("fits", "pair65", "user_over")]
    names += [f"grid-dense-r{r}" for r in GRID_R] + [f"grid-{k}-r{r}" for r in DENSITY_R for k in ("half", "below")]
    names += [f"grid-full-r{r}" for r in FULL_R] + ["grid-csr-r16", "grid-csr-r17", "pairmean-at", "pairmean-below"] + ["sort-" + n for n in sort_sizes()]
    return names
