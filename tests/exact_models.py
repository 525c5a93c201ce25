"""Models whose recommendation scores carry no rounding at all, and the exact reference built on them (no GPU, no
library): the inputs of test_serving_exact_cpu.py and test_gpu_serving_exact.py and of the serving branch of
scripts/fuzz_parity.py.

Every entry of theta and eta is a multiple of 1/8 (of 2^-m in the strictly monotone families), every entry of p a
multiple of 1/16 and every rating weight a small integer.  Then W = sum_r w_r p_r, the folded side eta W^T (or theta W),
every partial sum of the device's fma chain over the concatenated rank and the numerator
sum_s theta_s W_s eta_s^T are multiples of 2^-10 (2^-(m+7)) far below 2^53: every operation is exact in fp64 whatever
its order, and the division by S is ONE correctly rounded IEEE division of an exact numerator.  So

    exact_scores(u, i) = (sum_s theta_s[u] W_s eta_s[i]^T) / S        (numerator first, one division)

is the device's score bit for bit, and np.lexsort((item, -score)) the one correct order: no tolerance band.
(test_recommend_cpu.restate_scores divides every probability by S before it weights them; for S = 3 that rounds.)
A zero numerator is +0.0 on the device (the chain starts from +0.0 and an exact cancellation rounds to +0.0), so the
reference adds +0.0 to its numerator: numpy's products of a negative weight and a zero would otherwise leave -0.0.
"""
import numpy as np

from test_ranking_cpu import restate_positions
from test_recommend_cpu import restate

TH_DEN, P_DEN = 8, 16
N_RARE = 7                  # items of the better level in the "rare" families: fewer than every N >= 10
BLOCK_FAMILIES = ("sorted", "interleaved", "ascending", "descending", "constant", "rare", "rare_end")
FAMILIES = ("mixed",) + BLOCK_FAMILIES
TIE_FAMILIES = ("sorted", "interleaved", "constant", "rare", "rare_end")     # large tie groups by construction
WEIGHT_KINDS = ("stars", "signed", "indicator")


def dyadic_simplex(rng, shape, den):
    """Array of `shape` whose rows (last axis) are non-negative multiples of 1/den summing to exactly 1; the sparse
    Dirichlet behind the counts makes exact zeros common."""
    n = shape[-1]
    lead = int(np.prod(shape[:-1], dtype=np.int64))
    pv = rng.dirichlet(np.full(n, 0.3), size=lead)
    counts = rng.multinomial(den, pv)
    assert (counts.sum(axis=1) == den).all()
    return (counts / float(den)).reshape(shape)


def weights_of(kind, R):
    """Integer rating weights: 1..R; a vector with zeros and negative entries (scores of 0 and below next to the
    -inf of excluded items); the indicator of the last rating value."""
    if kind == "stars":
        return np.arange(1.0, R + 1)
    if kind == "indicator":
        return np.eye(R)[R - 1]
    assert kind == "signed" and R >= 2, (kind, R)
    w = np.array([float(r % 2) for r in range(R)])
    w[0], w[R - 1] = -2.0, 2.0
    return w


def item_groups(family, I, L):
    """Group of every item in the one-hot block families."""
    ids = np.arange(I)
    if family == "sorted":
        return ids * L // I
    if family in ("interleaved", "constant"):
        return ids % L
    rare = np.zeros(I, dtype=bool)
    if family == "rare_end":
        rare[max(0, I - N_RARE):] = True
    else:
        assert family == "rare", family
        rare[(np.arange(N_RARE) * 2654435761 + 3) % I] = True      # scattered over the catalogue, first id 3
    g = 1 + ids % max(L - 1, 1) if L > 1 else np.zeros(I, dtype=np.int64)
    g[rare] = 0
    return g


def _levels(family, K, L):
    """a[k, l] in 0 .. L: the score level of user group k on item group l before the slot's shift."""
    k, l = np.arange(K)[:, None], np.arange(L)[None, :]
    if family in ("sorted", "interleaved"):                  # even user groups ascend with the item group, odd descend
        return np.where(k % 2 == 0, l, L - 1 - l)
    if family == "ascending":                                # item group 0 (weight i / 2^m) above item group 1
        return np.where(l == 0, 4 + k % 3, k % 2)
    if family == "descending":
        return np.where(l == 0, k % 2, 4 + k % 3)
    assert family in ("rare", "rare_end"), family            # item group 0 (the rare one) above all the others
    return np.where(l == 0, 3 + k % 3, k % 2)


def model(family, rng, U, I, K, L, R, S, weight_kind="stars"):
    """(params, weights): S parameter sets (theta (U, K), eta (I, L), p (K, L, R)) of `family` and integer weights."""
    assert family in FAMILIES, family
    w = weights_of(weight_kind, R)
    if family == "mixed":
        return [(dyadic_simplex(rng, (U, K), TH_DEN), dyadic_simplex(rng, (I, L), TH_DEN),
                 dyadic_simplex(rng, (K, L, R), P_DEN)) for _ in range(S)], w
    assert L <= 9, "block families: level + shift must stay within 0 .. 16"
    theta = np.eye(K)[np.arange(U) % K]
    if family in ("ascending", "descending"):
        assert L >= 2
        m = max(1, int(np.ceil(np.log2(max(I, 2)))))
        eta = np.zeros((I, L))
        eta[:, 0] = np.arange(I) / float(1 << m)             # exact: 2^m >= I
        eta[:, 1] = 1.0 - eta[:, 0]
    else:
        eta = np.eye(L)[item_groups(family, I, L)]
    r_lo, r_hi = int(np.argmin(w)), int(np.argmax(w))        # W rises with the level when the weights differ
    params = []
    for _ in range(S):
        p = np.zeros((K, L, R))
        if family == "constant":
            p[:] = dyadic_simplex(rng, (R,), P_DEN)
        else:
            a = _levels(family, K, L) + rng.integers(0, P_DEN - 9, K)[:, None]   # the slot's shift per user group
            assert a.min() >= 0 and a.max() <= P_DEN
            kk, ll = np.meshgrid(np.arange(K), np.arange(L), indexing="ij")
            p[kk, ll, r_lo] += 1.0 - a / float(P_DEN)
            p[kk, ll, r_hi] += a / float(P_DEN)
        params.append((theta.copy(), eta.copy(), p))
    return params, w


# ---- the exact reference ----------------------------------------------------------------------------------------------
def exact_scores(params, users, n_items, weights):
    """(len(users), n_items): the numerator summed over the slots first, then one division by S."""
    users = np.asarray(users, dtype=np.int64)
    w = np.asarray(weights, dtype=np.float64)
    num = np.zeros((len(users), n_items))
    for theta, eta, p in params:
        assert eta.shape[0] == n_items
        num += (theta[users] @ (p @ w)) @ eta.T
    return (num + 0.0) / float(len(params))


def exact_top_n(scores, users, n, seen=None):
    """(items, scores, counts) as recommend_query returns them, from exact scores (row b = users[b])."""
    return restate(None, users, scores.shape[1], None, n, seen, scores=scores)


def exact_positions(scores, offsets, items, users=None, seen=None):
    """(positions, candidates) as recommend_positions returns them, from exact scores."""
    return restate_positions(scores, offsets, items, users, seen)


def first_n(top, n):
    """The answer for a smaller n out of exact_top_n's for a larger one: the order is total, so it is a prefix."""
    items, scores, counts = top
    return items[:, :n], scores[:, :n], np.minimum(counts, n)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- launch shapes of the serving frame (serve_frame.hpp), restated --------------------------------------------------------------------
REC_MIN_PER, POS_MIN_PER = 1024, 2048     # kRecMinPerPart, kPosMinPerPart
REC_WAVES_PER_CU, POS_GROUPS_PER_CU = 32, 8
CU_COUNTS = (64, 104, 110, 120, 128, 208, 220, 228, 240, 256, 304)


def batch_users(I, n_users, batch_bytes=128 << 20, tile=128):
    """rec_batch_users: users per batch of ~128 MB of scores."""
    bu = min(max(1, batch_bytes // (I * 8)), 32768)
    if bu >= tile:
        bu = bu // tile * tile
    return min(bu, n_users)


def item_parts(I, bu, target, min_per):
    """item_parts: (parts, per) of the split of I items across waves / workgroups."""
    parts = 1
    if bu < target:
        parts = min((target + bu - 1) // bu, (I + min_per - 1) // min_per)
    parts = max(parts, 1)
    per = (I + parts - 1) // parts
    return ((I + per - 1) // per if I > 0 else 1), per


def select_split(I, n_users, cus):
    return item_parts(I, batch_users(I, n_users), REC_WAVES_PER_CU * cus, REC_MIN_PER)


def position_split(I, n_rows, cus):
    return item_parts(I, batch_users(I, n_rows), POS_GROUPS_PER_CU * cus, POS_MIN_PER)


def threshold_group_spans(scores_row, cand, n, per):
    """True when the tie group of the n-th best candidate of the row holds item ids on both sides of a boundary
    between two ranges of `per` items (cand: candidate ids, ascending)."""
    if len(cand) <= n:
        return False
    s = scores_row[cand]
    nth = np.sort(s)[::-1][n - 1]
    grp = cand[s == nth]
    return bool(grp.min() // per != grp.max() // per)


def ties_at(scores_row, cand, n):
    """True when candidates n and n + 1 of the row (1-based, in the order) score exactly the same."""
    if len(cand) <= n:
        return False
    s = np.sort(scores_row[cand])[::-1]
    return bool(s[n - 1] == s[n])


def candidates(I, seen_u):
    cand = np.arange(I)
    return cand if seen_u is None else cand[~np.isin(cand, np.fromiter(seen_u, dtype=np.int64, count=len(seen_u)))]


# ---- training triples built for the edges ---------------------------------------------------------------------------
LEFT = 9                                  # candidates of the "all but" user: fewer than every N >= 10


def edge_triples(rng, U, I, R, n_random, per, best_items=None):
    """Triples (n, 3) and the role of every edge user.  With U >= 4: user 0 has seen every item (no candidate);
    user 1 all of item range [0, per) and all but LEFT items overall; user 2 exactly best_items (its better level;
    nothing when None); user 3 nothing; the others random items.  With U == 3 the roles are all-but, better level and
    nothing; a single user has seen random items."""
    roles = {}
    if U >= 4:
        roles = {0: "all", 1: "all_but", 2: "best", 3: "none"}
    elif U == 3:
        roles = {0: "all_but", 1: "best", 2: "none"}
    rows = []
    for u, role in roles.items():
        if role == "all":
            it = np.arange(I)
        elif role == "all_but":
            assert I >= 2 * LEFT
            keep = (per + rng.choice(I - per, LEFT, replace=False) if I - per >= LEFT
                    else rng.choice(I, LEFT, replace=False))       # (one range: anywhere)
            it = np.setdiff1d(np.arange(I), keep)
        elif role == "best":
            it = np.zeros(0, dtype=np.int64) if best_items is None else np.asarray(best_items(u), dtype=np.int64)
        else:
            it = np.zeros(0, dtype=np.int64)
        rows.append(np.stack([np.full(len(it), u), it, rng.integers(0, R, len(it))], 1))
    free = np.setdiff1d(np.arange(U), np.fromiter(roles, dtype=np.int64, count=len(roles)))
    if len(free) and n_random:
        rows.append(np.stack([rng.choice(free, n_random), rng.integers(0, I, n_random), rng.integers(0, R, n_random)], 1))
    assert sum(len(r) for r in rows) > 0, "a context needs one triple"
    return np.concatenate(rows).astype(np.int64), roles


def best_level(params, I, w):
    """u -> the items of user u's best score level."""
    def items(u):
        s = exact_scores(params, [u], I, w)[0]
        return np.flatnonzero(s == s.max())
    return items


def position_lists(rng, scores, seen, lengths=(0, 1, 4, 5, 16, 17, 33, 200)):
    """(offsets, items): per row a test list whose length cycles through `lengths` (the narrow pass takes at most 4
    keys, a chunk 16) and that holds, as far as it is long enough: the first and the last item id, an excluded item,
    a repeat, and every member (up to 12) of the tie group of a random item; the rest random."""
    n_rows, I = scores.shape
    per, out = [], []
    for b in range(n_rows):
        n = lengths[b % len(lengths)]
        it = rng.integers(0, I, n)
        fixed = [0, I - 1]
        if seen is not None and seen[b]:
            fixed.append(min(seen[b]))
        fixed.append(fixed[0])
        t = int(np.argmax(scores[b])) if b % 2 else int(rng.integers(0, I))   # (the best level: all 7 in "rare")
        fixed.extend(np.flatnonzero(scores[b] == scores[b, t])[:12].tolist())
        m = min(n, len(fixed))
        it[:m] = fixed[:m]
        per.append(n)
        out.extend(it.tolist())
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64), np.asarray(out, dtype=np.int32)


# ---- the cases both test files run ---------------------------------------------------------------------------------
NS = (1, 10, 255, 256, 257, 1023, 1024)
VARIANTS = [(f, k) for f in FAMILIES for k in WEIGHT_KINDS]
# (U, I, K, L, R, S): one range per user, partial 128 x 128 tiles on both sides, rank x slots = 21 and 20
MANY = [(300, 997, 7, 9, 5, 3), (260, 1021, 9, 5, 4, 4)]
# few users over many items: the items split across waves (selection: ranges of 1,000) and merged
# (the position count splits one user's 9,000 items into 5 ranges and 40,000 into 20)
SPLIT = [(1, 5000, 4, 6, 5, 2), (3, 5000, 4, 6, 5, 2), (1, 9000, 4, 6, 5, 2), (1, 40000, 4, 6, 5, 2), (3, 40000, 6, 4, 5, 3)]
# users beyond one batch of 128 MB of scores (128 + 128 + 44), a small rank
BATCHES = (300, 100_003, 4, 6, 3, 1)
GEN_CUS = 256                              # the CU count the edge triples' "whole item range" is laid out for


def case_seed(family, weight_kind, shape):
    return [FAMILIES.index(family), WEIGHT_KINDS.index(weight_kind), *shape]


def make_case(family, weight_kind, shape, n_random=None):
    """One session's inputs and exact answers: params, weights, training triples with the edge users, their seen
    sets, and the exact scores of every user."""
    U, I, K, L, R, S = shape
    rng = np.random.default_rng(case_seed(family, weight_kind, shape))
    params, w = model(family, rng, U, I, K, L, R, S, weight_kind)
    per = select_split(I, U, GEN_CUS)[1]
    data, roles = edge_triples(rng, U, I, R, 20 * U if n_random is None else n_random, per, best_level(params, I, w))
    seen = [set() for _ in range(U)]
    for u, i in zip(data[:, 0].tolist(), data[:, 1].tolist()):
        seen[u].add(i)
    users = np.arange(U, dtype=np.int32)
    return {"shape": shape, "params": params, "w": w, "data": data, "roles": roles, "seen": seen, "users": users,
            "scores": exact_scores(params, users, I, w)}


# ---- fold-in inputs the random grids lack ---------------------------------------------------------------------------
def rows_with_degrees(rng, degrees, n_other, R):
    """Rows [new id, other id, rating] of new users (items) 0 .. len(degrees)-1, shuffled."""
    u = np.repeat(np.arange(len(degrees)), degrees)
    rows = np.stack([u, rng.integers(0, n_other, len(u)), rng.integers(0, R, len(u))], 1)
    return rows[rng.permutation(len(rows))].astype(np.int64)


def impossible_rating_case(rng, U, I, K, L, R, degrees):
    """A model in which rating value R - 1 never occurs (p[:, :, R - 1] = 0) and new users a third of whose rows carry
    it: such a row has probability zero whatever theta.  The last new user holds impossible rows only.
    -> (theta, eta, p), rows, z (impossible rows per new user)"""
    p = np.zeros((K, L, R))
    p[:, :, :R - 1] = rng.random((K, L, R - 1)) + 0.05
    p /= p.sum(axis=2, keepdims=True)
    theta, eta = rng.random((U, K)), rng.random((I, L)) + 0.05
    rows = rows_with_degrees(rng, degrees, I, R - 1)
    n_new = len(degrees)
    for u in range(n_new):
        mine = np.flatnonzero(rows[:, 0] == u)
        rows[mine[:len(mine) if u == n_new - 1 else len(mine) // 3], 2] = R - 1
    z = np.bincount(rows[rows[:, 2] == R - 1, 0], minlength=n_new)
    return (theta, eta, p), rows, z


def disjoint_support_case(rng, U, I, K, L, R, degrees):
    """One-hot eta (item group i % L), p[k, l, 0] = 0 for even k and odd l, and a theta0 whose support is the even k
    for every second new user: its rows (item of an odd group, rating 0) have theta0 . v = 0 although v != 0, and stay
    so, because a zero entry of theta stays zero.  -> (theta, eta, p), rows, theta0, z"""
    assert K >= 2 and L >= 2 and R >= 2
    p = rng.random((K, L, R)) + 0.05
    p[0::2, 1::2, 0] = 0.0
    p /= p.sum(axis=2, keepdims=True)
    eta = np.eye(L)[np.arange(I) % L]
    theta = dyadic_simplex(rng, (U, K), TH_DEN)
    n_new = len(degrees)
    theta0 = rng.random((n_new, K)) + 0.05
    theta0[0::2, 1::2] = 0.0
    theta0 /= theta0.sum(axis=1, keepdims=True)
    rows = rows_with_degrees(rng, degrees, I, R)
    v = np.einsum("klj,jl->jk", p[:, :, rows[:, 2]], eta[rows[:, 1]])
    dead = (theta0[rows[:, 0]] * v).sum(axis=1) == 0.0
    return (theta, eta, p), rows, theta0, np.bincount(rows[dead, 0], minlength=n_new)


def power_of_two_case(rng, U, I, K, L, degrees):
    """R = K a power of two, one-hot eta, and p[:, l, :] a doubly stochastic matrix with entries in multiples of 1/16
    (the mean of 16 permutation matrices): from the uniform theta0 = 1/K every row's dot product is exactly 1/K, its
    reciprocal K, and theta'[u, k] = (sum_j p[k, l_j, r_j]) / d_u -- an exact sum and ONE division, in either form of
    the kernel.  -> (theta, eta, p), rows, expected theta after one iteration"""
    assert K & (K - 1) == 0
    p = np.zeros((K, L, K))
    for l in range(L):
        for _ in range(P_DEN):
            p[np.arange(K), l, rng.permutation(K)] += 1.0 / P_DEN
    eta = np.eye(L)[np.arange(I) % L]
    theta = dyadic_simplex(rng, (U, K), TH_DEN)
    rows = rows_with_degrees(rng, degrees, I, K)
    acc = np.zeros((len(degrees), K))
    np.add.at(acc, rows[:, 0], p[:, rows[:, 1] % L, rows[:, 2]].T)
    return (theta, eta, p), rows, acc / np.asarray(degrees, dtype=np.float64)[:, None]


def transposed(model_params, rows):
    """The same problem with the sides exchanged (test_gpu_fold_in_items.test_transposition_identity):
    fold_in_items of it is fold_in of the original."""
    theta, eta, p = model_params
    return (eta, theta, np.ascontiguousarray(p.transpose(1, 0, 2))), np.ascontiguousarray(rows[:, [1, 0, 2]])


FOLD_KS = (4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
FOLD_LANES = ((4, 1), (8, 2), (16, 4), (32, 8), (64, 16), (128, 32), (1 << 30, 64))   # fold_code / fold_lanes: K <= a -> G


def fold_lanes(K):
    return next(g for top, g in FOLD_LANES if K <= top)


def fold_waves(degrees, K):
    """The users of every wave of the on-chip form, as tu_fold_in.hip packs them: in request order, a new wave when
    the 64 / G groups are taken or the users' rows would exceed 1,024 doubles of LDS."""
    gpw, waves, used = 64 // fold_lanes(K), [], 0
    for u, d in enumerate(degrees):
        if d == 0 or d * K > 1024:
            continue
        if not waves or len(waves[-1]) == gpw or used + d * K > 1024:
            waves.append([])
            used = 0
        waves[-1].append(u)
        used += d * K
    return waves


def border_degrees(K):
    """Degrees on both sides of the border d * K = 1024 between the form that keeps a user's rows on chip and the
    streamed one, then enough short users (1-3 rows) that several share one wave's 1,024 doubles of LDS and that the
    last wave of the request is partly empty whenever a wave holds more than one user."""
    top = 1024 // K
    gpw = 64 // fold_lanes(K)
    deg = [top, top + 1] + ([1 + j % 3 for j in range(gpw + 3)] if top >= 3 else [1] * 3) + [2 * top + 5]
    if gpw > 1 and len(fold_waves(deg, K)[-1]) == gpw:
        deg.append(1)
    return deg


def likelihood_floor(K, d, lik=0.0):
    """How far rounding alone can push sum_j log(theta_u . v_j) down from one iteration to the next, although EM
    never decreases it: the d dot products carry K products and K - 1 additions each, theta itself the K + d roundings
    of its update (each moving a log by as much, relatively), the logs and their sum one rounding each (2^-52)."""
    d = np.asarray(d, dtype=np.float64)
    return (d * (2 * K + d + 4) + np.abs(lik)) * 2.0 ** -52
