"""Cases, long-double references and check functions of the five serving entry points that were merged with their
feature tests only -- explain, the item side (recommend_query_items / recommend_audience), recommendation within a part
of the catalogue (recommend_query_within / recommend_rank), recommend_diverse and overlap_query -- on the late-stage
parameter families of staged_params.py.  Shared by test_gpu_staged_serving.py (the device) and
test_staged_serving_cpu.py (which pins the inputs, shows the references inside their own bounds and runs the same check
functions through the CPU stand-ins).  A plain module.

Models: staged_after_fit.family_slots(family, ..., n_slots = 3) -- S = 3 ON PURPOSE: dividing by S and by S d_u rounds --
with zeroed users and items.  (K, L) in SHAPES; (7, 33) is where exp_row_kernel's v chain passes L = 16 and waits in the
c buffer.  U = 120, I = 300, about 25 uniform rows per user; planted users with 1, 63, 64, 65 and 300 rows (the last
takes the four-rows-per-lane round of exp_pair_kernel); a zeroed user among the planted ones, a zeroed item in the
planted histories; duplicated triples.

THE BOUNDS.  Every quantity below is a sum of products of non-negative numbers with non-negative weights, so a chain of
n roundings gives a relative error of at most n 2^-53 (1 + o(1)) of the EXACT value whatever the magnitudes of the
terms; as in staged_after_fit.score_bound the count is multiplied by 2^-52.  One contribution a(u, t, j) passes through

    the W chain             W[k, l] = sum_r w_r p[k, l, r]                                   R
    the fold chain of G     G[t, k] = sum_l W[k, l] eta[t, l]                                L
    the v chain             v_j[k]  = sum_l p[k, l, r_j] eta[i_j, l]                         L
    the dot chain           theta_u . v_j over k (it enters through 1 / max(dot, eps))       K
    theta[k] v[k], the ONE division 1 / max(dot, eps), the multiply by it                    3
    the chain over f = s K + k of c_{s,j}[k] G_s[t, k]                                       S K
    the division by S d_u                                                                    1

    contribution_bound = (R + 2 L + K + S K + 4) 2^-52

explained(u, t) adds its fixed tree: ceil(d_u / 64) additions per lane and 6 butterfly levels,

    explained_bound(d) = contribution_bound + (ceil(d / 64) + 6) 2^-52

and the score is the W chain, the fold chain of G, the chain over f and one division: (R + L + S K + 1) 2^-52.
A product that falls into the subnormal range loses bits absolutely, not relatively: at most 2^-1075 per term, times
1 / eps = 2^52, times max|w| K -- below 2e-306 here, i.e. below 2^-52 of any value above conftest.ELEMENT_FLOOR (1e-290).
So the comparison is staged_after_fit.score_errors': relative above the floor, within the floor at or below it.  The
long-double reference's own error is the same count times 2^-64: a 2,048th of the bound.

The overlap matrix: (rows + 2) 2^-52 relative (test_gpu_overlap.py derives (rows + 2) 2^-53 for the fma chain of a slab
and the tree over the slabs), with the same floor."""
import collections
import functools
import math

import numpy as np

import catalogue_reference as cat
import exact_models as xm
import staged_after_fit as saf
from mmsbm_amd import align
from staged_params import uniform_rows
from test_align_cpu import restate_overlap, side_tables
from test_audience_cpu import by_item, restate_audience, restate_item_query
from test_gpu_audience import same_csr
from test_gpu_diverse import device_greedy, pool_tables, same_diverse, sessions
from test_gpu_serving_exact import same_answer
from test_gpu_staged_after_fit import full_rows
from test_recommend_cpu import seen_items

LD = np.longdouble
EPS = saf.EPS
FAMILIES = saf.SERVE_FAMILIES
SHAPES = [(20, 20), (7, 33), (33, 7)]
SHAPE_IDS = [f"K{k}L{l}" for k, l in SHAPES]
U, I, R, S = 120, 300, 5, 3
BIG_U, BIG_I = 40, 2100                                    # a row of 2,100 items is split across selecting waves
PLANTED = {5: 1, 17: 63, 29: 64, 41: 65, 53: 300}        # user -> training rows
W = np.arange(1.0, R + 1)
W_UP = W * 2.0 ** 200                                     # exact scalings: tiny's contributions about 1e-257, normal
W_DOWN = W * 2.0 ** -305                                  # ... and tiny's scores about 1e-311, subnormal
ALL_ROWS = 300                                            # an n that is >= every degree
UNIT = 5e-324                                             # the smallest subnormal

Case = collections.namedtuple("Case", "k l family data dims params zero_users zero_items")


def bits(a):
    return xm.bits(a)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ---- the cases ------------------------------------------------------------------------------------------------------------
def zero_rows(n_u, n_i):
    """The zeroed users and items: serve_zero_rows' items (two of them neighbours either side of a split of 2,100
    items); with the planted data user 29 (64 rows) instead of user 3."""
    zu, zi = saf.serve_zero_rows(n_u, n_i)
    return ((29, n_u - 1) if n_u == U else zu), zi


@functools.lru_cache(maxsize=None)
def training_rows(k, l, n_u, n_i):
    rng = np.random.default_rng([n_u, n_i, k, l, 5])
    base = uniform_rows(rng, 3000, n_u, n_i, R)
    if n_u != U:
        base.setflags(write=False)
        return base
    zi = zero_rows(n_u, n_i)[1]
    base = base[~np.isin(base[:, 0], list(PLANTED))]
    parts = [base, base[:40]]                              # duplicate triples: separate rows
    for u, d in PLANTED.items():
        fresh = min(d, 280)
        rows = np.stack([np.full(fresh, u), rng.integers(0, n_i, fresh), rng.integers(0, R, fresh)], 1)
        if d > 1:
            rows[0, 1] = zi[1]                             # a zeroed item in the history
        parts.append(rows)
        parts.append(rows[:d - fresh])                     # the 300-row user repeats 20 of its triples
    data = np.concatenate(parts).astype(np.int64)
    data = data[rng.permutation(len(data))]                # a user's rows lie scattered
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def case(k, l, family, n_u=U, n_i=I, n_slots=S):
    data = training_rows(k, l, n_u, n_i)
    dims = (n_u, n_i, R)
    zu, zi = zero_rows(n_u, n_i)
    return Case(k, l, family, data, dims, saf.family_slots(family, data, dims, k, l, n_slots, zero_users=zu, zero_items=zi), zu, zi)


def degrees(c):
    return np.bincount(c.data[:, 0], minlength=c.dims[0])


def row_dots(c):
    """theta_u . v_j of every (slot, training row), in float64: what exp_row_kernel clamps at eps."""
    u, i, r = c.data[:, 0], c.data[:, 1], c.data[:, 2]
    out = []
    for theta, eta, pr in c.params:
        v = np.einsum("klj,jl->jk", pr[:, :, r], eta[i])
        out.append((v * theta[u]).sum(axis=1))
    return np.stack(out)


# ---- explain: the long-double restatement and its bounds ---------------------------------------------------------------------
def contribution_bound(k, l, n_r=R, n_slots=S):
    return (n_r + 2 * l + k + n_slots * k + 4) * 2.0 ** -52


def explained_bound(k, l, d, n_r=R, n_slots=S):
    return contribution_bound(k, l, n_r, n_slots) + (math.ceil(d / 64) + 6) * 2.0 ** -52


def explain_score_bound(k, l, n_r=R, n_slots=S):
    return (n_r + l + n_slots * k + 1) * 2.0 ** -52


class LongExplain:
    """explain.hpp's formulas in np.longdouble: v, dot, c with max(dot, eps), a(u, t, j), explained and score.
    clamp=False drops the max(dot, eps) (the mutation the tests must catch)."""

    def __init__(self, data, params, w, clamp=True):
        self.data = np.asarray(data, dtype=np.int64).reshape(-1, 3)
        self.params = [tuple(np.asarray(a).astype(LD) for a in p) for p in params]
        self.w = np.asarray(w).astype(LD)
        self.W = [(p * self.w).sum(axis=2) for _, _, p in self.params]
        self.clamp = clamp
        self._c = {}

    def rows(self, user):
        return self.data[self.data[:, 0] == user][:, 1:]

    def shares(self, user):
        if user not in self._c:
            rows = self.rows(user)
            out = []
            for theta, eta, pr in self.params:
                v = np.einsum("klj,jl->jk", pr[:, :, rows[:, 1]], eta[rows[:, 0]])
                dot = v @ theta[user]
                with np.errstate(divide="ignore", invalid="ignore"):
                    out.append(theta[user] * v / (np.maximum(dot, LD(EPS)) if self.clamp else dot)[:, None])
            self._c[user] = out
        return self._c[user]

    def g(self, item):
        return [Wk @ eta[item] for Wk, (_, eta, _) in zip(self.W, self.params)]

    def pair(self, user, item):
        """dict: items, ratings, a (d_u,), explained, score, degree."""
        user, item = int(user), int(item)
        rows, c, g = self.rows(user), self.shares(user), self.g(item)
        n_slots, d = len(self.params), len(rows)
        a = sum(cs @ gs for cs, gs in zip(c, g)) / LD(n_slots * max(d, 1))
        score = sum(th[user] @ gs for (th, _, _), gs in zip(self.params, g)) / LD(n_slots)
        return {"items": rows[:, 0], "ratings": rows[:, 1], "a": a, "explained": a.sum(), "score": score, "degree": d}


def explain_request(c):
    """(users, offsets, items): every planted user, two ordinary ones, both zeroed users, user 41 twice; 2-3 targets
    each, a zeroed item among them."""
    n_u, n_i = c.dims[:2]
    users = list(PLANTED) + [7, 88, 41, n_u - 1]
    sizes = [2, 3, 2, 3, 3, 2, 2, 2, 2]
    rng = np.random.default_rng([c.k, c.l, 9])
    items = rng.integers(0, n_i, sum(sizes)).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for b in (1, 4, 5):
        items[off[b]] = c.zero_items[0]                   # a zeroed target: for a 63-row, the 300-row and an ordinary user
    return i32(users), off, items


def pairs_of(users, offsets, items):
    return [(int(u), int(items[e])) for b, u in enumerate(users) for e in range(int(offsets[b]), int(offsets[b + 1]))]


def open_explain(em, w, n_slots=S):
    em.explain_begin(w)
    for s in range(n_slots):
        em.select(s).explain_add()


def check_explain(em, c, w, floor, what, dev=None):
    """explain_query at n = 300 (every row of every user comes back) against the long-double restatement, element-wise;
    n = 1 and n = 5 against the lexsort of the n = 300 answer, bit for bit.  dev: the (U, I) scores of recommend_query
    with the same weights, where the score is to be bit for bit that (K <= L on the device), else None.
    Returns {"contribution", "explained", "score": worst error / bound, "above": entries above the floor}."""
    ref = LongExplain(c.data, c.params, w)
    users, offsets, items = explain_request(c)
    pairs = pairs_of(users, offsets, items)
    open_explain(em, w)
    full = em.explain_query(users, offsets, items, ALL_ROWS)
    small = {n: em.explain_query(users, offsets, items, n) for n in (1, 5)}
    em.explain_end()
    hi, hr, co, counts, explained, score, degree = full
    worst = collections.defaultdict(float)
    for q, (u, t) in enumerate(pairs):
        r = ref.pair(u, t)
        d = r["degree"]
        assert degree[q] == d and counts[q] == d, (what, q, degree[q], counts[q], d)
        assert (hi[q, d:] == -1).all() and (hr[q, d:] == -1).all() and np.isneginf(co[q, d:]).all(), (what, q)
        # the rows that came back are the user's rows, each as often as the user holds it
        have = collections.Counter(zip(r["items"].tolist(), r["ratings"].tolist()))
        took = collections.Counter(zip(hi[q, :d].tolist(), hr[q, :d].tolist()))
        assert have == took, (what, q)
        a_of = dict(zip(zip(r["items"].tolist(), r["ratings"].tolist()), r["a"]))       # (equal rows: equal contributions)
        want = np.array([a_of[key] for key in zip(hi[q, :d].tolist(), hr[q, :d].tolist())], dtype=LD)
        assert np.isfinite(co[q, :d]).all() and (co[q, :d] >= 0).all(), (what, q)
        assert np.isfinite(explained[q]) and explained[q] >= 0 and np.isfinite(score[q]) and score[q] >= 0, (what, q)
        for name, got, exact, bound in (("contribution", co[q, :d], want, contribution_bound(c.k, c.l)),
                                        ("explained", explained[q:q + 1], np.array([r["explained"]]), explained_bound(c.k, c.l, d)),
                                        ("score", score[q:q + 1], np.array([r["score"]]), explain_score_bound(c.k, c.l))):
            frac, small_ok = saf.score_errors(got, exact, bound, floor)
            worst[name] = max(worst[name], frac)
            assert small_ok and frac <= 1.0, (what, q, (u, t, d), name, frac)
        worst["above"] += int((want > floor).sum())
        # exact zeros: a zeroed user, a zeroed target, a history row whose item is zeroed
        if u in c.zero_users or t in c.zero_items:
            assert (bits(co[q, :d]) == 0).all() and bits(explained[q]) == 0 and bits(score[q]) == 0, (what, q, u, t)
        gone = np.isin(hi[q, :d], c.zero_items)
        assert (bits(co[q, :d][gone]) == 0).all(), (what, q)
        if dev is not None:
            assert bits(score[q]) == bits(dev[u, t]), (what, q, score[q], dev[u, t])
        # the order: contribution descending, then item id, then rating id -- of the device's OWN numbers
        order = np.lexsort((hr[q, :d], hi[q, :d], -co[q, :d]))
        assert np.array_equal(order, np.arange(d)), (what, q, "the n = 300 answer is not in its own order")
        for n, (shi, shr, sco, scounts, sexp, ssc, sdeg) in small.items():
            m = min(n, d)
            assert scounts[q] == m and sdeg[q] == d, (what, q, n)
            assert np.array_equal(shi[q, :m], hi[q, :m]) and np.array_equal(shr[q, :m], hr[q, :m]), (what, q, n)
            assert np.array_equal(bits(sco[q, :m]), bits(co[q, :m])), (what, q, n)
            assert (shi[q, m:] == -1).all() and (shr[q, m:] == -1).all() and np.isneginf(sco[q, m:]).all(), (what, q, n)
            assert bits(sexp[q]) == bits(explained[q]) and bits(ssc[q]) == bits(score[q]), (what, q, n)
    return dict(worst)


def check_identity(em, c, w, floor, what):
    """explained(u, t) against sum_k theta'_u[k] g_t[k] (long double), theta' from em's OWN fold_in of the user's rows
    at one iteration started at theta_u, per slot: within explained_bound.  Returns the worst error / bound."""
    users, offsets, items = explain_request(c)
    distinct = sorted(set(users.tolist()))
    own = np.concatenate([np.column_stack([np.full((c.data[:, 0] == u).sum(), b), c.data[c.data[:, 0] == u][:, 1:]])
                          for b, u in enumerate(distinct)])
    nxt = [em.select(s).fold_in(own, len(distinct), 1, theta0=np.ascontiguousarray(c.params[s][0][distinct]))[0] for s in range(S)]
    open_explain(em, w)
    explained = em.explain_query(users, offsets, items, 1)[4]
    em.explain_end()
    ref = LongExplain(c.data, c.params, w)
    deg = degrees(c)
    worst = 0.0
    for q, (u, t) in enumerate(pairs_of(users, offsets, items)):
        g = ref.g(t)
        want = sum(nxt[s][distinct.index(u)].astype(LD) @ g[s] for s in range(S)) / LD(S)
        frac, small_ok = saf.score_errors(explained[q:q + 1], np.array([want]), explained_bound(c.k, c.l, int(deg[u])), floor)
        worst = max(worst, frac)
        assert small_ok and frac <= 1.0, (what, q, (u, t), frac, explained[q], float(want))
    return worst


# ---- the item side -----------------------------------------------------------------------------------------------------------
def floor_acc(thr, n_slots):
    """top_pairs.hpp's gtop_floor_acc in numpy doubles: the smallest accumulator a with a / n_slots >= thr, or -inf
    when the search gives up (the kernel then divides every accumulator and compares)."""
    thr, n = np.float64(thr), np.float64(n_slots)
    with np.errstate(over="ignore"):
        a = thr * n
        for _ in range(4):
            if a / n >= thr:
                break
            a = np.nextafter(a, np.inf)
        if not (a / n >= thr) or not (a > -np.inf):
            return -np.inf
        for _ in range(6):
            below = np.nextafter(a, -np.inf)
            if not (below / n >= thr):
                return float(a)
            a = below
    return -np.inf


def same_quotient(bar, n_slots=S):
    """How many accumulators a have a / n_slots == bar (among the 12 neighbours either side of bar * n_slots)."""
    n = np.float64(n_slots)
    with np.errstate(over="ignore"):
        a = np.float64(bar) * n
        for _ in range(12):
            a = np.nextafter(a, -np.inf)
        count = 0
        for _ in range(25):
            count += int(a / n == bar)
            a = np.nextafter(a, np.inf)
    return count


WIDE_S = 16              # slots of the one case whose subnormal bars make gtop_floor_acc give up (see check_bar_paths)


def audience_bars(scores):
    """The bars of a case, from a (U, I) score matrix: the smallest positive score and its two neighbours, the median,
    the maximum and the double above it, 0.0 and the smallest subnormal; where the scores are subnormal, one more bar
    between two adjacent distinct scores."""
    pos = np.sort(scores[scores > 0])
    s0, mx = float(pos[0]), float(pos[-1])
    bars = [s0, float(np.nextafter(s0, -np.inf)), float(np.nextafter(s0, np.inf)), float(pos[len(pos) // 2]), mx,
            float(np.nextafter(mx, np.inf)), 0.0, UNIT]
    if mx < 2.0 ** -1022:
        distinct = np.unique(pos)
        gap = np.flatnonzero(np.diff(distinct) >= 2 * UNIT)
        assert len(gap), "no two adjacent subnormal scores with a double between them"
        bars.append(float(distinct[gap[len(gap) // 2]] + UNIT))
    return bars


def check_bar_paths(bars, n_slots):
    """Which path of aud_decide a bar takes is known from gtop_floor_acc alone (restated in floor_acc, asserted here).
    Take a SUBNORMAL bar of q units of 2^-1074 and S slots: bar * S = S q units exactly, and m / S is m / S rounded to
    the nearest unit (ties to even), so the accumulators that divide to q are S q - S/2 .. S q + S/2 (the ends by the
    tie rule).
      S = 3:  3 q - 1, 3 q, 3 q + 1 divide to q and 3 q - 2 to q - 1: the downward search stops after two steps at
              lo = 3 q - 1 units.  In the normal range at most two neighbouring accumulators share a quotient.  So
              with three slots never more than three accumulators share a quotient, the six-step search cannot give
              up, and EVERY finite bar takes the `acc >= lo` path (bar * 3 = -inf included: the upward search
              starts again from -DBL_MAX).
      S = 16: 16 q - 7 .. 16 q all divide to q: after six steps down the search is at 16 q - 6, still inside the
              group, gives up and answers -inf: every subnormal bar >= 1 unit takes the DIVIDE path.
    So the subnormal `tiny` scores are run twice: with three slots (`lo > -inf`) and with WIDE_S slots (divide)."""
    for bar in bars:
        lo = floor_acc(bar, n_slots)
        tiny_bar = 0 < bar and bar * n_slots < 2.0 ** -1022
        if n_slots == S:
            assert lo > -np.inf, bar
            if lo < np.inf:
                assert np.float64(lo) / n_slots >= bar and not (np.nextafter(np.float64(lo), -np.inf) / n_slots >= bar), (bar, lo)
            if tiny_bar:
                q = round(bar / UNIT)
                assert lo == (3 * q - 1) * UNIT and same_quotient(bar, n_slots) == 3, (bar, lo)
        elif tiny_bar:
            assert n_slots == WIDE_S and lo == -np.inf and same_quotient(bar, n_slots) >= 8, (bar, lo)


def open_recommend(em, w, exclude, n_slots=S):
    em.recommend_begin(w, exclude)
    for s in range(n_slots):
        em.select(s).recommend_add()


def check_item_side(em, c, w, what):
    """recommend_query_items(all items, n = U) and recommend_audience at every bar of audience_bars against em's OWN
    user side (full_rows of recommend_query): users, counts, offsets, padding and score bits.  restate_item_query
    is the (U, I) array read column by column in the item side's order, so equality with it is equality of the
    scattered array and of the order.  Returns (the (U, I) array, the bars)."""
    n_u, n_i = c.dims[:2]
    items = np.arange(n_i, dtype=np.int32)
    seen_by = by_item(seen_items(c.data, n_u), n_i)
    dev = bars = None
    for exclude in (False, True):
        open_recommend(em, w, exclude, len(c.params))
        if dev is None:
            dev = full_rows(em, c, n_u, n_i)
            assert np.isfinite(dev).all() and (dev >= 0).all()
            dev_t = np.ascontiguousarray(dev.T)
            bars = audience_bars(dev)
            check_bar_paths(bars, len(c.params))
        sb = seen_by if exclude else None
        same_answer(em.recommend_query_items(items, n_u), restate_item_query(dev_t, items, n_u, sb), f"{what} exclude={exclude} query_items")
        for bar in bars:
            want = restate_audience(dev_t, items, bar, sb)
            same_csr(em.recommend_audience(items, bar), want, f"{what} exclude={exclude} bar={bar!r}")
            sizes = em.recommend_audience(items, bar, count_only=True)
            assert sizes[1] is None and sizes[2] is None and np.array_equal(sizes[0], want[0]), (what, exclude, bar)
        em.recommend_end()
    return dev, bars


# ---- within a part of the catalogue; diverse -----------------------------------------------------------------------------------
def check_catalogue(em, c, w, what):
    """recommend_query_within and recommend_rank against the filtered, re-sorted rows of em's OWN full rows."""
    n_u, n_i = c.dims[:2]
    users = np.arange(n_u, dtype=np.int32)
    seen = seen_items(c.data, n_u)
    rng = np.random.default_rng([c.k, c.l, n_i, 3])
    zi = list(c.zero_items)
    subsets = {"the zeroed items and forty others": np.unique(np.concatenate([zi, rng.choice(n_i, 40, replace=False)])),
               "one item": [n_i // 2], "one zeroed item": zi[:1], "every item": np.arange(n_i), "none given": None}
    lists = [np.unique(np.concatenate([rng.choice(n_i, 12), zi[:2]])) for _ in users]
    off, flat = cat.csr(lists)
    dev = None
    for exclude in (False, True):
        open_recommend(em, w, exclude)
        if dev is None:
            dev = full_rows(em, c, n_u, n_i)
            positive = [np.flatnonzero(dev[u] > 0) for u in users]       # a row's ENTIRE positive part
            extra = cat.csr(positive)
        sn = seen if exclude else None
        for name, cand in subsets.items():
            size = n_i if cand is None else len(cand)
            for n in sorted({1, min(10, size), min(size, saf.MAX_QUERY)}):
                got = em.recommend_query_within(users, n, None if cand is None else i32(cand))
                same_answer(got, cat.within_top_n(dev, users, n, cand, sn), f"{what} exclude={exclude} {name} n={n}")
        for n in (1, 10):                                  # only the +0.0 tie group is left: ascending item id
            want = cat.within_top_n(dev, users, n, None, sn, positive)
            same_answer(em.recommend_query_within(users, n, None, extra), want, f"{what} exclude={exclude} positive part excluded n={n}")
            valid = np.arange(n)[None, :] < want[2][:, None]
            assert (bits(want[1][valid]) == 0).all() and (n == 1 or (want[2] >= 2).any()), what
            assert all((np.diff(want[0][b, :want[2][b]]) > 0).all() for b in range(n_u)), what
        for n in (1, 5, 20):
            same_answer(em.recommend_rank(users, off, flat, n), cat.rank_lists(dev, users, off, flat, n, sn), f"{what} exclude={exclude} rank n={n}")
        em.recommend_end()
    return dev


def diverse_users(c):
    n_u = c.dims[0]
    return i32([c.zero_users[0], 7, 53, 88] if n_u == U else [c.zero_users[0], 7, 20, n_u - 2])


def check_diverse(em, c, w, what, pools=(10, 300), lambdas=(0.0, 1.0, 1e200)):
    """recommend_diverse against diverse_reference.greedy fed em's OWN pool (recommend_query_within) and em's OWN
    similar_pairs distances: ids, score bits, m at the pick.  The zeroed items are identical rows: D = +0.0.  Returns
    in how many (row, n, pool, trade_off > 0) the list differs from the plain one (some, unless every distance is +0.0)."""
    users = diverse_users(c)
    zi = list(c.zero_items)
    with sessions(em, w, True, range(S)):
        twins = em.similar_pairs(np.repeat(zi, len(zi)), np.tile(zi, len(zi)))
        assert (bits(twins) == 0).all(), (what, twins)
        tables = pool_tables(em, users, max(pools))
        for ids, d in tables:
            assert np.isfinite(d).all() and (d >= 0).all(), what
        moved = 0
        for pool in pools:
            for n in sorted({1, 10, pool}):
                plain = None
                for lam in lambdas:
                    got = em.recommend_diverse(users, n, pool, lam)
                    same_diverse(got, device_greedy(em, users, n, pool, lam, tables), f"{what} n={n} pool={pool} trade_off={lam}")
                    plain = got if lam == 0.0 else plain
                    moved += int((got[0] != plain[0]).any(axis=1).sum())
        spread = max(float(d.max()) for _, d in tables if d.size)
        # (tiny: every distance underflows to +0.0, every v ties, and the ties go to the earlier place: the plain order)
        assert (moved > 0) == (spread > 0), (what, moved, spread)
    return moved


# ---- overlap ---------------------------------------------------------------------------------------------------------------------
OVERLAP_FAMILIES = ("late", "tiny", "dead", "sub")
OVERLAP_SLAB = 2048                                      # overlap.hpp: kOvlSlab
OVERLAP_ROWS = (OVERLAP_SLAB - 1, OVERLAP_SLAB, OVERLAP_SLAB + 1)
OVERLAP_KL = (7, 33)                                     # S G = 21 columns (users), 99 (items: across two 64-column tiles)


@functools.lru_cache(maxsize=None)
def overlap_case(family, rows):
    k, l = OVERLAP_KL
    dims = (rows, rows, R)
    data = uniform_rows(np.random.default_rng([rows, k, l]), 4 * rows, *dims)
    data.setflags(write=False)
    return Case(k, l, family, data, dims, saf.family_slots(family, data, dims, k, l, S), (), ())


def check_overlap(em, c, side, floor, what):
    """overlap_query element-wise against the long-double Gram matrix within (rows + 2) 2^-52; zero rows and columns
    of dead groups and the symmetry by their bits; align_side finite, similarity 0.0 for a dead group.  Returns the
    worst error / bound."""
    rows = c.dims[0]
    G = c.k if side == "users" else c.l
    em.overlap_begin(side)
    try:
        for s in range(S):
            em.select(s).overlap_add()
        O = em.overlap_query()
    finally:
        em.overlap_end()
    want = restate_overlap(c.params, side)
    assert O.shape == want.shape == (S * G, S * G) and np.isfinite(O).all() and (O >= 0).all(), what
    frac, small_ok = saf.score_errors(O, want, (rows + 2) * 2.0 ** -52, floor)
    assert small_ok and frac <= 1.0, (what, frac)
    dead = (np.concatenate(side_tables(c.params, side), axis=1) == 0).all(axis=0)
    assert (bits(O[dead]) == 0).all() and (bits(O[:, dead]) == 0).all(), what
    assert np.array_equal(bits(O), bits(np.ascontiguousarray(O.T))), what
    groups, similarity, agreement = align.align_side(O, G, rows, 0)
    assert np.isfinite(similarity).all() and np.isfinite(agreement).all(), what
    assert all(sorted(g.tolist()) == list(range(G)) for g in groups), what
    if c.family == "dead":
        assert dead[:G].any() and not dead[:G].all(), what
        assert (similarity[1:, dead[:G]] == 0.0).all(), (what, similarity)
    return frac
