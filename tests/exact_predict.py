"""Models on which the predict / score session carries no rounding at all, the exact reference built on them and the
checker both suites drive (no GPU, no library): the inputs of test_exact_predict_cpu.py and test_gpu_exact_predict.py.

Every entry of theta and eta is a multiple of 1/8, every entry of p a multiple of 1/16 and every rating weight a small
integer.  Then P[m, r] = sum_kl theta[u, k] eta[i, l] p[k, l, r] is a multiple of 2^-10 and at most 1, the entries
sum_l p[k, l, r] eta[i, l] of the (item, rating) table multiples of 2^-7, and every partial sum of every fma chain,
lane tree and matrix-core accumulation is exact in fp64 whatever its order; so are pond = sum_r P[m, r] w_r,
|pond - real| and their sums over a few thousand rows.  The reference is therefore INTEGER arithmetic:

    N_s[m, r] = sum_kl (8 theta_s)[u, k] (8 eta_s)[i, l] (16 p_s)[k, l, r]        (np.int64)
    P_s = N_s / 1024,    mean = (sum_s N_s) / 1024 / S                             (an exact numerator, ONE division)

and the six sums of a distribution with numerators N over the denominator D come from N and D alone: the first maximum
(np.argmax), |argmax - real|, the rows whose numerators are all zero, pond = (N . w) / D as a rational number rounded
half to even (np.round), and sum |N . w - real D| / D.  On the device every one of them has this one correct value,
bit for bit.  With S not a power of two the mean is rounded once per entry: its argmax is still exact (equal
numerators give equal quotients, numerators one unit apart different ones), sums [0]..[3] with it; [4] can differ from
the host formula only on a row whose exact pond is half-way, [5] is held at the project's 1e-12.

Ties and half-way ponds are PLANTED (random dyadic rows tie almost never): two of every three cells (k, l) of p hold
a row of `planted(R)` -- equal maxima next to each other, two apart, three in a row, a flat row, (1/2, 1/2) on
ratings r, r + 1 for even and odd r, (1/2, 0, 1/2), an all-zero row, a single peak -- the SAME row in every slot, so
that the mean keeps it; the third cell holds a random dyadic row per slot, so that the slots differ.  With one-hot theta
and eta a test row's distribution is one cell, P[m, :] = p[k, l, :].  Where S is not a power of two the last slot holds
a random row in the half-way cells, which leaves the mean few half-way ponds (the cap on [4] stays small) and the
other slots all of theirs.  Users u = 5 (mod 11) have an all-zero theta row: their distributions are all zero.
"""
import functools

import numpy as np

from exact_models import bits, dyadic_simplex, weights_of

TH_DEN, P_DEN = 8, 16
SCALE = TH_DEN * TH_DEN * P_DEN                      # 1024: P = N / SCALE
FAMILIES = ("onehot_ties", "onehot_half", "mixed_planted", "constant")
WEIGHT_KINDS = ("index", "stars", "signed")          # arange(R): the reference's rating indices
ZERO_USER_EVERY, ZERO_USER_AT = 11, 5


# ---- the planted rows ---------------------------------------------------------------------------------------------------
def _row(R, at):
    row = np.zeros(R, dtype=np.int64)
    for r, v in at.items():
        row[r] = v
    return row


def planted(R, kind="ties"):
    """(n, R) numerators over 16: the planted rows in the order the cells take them, the categories in turn so that a
    handful of cells already holds one of each."""
    adj = [_row(R, {r: 5, r + 1: 5, (r + 2 if r + 2 < R else r - 1): 2} if R > 2 else {r: 5, r + 1: 5}) for r in range(R - 1)]
    half = [_row(R, {r: 8, r + 1: 8}) for r in range(R - 1)]
    apart = [_row(R, {r: 5, r + 1: 3, r + 2: 5}) for r in range(R - 2)]
    triple = [_row(R, {r: 4, r + 1: 4, r + 2: 4}) for r in range(R - 2)]
    half_apart = [_row(R, {r: 8, r + 2: 8}) for r in range(R - 2)]
    misc = [np.zeros(R, dtype=np.int64), np.ones(R, dtype=np.int64), _row(R, {R - 1: 16}), _row(R, {0: 9, R - 1: 7})]
    cats = [adj, half[0::2], half[1::2], misc, apart, triple, half_apart]
    if kind == "half":
        cats = [cats[1], cats[2], cats[6], cats[0], cats[3], cats[4], cats[5]]
    return np.array([c[j] for j in range(max(len(c) for c in cats)) for c in cats if j < len(c)])


def one_hot_groups(n, d):
    """Group of every one-hot user (item): all d groups in turn where there are enough rows; else spread over them,
    every third one counted down from the LAST group (rows of more than 1,024 groups: the columns of the tail loop)."""
    ids = np.arange(n)
    if n >= d:
        return ids % d
    return np.where(ids % 3 == 1, d - 1 - ids // 3, (ids * (d // n + 1)) % d)


def model(family, rng, U, I, K, L, R, S, w):
    """S parameter sets (theta (U, K), eta (I, L), p (K, L, R)) of `family`, all entries exact dyadic fractions.
    w: the session's integer rating weights (they decide which planted rows have a half-way pond)."""
    assert family in FAMILIES, family
    kl = np.arange(K * L)
    is_planted = kl % 3 != 2
    slot_of = 2 * (kl // 3) + kl % 3                         # position of a planted cell among the planted ones
    pat = planted(R, "half" if family == "onehot_half" else "ties")
    pat_half = half_way(pat, P_DEN, w)
    which = slot_of % len(pat)
    hot_u, hot_i = np.eye(K)[one_hot_groups(U, K)], np.eye(L)[one_hot_groups(I, L)]
    zero_u = np.arange(U) % ZERO_USER_EVERY == ZERO_USER_AT
    params = []
    for s in range(S):
        if family == "constant":
            p = np.full((K, L, R), float(8 >> s) / P_DEN)     # every cell the same flat row: argmax 0 everywhere
        else:
            p = dyadic_simplex(rng, (K * L, R), P_DEN)
            keep = is_planted.copy()
            if S & (S - 1) and s == S - 1:
                keep &= ~pat_half[which]                      # (the mean of these slots keeps few half-way ponds)
            p[keep] = pat[which[keep]] / float(P_DEN)
            if S & (S - 1) and s == S - 1:                    # ... nor a free cell whose slots happen to add up to one
                for _ in range(50):
                    total = sum(_ints(q.reshape(K * L, R), P_DEN) for _, _, q in params) + _ints(p, P_DEN)
                    again = ~keep & half_way(total, P_DEN * S, w)
                    if not again.any():
                        break
                    p[again] = dyadic_simplex(rng, (int(again.sum()), R), P_DEN)
            p = p.reshape(K, L, R)
        if family in ("onehot_ties", "onehot_half"):
            theta, eta = hot_u.copy(), hot_i.copy()
        else:
            theta, eta = dyadic_simplex(rng, (U, K), TH_DEN), dyadic_simplex(rng, (I, L), TH_DEN)
            if family == "mixed_planted":                     # every second user and item one-hot: their pairs are cells
                theta[0::2], eta[0::2] = hot_u[0::2], hot_i[0::2]
        theta[zero_u] = 0.0
        params.append((theta, eta, p))
    return params


def weights(kind, R):
    if kind == "index" or R == 1:
        return np.arange(R, dtype=np.float64)
    return weights_of(kind, R)


# ---- the exact reference --------------------------------------------------------------------------------------------------
def _ints(a, den):
    n = np.rint(np.asarray(a) * den).astype(np.int64)
    assert np.array_equal(n / float(den), a), "not a multiple of 1 / %d" % den
    return n


def numerators(param, u, i):
    """N[m, r] = sum_kl (8 theta)[u_m, k] (8 eta)[i_m, l] (16 p)[k, l, r], int64."""
    theta, eta, p = param
    b = np.einsum("ml,klr->mkr", _ints(eta, TH_DEN)[i], _ints(p, P_DEN))
    return np.einsum("mk,mkr->mr", _ints(theta, TH_DEN)[u], b)


def half_way(num, den, w):
    """Rows whose exact pond = (num . w) / den is an integer plus one half."""
    pn = num @ _ints(w, 1)
    return ((2 * pn) % den == 0) & (((2 * pn) // den) % 2 == 1)


def six_sums(num, den, real, w, argmax="first", half="even", border="le", zeros="drop"):
    """The six sums of the distribution num / den from integers.  The keywords select the WRONG rules the tests must
    tell from the right ones: argmax="last", half="away", border="lt" (|argmax - real| < 1), zeros="keep"."""
    num, real = np.asarray(num, dtype=np.int64), np.asarray(real, dtype=np.int64)
    R = num.shape[1]
    keep = (num.sum(axis=1) != 0) if zeros == "drop" else np.ones(len(num), dtype=bool)
    best = np.argmax(num, axis=1) if argmax == "first" else R - 1 - np.argmax(num[:, ::-1], axis=1)
    d = np.abs(best - real)
    pn = num @ _ints(w, 1)
    up = (2 * pn + den) // (2 * den)                          # floor(pond + 1/2)
    hw = half_way(num, den, w)
    down = hw & ((up % 2 == 1) if half == "even" else (pn < 0))
    q = np.where(down, up - 1, up)
    s5 = int(np.abs(pn - real * den)[keep].sum())
    assert s5 < 2 ** 53
    return np.array([keep.sum(), (d == 0)[keep].sum(), (d <= 1 if border == "le" else d < 1)[keep].sum(), d[keep].sum(),
                     (real == q)[keep].sum(), s5 / float(den)], dtype=np.float64)


def exact_session(params, rows, w, **rules):
    """The session's exact answers: per slot P_s, the mean, the six sums of every slot and of the mean, and for every
    row whether its exact pond is half-way (per slot, and for the mean).  `rules`: six_sums' wrong rules."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    S = len(params)
    nums = [numerators(p, rows[:, 0], rows[:, 1]) for p in params]
    total = np.sum(nums, axis=0)
    return {"nums": nums, "total": total,
            "P": [n / float(SCALE) for n in nums],
            "mean": total / float(SCALE) / float(S),
            "slot_sums": [six_sums(n, SCALE, rows[:, 2], w, **rules) for n in nums],
            "mean_sums": six_sums(total, SCALE * S, rows[:, 2], w, **rules),
            "half": [half_way(n, SCALE, w) for n in nums],
            "mean_half": half_way(total, SCALE * S, w)}


# ---- the test rows -------------------------------------------------------------------------------------------------------
def rows(rng, params, U, I, R, max_pairs=720):
    """Test rows (user, item, real), shuffled.  Every chosen (user, item) pair comes with real = argmax - 2, - 1, + 1,
    + 2 of slot 0's exact distribution and every LATER rating that ties with its maximum; one pair in two, drawn at
    random, also with the argmax itself and one in three without argmax + 2 (so that a tie row meets its second
    maximum more often than its first, and the two neighbours of a half-way pond do not come equally often)."""
    if U * I <= max_pairs:
        pairs = np.stack(np.meshgrid(np.arange(U), np.arange(I), indexing="ij"), -1).reshape(-1, 2)
    else:
        flat = rng.choice(U * I, max_pairs, replace=False)
        pairs = np.stack([flat // I, flat % I], 1)
    num = numerators(params[0], pairs[:, 0], pairs[:, 1])
    coin = rng.integers(0, 6, len(pairs))
    out = []
    for j, (u, i) in enumerate(pairs.tolist()):
        best = int(np.argmax(num[j]))
        reals = {best - 2, best - 1, best + 1, best + 2} | set(np.flatnonzero(num[j] == num[j, best])[1:].tolist())
        if coin[j] % 2 == 0:
            reals.add(best)
        if coin[j] % 3 == 0:
            reals.discard(best + 2)
        out.extend((u, i, r) for r in sorted(reals) if 0 <= r < R)
    out = np.array(out, dtype=np.int64).reshape(-1, 3)
    return out[rng.permutation(len(out))]


def training_data(U, I, R):
    """A context needs triples; these name the last user, item and rating (the host class sizes itself from them)."""
    n = np.arange(max(U, I, R))
    return np.stack([n % U, n % I, n % R], 1).astype(np.int64)


# ---- what makes a case bite --------------------------------------------------------------------------------------------
def conditions(num, den, real, w):
    """Counts over the rows that are kept (not all zero): rows with tied maxima, those whose real is a later tied
    rating, ponds of even + 1/2 and odd + 1/2, |argmax - real| = 0, 1, 2, and the all-zero rows."""
    num, real = np.asarray(num, dtype=np.int64), np.asarray(real, dtype=np.int64)
    keep = num.sum(axis=1) != 0
    top = num.max(axis=1)
    tied = keep & ((num == top[:, None]).sum(axis=1) > 1)
    best = np.argmax(num, axis=1)
    later = tied & (real > best) & (num[np.arange(len(num)), real] == top)
    pn = num @ _ints(w, 1)
    hw = keep & half_way(num, den, w)
    floor = (2 * pn - den) // (2 * den)                       # of a half-way pond
    d = np.abs(best - real)
    return {"tied": int(tied.sum()), "later": int(later.sum()),
            "half_even": int((hw & (floor % 2 == 0)).sum()), "half_odd": int((hw & (floor % 2 == 1)).sum()),
            "d0": int((keep & (d == 0)).sum()), "d1": int((keep & (d == 1)).sum()), "d2": int((keep & (d == 2)).sum()),
            "zero": int((~keep).sum()), "rows": len(num)}


def required(family, R):
    """The least count of every condition for a case of `family` with R ratings.  What the arithmetic rules out is
    left out, nothing else: R = 1 has one rating (no tie, no distance), R = 2 no odd r below R - 1 and no distance 2,
    and in "constant" every kept row has the same pond c sum(w) / 16 times a dyadic factor -- two such ponds
    e + 1/2 and o + 1/2 would have the odd ratio (2e + 1) / (2o + 1) dyadic, so at most one parity occurs."""
    need = {"zero": 10, "d0": 10}
    if R >= 2:
        need.update({"tied": 50, "later": 20, "d1": 10})
        if family != "constant":
            need["half_even"] = 20
    if R >= 3:
        need["d2"] = 10
        if family != "constant":
            need["half_odd"] = 20
    return need


# ---- the cases both test files run -------------------------------------------------------------------------------------
# name -> (family, weight kind, (U, I, K, L, R, S), swap_sides).  K and L are the caller's; with swap_sides = 0 they are
# the internal ones too, and group_code (shapes.hpp) goes by the padded internal K: <= 16, 32, 64, 128, 256, 512, more.
FORM_KS = (16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1040)
GROUPS_OF_K = {16: (4, 4), 17: (8, 4), 32: (8, 4), 33: (16, 4), 64: (16, 4), 65: (32, 4), 128: (32, 4), 129: (64, 4),
               256: (64, 4), 257: (64, 8), 512: (64, 8), 513: (64, 16), 1040: (64, 16)}    # K -> (G, VEC)
RATING_RS = (1, 2, 3, 4, 5, 7, 8, 9)
CASES = {}
for _n, _k in enumerate(FORM_KS):
    _fam = FAMILIES[_n % 3] if _k < 64 else ("mixed_planted" if _n % 2 else "onehot_ties")
    CASES[f"K{_k}"] = (_fam, WEIGHT_KINDS[_n % 3], (40 if _k > 1024 else 66, 10, _k, 3, 5, 1 + _n % 2), 0)
for _n, (_r, _kind) in enumerate(zip(RATING_RS, ("index", "index", "stars", "signed", "signed", "index", "stars", "signed"))):
    CASES[f"R{_r}"] = (FAMILIES[_n % 3], _kind, (60, 12, 6, 5, _r, (2, 3, 1, 4)[_n % 4]), 0)
CASES.update({
    "constant": ("constant", "stars", (44, 12, 6, 5, 5, 2), 0),
    "constantS3": ("constant", "index", (44, 12, 5, 7, 4, 3), 0),
    "constantR2": ("constant", "index", (44, 12, 6, 5, 2, 2), 0),          # slot 0: the flat row (1/2, 1/2), pond 1/2
    "mfma": ("mixed_planted", "index", (60, 30, 40, 40, 4, 2), 0),        # 40 x 40 tile: the one-block matrix-core form
    "halfS3": ("onehot_half", "signed", (60, 20, 9, 7, 6, 3), 0),
    "swapped": ("mixed_planted", "stars", (50, 60, 6, 9, 5, 3), 1),
    "swappedK70": ("onehot_ties", "signed", (40, 30, 5, 70, 7, 2), 1),    # internal K = 70
    "perrow": ("onehot_half", "index", (60, 3, 6, 3, 5, 2), 0),           # I = 3: any row count takes the table form
    "rows64": ("onehot_half", "stars", (48, 3, 130, 3, 5, 2), 0),         # 64 lanes per row, 4 rows per workgroup
    "I1": ("onehot_ties", "index", (300, 1, 7, 1, 4, 2), 0),
})
ROW_COUNTS = {"perrow": (1, 63, 64, 65, 193, 255, 256, 257, 513), "rows64": (1, 3, 4, 5, 13)}


@functools.lru_cache(maxsize=None)
def make_case(name):
    """One case's inputs and exact answers.  Cached and shared: treat every array as read-only."""
    family, kind, shape, swap = CASES[name]
    U, I, K, L, R, S = shape
    rng = np.random.default_rng([FAMILIES.index(family), WEIGHT_KINDS.index(kind), *shape])
    w = weights(kind, R)
    params = model(family, rng, U, I, K, L, R, S, w)
    test = rows(rng, params, U, I, R)
    return {"name": name, "family": family, "shape": shape, "swap": swap, "params": params, "w": w, "rows": test,
            "data": training_data(U, I, R), "ref": exact_session(params, test, w)}


def prefix(case, n):
    """The case cut to its first n rows (the rows are shuffled), with the exact answers of those rows."""
    test = case["rows"][:n]
    assert len(test) == n, (case["name"], n, len(case["rows"]))
    return dict(case, rows=test, ref=exact_session(case["params"], test, case["w"]))


# ---- the checker both suites drive ---------------------------------------------------------------------------------------
def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError(f"{what}: {len(bad)} entries differ, first at {bad[0].tolist()}: "
                             f"device {got[tuple(bad[0])]!r}, exact {want[tuple(bad[0])]!r}")


def same_sums(got, want, what, upto=6):
    assert np.array_equal(np.asarray(got)[:upto], np.asarray(want)[:upto]), (what, list(got), list(want))


def host_sums(mean, real, w):
    """[4] and [5] by the host formulas (MMSBM._compute_stats) on the matrix the device returned."""
    keep = mean.sum(axis=1) != 0
    pond = (mean @ w)[keep]
    return float((np.round(pond) == real[keep]).sum()), float(np.abs(pond - real[keep]).sum())


def check_mean(mean, raw, case, what):
    """The finished session: the mean bit for bit; its six sums exact where S is a power of two, else [0]..[3] exact,
    [5] within 1e-12 of the host formula on the device's own mean and [4] off it by at most the rows whose exact pond
    is half-way."""
    ref, S = case["ref"], len(case["params"])
    same_bits(mean, ref["mean"], f"{what}: mean")
    if S & (S - 1) == 0:
        same_sums(raw, ref["mean_sums"], f"{what}: sums of the mean")
        return
    same_sums(raw, ref["mean_sums"], f"{what}: sums [0]..[3] of the mean", upto=4)
    h4, h5 = host_sums(np.asarray(mean), case["rows"][:, 2], case["w"])
    assert abs(raw[5] - h5) <= 1e-12 * h5, (what, raw[5], h5)
    assert abs(raw[4] - h4) <= int(ref["mean_half"].sum()), (what, raw[4], h4, int(ref["mean_half"].sum()))


def check_session(em, case, what="", slots=None):
    """Open a session over the case's rows on `em` (whose slots hold the case's parameter sets), add `slots` (all, in
    order) and finish: every slot's six sums and the mean against the exact reference.  Returns (mean, raw)."""
    ref = case["ref"]
    order = list(range(len(case["params"]))) if slots is None else list(slots)
    assert order == list(range(len(case["params"]))), "the reference's mean is over all slots in order"
    em.predict_begin(case["rows"], case["w"])
    for s in order:
        same_sums(em.select(s).predict_add(), ref["slot_sums"][s], f"{what} {case['name']}: sums of slot {s}")
    mean, raw = em.predict_finish()
    check_mean(mean, raw, case, f"{what} {case['name']}")
    return mean, raw


def check_prod_dist(em, case, what=""):
    for s, want in enumerate(case["ref"]["P"]):
        same_bits(em.select(s).prod_dist(case["rows"]), want, f"{what} {case['name']}: prod_dist of slot {s}")
