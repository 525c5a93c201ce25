"""The leave-one-out reliability of the training rows, restated in plain numpy (TEST INFRASTRUCTURE ONLY): what
``MMSBM.rating_reliability`` / ``spurious_ratings`` / ``misfit_users`` / ``misfit_items`` and ``mmsbm_hip_loo_*``
compute, written down the way ``compute_omegas`` writes the E-step, with ``np.add.at`` for the users' and items' sums.

Per slot, for training row j = (u, i, r):
  v_j[k] = sum_l p[k,l,r] eta[i,l]      w_j[l] = sum_k p[k,l,r] theta[u,k]      fit_j = sum_k theta[u,k] v_j[k]
  c_j[k] = (theta[u,k] v_j[k]) / max(fit_j, eps)        e_j[l] = (eta[i,l] w_j[l]) / max(fit_j, eps)
  C_u = sum_{j in u} c_j                                 E_i = sum_{j in i} e_j
  theta-[k] = max(C_u[k] - c_j[k], 0) / (d_u - 1), or the mean theta row over all users where d_u = 1; eta- likewise
  rel_j = sum_kl theta-[k] p[k,l,r] eta-[l]
Over the slots: reliability = mean rel, fitted = mean fit, surprise = -log(max(reliability, eps)); a user's (item's)
surprise is the mean of its rows' surprises.

Also the training table the reliability tests share (``training_rows``) and their models (``model``)."""
import numpy as np

EPS = np.finfo(np.float64).eps


def slot_terms(data, theta, eta, pr):
    """{v, w, fit, c, e, C, E} of one slot: the E-step shares of every row and the M-step numerators."""
    u, i, r = data[:, 0], data[:, 1], data[:, 2]
    pj = np.moveaxis(pr, 2, 0)[r]                                   # (N, K, L)
    v = np.einsum("nkl,nl->nk", pj, eta[i])
    w = np.einsum("nkl,nk->nl", pj, theta[u])
    fit = (theta[u] * v).sum(axis=1)
    inv = 1.0 / np.maximum(fit, EPS)
    c, e = (theta[u] * v) * inv[:, None], (eta[i] * w) * inv[:, None]
    C, E = np.zeros_like(theta), np.zeros_like(eta)
    np.add.at(C, u, c)
    np.add.at(E, i, e)
    return {"v": v, "w": w, "fit": fit, "c": c, "e": e, "C": C, "E": E, "pj": pj}


def slot_reliability(data, theta, eta, pr):
    """{rel, fit, theta_minus, eta_minus} of one slot."""
    u, i = data[:, 0], data[:, 1]
    t = slot_terms(data, theta, eta, pr)
    du, di = np.bincount(u, minlength=len(theta)), np.bincount(i, minlength=len(eta))
    tbar, ebar = theta.sum(axis=0) / len(theta), eta.sum(axis=0) / len(eta)   # inform_mean_theta's definition
    tm = np.maximum(t["C"][u] - t["c"], 0.0) / np.maximum(du[u] - 1, 1)[:, None]
    em = np.maximum(t["E"][i] - t["e"], 0.0) / np.maximum(di[i] - 1, 1)[:, None]
    tm = np.where((du[u] > 1)[:, None], tm, tbar[None, :])
    em = np.where((di[i] > 1)[:, None], em, ebar[None, :])
    rel = np.einsum("nk,nkl,nl->n", tm, t["pj"], em)
    return {"rel": rel, "fit": t["fit"], "theta_minus": tm, "eta_minus": em, "C": t["C"], "E": t["E"]}


class Restatement:
    """Every number of a loo session over ``data`` with the slots ``params`` = [(theta, eta, pr), ...] added."""

    def __init__(self, data, params):
        self.data = np.asarray(data, dtype=np.int64)
        self.slots = [slot_reliability(self.data, *p) for p in params]
        S = len(params)
        rel_sum, fit_sum = np.zeros(len(self.data)), np.zeros(len(self.data))
        for s in self.slots:
            rel_sum, fit_sum = rel_sum + s["rel"], fit_sum + s["fit"]
        self.reliability, self.fitted = rel_sum / S, fit_sum / S
        self.surprise = -np.log(np.maximum(self.reliability, EPS))
        self.fitted_surprise = -np.log(np.maximum(self.fitted, EPS))
        U, I = len(params[0][0]), len(params[0][1])
        self.d_user = np.bincount(self.data[:, 0], minlength=U)
        self.d_item = np.bincount(self.data[:, 1], minlength=I)

    def rows(self, rows=None):
        """(fitted, reliability) at the positions ``rows`` (None: all)."""
        at = slice(None) if rows is None else np.asarray(rows, dtype=np.int64)
        return self.fitted[at].copy(), self.reliability[at].copy()

    def _side(self, column, degree):
        out = []
        for x in (self.surprise, self.fitted_surprise):
            tot = np.zeros(len(degree))
            np.add.at(tot, self.data[:, column], x)
            with np.errstate(invalid="ignore", divide="ignore"):
                out.append(tot / degree)                               # (no rows: NaN)
        return out

    def sides(self):
        """(user surprise, user fitted_surprise, item surprise, item fitted_surprise)."""
        return tuple(self._side(0, self.d_user) + self._side(1, self.d_item))

    def lowest(self, m, user_flags=None, item_flags=None):
        return lowest_of(self.data, self.reliability, m, user_flags, item_flags)


def lowest_of(data, reliability, m, user_flags=None, item_flags=None):
    """(rows (m,) padded with -1, reliability (m,) padded with +inf, count): a stable sort of the eligible rows."""
    ok = np.ones(len(data), dtype=bool)
    if user_flags is not None:
        ok &= np.asarray(user_flags, dtype=bool)[data[:, 0]]
    if item_flags is not None:
        ok &= np.asarray(item_flags, dtype=bool)[data[:, 1]]
    pos = np.flatnonzero(ok)
    pos = pos[np.argsort(reliability[pos], kind="stable")][:m]
    rows, rel = np.full(m, -1, dtype=np.int64), np.full(m, np.inf)
    rows[:len(pos)], rel[:len(pos)] = pos, reliability[pos]
    return rows, rel, len(pos)


# ---- the table and the models the reliability tests share ------------------------------------------------------------------
U, I, R = 300, 1500, 5
PLANTED = {0: 1, 1: 2, 2: 63, 3: 64, 4: 65}        # user -> rows
HEAVY, HEAVY_ROWS, HEAVY_DUPLICATES = 5, 1300, 100
HEAVY_ITEM, HEAVY_ITEM_ROWS = 0, 900
LONE_ITEM, LONE_ITEM_2 = I - 1, I - 2              # one row each; LONE_ITEM's row is the only row of user 0
ZERO_RATING = 2                                    # the rating whose tile the "zero" model empties
SHAPES = [(1, 4), (3, 5), (5, 3), (20, 20), (70, 3), (4, 1)]
KINDS = ("soft", "sharp", "onehot", "zero")
_CACHE = {}


def training_rows():
    """About 8,700 rows in scattered order: planted users of 1, 2, 63, 64 and 65 rows, one user of 1,300 rows of which
    100 are duplicated triples, one item of 900 rows, two items of one row, and one row whose user and item both hold
    nothing else."""
    if "data" not in _CACHE:
        rng = np.random.default_rng(23)
        free = np.arange(HEAVY + 1, U)
        mid = lambda n: rng.integers(1, I - 2, n)                                   # noqa: E731  (ordinary items)
        parts = [np.stack([rng.choice(free, 6000), mid(6000), rng.integers(0, R, 6000)], 1),
                 np.stack([free, 1 + free % (I - 3), free % R], 1),                 # every user holds a row
                 np.stack([rng.choice(free, HEAVY_ITEM_ROWS), np.full(HEAVY_ITEM_ROWS, HEAVY_ITEM),
                           rng.integers(0, R, HEAVY_ITEM_ROWS)], 1),
                 np.array([[free[7], LONE_ITEM_2, 3]])]
        for u, d in PLANTED.items():
            items = mid(d)
            if d == 1:
                items[0] = LONE_ITEM
            parts.append(np.stack([np.full(d, u), items, rng.integers(0, R, d)], 1))
        first = HEAVY_ROWS - HEAVY_DUPLICATES
        heavy = np.stack([np.full(first, HEAVY), mid(first), rng.integers(0, R, first)], 1)
        parts += [heavy, heavy[:HEAVY_DUPLICATES]]                                  # duplicate triples: separate rows
        data = np.concatenate(parts)
        data = data[rng.permutation(len(data))]                                     # a segment's rows lie scattered
        du, di = np.bincount(data[:, 0], minlength=U), np.bincount(data[:, 1], minlength=I)
        assert all(du[u] == d for u, d in PLANTED.items()) and du[HEAVY] == HEAVY_ROWS and du.min() >= 1
        assert di[HEAVY_ITEM] == HEAVY_ITEM_ROWS and di[LONE_ITEM] == 1 and di[LONE_ITEM_2] == 1
        lone = data[data[:, 1] == LONE_ITEM][0]
        assert du[lone[0]] == 1
        _CACHE["data"] = data
    return _CACHE["data"]


def _simplex(x):
    return x / x.sum(axis=-1, keepdims=True)


def model(K, L, S, kind="soft"):
    """S parameter sets of ``kind``: "soft" random rows on the simplex; "sharp" the same with every row raised to the
    8th power and renormalised (late-stage); "onehot" soft with exactly one-hot theta rows; "zero" soft with the tile of
    rating ZERO_RATING emptied (p renormalised over the other ratings): every row of that rating has fit = 0."""
    key = (K, L, S, kind)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * K + 10 * L + S)
        params = []
        for s in range(S):
            th, eta, pr = _simplex(rng.random((U, K))), _simplex(rng.random((I, L))), _simplex(rng.random((K, L, R)))
            if kind == "sharp":
                th, eta, pr = _simplex(th ** 8), _simplex(eta ** 8), _simplex(pr ** 8)
            elif kind == "onehot":
                th = np.eye(K)[(np.arange(U) + s) % K]
            elif kind == "zero":
                pr[:, :, ZERO_RATING] = 0.0
                pr = _simplex(pr)
            params.append((np.ascontiguousarray(th), np.ascontiguousarray(eta), np.ascontiguousarray(pr)))
        _CACHE[key] = params
    return _CACHE[key]


def restatement(K, L, S, kind="soft"):
    key = ("ref", K, L, S, kind)
    if key not in _CACHE:
        _CACHE[key] = Restatement(training_rows(), model(K, L, S, kind))
    return _CACHE[key]
