"""The numpy restatement of mmsbm_hip_explain_* (mmsbm_amd/csrc/explain.hpp), written as the formulas of the header, in
float64 with plain loops over slots, rows and k:

    v_j[k]     = sum_l p[k, l, r_j] eta[i_j, l]
    c_j[k]     = theta_u[k] v_j[k] / max(theta_u . v_j, eps)
    g_t[k]     = sum_l W[k, l] eta[t, l],  W[k, l] = sum_r w_r p[k, l, r]
    a(u, t, j) = (1 / (S d_u)) sum_s sum_k c_{s,j}[k] g_{s,t}[k]
    explained  = sum_j a(u, t, j),  score = (1/S) sum_s sum_k theta_s[u, k] g_{s,t}[k]

TEST INFRASTRUCTURE ONLY: nothing under mmsbm_amd/ imports it."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def user_rows(data, user):
    """(d_u, 2) [item, rating] of ``user`` in the order the triples were given (duplicates are separate rows)."""
    data = np.asarray(data, dtype=np.int64).reshape(-1, 3)
    return data[data[:, 0] == user][:, 1:]


def fold_w(pr, w):
    K, L, R = pr.shape
    W = np.zeros((K, L))
    for k in range(K):
        for l in range(L):
            for r in range(R):
                W[k, l] += w[r] * pr[k, l, r]
    return W


def item_g(W, eta_t):
    K, L = W.shape
    g = np.zeros(K)
    for k in range(K):
        for l in range(L):
            g[k] += W[k, l] * eta_t[l]
    return g


def row_shares(rows, theta_u, eta, pr):
    """c (d_u, K) of one slot: the share of each row that each group takes."""
    K = pr.shape[0]
    c = np.zeros((len(rows), K))
    for j, (i, r) in enumerate(rows):
        v = np.zeros(K)
        dot = 0.0
        for k in range(K):
            v[k] = float(np.dot(pr[k, :, r], eta[i]))
            dot += theta_u[k] * v[k]
        for k in range(K):
            c[j, k] = theta_u[k] * v[k] / max(dot, EPS)
    return c


class Restatement:
    """The answers for one model (S parameter sets (theta, eta, p)), one set of weights and the training triples; a
    user's shares and an item's g are computed once and kept."""

    def __init__(self, data, params, w):
        self.data = np.asarray(data, dtype=np.int64).reshape(-1, 3)
        self.params = [tuple(np.asarray(a, dtype=np.float64) for a in p) for p in params]
        self.w = np.asarray(w, dtype=np.float64)
        self.W = [fold_w(p, self.w) for _, _, p in self.params]
        self._c, self._g = {}, {}

    def rows(self, user):
        return user_rows(self.data, user)

    def shares(self, user):
        if user not in self._c:
            rows = self.rows(user)
            self._c[user] = [row_shares(rows, th[user], eta, pr) for th, eta, pr in self.params]
        return self._c[user]

    def g(self, item):
        if item not in self._g:
            self._g[item] = [item_g(W, eta[item]) for W, (_, eta, _) in zip(self.W, self.params)]
        return self._g[item]

    def pair(self, user, item):
        """dict: items, ratings (d_u,), a (d_u,) the contribution of every row, explained, score, degree."""
        user, item = int(user), int(item)
        rows, c, g = self.rows(user), self.shares(user), self.g(item)
        S, d, K = len(self.params), len(rows), len(g[0])
        a = np.zeros(d)
        score = 0.0
        for s in range(S):
            th = self.params[s][0][user]
            for k in range(K):
                a += c[s][:, k] * g[s][k]                 # (over the user's rows at once)
                score += th[k] * g[s][k]
        a = a / (S * d) if d else a
        explained = 0.0
        for j in range(d):
            explained += a[j]
        return {"items": rows[:, 0], "ratings": rows[:, 1], "a": a, "explained": explained, "score": score / S,
                "degree": d}

    def theta_next(self, user):
        """[theta'_u of each slot]: the mean of the user's shares -- one theta update with eta and p fixed."""
        return [c.sum(axis=0) / max(len(c), 1) for c in self.shares(int(user))]

    def query(self, users, offsets, items, n):
        """What HipEM.explain_query returns."""
        q = len(items)
        hi, hr = np.full((q, n), -1, dtype=np.int32), np.full((q, n), -1, dtype=np.int32)
        co = np.full((q, n), -np.inf)
        counts, degree = np.zeros(q, dtype=np.int32), np.zeros(q, dtype=np.int32)
        explained, score = np.zeros(q), np.zeros(q)
        for b, u in enumerate(users):
            for e in range(int(offsets[b]), int(offsets[b + 1])):
                r = self.pair(u, items[e])
                order = top_rows(r["items"], r["ratings"], r["a"], n)
                m = len(order)
                hi[e, :m], hr[e, :m], co[e, :m] = r["items"][order], r["ratings"][order], r["a"][order]
                counts[e], degree[e], explained[e], score[e] = m, r["degree"], r["explained"], r["score"]
        return hi, hr, co, counts, explained, score, degree


def top_rows(items, ratings, a, n):
    """The places of the n rows in front: contribution descending, equal ones by ascending item id, then rating."""
    return np.lexsort((ratings, items, -a))[:n]
