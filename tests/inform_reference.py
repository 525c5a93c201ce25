"""The numpy restatement of the information gain the inform session computes on the device (mmsbm_amd/csrc/inform.hpp),
of the population's mean membership and of the top-n order; test_inform_cpu.py checks the restatement itself,
test_gpu_inform.py compares the device against it.

    q_s[i, k, r] = sum_l eta_s[i, l] p_s[k, l, r]                           the rating profile of item i
    gain_s(u, i) = H( sum_k theta_s[u,k] q_s[i,k,.] ) - sum_k theta_s[u,k] H( q_s[i,k,.] )       (nats)
    gain(u, i)   = (1/S) sum_s max(gain_s(u, i), 0)
    H(x)         = sum_r phi(x_r),   phi(x) = -x log x for x > 0, else 0
Order: gain descending, equal gains by ascending item id (np.lexsort((id, -gain))).

The error bound, ``tolerance(K, L, R, S)``.  Write u = 2^-53 (half an ulp of 1) and take theta and eta rows that sum
to 1 and p[k, l, :] that sum to 1, so every q, every mixture m_r and every weight lies in [0, 1] and every entropy in
[0, log R].
  * q is a sum of L non-negative products: relative error <= (L + 1) u, whatever the order of the sum.
  * m_r = sum_k theta_k q_k is a sum of K non-negative products of such q: relative error <= (K + 1) u + (L + 1) u.
  * phi(x (1 + e)) - phi(x) = -e x (1 + log x) to first order, and x |1 + log x| <= 1 on [0, 1]: a relative error e of
    the argument moves phi by at most |e|, whatever x.  The device's and numpy's log are accurate to 1 ulp = 2 u and the
    product x log x is rounded once more: x |log x| <= 1/e, so both add at most 3 u / e <= 2 u.  One phi term of H
    therefore carries an absolute error <= (K + L + 4) u, one of an item's own h[i, k] <= (L + 3) u.
  * H adds R such terms, each partial sum <= log R: R (K + L + 4) u + R u log R.  h[i, k] likewise: R (L + 3) u +
    R u log R; lin = sum_k theta_k h_k is a convex combination of them (no larger an error) plus the K-chain's own
    rounding, (K + 1) u log R.  The subtraction H - lin rounds once more: u log R; max(., 0) moves nothing further.
  * The mean over S slots does not enlarge the slots' errors; its S additions of partial sums <= S log R and the
    division add (S + 1) u log R after the division.
  Sum: u ( R (K + 2 L + 7) + (2 R + K + S + 3) log R ), with log R taken as log max(R, 2) so that R = 1 keeps the
  chain terms.  Doubled for the restatement's own rounding, which obeys the same bound:

    tolerance(K, L, R, S) = 2 x 2^-53 x ( R (K + 2 L + 7) + (2 R + K + S + 3) log max(R, 2) )

It is an absolute bound on a quantity in [0, log min(K, R)], derived from the operation counts alone; nothing in it is
tuned to what the device returns.
"""
import numpy as np

MASS_BLOCK = 256            # sim_mass_kernel: thread t adds rows t, t + 256, ... then the partial sums are halved 8 times


def tolerance(K, L, R, S=1):
    return 2.0 * 2.0 ** -53 * (R * (K + 2 * L + 7) + (2 * R + K + S + 3) * np.log(max(R, 2)))


def phi(x):
    """-x log x where x > 0, +0.0 elsewhere."""
    x = np.asarray(x, dtype=np.float64)
    safe = np.where(x > 0, x, 1.0)
    return np.where(x > 0, -(safe * np.log(safe)), 0.0)


def profiles(params):
    """Per restart (q (I, K, R), h (I, K)): the items' rating profiles and the entropy of each profile row."""
    out = []
    for _, eta, p in params:
        q = np.einsum("il,klr->ikr", eta, p)
        out.append((q, phi(q).sum(axis=2)))
    return out


def gains(params, thetas, chunk=64):
    """(M, I): gain of every (query row, item) pair.  thetas: one (M, K) block per restart of ``params``."""
    prof = profiles(params)
    M, I = thetas[0].shape[0], prof[0][0].shape[0]
    acc = np.zeros((M, I))
    for b in range(0, M, chunk):
        for (q, h), th in zip(prof, thetas):
            t = np.asarray(th[b:b + chunk], dtype=np.float64)
            H = phi(np.einsum("uk,ikr->uir", t, q)).sum(axis=2)
            acc[b:b + chunk] += np.maximum(H - t @ h.T, 0.0)
    return acc / float(len(params))


def gains_of_users(params, users):
    """gains for training users: each restart's own theta rows."""
    users = np.asarray(users, dtype=np.int64)
    return gains(params, [theta[users] for theta, _, _ in params])


def mass_fixed_order(theta):
    """sum_u theta[u, :] in sim_mass_kernel's order: 256 running sums over rows t, t + 256, ... from +0.0, then halved
    with strides 128, 64, ... 1."""
    U, K = theta.shape
    part = np.zeros((MASS_BLOCK, K))
    for start in range(0, U, MASS_BLOCK):
        block = theta[start:start + MASS_BLOCK]
        part[:len(block)] += block
    o = MASS_BLOCK // 2
    while o > 0:
        part[:o] += part[o:2 * o]
        o //= 2
    return part[0]


def mean_theta(params):
    """(S, K): the population's mean membership per restart, the fixed-order sum divided once by U."""
    return np.stack([mass_fixed_order(theta) / float(theta.shape[0]) for theta, _, _ in params])


def top_n(gain, n, allowed=None):
    """(items (M, n) padded with -1, gains (M, n) padded with -inf, counts (M,)) from gains (M, I); allowed: None or a
    boolean (M, I) / (I,) array, False where an item is no candidate."""
    M, I = gain.shape
    ok = np.ones((M, I), dtype=bool) if allowed is None else np.broadcast_to(np.asarray(allowed, dtype=bool), (M, I))
    items = np.full((M, n), -1, dtype=np.int32)
    vals = np.full((M, n), -np.inf)
    counts = np.zeros(M, dtype=np.int32)
    for b in range(M):
        cand = np.flatnonzero(ok[b])
        order = cand[np.lexsort((cand, -gain[b, cand]))][:n]
        counts[b] = len(order)
        items[b, :len(order)] = order
        vals[b, :len(order)] = gain[b, order]
    return items, vals, counts


def allowed_mask(M, I, candidates=None, lists=None):
    """The boolean (M, I) candidate mask: inside ``candidates`` (ids; None: all) and outside row b's
    lists = (offsets, items)."""
    ok = np.ones((M, I), dtype=bool)
    if candidates is not None:
        ok[:] = False
        ok[:, np.asarray(candidates, dtype=np.int64)] = True
    if lists is not None:
        off, it = lists
        for b in range(M):
            ok[b, np.asarray(it[off[b]:off[b + 1]], dtype=np.int64)] = False
    return ok


def train_lists(data, users):
    """(offsets, items): the training items of each requested user, from triples ``data``."""
    data = np.asarray(data)
    per = [np.unique(data[data[:, 0] == u, 1]) for u in np.asarray(users).tolist()]
    off = np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.int64)
    return off, (np.concatenate(per) if per else np.zeros(0)).astype(np.int32)
