"""What every serving query launches and returns -- the cases of tests/test_gpu_serving_launches.py and the recorder of
their expected table.

A case opens one context, runs one query and closes the context (the library appends its launch counts to
MMSBM_HIP_LAUNCH_LOG when a context is destroyed).  Recorded per case: the launch count per kernel name of this process
since the case began, and a SHA-256 per output array.  The kernels use no atomics -- top_pairs_bulk's only for counts and
for places that a sort then orders --, so on one device type both are a function of the library alone (two recordings of
one commit are equal, case by case).  The shapes are the smallest that take every branch of the queries' host side:

  BASIC    exact_models.SPLIT[1]: 3 users over 5,000 items -- the selection splits across waves and merges
  WIDE     129 users over 70,000 items: a batch of the 128 MB score buffer holds 128 rows, so 129 rows are two batches
           (128 + 1) and the second batch's first row is not 0; 300 groups are three
  MID      the same users over 5,000 items: groups, audience and diverse in one batch

The table a commit gives is recorded with

    python tests/serving_launch_cases.py --out tests/gpu_serving_launches_parent.json [--tree DIR]

(--tree: the checkout whose mmsbm_amd is imported, e.g. a build of the parent commit; this file's own by default).  The
committed table is the one of the commit BEFORE the queries' host side moved onto shared helpers and serve_plan.hpp: the
refactor must not move an entry.  The cases from "quota" on were recorded before the queries added since then (quota,
shelves, explore, allocate, assign, assortment, top_pairs_bulk, ensemble, the item side) moved onto one selection stage
and one batch frame, with the library's sources as that commit's.  The four from "theta-quota-candidates" on (the theta
entries' seen lists and the propensity lists beside a candidate subset) were recorded, twice and equal, from the commit
before the requests crossed from the C ABI into the units as values (abi_request.hpp).
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

BASIC = (3, 5000, 4, 6, 5, 2)      # U, I, K, L, R, S
WIDE = (129, 70_000, 4, 6, 3, 2)
MID = (129, 5000, 4, 6, 3, 2)
GROUP_SIZES = (1, 2, 7, 8, 9, 127, 128, 129)
GROUP_MODES = ("min", "max", "count", "mean")
_MODELS = {}


def model(shape):
    """(data, params, weights) of a shape: random triples and S parameter sets whose rows sum to 1.  Computed once."""
    if shape not in _MODELS:
        U, I, K, L, R, S = shape
        rng = np.random.default_rng(list(shape))
        n_obs = 20 * U + 2000
        data = np.stack([rng.integers(0, U, n_obs), rng.integers(0, I, n_obs), rng.integers(0, R, n_obs)], 1)
        simplex = lambda *dims: (lambda a: a / a.sum(axis=-1, keepdims=True))(rng.random(dims) + 0.01)  # noqa: E731
        params = [(simplex(U, K), simplex(I, L), simplex(K, L, R)) for _ in range(S)]
        _MODELS[shape] = (data, params, np.arange(1.0, R + 1))
    return _MODELS[shape]


def csr(lists, dtype=np.int32):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off, (np.concatenate(lists) if len(lists) else np.zeros(0)).astype(dtype)


def own_lists(rng, rows, I):
    """The query's own excluded items of `rows` request rows: any order, with a repeat, one row without any."""
    lists = [rng.integers(0, I, 1 + b % 5) for b in range(rows)]
    lists[0] = np.concatenate([lists[0], lists[0][:1]])
    if rows > 1:
        lists[1] = np.zeros(0, dtype=np.int64)
    return csr(lists)


def theta_rows(rng, S, M, K):
    a = rng.random((S, M, K)) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def group_request(U, many):
    """GROUP_SIZES (and an empty group) in one batch -- or, `many`, 300 groups: 128 groups of one; 60 of one, a group
    of 129 (cut into fragments at 16 blocks a run) and 67 of one; then GROUP_SIZES, whose last group is cut too."""
    rng = np.random.default_rng(77)
    draw = lambda s: rng.permutation(U)[:s]  # noqa: E731
    groups = [draw(s) for s in GROUP_SIZES[:4]] + [np.zeros(0, dtype=np.int64)] + [draw(s) for s in GROUP_SIZES[4:]]
    if many:
        groups = [draw(1) for _ in range(188)] + [draw(129)] + [draw(1) for _ in range(67)] + groups
    return csr(groups)


def audience_runs(counts, rows, cap):
    """[(first row, rows), ...] of the WRITE launches: inside batches of `rows` rows, consecutive rows whose entries
    stay within `cap` (a larger row goes alone); a run without entries is not launched."""
    runs = []
    for r0 in range(0, len(counts), rows):
        batch, s0 = counts[r0:r0 + rows], 0
        while s0 < len(batch):
            s1, e = s0 + 1, int(batch[s0])
            while s1 < len(batch) and e + batch[s1] <= cap:
                e, s1 = e + int(batch[s1]), s1 + 1
            if e > 0:
                runs.append((r0 + s0, s1 - s0))
            s0 = s1
    return runs


# ---- the cases: name -> (shape, sessions to open, the query) ---------------------------------------------------------------
def _basic(query):
    return (BASIC, ("recommend",), query)


def _groups(mode, many):
    def query(em, shape):
        U, I = shape[:2]
        off, mem = group_request(U, many)
        em.set_option("group_run_blocks", 16)
        cand = None if many else np.arange(0, I, 3, dtype=np.int32)
        return em.recommend_query_groups(off, mem, 10, mode, bar=2.0, candidates=cand)
    return (WIDE if many else MID, ("recommend",), query)


def _audience(em, shape):
    U, I = shape[:2]
    items = np.arange(0, 70, 10, dtype=np.int32)
    sample = em.recommend_query(np.arange(U, dtype=np.int32), 1000)[1]
    bar = float(np.percentile(sample[np.isfinite(sample)], 10))   # (of every user's 1,000 best: about a sixth of all pairs)
    counts = np.diff(em.recommend_audience(items, bar, count_only=True)[0])
    # the smallest entry cap under which one row goes alone and two rows share a run
    caps = [cap for cap in range(1, int(counts.sum()) + 1)
            if {1, 2} <= {n for _, n in audience_runs(counts, 3, cap)}]
    assert caps, counts
    em.set_option("audience_rows", 3)
    em.set_option("audience_entries", caps[0])
    return em.recommend_audience(items, bar)


def _diverse(em, shape):
    I = shape[1]
    rng = np.random.default_rng(5)
    em.set_option("diverse_rows", 2)
    return em.recommend_diverse(np.array([4, 0, 128, 17, 64], dtype=np.int32), 5, 40, 0.5,
                                candidates=np.arange(1, I, 2, dtype=np.int32), exclude=own_lists(rng, 5, I))


def _top_pairs(em, shape):
    em.set_option("top_pairs_groups", 7)
    return em.recommend_top_pairs(50)


def _rank(em, shape):
    U, I = shape[:2]
    rng = np.random.default_rng(9)
    off, it = csr([np.sort(rng.choice(I, s, replace=False)) for s in (300, 0, 2500)])
    return em.recommend_rank(np.arange(U, dtype=np.int32), off, it, 10)


def _positions(em, shape):
    U, I = shape[:2]
    rng = np.random.default_rng(10)
    off, it = csr([rng.choice(I, s, replace=False) for s in (5, 0, 40)])
    return em.recommend_positions(np.arange(U, dtype=np.int32), off, it)


def _users(shape):
    return np.arange(shape[0], dtype=np.int32)


def _cand(shape):
    return np.arange(0, shape[1], 2, dtype=np.int32)       # 2,500 columns: still split across waves


def _rng():
    return np.random.default_rng(21)


def _cats(I):
    """(offsets, items) of six disjoint categories of catalogue items: two long ones (the multiples of 4; 1 mod 4), a
    short one of 50 and one of 5 even items (2 mod 4), a short one of 4 odd items (3 mod 4: no candidate of _cand) and
    one of 2 (never full under _CAPS: quota drops it, as it drops the second long one, whose cap is n)."""
    return csr([np.arange(0, I, 4), np.arange(2, I, I // 50)[:50], np.array([6, 10, 14, 18, 22]),
                np.array([3, 7, 11, 15]), np.array([26, 30]), np.arange(1, I, 4)], dtype=np.int32)


_CAPS = np.array([3, 1, 2, 1, 5, 10], dtype=np.int32)     # (n = 10: the last two never bind, so plan_quota drops them)


def _state():
    return np.random.PCG64(5)                              # the four state words of a fixed stream


def _lists(shape):
    rng = np.random.default_rng(12)
    return csr([rng.choice(shape[1], s, replace=False) for s in (0, 1, 40)])


def _allocate(caps_of, n, max_rounds=10000, rounds_at_least=1):
    def query(em, shape):
        items, scores, counts, info = em.recommend_allocate(_users(shape), n, caps_of(shape[1]), max_rounds=max_rounds)
        assert info["rounds"] >= rounds_at_least and info["rounds"] == em.get_option("allocate_rounds"), info
        return items, scores, counts, info["rounds"], info["converged"]
    return query


def _assign(max_rounds=10000, rounds_at_least=1):
    def query(em, shape):
        U, I = shape[:2]
        caps = np.array([0, 1, 2, -1], dtype=np.int32)[np.arange(I) % 4]    # p1 / p2 take every initial value
        out = em.recommend_assign(np.random.default_rng(13).permutation(U), caps, 0.0, 0.05, max_rounds=max_rounds)
        assert out["rounds"] >= rounds_at_least, out["rounds"]
        return [out[k] for k in ("items", "scores", "paid", "pi", "price", "price_sum", "load", "rounds", "converged",
                                 "bids")]
    return query


def _assortment(mode, level):
    def query(em, shape):
        U, I = shape[:2]
        users = np.random.default_rng(14).permutation(U)
        items, gains, n, stop, s_items, s_scores, start = em.recommend_assortment(
            users, 6, mode, level, given=[3, 10], candidates=np.arange(0, I, 3, dtype=np.int32))
        assert n >= 2, (n, stop)
        return items, gains, n, em.ASSORT_STOPS.index(stop), s_items, s_scores, start
    return query


def _top_pairs_bulk(em, shape):
    em.set_option("pairs_bulk_collect", 256)               # (15,000 candidates: histogram passes, then a collected bin)
    users, items, scores, count, info = em.recommend_top_pairs_bulk(2000)
    return users, items, scores, count, info["bar"], info["above"], info["ties"], info["candidates"]


def _pair_bar(em, shape):
    em.set_option("pairs_bulk_collect", 256)
    info = em.recommend_pair_bar(2000)
    return info["bar"], info["above"], info["ties"], info["candidates"]


CASES = {
    "recommend": _basic(lambda em, s: em.recommend_query(_users(s), 10)),
    "within-candidates": _basic(lambda em, s: em.recommend_query_within(_users(s), 10, candidates=_cand(s))),
    "within-own": _basic(lambda em, s: em.recommend_query_within(_users(s), 10, exclude=own_lists(_rng(), s[0], s[1]))),
    "within-both": _basic(lambda em, s: em.recommend_query_within(_users(s), 10, candidates=_cand(s),
                                                                  exclude=own_lists(_rng(), s[0], s[1]))),
    "theta": _basic(lambda em, s: em.recommend_query_theta(theta_rows(_rng(), s[5], 4, s[2]), 10,
                                                           seen=own_lists(_rng(), 4, s[1]))),
    "theta-within": _basic(lambda em, s: em.recommend_query_theta(theta_rows(_rng(), s[5], 4, s[2]), 10,
                                                                  seen=own_lists(_rng(), 4, s[1]), candidates=_cand(s))),
    "rank": _basic(_rank),
    "positions": _basic(_positions),
    "top-pairs": _basic(_top_pairs),
    "inform": (BASIC, ("inform",), lambda em, s: em.inform_query(_users(s), 10)),
    "inform-theta": (BASIC, ("inform",), lambda em, s: em.inform_query_theta(theta_rows(_rng(), s[5], 4, s[2]), 10,
                                                                             seen=own_lists(_rng(), 4, s[1]))),
    "inform-mask-own": (BASIC, ("inform",), lambda em, s: em.inform_query(_users(s), 10, candidates=_cand(s),
                                                                          exclude=own_lists(_rng(), s[0], s[1]))),
    "two-batches-recommend": (WIDE, ("recommend",), lambda em, s: em.recommend_query_within(
        _users(s), 10, exclude=own_lists(_rng(), s[0], s[1]))),
    "two-batches-inform": (WIDE, ("inform",), lambda em, s: em.inform_query(_users(s), 10,
                                                                            exclude=own_lists(_rng(), s[0], s[1]))),
    **{f"groups-{mode}": _groups(mode, False) for mode in GROUP_MODES},
    **{f"groups-{mode}-three-batches": _groups(mode, True) for mode in GROUP_MODES},
    "audience": (MID, ("recommend",), _audience),
    "diverse": (MID, ("recommend", "similar"), _diverse),
    "quota": _basic(lambda em, s: em.recommend_query_quota(_users(s), 10, *_cats(s[1]), _CAPS)),
    "quota-candidates": _basic(lambda em, s: em.recommend_query_quota(_users(s), 10, *_cats(s[1]), _CAPS, candidates=_cand(s),
                                                                      exclude=own_lists(_rng(), s[0], s[1]))),
    "theta-quota": _basic(lambda em, s: em.recommend_query_theta_quota(theta_rows(_rng(), s[5], 4, s[2]), 10, *_cats(s[1]),
                                                                       _CAPS, seen=own_lists(_rng(), 4, s[1]))),
    "shelves-items": _basic(lambda em, s: em.recommend_query_shelves(_users(s), *_cats(s[1]), 5, 1, 3, 4)),
    "shelves-values": _basic(lambda em, s: em.recommend_query_shelves(_users(s), *_cats(s[1]), 5, 3, 3, 0, candidates=_cand(s),
                                                                      exclude=own_lists(_rng(), s[0], s[1]))),
    "theta-shelves": _basic(lambda em, s: em.recommend_query_theta_shelves(theta_rows(_rng(), s[5], 4, s[2]), *_cats(s[1]), 5,
                                                                           1, 3, 4, seen=own_lists(_rng(), 4, s[1]))),
    "two-batches-shelves": (WIDE, ("recommend",), lambda em, s: em.recommend_query_shelves(
        _users(s), *_cats(s[1]), 5, 1, 3, 4, exclude=own_lists(_rng(), s[0], s[1]))),
    "explore": _basic(lambda em, s: em.recommend_query_explore(_users(s), 10, 0.1, _state())),
    "explore-candidates": _basic(lambda em, s: em.recommend_query_explore(_users(s), 10, 0.1, _state(), candidates=_cand(s),
                                                                          exclude=own_lists(_rng(), s[0], s[1]))),
    "two-batches-explore": (WIDE, ("recommend",), lambda em, s: em.recommend_query_explore(_users(s), 10, 0.1, _state())),
    "list-propensity": _basic(lambda em, s: em.recommend_list_propensity(_users(s), _lists(s), 0.1, candidates=_cand(s))),
    "allocate-free": _basic(_allocate(lambda I: np.full(I, -1, dtype=np.int32), 10)),
    "allocate": (MID, ("recommend",), _allocate(lambda I: np.array([1, -1, 2, 0, 3, -1], dtype=np.int32)[np.arange(I) % 6], 10,
                                                rounds_at_least=2)),
    "allocate-wide": (WIDE, ("recommend",), _allocate(lambda I: (1 + np.arange(I) % 3).astype(np.int32), 10, max_rounds=3)),
    "assign": (MID, ("recommend",), _assign(rounds_at_least=2)),
    "assign-wide": (WIDE, ("recommend",), _assign(max_rounds=3)),
    "assortment-best": (MID, ("recommend",), _assortment("best_score", 1.0)),
    "assortment-reach": (MID, ("recommend",), _assortment("reach", 2.055)),   # (a bar that each round's item still reaches)
    "top-pairs-bulk": _basic(_top_pairs_bulk),
    "pair-bar": _basic(_pair_bar),
    "ensemble-lcb": _basic(lambda em, s: em.recommend_query_ensemble(_users(s), 10, "lcb", risk=1.0, candidates=_cand(s),
                                                                     exclude=own_lists(_rng(), s[0], s[1]))),
    "ensemble-min": _basic(lambda em, s: em.recommend_query_ensemble(_users(s), 10, "min", candidates=_cand(s),
                                                                     exclude=own_lists(_rng(), s[0], s[1]))),
    "items": (MID, ("recommend",), lambda em, s: em.recommend_query_items(np.arange(0, s[1], 25, dtype=np.int32), 10)),
    # the theta entries' seen lists and the propensity lists beside a candidate subset (recorded before the requests
    # crossed into the units as values)
    "theta-quota-candidates": _basic(lambda em, s: em.recommend_query_theta_quota(
        theta_rows(_rng(), s[5], 4, s[2]), 10, *_cats(s[1]), _CAPS, seen=own_lists(_rng(), 4, s[1]), candidates=_cand(s))),
    "theta-shelves-candidates": _basic(lambda em, s: em.recommend_query_theta_shelves(
        theta_rows(_rng(), s[5], 4, s[2]), *_cats(s[1]), 5, 1, 3, 4, seen=own_lists(_rng(), 4, s[1]), candidates=_cand(s))),
    "inform-theta-candidates": (BASIC, ("inform",), lambda em, s: em.inform_query_theta(
        theta_rows(_rng(), s[5], 4, s[2]), 10, seen=own_lists(_rng(), 4, s[1]), candidates=_cand(s))),
    "list-propensity-own": _basic(lambda em, s: em.recommend_list_propensity(
        _users(s), _lists(s), 0.1, candidates=_cand(s), exclude=own_lists(_rng(), s[0], s[1]))),
}


def _digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def _launches(path, pos):
    """{kernel name: launches} of this process in the log behind `pos`."""
    counts = {}
    if os.path.exists(path):
        with open(path) as fh:
            fh.seek(pos)
            for row in (ln.rstrip("\n").split("\t") for ln in fh):
                if len(row) >= 4 and row[0] == str(os.getpid()):
                    counts[row[2]] = counts.get(row[2], 0) + int(row[1])
    return counts


def run_case(pkg, name):
    """{"launches": {kernel: count}, "outputs": [sha256, ...]} of one case."""
    shape, sessions, query = CASES[name]
    U, I, K, L, R, S = shape
    data, params, w = model(shape)
    path = os.environ["MMSBM_HIP_LAUNCH_LOG"]
    pos = os.path.getsize(path) if os.path.exists(path) else 0
    em = pkg.HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S)
    try:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for kind in sessions:
            {"recommend": lambda: em.recommend_begin(w, True), "inform": em.inform_begin,
             "similar": lambda: em.similar_begin("items")}[kind]()
            for s in range(S):
                getattr(em.select(s), kind + "_add")()
        out = query(em, shape)
    finally:
        em.close()
    return {"launches": dict(sorted(_launches(path, pos).items())), "outputs": [_digest(a) for a in out if a is not None]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    if not os.environ.get("MMSBM_HIP_LAUNCH_LOG"):   # (the library reads it when it is loaded)
        os.environ["MMSBM_HIP_LAUNCH_LOG"] = os.path.join(tempfile.mkdtemp(), "launch_log.tsv")
    sys.path.insert(0, os.path.abspath(args.tree))
    import mmsbm_amd
    table = {name: run_case(mmsbm_amd, name) for name in CASES}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(table, fh, indent=1)
        fh.write("\n")
    print(f"{len(table)} cases from {os.path.dirname(mmsbm_amd.__file__)} -> {args.out}")


if __name__ == "__main__":
    main()
