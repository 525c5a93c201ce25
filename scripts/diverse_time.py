"""Diversified top-N (HipEM.recommend_diverse): device times at BASELINE C3's shape next to the query that selects its
pool, recommend_query_within(n = pool), of the same sessions.

    python scripts/diverse_time.py [--reps 5] [--slots 1,8]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded.  Per S, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each, n = 10, trade_off 1:
    recommend_diverse with pool 50, 100 and 1,024 for all users, and for one user,
    recommend_query_within(n = pool) of the same request (without candidates and own lists it IS recommend_query: the
    parent's path, and the launches recommend_diverse issues before its own kernel).
Each figure is the median of the device times (HIP events around each call's kernels: options "diverse_ms" /
"recommend_ms"); the host time of the call, with its copies, is printed beside it.
answers_equal: for 200 sampled users at pool 100, recommend_diverse at trade_off 0 against recommend_query_within(10)
-- items and score bits -- and at trade_off 1 the picks' distances against similar_pairs of (pick, nearest earlier pick).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from mmsbm_amd import HipEM, _lib  # noqa: E402
from mmsbm_amd.synthetic import synthetic_triples  # noqa: E402

N_OBS, USERS, ITEMS, R, K, L = 1_000_000, 100_000, 20_000, 5, 20, 20
POOLS = (50, 100, 1024)
TOP, LAM = 10, 1.0


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def check(em, rng, users, n_users=200, pool=100):
    """(rows compared, rows equal)"""
    ask = users[np.sort(rng.choice(len(users), n_users, replace=False))]
    pi, ps, pc = em.recommend_query_within(ask, TOP)
    zi, zs, _, zc = em.recommend_diverse(ask, TOP, pool, 0.0)
    di, _, dd, dc = em.recommend_diverse(ask, TOP, pool, LAM)
    same = 0
    for b in range(n_users):
        ok = np.array_equal(pi[b], zi[b]) and np.array_equal(ps[b].view(np.uint64), zs[b].view(np.uint64)) and pc[b] == zc[b]
        for j in range(1, dc[b]):                              # the distance of pick j: the minimum over the earlier picks
            d = em.similar_pairs(di[b, :j], np.full(j, di[b, j], dtype=np.int32))
            ok = ok and d.min().view(np.uint64) == dd[b, j].view(np.uint64)
        same += int(ok)
    return n_users, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", default="1,8")
    args = ap.parse_args()
    slot_list = [int(x) for x in args.slots.split(",")]
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    S_max = max(slot_list)
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S_max)]
    users = np.arange(U, dtype=np.int32)
    one = users[U // 2:U // 2 + 1]
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for S in slot_list:
            em.recommend_begin(np.arange(1.0, R + 1), True)
            em.similar_begin("items")
            for s in range(S):
                em.select(s).recommend_add()
                em.similar_add()
            seen, same = check(em, rng, users)

            def timed(call, option):
                t0 = time.perf_counter()
                call()
                return em.get_option(option), (time.perf_counter() - t0) * 1e3

            calls = {}
            for who, ask in (("all", users), ("one", one)):
                for pool in POOLS:
                    calls[f"diverse_{who}_pool{pool}"] = (lambda a=ask, p=pool: em.recommend_diverse(a, TOP, p, LAM), "diverse_ms")
                    calls[f"query_within_{who}_n{pool}"] = (lambda a=ask, p=pool: em.recommend_query_within(a, p), "recommend_ms")
            dev = {k: [] for k in calls}
            host = {k: [] for k in calls}
            for rep in range(args.reps + 1):                       # rep 0: the warm-up of each
                for k, (call, option) in calls.items():            # alternating
                    d, h = timed(call, option)
                    if rep:
                        dev[k].append(d)
                        host[k].append(h)
            out = {"build_id": _lib.build_id(), "users": U, "items": I, "profile_width": K * R, "restarts": S,
                   "reps": args.reps, "n": TOP, "trade_off": LAM,
                   "device_ms": {k: round(float(np.median(v)), 3) for k, v in dev.items()},
                   "host_ms": {k: round(float(np.median(v)), 3) for k, v in host.items()},
                   "rows_compared": seen, "answers_equal": bool(seen > 0 and same == seen)}
            print(json.dumps(out), flush=True)
            em.similar_end()
            em.recommend_end()


if __name__ == "__main__":
    main()
