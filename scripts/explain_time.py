"""Explaining recommendations (HipEM.explain_query): device times at BASELINE C3's shape next to the query that made
the lists.

    python scripts/explain_time.py [--reps 5] [--slots 1,8]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded.  Per S, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each:
    explain_query(every user's top-10 list, n = 5), explain_query(one user's list), explain_query(the list of the user
    with the most training rows) and recommend_query(all users, n = 10).
Each figure is the median of the device times (HIP events around each call's kernels: options "explain_ms",
"recommend_ms"); the host time of the call, with the copies of the answers, is printed beside it.  scores_equal: the
explain session's score of every pair against recommend_query's, by their bits (K <= L here).
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
TOP, N = 10, 5


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", default="1,8")
    args = ap.parse_args()
    slot_list = [int(x) for x in args.slots.split(",")]
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    degree = np.bincount(data[:, 0], minlength=U)
    rng = np.random.default_rng(1)
    S_max = max(slot_list)
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S_max)]
    users = np.arange(U, dtype=np.int32)
    w = np.arange(1.0, R + 1)
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for S in slot_list:
            em.recommend_begin(w, True)
            em.explain_begin(w)
            for s in range(S):
                em.select(s).recommend_add()
                em.select(s).explain_add()
            items, scores, counts = em.recommend_query(users, TOP)
            assert (counts == TOP).all()
            offsets = np.arange(U + 1, dtype=np.int64) * TOP
            flat = np.ascontiguousarray(items.reshape(-1))
            one, heavy = int(rng.integers(0, U)), int(np.argmax(degree))

            def listed(u):
                return np.array([u], dtype=np.int32), np.array([0, TOP], dtype=np.int64), flat[u * TOP:(u + 1) * TOP]

            def timed(call, option):
                t0 = time.perf_counter()
                out = call()
                return em.get_option(option), (time.perf_counter() - t0) * 1e3, out

            calls = {"explain_all_top10_n5": (lambda: em.explain_query(users, offsets, flat, N), "explain_ms"),
                     "explain_one_user": (lambda: em.explain_query(*listed(one), N), "explain_ms"),
                     "explain_heavy_user": (lambda: em.explain_query(*listed(heavy), N), "explain_ms"),
                     "recommend_query_all_n10": (lambda: em.recommend_query(users, TOP), "recommend_ms")}
            dev = {k: [] for k in calls}
            host = {k: [] for k in calls}
            equal = None
            for rep in range(args.reps + 1):                       # rep 0: the warm-up of each
                for k, (call, option) in calls.items():          # alternating
                    d, h, out = timed(call, option)
                    if rep:
                        dev[k].append(d)
                        host[k].append(h)
                    elif k == "explain_all_top10_n5":
                        equal = bool(np.array_equal(out[5].view(np.uint64), scores.reshape(-1).view(np.uint64)))
            out = {"build_id": _lib.build_id(), "users": U, "items": I, "K": K, "L": L, "restarts": S, "reps": args.reps,
                   "pairs": int(len(flat)), "rows": int(degree.sum()), "heavy_user_rows": int(degree[heavy]),
                   "one_user_rows": int(degree[one]),
                   "device_ms": {k: round(float(np.median(v)), 3) for k, v in dev.items()},
                   "device_ms_all": {k: [round(float(x), 3) for x in v] for k, v in dev.items()},
                   "host_ms": {k: round(float(np.median(v)), 3) for k, v in host.items()},
                   "scores_equal": equal}
            print(json.dumps(out), flush=True)
            em.explain_end()
            em.recommend_end()


if __name__ == "__main__":
    main()
