"""Positions of held-out items (HipEM.recommend_positions): time of one call over every test user of a 10 % hold-out,
at one and at eight restarts, the latency of a single user, and an all-user recommend_query of the same session next
to it (what recommend_time.py measures).

    python scripts/position_time.py [--config c3|c3s8|all] [--reps 5]

Shapes (random parameters: the time does not depend on their values):
  c3     BASELINE C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20, one restart; a random 10 % of the
         ratings held out (the rest is the training set whose items are excluded)
  c3s8   the same with 8 restarts (restart slots of one context)

The timed region is one recommend_positions call with every test user (median of --reps after one warm-up): HIP events
on the context's stream around the call's kernels (option "position_ms"); host_call_ms is the whole call, positions in
host memory.  query_all_ms is option "recommend_ms" of one recommend_query(all users, 10) in the same session.
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
from oracle import mmsbm_oracle as orc  # noqa: E402

SHAPES = {  # name: (ratings, users, items, R, K, L, restarts)
    "c3": (1_000_000, 100_000, 20_000, 5, 20, 20, 1),
    "c3s8": (1_000_000, 100_000, 20_000, 5, 20, 20, 8),
}


def one(name, reps):
    n_obs, U, I, R, K, L, S = SHAPES[name]
    data = synthetic_triples(n_obs, U, I, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    held = rng.random(len(data)) < 0.1
    train, test = data[~held], data[held]
    params = [(rng.random((U, K)), rng.random((I, L)), orc.normalize_with_self(rng.random((K, L, R)))) for _ in range(S)]
    w = np.arange(1.0, R + 1)
    order = np.argsort(test[:, 0], kind="stable")
    users, counts = np.unique(test[order, 0], return_counts=True)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    items = test[order, 1].astype(np.int32)
    users = users.astype(np.int32)
    with HipEM(train, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        em.recommend_begin(w, True)
        for s in range(S):
            em.select(s).recommend_add()
        em.recommend_positions(users, offsets, items)       # warm-up
        times, host = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            em.recommend_positions(users, offsets, items)
            host.append(time.perf_counter() - t0)
            times.append(em.get_option("position_ms"))      # HIP events around the call's kernels
        single, single_dev = [], []
        for b in rng.choice(len(users), 21, replace=False).tolist():
            sl = slice(int(offsets[b]), int(offsets[b + 1]))
            t0 = time.perf_counter()
            em.recommend_positions(users[b:b + 1], np.array([0, sl.stop - sl.start]), items[sl])
            single.append(time.perf_counter() - t0)
            single_dev.append(em.get_option("position_ms"))
        em.recommend_query(np.arange(U, dtype=np.int32), 10)
        query = em.get_option("recommend_ms")
        em.recommend_end()
    t = float(np.median(times))
    out = {"shape": name, "build_id": _lib.build_id(), "users": U, "items": I, "K": K, "L": L, "R": R, "restarts": S,
           "test_rows": int(len(items)), "test_users": int(len(users)),
           "position_ms": round(t, 3), "times_ms": [round(x, 3) for x in times],
           "host_call_ms": round(float(np.median(host)) * 1e3, 3),
           "single_user_ms": round(float(np.median(single)) * 1e3, 3),
           "single_user_device_ms": round(float(np.median(single_dev)), 3),
           "query_all_ms": round(query, 3)}
    print(f"{name:5s} {len(users):>7,} test users / {len(items):>8,} rows x {I:,} items, rank {min(K, L)} x {S}: "
          f"positions {t:8.2f} ms (host call {np.median(host) * 1e3:8.2f} ms)  one user {np.median(single) * 1e3:.3f} ms  "
          f"| recommend_query all users {query:8.2f} ms", flush=True)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=["all"] + list(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print(f"build {_lib.build_id()}", flush=True)
    for name in (SHAPES if args.config == "all" else [args.config]):
        one(name, args.reps)


if __name__ == "__main__":
    main()
