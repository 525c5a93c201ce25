"""Capacity-aware allocation (HipEM.recommend_allocate): rounds and device times at BASELINE C3's shape next to the two
plain queries a round consists of.

    python scripts/allocate_time.py [--reps 3] [--slots 1,8] [--max-rounds 10000] [--cases 10:50,10:100,10:1000,1:5]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded, all users.  Per S and per (n, cap) -- every item with the same cap --, IN ONE PROCESS:
    recommend_query(all users, n) and recommend_query_items(all items, n = cap), alternating, --reps times after one
        warm-up of each: the median of the device times (option "recommend_ms").  Their sum is the yardstick of one
        round: a round is the first with a threshold epilogue, then the second over the capped items with one;
    recommend_allocate(all users, n, caps), once after them: rounds, converged, device time of the whole call (option
        "allocate_ms": the host's one read per round included) and per round, the host time of the call, the rows
        filled, and the largest item load before (the plain query's lists) and after.
One JSON line per (S, n, cap), printed as soon as it is measured.
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


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", default="1,8")
    ap.add_argument("--max-rounds", type=int, default=10000)
    ap.add_argument("--cases", default="10:50,10:100,10:1000,1:5")
    args = ap.parse_args()
    slot_list = [int(x) for x in args.slots.split(",")]
    cases = [tuple(int(v) for v in c.split(":")) for c in args.cases.split(",")]
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    S_max = max(slot_list)
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S_max)]
    users, items = np.arange(U, dtype=np.int32), np.arange(I, dtype=np.int32)
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, prm in enumerate(params):
            em.select(s).set_params(*prm)
        for S in slot_list:
            em.recommend_begin(np.arange(1.0, R + 1), True)
            for s in range(S):
                em.select(s).recommend_add()
            for n, cap in cases:
                plain = {"query": lambda: em.recommend_query(users, n), "query_items": lambda: em.recommend_query_items(items, cap)}
                ms = {k: [] for k in plain}
                last = {}
                for rep in range(args.reps + 1):                      # rep 0: the warm-up of each
                    for k, call in plain.items():                     # alternating
                        last[k] = call()
                        if rep:
                            ms[k].append(em.get_option("recommend_ms"))
                med = {k: float(np.median(v)) for k, v in ms.items()}
                caps = np.full(I, cap, dtype=np.int32)
                t0 = time.perf_counter()
                got_items, _, counts, info = em.recommend_allocate(users, n, caps, args.max_rounds)
                host = (time.perf_counter() - t0) * 1e3
                total = em.get_option("allocate_ms")
                before = np.bincount(last["query"][0][last["query"][0] >= 0], minlength=I)
                after = np.bincount(got_items[got_items >= 0], minlength=I)
                one_round = med["query"] + med["query_items"]
                print(json.dumps({
                    "build_id": _lib.build_id(), "users": U, "items": I, "restarts": S, "n": n, "cap": cap,
                    "rounds": info["rounds"], "converged": info["converged"], "allocate_ms": round(total, 2),
                    "ms_per_round": round(total / info["rounds"], 3), "host_ms": round(host, 2),
                    "query_ms": round(med["query"], 3), "query_items_ms": round(med["query_items"], 3),
                    "two_queries_ms": round(one_round, 3), "round_over_two_queries": round(total / info["rounds"] / one_round, 3),
                    "filled": int(counts.sum()), "requested": U * n, "largest_load_before": int(before.max()),
                    "items_over_cap_before": int((before > cap).sum()), "largest_load_after": int(after.max())}), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
