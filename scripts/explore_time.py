"""Randomised top-N with propensities (HipEM.recommend_query_explore / recommend_list_propensity): device times at
BASELINE C3's shape next to the plain query of the same session.

    python scripts/explore_time.py [--reps 5] [--slots 1,8]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded.  Per S, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each, n = 10, temperature 0.5:
    recommend_query_explore, all users and one user,
    recommend_list_propensity of the all-user call's own output, all users and one user,
    recommend_query (the parent's path: the same tiles, exclusions and selection, no noise), all users and one user.
Each figure is the median of the device times (HIP events around each call's kernels: option "recommend_ms"); the host
time of the call, with its copies and allocations, is printed beside it.
answers_equal: recommend_list_propensity of the all-user call's lists returns that call's propensity bits, and every
returned score is recommend_query(n = 1024)'s score of that item for 500 sampled users (where the item is among them).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from mmsbm_amd import HipEM, _lib  # noqa: E402
from mmsbm_amd.core import pcg64_words  # noqa: E402
from mmsbm_amd.synthetic import synthetic_triples  # noqa: E402

N_OBS, USERS, ITEMS, R, K, L = 1_000_000, 100_000, 20_000, 5, 20, 20
TOP, TEMPERATURE = 10, 0.5


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def lists_of(items, counts):
    keep = np.arange(items.shape[1])[None, :] < counts[:, None]
    return (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), items[keep]), keep


def check(em, rng, users, state, n_users=500):
    items, scores, prop, counts = em.recommend_query_explore(users, TOP, TEMPERATURE, state)
    lists, keep = lists_of(items, counts)
    sc, pr = em.recommend_list_propensity(users, lists, TEMPERATURE)
    same = np.array_equal(pr.view(np.uint64), prop[keep].view(np.uint64)) and np.array_equal(sc.view(np.uint64), scores[keep].view(np.uint64))
    pick = np.sort(rng.choice(len(users), n_users, replace=False))
    fi, fs, fc = em.recommend_query(users[pick], 1024)
    seen = 0
    for b, row in enumerate(pick.tolist()):
        at = {int(i): k for k, i in enumerate(fi[b, :fc[b]].tolist())}
        for k in range(counts[row]):
            if int(items[row, k]) in at:
                seen += 1
                same = same and fs[b, at[int(items[row, k])]] == scores[row, k]
    return seen, bool(same), float(np.median(np.prod(np.where(keep, prop, 1.0), axis=1)))


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
    state = pcg64_words(np.random.default_rng(0).bit_generator)
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for S in slot_list:
            em.recommend_begin(np.arange(1.0, R + 1), True)
            for s in range(S):
                em.select(s).recommend_add()
            seen, same, list_probability = check(em, rng, users, state)
            all_lists = lists_of(*[em.recommend_query_explore(users, TOP, TEMPERATURE, state)[j] for j in (0, 3)])[0]
            one_lists = lists_of(*[em.recommend_query_explore(one, TOP, TEMPERATURE, state)[j] for j in (0, 3)])[0]

            def timed(call):
                t0 = time.perf_counter()
                call()
                return em.get_option("recommend_ms"), (time.perf_counter() - t0) * 1e3

            calls = {"query_explore_all": lambda: em.recommend_query_explore(users, TOP, TEMPERATURE, state),
                     "list_propensity_all": lambda: em.recommend_list_propensity(users, all_lists, TEMPERATURE),
                     "recommend_query_all": lambda: em.recommend_query(users, TOP),
                     "query_explore_one": lambda: em.recommend_query_explore(one, TOP, TEMPERATURE, state),
                     "list_propensity_one": lambda: em.recommend_list_propensity(one, one_lists, TEMPERATURE),
                     "recommend_query_one": lambda: em.recommend_query(one, TOP)}
            dev = {k: [] for k in calls}
            host = {k: [] for k in calls}
            for rep in range(args.reps + 1):                       # rep 0: the warm-up of each
                for k, call in calls.items():                      # alternating
                    d, h = timed(call)
                    if rep:
                        dev[k].append(d)
                        host[k].append(h)
            out = {"build_id": _lib.build_id(), "users": U, "items": I, "rank": min(K, L), "restarts": S, "reps": args.reps,
                   "n": TOP, "temperature": TEMPERATURE,
                   "device_ms": {k: round(float(np.median(v)), 3) for k, v in dev.items()},
                   "device_ms_min_max": {k: [round(float(min(v)), 3), round(float(max(v)), 3)] for k, v in dev.items()},
                   "host_ms": {k: round(float(np.median(v)), 3) for k, v in host.items()},
                   "scores_compared": seen, "answers_equal": same, "median_list_probability": list_probability}
            print(json.dumps(out), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
