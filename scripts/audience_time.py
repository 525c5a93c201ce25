"""Item-side serving (HipEM.recommend_query_items / recommend_audience): device times at BASELINE C3's shape next to
the user-side queries of the same session.

    python scripts/audience_time.py [--reps 5] [--slots 1,8]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded.  Per S, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each:
    recommend_query_items(all items, n = 10), recommend_query_items(one item, n = 1000),
    recommend_audience(all items) sizes-only and filled at three bars -- the 99.9th, 99th and 90th percentile of a
    sampled score set (every user's score for 20 random items) --
    recommend_query(all users, n = 10) and recommend_top_pairs(m = 1000).
Each figure is the median of the device times (HIP events around each call's kernels: options "recommend_ms",
"audience_ms", "top_pairs_ms").  The filled audience figure is ONE C call (its own COUNT pass and the WRITE pass); its
host time, with the copies of the entries, is printed beside it.  answers_equal: the audience's (user, item, score) at
the highest bar, sampled, against recommend_query of those users -- same score bits wherever the item is among the
user's 1,024 best.
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
PERCENTILES = (99.9, 99.0, 90.0)


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def check_against_user_side(em, rng, items, bar, n_pairs=300):
    """(pairs compared, pairs with the same score bits) of a sample of the audience at `bar`."""
    ask = rng.choice(items, 50, replace=False).astype(np.int32)
    off, us, sc = em.recommend_audience(ask, bar)
    if off[-1] == 0:
        return 0, 0
    at = np.repeat(ask, np.diff(off))
    pick = rng.choice(len(us), min(n_pairs, len(us)), replace=False)
    users = np.unique(us[pick])
    ri, rs, rc = em.recommend_query(users, 1024)
    row = {int(u): b for b, u in enumerate(users.tolist())}
    seen = same = 0
    for e in pick.tolist():
        b = row[int(us[e])]
        hit = np.flatnonzero(ri[b, :rc[b]] == at[e])
        if len(hit):
            seen += 1
            same += int(np.float64(rs[b, hit[0]]).view(np.uint64) == np.float64(sc[e]).view(np.uint64))
    return seen, same


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
    users, items = np.arange(U, dtype=np.int32), np.arange(I, dtype=np.int32)
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for S in slot_list:
            em.recommend_begin(np.arange(1.0, R + 1), True)
            for s in range(S):
                em.select(s).recommend_add()
            sample = em.recommend_audience(rng.choice(I, 20, replace=False).astype(np.int32), -1e300)[2]
            bars = [float(np.percentile(sample, q)) for q in PERCENTILES]
            one = [int(rng.integers(0, I))]
            totals = [int(em.recommend_audience(items, b, count_only=True)[0][-1]) for b in bars]   # (warm-up too)
            seen, same = check_against_user_side(em, rng, items, bars[0])

            def timed(call, option):
                t0 = time.perf_counter()
                call()
                return em.get_option(option), (time.perf_counter() - t0) * 1e3

            calls = {"query_items_all_n10": (lambda: em.recommend_query_items(items, 10), "recommend_ms"),
                     "query_items_one_n1000": (lambda: em.recommend_query_items(one, 1000), "recommend_ms"),
                     "recommend_query_all_n10": (lambda: em.recommend_query(users, 10), "recommend_ms"),
                     "top_pairs_m1000": (lambda: em.recommend_top_pairs(1000), "top_pairs_ms")}
            for q, b, t in zip(PERCENTILES, bars, totals):
                calls[f"audience_sizes_p{q}"] = (lambda b=b: em.recommend_audience(items, b, count_only=True), "audience_ms")
                calls[f"audience_filled_p{q}"] = (lambda b=b, t=t: em.recommend_audience(items, b, total=t), "audience_ms")
            dev = {k: [] for k in calls}
            host = {k: [] for k in calls}
            for rep in range(args.reps + 1):                       # rep 0: the warm-up of each
                for k, (call, option) in calls.items():          # alternating
                    d, h = timed(call, option)
                    if rep:
                        dev[k].append(d)
                        host[k].append(h)
            out = {"build_id": _lib.build_id(), "users": U, "items": I, "rank": min(K, L), "restarts": S, "reps": args.reps,
                   "bars": dict(zip((f"p{q}" for q in PERCENTILES), bars)),
                   "entries": dict(zip((f"p{q}" for q in PERCENTILES), totals)),
                   "device_ms": {k: round(float(np.median(v)), 3) for k, v in dev.items()},
                   "host_ms": {k: round(float(np.median(v)), 3) for k, v in host.items()},
                   "pairs_compared": seen, "answers_equal": bool(seen > 0 and same == seen)}
            print(json.dumps(out), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
