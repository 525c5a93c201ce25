"""Greedy assortment selection (HipEM.recommend_assortment): device times at BASELINE C3's shape next to the group pass
over the same rows and to recommend_query.

    python scripts/assortment_time.py [--reps 5] [--slots 1,8] [--rounds 10,100]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded.  Cases: c = 10 and c = 100; both objectives (the floor at min(weights), the reach bar at the 99th percentile
of a sampled score set); all users and a segment of 1,000; the whole catalogue and candidates = 10 % of it.  Per S and
case, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each:
    recommend_query_groups(one group of the same users, "max", n = 10)   -- one pass of the same score tiles with a
                                                                            column reduction: the yardstick of a ROUND --
    recommend_query(the same users, n = 10)
    recommend_assortment(c rounds)
Each figure is the median of the device times (HIP events around each call's kernels: options "assortment_ms" /
"group_ms" / "recommend_ms").  ms_per_round = assortment_ms / rounds run; round_vs_group = ms_per_round / group_ms.
split: one more call with option "assortment_timing" set (events between the phases of every round) -- the device time
of the gain + join, the pick and the update kernels, summed over the rounds.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from mmsbm_amd import HipEM, _lib  # noqa: E402
from mmsbm_amd.synthetic import synthetic_triples  # noqa: E402

N_OBS, USERS, ITEMS, R, K, L = 1_000_000, 100_000, 20_000, 5, 20, 20
TOP = 10


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", default="1,8")
    ap.add_argument("--rounds", default="10,100")
    args = ap.parse_args()
    slot_list = [int(x) for x in args.slots.split(",")]
    round_list = [int(x) for x in args.rounds.split(",")]
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    S_max = max(slot_list)
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S_max)]
    w = np.arange(1.0, R + 1)
    requests = {"all_users": np.arange(U, dtype=np.int32),
                "segment_1000": np.sort(rng.choice(U, 1000, replace=False)).astype(np.int32)}
    catalogues = {"whole": None, "tenth": np.sort(rng.choice(I, I // 10, replace=False)).astype(np.int32)}
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for S in slot_list:
            em.recommend_begin(w, True)
            for s in range(S):
                em.select(s).recommend_add()
            # the 99th percentile of the scores of 500 users x 1,000 items drawn at random
            probe = np.sort(rng.choice(I, 1000, replace=False)).astype(np.int32)
            sample = em.recommend_query_within(rng.choice(U, 500, replace=False).astype(np.int32), 1000, probe)[1]
            bar = float(np.quantile(sample[np.isfinite(sample)], 0.99))
            for uname, users in requests.items():
                off = np.array([0, len(users)], dtype=np.int64)
                for cname, cand in catalogues.items():
                    for objective, level in (("best_score", float(w.min())), ("reach", bar)):
                        for c in round_list:
                            dev = {"group": [], "recommend": [], "assortment": []}
                            rounds = stop = None
                            for rep in range(args.reps + 1):           # rep 0: the warm-up of each
                                em.recommend_query_groups(off, users, TOP, "max", 0.0, cand)
                                ms = {"group": em.get_option("group_ms")}
                                if cand is None:
                                    em.recommend_query(users, TOP)
                                else:
                                    em.recommend_query_within(users, TOP, cand)
                                ms["recommend"] = em.get_option("recommend_ms")
                                got = em.recommend_assortment(users, c, objective, level, None, cand)
                                ms["assortment"] = em.get_option("assortment_ms")
                                rounds, stop = got[2], got[3]
                                if rep:
                                    for k, v in ms.items():
                                        dev[k].append(v)
                            em.set_option("assortment_timing", 1)
                            em.recommend_assortment(users, c, objective, level, None, cand)
                            split = {k: round(em.get_option(f"assortment_{k}_ms"), 3) for k in ("gain", "pick", "update")}
                            em.set_option("assortment_timing", 0)
                            med = {k: float(np.median(v)) for k, v in dev.items()}
                            ran = rounds + (1 if stop != "c" else 0)   # (the round that found nothing ran too)
                            per_round = med["assortment"] / max(ran, 1)
                            print(json.dumps({
                                "build_id": _lib.build_id(), "users": len(users), "items": I if cand is None else len(cand),
                                "rank": min(K, L), "restarts": S, "reps": args.reps, "request": uname, "catalogue": cname,
                                "objective": objective, "level": level, "c": c, "rounds": int(rounds), "stopped": stop,
                                "assortment_ms": round(med["assortment"], 3), "ms_per_round": round(per_round, 3),
                                "group_ms": round(med["group"], 3), "recommend_ms": round(med["recommend"], 3),
                                "round_vs_group": round(per_round / med["group"], 3), "split_ms": split}), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
