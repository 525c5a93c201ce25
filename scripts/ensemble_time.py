"""Ensemble-aware recommendation (HipEM.recommend_query_ensemble / recommend_pair_spread): device times at BASELINE C3's
shape next to recommend_query.

    python scripts/ensemble_time.py [--reps 5] [--slots 1,8]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded, n = 10.  Per S, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each:
    recommend_query(all users, n = 10)                              -- the mean over the restarts, one chain across them
    recommend_query_ensemble(all users, n = 10) in each mode (min, max, lcb at risk 1)
    recommend_query_ensemble(one user, n = 10) in each mode
    recommend_pair_spread(every user's top-10 list of recommend_query)
Each figure is the median of the device times (HIP events around each call's kernels: options "ensemble_ms" /
"recommend_ms"); recommend_spread is the smallest and the largest of the repeated recommend_query runs; ratio =
ensemble / recommend over all users.  answers_equal (S = 1 only, where it must hold): every mode against recommend_query,
items, counts and score bits.
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
MODES = ("min", "max", "lcb")
RISK = 1.0


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def same_bits(got, want):
    return all(np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                              w.view(np.uint64) if w.dtype == np.float64 else w) for g, w in zip(got, want))


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
    everyone, one = np.arange(U, dtype=np.int32), np.array([U // 2], dtype=np.int32)
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for S in slot_list:
            em.recommend_begin(np.arange(1.0, R + 1), True)
            for s in range(S):
                em.select(s).recommend_add()
            want = em.recommend_query(everyone, TOP)
            equal = None
            if S == 1:
                equal = all(same_bits(em.recommend_query_ensemble(everyone, TOP, mode, RISK), want) for mode in MODES)
            keep = np.arange(TOP)[None, :] < want[2][:, None]
            pair_users, pair_items = np.repeat(everyone, want[2]), want[0][keep]
            dev = {k: [] for k in ("recommend", "pair_spread") + tuple(f"{m}_{w}" for m in MODES for w in ("all", "one"))}
            for rep in range(args.reps + 1):                       # rep 0: the warm-up of each
                em.recommend_query(everyone, TOP)                  # alternating
                ms = {"recommend": em.get_option("recommend_ms")}
                for mode in MODES:
                    for who, users in (("all", everyone), ("one", one)):
                        em.recommend_query_ensemble(users, TOP, mode, RISK)
                        ms[f"{mode}_{who}"] = em.get_option("ensemble_ms")
                em.recommend_pair_spread(pair_users, pair_items)
                ms["pair_spread"] = em.get_option("ensemble_ms")
                if rep:
                    for k, v in ms.items():
                        dev[k].append(v)
            med = {k: float(np.median(v)) for k, v in dev.items()}
            out = {"build_id": _lib.build_id(), "users": U, "items": I, "rank": min(K, L), "restarts": S, "reps": args.reps,
                   "n": TOP, "risk": RISK, "recommend_ms": round(med["recommend"], 3),
                   "recommend_spread": [round(min(dev["recommend"]), 3), round(max(dev["recommend"]), 3)],
                   "ensemble_all_users_ms": {m: round(med[f"{m}_all"], 3) for m in MODES},
                   "ensemble_one_user_ms": {m: round(med[f"{m}_one"], 3) for m in MODES},
                   "ratio": {m: round(med[f"{m}_all"] / med["recommend"], 3) for m in MODES},
                   "pair_spread_pairs": int(len(pair_users)), "pair_spread_ms": round(med["pair_spread"], 3),
                   "answers_equal": equal}
            print(json.dumps(out), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
