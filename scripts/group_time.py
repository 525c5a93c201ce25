"""Group recommendation (HipEM.recommend_query_groups): device times at BASELINE C3's shape next to recommend_query over
the same member rows.

    python scripts/group_time.py [--reps 5] [--slots 1,8]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded, n = 10.  Cases: 10,000 groups of 4, 700 groups of 128, one group of all users; members drawn without repeats
within a group.  Per S and case, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each:
    recommend_query(the request's member rows, n = 10)   -- the same score tiles, with the members x items buffer --
    recommend_query_groups in each mode (min, max, count at the median of a sampled score set, mean).
Each figure is the median of the device times (HIP events around each call's kernels: options "group_ms" /
"recommend_ms"); recommend_spread is the smallest and the largest of the repeated recommend_query runs, the yardstick
for "no longer than"; ratio = group / recommend.  The one group of all users is reported alone as well: at a larger U
its recommend_query counterpart would not be asked for.  answers_equal: groups of one against recommend_query, by bits.
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
MODES = ("min", "max", "count", "mean")


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def groups_of(rng, U, count, size):
    """(offsets, members): `count` groups of `size` users, distinct within a group."""
    if size == U:
        members = rng.permutation(U)
    else:
        members = np.concatenate([rng.choice(U, size, replace=False) for _ in range(count)])
    return np.arange(count + 1, dtype=np.int64) * size, members.astype(np.int32)


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
    cases = {"10000_groups_of_4": groups_of(rng, U, 10_000, 4), "700_groups_of_128": groups_of(rng, U, 700, 128),
             "one_group_of_all_users": groups_of(rng, U, 1, U)}
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for S in slot_list:
            em.recommend_begin(np.arange(1.0, R + 1), True)
            for s in range(S):
                em.select(s).recommend_add()
            ones = rng.choice(U, 500, replace=False).astype(np.int32)
            want = em.recommend_query(ones, TOP)
            sample = want[1][np.isfinite(want[1])]
            bar = float(np.median(sample))
            equal = all(np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                                       w.view(np.uint64) if w.dtype == np.float64 else w)
                        for mode in ("min", "max", "mean")
                        for g, w in zip(em.recommend_query_groups(np.arange(501, dtype=np.int64), ones, TOP, mode), want))
            for name, (off, mem) in cases.items():
                dev = {k: [] for k in ("recommend",) + MODES}
                for rep in range(args.reps + 1):                   # rep 0: the warm-up of each
                    em.recommend_query(mem, TOP)                   # alternating
                    ms = {"recommend": em.get_option("recommend_ms")}
                    for mode in MODES:
                        em.recommend_query_groups(off, mem, TOP, mode, bar)
                        ms[mode] = em.get_option("group_ms")
                    if rep:
                        for k, v in ms.items():
                            dev[k].append(v)
                med = {k: float(np.median(v)) for k, v in dev.items()}
                out = {"build_id": _lib.build_id(), "users": U, "items": I, "rank": min(K, L), "restarts": S,
                       "reps": args.reps, "case": name, "groups": len(off) - 1, "member_rows": len(mem), "n": TOP, "bar": bar,
                       "recommend_ms": round(med["recommend"], 3),
                       "recommend_spread": [round(min(dev["recommend"]), 3), round(max(dev["recommend"]), 3)],
                       "group_ms": {m: round(med[m], 3) for m in MODES},
                       "ratio": {m: round(med[m] / med["recommend"], 3) for m in MODES},
                       "answers_equal": bool(equal)}
                print(json.dumps(out), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
