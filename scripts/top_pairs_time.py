"""The m best pairs of the whole model (HipEM.recommend_top_pairs): device time at BASELINE C3's shape next to the only
exact way to get the same answer from the existing query -- recommend_query(all users, n = m), whose rows the host
would still have to sort (that sort is left out, in the yardstick's favour).

    python scripts/top_pairs_time.py [--reps 5] [--ms 10,100,1000] [--slots 1,8] [--groups 0]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded.  Per (S, m) both queries run IN THE SAME PROCESS, ALTERNATING, --reps times after one warm-up of each; the
figures are medians of the device times (HIP events around each query's kernels: options "top_pairs_ms" and
"recommend_ms").  Also one user against all items.  Printed per row: pairs/s, FLOP/s = 2 x rank x S x pairs / time and
its share of 78.6 TFLOP/s (fp64 vector, the figure DESIGN 7d uses), and whether the two answers agree (they must:
same ids, same score bits).  The split fused kernel / merge comes from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python scripts/top_pairs_time.py --reps 1 --ms 1000 --slots 1).
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
PEAK_FP64 = 78.6e12


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def merged(users, items, scores, counts, m):
    """The first m of recommend_query's rows in the global order (host sort: NOT part of any time reported)."""
    keep = np.arange(m)[None, :] < counts[:, None]
    u, i, s = np.repeat(users.astype(np.int64), counts), items[keep].astype(np.int64), scores[keep]
    order = np.lexsort((i, u, -s))[:m]
    return u[order], i[order], s[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ms", default="10,100,1000")
    ap.add_argument("--slots", default="1,8")
    ap.add_argument("--groups", type=int, default=0, help="option top_pairs_groups (0: the library's choice)")
    args = ap.parse_args()
    ms_list = [int(x) for x in args.ms.split(",")]
    slot_list = [int(x) for x in args.slots.split(",")]
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    S_max = max(slot_list)
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S_max)]
    users = np.arange(U, dtype=np.int32)
    rank = min(K, L)
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        em.set_option("top_pairs_groups", args.groups)
        for S in slot_list:
            em.recommend_begin(np.arange(1.0, R + 1), True)
            for s in range(S):
                em.select(s).recommend_add()
            for m in ms_list:
                got = em.recommend_top_pairs(m)                      # warm-up of each
                ref = em.recommend_query(users, m)
                ru, ri, rs = merged(users, *ref, m)
                same = (got[3] == len(ru) and np.array_equal(got[0][:got[3]], ru) and np.array_equal(got[1][:got[3]], ri)
                        and np.array_equal(got[2][:got[3]].view(np.uint64), rs.view(np.uint64)))
                del ref
                new, old, host = [], [], []
                for _ in range(args.reps):                           # alternating
                    t0 = time.perf_counter()
                    em.recommend_top_pairs(m)
                    host.append((time.perf_counter() - t0) * 1e3)
                    new.append(em.get_option("top_pairs_ms"))
                    em.recommend_query(users, m)
                    old.append(em.get_option("recommend_ms"))
                t_new, t_old = float(np.median(new)), float(np.median(old))
                pairs = float(U) * I
                flops = 2.0 * rank * S * pairs / (t_new / 1e3)
                print(json.dumps({
                    "case": "all_users", "build_id": _lib.build_id(), "users": U, "items": I, "rank": rank, "restarts": S,
                    "m": m, "groups": args.groups, "top_pairs_ms": round(t_new, 3), "recommend_query_ms": round(t_old, 3),
                    "ratio": round(t_old / t_new, 2), "top_pairs_times_ms": [round(x, 3) for x in new],
                    "recommend_times_ms": [round(x, 3) for x in old], "host_call_ms": round(float(np.median(host)), 3),
                    "pairs_per_s": round(pairs / (t_new / 1e3), 0), "tflops": round(flops / 1e12, 3),
                    "share_of_fp64_peak": round(flops / PEAK_FP64, 4), "answers_equal": bool(same)}), flush=True)
            # one user against all items
            one_new, one_old = [], []
            for u in rng.choice(U, 11, replace=False).tolist():
                em.recommend_top_pairs(10, [u])
                one_new.append(em.get_option("top_pairs_ms"))
                em.recommend_query([u], 10)
                one_old.append(em.get_option("recommend_ms"))
            print(json.dumps({"case": "one_user", "build_id": _lib.build_id(), "items": I, "restarts": S, "m": 10,
                              "top_pairs_ms": round(float(np.median(one_new)), 4),
                              "recommend_query_ms": round(float(np.median(one_old)), 4)}), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
