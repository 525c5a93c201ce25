"""The most informative items (HipEM.inform_*): device times at BASELINE C3's shape next to the all-user
recommend_query(n = 10) of the same process.

    python scripts/inform_time.py [--reps 5] [--slots 1,8]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters).  Per S, IN ONE
PROCESS and ALTERNATING, --reps times after one warm-up of each, n = 10:
    interview    inform_query_theta of the one row theta-bar (inform_mean_theta), every item a candidate;
    ask_next     what MMSBM.ask_next does for 1,000 new users with 3 ratings each once the session stands: the shrinkage
                 (prior 1) on the host and inform_query_theta of the 1,000 rows without their rated items; the slots'
                 fold-ins (100 iterations) are timed once, beside it ("fold_in_ms", summed over the slots);
    inform_all   inform_query for all users, training items excluded;
    recommend_all  recommend_query(n = 10) for all users, training items excluded.
Each figure is the median of the device times (HIP events around each call's kernels: options "inform_ms" /
"recommend_ms"); the host time of the call, with its copies, is printed beside it.
answers_equal: for 200 sampled users inform_query_theta of the slots' own theta rows, with their training items as the
seen lists, against inform_query -- items and gain bits; and every one of those gains within [0, log min(K, R)].
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
NEW_USERS, NEW_RATINGS, FOLD_ITERATIONS, PRIOR = 1000, 3, 100, 1.0
TOP = 10


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def check(em, rng, data, params, users, n_users=200):
    """(rows compared, rows equal)"""
    ask = users[np.sort(rng.choice(len(users), n_users, replace=False))]
    mine = [np.unique(data[data[:, 0] == u, 1]) for u in ask.tolist()]
    seen = (np.concatenate([[0], np.cumsum([len(x) for x in mine])]).astype(np.int64), np.concatenate(mine).astype(np.int32))
    qi, qg, qc = em.inform_query(ask, TOP)
    ti, tg, tc = em.inform_query_theta(np.stack([p[0][ask] for p in params]), TOP, seen)
    top = np.log(min(K, R)) * (1 + 1e-12)
    same = 0
    for b in range(n_users):
        ok = np.array_equal(qi[b], ti[b]) and np.array_equal(qg[b].view(np.uint64), tg[b].view(np.uint64)) and qc[b] == tc[b]
        same += int(ok and (qg[b, :qc[b]] >= 0).all() and (qg[b, :qc[b]] <= top).all())
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
    new_rows = np.stack([np.repeat(np.arange(NEW_USERS), NEW_RATINGS), rng.integers(0, I, NEW_USERS * NEW_RATINGS),
                         rng.integers(0, R, NEW_USERS * NEW_RATINGS)], 1).astype(np.int32)
    order = np.lexsort((new_rows[:, 1], new_rows[:, 0]))
    new_seen = (np.arange(0, NEW_USERS * NEW_RATINGS + 1, NEW_RATINGS, dtype=np.int64), new_rows[order, 1].astype(np.int32))
    d = np.full((1, NEW_USERS, 1), float(NEW_RATINGS))
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for S in slot_list:
            em.recommend_begin(np.arange(1.0, R + 1), True)
            em.inform_begin()
            folds, fold_ms = [], 0.0
            for s in range(S):
                em.select(s).recommend_add()
                em.inform_add()
                folds.append(em.fold_in(new_rows, NEW_USERS, FOLD_ITERATIONS)[0])
                fold_ms += em.get_option("fold_in_ms")
            folds = np.stack(folds)
            seen, same = check(em, rng, data, params[:S], users)

            def timed(call, option):
                t0 = time.perf_counter()
                call()
                return em.get_option(option), (time.perf_counter() - t0) * 1e3

            def ask_next():
                theta = (d * folds + PRIOR * em.inform_mean_theta()[:, None, :]) / (d + PRIOR)
                return em.inform_query_theta(theta, TOP, new_seen)

            calls = {"interview": (lambda: em.inform_query_theta(em.inform_mean_theta()[:, None, :], TOP), "inform_ms"),
                     "ask_next": (ask_next, "inform_ms"),
                     "inform_all": (lambda: em.inform_query(users, TOP), "inform_ms"),
                     "recommend_all": (lambda: em.recommend_query(users, TOP), "recommend_ms")}
            dev = {k: [] for k in calls}
            host = {k: [] for k in calls}
            for rep in range(args.reps + 1):                       # rep 0: the warm-up of each
                for k, (call, option) in calls.items():            # alternating
                    dv, h = timed(call, option)
                    if rep:
                        dev[k].append(dv)
                        host[k].append(h)
            out = {"build_id": _lib.build_id(), "users": U, "items": I, "profile_width": K * R, "restarts": S,
                   "reps": args.reps, "n": TOP, "new_users": NEW_USERS, "ratings_per_new_user": NEW_RATINGS,
                   "fold_in_ms": round(float(fold_ms), 3),
                   "device_ms": {k: round(float(np.median(v)), 3) for k, v in dev.items()},
                   "host_ms": {k: round(float(np.median(v)), 3) for k, v in host.items()},
                   "rows_compared": seen, "answers_equal": bool(seen > 0 and same == seen)}
            print(json.dumps(out), flush=True)
            em.inform_end()
            em.recommend_end()


if __name__ == "__main__":
    main()
