"""Welfare-maximising assignment (HipEM.recommend_assign): rounds, bids and device times at BASELINE C3's shape next to
the stable walk under the same caps and the plain query.

    python scripts/assign_time.py [--slots 1,8] [--caps 5,50,1000] [--eps 0.1,0.01] [--max-rounds 10000] [--reps 3]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded, all users, the same cap on every item, the default reserve (below every score).  Per S and cap, IN ONE PROCESS:
    recommend_query(all users, n = 1), recommend_query(all users, n = 2) and recommend_allocate(all users, n = 1, caps),
        alternating, the queries --reps times after one warm-up of each (the median of "recommend_ms"), the walk once
        ("allocate_ms", its rounds, its total score);
    then per epsilon recommend_assign(all users, caps): rounds, bids, converged, the device time of the whole call
        (option "assign_ms": the host's one read per round included) and per round, the host time, the users assigned,
        the total score, the bound, and the mean active rows of a round.  The expectation this reports and does not
        assert: a round with b active rows costs about b / U of the all-user query(n = 2), plus a floor of launch
        latencies -- "round_model_ms" is that share, "round_floor_ms" what is left of the measured round.
One JSON line per (S, cap, epsilon), printed as soon as it is measured.
"""
import argparse
import json
import math
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
    ap.add_argument("--caps", default="5,50,1000")
    ap.add_argument("--eps", default="0.1,0.01")
    ap.add_argument("--max-rounds", type=int, default=10000)
    args = ap.parse_args()
    slot_list = [int(x) for x in args.slots.split(",")]
    cap_list = [int(x) for x in args.caps.split(",")]
    eps_list = [float(x) for x in args.eps.split(",")]
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    S_max = max(slot_list)
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S_max)]
    users = np.arange(U, dtype=np.int32)
    w = np.arange(1.0, R + 1)
    reserve = float(w.min() - (w.max() - w.min()))
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, prm in enumerate(params):
            em.select(s).set_params(*prm)
        for S in slot_list:
            em.recommend_begin(w, True)
            for s in range(S):
                em.select(s).recommend_add()
            for cap in cap_list:
                caps = np.full(I, cap, dtype=np.int32)
                ms = {1: [], 2: []}
                walk = None
                for rep in range(args.reps + 1):                      # rep 0: the warm-up of each
                    for n in (1, 2):                                  # alternating
                        em.recommend_query(users, n)
                        if rep:
                            ms[n].append(em.get_option("recommend_ms"))
                    if rep == 1:
                        _, wscores, wcounts, winfo = em.recommend_allocate(users, 1, caps, args.max_rounds)
                        walk = {"allocate_ms": round(em.get_option("allocate_ms"), 2), "allocate_rounds": winfo["rounds"],
                                "allocate_total": math.fsum(wscores[wcounts > 0, 0].tolist()),
                                "allocate_filled": int(wcounts.sum())}
                q1, q2 = float(np.median(ms[1])), float(np.median(ms[2]))
                for eps in eps_list:
                    t0 = time.perf_counter()
                    got = em.recommend_assign(users, caps, reserve, eps, args.max_rounds)
                    host = (time.perf_counter() - t0) * 1e3
                    total_ms = em.get_option("assign_ms")
                    has = got["items"] >= 0
                    rounds = max(got["rounds"], 1)
                    active = (got["bids"] + int((~has).sum()) if got["converged"] else got["bids"]) / rounds
                    per_round = (total_ms - q1) / rounds              # (the certificate pass is one query(n = 1))
                    model = active / U * q2
                    print(json.dumps({
                        "build_id": _lib.build_id(), "users": U, "items": I, "restarts": S, "cap": cap, "epsilon": eps,
                        "rounds": got["rounds"], "bids": got["bids"], "converged": got["converged"],
                        "assign_ms": round(total_ms, 2), "ms_per_round": round(per_round, 4), "host_ms": round(host, 2),
                        "mean_active_rows": round(active, 1), "query_n1_ms": round(q1, 3), "query_n2_ms": round(q2, 3),
                        "round_model_ms": round(model, 4), "round_floor_ms": round(per_round - model, 4),
                        "assigned": int(has.sum()), "total": math.fsum(got["scores"][has].tolist()),
                        "bound": math.fsum(got["pi"].tolist() + got["price_sum"].tolist()),
                        "gap_limit": int(has.sum()) * eps, "largest_price": float(got["price"].max()), **walk}), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
