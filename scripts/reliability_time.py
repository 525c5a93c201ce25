"""Leave-one-out reliability of the training rows (HipEM.loo_*): device times at BASELINE C3's shape next to the two
ways the library already had of touching every training row once.

    python scripts/reliability_time.py [--reps 5] [--slots 1,8]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters).  Per S, in a context
of S slots, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each:
    loo      begin; loo_add of every slot (per slot: "loo_sums_ms" -- the mean rows, fit, both sides' chunk sums and
             their combination -- and "loo_rows_ms", the row pass); loo_sides (the finish: "loo_ms"); loo_lowest(100)
             ("loo_ms"); end;
    heldout  heldout_begin(the training rows); heldout_add of every slot ("heldout_ms" each); heldout_mean (host time):
             how the `fitted` column could be reached before;
    em       one EM iteration of the S slots (time_iterations(2) / 2), also divided by S.
Each figure is the median over the repetitions (per-slot figures: over repetitions and slots) of the device times
(HIP events around each call's kernels); host times of whole calls are marked host_ms.
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
LOWEST = 100


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", default="1,8")
    args = ap.parse_args()
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    for S in (int(x) for x in args.slots.split(",")):
        params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S)]
        with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S) as em:
            got = {k: [] for k in ("loo_sums", "loo_rows", "loo_add", "loo_finish", "loo_lowest", "loo_session_host",
                                   "heldout_add", "heldout_mean_host", "em_iteration")}
            for rep in range(args.reps + 1):                       # rep 0: the warm-up of each
                keep = rep > 0
                for s, p in enumerate(params):                     # (the iterations below move the parameters)
                    em.select(s).set_params(*p)
                t0 = time.perf_counter()
                em.loo_begin()
                for s in range(S):
                    em.select(s).loo_add()
                    if keep:
                        got["loo_add"].append(em.get_option("loo_ms"))
                        got["loo_sums"].append(em.get_option("loo_sums_ms"))
                        got["loo_rows"].append(em.get_option("loo_rows_ms"))
                em.loo_sides()
                finish = em.get_option("loo_ms")
                rows, rel, count = em.loo_lowest(LOWEST)
                lowest = em.get_option("loo_ms")
                em.loo_end()
                session = (time.perf_counter() - t0) * 1e3
                assert count == LOWEST and (np.diff(rel) >= 0).all()
                em.heldout_begin(data)
                adds = []
                for s in range(S):
                    em.select(s).heldout_add()
                    adds.append(em.get_option("heldout_ms"))
                t0 = time.perf_counter()
                em.heldout_mean()
                mean_host = (time.perf_counter() - t0) * 1e3
                em.heldout_end()
                it = em.time_iterations(2) / 2
                if keep:
                    got["loo_finish"].append(finish)
                    got["loo_lowest"].append(lowest)
                    got["loo_session_host"].append(session)
                    got["heldout_add"] += adds
                    got["heldout_mean_host"].append(mean_host)
                    got["em_iteration"].append(it)
            med = {k: float(np.median(v)) for k, v in got.items()}
            out = {"config": "C3", "ratings": N_OBS, "users": U, "items": I, "K": K, "L": L, "slots": S, "reps": args.reps,
                   "per_slot_ms": {"loo_sums": round(med["loo_sums"], 3), "loo_rows": round(med["loo_rows"], 3),
                                   "loo_add": round(med["loo_add"], 3), "heldout_add": round(med["heldout_add"], 3),
                                   "em_iteration": round(med["em_iteration"] / S, 4)},
                   "loo_finish_ms": round(med["loo_finish"], 3), "loo_lowest_ms": round(med["loo_lowest"], 3),
                   "em_iteration_all_slots_ms": round(med["em_iteration"], 4),
                   "loo_session_host_ms": round(med["loo_session_host"], 1),
                   "heldout_mean_host_ms": round(med["heldout_mean_host"], 2),
                   "loo_add_over_em_iteration": round(med["loo_add"] / (med["em_iteration"] / S), 2)}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
