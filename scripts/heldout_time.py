"""The held-out log-likelihood as a monitor (HipEM.heldout_eval): device time of ONE evaluation of every slot next to the
device time of one EM iteration of the same context, and the wall clock of a monitored fit against the plain one.

    python scripts/heldout_time.py [--configs c3,c5] [--slots 1,8] [--reps 9] [--fit-iterations 200] [--no-fit]

Per config (BASELINE C3: 1M ratings, K = L = 20; C5: 10M ratings, K = L = 50) the synthetic triples are split 90 / 10
by a seeded permutation: the context is created over the 90 %, the session over the 10 % whose users and items occur in
it.  Per slot count S (every slot a random start advanced by a few iterations): `heldout_eval` --reps times after a
warm-up, median of the device times (option "heldout_ms": HIP events around the two launches), and
mmsbm_hip_time_iterations over 20 iterations of the same context / 20.  The expectation of DESIGN 7j: a check gathers
2 M rows where an iteration gathers at least 2 N, so at M = N / 10 a check should cost no more than one iteration.
The fit: MMSBM on C3's 90 %, sampling = S restarts in one batch, check_every = 50 -- plain, then with validation = the
10 % -- host wall clock of fit_encoded after a warm-up fit of 10 iterations.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from mmsbm_amd import MMSBM, HipEM, _lib  # noqa: E402
from mmsbm_amd.synthetic import CONFIGS, synthetic_triples  # noqa: E402


def split(config, seed=0):
    """(train, held): 90 / 10 of the config's triples, the held rows restricted to training users, items and ratings,
    every id column of the training part dense."""
    n, u, i, r, k, l = CONFIGS[config]
    data = synthetic_triples(n, u, i, r, seed=seed)
    order = np.random.default_rng(seed + 1).permutation(len(data))
    cut = len(data) // 10
    held, train = data[order[:cut]], data[order[cut:]]
    cols = []
    keep = np.ones(len(held), dtype=bool)
    for j in range(3):
        ids, inv = np.unique(train[:, j], return_inverse=True)
        cols.append(inv)
        at = np.searchsorted(ids, held[:, j])
        at[at == len(ids)] = 0
        keep &= ids[at] == held[:, j]
        held[:, j] = at
    return np.stack(cols, 1).astype(np.int64), held[keep].astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c5")
    ap.add_argument("--slots", default="1,8")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--fit-iterations", type=int, default=200)
    ap.add_argument("--no-fit", action="store_true")
    args = ap.parse_args()
    slot_list = [int(x) for x in args.slots.split(",")]
    print(f"build {_lib.build_id()}", flush=True)
    for config in args.configs.split(","):
        k, l = CONFIGS[config][4:6]
        train, held = split(config)
        U, I, R = (int(train[:, j].max()) + 1 for j in range(3))
        for S in slot_list:
            with HipEM(train, k, l, n_users=U, n_items=I, n_ratings=R, slots=S) as em:
                for s in range(S):
                    em.select(s).init_params(np.random.SeedSequence(s))
                em.iterate(3)
                iter_ms = em.time_iterations(20) / 20
                em.heldout_begin(held)
                em.heldout_eval()
                times, host = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    values = em.heldout_eval()
                    host.append((time.perf_counter() - t0) * 1e3)
                    times.append(em.get_option("heldout_ms"))
                em.heldout_end()
                iter_again = em.time_iterations(20) / 20
                ev = float(np.median(times))
                print(json.dumps({
                    "case": "eval", "build_id": _lib.build_id(), "config": config, "train_rows": len(train),
                    "held_rows": len(held), "restarts": S, "launches": em.get_option("launches"),
                    "heldout_eval_ms": round(ev, 4), "heldout_times_ms": [round(x, 4) for x in times],
                    "host_call_ms": round(float(np.median(host)), 4), "iteration_ms": round(iter_ms, 4),
                    "iteration_again_ms": round(iter_again, 4), "eval_over_iteration": round(ev / iter_ms, 3),
                    "loglik_per_row": round(float(values[0]) / max(len(held), 1), 6)}), flush=True)
        if config == "c3" and not args.no_fit:
            for S in slot_list:
                walls = {}
                for name, val in (("warm-up", None), ("plain", None), ("monitored", held), ("plain again", None)):
                    its = 10 if name == "warm-up" else args.fit_iterations
                    m = MMSBM(k, l, iterations=its, sampling=S, seed=3, restarts_per_launch=S, check_every=50)
                    t0 = time.perf_counter()
                    m.fit_encoded(train, validation=val)
                    walls[name] = time.perf_counter() - t0
                    m._release()
                print(json.dumps({
                    "case": "fit", "build_id": _lib.build_id(), "config": config, "restarts": S,
                    "iterations": args.fit_iterations, "check_every": 50, "plain_s": round(walls["plain"], 4),
                    "monitored_s": round(walls["monitored"], 4), "plain_again_s": round(walls["plain again"], 4),
                    "monitored_over_plain": round(walls["monitored"] / walls["plain"], 4)}), flush=True)


if __name__ == "__main__":
    main()
