"""Fold-in of new users (HipEM.fold_in, MMSBM.recommend_new): device time of the all-iterations launch, next to the
device time of the same number of EM iterations on the same data.

    python scripts/fold_in_time.py [--config c3|c3s8|one|zipf|recommend_new|all] [--iters 100] [--reps 5]

Shapes (random parameters: the time does not depend on their values, only the iteration count does -- no tol):
  c3             BASELINE C3: all 99,997 users re-folded from their own 1M training rows, K = L = 20, R = 5, one restart
  c3s8           the same for 8 restarts (one fold-in per restart slot, device times summed)
  one            one new user with 20 ratings of the C3 model
  zipf           160k new users whose degrees follow Zipf(2.0) (capped at 20k rows), about 1M rows, the C3 model
  recommend_new  MMSBM.recommend_new wall clock for 1,000 new users x 20 ratings, n = 10, on a model fitted to C3
                 (3 restarts, 20 EM iterations: the fit is not what is timed)

fold_in_ms is the option "fold_in_ms" (HIP events around the fold-in's kernels, median of --reps after a warm-up);
em_ms is mmsbm_hip_time_iterations over the same number of EM iterations on the training data.  FLOP counts the update
only: per row and iteration 2 K (dot) + 2 K (q, fma) + the division, per row once 2 K L (v).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from mmsbm_amd import HipEM, MMSBM, _lib  # noqa: E402
from mmsbm_amd.synthetic import synthetic_triples  # noqa: E402
from oracle import mmsbm_oracle as orc  # noqa: E402

PEAK = 78.6e12
C3 = (1_000_000, 100_000, 20_000, 5, 20, 20)


def c3_context(slots):
    n_obs, U, I, R, K, L = C3
    data = synthetic_triples(n_obs, U, I, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    params = [(rng.random((U, K)), rng.random((I, L)), orc.normalize_with_self(rng.random((K, L, R))))
              for _ in range(slots)]
    em = HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=slots)
    for s, p in enumerate(params):
        em.select(s).set_params(*p)
    return em, data, U, I, R, K, L


def timed_fold(em, slots, rows, n_new, iters, reps):
    em.select(0).fold_in(rows, n_new, iters)                  # warm-up
    dev, host = [], []
    for _ in range(reps):
        ms, t0 = 0.0, time.perf_counter()
        for s in range(slots):
            em.select(s).fold_in(rows, n_new, iters)
            ms += em.get_option("fold_in_ms")
        host.append(time.perf_counter() - t0)
        dev.append(ms)
    return float(np.median(dev)), float(np.median(host)) * 1e3, dev


def report(name, rows, n_new, K, L, iters, slots, dev, host, devs, em_ms=None):
    flop = slots * (len(rows) * iters * (4.0 * K + 1) + 2.0 * K * L * len(rows))
    out = {"shape": name, "build_id": _lib.build_id(), "new_users": int(n_new), "rows": int(len(rows)), "K": K, "L": L,
           "restarts": slots, "iterations": iters, "fold_in_ms": round(dev, 3), "times_ms": [round(x, 3) for x in devs],
           "host_call_ms": round(host, 2), "gflops": round(flop / dev / 1e6, 1), "peak_share": round(flop / dev / 1e-3 / PEAK, 4)}
    if em_ms is not None:
        out["em_ms_same_iterations"] = round(em_ms, 3)
    print(f"{name:8s} {n_new:>7,} users {len(rows):>9,} rows x {slots}: fold-in {dev:8.3f} ms  host {host:8.1f} ms  "
          f"{flop / dev / 1e6:8.1f} GFLOP/s" + (f"  EM x {iters}: {em_ms:8.3f} ms" if em_ms is not None else ""), flush=True)
    print(json.dumps(out), flush=True)
    return out


def run_c3(name, slots, iters, reps):
    em, data, U, I, R, K, L = c3_context(slots)
    with em:
        dev, host, devs = timed_fold(em, slots, data, U, iters, reps)
        em_ms = em.time_iterations(iters) if slots == 1 else None
    return report(name, data, U, K, L, iters, slots, dev, host, devs, em_ms)


def run_one(iters, reps):
    em, data, U, I, R, K, L = c3_context(1)
    rng = np.random.default_rng(3)
    rows = np.stack([np.zeros(20, dtype=np.int64), rng.integers(0, I, 20), rng.integers(0, R, 20)], 1)
    with em:
        dev, host, devs = timed_fold(em, 1, rows, 1, iters, reps)
    return report("one", rows, 1, K, L, iters, 1, dev, host, devs)


def run_zipf(iters, reps):
    em, data, U, I, R, K, L = c3_context(1)
    rng = np.random.default_rng(4)
    deg = np.minimum(rng.zipf(2.0, 160_000), 20_000)
    u = np.repeat(np.arange(len(deg)), deg)
    rows = np.stack([u, rng.integers(0, I, len(u)), rng.integers(0, R, len(u))], 1)
    with em:
        dev, host, devs = timed_fold(em, 1, rows, len(deg), iters, reps)
    return report("zipf", rows, len(deg), K, L, iters, 1, dev, host, devs)


def run_recommend_new(iters, reps):
    n_obs, U, I, R, K, L = C3
    data = synthetic_triples(n_obs, U, I, R, seed=0)
    model = MMSBM(K, L, iterations=20, sampling=3, seed=0)
    model.fit(pd.DataFrame(data, columns=["users", "items", "ratings"]), silent=True)
    rng = np.random.default_rng(5)
    new = pd.DataFrame({"users": np.repeat([f"new{x}" for x in range(1000)], 20),
                        "items": rng.choice(data[:, 1], 20_000), "ratings": rng.choice(data[:, 2], 20_000)})
    model.recommend_new(new, n=10, iterations=iters)          # warm-up
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        model.recommend_new(new, n=10, iterations=iters)
        wall.append(time.perf_counter() - t0)
    model._release()
    out = {"shape": "recommend_new", "build_id": _lib.build_id(), "new_users": 1000, "rows": 20_000, "restarts": 3,
           "iterations": iters, "n": 10, "wall_ms": round(float(np.median(wall)) * 1e3, 2)}
    print(f"recommend_new 1,000 users x 20 ratings, 3 restarts: {np.median(wall) * 1e3:8.2f} ms wall", flush=True)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=["all", "c3", "c3s8", "one", "zipf", "recommend_new"])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print(f"build {_lib.build_id()}", flush=True)
    todo = ["c3", "c3s8", "one", "zipf", "recommend_new"] if args.config == "all" else [args.config]
    for name in todo:
        if name == "c3":
            run_c3("c3", 1, args.iters, args.reps)
        elif name == "c3s8":
            run_c3("c3s8", 8, args.iters, args.reps)
        elif name == "one":
            run_one(args.iters, args.reps)
        elif name == "zipf":
            run_zipf(args.iters, args.reps)
        else:
            run_recommend_new(args.iters, args.reps)


if __name__ == "__main__":
    main()
