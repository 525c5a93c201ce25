"""Fold-in of new items (HipEM.fold_in_items, HipEM.recommend_add_items): device time of the all-iterations launch,
next to the device time of the same number of EM iterations on the same data, and the cost of an extended catalogue.

    python scripts/fold_in_items_time.py [--config c3|c3s8|one|extended|all] [--iters 100] [--reps 5]

Shapes (random parameters: the time does not depend on their values, only the iteration count does -- no tol):
  c3        BASELINE C3: all 20,000 items re-folded from their own 1M training rows, K = L = 20, R = 5, one restart
  c3s8      the same for 8 restarts (one fold-in per restart slot, device times summed)
  one       one new item with 20 ratings of the C3 model
  extended  an all-user top-10 recommend_query at C3, before and after recommend_add_items of 2,000 items, in the same
            session (option "recommend_ms", median of --reps after a warm-up)

fold_in_ms is the option "fold_in_ms" (HIP events around the fold-in's kernels, median of --reps after a warm-up);
em_ms is mmsbm_hip_time_iterations over the same number of EM iterations on the training data.  FLOP counts the update
only: per row and iteration 2 L (dot) + 2 L (q, fma) + the division, per row once 2 K L (v).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fold_in_time as fu  # noqa: E402  (the C3 context, the fold-in timing report)
import numpy as np  # noqa: E402

from mmsbm_amd import _lib  # noqa: E402


def timed_fold_items(em, slots, rows, n_new, iters, reps):
    em.select(0).fold_in_items(rows, n_new, iters)            # warm-up
    dev, host = [], []
    for _ in range(reps):
        ms, t0 = 0.0, time.perf_counter()
        for s in range(slots):
            em.select(s).fold_in_items(rows, n_new, iters)
            ms += em.get_option("fold_in_ms")
        host.append(time.perf_counter() - t0)
        dev.append(ms)
    return float(np.median(dev)), float(np.median(host)) * 1e3, dev


def report(name, rows, n_new, K, L, iters, slots, dev, host, devs, em_ms=None):
    flop = slots * (len(rows) * iters * (4.0 * L + 1) + 2.0 * K * L * len(rows))
    out = {"shape": name, "build_id": _lib.build_id(), "new_items": int(n_new), "rows": int(len(rows)), "K": K, "L": L,
           "restarts": slots, "iterations": iters, "fold_in_ms": round(dev, 3), "times_ms": [round(x, 3) for x in devs],
           "host_call_ms": round(host, 2), "gflops": round(flop / dev / 1e6, 1), "peak_share": round(flop / dev / 1e-3 / fu.PEAK, 4)}
    if em_ms is not None:
        out["em_ms_same_iterations"] = round(em_ms, 3)
    print(f"{name:8s} {n_new:>7,} items {len(rows):>9,} rows x {slots}: fold-in {dev:8.3f} ms  host {host:8.1f} ms  "
          f"{flop / dev / 1e6:8.1f} GFLOP/s" + (f"  EM x {iters}: {em_ms:8.3f} ms" if em_ms is not None else ""), flush=True)
    print(json.dumps(out), flush=True)
    return out


def run_c3(name, slots, iters, reps):
    em, data, U, I, R, K, L = fu.c3_context(slots)
    with em:
        dev, host, devs = timed_fold_items(em, slots, data, I, iters, reps)
        em_ms = em.time_iterations(iters) if slots == 1 else None
    d = np.bincount(data[:, 1], minlength=I)
    print(f"         items on chip (d L <= 1024): {int((d * L <= 1024).sum()):,} of {I:,}, streamed: "
          f"{int((d * L > 1024).sum()):,} (max degree {int(d.max())})", flush=True)
    return report(name, data, I, K, L, iters, slots, dev, host, devs, em_ms)


def run_one(iters, reps):
    em, data, U, I, R, K, L = fu.c3_context(1)
    rng = np.random.default_rng(3)
    rows = np.stack([rng.integers(0, U, 20), np.zeros(20, dtype=np.int64), rng.integers(0, R, 20)], 1)
    with em:
        dev, host, devs = timed_fold_items(em, 1, rows, 1, iters, reps)
    return report("one", rows, 1, K, L, iters, 1, dev, host, devs)


def run_extended(reps, n_new=2000):
    em, data, U, I, R, K, L = fu.c3_context(1)
    users = np.arange(U, dtype=np.int32)
    eta = np.random.default_rng(6).random((1, n_new, L))

    def query():
        em.recommend_query(users, 10)                         # warm-up
        ms = []
        for _ in range(reps):
            em.recommend_query(users, 10)
            ms.append(em.get_option("recommend_ms"))
        return float(np.median(ms)), ms

    with em:
        em.recommend_begin(np.arange(1.0, R + 1), True)
        em.select(0).recommend_add()
        plain, plain_all = query()
        em.recommend_add_items(eta)
        wide, wide_all = query()
        em.recommend_end()
    out = {"shape": "extended", "build_id": _lib.build_id(), "users": int(U), "items": int(I), "new_items": n_new,
           "n": 10, "recommend_ms": round(plain, 3), "recommend_ms_extended": round(wide, 3),
           "times_ms": [round(x, 3) for x in plain_all], "times_ms_extended": [round(x, 3) for x in wide_all],
           "ratio": round(wide / plain, 4), "item_ratio": round((I + n_new) / I, 4)}
    print(f"extended all {U:,} users top-10: {plain:8.3f} ms over {I:,} items, {wide:8.3f} ms over {I + n_new:,} "
          f"(x{wide / plain:.3f}; items x{(I + n_new) / I:.3f})", flush=True)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=["all", "c3", "c3s8", "one", "extended"])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print(f"build {_lib.build_id()}", flush=True)
    todo = ["c3", "c3s8", "one", "extended"] if args.config == "all" else [args.config]
    for name in todo:
        if name == "c3":
            run_c3("c3", 1, args.iters, args.reps)
        elif name == "c3s8":
            run_c3("c3s8", 8, args.iters, args.reps)
        elif name == "one":
            run_one(args.iters, args.reps)
        else:
            run_extended(args.reps)


if __name__ == "__main__":
    main()
