"""Top-N recommendation (HipEM.recommend_*): time of a query over every user, its share of the fp64 peak, the
latency of a single user, and the numpy restatement on a sample of users scaled up for comparison.

    python scripts/recommend_time.py [--config c3|c3s8|ml20m|c5|all] [--n 10] [--reps 5]

Shapes (random parameters: the time does not depend on their values):
  c3     BASELINE C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20, one restart
  c3s8   the same with 8 restarts (restart slots of one context)
  ml20m  MovieLens-20M's shape: 20M ratings, 138,493 users x 26,744 items, R = 10, K = L = 20
  c5     BASELINE C5: 10M ratings, 1M users x 100k items, R = 10, K = L = 50

The timed region is one recommend_query of all users (median of --reps after one warm-up): HIP events on the context's
stream around the query's kernels (option "recommend_ms"); host_call_ms is the whole call, results in host memory.
FLOP = 2 x rank x restarts per (user, item) pair, rank = min(K, L); the peak is AMD's 78.6 TFLOP/s fp64 figure for the
MI355X.
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
from oracle import mmsbm_oracle as orc  # noqa: E402

PEAK = 78.6e12
SHAPES = {  # name: (ratings, users, items, R, K, L, restarts)
    "c3": (1_000_000, 100_000, 20_000, 5, 20, 20, 1),
    "c3s8": (1_000_000, 100_000, 20_000, 5, 20, 20, 8),
    "ml20m": (20_000_263, 138_493, 26_744, 10, 20, 20, 1),
    "c5": (10_000_000, 1_000_000, 100_000, 10, 50, 50, 1),
}


def numpy_time(params, users, n_items, w, n, seen):
    """The restatement (oracle prod_dist per restart, mean, @ w, exclusion, lexsort) on `users`; seconds."""
    t0 = time.perf_counter()
    for u in users.tolist():
        pairs = np.stack([np.full(n_items, u), np.arange(n_items), np.zeros(n_items, dtype=np.int64)], 1)
        s = np.array([orc.prod_dist(pairs, t, e, p) for t, e, p in params]).mean(axis=0) @ w
        cand = np.setdiff1d(np.arange(n_items), seen.get(u, np.zeros(0, dtype=np.int64)))
        _ = cand[np.lexsort((cand, -s[cand]))][:n]
    return time.perf_counter() - t0


def one(name, n, reps):
    n_obs, U, I, R, K, L, S = SHAPES[name]
    data = synthetic_triples(n_obs, U, I, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    params = [(rng.random((U, K)), rng.random((I, L)), orc.normalize_with_self(rng.random((K, L, R)))) for _ in range(S)]
    w = np.arange(1.0, R + 1)
    users = np.arange(U, dtype=np.int32)
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        t0 = time.perf_counter()
        em.recommend_begin(w, True)
        for s in range(S):
            em.select(s).recommend_add()
        t_setup = time.perf_counter() - t0
        em.recommend_query(users, n)                      # warm-up
        times, host = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            em.recommend_query(users, n)
            host.append(time.perf_counter() - t0)
            times.append(em.get_option("recommend_ms") / 1e3)   # HIP events around the query's kernels
        single = []
        for u in rng.choice(U, 21, replace=False).tolist():
            t0 = time.perf_counter()
            em.recommend_query([u], n)
            single.append(time.perf_counter() - t0)
        em.recommend_end()
    t = float(np.median(times))
    flop = 2.0 * min(K, L) * S * U * I
    # numpy on a few users, scaled up to all of them
    sample = rng.choice(U, 4 if K * L * S <= 400 else 2, replace=False)
    mask = np.isin(data[:, 0], sample)
    seen = {int(u): np.unique(data[mask & (data[:, 0] == u), 1]) for u in sample}
    t_np = numpy_time(params, sample, I, w, n, seen) / len(sample) * U
    out = {"shape": name, "build_id": _lib.build_id(), "users": U, "items": I, "K": K, "L": L, "R": R, "restarts": S,
           "n": n, "query_all_ms": round(t * 1e3, 3), "times_ms": [round(x * 1e3, 3) for x in times],
           "host_call_ms": round(float(np.median(host)) * 1e3, 3),
           "gflops": round(flop / t / 1e9, 1), "peak_share": round(flop / t / PEAK, 4),
           "session_setup_ms": round(t_setup * 1e3, 1), "single_user_ms": round(float(np.median(single)) * 1e3, 3),
           "numpy_scaled_s": round(t_np, 1), "speedup_vs_numpy": round(t_np / t, 0)}
    print(f"{name:6s} {U:>9,} x {I:>7,} rank {min(K, L)} x {S}: all users {t * 1e3:9.2f} ms  {flop / t / 1e9:9.1f} GFLOP/s "
          f"({100 * flop / t / PEAK:5.1f} % of 78.6 TFLOP/s)  one user {np.median(single) * 1e3:.3f} ms  "
          f"numpy (scaled) {t_np:9.1f} s", flush=True)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=["all"] + list(SHAPES))
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print(f"build {_lib.build_id()}", flush=True)
    for name in (SHAPES if args.config == "all" else [args.config]):
        one(name, args.n, args.reps)


if __name__ == "__main__":
    main()
