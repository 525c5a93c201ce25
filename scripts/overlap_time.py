"""The overlap of the restarts' groups (HipEM.overlap_*): time of a query, next to numpy's X.T @ X on the same tables on
this host -- context, not a gate: a host BLAS gives a result that depends on its thread count, the device's does not.

    python scripts/overlap_time.py [--reps 5] [--cases users_c3_s1,users_c3_s8,items_c3_s1,items_c3_s8,users_c5_s8]

C3: 99,997 users x 20,000 items, K = L = 20; C5's user side: 1,000,000 users, K = 50.  Random row-normalised tables (the
time does not depend on their values).  Cases: <side>_<shape>_s<restarts>; X is rows x (restarts x groups).
The timed region is one overlap_query (median of --reps after one warm-up): HIP events on the context's stream around
the query's two kernels (option "overlap_ms"); host_call_ms is the whole call, the copy of the result included.
numpy: the wall time of X.T @ X (median of 3 after one warm-up) at the threads this process is granted
(OMP_NUM_THREADS and its like, reported).
The C5 case uses a context of its own with one slot and few items and ratings -- the session only reads the user
table -- whose slot is given new parameters and added eight times.
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

C3 = (1_000_000, 100_000, 20_000, 5, 20, 20)              # N, U, I, R, K, L
C5_USERS, C5_K = 1_000_000, 50
CASES = ("users_c3_s1", "users_c3_s8", "items_c3_s1", "items_c3_s8", "users_c5_s8")


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def numpy_ms(tables):
    X = np.ascontiguousarray(np.concatenate(tables, axis=1))
    _ = X.T @ X
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        _ = X.T @ X
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3


def timed_queries(em, reps):
    em.overlap_query()                                    # warm-up
    dev, host = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        em.overlap_query()
        host.append(time.perf_counter() - t0)
        dev.append(em.get_option("overlap_ms"))
    return float(np.median(dev)), float(np.median(host)) * 1e3, [round(x, 3) for x in dev]


def report(name, rows, groups, restarts, setup_ms, timing, tables):
    ms, host, all_ms = timing
    fma = float(rows) * (restarts * groups) ** 2
    t_np = numpy_ms(tables)
    out = {"case": name, "build_id": _lib.build_id(), "rows": rows, "groups": groups, "restarts": restarts,
           "columns": restarts * groups, "overlap_ms": round(ms, 3), "times_ms": all_ms, "host_call_ms": round(host, 3),
           "session_setup_ms": round(setup_ms, 1), "gfma_per_s_full_square": round(fma / ms / 1e6, 1),
           "numpy_xtx_ms": round(t_np, 3), "numpy_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
           "numpy_over_device": round(t_np / ms, 1)}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    cases = args.cases.split(",")
    assert set(cases) <= set(CASES), cases
    print(f"build {_lib.build_id()}", flush=True)
    rng = np.random.default_rng(1)

    def session(em, side, slots):
        t0 = time.perf_counter()
        em.overlap_begin(side)
        for s in slots:
            em.select(s).overlap_add()
        return (time.perf_counter() - t0) * 1e3

    if any("_c3_" in c for c in cases):
        N, U, I, R, K, L = C3
        data = synthetic_triples(N, U, I, R, seed=0)
        U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
        S = 8 if any(c.endswith("_c3_s8") for c in cases) else 1
        params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S)]
        with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S) as em:
            for s, p in enumerate(params):
                em.select(s).set_params(*p)
            for side, rows, G, at in (("users", U, K, 0), ("items", I, L, 1)):
                for n in (1, 8):
                    name = f"{side}_c3_s{n}"
                    if name not in cases:
                        continue
                    setup = session(em, side, range(n))
                    report(name, rows, G, n, setup, timed_queries(em, args.reps), [p[at] for p in params[:n]])
                    em.overlap_end()
    if "users_c5_s8" in cases:
        U, K, I, L, R, S = C5_USERS, C5_K, 1000, 2, 2, 8
        data = np.stack([np.arange(U), np.arange(U) % I, np.arange(U) % R], 1)
        eta, p = row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))
        tables = []
        with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=1) as em:
            t0 = time.perf_counter()
            em.overlap_begin("users")
            for _ in range(S):
                tables.append(row_normalised(rng, (U, K)))
                em.set_params(tables[-1], eta, p)
                em.overlap_add()
            setup = (time.perf_counter() - t0) * 1e3      # (with the eight uploads)
            report("users_c5_s8", U, K, S, setup, timed_queries(em, args.reps), tables)
            em.overlap_end()


if __name__ == "__main__":
    main()
