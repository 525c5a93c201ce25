"""Nearest items / users (HipEM.similar_*): time of a query at BASELINE C3's shape, next to two yardsticks that are not
the code under test -- the numpy restatement on the host, and the recommend query of the same context.

    python scripts/similar_time.py [--n 10] [--reps 5] [--cases items_s1,items_s8,one_item,users_1000,recommend]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters: the time does not
depend on their values).  Cases:
  items_s1    every item against every item, one restart          (4.0e8 pairs x 100 profile entries)
  items_s8    the same with 8 restarts                             (x 800 profile entries)
  one_item    one item against all 20,000 (median over 21 items, whole host call as well)
  users_1000  1,000 users against all 99,997, one restart          (1.0e8 pairs x 100 profile entries)
  recommend   the recommend query of all users of the same context (2.0e9 pairs x rank 20): the yardstick per
              (pair x rank entry)
The timed region is one similar_query (median of --reps after one warm-up): HIP events on the context's stream around
the query's kernels (option "similar_ms"), distance tile and selection together; the split between the two comes from
a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python scripts/similar_time.py --reps 1).
numpy: profiles by einsum once, then per query row the direct form against every row and a lexsort, on a few rows,
scaled to the rows of the case.
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
CASES = ("items_s1", "items_s8", "one_item", "users_1000", "recommend")


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def numpy_seconds_per_row(params, side, sample, n):
    """The restatement on the host for the query rows `sample`; seconds per query row (the profiles are not timed)."""
    prof = []
    for theta, eta, p in params:
        if side == "items":
            prof.append((np.einsum("il,klr->ikr", eta, p), theta.sum(axis=0)))
        else:
            prof.append((np.einsum("uk,klr->ulr", theta, p), eta.sum(axis=0)))
    rows = prof[0][0].shape[0]
    others = params[0][0].shape[0] if side == "items" else params[0][1].shape[0]
    t0 = time.perf_counter()
    for i in sample.tolist():
        num = np.zeros(rows)
        for q, m in prof:
            d = q[i][None] - q
            num += ((d * d).sum(axis=2) * m[None, :]).sum(axis=1)
        dist = num / (len(params) * others)
        cand = np.delete(np.arange(rows), i)
        _ = cand[np.lexsort((cand, dist[cand]))][:n]
    return (time.perf_counter() - t0) / len(sample)


def timed_queries(em, ids, n, reps):
    em.similar_query(ids, n)                              # warm-up
    dev, host = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        em.similar_query(ids, n)
        host.append(time.perf_counter() - t0)
        dev.append(em.get_option("similar_ms"))
    return float(np.median(dev)), float(np.median(host)) * 1e3, [round(x, 3) for x in dev]


def report(name, **kw):
    out = {"case": name, "build_id": _lib.build_id(), **kw}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    cases = args.cases.split(",")
    assert set(cases) <= set(CASES), cases
    n, reps = args.n, args.reps
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    S = 8 if "items_s8" in cases else 1
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S)]
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)

        def session(side, slots):
            t0 = time.perf_counter()
            em.similar_begin(side)
            for s in range(slots):
                em.select(s).similar_add()
            return (time.perf_counter() - t0) * 1e3

        if "items_s1" in cases or "one_item" in cases:
            setup = session("items", 1)
            if "items_s1" in cases:
                ms, host, all_ms = timed_queries(em, np.arange(I, dtype=np.int32), n, reps)
                entries = float(I) * I * K * R
                t_np = numpy_seconds_per_row(params[:1], "items", rng.choice(I, 8, replace=False), n) * I
                report("items_s1", rows=I, queries=I, restarts=1, profile=K * R, n=n, similar_ms=round(ms, 3), times_ms=all_ms,
                       host_call_ms=round(host, 3), session_setup_ms=round(setup, 1),
                       ps_per_pair_entry=round(ms * 1e9 / entries, 4), numpy_scaled_s=round(t_np, 1),
                       speedup_vs_numpy=round(t_np / (ms / 1e3), 0))
            if "one_item" in cases:
                dev, host = [], []
                for i in rng.choice(I, 21, replace=False).tolist():
                    t0 = time.perf_counter()
                    em.similar_query([i], n)
                    host.append((time.perf_counter() - t0) * 1e3)
                    dev.append(em.get_option("similar_ms"))
                t_np = numpy_seconds_per_row(params[:1], "items", rng.choice(I, 8, replace=False), n)
                report("one_item", rows=I, queries=1, restarts=1, profile=K * R, n=n, similar_ms=round(float(np.median(dev)), 3),
                       host_call_ms=round(float(np.median(host)), 3), numpy_ms=round(t_np * 1e3, 3))
            em.similar_end()
        if "items_s8" in cases:
            setup = session("items", 8)
            ms, host, all_ms = timed_queries(em, np.arange(I, dtype=np.int32), n, reps)
            entries = float(I) * I * K * R * 8
            t_np = numpy_seconds_per_row(params, "items", rng.choice(I, 4, replace=False), n) * I
            report("items_s8", rows=I, queries=I, restarts=8, profile=K * R * 8, n=n, similar_ms=round(ms, 3), times_ms=all_ms,
                   host_call_ms=round(host, 3), session_setup_ms=round(setup, 1),
                   ps_per_pair_entry=round(ms * 1e9 / entries, 4), numpy_scaled_s=round(t_np, 1),
                   speedup_vs_numpy=round(t_np / (ms / 1e3), 0))
            em.similar_end()
        if "users_1000" in cases:
            setup = session("users", 1)
            ids = rng.choice(U, 1000, replace=False).astype(np.int32)
            ms, host, all_ms = timed_queries(em, ids, n, reps)
            entries = 1000.0 * U * L * R
            t_np = numpy_seconds_per_row(params[:1], "users", ids[:4], n) * 1000
            report("users_1000", rows=U, queries=1000, restarts=1, profile=L * R, n=n, similar_ms=round(ms, 3), times_ms=all_ms,
                   host_call_ms=round(host, 3), session_setup_ms=round(setup, 1),
                   ps_per_pair_entry=round(ms * 1e9 / entries, 4), numpy_scaled_s=round(t_np, 1),
                   speedup_vs_numpy=round(t_np / (ms / 1e3), 0))
            em.similar_end()
        if "recommend" in cases:                         # the yardstick: the score tile's time per (pair x rank entry)
            em.recommend_begin(np.arange(1.0, R + 1), True)
            em.select(0).recommend_add()
            users = np.arange(U, dtype=np.int32)
            em.recommend_query(users, n)
            dev = []
            for _ in range(reps):
                em.recommend_query(users, n)
                dev.append(em.get_option("recommend_ms"))
            em.recommend_end()
            ms = float(np.median(dev))
            report("recommend", users=U, items=I, rank=min(K, L), n=n, recommend_ms=round(ms, 3),
                   times_ms=[round(x, 3) for x in dev], ps_per_pair_entry=round(ms * 1e9 / (float(U) * I * min(K, L)), 4))


if __name__ == "__main__":
    main()
