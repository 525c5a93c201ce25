"""Category-level recommendation (HipEM.recommend_query_shelves): device times at BASELINE C3's shape next to the plain
query and the quota query of the same session, and next to the emulation the query replaces.

    python scripts/shelves_time.py [--reps 5] [--slots 1,8] [--emulate 20,200,2000] [--mean-entries 20000000]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded.  Per S, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each, all users, n_shelves = 5,
per_shelf = 10, depth = 10, min_items = 1:
    recommend_query_shelves over
        20 / 200 / 2,000 equal categories, once as item % G (a category's columns are G apart: every column its own
        cache line) and once as contiguous blocks (a category's columns are neighbours) -- the same shuffles and lists,
        different lines gathered;
        313 and 307 equal categories (63-64 and 65-66 columns each: the widest short groups next to the shortest long
        categories), both ways;
    recommend_query_quota(cap 1, n = 10) on the same layouts;
    recommend_query(n = 10), the plain query.
Each figure is the median of the device times (HIP events around each call's kernels: option "recommend_ms"); the host
time of the call, with its copies, is printed beside it.
The emulation, once per G of --emulate on the item % G layout after the loop above: one recommend_query_within(n = depth,
candidates = the category) per category, all users -- device times summed, host times summed -- and, timed apart, the
host mean and sort of the users x G values over as many users as --mean-entries allows; its categories and values are
compared with the query's by equality (answers_equal).
Not measured: the spread of the repetitions beyond their median, and how the gathered lines split between the L2 and the
MALL.
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
SHELVES, PER_SHELF, DEPTH, TOP = 5, 10, 10, 10
EQUAL = (20, 200, 2000)
BORDER = (313, 307)


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def csr_of(category_of, n_cats):
    order = np.argsort(category_of, kind="stable")
    counts = np.bincount(category_of, minlength=n_cats)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), order.astype(np.int32)


def emulate(em, users, off, items, mean_entries):
    """(device ms, host ms of the calls, mean-and-sort ms, users done, categories [users done][SHELVES], values)."""
    G = len(off) - 1
    rows = max(1, min(len(users), mean_entries // (G * DEPTH)))
    got_s = np.empty((rows, G, DEPTH))
    got_n = np.empty((rows, G), dtype=np.int32)
    dev = host = 0.0
    for g in range(G):
        t0 = time.perf_counter()
        _, sc, cn = em.recommend_query_within(users, DEPTH, items[off[g]:off[g + 1]])
        host += (time.perf_counter() - t0) * 1e3
        dev += em.get_option("recommend_ms")
        got_s[:, g], got_n[:, g] = sc[:rows], cn[:rows]
    t0 = time.perf_counter()
    acc = got_s[:, :, 0].copy()
    for j in range(1, DEPTH):                                  # left to right, as the query adds
        acc = np.where(j < got_n, acc + got_s[:, :, j], acc)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(got_n > 0, acc / np.minimum(DEPTH, got_n), -np.inf)
    top = np.argsort(-v, axis=1, kind="stable")[:, :SHELVES]
    vals = np.take_along_axis(v, top, axis=1)
    return dev, host, (time.perf_counter() - t0) * 1e3, rows, np.where(vals > -np.inf, top, -1), vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", default="1,8")
    ap.add_argument("--emulate", default="20,200,2000")
    ap.add_argument("--mean-entries", type=int, default=20_000_000)
    args = ap.parse_args()
    slot_list = [int(x) for x in args.slots.split(",")]
    emulated = [int(x) for x in args.emulate.split(",") if x]
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    S_max = max(slot_list)
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S_max)]
    users = np.arange(U, dtype=np.int32)
    layouts = {}
    for G in EQUAL + BORDER:
        layouts[f"mod{G}"] = csr_of(np.arange(I) % G, G)
        layouts[f"blocks{G}"] = csr_of(np.arange(I) * G // I, G)
    sizes = {k: np.diff(v[0]) for k, v in layouts.items()}
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, prm in enumerate(params):
            em.select(s).set_params(*prm)
        for S in slot_list:
            em.recommend_begin(np.arange(1.0, R + 1), True)
            for s in range(S):
                em.select(s).recommend_add()

            def timed(call):
                t0 = time.perf_counter()
                out = call()
                return em.get_option("recommend_ms"), (time.perf_counter() - t0) * 1e3, out

            calls = {}
            for name, c in layouts.items():
                calls[f"shelves_{name}"] = lambda c=c: em.recommend_query_shelves(users, c[0], c[1], DEPTH, 1, SHELVES, PER_SHELF)
                calls[f"quota_{name}_cap1"] = lambda c=c: em.recommend_query_quota(
                    users, TOP, c[0], c[1], np.ones(len(c[0]) - 1, dtype=np.int32))
            calls["recommend_query_all_n10"] = lambda: em.recommend_query(users, TOP)
            dev = {k: [] for k in calls}
            host = {k: [] for k in calls}
            last = {}
            for rep in range(args.reps + 1):                       # rep 0: the warm-up of each
                for k, call in calls.items():                      # alternating
                    d, h, out = timed(call)
                    if k.startswith("shelves_mod"):
                        last[k] = (out[0], out[1])
                    del out
                    if rep:
                        dev[k].append(d)
                        host[k].append(h)
            med = {k: float(np.median(v)) for k, v in dev.items()}
            plain = med["recommend_query_all_n10"]
            emu = {}
            for G in emulated:
                off, items = layouts[f"mod{G}"]
                d, h, m, rows, cats, vals = emulate(em, users, off, items, args.mean_entries)
                want = last[f"shelves_mod{G}"]
                emu[f"mod{G}"] = {"device_ms": round(d, 3), "host_ms": round(h, 3), "mean_sort_ms": round(m, 3), "users_done": rows,
                                  "answers_equal": bool(np.array_equal(cats, want[0][:rows]) and
                                                        np.array_equal(vals.view(np.int64), want[1][:rows].view(np.int64)))}
            out = {"build_id": _lib.build_id(), "users": U, "items": I, "rank": min(K, L), "restarts": S, "reps": args.reps,
                   "n_shelves": SHELVES, "per_shelf": PER_SHELF, "depth": DEPTH,
                   "category_sizes": {k: [int(v.min()), int(np.median(v)), int(v.max())] for k, v in sizes.items()},
                   "short_categories": {k: int(((v <= 64) & (v > 0)).sum()) for k, v in sizes.items()},
                   "device_ms": {k: round(v, 3) for k, v in med.items()},
                   "host_ms": {k: round(float(np.median(v)), 3) for k, v in host.items()},
                   "ms_over_plain": {k: round(v - plain, 3) for k, v in med.items() if k != "recommend_query_all_n10"},
                   "emulation": emu}
            print(json.dumps(out), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
