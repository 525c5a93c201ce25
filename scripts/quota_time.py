"""Per-category caps on a top-N list (HipEM.recommend_query_quota): device times at BASELINE C3's shape next to the plain
query of the same session and next to the emulation the query replaces.

    python scripts/quota_time.py [--reps 5] [--slots 1,8] [--merge-entries 20000000]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded.  Per S, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each, all users, n = 10:
    recommend_query_quota with caps 1 and 2 over
        20 / 200 / 2,000 equal categories (item % G: 1,000 / 100 / 10 columns each -- the long form, the long form, the
        short form),
        313 and 307 equal categories (63-64 and 65-66 columns each: the widest short groups next to the shortest long
        categories, about the same work in either form),
        one Zipf-sized layout (2,000 categories, sizes ~ 1 / rank, items dealt at random: both forms in one query);
    recommend_query(n = 10), the plain query.
Each figure is the median of the device times (HIP events around each call's kernels: option "recommend_ms"); the host
time of the call, with its copies, is printed beside it.
The emulation, once per (G, cap) for G = 20 / 200 / 2,000 after the loop above: one recommend_query_within(n = cap,
candidates = the category) per category, all users -- device times summed, host times summed -- and, timed apart, the
host merge of the users x (G x cap) entries (numpy, by (score descending, item id)) over as many users as
--merge-entries allows; its answer is compared with the quota query's (answers_equal).
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
TOP = 10
EQUAL = (20, 200, 2000)
BORDER = (313, 307)
CAPS = (1, 2)


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def csr_of(category_of, n_cats):
    order = np.argsort(category_of, kind="stable")
    counts = np.bincount(category_of, minlength=n_cats)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), order.astype(np.int32)


def emulate(em, users, off, items, cap, merge_entries):
    """(device ms, host ms of the calls, merge ms, users merged, merged items [users merged][TOP])."""
    G = len(off) - 1
    rows = max(1, min(len(users), merge_entries // (G * cap)))
    got_i = np.empty((rows, G * cap), dtype=np.int32)
    got_s = np.empty((rows, G * cap))
    dev = host = 0.0
    for g in range(G):
        t0 = time.perf_counter()
        it, sc, _ = em.recommend_query_within(users, cap, items[off[g]:off[g + 1]])
        host += (time.perf_counter() - t0) * 1e3
        dev += em.get_option("recommend_ms")
        got_i[:, g * cap:(g + 1) * cap] = it[:rows]
        got_s[:, g * cap:(g + 1) * cap] = sc[:rows]
    t0 = time.perf_counter()
    ids = np.where(got_i < 0, np.iinfo(np.int32).max, got_i)
    order = np.lexsort((ids, -got_s), axis=1)[:, :TOP]
    merged = np.take_along_axis(got_i, order, axis=1)
    return dev, host, (time.perf_counter() - t0) * 1e3, rows, merged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", default="1,8")
    ap.add_argument("--merge-entries", type=int, default=20_000_000)
    args = ap.parse_args()
    slot_list = [int(x) for x in args.slots.split(",")]
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    S_max = max(slot_list)
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S_max)]
    users = np.arange(U, dtype=np.int32)
    layouts = {f"equal{G}": csr_of(np.arange(I) % G, G) for G in EQUAL + BORDER}
    p = 1.0 / np.arange(1, 2001)
    layouts["zipf2000"] = csr_of(rng.choice(2000, I, p=p / p.sum()), 2000)
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

            calls = {f"quota_{name}_cap{q}": (lambda c=csr, q=q: em.recommend_query_quota(
                users, TOP, c[0], c[1], np.full(len(c[0]) - 1, q, dtype=np.int32)))
                for name, csr in layouts.items() for q in CAPS}
            calls["recommend_query_all_n10"] = lambda: em.recommend_query(users, TOP)
            dev = {k: [] for k in calls}
            host = {k: [] for k in calls}
            last = {}
            for rep in range(args.reps + 1):                       # rep 0: the warm-up of each
                for k, call in calls.items():                      # alternating
                    d, h, last[k] = timed(call)
                    if rep:
                        dev[k].append(d)
                        host[k].append(h)
            med = {k: float(np.median(v)) for k, v in dev.items()}
            plain = med["recommend_query_all_n10"]
            emu = {}
            for G in EQUAL:
                off, items = layouts[f"equal{G}"]
                for q in CAPS:
                    d, h, m, rows, merged = emulate(em, users, off, items, q, args.merge_entries)
                    emu[f"equal{G}_cap{q}"] = {
                        "device_ms": round(d, 3), "host_ms": round(h, 3), "merge_ms": round(m, 3), "users_merged": rows,
                        "answers_equal": bool(np.array_equal(merged, last[f"quota_equal{G}_cap{q}"][0][:rows]))}
            out = {"build_id": _lib.build_id(), "users": U, "items": I, "rank": min(K, L), "restarts": S, "reps": args.reps,
                   "category_sizes": {k: [int(v.min()), int(np.median(v)), int(v.max())] for k, v in sizes.items()},
                   "short_categories": {k: int(((v <= 64) & (v > 0)).sum()) for k, v in sizes.items()},
                   "device_ms": {k: round(v, 3) for k, v in med.items()},
                   "host_ms": {k: round(float(np.median(v)), 3) for k, v in host.items()},
                   "mask_ms_over_plain": {k: round(v - plain, 3) for k, v in med.items() if k.startswith("quota_")},
                   "emulation": emu}
            print(json.dumps(out), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
