"""Recommendation within a part of the catalogue (HipEM.recommend_query_within / recommend_rank): device times at
BASELINE C3's shape next to the plain query of the same session.

    python scripts/catalogue_time.py [--reps 5] [--slots 1,8]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded.  Per S, IN ONE PROCESS and ALTERNATING, --reps times after one warm-up of each, all users, n = 10:
    recommend_query_within with C = 1 %, 10 % and 100 % of the catalogue (random ascending ids; 100 %: every id named),
    recommend_rank with 200 random candidates per user,
    recommend_query (the parent's path: all I columns scored and selected).
Each figure is the median of the device times (HIP events around each call's kernels, the gather of the candidates'
rows included: option "recommend_ms"); the host time of the call, with its copies, is printed beside it.
answers_equal: the 1 % query and the rank query of 500 sampled users against the rows of recommend_query(n = 1024)
filtered to the candidates -- same items and same score bits wherever 10 candidates are among a user's 1,024 best.
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
SHARES = (0.01, 0.10, 1.00)
TOP, PER_USER = 10, 200


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def check_against_plain(em, rng, users, cand, off, lists, n_users=500):
    """(rows compared, rows equal): the subset and the rank answers of sampled users against recommend_query's rows
    filtered to the candidates (rows whose 1,024 best hold fewer than TOP candidates are not compared)."""
    pick = np.sort(rng.choice(len(users), n_users, replace=False))
    ask = users[pick]
    fi, fs, fc = em.recommend_query(ask, 1024)
    wi, ws, _ = em.recommend_query_within(ask, TOP, cand)
    r_off = np.concatenate([[0], np.cumsum(off[pick + 1] - off[pick])]).astype(np.int64)
    r_items = np.concatenate([lists[off[b]:off[b + 1]] for b in pick.tolist()])
    ri, rs, _ = em.recommend_rank(ask, r_off, r_items, TOP)
    seen = same = 0
    for b in range(n_users):
        for got_i, got_s, keep in ((wi[b], ws[b], cand), (ri[b], rs[b], r_items[r_off[b]:r_off[b + 1]])):
            ok = np.isin(fi[b, :fc[b]], keep)
            if ok.sum() < TOP:
                continue
            seen += 1
            same += int(np.array_equal(fi[b, :fc[b]][ok][:TOP], got_i) and
                        np.array_equal(fs[b, :fc[b]][ok][:TOP].view(np.uint64), got_s.view(np.uint64)))
    return seen, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", default="1,8")
    args = ap.parse_args()
    slot_list = [int(x) for x in args.slots.split(",")]
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    S_max = max(slot_list)
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S_max)]
    users = np.arange(U, dtype=np.int32)
    subsets = {s: np.sort(rng.choice(I, max(1, int(round(s * I))), replace=False)).astype(np.int32) for s in SHARES}
    # PER_USER distinct ascending candidates per user: a random start and random positive steps
    steps = rng.integers(1, I // PER_USER, (U, PER_USER))
    steps[:, 0] = rng.integers(0, I // PER_USER, U)
    lists = np.cumsum(steps, axis=1).astype(np.int32).ravel()
    off = np.arange(U + 1, dtype=np.int64) * PER_USER
    assert lists.max() < I
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for S in slot_list:
            em.recommend_begin(np.arange(1.0, R + 1), True)
            for s in range(S):
                em.select(s).recommend_add()
            seen, same = check_against_plain(em, rng, users, subsets[SHARES[0]], off, lists)

            def timed(call):
                t0 = time.perf_counter()
                call()
                return em.get_option("recommend_ms"), (time.perf_counter() - t0) * 1e3

            calls = {f"query_within_{int(round(s * 100))}pct": (lambda c=c: em.recommend_query_within(users, TOP, c))
                     for s, c in subsets.items()}
            calls[f"recommend_rank_{PER_USER}_per_user"] = lambda: em.recommend_rank(users, off, lists, TOP)
            calls["recommend_query_all_n10"] = lambda: em.recommend_query(users, TOP)
            dev = {k: [] for k in calls}
            host = {k: [] for k in calls}
            for rep in range(args.reps + 1):                       # rep 0: the warm-up of each
                for k, call in calls.items():                      # alternating
                    d, h = timed(call)
                    if rep:
                        dev[k].append(d)
                        host[k].append(h)
            out = {"build_id": _lib.build_id(), "users": U, "items": I, "rank": min(K, L), "restarts": S, "reps": args.reps,
                   "candidates": {f"{int(round(s * 100))}pct": int(len(c)) for s, c in subsets.items()},
                   "device_ms": {k: round(float(np.median(v)), 3) for k, v in dev.items()},
                   "host_ms": {k: round(float(np.median(v)), 3) for k, v in host.items()},
                   "rows_compared": seen, "answers_equal": bool(seen > 0 and same == seen)}
            print(json.dumps(out), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
