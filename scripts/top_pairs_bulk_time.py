"""The m best pairs beyond 1,024 (HipEM.recommend_top_pairs_bulk): device time at BASELINE C3's shape next to the only
exact route the library had before it -- a bisection on the bar with recommend_audience counts, then the filled
audience at the bar, then a host sort and the cut of the ties.

    python scripts/top_pairs_bulk_time.py [--reps 5] [--ms 1024,10000,100000,1000000,10000000] [--slots 1,8]

C3: 1M ratings, 99,997 users x 20,000 items, R = 5, K = L = 20 (random row-normalised parameters), training pairs
excluded.  Per (S, m) both routes run IN THE SAME PROCESS, ALTERNATING, --reps times after one warm-up of each; the
figures are medians.  Bulk query: option "pairs_bulk_ms" (HIP events around the whole query, the host steps between its
launches included) and the wall time of the call.  Emulation: the sum of "audience_ms" over its count passes and the
filled call (device), and its wall time with the host sort.  At m = 1,024 recommend_top_pairs alternates too
("top_pairs_ms").  The script asserts that the answers are equal -- ids, and scores by their bits -- before it reports.
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


def row_normalised(rng, shape):
    a = rng.random(shape) + 0.01
    return a / a.sum(axis=-1, keepdims=True)


def key_of(x):
    """The order-preserving 64-bit key of a double (pairs_bulk_plan.hpp), as a Python int."""
    b = int(np.float64(x + 0.0).view(np.uint64))
    return (~b) & (2 ** 64 - 1) if b >> 63 else b | (1 << 63)


def value_of(key):
    b = key & ~(1 << 63) if key >> 63 else (~key) & (2 ** 64 - 1)
    return float(np.uint64(b).view(np.float64))


def emulate(em, items, m, lo, hi):
    """(users, items, scores, device ms, count passes): the m best pairs by bisection on the bar.  lo / hi: scores with
    count(lo) >= m and count(hi) < m (the session's smallest rating weight and above its largest)."""
    dev, passes = 0.0, 0

    def count(bar):
        nonlocal dev, passes
        n = int(em.recommend_audience(items, bar, count_only=True)[0][-1])
        dev += em.get_option("audience_ms")
        passes += 1
        return n
    a, b = key_of(lo), key_of(hi)                            # count(a) >= m > count(b)
    while b - a > 1:
        mid = (a + b) // 2
        if count(value_of(mid)) >= m:
            a = mid
        else:
            b = mid
    bar = value_of(a)
    off, us, sc = em.recommend_audience(items, bar)
    dev += em.get_option("audience_ms")
    it = np.repeat(items.astype(np.int64), np.diff(off))
    order = np.lexsort((it, us, -sc))[:m]                   # the host sort and the cut of the ties
    return us[order], it[order], sc[order], dev, passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ms", default="1024,10000,100000,1000000,10000000")
    ap.add_argument("--slots", default="1,8")
    args = ap.parse_args()
    ms_list = [int(x) for x in args.ms.split(",")]
    slot_list = [int(x) for x in args.slots.split(",")]
    print(f"build {_lib.build_id()}", flush=True)
    data = synthetic_triples(N_OBS, USERS, ITEMS, R, seed=0)
    U, I = int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1
    rng = np.random.default_rng(1)
    S_max = max(slot_list)
    params = [(row_normalised(rng, (U, K)), row_normalised(rng, (I, L)), row_normalised(rng, (K, L, R))) for _ in range(S_max)]
    items = np.arange(I, dtype=np.int32)
    w = np.arange(1.0, R + 1)
    with HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R, swap_sides=0, slots=S_max) as em:
        for s, p in enumerate(params):
            em.select(s).set_params(*p)
        for S in slot_list:
            em.recommend_begin(w, True)
            for s in range(S):
                em.select(s).recommend_add()
            for m in ms_list:
                gu, gi, gs, count, info = em.recommend_top_pairs_bulk(m)          # warm-up of each
                eu, ei, es, _, passes = emulate(em, items, m, w.min(), w.max() + 1.0)
                assert count == m == len(eu), (count, len(eu))
                assert np.array_equal(gu, eu) and np.array_equal(gi, ei), "the two routes return different pairs"
                assert np.array_equal(gs.view(np.uint64), es.view(np.uint64)), "the two routes return different score bits"
                if m <= HipEM.MAX_TOP_PAIRS:
                    tu, ti, ts, _ = em.recommend_top_pairs(m)
                    assert np.array_equal(gu, tu) and np.array_equal(gi, ti) and np.array_equal(gs.view(np.uint64), ts.view(np.uint64))
                new, new_wall, old, old_wall, top = [], [], [], [], []
                for _ in range(args.reps):                                       # alternating
                    t0 = time.perf_counter()
                    em.recommend_top_pairs_bulk(m)
                    new_wall.append((time.perf_counter() - t0) * 1e3)
                    new.append(em.get_option("pairs_bulk_ms"))
                    t0 = time.perf_counter()
                    old.append(emulate(em, items, m, w.min(), w.max() + 1.0)[3])
                    old_wall.append((time.perf_counter() - t0) * 1e3)
                    if m <= HipEM.MAX_TOP_PAIRS:
                        em.recommend_top_pairs(m)
                        top.append(em.get_option("top_pairs_ms"))
                med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
                print(json.dumps({
                    "build_id": _lib.build_id(), "users": U, "items": I, "restarts": S, "m": m, "reps": args.reps,
                    "pairs_bulk_ms": med(new), "pairs_bulk_wall_ms": med(new_wall),
                    "passes": int(em.get_option("pairs_bulk_passes")), "collected": int(em.get_option("pairs_bulk_collected")),
                    "emulation_device_ms": med(old), "emulation_wall_ms": med(old_wall), "emulation_count_passes": passes,
                    "top_pairs_ms": med(top) if top else None, "bar": info["bar"], "above": info["above"],
                    "ties": info["ties"], "pairs_bulk_times_ms": [round(x, 3) for x in new], "answers_equal": True}), flush=True)
            em.recommend_end()


if __name__ == "__main__":
    main()
