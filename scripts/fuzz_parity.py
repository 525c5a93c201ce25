"""Randomised parity fuzz (not part of the test suite): random shapes, degrees, slot counts and kernel-family
options against the dense oracle -- numerators after one step, parameters after a few iterations, likelihood in all
three device forms, prod_dist; and, one case in four, the serving kernels on a model family of tests/exact_models.py at
random sizes -- top-N lists, scores (by their bits), counts and positions EQUAL to the exact reference.
usage: python scripts/fuzz_parity.py [seconds] [seed]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
from mmsbm_amd import HipEM
from oracle import mmsbm_oracle as orc
import exact_models as xm

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 240.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)


def rel(a, b):
    m = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (m if m > 0 else 1.0))


def serving_case(rng):
    """One exact-model session: None when the device equals the exact reference, else what differs."""
    family, kind = xm.FAMILIES[rng.integers(len(xm.FAMILIES))], xm.WEIGHT_KINDS[rng.integers(len(xm.WEIGHT_KINDS))]
    few = rng.random() < 0.3                           # few users over many items: the split across waves + the merge
    U, I = (int(rng.integers(1, 4)), int(rng.integers(1100, 30000))) if few else (int(rng.integers(1, 400)), int(rng.integers(20, 3000)))
    shape = (U, I, int(rng.integers(2, 10)), int(rng.integers(2, 10)), int(rng.integers(2, 7)), int(rng.integers(1, 5)))
    case = xm.make_case(family, kind, shape, n_random=int(rng.integers(1, 30 * U + 2)))
    swap, exclude = int(rng.integers(-1, 2)), bool(rng.integers(0, 2))
    tag = f"serving {family}/{kind} U={U} I={I} K={shape[2]} L={shape[3]} R={shape[4]} S={shape[5]} swap={swap} exclude={exclude}"
    seen = case["seen"] if exclude else None
    off, items = xm.position_lists(rng, case["scores"], seen, lengths=tuple(int(x) for x in rng.choice([0, 1, 4, 5, 16, 17, 33, 200], 3)))
    ns = sorted({1, int(rng.integers(1, 1025)), int(rng.integers(1, 1025)), 1024})
    with HipEM(case["data"], shape[2], shape[3], U, I, shape[4], slots=shape[5], swap_sides=swap) as em:
        for s, p in enumerate(case["params"]):
            em.select(s).set_params(*p)
        em.recommend_begin(case["w"], exclude)
        for s in range(shape[5]):
            em.select(s).recommend_add()
        got = {n: em.recommend_query(case["users"], n) for n in ns}
        pos = em.recommend_positions(case["users"], off, items)
        em.recommend_end()
    top = xm.exact_top_n(case["scores"], case["users"], 1024, seen)
    for n in ns:
        wi, ws, wc = xm.first_n(top, n)
        gi, gs, gc = got[n]
        if not (np.array_equal(gi, wi) and np.array_equal(xm.bits(gs), xm.bits(ws)) and np.array_equal(gc, wc)):
            return tag, f"top-{n} differs"
    want = xm.exact_positions(case["scores"], off, items, case["users"].tolist(), seen)
    if not (np.array_equal(pos[0], want[0]) and np.array_equal(pos[1], want[1])):
        return tag, "positions differ"
    return tag, None


t0, cases, serving, worst = time.time(), 0, 0, 0.0
while time.time() - t0 < budget:
    if rng.random() < 0.25:
        tag, bad = serving_case(rng)
        cases += 1
        serving += 1
        if bad:
            print(f"MISMATCH {tag}: {bad}", flush=True)
            sys.exit(1)
        continue
    kind = rng.integers(0, 10)
    if kind < 6:
        k, l = int(rng.integers(1, 26)), int(rng.integers(1, 26))
    elif kind < 9:
        k, l = int(rng.integers(1, 90)), int(rng.integers(1, 90))
    else:
        k, l = (int(rng.integers(200, 1300)), int(rng.integers(1, 6)))[:: 1 if rng.random() < 0.5 else -1]
    n_u, n_i, n_r = int(rng.integers(1, 400)), int(rng.integers(1, 200)), int(rng.integers(1, 9))
    n = int(rng.integers(1, 6000)) if k * l < 4000 else int(rng.integers(1, 600))
    shape = rng.random()
    if shape < 0.25 and k * l <= 700:   # few busy users, popular items (the MovieLens-100k shape in small): segments cut into
        n = int(rng.integers(3000, 30000))   # pieces on both sides -- whole-segment lists of the two-launch form (round 4)
        n_u, n_i = int(rng.integers(20, 400)), int(rng.integers(20, 600))
        pu, pi = rng.lognormal(0, rng.uniform(0.3, 1.5), n_u), rng.lognormal(0, rng.uniform(0.3, 2.0), n_i)
        u_col, i_col = rng.choice(n_u, n, p=pu / pu.sum()), rng.choice(n_i, n, p=pi / pi.sum())
    elif shape < 0.5:   # skewed degrees
        u_col = (rng.zipf(1.3, n) - 1) % n_u
        i_col = (rng.zipf(1.3, n) - 1) % n_i
    else:
        u_col, i_col = rng.integers(0, n_u, n), rng.integers(0, n_i, n)
    data = np.stack([u_col, i_col, rng.integers(0, n_r, n)], axis=1).astype(np.int64)
    d_u, d_i = orc.degrees(data, n_u, n_i)
    theta, eta, pr = orc.init_params(int(rng.integers(0, 1 << 30)), n_u, n_i, n_r, k, l, d_u, d_i)
    if rng.random() < 0.3:   # concentrated memberships: clamps in the likelihood
        theta = theta ** rng.integers(1, 30, theta.shape); eta = eta ** rng.integers(1, 30, eta.shape)
    slots, swap, iters = int(rng.integers(1, 4)), int(rng.integers(-1, 2)), int(rng.integers(1, 4))
    want = orc.update_coefficients(data, theta, eta, pr)
    t, e, p = theta, eta, pr
    for _ in range(iters):
        t, e, p = orc.em_step(data, t, e, p, d_u, d_i)
    lik = float(orc.compute_likelihood(data, t, e, p))
    tag = f"K={k} L={l} N={n} U={n_u} I={n_i} R={n_r} slots={slots} swap={swap} iters={iters}"
    with HipEM(data, k, l, n_u, n_i, n_r, slots=slots, swap_sides=swap) as em:
        fused = em.get_option("fused") + 10 * em.get_option("fused_split")
        if em.get_option("fused") and rng.random() < 0.3:
            em.set_option("fused", 0)
        if em.get_option("mfma") and rng.random() < 0.2:
            em.set_option("mfma", 0)
        sel = int(rng.integers(0, slots))
        for s in range(slots):
            em.select(s).set_params(theta * (1.0 if s == sel else 0.5 + 0.1 * s), eta, pr)
        em.select(sel)
        errs = [rel(g, w) for g, w in zip(em.update_coefficients(), want)]
        em.iterate(iters)
        errs += [rel(g, w) for g, w in zip(em.get_params(), (t, e, p))]
        for mode in (2, 1, 0):
            em.set_option("lik_fast", mode)
            got = em.likelihood()
            # (K = L = 1: the likelihood is exactly 0; every form subtracts per element, as the reference does)
            errs.append(abs(got - lik) / max(abs(lik), 1e-6 * n))
        rows = data[: min(n, 200)]
        errs.append(rel(em.prod_dist(rows), orc.prod_dist(rows, t, e, p)))
    bad = max(errs)
    worst = max(worst, bad)
    cases += 1
    if bad > 1e-10 or not np.isfinite(bad):
        print(f"MISMATCH {tag} fused={fused}: {errs}", flush=True)
        sys.exit(1)
    if cases % 50 == 0:
        print(f"{cases} cases, worst relative error {worst:.2e}  [{time.time() - t0:.0f}s]  last: {tag}", flush=True)
print(f"done: {cases} cases ({serving} of them serving sessions, each equal to the exact reference), worst relative error {worst:.2e}")
