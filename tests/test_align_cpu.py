"""MMSBM.align_restarts() / consensus() without a GPU: the restatement of the Gram matrix the device computes
(test_gpu_overlap.py compares the device against it) against a triple loop; mmsbm_amd.align.best_assignment against brute
force and scipy; planted relabellings recovered -- after the restatement alone has shown that the optimum is decided;
the aligned mean; and the host class's side through a CPU stand-in that answers the overlap_* calls with the
restatement.

    O[(s G + a), (t G + b)] = sum_row x_s[row, a] x_t[row, b],   x = theta (users, G = K) or eta (items, G = L)"""
import itertools
import math

import numpy as np
import pytest

import exact_models as xm
import fake_device
from mmsbm_amd import align
from test_recommend_cpu import fitted, string_frame

SIDES = ("items", "users")
LONG = np.finfo(np.longdouble).eps < 2.0 ** -60          # an extended type exists (x86: 64 bits of mantissa)


# ---- the restatement ----------------------------------------------------------------------------------------------
def side_tables(params, side):
    """The restarts' membership tables of one side: theta (users) or eta (items) of every (theta, eta, p)."""
    return [np.asarray(p[0] if side == "users" else p[1], dtype=np.float64) for p in params]


def restate_overlap(params, side):
    """The Gram matrix (S G, S G) of the restarts' tables side by side, in np.longdouble where that is wider than a
    double (rounding error <= rows x 2^-64 relative: every term is a product of doubles, exact in 106 bits, summed in
    64), else entry by entry with math.fsum over exact products (fractions)."""
    X = np.concatenate(side_tables(params, side), axis=1)
    if LONG:
        XL = X.astype(np.longdouble)
        return XL.T @ XL
    from fractions import Fraction
    F = X.shape[1]
    cols = [[Fraction(v) for v in X[:, f]] for f in range(F)]
    out = np.zeros((F, F), dtype=np.longdouble)
    for f in range(F):
        for g in range(f, F):
            out[f, g] = out[g, f] = float(sum(a * b for a, b in zip(cols[f], cols[g])))
    return out


def random_params(rng, U, I, K, L, R, S, alpha=0.3):
    """S parameter sets with Dirichlet(alpha) rows."""
    return [(rng.dirichlet(np.full(K, alpha), U), rng.dirichlet(np.full(L, alpha), I),
             rng.dirichlet(np.full(R, 1.0), (K, L))) for _ in range(S)]


@pytest.mark.parametrize("side", SIDES)
def test_restatement_matches_a_triple_loop(side):
    rng = np.random.default_rng(1)
    U, I, K, L, R, S = 7, 5, 3, 2, 2, 3
    params = random_params(rng, U, I, K, L, R, S)
    G, rows = (K, U) if side == "users" else (L, I)
    got = restate_overlap(params, side)
    assert got.shape == (S * G, S * G)
    for s in range(S):
        for t in range(S):
            xs, xt = side_tables(params, side)[s], side_tables(params, side)[t]
            for a in range(G):
                for b in range(G):
                    want = math.fsum(float(xs[row, a]) * float(xt[row, b]) for row in range(rows))
                    assert abs(float(got[s * G + a, t * G + b]) - want) <= 4 * 2.0 ** -52 * want
    assert np.array_equal(got, got.T)


# ---- best_assignment: the optimum ----------------------------------------------------------------------------------
def total(M, col):
    return M[np.arange(len(col)), col].sum()


def is_permutation(col, G):
    return col.dtype == np.int64 and sorted(col.tolist()) == list(range(G))


def brute_totals(M):
    G = len(M)
    return sorted((sum(M[k, p[k]] for k in range(G)) for p in itertools.permutations(range(G))), reverse=True)


@pytest.mark.parametrize("G", range(1, 8))
def test_best_assignment_reaches_the_brute_force_optimum(G):
    rng = np.random.default_rng(G)
    for rep in range(12):
        if rep % 3 == 0:
            M = rng.random((G, G))
        elif rep % 3 == 1:
            M = rng.integers(0, 3, (G, G)).astype(np.float64)        # many ties
        else:
            M = rng.integers(-4, 5, (G, G)).astype(np.float64)
        col = align.best_assignment(M)
        assert is_permutation(col, G)
        tops = brute_totals(M)
        assert abs(total(M, col) - tops[0]) <= 1e-12 * max(1.0, abs(tops[0])), (G, rep)
        assert np.array_equal(col, align.best_assignment(M.copy()))  # deterministic
        margin = align.assignment_margin(M)
        if G == 1:
            assert margin == np.inf
        else:                                                        # the second best, exactly
            assert abs(margin - (tops[0] - tops[1])) <= 1e-12 * max(1.0, abs(tops[0])), (G, rep)


@pytest.mark.parametrize("G", [2, 8, 20, 33, 64, 65, 128, 129])
def test_best_assignment_agrees_with_scipy_on_integer_matrices(G):
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(100 + G)
    for hi in (2, 50, 10_000):
        M = rng.integers(0, hi, (G, G)).astype(np.float64)
        col = align.best_assignment(M)
        assert is_permutation(col, G)
        r, c = opt.linear_sum_assignment(M, maximize=True)
        assert total(M, col) == M[r, c].sum(), (G, hi)


def test_best_assignment_traps():
    assert align.best_assignment(np.array([[3.5]])).tolist() == [0]
    assert align.best_assignment(np.zeros((1, 1))).tolist() == [0]
    M = np.array([[0.0, 0.0, 0.0], [1.0, 5.0, 2.0], [4.0, 6.0, 1.0]])     # a zero row
    col = align.best_assignment(M)
    assert is_permutation(col, 3) and total(M, col) == 9.0
    col = align.best_assignment(M.T.copy())                               # a zero column
    assert is_permutation(col, 3) and total(M.T, col) == 9.0
    assert is_permutation(align.best_assignment(np.zeros((5, 5))), 5)     # nothing to choose by
    # greedy takes 10 first and ends at 10 + 1; the optimum is 9 + 9
    assert align.best_assignment(np.array([[10.0, 9.0], [9.0, 1.0]])).tolist() == [1, 0]
    for bad in (np.zeros((2, 3)), np.zeros(4), np.array([[np.nan]])):
        with pytest.raises(ValueError):
            align.best_assignment(bad)


def test_group_cosine():
    rng = np.random.default_rng(3)
    x, y = rng.random((50, 4)), rng.random((50, 4))
    y[:, 2] = 0.0                                                         # a group nobody is in
    X = np.concatenate([x, y], axis=1)
    O = X.T @ X
    col = np.array([1, 2, 3, 0])
    got = align.group_cosine(O, 4, 0, 1, col)
    for k in range(4):
        den = np.linalg.norm(x[:, k]) * np.linalg.norm(y[:, col[k]])
        assert got[k] == 0.0 if den == 0 else abs(got[k] - x[:, k] @ y[:, col[k]] / den) < 1e-14
    assert got[1] == 0.0 and ((got >= 0) & (got <= 1)).all()
    assert np.allclose(align.group_cosine(O, 4, 0, 0, np.arange(4)), 1.0, atol=1e-15)


# ---- planted relabellings --------------------------------------------------------------------------------------------
PLANTED = [(300, 7, 0), (260, 9, 1), (2000, 20, 2), (1021, 65, 3), (997, 129, 4)]     # (rows, G, seed)
MARGIN = 1e-4                                                                          # of rows


def planted_tables(rows, G, seed):
    """(x0, copy, noisy, pi): Dirichlet(0.3) rows, x0 with its columns permuted by pi, and 0.9 of that + 0.1 noise."""
    rng = np.random.default_rng(seed)
    x0 = rng.dirichlet(np.full(G, 0.3), rows)
    pi = rng.permutation(G)
    noise = rng.dirichlet(np.full(G, 0.3), rows)
    return x0, np.ascontiguousarray(x0[:, pi]), 0.9 * x0[:, pi] + 0.1 * noise, pi


def planted_params(rows, G, seed, side):
    """The three tables as the `side` tables of three parameter sets (the other side: 3 rows, 2 groups)."""
    rng = np.random.default_rng(seed + 1000)
    tabs = planted_tables(rows, G, seed)
    out = []
    for x in tabs[:3]:
        o = rng.dirichlet(np.full(2, 0.3), 3)
        p = rng.dirichlet(np.ones(2), (G, 2) if side == "users" else (2, G))
        out.append((x, o, p) if side == "users" else (o, x, p))
    return out, tabs[3]


def assert_decided(block, rows, what):
    """From the restatement alone: the optimum of `block` beats the exact second-best assignment by more than
    MARGIN x rows."""
    margin = align.assignment_margin(np.asarray(block, dtype=np.float64))
    print(f"{what}: margin {margin / rows:.3e} of rows")
    assert margin > MARGIN * rows, (what, margin / rows)


@pytest.mark.parametrize("rows,G,seed", PLANTED)
def test_planted_relabellings_are_recovered(rows, G, seed):
    params, pi = planted_params(rows, G, seed, "users")
    want = np.argsort(pi)                     # column b of the copy is column pi[b] of x0: group a sits at pi^-1[a]
    x0 = params[0][0]
    # an exact copy: the planted matching is the optimum (rearrangement inequality), the only one iff no two columns
    # of x0 are equal
    assert len(np.unique(x0.T, axis=0)) == G
    O = restate_overlap(params, "users")
    for t, name in ((1, "copy"), (2, "noisy")):
        blk = align.block(O, G, 0, t)
        assert_decided(blk, rows, f"rows={rows} G={G} {name}")
        got = align.best_assignment(np.asarray(blk, dtype=np.float64))
        assert np.array_equal(got, want), name
        cos = align.group_cosine(np.asarray(O, dtype=np.float64), G, 0, t, got)
        assert (cos > (1 - 1e-12 if t == 1 else 0.9)).all()


# ---- consensus_params ------------------------------------------------------------------------------------------------
def test_aligned_copies_average_back_to_the_restart_bit_for_bit():
    rng = np.random.default_rng(5)
    U, I, K, L, R, S = 40, 30, 5, 4, 3, 4                                 # S a power of two: the division is exact
    theta, eta, pr = random_params(rng, U, I, K, L, R, 1)[0]
    ug = np.stack([np.arange(K)] + [rng.permutation(K) for _ in range(S - 1)])
    ig = np.stack([np.arange(L)] + [rng.permutation(L) for _ in range(S - 1)])
    results = []
    for s in range(S):                        # restart s holds group k of the reference at ug[s, k]
        t, e, p = np.empty_like(theta), np.empty_like(eta), np.empty_like(pr)
        t[:, ug[s]] = theta
        e[:, ig[s]] = eta
        p[np.ix_(ug[s], ig[s])] = pr
        results.append({"theta": t, "eta": e, "pr": p})
    got = align.consensus_params(results, ug, ig)
    for a, b in zip(got, (theta, eta, pr)):
        assert np.array_equal(xm.bits(a), xm.bits(b))
    with pytest.raises(ValueError):
        align.consensus_params(results, ug[:2], ig)


def test_the_aligned_mean_is_a_model():
    rng = np.random.default_rng(6)
    U, I, K, L, R, S = 60, 50, 6, 5, 4, 3
    params = random_params(rng, U, I, K, L, R, S, alpha=1.0)
    results = [{"theta": t, "eta": e, "pr": p} for t, e, p in params]
    ug = np.stack([rng.permutation(K) for _ in range(S)])
    ig = np.stack([rng.permutation(L) for _ in range(S)])
    theta, eta, pr = align.consensus_params(results, ug, ig)
    assert theta.shape == (U, K) and eta.shape == (I, L) and pr.shape == (K, L, R)
    for a in (theta, eta, pr):
        assert np.abs(a.sum(axis=-1) - 1.0).max() <= 4 * 2.0 ** -52
        assert (a >= 0).all() and (a <= 1).all()
    k, l, r = 2, 3, 1
    want = (params[0][2][ug[0, k], ig[0, l], r] + params[1][2][ug[1, k], ig[1, l], r]
            + params[2][2][ug[2, k], ig[2, l], r]) / 3
    assert pr[k, l, r] == want


# ---- the CPU stand-in ---------------------------------------------------------------------------------------------------
class OverlapFakeHipEM(fake_device.FakeHipEM):
    """FakeHipEM with the overlap session, answered by the restatement (rounded to doubles)."""
    _ov = None

    def overlap_begin(self, side):
        side = {0: "items", 1: "users"}.get(side, side)
        assert side in SIDES
        self._ov = {"side": side, "params": []}
        fake_device.LOG.append(("overlap_begin", side))

    def overlap_add(self):
        self._ov["params"].append(self.get_params())
        fake_device.LOG.append(("overlap_add", self._sel))

    def overlap_query(self):
        assert self._ov["params"], "overlap_query before overlap_add"
        fake_device.LOG.append(("overlap_query", len(self._ov["params"])))
        return np.asarray(restate_overlap(self._ov["params"], self._ov["side"]), dtype=np.float64)

    def overlap_end(self):
        self._ov = None
        fake_device.LOG.append(("overlap_end", None))


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", OverlapFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(OverlapFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def model_params(m):
    return [(r["theta"], r["eta"], r["pr"]) for r in m.results]


def snapshot(m):
    return [{k: np.array(v, copy=True) for k, v in r.items() if k in ("theta", "eta", "pr", "likelihood")} for r in m.results]


def check_alignment(m, out, reference):
    S, K, L = len(m.results), m.results[0]["theta"].shape[1], m.results[0]["eta"].shape[1]
    assert out["reference"] == reference
    for side, G, rows in (("user", K, m.p + 1), ("item", L, m.m + 1)):
        O = np.asarray(restate_overlap(model_params(m), side + "s"), dtype=np.float64)
        groups, sim, agree = out[side + "_groups"], out[side + "_similarity"], out[side + "_agreement"]
        assert groups.shape == (S, G) and groups.dtype == np.int64 and sim.shape == (S, G) and agree.shape == (S, S)
        assert groups[reference].tolist() == list(range(G)) and (sim[reference] == 1.0).all()
        for s in range(S):
            assert is_permutation(groups[s], G)
            blk = align.block(O, G, reference, s)
            assert abs(total(blk, groups[s]) - brute_totals(blk)[0]) <= 1e-12 * rows
            if s != reference:
                assert np.array_equal(sim[s], align.group_cosine(O, G, reference, s, groups[s]))
            for t in range(S):
                assert abs(agree[s, t] - brute_totals(align.block(O, G, s, t))[0] / rows) <= 1e-12
        assert ((sim >= 0) & (sim <= 1)).all()
        assert np.array_equal(agree, agree.T) and (agree > 0).all() and (agree <= 1 + 1e-12).all()


def test_string_labels_and_the_default_reference(host):
    df = string_frame()
    m = fitted(host, df, sampling=3)
    m.predict(df.iloc[:40])
    before_stats, before = m.score(silent=True)["stats"], snapshot(m)
    best = int(np.argmax([r["likelihood"] for r in m.results]))
    out = m.align_restarts()
    check_alignment(m, out, best)
    for a, b in zip(before, snapshot(m)):                                  # self.results is untouched
        for key in a:
            assert np.array_equal(a[key], b[key])
    assert m.score(silent=True)["stats"] == before_stats                  # and so are the stored predictions
    events = [e for e, _ in fake_device.LOG if e.startswith("overlap")]
    assert events == (["overlap_begin"] + ["overlap_add"] * 3 + ["overlap_query", "overlap_end"]) * 2
    assert [d for e, d in fake_device.LOG if e == "overlap_begin"] == ["users", "items"]

    cons = m.consensus()
    enc = m.data_handler
    assert cons["alignment"]["reference"] == best
    assert list(cons["theta"].index) == list(enc.user_labels()) and cons["theta"].shape == m.theta.shape
    assert list(cons["eta"].index) == list(enc.item_labels()) and cons["eta"].shape == m.eta.shape
    assert list(cons["pr"]) == list(m.pr) and all(cons["pr"][k].shape == m.pr[k].shape for k in m.pr)
    want = align.consensus_params(m.results, out["user_groups"], out["item_groups"])
    assert np.array_equal(cons["theta"].to_numpy(), want[0]) and np.array_equal(cons["eta"].to_numpy(), want[1])
    for j, lab in enumerate(cons["pr"]):
        assert np.array_equal(cons["pr"][lab].to_numpy(), want[2][:, :, j])
    assert np.abs(cons["theta"].to_numpy().sum(axis=1) - 1).max() <= 4 * 2.0 ** -52


def test_ties_in_the_likelihood_go_to_the_lowest_position(host):
    m = fitted(host, string_frame(), sampling=3)
    top = max(r["likelihood"] for r in m.results)
    for r in m.results[1:]:
        r["likelihood"] = top
    m.results[0]["likelihood"] = top - 1.0
    assert m.align_restarts()["reference"] == 1


def test_an_explicit_reference_and_one_out_of_range(host):
    m = fitted(host, string_frame(), sampling=3)
    for ref in (0, 2, np.int64(1)):
        check_alignment(m, m.align_restarts(reference=ref), int(ref))
    assert m.consensus(reference=2)["alignment"]["reference"] == 2
    fake_device.LOG.clear()
    for bad in (3, -1, 17):
        with pytest.raises(ValueError, match="position"):
            m.align_restarts(reference=bad)
        with pytest.raises(ValueError, match="position"):
            m.consensus(reference=bad)
    for bad in (1.0, "0", True):
        with pytest.raises(ValueError):
            m.align_restarts(reference=bad)
    assert not [e for e, _ in fake_device.LOG if e.startswith("overlap")]    # refused before any device call


def test_one_restart_is_aligned_with_itself(host):
    m = fitted(host, string_frame(), sampling=1)
    out = m.align_restarts()
    K, L = m.results[0]["theta"].shape[1], m.results[0]["eta"].shape[1]
    assert out["reference"] == 0
    assert out["user_groups"].tolist() == [list(range(K))] and out["item_groups"].tolist() == [list(range(L))]
    assert (out["user_similarity"] == 1.0).all() and (out["item_similarity"] == 1.0).all()
    assert out["user_agreement"].shape == (1, 1) and out["item_agreement"].shape == (1, 1)
    cons = m.consensus()
    assert np.array_equal(cons["theta"].to_numpy(), m.results[0]["theta"])
    assert np.array_equal(cons["eta"].to_numpy(), m.results[0]["eta"])


def test_a_relabelled_restart_is_matched_back(host):
    m = fitted(host, string_frame(n_obs=400), sampling=2)
    r0 = m.results[0]
    m.results[1] = {**m.results[1], "theta": r0["theta"][:, [1, 0]].copy(), "eta": r0["eta"][:, [2, 0, 1]].copy(),
                    "pr": r0["pr"][[1, 0]][:, [2, 0, 1]].copy()}
    m._resident.clear()                       # (the stand-in's slots hold the fitted parameters, not these)
    assert len(np.unique(r0["theta"].T, axis=0)) == 2 and len(np.unique(r0["eta"].T, axis=0)) == 3
    out = m.align_restarts(reference=0)
    assert out["user_groups"].tolist() == [[0, 1], [1, 0]]
    assert out["item_groups"].tolist() == [[0, 1, 2], [1, 2, 0]]
    assert np.allclose(out["user_similarity"], 1.0, atol=1e-12) and np.allclose(out["item_similarity"], 1.0, atol=1e-12)
    cons = m.consensus(reference=0)                                       # S = 2: the mean of two equal values is exact
    assert np.array_equal(cons["theta"].to_numpy(), r0["theta"]) and np.array_equal(cons["eta"].to_numpy(), r0["eta"])
    for j, lab in enumerate(cons["pr"]):
        assert np.array_equal(cons["pr"][lab].to_numpy(), r0["pr"][:, :, j])


def test_ids_after_fit_encoded(host):
    rng = np.random.default_rng(2)
    train = np.stack([rng.integers(0, 9, 80), rng.integers(0, 11, 80), rng.integers(0, 4, 80)], 1)
    train[:9, 0], train[:11, 1], train[:4, 2] = np.arange(9), np.arange(11), np.arange(4)
    m = host.MMSBM(2, 3, iterations=3, sampling=2, seed=7)
    m.fit_encoded(train)
    cons = m.consensus()
    assert cons["theta"].shape == (9, 2) and cons["eta"].shape == (11, 3) and list(cons["pr"]) == [0, 1, 2, 3]
    check_alignment(m, cons["alignment"], cons["alignment"]["reference"])


def test_the_session_ends_when_a_query_fails(host, monkeypatch):
    m = fitted(host, string_frame())

    def broken(self):
        raise RuntimeError("device lost")
    monkeypatch.setattr(OverlapFakeHipEM, "overlap_query", broken)
    for call in (m.align_restarts, m.consensus):
        fake_device.LOG.clear()
        with pytest.raises(RuntimeError, match="device lost"):
            call()
        assert [e for e, _ in fake_device.LOG][-1] == "overlap_end"


def test_distributed_share_is_refused(host):
    m = fitted(host, string_frame(), sampling=3)
    m._restart_ids = m._restart_ids[:1]                                  # what fit_distributed(gather=False) leaves on a rank
    m.results = m.results[:1]
    for call in (m.align_restarts, m.consensus):
        with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
            call()


def test_an_unfitted_model_is_refused(host):
    with pytest.raises(AssertionError, match="fit the model"):
        host.MMSBM(2, 3).align_restarts()


def test_the_binding_declares_the_session():
    from mmsbm_amd import _lib
    from mmsbm_amd.core import HipEM
    for name in ("begin", "add", "query", "end"):
        assert "mmsbm_hip_overlap_" + name in _lib.SIGNATURES
        assert callable(getattr(HipEM, "overlap_" + name))
