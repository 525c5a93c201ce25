"""Held-out log-likelihood on the device (mmsbm_hip_heldout_*, mmsbm_hip_snapshot_*, HipEM.heldout_*, MMSBM.log_likelihood
and the validation-monitored fit) against the numpy restatement of test_heldout_cpu.py.

Row probabilities are compared by their bits where the model carries no rounding (exact_models, family `mixed`); the
log-likelihood of general models within ll_bound -- chain length, one rounded log, the sum -- computed per case from
the restatement.  What the kernels promise beyond that is checked bit for bit: the same value whatever the slot count,
the slot, the call, the side layout; no change to any slot or session; snapshots that return what was saved; a monitored
fit that keeps the parameters of a plain fit stopped at the best check.
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

import exact_models as xm
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip  # noqa: F401  (hip: the module fixture)
from test_heldout_cpu import EPS, ll_bound, random_problem, restate_heldout, restate_ll, restate_p

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW = {}


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


bits = xm.bits

# (name, U, I, R, K, L, option "fused" or None, swap): a fused and a four-launch shape, the matrix-core context
# (K L > 1024), a side of 80 groups, 600 x 5 and its mirror (pieces over k / over l), R = 1, rows of 8 lanes, a tile
# beyond the 64 KB a launch gets unasked, and a tile beyond the LDS with a side beyond 1,024 groups
SHAPES = [
    ("fused", 70, 50, 4, 5, 6, 1, 0),
    ("four_launch", 70, 50, 4, 5, 6, 0, 0),
    ("lanes8", 90, 80, 5, 20, 20, None, 0),
    ("matrix_core", 60, 50, 3, 40, 30, None, 0),
    ("side80", 60, 50, 3, 80, 6, None, 0),
    ("skinny", 40, 30, 3, 600, 5, None, 0),
    ("skinny_l", 40, 30, 3, 4, 700, None, 0),
    ("one_rating", 50, 40, 1, 3, 4, None, 0),
    ("big_tile", 30, 30, 2, 100, 100, None, 0),
    ("no_tile", 24, 20, 2, 1100, 17, None, 0),
]
SHAPE_IDS = [s[0] for s in SHAPES]


def shape_problem(shape, S, M, seed=0):
    name, U, I, R, K, L, fused, swap = shape
    rng = np.random.default_rng([seed, SHAPE_IDS.index(name)])
    params, rows = random_problem(rng, U, I, R, K, L, S, M)
    data = np.stack([rng.integers(0, U, 6 * U), rng.integers(0, I, 6 * U), rng.integers(0, R, 6 * U)], 1)
    return data, params, rows


def shape_context(hip, shape, data, params, swap=None):
    name, U, I, R, K, L, fused, sw = shape
    em = context(hip, data, params, U, I, R, swap=sw if swap is None else swap)
    if fused is not None:
        em.set_option("fused", fused)
        assert em.get_option("launches") == (2 if fused else 4)
    if name == "matrix_core":
        assert em.get_option("mfma") > 0
    return em


def evaluate(em, rows, slots):
    """(eval (n_slots,), [add of each slot], mean_p, mean ll) of one session over `rows`."""
    em.heldout_begin(rows)
    ev = em.heldout_eval()
    adds = [em.select(s).heldout_add() for s in slots]
    mean_p, mean_ll = em.heldout_mean()
    em.heldout_end()
    return ev, adds, mean_p, mean_ll


# ---- 1. per-row mean probability by equality ---------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 4])
@pytest.mark.parametrize("dims", [(300, 997, 7, 9, 5), (120, 200, 20, 17, 4), (50, 60, 70, 3, 3)], ids=str)
def test_mean_p_equals_the_exact_value_by_its_bits(hip, S, dims):
    U, I, K, L, R = dims
    case = xm.make_case("mixed", "stars", (U, I, K, L, R, S), n_random=4 * U)
    rng = np.random.default_rng([S, U])
    M = 3 * 256 + 1 + 37                                   # partial blocks in every rating, no multiple of a block
    rows = np.stack([rng.integers(0, U, M), rng.integers(0, I, M), rng.integers(0, R, M)], 1)
    rows[M - 40:] = rows[:40]                              # repeated rows
    want = restate_heldout(case["params"], rows)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        ev, adds, mean_p, mean_ll = evaluate(em, rows, range(S))
    finally:
        em.close()
    assert np.array_equal(bits(mean_p), bits(want["mean_p"]))
    assert abs(mean_ll - want["mean_ll"]) <= ll_bound(K, L, want["mean_p"])
    for s in range(S):
        assert abs(ev[s] - want["ll"][s]) <= ll_bound(K, L, want["p"][s])


# ---- 2. the log-likelihood against the restatement --------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_log_likelihood_within_the_derived_bound(hip, shape):
    name, U, I, R, K, L, fused, swap = shape
    S = 3
    for M in (1, 2500 + 13):
        data, params, rows = shape_problem(shape, S, M)
        want = restate_heldout(params, rows)
        em = shape_context(hip, shape, data, params)
        try:
            ev, adds, mean_p, mean_ll = evaluate(em, rows, range(S))
        finally:
            em.close()
        for s in range(S):
            bound = ll_bound(K, L, want["p"][s])
            print(f"{name} M={M} slot {s}: |delta| = {abs(ev[s] - want['ll'][s]):.3e}, bound {bound:.3e}")
            assert abs(ev[s] - want["ll"][s]) <= bound
            assert bits(adds[s]) == bits(ev[s])
        assert np.allclose(mean_p, want["mean_p"], rtol=(K * L + 4) * 2.0 ** -52, atol=0)
        assert abs(mean_ll - want["mean_ll"]) <= ll_bound(K, L, want["mean_p"])


def test_more_than_256_blocks_take_the_second_trip_of_the_final_sum(hip):
    """hold_sum_kernel: thread t adds the block sums t, t + 256, ... -- a second trip only beyond 256 blocks, which the
    2,513 rows above (about 14 blocks) never reach.  70,001 rows at R = 4: every rating's run is longer than a block
    and there are more than 256 blocks."""
    shape = SHAPES[SHAPE_IDS.index("four_launch")]
    name, U, I, R, K, L, fused, swap = shape
    S, M = 3, 70_001
    data, params, rows = shape_problem(shape, S, M)
    runs = np.bincount(rows[:, 2], minlength=R)
    assert runs.min() > 256 and int(np.ceil(runs / 256).sum()) > 256
    want = restate_heldout(params, rows)
    em = shape_context(hip, shape, data, params)
    try:
        ev, adds, mean_p, mean_ll = evaluate(em, rows, range(S))
    finally:
        em.close()
    for s in range(S):
        bound = ll_bound(K, L, want["p"][s])
        print(f"{name} M={M} slot {s}: |delta| = {abs(ev[s] - want['ll'][s]):.3e}, bound {bound:.3e}")
        assert abs(ev[s] - want["ll"][s]) <= bound
        assert bits(adds[s]) == bits(ev[s])
    assert np.allclose(mean_p, want["mean_p"], rtol=(K * L + 4) * 2.0 ** -52, atol=0)
    assert abs(mean_ll - want["mean_ll"]) <= ll_bound(K, L, want["mean_p"])
    for s in range(S):                                     # a parameter set alone in a one-slot context == slot s of 3
        one = shape_context(hip, shape, data, [params[s]])
        try:
            ev1, adds1, p1, ll1 = evaluate(one, rows, [0])
        finally:
            one.close()
        assert bits(ev1[0]) == bits(ev[s]) == bits(adds1[0])
        assert abs(ll1 - ev1[0]) <= ll_bound(K, L, p1)     # (the mean of one add: the same logs summed in request order)


# ---- 3. the clamp ----------------------------------------------------------------------------------------------------
def test_impossible_ratings_are_clamped_and_their_mean_p_is_zero(hip):
    U, I, K, L, R = 40, 50, 6, 5, 4
    rng = np.random.default_rng(3)
    model, rows, _ = xm.impossible_rating_case(rng, U, I, K, L, R, [30, 41, 7, 300, 12])
    rows = np.stack([rng.integers(0, U, len(rows)), rows[:, 1], rows[:, 2]], 1)
    data = np.stack([rng.integers(0, U, 300), rng.integers(0, I, 300), rng.integers(0, R, 300)], 1)
    dead = rows[:, 2] == R - 1
    assert dead.sum() > 20 and (~dead).sum() > 20
    want = restate_heldout([model], rows)
    assert (want["p"][0][dead] == 0.0).all()
    em = context(hip, data, [model], U, I, R)
    try:
        ev, adds, mean_p, mean_ll = evaluate(em, rows, [0])
    finally:
        em.close()
    assert (bits(mean_p[dead]) == 0).all() and (mean_p[~dead] > 0).all()
    bound = ll_bound(K, L, want["p"][0])
    assert abs(ev[0] - want["ll"][0]) <= bound and abs(mean_ll - want["mean_ll"]) <= bound
    live = float(np.log(want["p"][0][~dead]).sum())                  # every dead row counts log(eps), no more, no less
    assert abs(ev[0] - (dead.sum() * np.log(EPS) + live)) <= bound


# ---- 4. identities, all bitwise ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 1100 + 7])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_identities_hold_bit_for_bit(hip, shape, M):
    name, U, I, R, K, L, fused, swap = shape
    S = 8
    data, params, rows = shape_problem(shape, S, M, seed=1)
    em = shape_context(hip, shape, data, params)
    try:
        ev, adds, mean_p, mean_ll = evaluate(em, rows, range(S))
        ev2, adds2, mean_p2, mean_ll2 = evaluate(em, rows, range(S))
        perm = np.random.default_rng(5).permutation(M)
        _, _, mean_perm, _ = evaluate(em, rows[perm], range(S))
        only3 = evaluate(em, rows, [3])
    finally:
        em.close()
    assert np.array_equal(bits(ev), bits(np.array(adds)))                          # eval's entry s == add on slot s
    assert np.array_equal(bits(ev), bits(ev2)) and bits(mean_ll) == bits(mean_ll2)  # two calls
    assert np.array_equal(bits(mean_p), bits(mean_p2))
    assert np.array_equal(bits(mean_perm), bits(mean_p[perm]))                      # mean_p follows the request
    # a parameter set alone in a one-slot context == the same set as slot 3 of 8
    one = shape_context(hip, shape, data, [params[3]])
    try:
        ev1, adds1, p1, ll1 = evaluate(one, rows, [0])
    finally:
        one.close()
    assert bits(ev1[0]) == bits(ev[3]) == bits(adds1[0])
    assert np.array_equal(bits(p1), bits(only3[2])) and bits(ll1) == bits(only3[3])
    # a swapped context == an unswapped one, for the same external parameters
    both = []
    for sw in (0, 1):
        em = shape_context(hip, shape, data, params[:2], swap=sw)
        try:
            assert em.swapped == bool(sw)
            both.append(evaluate(em, rows, range(2)))
        finally:
            em.close()
    assert np.array_equal(bits(both[0][0]), bits(both[1][0])) and np.array_equal(bits(both[0][2]), bits(both[1][2]))
    assert bits(both[0][3]) == bits(both[1][3])
    assert np.array_equal(bits(both[0][0]), bits(ev[:2]))


# ---- 5. no side effects -----------------------------------------------------------------------------------------------
def all_params(em, S):
    return [em.select(s).get_params() for s in range(S)]


def same_params(a, b):
    return all(np.array_equal(bits(x), bits(y)) for pa, pb in zip(a, b) for x, y in zip(pa, pb))


def em_problem(shape, S):
    """A context's worth of data and normalised starting parameters an EM iteration is happy with."""
    name, U, I, R, K, L, fused, swap = shape
    rng = np.random.default_rng([7, SHAPE_IDS.index(name)])
    data = np.stack([rng.integers(0, U, 12 * U), rng.integers(0, I, 12 * U), rng.integers(0, R, 12 * U)], 1)
    data[:U, 0], data[:I, 1], data[:R, 2] = np.arange(U), np.arange(I), np.arange(R)
    params, rows = random_problem(rng, U, I, R, K, L, S, 700)
    params = [(t / t.sum(1, keepdims=True), e / e.sum(1, keepdims=True), p) for t, e, p in params]
    return data, params, rows


@pytest.mark.parametrize("shape", SHAPES[:2] + SHAPES[3:4], ids=SHAPE_IDS[:2] + SHAPE_IDS[3:4])
def test_chunked_iteration_equals_the_fixed_length_run(hip, shape):
    """iterate(a); iterate(b) is iterate(a + b), bit for bit -- what the monitored fit rests on."""
    S = 2
    data, params, _ = em_problem(shape, S)
    out = []
    for chunks in ((7,), (3, 4), (1, 1, 5)):
        em = shape_context(hip, shape, data, params)
        try:
            for n in chunks:
                em.iterate(n)
            out.append(all_params(em, S))
        finally:
            em.close()
    assert same_params(out[0], out[1]) and same_params(out[0], out[2])


# the shapes the issue lists (fused, four-launch, K L > 1,024, a side of 80, 600 x 5, R = 1) and the widest side
EM_SHAPES = [sh for sh in SHAPES if sh[0] in ("fused", "four_launch", "matrix_core", "side80", "skinny", "one_rating",
                                              "no_tile")]
EM_IDS = [sh[0] for sh in EM_SHAPES]


@pytest.mark.parametrize("M", [1, 700])
@pytest.mark.parametrize("shape", EM_SHAPES, ids=EM_IDS)
def test_an_evaluation_changes_no_slot_and_no_session(hip, shape, M):
    name, U, I, R, K, L, fused, swap = shape
    S, n = 3, 3
    data, params, rows = em_problem(shape, S)
    w = np.arange(1.0, R + 1)
    test, rows = rows[:200], rows[:M]
    em = shape_context(hip, shape, data, params)
    ref = shape_context(hip, shape, data, params)
    try:
        ref.iterate(2 * n)
        em.iterate(n)
        # open sessions of the three other kinds, asked before and after
        em.recommend_begin(w, True)
        em.similar_begin(0)
        for s in range(S):
            em.select(s).recommend_add()
            em.select(s).similar_add()
        em.predict_begin(test, w)
        first = em.select(0).predict_add()
        rec = em.recommend_query(np.arange(U), 10)
        sim = em.similar_query(np.arange(I), 5)
        em.heldout_begin(rows)
        ev = em.heldout_eval()
        em.select(1).snapshot_save()
        saved = em.select(1).get_params()
        assert np.array_equal(bits(ev), bits(em.heldout_eval()))
        em.select(2).heldout_add()
        rec2 = em.recommend_query(np.arange(U), 10)
        sim2 = em.similar_query(np.arange(I), 5)
        for a, b in zip(rec + sim, rec2 + sim2):
            assert np.array_equal(a, b) if a.dtype.kind == "i" else np.array_equal(bits(a), bits(b))
        second = em.select(1).predict_add()
        matrix, raw = em.predict_finish()
        em.iterate(n)
        assert same_params(all_params(em, S), all_params(ref, S))              # iterate(n), eval, iterate(n) == iterate(2n)
        got = em.select(1).snapshot_get()                                      # ... and the snapshot is what was saved
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, saved))
        assert not same_params([got], [em.select(1).get_params()])
        em.heldout_end()
        em.recommend_end()
        em.similar_end()
    finally:
        em.close()
        ref.close()
    # the predict session gave what one without any held-out call in between gives
    em = shape_context(hip, shape, data, params)
    try:
        em.iterate(n)
        em.predict_begin(test, w)
        f2 = em.select(0).predict_add()
        s2 = em.select(1).predict_add()
        m2, r2 = em.predict_finish()
    finally:
        em.close()
    assert np.array_equal(first, f2) and np.array_equal(second, s2)
    assert np.array_equal(bits(matrix), bits(m2)) and np.array_equal(raw, r2)


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("shape", EM_SHAPES, ids=EM_IDS)
def test_snapshots_return_what_was_saved_whatever_the_side_layout(hip, shape, swap):
    """Every slot's snapshot, saved at different moments, against get_params at its save -- with the wide sides (K = 600,
    1,100: main and tail parts of the slot-interleaved rows) and in a swapped context, whose snapshot_get hands the
    internal tables back as the external theta and eta."""
    S = 3
    data, params, _ = em_problem(shape, S)
    em = shape_context(hip, shape, data, params, swap=swap)
    try:
        assert em.swapped == bool(swap)
        saved = {}
        for s in (2, 0, 1):
            em.select(s).snapshot_save()
            saved[s] = em.select(s).get_params()
            if s == 2:                                                          # nothing yet iterated: what was set
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(saved[s], params[s]))
            em.iterate(2)
        for s in range(S):
            got = em.select(s).snapshot_get()
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, saved[s])), s
            assert not same_params([got], [em.select(s).get_params()])
        em.select(1).snapshot_save()                                            # a later save replaces the slot's own only
        assert same_params([em.select(1).snapshot_get()], [em.select(1).get_params()])
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(em.select(0).snapshot_get(), saved[0]))
    finally:
        em.close()


# ---- 6. the monitored fit ----------------------------------------------------------------------------------------------
def rating_frames(seed=11, n_u=60, n_i=40, n_obs=900, held=250):
    rng = np.random.default_rng(seed)
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"i{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    return df.iloc[held:], df.iloc[:held]


def model(hip, iterations, sampling=3, **kw):
    return hip.MMSBM(4, 3, iterations=iterations, sampling=sampling, seed=5, restarts_per_launch=sampling, **kw)


def test_monitored_fit_keeps_the_parameters_of_a_plain_fit_stopped_at_the_best_check(hip):
    train, held = rating_frames()
    m = model(hip, 22, check_every=5)
    m.fit(train, silent=True, validation=held)
    try:
        checks = [5, 10, 15, 20, 22]
        assert all([it for it, _ in m.validation_curve[i]] == checks for i in range(3))
        assert m.iterations_run == {0: 22, 1: 22, 2: 22}
        plain = {}
        for it in checks:
            p = model(hip, it)
            p.fit(train, silent=True)
            try:
                ctx = p._ctx(0)
                assert ctx.slots == 3
                ctx.heldout_begin(p.data_handler.transform(held, p.logger))
                values = ctx.heldout_eval()
                ctx.heldout_end()
                plain[it] = ([dict(r) for r in p.results], values)
            finally:
                p._release()
        for i in range(3):
            curve = m.validation_curve[i]
            for it, v in curve:
                assert bits(v) == bits(plain[it][1][i]), (i, it)                 # every curve point
            values = [v for _, v in curve]
            best = checks[int(np.argmax(values))]                                # the first of the highest
            assert m.best_iteration[i] == best and m.results[i]["validation"] == max(values)
            for key in ("theta", "eta", "pr"):
                assert np.array_equal(bits(m.results[i][key]), bits(plain[best][0][i][key])), (i, key)
            assert bits(m.results[i]["likelihood"]) == bits(plain[best][0][i]["likelihood"])
        # the model's queries use the kept parameters
        got = m.log_likelihood(held)
        rows = m.data_handler.transform(held, m.logger)
        want = restate_heldout([(r["theta"], r["eta"], r["pr"]) for r in m.results], rows)
        assert got["rows"] == len(rows)
        assert abs(got["log_likelihood"] - want["mean_ll"]) <= ll_bound(4, 3, want["mean_p"])
        for s in range(3):
            assert bits(got["per_restart"][s]) == bits(m.results[s]["validation"])
        assert got["perplexity"] == float(np.exp(-got["log_likelihood"] / len(rows)))
    finally:
        m._release()


def test_patience_stops_the_batch_at_the_stated_check(hip):
    train, held = rating_frames()
    full = model(hip, 60, check_every=3)
    full.fit(train, silent=True, validation=held)
    full._release()
    checks = [it for it, _ in full.validation_curve[0]]
    for patience in (1, 2):
        stale, best, stop = [0] * 3, [None] * 3, checks[-1]
        for c, it in enumerate(checks):
            for i in range(3):
                v = full.validation_curve[i][c][1]
                if best[i] is None or v > best[i]:
                    best[i], stale[i] = v, 0
                else:
                    stale[i] += 1
            if all(s >= patience for s in stale):
                stop = it
                break
        m = model(hip, 60, check_every=3)
        m.fit(train, silent=True, validation=held, patience=patience)
        m._release()
        print(f"patience {patience}: stops after {stop} of 60 iterations")
        if patience == 1:
            assert stop < 60, "no restart stalls on this data: the case shows nothing about stopping early"
        assert m.iterations_run == {0: stop, 1: stop, 2: stop}
        for i in range(3):
            assert m.validation_curve[i] == full.validation_curve[i][:checks.index(stop) + 1]
            assert m.best_iteration[i] == max(m.validation_curve[i], key=lambda x: (x[1], -x[0]))[0]


def test_predict_after_a_monitored_fit_is_predict_after_the_plain_fit(hip):
    train, held = rating_frames(seed=12)
    m = model(hip, 40, sampling=1, check_every=4)
    m.fit(train, silent=True, validation=held)
    p = model(hip, m.best_iteration[0], sampling=1)
    p.fit(train, silent=True)
    try:
        assert np.array_equal(bits(m.predict(held)), bits(p.predict(held)))
        assert m.score(silent=True)["stats"] == p.score(silent=True)["stats"]
    finally:
        m._release()
        p._release()


# ---- 7. refusals by status code, and no rows -----------------------------------------------------------------------------
def refused(hip, code, fn, *args):
    with pytest.raises(hip._lib.HipLibraryError) as e:
        fn(*args)
    assert e.value.code == code, (e.value.code, e.value.message)


def test_refusals_by_status_code_and_an_empty_request(hip):
    shape = SHAPES[1]
    name, U, I, R, K, L, fused, swap = shape
    data, params, rows = shape_problem(shape, 2, 50)
    lib = hip._lib
    em = shape_context(hip, shape, data, params)
    try:
        for call in (em.heldout_eval, em.heldout_add, em.heldout_mean, em.heldout_end):
            refused(hip, lib.E_INVALID, call)                                # no session
        for col, bad in ((0, U), (0, -1), (1, I), (2, R), (2, -1)):
            wrong = rows.copy()
            wrong[7, col] = bad
            if bad < 0:
                with pytest.raises(ValueError):
                    em.heldout_begin(wrong)                                  # (split_triples refuses negative ids itself)
                u, i, r = (np.ascontiguousarray(wrong[:, j], dtype=np.int32) for j in range(3))
                import ctypes as C
                ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
                refused(hip, lib.E_INVALID, lib.call, "mmsbm_hip_heldout_begin", em._h, len(u), ptr(u), ptr(i), ptr(r))
            else:
                refused(hip, lib.E_INVALID, em.heldout_begin, wrong)
        refused(hip, lib.E_INVALID, em.heldout_eval)                          # a refused begin opens nothing
        refused(hip, lib.E_UNSUPPORTED, lib.call, "mmsbm_hip_heldout_begin", em._h, 2 ** 31, None, None, None)
        refused(hip, lib.E_INVALID, em.snapshot_get)                          # nothing saved
        em.heldout_begin(rows)
        refused(hip, lib.E_INVALID, em.heldout_mean)                          # before any add
        first = em.select(1).heldout_add()
        wrong = rows[:5].copy()
        wrong[2, 0] = U
        refused(hip, lib.E_INVALID, em.heldout_begin, wrong)                  # a refused begin leaves the open session alone:
        mean_p, mean_ll = em.heldout_mean()                                   # its rows, its adds, the wrapper's row count
        assert mean_p.shape == (len(rows),) and (mean_p > 0).all()
        assert abs(mean_ll - first) <= ll_bound(K, L, mean_p)
        em.select(0).snapshot_save()
        refused(hip, lib.E_INVALID, em.select(1).snapshot_get)                # nothing saved for THIS slot
        assert all(np.array_equal(a, b) for a, b in zip(em.select(0).snapshot_get(), em.select(0).get_params()))
        em.set_slots(2)                                                       # drops parameters and snapshots ...
        refused(hip, lib.E_INVALID, em.select(0).snapshot_get)
        refused(hip, lib.E_INVALID, em.heldout_eval)                          # ... a slot has no parameters
        refused(hip, lib.E_INVALID, em.snapshot_save)
        em.select(1).set_params(*params[1])
        refused(hip, lib.E_INVALID, em.heldout_eval)                          # slot 0 still has none
        assert bits(em.select(1).heldout_add()) == bits(first)                # ... and keeps the session's rows
        em.heldout_begin(rows[:0])                                            # no rows: the next begin ends the session
        em.select(0).set_params(*params[0])
        assert em.heldout_eval().tolist() == [0.0, 0.0]
        assert em.heldout_add() == 0.0
        mean_p, mean_ll = em.heldout_mean()
        assert mean_p.shape == (0,) and mean_ll == 0.0
        assert em.get_option("heldout_ms") >= 0.0
        em.heldout_end()
        refused(hip, lib.E_INVALID, em.heldout_end)
        em.heldout_begin(rows)
    finally:
        em.close()                                                            # (destroy ends the open session)
    fresh = hip.HipEM(data, K, L, n_users=U, n_items=I, n_ratings=R)
    try:
        fresh.heldout_begin(rows)
        refused(hip, lib.E_INVALID, fresh.heldout_eval)                       # no parameters yet
        refused(hip, lib.E_INVALID, fresh.heldout_add)
        refused(hip, lib.E_INVALID, fresh.snapshot_save)
    finally:
        fresh.close()


# ---- 8. the launch log -------------------------------------------------------------------------------------------------
def test_plain_fit_and_recommend_launch_no_heldout_kernel(hip):
    train, held = rating_frames()
    with LaunchWindow() as lw:
        m = model(hip, 6, check_every=2)
        m.fit(train, silent=True)
        m.recommend(n=5)
        m.predict(held)
        m._release()
        names = lw.names()
    assert names and not [n for n in names if n.startswith("hold_")], sorted(names)


def test_every_heldout_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("hold_")]
    for k in ("hold_sum_kernel", "hold_mean_kernel"):
        assert k in compiled, (k, compiled)
    assert len([k for k in compiled if k.startswith("hold_rows_kernel<")]) == 6, compiled
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
