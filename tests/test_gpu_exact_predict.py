"""The predict / score session (mmsbm_hip_predict_begin / _add / _finish, mmsbm_hip_prod_dist: predict_score_kernel,
prod_dist_kernel and the seven predict_rows_kernel forms of once_kernels.hpp) on models without rounding
(exact_predict.py), where maxima tie and weighted means land exactly half-way between two ratings -- what the random
models of test_gpu_parity.py never produce.

Everything is compared with the integer reference by EQUALITY: the distributions and the mean bit for bit, the six sums
by ==.  The first maximum, round-half-to-even, the one-off border, the dropped all-zero rows, the workgroup trees and
the host's block-order sums each have one correct answer here.  The only comparisons that are not exact are sums [4]
and [5] of a mean over three slots (one rounding per entry): [5] at the 1e-12 of test_gpu_parity.py against the host
formula on the device's own mean, [4] off that formula by at most the rows whose exact pond is half-way.

The per-row form (predict_fast = 0) and the table form (B = p_r eta_i from the A launch -- lane per pair, matrix cores,
blocked matrix cores, wide rows -- then a group of G lanes per row with group_sum<G> and, beyond 1,024 columns, the tail
loop) run on the same cases and must both give the reference's bits.  That the inputs hold enough ties, half-way
ponds, borders and all-zero rows to tell the wrong rules apart is asserted on the CPU (test_exact_predict_cpu.py).
"""
import numpy as np
import pytest

import exact_predict as xp
from test_gpu_recommend import LaunchWindow, hip  # noqa: F401  (hip: the fixture)

pytestmark = pytest.mark.gpu

WINDOW = {}
PER_ROW = ("predict_score_kernel<false>", "predict_score_kernel<true>", "prod_dist_kernel")


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


def context(hip, case, swap=None, options=()):
    U, I, K, L, R, S = case["shape"]
    em = hip.HipEM(case["data"], K, L, n_users=U, n_items=I, n_ratings=R,
                   swap_sides=case["swap"] if swap is None else swap, slots=S)
    for name, value in options:
        em.set_option(name, value)
    for s, p in enumerate(case["params"]):
        em.select(s).set_params(*p)
    return em


def both_forms(hip, case, what="", swap=None, options=()):
    """prod_dist and one session through the table form and through the per-row form; the kernels launched."""
    with LaunchWindow() as lw:
        em = context(hip, case, swap, options)
        try:
            for fast in (1, 0):
                em.set_option("predict_fast", fast)
                xp.check_prod_dist(em, case, f"{what} predict_fast={fast}")
                xp.check_session(em, case, f"{what} predict_fast={fast}")
        finally:
            em.close()
        return lw.names()


def rows_kernels(G, VEC):
    return [f"predict_rows_kernel<{G},{VEC},{mode}>" for mode in (0, 1)]


def assert_launched(names, wanted):
    missing = [k for k in wanted if k not in names]
    assert not missing, (missing, sorted(names))


def a_launch_forms(names):
    """The forms of the A launch's mat-vec among the launched kernels."""
    return {form for form, prefixes in {
        "lane per pair": ("pair_block_kernel<true,", "pair_quad_a_kernel<"), "matrix cores": ("pair_mfma_kernel<true,",),
        "blocked matrix cores": ("mfma_rows_kernel<true>",), "wide rows": ("wide_matvec_kernel<true>",)}.items()
        if any(n.startswith(prefixes) for n in names)}


# ---- every (G, VEC) form of the rows kernel, both sides of every border of group_code ---------------------------------
@pytest.mark.parametrize("K", xp.FORM_KS)
def test_both_forms_at_every_group_size(hip, K):
    case = xp.make_case(f"K{K}")
    names = both_forms(hip, case)
    assert_launched(names, rows_kernels(*xp.GROUPS_OF_K[K]) + list(PER_ROW))
    padded = -(-K // 4) * 4 if K <= 256 else (-(-K // 8) * 8 if K <= 512 else (-(-K // 16) * 16 if K <= 1024 else -(-K // 32) * 32))
    want = "blocked matrix cores" if padded * 4 > 1024 else "lane per pair"      # (L = 3: rows of 4; 1,024 entries: 8 KB)
    assert want in a_launch_forms(names), (want, sorted(names))


def test_tail_loop_over_a_table_from_the_wide_row_mat_vec(hip):
    """1,040 groups: the columns past 1,024 go through the tail loop; with the matrix cores switched off the table
    comes from the wide-row kernel."""
    case = xp.make_case("K1040")
    names = both_forms(hip, case, "mfma=0", options=[("mfma", 0)])
    assert_launched(names, rows_kernels(64, 16))
    assert a_launch_forms(names) == {"wide rows"}, sorted(names)


def test_table_from_the_one_block_matrix_core_mat_vec(hip):
    names = both_forms(hip, xp.make_case("mfma"))
    assert_launched(names, rows_kernels(16, 4))
    assert "matrix cores" in a_launch_forms(names), sorted(names)


# ---- rating counts on both sides of every block of four, and the clamped load --------------------------------------------
@pytest.mark.parametrize("R", xp.RATING_RS)
def test_rating_counts_around_the_blocks_of_four(hip, R):
    names = both_forms(hip, xp.make_case(f"R{R}"))
    assert_launched(names, rows_kernels(4, 4) + list(PER_ROW))


@pytest.mark.parametrize("name", ["constant", "constantS3", "constantR2", "halfS3", "I1"])
def test_named_cases(hip, name):
    both_forms(hip, xp.make_case(name))


# ---- row counts around the rows of a workgroup ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [(name, n) for name, ns in xp.ROW_COUNTS.items() for n in ns],
                         ids=lambda v: str(v))
def test_row_counts_around_a_workgroup(hip, name, n):
    """PER = 256 / G rows per workgroup of the table form (64 at G = 4, 4 at G = 64), 256 of the per-row kernels:
    1, PER - 1, PER, PER + 1, 3 PER + 1 rows and 255, 256, 257, 513.  Three items, so that the table form is taken
    whatever the row count."""
    case = xp.prefix(xp.make_case(name), n)
    assert case["shape"][1] == 3
    names = both_forms(hip, case, f"{n} rows")
    assert_launched(names, rows_kernels(*{"perrow": (4, 4), "rows64": (64, 4)}[name]) + list(PER_ROW))


def test_an_empty_session_after_a_full_one(hip):
    case = xp.make_case("R5")
    em = context(hip, case)
    try:
        xp.check_session(em, case)
        empty = xp.prefix(case, 0)
        mean, raw = xp.check_session(em, empty, "empty")
        assert mean.shape == (0, 5) and not raw.any()
        xp.check_session(em, case, "after the empty one")
    finally:
        em.close()


# ---- state --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [1, 0])
def test_a_second_session_starts_from_nothing(hip, fast):
    """Two sessions back to back on one context, the first over more rows and with other weights: the second is
    exact, so `first` overwrites the sum buffer and nothing of the earlier session survives."""
    case = xp.make_case("R5")
    other = dict(case, w=xp.weights("stars", 5))
    other["ref"] = xp.exact_session(case["params"], case["rows"], other["w"])
    em = context(hip, case)
    try:
        em.set_option("predict_fast", fast)
        xp.check_session(em, other, "first session")
        for n in (300, len(case["rows"])):
            xp.check_session(em, xp.prefix(case, n), f"second session, {n} rows")
    finally:
        em.close()


@pytest.mark.parametrize("fast", [1, 0])
def test_the_same_slot_twice_and_prod_dist_in_between(hip, fast):
    """A slot added twice gives its own distribution back (2 N / 1024 / 2); prod_dist between two adds releases the
    (item, rating) table the session uses and leaves the session as it was."""
    case = xp.make_case("R7")
    ref, rows, w = case["ref"], case["rows"], case["w"]
    em = context(hip, case)
    try:
        em.set_option("predict_fast", fast)
        em.predict_begin(rows, w)
        for _ in range(2):
            xp.same_sums(em.select(1).predict_add(), ref["slot_sums"][1], "slot 1")
        mean, raw = em.predict_finish()
        xp.same_bits(mean, ref["P"][1], "slot 1 twice")
        xp.same_sums(raw, ref["slot_sums"][1], "sums of slot 1 twice")
        em.predict_begin(rows, w)
        for s in range(3):
            xp.same_sums(em.select(s).predict_add(), ref["slot_sums"][s], f"slot {s}")
            xp.same_bits(em.select((s + 1) % 3).prod_dist(rows[:257]), ref["P"][(s + 1) % 3][:257], "prod_dist in between")
        xp.check_mean(*em.predict_finish(), case, "interleaved")
    finally:
        em.close()


@pytest.mark.parametrize("name", ["swapped", "swappedK70", "R5"])
def test_swapped_and_unswapped_contexts_give_the_same_bits(hip, name):
    case = xp.make_case(name)
    names = {}
    for swap in (0, 1):
        names[swap] = both_forms(hip, case, f"swap_sides={swap}", swap=swap)
    if name == "swappedK70":                                 # internal K = 70 when the sides are swapped, 5 when not
        assert_launched(names[1], rows_kernels(32, 4))
        assert_launched(names[0], rows_kernels(4, 4))


# ---- the host class -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R4", "R7"])
def test_host_predict_and_score_are_the_reference(hip, name):
    """An MMSBM whose results are the exact parameter sets: predict() uploads them one by one (they are not resident,
    test_gpu_parity.test_host_predict_uses_resident_slots_or_uploads) and score() reads the device's sums."""
    case = xp.make_case(name)
    if not np.array_equal(case["w"], np.arange(len(case["w"]))):      # the class weighs with the rating indices
        case = dict(case, w=np.arange(len(case["w"]), dtype=np.float64))
        case["ref"] = xp.exact_session(case["params"], case["rows"], case["w"])
    U, I, K, L, R, S = case["shape"]
    ref = case["ref"]
    mm = hip.MMSBM(K, L, iterations=1, sampling=S, seed=0)
    mm._prepare_objects(case["data"])
    assert mm.ratings == list(range(R)) and (mm.p, mm.m) == (U - 1, I - 1)
    mm.results = [{"theta": t, "eta": e, "pr": p, "likelihood": -1.0 - s} for s, (t, e, p) in enumerate(case["params"])]
    mm._restart_ids = list(range(S))
    mm.data_handler = type("Id", (), {"transform": staticmethod(lambda d, log: d),
                                       "user_labels": lambda s: list(range(U)), "item_labels": lambda s: list(range(I)),
                                       "rating_labels": lambda s: [str(x) for x in range(R)]})()
    try:
        pm = mm.predict(case["rows"])
        stats = mm.score(silent=True)["stats"]
        final = hip.HipEM.final_stats
        xp.check_mean(pm, mm._scored[1], case, "MMSBM.predict")
        assert mm.run_stats == [final(ref["slot_sums"][s]) for s in range(S)]
        best = int(np.argmax([st["accuracy"] for st in mm.run_stats]))
        assert mm.likelihood == -1.0 - best
        want = final(ref["mean_sums"])
        keys = ("accuracy", "one_off_accuracy", "s2") + (("mae", "s2pond") if S & (S - 1) == 0 else ())
        for key in keys:
            assert stats[key] == want[key], (key, stats[key], want[key])
    finally:
        mm._release()


# ---- the launch log: every form the session has ran in this file -----------------------------------------------------------
def test_every_form_of_the_session_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    forms = [f"predict_rows_kernel<{g},{v},{mode}>" for g, v in sorted(set(xp.GROUPS_OF_K.values())) for mode in (0, 1)]
    assert len(forms) == 14
    assert_launched(names, forms + list(PER_ROW))
    assert a_launch_forms(names) == {"lane per pair", "matrix cores", "blocked matrix cores", "wide rows"}, sorted(names)
