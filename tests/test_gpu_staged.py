"""The M-step kernels on the parameters a long run ends in: late, border, row-border, tiny, dead-group and subnormal
starts (staged_params.py) through every kernel family, element-wise against the dense oracle.

The other parity files start from orc.init_params or rng.random -- memberships of one magnitude, nothing zero, no row sum
near eps -- and measure in the max-norm, which cannot see a small entry that is wrong by a factor.  Here every cell
(kernel family x shape x stage) checks update_coefficients() at 1e-12 element-wise (and in the max-norm), three
iterations at 1e-11 element-wise, that every returned number is finite and, where the start holds exact zeros, that the
zero pattern is the oracle's (a zero times a finite sum is an exact zero on the device by construction).  The inputs are
unambiguous in the reference alone: test_staged_params_cpu.py.  Each cell asserts from the launch log that the kernels
it is about ran, and records its worst element-wise error; the table is printed when the module is done (-s shows it).
"""
import collections

import numpy as np
import pytest

from conftest import ELEMENT_FLOOR, assert_elementwise, elem_rel_err, rel_err
from oracle import mmsbm_oracle as orc
from staged_params import FAMILIES, staged, uniform_rows
from test_gpu_instantiations import LaunchWindow, hip  # noqa: F401  (hip: the fixture)

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-12     # one update_coefficients call, element-wise
TOL_LOOP = 1e-11     # three iterations, element-wise
ZERO_PATTERN = ("dead", "border")
NAMES = ("theta", "eta", "pr")

WORST = collections.defaultdict(float)     # (kernel family, stage, "step" | "loop") -> worst element-wise error seen


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    def cell(fam, stage):
        return " / ".join(f"{WORST[fam, stage, kind]:.1e}" if (fam, stage, kind) in WORST else "-" for kind in ("step", "loop"))
    print("\nworst element-wise relative error, one step / three iterations")
    print(f"{'kernel family':30s}" + "".join(f"{s:>20s}" for s in FAMILIES))
    for fam in sorted({k[0] for k in WORST if k[2] in ("step", "loop")}):
        print(f"{fam:30s}" + "".join(f"{cell(fam, s):>20s}" for s in FAMILIES))
    for key in sorted(k for k in WORST if k[2] not in ("step", "loop") or k[1] not in FAMILIES):
        print(f"{key[0]:30s} {key[1]:10s} {key[2]:34s} {WORST[key]:.1e}")


def record(fam, stage, kind, err):
    WORST[fam, stage, kind] = max(WORST[fam, stage, kind], err)


# ---- the data of each case: the smallest shapes of the tests that already select each kernel family ----
def rows_for(k, l):
    """About 3,000 rows; 1,500 where the dense oracle's (N, K, L) tensor would pass 100 MB; 700 for rows of more than 1,024 groups."""
    return 700 if max(k, l) > 1024 else 1500 if k * l > 5000 else 3000


def make_data(kind, k, l):
    rng = np.random.default_rng(k * 131 + l)
    if kind == "uniform":
        return uniform_rows(rng, rows_for(k, l), 120, 80, 5), (120, 80, 5)
    if kind == "sparse":      # users with one or two ratings each: no user segment is cut, the tail runs its whole-segment form
        return uniform_rows(rng, 3000, 2000, 300, 5), (2000, 300, 5)
    if kind == "skew":        # test_two_launch_tail_with_unequal_sides: user 11 holds 30 % of 30,000 rows (cut user segments)
        n = 30_000
        u = np.where(rng.random(n) < 0.3, 11, rng.integers(0, 2000, n))
        data = np.stack([u, rng.integers(0, 300, n), rng.integers(0, 5, n)], axis=1).astype(np.int64)
    elif kind == "split":     # test_split_segments_with_wide_rows: one user with ~45 % of the rows, one item with half
        n = 7000
        u = np.where(rng.random(n) < 0.45, 3, np.where(rng.random(n) < 0.3, rng.integers(4, 9, n), rng.integers(9, 400, n)))
        i = np.where(rng.random(n) < 0.5, 1, rng.integers(0, 60, n))
        data = np.stack([u, i, rng.integers(0, 2, n)], axis=1).astype(np.int64)
    elif kind == "busy":      # test_more_than_1024_groups_per_side: user 4 and item 2 with ~ n / 3 triples each (> 64)
        n = rows_for(k, l)
        u = np.where(rng.random(n) < 0.3, 4, rng.integers(0, 30, n))
        i = np.where(rng.random(n) < 0.3, 2, rng.integers(0, 12, n))
        data = np.stack([u, i, rng.integers(0, 3, n)], axis=1).astype(np.int64)
    elif kind in ("r1", "r33"):   # test_many_or_single_rating_values: one rating value / 33 with some unused
        n_r = int(kind[1:])
        r_col = rng.integers(0, n_r, 2500)
        if n_r > 10:
            r_col[r_col % 7 == 3] = 0
        return np.stack([rng.integers(0, 120, 2500), rng.integers(0, 60, 2500), r_col], axis=1).astype(np.int64), (120, 60, n_r)
    else:
        raise ValueError(kind)
    for j in range(3):
        data[:, j] = np.unique(data[:, j], return_inverse=True)[1]
    return data, tuple(int(data[:, j].max()) + 1 for j in range(3))


Ref = collections.namedtuple("Ref", "data dims k l d_u d_i start want_step want_loop")
_DATA, _REFS = {}, {}


def reference(kind, k, l, stage, loops=3):
    """Data, staged start and the oracle's answers of one cell: computed once, shared by the kernel families that run
    the same inputs (two- and four-launch form, vector ALUs and matrix cores), never changed."""
    key = (kind, k, l, stage, loops)
    if key not in _REFS:
        if (kind, k, l) not in _DATA:
            _DATA[kind, k, l] = make_data(kind, k, l)
        data, (n_u, n_i, n_r) = _DATA[kind, k, l]
        d_u, d_i = orc.degrees(data, n_u, n_i)
        rng = np.random.default_rng([k, l, len(stage), ord(stage[0])])
        start = staged(stage, rng, data, n_u, n_i, n_r, k, l)
        want_step = orc.update_coefficients(data, *start)
        t, e, p = start
        for _ in range(loops):
            t, e, p = orc.em_step(data, t, e, p, d_u, d_i)
        for a in start + want_step + (t, e, p):
            a.setflags(write=False)
        _REFS[key] = Ref(data, (n_u, n_i, n_r), k, l, d_u, d_i, start, want_step, (t, e, p))
    return _REFS[key]


def check_against_oracle(em, ref, fam, stage, what, loops=3):
    """One step at 1e-12 and `loops` iterations at 1e-11, element-wise, from the parameters the context holds."""
    step = em.update_coefficients()
    for got, want, nm in zip(step, ref.want_step, NAMES):
        assert np.all(np.isfinite(got)), (what, "n_" + nm)
        err = elem_rel_err(got, want)
        record(fam, stage, "step", err)
        print(f"{fam} {what} {stage} n_{nm}: element-wise {err:.2e}, max-norm {rel_err(got, want):.2e}")
        assert rel_err(got, want) < TOL_STEP, (what, "n_" + nm)
        assert_elementwise(got, want, f"{what} {stage} n_{nm}", rtol=TOL_STEP)
        if stage in ZERO_PATTERN:
            assert np.array_equal(got == 0, want == 0), (what, "n_" + nm)
        if stage == "sub":      # what becomes of results at or below the floor (compared absolutely): kept as subnormals or flushed?
            low = (want != 0) & (np.abs(want) <= ELEMENT_FLOOR)
            if low.any():
                flushed = float(np.mean(got[low] == 0))
                record(fam, stage, "share of sub-floor results returned as 0", flushed)
                print(f"{fam} {what} sub n_{nm}: {int(low.sum())} expected entries at or below the floor, {flushed:.3f} of them returned as exact zeros")
    em.iterate(loops)
    params = em.get_params()
    for got, want, nm in zip(params, ref.want_loop, NAMES):
        assert np.all(np.isfinite(got)), (what, nm)
        err = elem_rel_err(got, want)
        record(fam, stage, "loop", err)
        print(f"{fam} {what} {stage} {nm} after {loops}: element-wise {err:.2e}")
        assert_elementwise(got, want, f"{what} {stage} {nm} after {loops} iterations", rtol=TOL_LOOP)
        if stage in ZERO_PATTERN:
            assert np.array_equal(got == 0, want == 0), (what, nm)
    return step + params


TAIL_WHOLE = ("tail_fused_kernel<", ",false>")


def ran(launched, *wanted):
    """Every entry of `wanted` -- a prefix, or a (prefix, suffix) pair -- names a kernel that was launched."""
    for w in wanted:
        pre, suf = (w, "") if isinstance(w, str) else w
        assert any(n.startswith(pre) and n.endswith(suf) for n in launched), (w, sorted(launched))


def run_cell(hip, ref, fam, stage, swaps, setup, kernels, check=True):
    """One context per side layout: `setup` selects (and asserts) the kernel family, the launch log confirms it."""
    outs = []
    for swap in swaps:
        with LaunchWindow() as lw:
            with hip.HipEM(ref.data, ref.k, ref.l, *ref.dims, swap_sides=swap) as em:
                setup(em)
                em.set_params(*ref.start)
                if check:
                    outs.append(check_against_oracle(em, ref, fam, stage, f"K={ref.k} L={ref.l} swap={swap}"))
                else:
                    step = em.update_coefficients()
                    em.iterate(3)
                    outs.append(step + em.get_params())
            ran(lw.names(), *kernels)
    return outs


def two_launch(em):
    assert em.get_option("launches") == 2.0


def four_launch(em):
    em.set_option("fused", 0)
    assert em.get_option("launches") == 4.0


SMALL = [("uniform", 7, 13, (0, 1)), ("uniform", 20, 20, (0, 1)), ("sparse", 20, 20, (0,)), ("skew", 20, 10, (0,))]
SMALL_IDS = [f"{c[0]}-{c[1]}x{c[2]}" for c in SMALL]


# ---- the two-launch iteration (pairs_fused_kernel + tail_fused_kernel: fused_small.hpp) ----
@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("kind,k,l,swaps", SMALL, ids=SMALL_IDS)
def test_two_launch_iteration(hip, kind, k, l, swaps, stage):
    ref = reference(kind, k, l, stage)

    def setup(em):
        two_launch(em)
        if kind == "skew":
            assert em.get_option("splits_users") > 0 and int(em.get_option("fused_split")) & 2
        if kind == "sparse":
            assert em.get_option("splits_users") == 0 and not int(em.get_option("fused_split")) & 2
    # (the uniform cases' users hold 25 ratings each: their segments go through the tail's work lists, like the skewed
    # ones; the sparse case runs the whole-segment form, tail_fused_kernel<..., false>)
    tail = TAIL_WHOLE if kind == "sparse" else "tail_fused_kernel"
    run_cell(hip, ref, "two-launch iteration", stage, swaps, setup, ("pairs_fused_kernel", tail))


# ---- the four-launch iteration (seg_pass.hpp, the pair stage, eta_p.hpp): against the oracle, and bitwise the two-launch form ----
@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("kind,k,l,swaps", SMALL, ids=SMALL_IDS)
def test_four_launch_iteration(hip, kind, k, l, swaps, stage):
    ref = reference(kind, k, l, stage)
    four = run_cell(hip, ref, "four-launch iteration", stage, swaps, four_launch, ("seg_pass_kernel", "eta_p_kernel"))
    two = run_cell(hip, ref, "", stage, swaps, two_launch, ("tail_fused_kernel",), check=False)
    for a, b in zip(four, two):
        for x, y, nm in zip(a, b, ("n_theta", "n_eta", "n_pr") + NAMES):
            assert np.array_equal(x, y), nm


# ---- restart slots sharing the index stream, every slot in another family: a clamp or a zero row belongs to its slot ----
@pytest.mark.parametrize("k,l,stages", [(10, 10, ("init", "tiny", "rowborder")), (10, 10, ("dead", "late", "border")),
                                        (20, 20, ("init", "tiny", "rowborder", "dead")), (20, 20, ("sub", "border", "late", "tiny"))])
def test_restart_slots_hold_different_families(hip, k, l, stages):
    refs = [reference("uniform", k, l, s) for s in stages]
    ref = refs[0]
    with LaunchWindow() as lw:
        with hip.HipEM(ref.data, k, l, *ref.dims, swap_sides=0, slots=len(stages)) as em:
            em.set_option("fused", 0)
            for s, r in enumerate(refs):
                em.select(s).set_params(*r.start)
            em.iterate(3)
            got = [em.select(s).get_params() for s in range(len(stages))]
        ran(lw.names(), "seg_pass_slots_kernel")
    for s, (r, stage) in enumerate(zip(refs, stages)):
        for g, want, nm in zip(got[s], r.want_loop, NAMES):
            assert np.all(np.isfinite(g)), (stage, nm)
            err = elem_rel_err(g, want)
            record("restart slots", stage if stage in FAMILIES else "init", "loop", err)
            print(f"restart slots K={k} slot {s} {stage} {nm}: element-wise {err:.2e}")
            assert_elementwise(g, want, f"slot {s} ({stage}) {nm}", rtol=TOL_LOOP)
            if stage in ZERO_PATTERN:
                assert np.array_equal(g == 0, want == 0), (stage, nm)
        with hip.HipEM(ref.data, k, l, *ref.dims, swap_sides=0) as one:     # ... and bitwise a one-slot context
            one.set_option("fused", 0)
            one.set_params(*r.start)
            one.iterate(3)
            for a, b, nm in zip(one.get_params(), got[s], NAMES):
                assert np.array_equal(a, b), (stage, nm)


# ---- segments cut into many pieces and combined (seg_combine_both_kernel) ----
@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("k,l", [(100, 4), (400, 2)])
def test_split_segments_and_combine(hip, k, l, stage):
    ref = reference("split", k, l, stage)
    assert ref.d_u.max() > 64 * 32 and np.sum((ref.d_u > 64) & (ref.d_u <= 64 * 32)) >= 2

    def setup(em):
        assert em.get_option("splits_users") >= 3 and em.get_option("splits_pairs") >= 1
    run_cell(hip, ref, "split segments + combine", stage, (0,), setup, ("seg_combine_both_kernel",))


# ---- the pair stage on the matrix cores, one block (pair_mfma_kernel): 36 and 40 reach the 4 x 4 remainder blocks, 60 a padded tile ----
@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("k,l", [(50, 50), (36, 36), (40, 60), (64, 17)])
def test_matrix_cores_one_block(hip, k, l, stage):
    ref = reference("uniform", k, l, stage)

    def setup(em):
        assert em.get_option("mfma") == 1.0
    run_cell(hip, ref, "matrix cores, one block", stage, (0, 1), setup, ("pair_mfma_kernel",))


# ---- ... blocked (mfma_rows_kernel + mfma_slab_kernel) ----
@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("k,l", [(80, 80), (65, 16), (130, 70)])
def test_matrix_cores_blocked(hip, k, l, stage):
    ref = reference("uniform", k, l, stage)

    def setup(em):
        assert em.get_option("mfma") == 2.0
    run_cell(hip, ref, "matrix cores, blocked", stage, (0, 1), setup, ("mfma_rows_kernel", "mfma_slab_kernel"))


# ---- big tiles on the vector ALUs (option mfma = 0): against the oracle and against the matrix cores on the same inputs ----
@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("k,l,kernel", [(92, 92, "pair_block_kernel"), (200, 24, "pair_block_kernel"), (32, 48, "pair_quad_a_kernel")])
def test_big_tiles_on_the_vector_alus(hip, k, l, kernel, stage):
    ref = reference("uniform", k, l, stage)

    def valu(em):
        assert em.get_option("mfma") > 0           # the library's own choice for these tiles: the matrix cores
        em.set_option("mfma", 0)
        assert em.get_option("mfma") == 0.0

    def cores(em):
        assert em.get_option("mfma") > 0
    (vec,) = run_cell(hip, ref, "big tiles on the vector ALUs", stage, (0,), valu, (kernel,))
    (mat,) = run_cell(hip, ref, "", stage, (0,), cores, ("mfma",) if max(k, l) > 64 else ("pair_mfma_kernel",), check=False)
    for a, b, nm in zip(vec, mat, ("n_theta", "n_eta", "n_pr") + NAMES):      # the two forms differ in association order only
        assert rel_err(a, b) < 1e-12, nm


# ---- wide rows (more than 256 groups on one side: 64 lanes x 8 or 16 doubles) ----
@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("k,l", [(300, 24), (600, 5), (8, 520)])
def test_wide_rows(hip, k, l, stage):
    ref = reference("uniform", k, l, stage)

    def setup(em):
        assert em.get_option("wide") == 1.0
    for swap in (0, 1):     # the wide side is the triple passes' row (64 lanes x 8 or 16 doubles) or, on the other side, eta_p's
        inner = l if swap else k
        run_cell(hip, ref, "wide rows", stage, (swap,), setup, ("seg_pass_kernel<64," if inner > 256 else "eta_p_kernel<64,",))


# ---- more than 1,024 groups per side (32 doubles per lane; seg_wide_kernel beyond 2,048), segments longer than a wave's 64 triples ----
@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("k,l", [(1500, 3), (3, 1500), (2100, 2)])
def test_more_than_1024_groups(hip, k, l, stage):
    ref = reference("busy", k, l, stage)
    for swap in (0, 1):     # 32 doubles per lane in the triple passes, or 16 and one more trip per 1,024 columns in eta_p
        inner = l if swap else k
        run_cell(hip, ref, "more than 1,024 groups", stage, (swap,), lambda em: None,
                 ("seg_wide_kernel" if inner > 2048 else "seg_pass_kernel<64,32," if inner > 1024 else ("eta_p_", "kernel<64,16>"),))


# ---- one rating value (p stays 1) and 33 with unused values (several passes of p_update, all-zero p rows of unused ratings) ----
@pytest.mark.parametrize("stage", FAMILIES)
@pytest.mark.parametrize("kind", ["r1", "r33"])
def test_rating_values(hip, kind, stage):
    ref = reference(kind, 5, 6, stage)
    run_cell(hip, ref, "rating values", stage, (0, 1), two_launch, ("tail_fused_kernel",))
    run_cell(hip, ref, "rating values", stage, (0, 1), four_launch, ("eta_p_kernel",))


# ---- the collapse of `tiny`: the reference's parameters underflow to an all-zero model within a few iterations ----
@pytest.mark.parametrize("k,l,form", [(7, 13, "two"), (20, 20, "four"), (50, 50, "cores")])
def test_tiny_collapses_like_the_reference(hip, k, l, form):
    ref = reference("uniform", k, l, "tiny", loops=4)
    assert all(not w.any() for w in ref.want_loop)     # theta' ~ 1e-205, so every omega of the second step underflows
    want_lik = float(orc.compute_likelihood(ref.data, *ref.want_loop))
    with hip.HipEM(ref.data, k, l, *ref.dims, swap_sides=0) as em:
        {"two": two_launch, "four": four_launch, "cores": lambda e: None}[form](em)
        if form == "cores":
            assert em.get_option("mfma") == 1.0
        em.set_params(*ref.start)
        em.iterate(4)
        for got, want, nm in zip(em.get_params(), ref.want_loop, NAMES):
            assert np.all(np.isfinite(got)), nm
            assert_elementwise(got, want, f"{form} {nm}", rtol=TOL_LOOP)
        assert em.likelihood() == pytest.approx(want_lik, abs=1e-12)


# ---- whole subnormal columns (the numerators of one step): rows of the C table that are subnormal throughout, so that
# some results depend on subnormal operands of the pair stage alone -- do the matrix cores keep them? ----
@pytest.mark.parametrize("k,l,form", [(20, 20, "two"), (20, 20, "four"), (50, 50, "cores"), (80, 80, "cores"), (92, 92, "valu")])
def test_whole_subnormal_columns_one_step(hip, k, l, form):
    ref = reference("uniform", k, l, "subcolumn", loops=0)
    with LaunchWindow() as lw:
        with hip.HipEM(ref.data, k, l, *ref.dims, swap_sides=0) as em:
            if form in ("two", "four"):
                {"two": two_launch, "four": four_launch}[form](em)
            else:
                assert em.get_option("mfma") == (1.0 if max(k, l) <= 64 else 2.0)
                if form == "valu":
                    em.set_option("mfma", 0)
            em.set_params(*ref.start)
            got = em.update_coefficients()
        ran(lw.names(), {"two": "pairs_fused_kernel", "four": "seg_pass_kernel", "valu": "pair_block_kernel",
                         "cores": "pair_mfma_kernel" if max(k, l) <= 64 else "mfma_slab_kernel"}[form])
    for g, want, nm in zip(got, ref.want_step, NAMES):
        assert np.all(np.isfinite(g)), nm
        low = (want != 0) & (np.abs(want) <= ELEMENT_FLOOR)
        flushed = float(np.mean(g[low] == 0)) if low.any() else 0.0
        err = elem_rel_err(g, want)
        record(f"whole subnormal columns, {form} {k}x{l}", "n_" + nm, "share of sub-floor results returned as 0", flushed)
        print(f"whole subnormal columns {form} K={k} L={l} n_{nm}: element-wise {err:.2e}; {int(low.sum())} expected entries at or "
              f"below the floor, {flushed:.3f} of them returned as exact zeros")
        assert_elementwise(g, want, f"{form} n_{nm}", rtol=TOL_STEP)


# ---- non-temporal output rows and eta_p in 256-thread workgroups: the two bitwise tests, on dead and row-border starts ----
@pytest.mark.parametrize("stage", ["dead", "rowborder"])
def test_non_temporal_output_rows_change_nothing_on_staged_starts(hip, stage):
    data = orc.synthetic_triples(30_000, 3_000, 700, 5, seed=3)
    dims = tuple(int(data[:, j].max()) + 1 for j in range(3))
    for k, l, fused in ((20, 20, 0), (20, 20, 1), (10, 7, 1), (32, 9, 0)):
        start = staged(stage, np.random.default_rng(k + l), data, *dims, k, l)
        runs = []
        for nt in (1, 0):
            with hip.HipEM(data, k, l, *dims) as em:
                assert em.get_option("nt_out") == 7.0
                em.set_option("nt_out", 7 * nt)
                assert em.get_option("nt_out") == 7.0 * nt
                em.set_option("fused", fused)
                em.set_params(*start)
                em.iterate(6)
                runs.append(em.get_params() + (em.likelihood(),))
        for a, b in zip(*runs):
            assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("stage", ["dead", "rowborder"])
def test_eta_p_in_256_thread_workgroups_is_bitwise_on_staged_starts(hip, stage):
    k = l = 10
    data = orc.synthetic_triples(100_000, 8_000, 20_000, 5, seed=5)
    dims = tuple(int(data[:, j].max()) + 1 for j in range(3))
    starts = [staged(stage if s in (0, 5, 7) else "init", np.random.default_rng(300 + s), data, *dims, k, l) for s in range(8)]
    with LaunchWindow() as lw:
        with hip.HipEM(data, k, l, *dims, swap_sides=0, slots=8) as em:
            em.set_option("fused", 0)
            for s in range(8):
                em.select(s).set_params(*starts[s])
            em.iterate(3)
            eight = [em.select(s).get_params() for s in (0, 5, 7)]
        ran(lw.names(), "eta_p_w4_kernel")
    with LaunchWindow() as lw:
        for j, s in enumerate((0, 5, 7)):
            with hip.HipEM(data, k, l, *dims, swap_sides=0) as one:
                one.set_option("fused", 0)
                one.set_params(*starts[s])
                one.iterate(3)
                for a, b, nm in zip(one.get_params(), eight[j], NAMES):
                    assert np.array_equal(a, b), (s, nm)
        names = lw.names()
        ran(names, "eta_p_kernel")
        assert not any(n.startswith("eta_p_w4_kernel") for n in names)


# ---- prod_dist on late, subnormal and tiny parameters, element-wise: under an atol of 1e-14 a small probability is unseen
# (tiny: every probability is about 1e-220, so only an element-wise measure sees them at all) ----
@pytest.mark.parametrize("stage", ["late", "sub", "tiny"])
@pytest.mark.parametrize("k,l", [(20, 20), (50, 50), (300, 3)])
def test_prod_dist_element_wise(hip, k, l, stage):
    ref = reference("uniform", k, l, stage)
    n_u, n_i, n_r = ref.dims
    test = uniform_rows(np.random.default_rng(k), 1001, n_u, n_i, n_r)
    want = orc.prod_dist(test, *ref.start)
    if stage == "tiny":
        assert ELEMENT_FLOOR < want.min() and want.max() < 1e-200
    with hip.HipEM(ref.data, k, l, *ref.dims) as em:
        em.set_params(*ref.start)
        for fast in (0, 1):
            em.set_option("predict_fast", fast)
            got = em.prod_dist(test)
            err = elem_rel_err(got, want)
            record("prod_dist", stage, f"fast {fast}", err)
            print(f"prod_dist K={k} L={l} {stage} predict_fast={fast}: element-wise {err:.2e} (smallest expected {want.min():.1e})")
            assert np.all(np.isfinite(got))
            assert_elementwise(got, want, f"prod_dist predict_fast={fast}", rtol=1e-12)


# ---- fold-in against staged models: the theta half and the eta half of the same step ----
@pytest.mark.parametrize("stage", ["late", "rowborder", "dead"])
@pytest.mark.parametrize("k,l", [(20, 20), (80, 3), (7, 33)])
def test_fold_in_against_staged_models(hip, k, l, stage):
    ref = reference("uniform", k, l, stage)
    n_u, n_i, n_r = ref.dims
    theta, eta, pr = ref.start
    rng = np.random.default_rng(k * l)
    with hip.HipEM(ref.data, k, l, *ref.dims) as em:
        em.set_params(theta, eta, pr)
        for side, n_old, fold, pick in ((0, n_i, em.fold_in, 0), (1, n_u, em.fold_in_items, 1)):
            degrees = np.array([1, 3, 12, 52, 200])
            new = np.repeat(np.arange(len(degrees)), degrees)
            rows = np.stack([new, rng.integers(0, n_old, len(new)), rng.integers(0, n_r, len(new))], axis=1)
            if side:
                rows = rows[:, [1, 0, 2]]
            rows = np.ascontiguousarray(rows[rng.permutation(len(rows))])
            own = (theta, eta)[side]
            start0 = np.ascontiguousarray(own[rng.integers(0, own.shape[0], len(degrees))])   # staged rows as the new rows' start
            got, its = fold(rows, len(degrees), 1, **{("theta0", "eta0")[side]: start0})
            args = (rows, start0, eta, pr) if side == 0 else (rows, theta, start0, pr)
            want = orc.normalize_with_d(orc.update_coefficients(*args)[pick], degrees)
            err = elem_rel_err(got, want)
            record("fold-in", stage, ("users", "items")[side], err)
            print(f"fold-in K={k} L={l} {stage} side {side}: element-wise {err:.2e}")
            assert np.all(np.isfinite(got)) and (its == 1).all()
            assert_elementwise(got, want, f"fold-in side {side}", rtol=1e-12)
            if stage == "dead":
                assert np.array_equal(got == 0, want == 0)
