"""The EM step on triple tables built at the borders of the index (border_tables.py), element-wise against np.longdouble.

Every other training table of the suite is a random draw; which side of a border of the kernels' index arithmetic it
reaches -- a segment of exactly one chunk of indices, of 32 or 33 pieces, a rating of 320 or 328 slabs, an (item,
rating) grid exactly half full -- is chance.  The tables here sit on those borders by construction (asserted on the CPU
by test_border_tables_cpu.py, listed by file and line in DESIGN section 6).  Per table and kernel form: one
update_coefficients() at 1e-12 element-wise, three iterations at 1e-11, the likelihood at its 1e-12 / 1e-11, against the
long-double restatement of the M-step; every case asserts from the launch log or from get_option that the form it is
named after ran.  On `segments` the error is reported per segment length: a wrong last chunk reads "length 65".  Then
the bitwise contracts on these tables (two launches = four, slot s = a one-slot context, graph = eager, nt_out, a_units,
256- = 1,024-thread eta_p, no item grid = item grid, device-built = host-built index) and the later consumers of the
same index (every likelihood form, compute_omegas, a predict session).  Worst errors are printed when the module is
done (-s shows them).
"""
import collections

import numpy as np
import pytest

import border_tables as bt
import staged_after_fit as saf
from conftest import ELEMENT_FLOOR, elem_rel_err
from oracle import mmsbm_oracle as orc
from test_gpu_instantiations import LaunchWindow, hip  # noqa: F401  (hip: the fixture)
from test_gpu_staged import four_launch, ran, two_launch

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-12     # one update_coefficients call, element-wise
TOL_LOOP = 1e-11     # three iterations, element-wise
NAMES = ("theta", "eta", "pr")

WORST = collections.defaultdict(float)        # (form, table, "step" | "loop" | "lik") -> worst error seen
BY_LENGTH = collections.defaultdict(float)    # (table, side, length) -> worst element-wise error of a row of that length
WINDOW = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    WINDOW["lw"] = LaunchWindow().__enter__()      # the launch log from the first test of this file on (read by the last one)
    WINDOW["ran"] = set()
    yield
    WINDOW.pop("lw").__exit__(None, None, None)
    print("\nworst element-wise relative error: one step / three iterations / likelihood (relative)")
    for form, name in sorted({k[:2] for k in WORST}):
        print(f"{form:34s} {name:20s} " + " / ".join(f"{WORST[form, name, kind]:.1e}" if (form, name, kind) in WORST else "-"
                                                    for kind in ("step", "loop", "lik")))
    for name, side in sorted({k[:2] for k in BY_LENGTH}):
        per = sorted((length, err) for (n, s, length), err in BY_LENGTH.items() if (n, s) == (name, side))
        print(f"{name} {side}: worst error by segment length (of {len(per)} lengths): "
              + ", ".join(f"{length}: {err:.1e}" for length, err in sorted(per, key=lambda x: -x[1])[:8]))


@pytest.fixture(autouse=True)
def _ran(request):
    yield
    WINDOW["ran"].add(request.node.originalname)


def record(form, name, kind, err):
    WORST[form, name, kind] = max(WORST[form, name, kind], err)


# ---- references: computed once per (table, internal K, internal L, seed), never changed ----
_REFS = {}


class Ref(collections.namedtuple("Ref", "table k l start want_step want_loop d_u d_i")):
    """The likelihoods are computed when first asked for."""
    _lik = {}

    def _likelihood(self, which):
        key = (self.table.name, self.k, self.l, id(self.start), which)
        if key not in Ref._lik:
            Ref._lik[key] = bt.longdouble_likelihood(self.table.data, *(self.start if which == "start" else self.want_loop))
        return Ref._lik[key]

    @property
    def lik_start(self):
        return self._likelihood("start")

    @property
    def lik_loop(self):
        return self._likelihood("loop")


def reference(name, k, l, seed=11, loops=3):
    """The long-double answers for table `name` at swap_sides = 0 (K x L groups): numerators of one step, parameters
    after `loops` steps (each step rounded to float64, as the device's are), the likelihood of both."""
    key = (name, k, l, seed, loops)
    if key not in _REFS:
        t = bt.table(name)
        start, d_u, d_i = bt.friendly_start(t, k, l, seed)
        want_step, params = bt.reference_step(t.data, *start, d_u, d_i)
        for _ in range(loops - 1):
            params = bt.reference_step(t.data, *params, d_u, d_i)[1]
        for a in start + want_step + params:
            a.setflags(write=False)
        _REFS[key] = Ref(t, k, l, start, want_step, params, d_u, d_i)
    return _REFS[key]


def form_of(ref, swap):
    """(data, dims, K, L, start, want_step, want_loop) as a context of swap_sides = `swap` takes them: the swapped table
    has the sides exchanged, so that the INTERNAL index, row lengths and sums are those of swap_sides = 0."""
    if not swap:
        return ref.table.data, ref.table.dims, ref.k, ref.l, ref.start, ref.want_step, ref.want_loop
    return (ref.table.swapped, ref.table.swapped_dims, ref.l, ref.k, bt.swapped_params(ref.start),
            bt.swapped_params(ref.want_step), bt.swapped_params(ref.want_loop))


# ---- per-row reporting ----
def row_errors(got, want):
    """Element-wise relative error per row (entries at or below ELEMENT_FLOOR: absolute, as conftest.elem_rel_err)."""
    got, want = np.asarray(got), np.asarray(want)
    big = np.abs(want) > ELEMENT_FLOOR
    rel = np.where(big, np.abs(got - want) / np.where(big, np.abs(want), 1.0), np.where(np.abs(got - want) <= ELEMENT_FLOOR, 0.0, np.inf))
    return rel.max(axis=1) if rel.size else np.zeros(len(want))


_FACTS = {}


def segment_facts(name):
    """Per internal user: (triples, pieces); per internal item: (triples of its longest pair, pieces of that pair)."""
    if name not in _FACTS:
        t = bt.table(name)
        lay = bt.layout_of(t)
        users, pairs = bt.side_facts(lay, "users"), bt.side_facts(lay, "pairs")
        n_i = t.dims[1]
        item_len, item_pieces = np.zeros(n_i, dtype=np.int64), np.ones(n_i, dtype=np.int64)
        for q, it in enumerate(lay["pair_item"]):
            if pairs["lengths"][q] > item_len[it]:
                item_len[it], item_pieces[it] = pairs["lengths"][q], pairs["pieces"][q]
        _FACTS[name] = ((users["lengths"], users["pieces"]), (item_len, item_pieces))
    return _FACTS[name]


def assert_rows(got, want, rtol, what, name=None, side=None):
    """assert_elementwise whose message names the worst row and, on a table with designed segments, that row's segment
    length and piece count."""
    if got.ndim == 3 or name is None:
        err = elem_rel_err(got, want)
        assert err <= rtol, f"{what}: element-wise relative error {err:.3e} > {rtol:.1e}"
        return err
    errs = row_errors(got, want)
    lengths, pieces = segment_facts(name)[side]
    for length in np.unique(lengths):
        key = (name, ("users", "items")[side], int(length))
        BY_LENGTH[key] = max(BY_LENGTH[key], float(errs[lengths == length].max()))
    worst = int(np.argmax(errs))
    assert errs[worst] <= rtol, (f"{what}: row {worst}, a segment of length {lengths[worst]} in {pieces[worst]} piece(s)"
                                 + (" (the item's longest pair)" if side else "")
                                 + f": element-wise relative error {errs[worst]:.3e} > {rtol:.1e}; lengths above the bar: "
                                 + str(sorted({int(x) for x in lengths[errs > rtol]})[:20]))
    return float(errs[worst]) if len(errs) else 0.0


def check(em, ref, swap, form, what, lik=True):
    """One step at 1e-12, three iterations at 1e-11 and the likelihood of both states, from the parameters the context holds."""
    _, _, _, _, _, want_step, want_loop = form_of(ref, swap)
    name = ref.table.name
    by_rows = name if name.startswith("segments") else None
    sides = (1, 0) if swap else (0, 1)        # internal side of the external theta rows / eta rows
    if lik:
        got = float(em.likelihood())
        err = abs(got - ref.lik_start) / abs(ref.lik_start)
        record(form, name, "lik", err)
        assert err <= saf.TOL_LIK, (what, "likelihood of the start", got, ref.lik_start)
    step = em.update_coefficients()
    for j, (got, want, nm) in enumerate(zip(step, want_step, NAMES)):
        assert np.all(np.isfinite(got)), (what, "n_" + nm)
        err = assert_rows(got, want, TOL_STEP, f"{form} {name} {what} n_{nm}", by_rows, sides[j] if j < 2 else None)
        record(form, name, "step", err)
    em.iterate(3)
    params = em.get_params()
    for j, (got, want, nm) in enumerate(zip(params, want_loop, NAMES)):
        assert np.all(np.isfinite(got)), (what, nm)
        err = assert_rows(got, want, TOL_LOOP, f"{form} {name} {what} {nm} after 3 iterations", by_rows, sides[j] if j < 2 else None)
        record(form, name, "loop", err)
    if lik:
        got = float(em.likelihood())
        err = abs(got - ref.lik_loop) / abs(ref.lik_loop)
        record(form, name, "lik", err)
        assert err <= saf.TOL_LIK_LOOP, (what, "likelihood after 3 iterations", got, ref.lik_loop)
    return step + params


def run(hip, ref, form, swaps, setup, kernels, slots=1, lik=True):
    """One context per side layout: `setup` selects (and asserts) the kernel form, the launch log confirms it."""
    outs = []
    for swap in swaps:
        data, dims, k, l, start = form_of(ref, swap)[:5]
        with LaunchWindow() as lw:
            with hip.HipEM(data, k, l, *dims, swap_sides=swap, slots=slots) as em:
                assert em.get_option("ranges_pairs") == 1.0 and em.get_option("ranges_users") == 1.0   # the work lists are the host layout's
                setup(em)
                em.set_params(*start)
                outs.append(check(em, ref, swap, form, f"K={k} L={l} swap={swap}", lik))
            ran(lw.names(), *kernels)
    return outs


def plain(em, ref, swap, setup, loops=3):
    """Numerators, parameters after `loops` iterations and the likelihood, unchecked (for the bitwise comparisons)."""
    data, dims, k, l, start = form_of(ref, swap)[:5]
    with em(data, k, l, *dims, swap_sides=swap) as ctx:
        setup(ctx)
        ctx.set_params(*start)
        step = ctx.update_coefficients()
        ctx.iterate(loops)
        return step + ctx.get_params() + (np.float64(ctx.likelihood()),)


def same_bits(a, b, what):
    for x, y, nm in zip(a, b, ("n_theta", "n_eta", "n_pr") + NAMES + ("likelihood",)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), (what, nm)


def refuses_two_launches(hip, em):
    try:
        em.set_option("fused", 1)
    except hip._lib.HipLibraryError:
        return True
    return False


SEG_KERNELS = {4: "seg_pass_kernel<4,4,", 8: "seg_pass_kernel<8,4,", 16: "seg_pass_kernel<16,4,", 32: "seg_pass_kernel<32,4,"}


# ---- `segments`: four launches with work lists and both combine kernels; the pair stage the shape selects ----
@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("item_len,g,k,l", bt.SEGMENT_CASES, ids=[f"len{c[0]}-g{c[1]}-{c[2]}x{c[3]}" for c in bt.SEGMENT_CASES])
def test_segments_four_launches(hip, item_len, g, k, l, swap):
    ref = reference(f"segments{item_len}-g{g}", k, l)
    pair_stage = "pair_mfma_kernel" if (k, l) == (50, 50) else "mfma_rows_kernel" if (k, l) == (80, 80) else "pair_block_kernel"

    def setup(em):
        assert em.get_option("launches") == 4.0 and refuses_two_launches(hip, em)     # a pair of more than 64 pieces
        # (the user list is built where the two-launch kernels exist for the shape; the pair list never: 65 pieces and more)
        assert int(em.get_option("fused_split")) == (2 if max(k, l) <= 24 else 0)
        assert em.get_option("items_users") > 0 and em.get_option("items_pairs") > 0
        assert em.get_option("splits_users") >= 5 and em.get_option("splits_pairs") >= 5
        assert em.get_option("mfma") == (1.0 if (k, l) == (50, 50) else 2.0 if (k, l) == (80, 80) else 0.0)
    run(hip, ref, "four launches, work lists", (swap,), setup, (SEG_KERNELS[g], "seg_combine_both_kernel", pair_stage, "eta_p_kernel"))


@pytest.mark.parametrize("item_len,g,k,l", [c for c in bt.SEGMENT_CASES if c[2] >= 50], ids=["50x50", "80x80"])
def test_segments_big_tiles_on_the_vector_alus(hip, item_len, g, k, l):
    ref = reference(f"segments{item_len}-g{g}", k, l)

    def setup(em):
        assert em.get_option("mfma") > 0
        em.set_option("mfma", 0)
        assert em.get_option("mfma") == 0.0
    run(hip, ref, "big tiles on the vector ALUs", (0,), setup, (SEG_KERNELS[g], "pair_block_kernel"))


# ---- two launches (whole-segment lists) and four, bitwise the same ----
TWO_LAUNCH = [("segments-short", 10, 10), ("segments-short", 20, 12), ("whole-fits", 20, 20), ("units-r1", 10, 10), ("units-r5", 10, 10),
              ("units-r6", 10, 10), ("units-r7", 10, 10), ("units-r12", 20, 12), ("units-r13", 10, 10), ("units-chunk", 7, 13)]


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("name,k,l", TWO_LAUNCH, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in TWO_LAUNCH])
def test_two_launches_and_four_are_bitwise_the_same(hip, name, k, l, swap):
    ref = reference(name, k, l)
    cut = not name.startswith("units")

    def two(em):
        two_launch(em)
        assert int(em.get_option("fused_split")) == (3 if cut else 0)
        assert (em.get_option("items_users") > 0) == cut       # the units tables: four launches WITHOUT work lists
    tail = "tail_fused_kernel" if cut else ("tail_fused_kernel<", ",false>")
    (a,) = run(hip, ref, "two launches", (swap,), two, ("pairs_fused_kernel", tail))
    (b,) = run(hip, ref, "four launches" + (", work lists" if cut else ""), (swap,), four_launch,
               ("seg_pass_kernel", "eta_p_kernel") + (("seg_combine",) if cut else ()))
    for x, y, nm in zip(a, b, ("n_theta", "n_eta", "n_pr") + NAMES):
        assert np.array_equal(x, y), nm


@pytest.mark.parametrize("kind,bits", [("pair65", 2), ("user_over", 1)])
def test_whole_segment_lists_give_up_past_their_limits(hip, kind, bits):
    """A pair of 65 pieces, or one partial row more than kFusedSplitLds holds: that side's list is not built, `fused_split`
    says so, the two-launch form is refused and four launches give the right answer."""
    ref = reference("whole-" + kind, 20, 20)

    def setup(em):
        assert int(em.get_option("fused_split")) == bits
        assert em.get_option("launches") == 4.0 and refuses_two_launches(hip, em)
    run(hip, ref, "four launches, work lists", (0, 1), setup, ("seg_pass_kernel<8,4,", "seg_combine", "eta_p_kernel"))


# ---- `units` on the big-tile forms: pairs per rating around the workgroup's chunk ----
BIG = [("one block", 50, 50, 1.0, ("pair_mfma_kernel",)), ("one block", 64, 17, 1.0, ("pair_mfma_kernel",)),
       ("blocked", 80, 80, 2.0, ("mfma_rows_kernel", "mfma_slab_kernel")), ("blocked", 65, 16, 2.0, ("mfma_rows_kernel", "mfma_slab_kernel"))]


@pytest.mark.parametrize("name", ["units-chunk", "units-r12"])
@pytest.mark.parametrize("form,k,l,mfma,kernels", BIG, ids=[f"{c[0].replace(' ', '-')}-{c[1]}x{c[2]}" for c in BIG])
def test_units_on_the_matrix_cores(hip, form, k, l, mfma, kernels, name):
    ref = reference(name, k, l)

    def setup(em):
        assert em.get_option("mfma") == mfma and em.get_option("chunk_pairs") == 256.0
    run(hip, ref, "matrix cores, " + form, (0, 1), setup, kernels)


@pytest.mark.parametrize("k,l,kernel", [(92, 92, "pair_block_kernel"), (32, 48, "pair_quad_a_kernel")])
def test_units_big_tiles_on_the_vector_alus(hip, k, l, kernel):
    ref = reference("units-chunk", k, l)

    def setup(em):
        assert em.get_option("mfma") > 0 and em.get_option("chunk_pairs") == 256.0
        em.set_option("mfma", 0)
    run(hip, ref, "big tiles on the vector ALUs", (0, 1), setup, (kernel,))


@pytest.mark.parametrize("chunk", [512, 1024])
def test_units_with_longer_chunks(hip, chunk, monkeypatch):
    """MMSBM_HIP_MFMA_CHUNK (test_gpu_full_size.py sets 512): ratings of 511, 512, 513 and 1,023, 1,024, 1,025 pairs."""
    ref = reference("units-chunk", 50, 50)
    monkeypatch.setenv("MMSBM_HIP_MFMA_CHUNK", str(chunk))

    def setup(em):
        assert em.get_option("chunk_pairs") == float(chunk) and em.get_option("mfma") == 1.0
    run(hip, ref, f"matrix cores, {chunk} pairs", (0, 1), setup, ("pair_mfma_kernel",))


# ---- wide rows: 1,024 pairs per workgroup (kWideChunkPairs), 64 lanes x 8, 16 or 32 doubles, seg_wide_kernel beyond 2,048 ----
WIDE = [("units-chunk", 600, 5), ("units-r12", 600, 5), ("units-r12", 1500, 3), ("units-r12", 5, 600), ("units-r12", 3, 1500),
        ("segments-short", 600, 5), ("segments-short", 1500, 3), ("segments-short", 5, 600), ("segments-short", 2100, 2)]


@pytest.mark.parametrize("name,k,l", WIDE, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in WIDE])
def test_wide_rows(hip, name, k, l):
    """(K, L) are the INTERNAL row lengths on both side layouts: K wide = the triple passes' rows, L wide = eta_p's."""
    ref = reference(name, k, l)

    def setup(em):
        assert em.get_option("wide") == 1.0 and em.get_option("chunk_pairs") == 1024.0
    row = ("seg_pass_kernel<64,16," if k == 600 else "seg_pass_kernel<64,32," if k == 1500 else "seg_wide_kernel" if k > 2048
           else ("eta_p_", "kernel<64,16>"))
    run(hip, ref, "wide rows", (0, 1), setup, (row, "eta_p_"))
    if name == "segments-short" and k == 600:      # ... and the plain wide-row kernels in place of the blocked matrix-core ones
        def valu(em):
            setup(em)
            em.set_option("mfma", 0)
        run(hip, ref, "wide rows, vector ALUs", (0,), valu, (row, "wide_"))


# ---- restart slots: 2, 3 (one lane group of a super-group of four idle) and 8; slot s is bitwise a one-slot context ----
@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("name", ["segments16-g4", "units-r6"])
@pytest.mark.parametrize("slots", [2, 3, 8])
def test_restart_slots(hip, slots, name, swap):
    refs = [reference(name, 10, 10, seed=11 + s) for s in range(slots)]
    data, dims = refs[0].table.form(swap)
    by_rows = name if name.startswith("segments") else None
    sides = (1, 0) if swap else (0, 1)
    with LaunchWindow() as lw:
        with hip.HipEM(data, 10, 10, *dims, swap_sides=swap, slots=slots) as em:
            em.set_option("fused", 0)
            for s, r in enumerate(refs):
                em.select(s).set_params(*form_of(r, swap)[4])
            em.iterate(3)
            got = [em.select(s).get_params() + (np.float64(em.select(s).likelihood()),) for s in range(slots)]
        names = lw.names()
        ran(names, f"seg_pass_slots_kernel<4,4,4,{ {2: 2, 3: 4, 8: 8}[slots]}>")       # 3 slots: a super-group of four
        if name == "units-r6" and slots == 8:      # 20,481 items x 8 slots: the 256-thread form of eta_p
            ran(names, "eta_p_w4_kernel")
    with LaunchWindow() as lw:
        for s, r in enumerate(refs):
            for j, (g, want, nm) in enumerate(zip(got[s], form_of(r, swap)[6], NAMES)):
                err = assert_rows(g, want, TOL_LOOP, f"{slots} slots {name} swap={swap} slot {s} {nm}", by_rows, sides[j] if j < 2 else None)
                record(f"restart slots ({slots})", name, "loop", err)
            err = abs(got[s][3] - r.lik_loop) / abs(r.lik_loop)
            record(f"restart slots ({slots})", name, "lik", err)
            assert err <= saf.TOL_LIK_LOOP, (s, got[s][3], r.lik_loop)
            if s in (0, slots - 1, slots // 2):
                alone = plain(hip.HipEM, r, swap, four_launch)
                same_bits(alone[3:], got[s], f"slot {s} of {slots} against a one-slot context")
        names = lw.names()
        ran(names, "eta_p_kernel")                 # the 1,024-thread form: bitwise the 256-thread one
        assert not any(n.startswith("eta_p_w4_kernel") for n in names)


# ---- bitwise contracts ----
@pytest.mark.parametrize("name,k,l,fused", [("segments16-g4", 10, 10, 0), ("segments-short", 10, 10, 1), ("units-r6", 10, 10, 1),
                                            ("units-r13", 10, 10, 0), ("segments16-g16", 50, 50, 0), ("units-chunk", 80, 80, 0)])
def test_graph_replay_equals_eager_launches(hip, name, k, l, fused):
    ref = reference(name, k, l)
    outs = []
    for graph in (0, 1):
        def setup(em):
            em.set_option("fused", fused)
            em.set_option("graph", graph)
            assert em.get_option("graph") == float(graph)
        outs.append(plain(hip.HipEM, ref, 0, setup, loops=5))      # (a graph holds two iterations: replays and one eager step)
    same_bits(*outs, "graph replay against eager launches")


@pytest.mark.parametrize("name,k,l", [("units-r6", 10, 10), ("units-r12", 20, 12), ("units-r7", 7, 13)])
def test_non_temporal_output_rows_change_nothing(hip, name, k, l):
    ref = reference(name, k, l)
    for fused in (0, 1):
        outs = []
        for nt in (7, 0, 1, 2, 4):
            def setup(em):
                assert em.get_option("nt_out") == 7.0      # no work lists, one slot, rows of at most 32: the hints are on
                em.set_option("nt_out", nt)
                assert em.get_option("nt_out") == float(nt)
                em.set_option("fused", fused)
            outs.append(plain(hip.HipEM, ref, 0, setup))
        for other in outs[1:]:
            same_bits(outs[0], other, f"nt_out, fused={fused}")


@pytest.mark.parametrize("name,k,l", [("units-chunk", 50, 50), ("segments16-g16", 50, 50), ("units-chunk", 80, 80)])
def test_a_units_change_nothing(hip, name, k, l):
    ref = reference(name, k, l)
    outs = []
    for units in (0, 1, 2, 3, 4, 16):
        def setup(em):
            assert em.get_option("mfma") > 0
            em.set_option("a_units", units)      # (longer than the longest run of units: cut to that)
            assert units == 0 or em.get_option("a_units") <= units
            assert em.get_option("a_units") > 0 or em.get_option("mfma") == 2.0      # (runs of its own: the one-block form)
        outs.append(plain(hip.HipEM, ref, 0, setup))
    for other in outs[1:]:
        same_bits(outs[0], other, "a_units")


# ---- the dense item grid: its rule, its rounds of 8, 4, 2 and 1, and the pair lists it replaces ----
GRID_TABLES = [n for n in bt.all_names() if n.startswith("grid-")]
GRID_SHAPES = [(10, 10, 8), (8, 300, 4), (8, 520, 2)]      # (K, L, T rows in flight per group: item_sum_block's B)


@pytest.mark.parametrize("name", GRID_TABLES)
def test_item_grid_rule_rounds_and_pair_lists(hip, name, monkeypatch):
    t = bt.table(name)
    n_u, n_i, n_r = t.dims
    n_pairs = len({(int(i), int(r)) for _, i, r in t.data})
    want_grid = n_r <= bt.GRID_MAX_R and 2 * n_pairs >= n_i * n_r
    if "full" in name:
        assert want_grid and n_pairs == n_i * n_r
    if "dense" in name:
        assert want_grid == (n_r <= 16)
    if "half" in name or "below" in name:
        assert want_grid == ("half" in name) and 2 * n_pairs == n_i * n_r - (0 if want_grid else 2)
    for k, l, _ in GRID_SHAPES:
        ref = reference(name, k, l)
        outs = {}
        for no_grid in (0, 1):
            if no_grid:
                monkeypatch.setenv("MMSBM_HIP_NO_ITEMGRID", "1")
            else:
                monkeypatch.delenv("MMSBM_HIP_NO_ITEMGRID", raising=False)

            def setup(em):
                assert em.n_pairs == n_pairs
                assert em.get_option("item_grid") == (0.0 if no_grid else float(want_grid)), (name, no_grid)
                em.set_option("fused", 0)
            if no_grid:
                outs[no_grid] = [plain(hip.HipEM, ref, 0, setup)]
            else:
                outs[no_grid] = run(hip, ref, f"item grid, L={l}", (0,), setup, ("eta_p_kernel",))
                outs[no_grid][0] = outs[no_grid][0] + (None,)
        monkeypatch.delenv("MMSBM_HIP_NO_ITEMGRID", raising=False)
        for x, y, nm in zip(outs[0][0][:6], outs[1][0][:6], ("n_theta", "n_eta", "n_pr") + NAMES):
            assert np.array_equal(x, y), (name, l, nm, "MMSBM_HIP_NO_ITEMGRID=1 against the default")
    # the two-launch form walks the same grid (tail_fused_kernel), and the swapped layout has a grid of its own rule
    ref = reference(name, 10, 10)
    run(hip, ref, "item grid, two launches", (0,), two_launch, ("tail_fused_kernel",))
    data, dims, k, l, start = form_of(ref, 1)[:5]
    with hip.HipEM(data, k, l, *dims, swap_sides=1) as em:
        assert em.get_option("item_grid") == float(want_grid)


# ---- the device-built index equals the host-built one on every table ----
FAMILIES = ["segments", "units", "whole", "grid", "pairmean", "sort"]


@pytest.mark.parametrize("family", FAMILIES)
def test_device_built_index_equals_the_host_built_one(hip, family, monkeypatch):
    for name in (n for n in bt.all_names() if n.startswith(family)):
        k, l = next(((c[2], c[3]) for c in bt.SEGMENT_CASES if name == f"segments{c[0]}-g{c[1]}"), (10, 10))
        if name.startswith("whole"):
            k = l = 20
        ref = reference(name, k, l)
        for swap in (0, 1):
            outs = []
            for gpu in ("0", "1"):
                monkeypatch.setenv("MMSBM_HIP_GPU_LAYOUT", gpu)
                data, dims, kk, ll, start = form_of(ref, swap)[:5]
                with hip.HipEM(data, kk, ll, *dims, swap_sides=swap) as em:
                    em.set_params(*start)
                    step = em.update_coefficients()
                    em.iterate(3)
                    outs.append((em.n_pairs,) + tuple(em.degrees()) + step + em.get_params() + (np.float64(em.likelihood()),))
            monkeypatch.delenv("MMSBM_HIP_GPU_LAYOUT")
            for x, y, nm in zip(outs[0], outs[1], ("n_pairs", "d_u", "d_i", "n_theta", "n_eta", "n_pr") + NAMES + ("likelihood",)):
                assert np.array_equal(np.asarray(x), np.asarray(y)), (name, swap, nm)
            if family == "sort":       # ... and both are right (the other families: the tests above)
                want = form_of(ref, swap)
                for got, w, nm in zip(outs[1][3:6], want[5], NAMES):
                    assert elem_rel_err(got, w) <= TOL_STEP, (name, swap, "n_" + nm)
                for got, w, nm in zip(outs[1][6:9], want[6], NAMES):
                    err = elem_rel_err(got, w)
                    record("device-built index", name, "loop", err)
                    assert err <= TOL_LOOP, (name, swap, nm)
                assert outs[1][0] == len({(int(i), int(r)) for _, i, r in ref.table.data})
                d_u = np.bincount(ref.table.data[:, 0], minlength=ref.table.dims[0])
                d_i = np.bincount(ref.table.data[:, 1], minlength=ref.table.dims[1])
                assert np.array_equal(np.maximum(outs[1][1 + swap], 1), np.maximum(d_u, 1))
                assert np.array_equal(np.maximum(outs[1][2 - swap], 1), np.maximum(d_i, 1))


# ---- the later consumers of the same index ----
LIK_CASES = [("pairmean-at", 50, 50), ("pairmean-below", 50, 50), ("segments16-g4", 10, 10), ("segments-short", 20, 20), ("segments16-g16", 50, 50), ("segments-short", 7, 70),
             ("segments-short", 12, 150), ("units-r13", 10, 10), ("units-r12", 50, 50), ("units-r12", 70, 7), ("units-r5", 5, 200)]


@pytest.mark.parametrize("name,k,l", LIK_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in LIK_CASES])
def test_every_likelihood_form(hip, name, k, l):
    ref = reference(name, k, l)
    for swap in (0, 1):
        data, dims, kk, ll, start = form_of(ref, swap)[:5]
        forms = saf.lik_forms(kk, ll, swap)
        n_pairs = len({(int(i), int(r)) for _, i, r in ref.table.data})
        if 2 * len(data) < 5 * n_pairs:      # fewer than 2.5 triples per pair: no wave per pair, the table form instead
            assert name.startswith("units") or name == "pairmean-below"
            forms = {(fast, g): (forms[1, g] if kernel.startswith("lik_wave") else kernel) for (fast, g), kernel in forms.items()}
        elif name == "pairmean-at":
            assert 2 * len(data) == 5 * n_pairs and "lik_wave_kernel<1>" in forms.values()
        with LaunchWindow() as lw:
            with hip.HipEM(data, kk, ll, *dims, swap_sides=swap) as em:
                assert em.n_pairs == n_pairs
                for params, want, rtol in ((start, ref.lik_start, saf.TOL_LIK), (form_of(ref, swap)[6], ref.lik_loop, saf.TOL_LIK)):
                    em.set_params(*params)
                    for (fast, g), kernel in forms.items():
                        em.set_option("lik_fast", fast)
                        em.set_option("lik_g", g)
                        got = float(em.likelihood())
                        err = abs(got - want) / abs(want)
                        record("likelihood " + kernel.split("<")[0], name, "lik", err)
                        assert err <= rtol, (name, swap, kernel, got, want)
            missing = sorted(set(forms.values()) - lw.names())
            assert not missing, (name, swap, missing)


@pytest.mark.parametrize("name,k,l", [("segments16-g4", 10, 10), ("units-r6", 7, 13), ("units-chunk", 50, 50), ("segments-short", 80, 3)])
def test_compute_omegas_in_request_order(hip, name, k, l):
    ref = reference(name, k, l)
    for swap in (0, 1):
        data, dims, kk, ll, start = form_of(ref, swap)[:5]
        want = orc.compute_omegas(data, *start)         # three factors per element: the oracle's products ARE the reference
        with hip.HipEM(data, kk, ll, *dims, swap_sides=swap) as em:
            em.set_params(*start)
            got = em.compute_omegas()
        err = elem_rel_err(got, want)
        record("compute_omegas", name, "step", err)
        assert err <= 4 * 2.0 ** -53, (name, swap, err)     # two roundings, in either order of the three factors


@pytest.mark.parametrize("name,k,l", [("segments16-g4", 10, 10), ("units-r13", 10, 10), ("units-chunk", 50, 50), ("segments-short", 20, 12)])
def test_predict_session_through_the_item_rating_table(hip, name, k, l):
    ref = reference(name, k, l)
    t = ref.table
    n_u, n_i, n_r = t.dims
    rng = np.random.default_rng(k + l)
    test = np.stack([rng.integers(0, n_u, 700), rng.integers(0, n_i, 700), rng.integers(0, n_r, 700)], axis=1).astype(np.int64)
    test[:3] = [[0, 0, 0], [n_u - 1, n_i - 1, n_r - 1], [n_u // 2, n_i // 2, 0]]      # ids that occur in no training row
    weights = np.arange(n_r, dtype=np.float64)
    ld = np.longdouble
    for swap in (0, 1):
        data, dims, kk, ll, start = form_of(ref, swap)[:5]
        rows = test[:, [1, 0, 2]] if swap else test
        theta, eta, pr = start
        want = np.einsum("nk,nl,klr->nr", theta.astype(ld)[rows[:, 0]], eta.astype(ld)[rows[:, 1]], pr.astype(ld)).astype(np.float64)
        with hip.HipEM(data, kk, ll, *dims, swap_sides=swap) as em:
            em.set_params(*start)
            for fast in (0, 1):
                em.set_option("predict_fast", fast)
                got = em.prod_dist(rows)
                err = elem_rel_err(got, want)
                record(f"prod_dist predict_fast={fast}", name, "step", err)
                assert err <= 1e-12, (name, swap, fast, err)
                em.predict_begin(rows, weights)
                st = em.predict_add()
                mean, raw = em.predict_finish()
                assert np.array_equal(mean, got), (name, swap, fast)
                stats, ref_stats = hip.HipEM.final_stats(st), orc.score_stats(got, rows[:, 2], list(range(n_r)))
                for key in ("accuracy", "one_off_accuracy", "mae", "s2"):
                    assert stats[key] == ref_stats[key], (name, swap, fast, key)
                assert abs(stats["s2pond"] - ref_stats["s2pond"]) <= 1e-12 * ref_stats["s2pond"]


# ---- the forms this file is about were launched by it ----
def test_every_kernel_form_was_launched_by_this_file(hip):
    """Only means something after every other test of this module has run in this process (a whole-module run); under
    -k, --lf or a split across workers there is nothing to check and the test says so."""
    others = {n for n, f in globals().items() if n.startswith("test_") and callable(f)} - {"test_every_kernel_form_was_launched_by_this_file"}
    if others - WINDOW["ran"]:
        pytest.skip("needs the whole module in one process; not run here: " + ", ".join(sorted(others - WINDOW["ran"])))
    names = WINDOW["lw"].names()
    for kernel in ("pairs_fused_kernel", "tail_fused_kernel", "seg_pass_kernel<4,4,", "seg_pass_kernel<8,4,", "seg_pass_kernel<16,4,",
                   "seg_pass_kernel<32,4,", "seg_pass_kernel<64,16,", "seg_pass_kernel<64,32,", "seg_wide_kernel", "seg_combine_both_kernel",
                   "seg_pass_slots_kernel<4,4,4,2>", "seg_pass_slots_kernel<4,4,4,4>", "seg_pass_slots_kernel<4,4,4,8>", "pair_block_kernel", "pair_quad_a_kernel",
                   "pair_mfma_kernel", "mfma_rows_kernel", "mfma_slab_kernel", "eta_p_kernel", "eta_p_w4_kernel", "lik_lane_kernel<",
                   "lik_wave_kernel<1>", "lik_wave_kernel<2>", "lik_wave_kernel<3>", "likelihood_units_kernel", "likelihood_kernel"):
        assert any(n.startswith(kernel) for n in names), (kernel, sorted(names))
    lanes = {n.split(",")[1] for n in names if n.startswith("likelihood_fast_kernel<")}
    assert {"1", "2", "4", "8"} <= lanes, sorted(names)
