"""explain, the item side, recommendation within a part of the catalogue, recommend_diverse and overlap_query on the
parameters a long EM run ends in (staged_params.py: late, border, rowborder, tiny, dead, sub) -- the five entry points
that were merged with their feature tests only, i.e. on rng.random simplex models and few-bit dyadic ones.  Cases,
long-double references, derived bounds and the check functions are staged_serving.py's; test_staged_serving_cpu.py pins
the inputs (which rows `1 / fmax(dot, kEps)` clamps, the planted degrees, the audience bars and the path of aud_decide
each takes) and runs the same check functions through the CPU stand-ins.

  1. explain: every contribution, explained and score ELEMENT-WISE against the long-double restatement within the
     derived relative bounds (staged_serving.py's docstring), +0.0 by the bits where a user, a target or a history item
     is zeroed, the score bit for bit recommend_query's where K <= L, and n = 1 / n = 5 bit for bit the prefix of the
     lexsort of the device's own n = 300 answer (which judges subnormal ties too).  tiny runs twice: plain weights
     (contributions about 1e-317: the floor and the order) and weights x 2^200 (about 1e-257: the relative bound on
     the fully clamped branch).  The identity explained == sum_k theta'[k] g_t[k] with the device's own fold_in.
  2. the item side: recommend_query_items and recommend_audience against the device's own user side, bit for bit, at
     bars that are device scores, their neighbours, 0.0 and 5e-324; tiny also with subnormal scores, with three slots
     (the `acc >= lo` path) and with sixteen (the divide path): staged_serving.check_bar_paths has the arithmetic.
  3. recommend_query_within / recommend_rank against the filtered rows of the device's own full rows, whole rows tied
     at +0.0 next to scores of 1e-220; recommend_diverse against diverse_reference.greedy on the device's own pool
     and distances.
  4. overlap_query element-wise against the long-double Gram matrix, rows either side of the slab length.

Each test records its worst error as a fraction of its bound; the table is printed when the module is done (-s)."""
import os
import re

import numpy as np
import pytest

import staged_serving as ss
from conftest import ELEMENT_FLOOR, ROOT
from test_gpu_instantiations import LaunchWindow, hip  # noqa: F401  (hip: the fixture)
from test_gpu_recommend import context
from test_gpu_staged_after_fit import WORST, bits, full_rows, record

pytestmark = pytest.mark.gpu

WINDOW = {}
KINDS = ("contribution", "explained", "score", "identity", "overlap users", "overlap items")
SHAPES = pytest.mark.parametrize("k,l", ss.SHAPES, ids=ss.SHAPE_IDS)


@pytest.fixture(scope="module", autouse=True)
def _report():
    WINDOW["lw"] = LaunchWindow().__enter__()      # the launch log from the first test of this file on (read by the last one)
    yield
    rows = sorted({k[0] for k in WORST if k[2] in KINDS})
    print("\nstaged serving, largest error / derived bound: " + " / ".join(KINDS))
    print(f"{'':24s}" + "".join(f"{s:>12s}" for s in ss.FAMILIES))
    for kind in KINDS:
        for row in rows:
            if any((row, s, kind) in WORST for s in ss.FAMILIES):
                cells = (f"{WORST[row, s, kind]:.3f}" if (row, s, kind) in WORST else "-" for s in ss.FAMILIES)
                print(f"{kind + ' ' + row:24s}" + "".join(f"{c:>12s}" for c in cells))


def user_side(em, c, w):
    """(U, I) scores of recommend_query with the weights w, nothing excluded."""
    ss.open_recommend(em, w, False, len(c.params))
    dev = full_rows(em, c, *c.dims[:2])
    em.recommend_end()
    return dev


# ---- 1. explain ----------------------------------------------------------------------------------------------------------
EXPLAIN_CASES = [(20, 20, 0), (20, 20, 1), (7, 33, 0), (33, 7, 0)]


@pytest.mark.parametrize("family", ss.FAMILIES)
@pytest.mark.parametrize("k,l,swap", EXPLAIN_CASES, ids=[f"K{k}L{l}swap{s}" for k, l, s in EXPLAIN_CASES])
def test_explain_on_staged_models(hip, k, l, swap, family):
    c = ss.case(k, l, family)
    em = context(hip, c.data, c.params, *c.dims, swap=swap)
    try:
        assert em.swapped == bool(swap)
        for wname, w in (("plain", ss.W),) + ((("x 2^200", ss.W_UP),) if family == "tiny" else ()):
            what = f"K={k} L={l} swap={swap} {family} weights {wname}"
            dev = user_side(em, c, w) if k <= l else None
            worst = ss.check_explain(em, c, w, ELEMENT_FLOOR, what, dev=dev)
            print(f"{what}: largest error / bound: contribution {worst['contribution']:.3f}, explained "
                  f"{worst['explained']:.3f}, score {worst['score']:.3f}; {int(worst['above'])} contributions above the floor")
            if family == "tiny" and w is ss.W:
                assert worst["above"] == 0            # subnormal contributions: the floor and the order only
            else:
                assert worst["above"] > 500           # the relative bound was applied
                for kind in ("contribution", "explained", "score"):
                    record(f"K={k} L={l}", family, kind, worst[kind])
    finally:
        em.close()


@pytest.mark.parametrize("family", ["rowborder", "tiny", "dead"])
@SHAPES
def test_explained_is_the_score_under_the_devices_own_fold_in(hip, k, l, family):
    c = ss.case(k, l, family)
    w = ss.W_UP if family == "tiny" else ss.W      # (plain tiny: explained is subnormal, nothing relative to compare)
    em = context(hip, c.data, c.params, *c.dims)
    try:
        worst = ss.check_identity(em, c, w, ELEMENT_FLOOR, f"K={k} L={l} {family}")
    finally:
        em.close()
    print(f"K={k} L={l} {family}: |explained - theta' . g| / explained_bound at most {worst:.3f}")
    record(f"K={k} L={l}", family, "identity", worst)


# ---- 2. the item side -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ss.FAMILIES)
@SHAPES
def test_item_side_on_staged_models(hip, k, l, family):
    c = ss.case(k, l, family)
    em = context(hip, c.data, c.params, *c.dims)
    try:
        for wname, w in (("plain", ss.W),) + ((("x 2^-305", ss.W_DOWN),) if family == "tiny" else ()):
            what = f"K={k} L={l} {family} weights {wname}"
            dev, bars = ss.check_item_side(em, c, w, what)
            assert (bits(dev[list(c.zero_users)]) == 0).all() and (bits(dev[:, list(c.zero_items)]) == 0).all(), what
            print(f"{what}: scores {dev[dev > 0].min():.3e} .. {dev.max():.3e}, bars {bars}")
            if family == "tiny":
                assert dev.max() < (2.0 ** -1022 if w is ss.W_DOWN else 1e-200)
    finally:
        em.close()


def test_item_side_with_subnormal_scores_on_the_divide_path(hip):
    """Sixteen slots: every subnormal bar makes gtop_floor_acc give up (check_bar_paths asserts it from the restated
    search, on the bars this run takes from the device), so aud_decide divides every accumulator and compares."""
    c = ss.case(7, 33, "tiny", n_slots=ss.WIDE_S)
    em = context(hip, c.data, c.params, *c.dims)
    try:
        dev, bars = ss.check_item_side(em, c, ss.W_DOWN, "tiny, sixteen slots, weights x 2^-305")
    finally:
        em.close()
    assert 0 < dev.max() * ss.WIDE_S < 2.0 ** -1022
    assert sum(ss.floor_acc(bar, ss.WIDE_S) == -np.inf for bar in bars) >= 7


# ---- 3. within a part of the catalogue; diverse ----------------------------------------------------------------------------------
CATALOGUE_CASES = [(k, l, ss.U, ss.I, f) for f in ("late", "rowborder", "tiny", "dead") for k, l in ss.SHAPES[:2]]
CATALOGUE_CASES.append((20, 20, ss.BIG_U, ss.BIG_I, "rowborder"))
CATALOGUE_IDS = [f"K{k}L{l}U{u}I{i}-{f}" for k, l, u, i, f in CATALOGUE_CASES]


@pytest.mark.parametrize("k,l,n_u,n_i,family", CATALOGUE_CASES, ids=CATALOGUE_IDS)
def test_catalogue_subsets_on_staged_models(hip, k, l, n_u, n_i, family):
    c = ss.case(k, l, family, n_u, n_i)
    em = context(hip, c.data, c.params, *c.dims)
    try:
        dev = ss.check_catalogue(em, c, ss.W, f"K={k} L={l} I={n_i} {family}")
    finally:
        em.close()
    assert (bits(dev[list(c.zero_users)]) == 0).all() and (bits(dev[:, list(c.zero_items)]) == 0).all()
    if family == "tiny":
        assert ELEMENT_FLOOR < dev[dev > 0].min() and dev.max() < 1e-200      # +0.0 rows next to scores of 1e-220


@pytest.mark.parametrize("k,l,n_u,n_i,family", CATALOGUE_CASES, ids=CATALOGUE_IDS)
def test_diverse_on_staged_models(hip, k, l, n_u, n_i, family):
    c = ss.case(k, l, family, n_u, n_i)
    em = context(hip, c.data, c.params, *c.dims)
    try:
        moved = ss.check_diverse(em, c, ss.W, f"K={k} L={l} I={n_i} {family}")
        print(f"diverse K={k} L={l} I={n_i} {family}: the trade-off moved {moved} of {4 * 2 * 3 * 2} lists")
    finally:
        em.close()


# ---- 4. overlap --------------------------------------------------------------------------------------------------------------------
def test_the_slab_length_is_the_headers():
    with open(os.path.join(ROOT, "mmsbm_amd", "csrc", "overlap.hpp")) as fh:
        found = re.search(r"constexpr int kOvlSlab = (\d+);", fh.read())
    assert found and int(found.group(1)) == ss.OVERLAP_SLAB == 2048
    assert ss.OVERLAP_ROWS == (2047, 2048, 2049)           # one row below the slab length, at it, one above


@pytest.mark.parametrize("rows", ss.OVERLAP_ROWS)
@pytest.mark.parametrize("family", ss.OVERLAP_FAMILIES)
def test_overlap_on_staged_models(hip, family, rows):
    c = ss.overlap_case(family, rows)
    em = context(hip, c.data, c.params, *c.dims)
    try:
        for side in ("users", "items"):
            frac = ss.check_overlap(em, c, side, ELEMENT_FLOOR, f"{family} rows={rows} {side}")
            print(f"overlap {family} rows={rows} {side}: largest error / ((rows + 2) 2^-52) = {frac:.4f}")
            record(f"rows={rows}", family, f"overlap {side}", frac)
    finally:
        em.close()


# ---- the kernels this file is about were launched by it ---------------------------------------------------------------------------
def test_the_kernels_were_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    for kernel in ("exp_row_kernel", "exp_pair_kernel", "aud_tile_kernel<false>", "aud_tile_kernel<true>", "aud_offsets_kernel",
                   "div_greedy_kernel", "ovl_gram_kernel", "ovl_combine_kernel"):
        assert kernel in names, (kernel, sorted(names))
