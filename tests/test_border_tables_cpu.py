"""The designed tables of border_tables.py are what they claim to be, and their references stand alone.

test_gpu_border_tables.py holds the device to 1e-12 element-wise on these tables because each of them sits on a border
of the kernels' index arithmetic (DESIGN section 6 lists the borders).  That only means something if the host-side
layout -- core.build_layout, the code a context runs before it uploads its index -- really reports both sides of every
border the table is named after, and if the expected values do not depend on how a CPU evaluation associates its sums.
So: per table, the lengths, piece counts, units and empty units are asserted from the layout; and on every table the
factorised checker must agree with the np.longdouble restatement of one M-step within 1e-13 element-wise, with no
expected entry at or below ELEMENT_FLOOR.  These are conditions on the inputs: a table that misses one gets other
inputs, never another bar.  (The dense float64 oracle is NOT the reference here: its sequential sums stand up to 2e-13
from the long double on the larger tables -- recorded by test_dense_oracle_distance_is_recorded, asserted nowhere.)
"""
import numpy as np
import pytest

import border_tables as bt
from conftest import ELEMENT_FLOOR, elem_rel_err
from oracle import mmsbm_factorised as fact
from oracle import mmsbm_oracle as orc

AGREE = 1e-13
NAMES = ("theta", "eta", "pr")


def present(values, wanted):
    have = set(np.asarray(values).tolist())
    return sorted(set(wanted) - have)


# ---- segments ----
@pytest.mark.parametrize("item_len,g,k,l", bt.SEGMENT_CASES)
def test_segments_hold_every_length_and_piece_count_on_both_sides(item_len, g, k, l):
    t = bt.table(f"segments{item_len}-g{g}")
    lay = bt.layout_of(t)
    ng4 = 4 * (bt.BLOCK // g)
    assert len(t.data) < 100_000
    for side in ("users", "pairs"):
        f = bt.side_facts(lay, side)
        assert f["item_len"] == item_len, (side, f["item_len"])          # ... the value item_length() really gave
        assert f["n_items"] > 0                                           # a work list exists
        assert present(f["lengths"], range(1, 131)) == [], side           # 0 .. 2 CH + 1 for CH = 8 .. 64 (0: below)
        assert present(f["lengths"], (item_len - 1, item_len, item_len + 1)) == []
        assert present(f["pieces"], (1, 2, 3, bt.SMALL_PARTS, bt.SMALL_PARTS + 1, ng4, ng4 + 1, bt.odd_round_pieces(g))) == [], side
        # the split list: the segments one group sums (at most 32 pieces) first, then those of seg_combine_big
        n_parts = lay["user_splits" if side == "users" else "pair_splits"][:, 2]
        n_small = int(np.sum(n_parts <= bt.SMALL_PARTS))
        assert (n_parts[:n_small] <= bt.SMALL_PARTS).all() and (n_parts[n_small:] > bt.SMALL_PARTS).all(), side
        # the extremes of a piece count: the longest segment of 32 (4 NG) pieces, the shortest of 33 (4 NG + 1)
        assert present(f["lengths"], (32 * item_len, 32 * item_len + 1, ng4 * item_len, ng4 * item_len + 1)) == []
        assert f["lengths"].max() <= 20_000
    # ids that never occur: first, middle, last user; first, middle, last item
    d_u = np.diff(lay["user_off"])
    n_u, n_i, _ = t.dims
    assert d_u[0] == 0 and d_u[-1] == 0 and (d_u[1:-1] == 0).any()
    per_item = np.diff(lay["item_off"])
    assert per_item[0] == 0 and per_item[-1] == 0 and per_item[n_i // 2] == 0 and lay["item_deg"][n_i // 2] == 0


def test_segments_short_holds_0_to_130_on_both_sides():
    t = bt.table("segments-short")
    lay = bt.layout_of(t)
    for side in ("users", "pairs"):
        f = bt.side_facts(lay, side)
        assert present(f["lengths"], range(1, 131)) == [] and f["item_len"] == 16 and f["pieces"].max() <= bt.SMALL_PARTS
    assert np.diff(lay["user_off"])[0] == 0 and np.diff(lay["item_off"])[0] == 0


# ---- units ----
@pytest.mark.parametrize("kind", list(bt.UNITS))
def test_units_per_rating_padding_and_slab_rounds(kind):
    t = bt.table("units-" + kind)
    n_r = t.dims[2]
    assert n_r == len(bt.UNITS[kind]) and len(t.data) < 100_000
    lay = bt.layout_of(t)
    got = bt.units_per_rating(lay, n_r)
    for r, (n_units, empty, pairs) in enumerate(got):
        assert pairs == bt.UNITS[kind][r], (r, pairs)
        full = -(-pairs // bt.UNIT)
        want = full if (n_r == 1 or pairs == 0) else -(-full // bt.XCDS) * bt.XCDS
        assert (n_units, empty) == (want, want - full), (r, n_units, empty)
    assert len(lay["user_items"]) == 0 and len(lay["pair_items"]) == 0     # no work lists: the segments as they are
    units_of = [g[0] for g in got]
    if kind in ("r6", "r13"):      # a second trip of p_update_block's `off` loop, with empty units at its end
        assert max(units_of) == 328 > bt.SLAB_ROUND and got[int(np.argmax(units_of))][1] == 7
    if kind == "r7":               # exactly one trip
        assert max(units_of) == bt.SLAB_ROUND
    if kind == "r7":
        assert units_of[0] == 0
    if kind in ("r6", "r12"):
        assert units_of[-1] == 0 and 0 in units_of[1:-1]
    if kind == "r13":              # the 328 units sit in the third pass of six ratings, alone in it
        assert units_of.index(328) == 2 * bt.RED_GROUP
    if kind == "chunk":            # pairs per rating around 256, 512 and 1,024
        for c in (256, 512, 1024):
            assert present(bt.UNITS[kind], (c - 1, c, c + 1)) == []


def test_units_cover_the_passes_of_six_ratings():
    n_rs = sorted(len(v) for k, v in bt.UNITS.items() if k != "chunk")
    assert n_rs == [1, 5, 6, 7, 12, 13]      # one pass short / full, two passes short / full, a third (register path: R <= 6)
    seen = {c for k, v in bt.UNITS.items() if k != "chunk" for c in v}
    assert present(sorted(seen), (0, 1, 63, 64, 65, 511, 512, 513, 20480, 20481)) == []


# ---- whole segments (K = L = 20: rows of 20 doubles, groups of 8 lanes, 32 work items per user workgroup) ----
@pytest.mark.parametrize("kind", ["fits", "pair65", "user_over"])
def test_whole_segment_lists_at_their_limits(kind):
    kp, g = 20, 8
    t = bt.table("whole-" + kind)
    lay = bt.layout_of(t, fused_caps=(bt.UNIT, bt.BLOCK // g))
    users, pairs = bt.side_facts(lay, "users"), bt.side_facts(lay, "pairs")
    assert users["item_len"] == 16 and pairs["item_len"] == 16
    rows_fit = bt.FUSED_SPLIT_LDS // (8 * kp)
    assert pairs["pieces"].max() == bt.UNIT + (kind == "pair65")
    assert users["pieces"].max() == rows_fit + (kind == "user_over")
    fu, fp = lay["fused_users"], lay["fused_pairs"]
    assert fp["built"] == (kind != "pair65")                      # build_mv_chunks_capped gives up past 64 pieces
    assert fu["max_parts"] * kp * 8 <= bt.FUSED_SPLIT_LDS if kind != "user_over" else fu["max_parts"] * kp * 8 > bt.FUSED_SPLIT_LDS
    per_unit = fu["units"][:, 1] - fu["units"][:, 0]
    cap = bt.BLOCK // g
    assert cap in per_unit.tolist() and cap - 2 in per_unit.tolist()     # exactly the cap; cap - 2 + 3 would pass it
    if fp["built"]:
        per_unit = fp["units"][:, 1] - fp["units"][:, 0]
        assert per_unit.max() == bt.UNIT and bt.UNIT - 2 in per_unit.tolist()
        n_pairs_of = np.array([len(set(fp["items"][a:b, 0].tolist())) for a, b in fp["units"][:, :2]])
        assert (n_pairs_of[per_unit == bt.UNIT - 2] < bt.UNIT).all()      # ... closed by the item cap, not by 64 pairs


# ---- grid ----
def grid_expected(t, lay):
    n_pairs = len(lay["pair_off"]) - 1
    return t.dims[2] <= bt.GRID_MAX_R and 2 * n_pairs >= t.dims[1] * t.dims[2]


@pytest.mark.parametrize("n_r", bt.GRID_R)
def test_dense_grid_tables_have_holes_first_last_and_an_empty_item(n_r):
    t = bt.table(f"grid-dense-r{n_r}")
    lay = bt.layout_of(t)
    assert grid_expected(t, lay) == (n_r <= bt.GRID_MAX_R)
    item_of, rating_of = lay["pair_item"], np.repeat(np.arange(n_r), np.diff(lay["rating_off"]))
    have = set(zip(item_of.tolist(), rating_of.tolist()))
    assert (1, 0) not in have and (2, n_r - 1) not in have and not any(i == 3 for i, _ in have)
    assert len(have) == t.dims[1] * n_r - 2 - n_r
    per_item = np.diff(lay["item_off"])
    assert per_item[0] == n_r and per_item[3] == 0


@pytest.mark.parametrize("n_r", bt.FULL_R)
def test_full_grid_tables_hold_every_combination(n_r):
    t = bt.table(f"grid-full-r{n_r}")
    lay = bt.layout_of(t)
    assert len(lay["pair_off"]) - 1 == t.dims[1] * n_r and grid_expected(t, lay)
    assert (np.diff(lay["item_off"]) == n_r).all()


@pytest.mark.parametrize("n_r", bt.DENSITY_R)
def test_density_rule_tables_sit_on_both_sides(n_r):
    half, below = bt.table(f"grid-half-r{n_r}"), bt.table(f"grid-below-r{n_r}")
    lh, lb = bt.layout_of(half), bt.layout_of(below)
    cells = half.dims[1] * n_r
    assert 2 * (len(lh["pair_off"]) - 1) == cells and 2 * (len(lb["pair_off"]) - 1) == cells - 2
    assert grid_expected(half, lh) and not grid_expected(below, lb)
    per_item = np.diff(lb["item_off"])
    assert present(per_item, [c for c in bt.CSR_COUNTS if c <= n_r]) == []


def test_csr_tables_hold_items_of_0_1_7_8_9_16_17_pairs():
    for name, counts in (("grid-csr-r16", bt.CSR_COUNTS[:-1]), ("grid-csr-r17", bt.CSR_COUNTS)):
        t = bt.table(name)
        lay = bt.layout_of(t)
        assert not grid_expected(t, lay)
        assert present(np.diff(lay["item_off"]), counts) == []


def test_pairmean_tables_sit_on_both_sides_of_five_triples_per_two_pairs():
    for kind, n in (("at", 1000), ("below", 999)):
        t = bt.table("pairmean-" + kind)
        lay = bt.layout_of(t)
        assert len(t.data) == n and len(lay["pair_off"]) - 1 == 400
        assert (2 * len(t.data) >= 5 * 400) == (kind == "at")


# ---- sort sizes ----
def test_sort_sizes_sit_at_one_two_and_powers_of_two():
    tabs = bt.sort_sizes()

    def kind(x):
        return "1" if x == 1 else "2" if x == 2 else "2^k" if x & (x - 1) == 0 else "2^k+1" if (x - 1) & (x - 2) == 0 else "-"
    for pick in (lambda d: d[0], lambda d: d[1], lambda d: d[1] * d[2]):
        assert {kind(pick(t.dims)) for t in tabs.values()} >= {"1", "2", "2^k", "2^k+1"}
    assert len(tabs["one-triple"].data) == 1
    same = tabs["all-the-same-triple"].data
    assert len(same) > 64 and (same == same[0]).all()
    for name in ("all-the-same-triple", "empty-last-rating"):
        t = tabs[name]
        assert t.data[:, 2].max() < t.dims[2] - 1          # the last rating has no row


# ---- the references ----
@pytest.fixture(scope="module")
def evaluations():
    """name -> the evaluations of one step at K = L = 10 (and the shape of the case for the segments tables)."""
    out = {}
    for name in bt.all_names():
        t = bt.table(name)
        shapes = [(10, 10)] + [(k, l) for il, g, k, l in bt.SEGMENT_CASES if name == f"segments{il}-g{g}" and k * l <= 400 and (k, l) != (10, 10)]
        for k, l in shapes:
            (theta, eta, pr), d_u, d_i = bt.friendly_start(t, k, l)
            out[name, k, l] = dict(
                ld=bt.longdouble_step(t.data, theta, eta, pr, d_u, d_i),
                ld_fact=bt.longdouble_factorised_step(t.data, theta, eta, pr, d_u, d_i),
                fact=(fact.update_coefficients(t.data, theta, eta, pr), fact.em_step(t.data, theta, eta, pr, d_u, d_i)),
                dense=(orc.update_coefficients(t.data, theta, eta, pr), orc.em_step(t.data, theta, eta, pr, d_u, d_i)))
    return out


def test_the_factorised_checker_agrees_with_the_long_double_on_every_table(evaluations):
    for (name, k, l), ev in evaluations.items():
        for kind in (0, 1):       # numerators, parameters
            for x, y, nm in zip(ev["fact"][kind], ev["ld"][kind], NAMES):
                err = elem_rel_err(x, y)
                assert err <= AGREE, (name, k, l, ("numerators", "parameters")[kind], nm, err)


# a sequential long-double sum of n terms is within n 2^-64 of the exact one; the longest sum of any table here has 20,481
# terms (the pairs of one rating); then one rounding to float64 each
LD_AGREE = 20_481 * 2.0 ** -64 + 2.0 ** -52


def test_the_two_long_double_restatements_agree(evaluations):
    """The dense and the factorised long-double step (border_tables.reference_step uses the second where the first one's
    (N, K, L) tensor is out of reach) differ by their summation error in long double and a float64 rounding."""
    for (name, k, l), ev in evaluations.items():
        for kind in (0, 1):
            for x, y, nm in zip(ev["ld_fact"][kind], ev["ld"][kind], NAMES):
                err = elem_rel_err(x, y)
                assert err <= LD_AGREE, (name, k, l, nm, err)


def test_no_expected_entry_is_at_or_below_the_floor(evaluations):
    for (name, k, l), ev in evaluations.items():
        for kind in (0, 1):
            for a, nm in zip(ev["ld"][kind], NAMES):
                assert not np.any((a != 0) & (np.abs(a) <= ELEMENT_FLOOR)), (name, nm)


def test_dense_oracle_distance_is_recorded(evaluations):
    """Printed (-s), not asserted: the dense oracle adds a rating's increments one after the other, which no bar of
    1e-13 survives on 20,000 pairs of one rating (DESIGN section 6 has the figures)."""
    worst = {}
    for (name, k, l), ev in evaluations.items():
        for kind in (0, 1):
            for x, y, nm in zip(ev["dense"][kind], ev["ld"][kind], NAMES):
                err = elem_rel_err(x, y)
                if err > worst.get(nm, (0.0,))[0]:
                    worst[nm] = (err, name, k, l)
    for nm, rec in worst.items():
        print(f"dense float64 oracle vs long double, worst {nm}: {rec[0]:.2e} on {rec[1]} K={rec[2]} L={rec[3]}")
    assert all(np.isfinite(rec[0]) for rec in worst.values())
