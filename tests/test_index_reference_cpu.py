"""index_reference.sort_stage against the host builder (layout.hpp through core.build_layout) on every table of
index_cases.py: all nine arrays of the sort stage, whole, by equality.  This pins the numpy restatement that
test_gpu_index.py holds the device-built index to, and is the host builder's own test at key spaces beyond 2^26 (its
comparison-sort branch) and at 2^31 and more (where a context never sorts on the device).  No GPU."""
import numpy as np
import pytest

import index_cases as ic
import index_reference as ir
from mmsbm_amd.core import build_layout


@pytest.mark.parametrize("name", ic.NAMES)
def test_host_builder_equals_the_numpy_restatement(name):
    _, data, n_u, n_i, n_r = ic.case(name)
    for swap in (0, 1):                                     # the columns a swapped context sorts
        cols, dims = ic.internal(data, (n_u, n_i, n_r), swap)
        want = ir.sort_stage(cols, *dims)
        got = build_layout(cols, *dims)
        wrong = ir.differing(got, want)
        assert not wrong, (name, swap, wrong)


def test_the_cases_hold_what_they_are_named_after():
    for name in ic.NAMES:
        _, data, n_u, n_i, n_r = ic.case(name)
        top, bottom = np.all(data == [n_u - 1, n_i - 1, n_r - 1], axis=1).sum(), np.all(data == 0, axis=1).sum()
        if name == "absent-ends":
            assert top == 0 and bottom == 0
            assert data[:, 0].min() == 10 and data[:, 0].max() == 89 and data[:, 1].min() == 10 and data[:, 1].max() == 69
            assert sorted(np.unique(data[:, 2])) == [1, 3]
        elif name == "all-pairs-distinct":
            assert top == 1 and bottom == 1 and len(np.unique(data[:, 2] * n_i + data[:, 1])) == len(data)
        elif len(data) >= 4:
            assert top >= 3 and bottom >= 1, name
        else:
            assert top == len(data), name
    assert [len(ic.case(n)[1]) for n in ("n1", "n255", "n256", "n257", "n300k")] == [1, 255, 256, 257, 300_000]
    assert [ic.key_space(n) for n in ic.KEY_SPACES] == [2 ** 26, 2 ** 26 + 2 ** 21, 2 ** 27, 2 ** 31 - 2 ** 20, 2 ** 31, 4_000 * 2 ** 20]
    assert [ic.key_space(f"ri{k}") for k in (1, 2, 256, 257, 65_536, 65_537)] == [1, 2, 256, 257, 65_536, 65_537]
    for name in ("one-pair-u1", "one-pair-u50"):
        assert len(np.unique(ic.case(name)[1][:, 1:], axis=0)) == 1
    _, dup, *dims = ic.case("dup")
    assert tuple(dims) == (60, 40, 3) and len(dup) == 50_000 and len(np.unique(dup, axis=0)) <= 60 * 40 * 3
    a, b = ic.case("switch-99999")[1], ic.case("switch-100000")[1]
    assert len(a) == 99_999 and len(b) == 100_000 and np.array_equal(a, b[:-1])


def test_reference_on_a_table_worked_by_hand():
    # rows (user, item, rating); pairs in (rating, item) order: (i0, r0) (i2, r0) (i0, r2) (i2, r2)
    data = np.array([[0, 0, 0], [0, 0, 0], [2, 2, 2], [4, 0, 2], [0, 0, 2], [4, 2, 0]])
    ref = ir.sort_stage(data, 5, 3, 3)
    assert ref["pair_off"].tolist() == [0, 2, 3, 5, 6] and ref["pair_item"].tolist() == [0, 2, 0, 2]
    assert ref["pair_user"].tolist() == [0, 0, 4, 0, 4, 2] and ref["rating_off"].tolist() == [0, 2, 2, 4]
    assert ref["user_off"].tolist() == [0, 3, 3, 4, 4, 6] and ref["user_pair"].tolist() == [0, 0, 2, 3, 1, 2]
    assert ref["item_off"].tolist() == [0, 2, 2, 4] and ref["item_pairs"].tolist() == [0, 2, 1, 3]
    assert ref["item_deg"].tolist() == [4, 0, 2]
    empty = ir.sort_stage(np.zeros((0, 3), dtype=np.int64), 3, 2, 2)
    assert empty["pair_off"].tolist() == [0] and empty["rating_off"].tolist() == [0, 0, 0] and empty["user_off"].tolist() == [0] * 4
    assert not ir.differing(build_layout(np.zeros((0, 3), dtype=np.int64), 3, 2, 2), empty)


@pytest.mark.parametrize("name", ic.RANGE_TABLES)
def test_range_tables_hold_what_the_range_cut_tests_need(name):
    data, dims = ic.range_table(name)
    lay = build_layout(data, *dims)
    assert not ir.differing(lay, ir.sort_stage(data, *dims))
    deg = np.bincount(data[:, 0], minlength=dims[0])
    if name == "lognormal":
        assert deg[0] == 0 and deg[350] == 0 and deg[-1] == 0 and deg[1] == 1      # the planted empty users, one single triple
        assert len(lay["pair_splits"]) > 0 and len(lay["user_splits"]) > 0          # the host builder alone cuts both sides
    if name == "five-users":
        assert dims[0] == 5 and deg.min() > 64
    if name == "one-pair":
        assert len(lay["pair_item"]) == 1 and dims[1:] == (1, 1)


def test_check_work_lists_on_lists_made_by_hand():
    """4 segments over a table of 8 rows in 2 ranges (rows 0-3, 4-7), item length 4: a segment of one range left whole,
    a short one of two ranges left whole, an empty one, and a long one cut at the border and again at the item length."""
    off = np.array([0, 5, 7, 7, 17])
    idx = np.array([0, 1, 1, 2, 3,   3, 4,   0, 0, 1, 2, 3, 3, 4, 5, 6, 7])
    items = np.array([[3, 7, 11, 0], [3, 11, 13, 1], [3, 13, 17, 2], [2, 7, 7, -1], [1, 5, 7, -1]])
    # segment 0: 5 triples of range 0, longer than an item: cut in two
    items = np.vstack([items, [[0, 0, 4, 3], [0, 4, 5, 4]]])
    splits = np.array([[0, 3, 2, 0], [3, 0, 3, 0]])
    with pytest.raises(AssertionError):                     # partial rows are dealt in segment order
        ir.check_work_lists(off, idx, 8, 2, items, splits, item_len=4)
    items[:, 3] = [2, 3, 4, -1, -1, 0, 1]
    splits = np.array([[0, 0, 2, 0], [3, 2, 3, 0]])
    assert ir.check_work_lists(off, idx, 8, 2, items, splits, item_len=4) == 2
    bad = items.copy()
    bad[1, 2], bad[2, 1] = 14, 14                            # the second piece of segment 3 now ends in range 1
    with pytest.raises(AssertionError, match="more than one range"):
        ir.check_work_lists(off, idx, 8, 2, bad, splits, item_len=4)
    bad = items.copy()
    bad[0, 2], bad[1, 1] = 12, 12                            # its first piece: five triples of range 0
    with pytest.raises(AssertionError, match="longer than"):
        ir.check_work_lists(off, idx, 8, 2, bad, splits, item_len=4)
    with pytest.raises(AssertionError):                     # an item is missing
        ir.check_work_lists(off, idx, 8, 2, items[1:], splits, item_len=4)
    # segment 1 (2 triples < 2 x 2 ranges) must stay whole, however consistent the records of its pieces are
    cut = np.array([[3, 7, 11, 4], [3, 11, 13, 5], [3, 13, 17, 6], [2, 7, 7, -1], [1, 5, 6, 2], [1, 6, 7, 3], [0, 0, 4, 0], [0, 4, 5, 1]])
    with pytest.raises(AssertionError, match="not the rule's"):
        ir.check_work_lists(off, idx, 8, 2, cut, np.array([[0, 0, 2, 0], [1, 2, 2, 0], [3, 4, 3, 0]]), item_len=4)
    # placement: workgroups of 2 items, 2 ranges shared by 4 XCDs each (range r on XCDs r, r + 2, r + 4, r + 6)
    null = [-1, 0, 0, -1]
    blocks = {0: [items[5], items[6]], 2: [items[0], items[1]], 1: [items[2], items[4]], 4: [items[3], null]}
    placed = np.array([x for b in range(8) for x in blocks.get(b, [null, null])])
    assert ir.check_work_lists(off, idx, 8, 2, placed, splits, item_len=4, per_block=2) == 2
    blocks[3] = blocks.pop(2)                                # range 0 on XCD 3
    placed = np.array([x for b in range(8) for x in blocks.get(b, [null, null])])
    with pytest.raises(AssertionError, match="wrong XCD"):
        ir.check_work_lists(off, idx, 8, 2, placed, splits, item_len=4, per_block=2)
