"""Category-level recommendation, without a GPU: the reference of test_gpu_shelves.py (shelves_reference.py) pinned to the
literal definition and to the composition of catalogue_reference.within_top_n; the conditions that keep the GPU cases
from being vacuous; the host plan of the query (serve_plan.hpp: plan_shelves) against its rules; the parsing and the
argument checks of MMSBM.recommend_shelves / recommend_categories / recommend_new_shelves."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import exact_models as xm
import quota_reference as qr
import shelves_reference as sr
from conftest import ROOT

VARIANTS = [("mixed", "stars"), ("sorted", "indicator"), ("constant", "indicator")]
SHAPES = [(40, 997, 7, 9, 5, 3), (40, 1021, 9, 5, 4, 4)]     # xm.MANY's catalogues with fewer users: the edge users stay
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]
GPU_SHAPES = list(xm.MANY) + [(3, 5000, 4, 6, 5, 2)]         # test_gpu_shelves.py's


def same_answer(got, want, what):
    for g, w, nm in zip(got, want, sr.NAMES):
        gb, wb = (xm.bits(g), xm.bits(w)) if nm in ("values", "scores") else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        assert gb.shape == wb.shape and np.array_equal(gb, wb), (what, nm)


@functools.lru_cache(maxsize=None)
def case_of(variant, shape):
    case = xm.make_case(*variant, shape)
    case["scores"].setflags(write=False)
    return case


# ---- 1. the definition, its vectorised form and the composition of within_top_n ------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_the_reference_equals_the_definition_and_the_composition(variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    rows = np.array([0, 1, 2, 3, 7, 7, U - 1], dtype=np.int32)     # the edge users of make_case, one user twice
    scores = case["scores"][rows]
    extra = [rng.choice(I, (0, 1, 60)[b % 3], replace=False) for b in range(len(rows))]
    lay = qr.layouts(I, rng)
    requests = [(None, case["seen"], None), (np.arange(0, I, 2), case["seen"], extra), (np.arange(70, 199), None, extra)]
    asks = [(1, 1, 5, 10), (2, 3, 1, 0), (10, 10, 257, 1), (64, 1, 5, 257), (65, 3, 3, 2), (257, 1, 257, 3)]
    for name in ("mod2", "mod7", "mod64", "blocks", "all_but_three", "random"):
        category_of, G = lay[name]
        for cand, seen, ex in requests:
            fast = sr.Shelves(scores, rows, category_of, G, cand, seen, ex)
            for depth, min_items, n_shelves, per_shelf in asks:
                what = f"{name} depth={depth} min={min_items} shelves={n_shelves} per={per_shelf}"
                want = sr.literal_shelves(scores, rows, category_of, G, depth, min_items, n_shelves, per_shelf, cand, seen, ex)
                same_answer(fast.answer(depth, min_items, n_shelves, per_shelf), want, what)
                same_answer(sr.composed_shelves(scores, rows, category_of, G, depth, min_items, n_shelves, per_shelf,
                                                cand, seen, ex), want, what)
                if depth == 1 and min_items == 1 and per_shelf > 0:  # "the best item of the shelf", bit for bit
                    live = want[0] >= 0
                    assert np.array_equal(xm.bits(want[1][live]), xm.bits(want[5][:, :, 0][live])), what


def test_the_block_form_equals_the_definition():
    """block_shelves (the reference of the large-catalogue case) on a catalogue the definition can walk."""
    variant, shape = VARIANTS[0], SHAPES[0]
    case = case_of(variant, shape)
    rows = np.arange(12, dtype=np.int32)
    scores = case["scores"][rows]
    for m, seen in ((25, case["seen"]), (100, None), (100, case["seen"])):
        G = shape[1] // m
        category_of = np.where(np.arange(shape[1]) < G * m, np.arange(shape[1]) // m, -1)
        for ask in ((1, 1, 5, 10), (10, 3, 5, 10), (65, 1, 257, 1), (10, 1, 2, 0)):
            same_answer(sr.block_shelves(scores, rows, seen, m, G, *ask),
                        sr.literal_shelves(scores, rows, category_of, G, *ask, None, seen), f"m={m} {ask}")


def test_the_sum_is_sequential_not_pairwise():
    """A row where left-to-right and pairwise addition differ in the last bit: the reference gives the former."""
    s = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53] + [0.0] * 12)
    scores = s[None, :]
    got = sr.shelves(scores, [0], np.zeros(16, dtype=np.int64), 1, 4, 1, 1, 0)
    assert ((s[0] + s[1]) + (s[2] + s[3])) / 4 != 0.25                      # pairwise: 1 + 2^-52
    assert got[1][0, 0] == 0.25 == sr.sequential_mean(s[:4]) == np.cumsum(s[:4])[-1] / 4.0


# ---- 2. the GPU cases are not vacuous ---------------------------------------------------------------------------------------
def first_rows(variant, shape, n=40):
    case = case_of(variant, shape)
    rows = np.arange(min(shape[0], n), dtype=np.int32)
    return case, rows, case["scores"][rows]


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "U{}I{}".format(*s))
def test_the_depth_changes_the_shelves_on_the_mixed_family(shape):
    case, rows, scores = first_rows(("mixed", "stars"), shape)
    lay = qr.layouts(shape[1], np.random.default_rng(1))
    need = 30 if len(rows) == 40 else 2
    for name in ("mod7", "mod64", "blocks", "random"):
        fast = sr.Shelves(scores, rows, *lay[name], None, case["seen"])
        one, ten = fast.answer(1, 1, 5, 0), fast.answer(10, 1, 5, 0)
        differ = int((one[0] != ten[0]).any(axis=1).sum())
        print(shape, name, "rows whose top-5 categories differ between depth 1 and 10:", differ, "of", len(rows))
        assert differ >= need, (shape, name, differ)


@pytest.mark.parametrize("variant", VARIANTS[1:], ids=lambda v: v[0])
@pytest.mark.parametrize("shape", xm.MANY, ids=lambda s: "U{}I{}".format(*s))
def test_tied_values_leave_the_choice_to_the_index_rule(variant, shape):
    """sorted / constant: most rows have categories of exactly equal value."""
    case, rows, scores = first_rows(variant, shape)
    lay = qr.layouts(shape[1], np.random.default_rng(1))
    for name in ("mod7", "mod64", "random"):
        fast = sr.Shelves(scores, rows, *lay[name], None, case["seen"])
        for depth in (1, 10):
            v = np.where(fast.avail >= 1, fast.values(depth), -np.inf)
            tied = sum(int(len(np.unique(r[r > -np.inf])) < (r > -np.inf).sum()) for r in v)
            print(variant[0], shape, name, depth, "rows with tied category values:", tied, "of", len(rows))
            assert tied >= 30, (variant, shape, name, depth, tied)


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "U{}I{}".format(*s))
def test_min_items_removes_the_small_categories(shape):
    case, rows, scores = first_rows(("mixed", "stars"), shape)
    lay = qr.layouts(shape[1], np.random.default_rng(1))
    hit = []
    for name, (category_of, G) in lay.items():
        sizes = np.bincount(np.asarray(category_of)[np.asarray(category_of) >= 0], minlength=G)
        if not ((sizes >= 1) & (sizes <= 2)).any():
            continue
        fast = sr.Shelves(scores, rows, category_of, G)
        all_of, three = fast.answer(10, 1, G, 0), fast.answer(10, 3, G, 0)
        small = np.flatnonzero(sizes <= 2)
        assert np.isin(all_of[0], small).any() and not np.isin(three[0][three[0] >= 0], small).any(), name
        assert (three[3] < all_of[3]).all(), name
        hit.append(name)
    assert {"blocks", f"mod{shape[1]}"} <= set(hit), hit


# ---- 3. the host plan ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_exe(tmp):
    exe = os.path.join(tmp, "shelves_plan_dump")
    src = os.path.join(ROOT, "tests", "native", "shelves_plan_dump.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


def device_plan(exe, cand, lists):
    off, items = cat.csr(lists)
    words = [-1] if cand is None else [len(cand), *np.asarray(cand).tolist()]
    words += [len(lists), *off.tolist(), *items.tolist()]
    run = subprocess.run([exe], input=" ".join(str(int(x)) for x in words), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    out = {}
    for ln in run.stdout.splitlines():
        name, *vals = ln.split()
        out[name] = [int(v) for v in vals]
    return out


def expected_plan(cand, lists):
    """plan_shelves' rules, restated: columns under the candidates, categories without a column dropped, the short ones
    by width, the long ones behind them, value columns in the caller's order."""
    col_of = None if cand is None else {int(i): c for c, i in enumerate(np.asarray(cand).tolist())}
    cols = [[i if col_of is None else col_of[i] for i in lst if col_of is None or i in col_of] for lst in (np.asarray(x).tolist() for x in lists)]
    kept = [g for g, c in enumerate(cols) if len(c) > 0]
    width = lambda m: 1 << max(0, int(m - 1).bit_length())          # noqa: E731
    short = sorted((g for g in kept if len(cols[g]) <= 64), key=lambda g: (width(len(cols[g])), g))
    long_ = [g for g in kept if len(cols[g]) > 64]
    order = short + long_
    wave_first, wave_info = [], []
    at = 0
    for w in (1, 2, 4, 8, 16, 32, 64):
        mine = [g for g in short if width(len(cols[g])) == w]
        for k in range(0, len(mine), 64 // w):
            wave_first.append(at + k)
            wave_info.append(w | (min(64 // w, len(mine) - k) << 8))
        at += len(mine)
    slot = [kept.index(g) for g in order]
    return {"cat": order, "slot": slot, "of_slot": [order.index(g) for g in kept],
            "off": np.concatenate([[0], np.cumsum([len(cols[g]) for g in order])]).astype(int).tolist(),
            "col": [c for g in order for c in cols[g]], "wave_first": wave_first, "wave_info": wave_info,
            "n_short": [len(short)], "n_long": [len(long_)]}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_host_plan(tmp_path_factory):
    exe = plan_exe(str(tmp_path_factory.mktemp("shelves_plan")))
    I = 1700
    sizes = (1, 2, 63, 64, 65, 3, 4, 5, 33, 1, 1, 2, 130, 16, 17, 0, 1000, 3)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    lists = [np.arange(starts[g], starts[g + 1]) for g in range(len(sizes))]
    for cand in (None, np.arange(0, I, 2), np.arange(60, 200), np.array([0, 1, 2, 129, 699]), np.zeros(0, dtype=np.int64)):
        got, want = device_plan(exe, cand, lists), expected_plan(cand, lists)
        for name in want:
            assert got[name] == want[name], (None if cand is None else len(cand), name, got[name], want[name])
        assert sorted(got["slot"]) == list(range(len(got["cat"])))               # the value columns: a permutation ...
        assert [got["cat"][k] for k in got["of_slot"]] == sorted(got["cat"])     # ... in the caller's order
    whole = device_plan(exe, None, lists)
    assert sorted(whole["cat"]) == [g for g, m in enumerate(sizes) if m > 0]     # only the empty category is dropped
    assert whole["n_long"] == [3] and whole["cat"][-3:] == [4, 12, 16]           # 65, 130 and 1,000 columns: one wave each
    # the form at m = 1, 2, 3, 63, 64, 65, 1,000: the width of a short category, or the long form
    widths = {}
    for first, info in zip(whole["wave_first"], whole["wave_info"]):
        for k in range(first, first + (info >> 8)):
            widths[len(lists[whole["cat"][k]])] = info & 0xff
    assert [widths.get(m) for m in (1, 2, 3, 63, 64, 65, 1000)] == [1, 2, 4, 64, 64, None, None]
    two = device_plan(exe, np.array([5, 6]), lists)                              # every category but one emptied by the candidates
    assert two["cat"] == [2] and two["col"] == [0, 1] and two["wave_info"] == [2 | (1 << 8)] and two["slot"] == [0]
    none = device_plan(exe, np.zeros(0, dtype=np.int64), lists)
    assert none["cat"] == [] and none["off"] == [0] and none["wave_info"] == []
    # 2,000 singleton categories: 64 to a wave, the last wave partly filled
    got = device_plan(exe, None, [[g] for g in range(2000)])
    assert got["n_short"] == [2000] and len(got["wave_info"]) == 32 and got["wave_info"][-1] == (1 | (16 << 8))
    assert got["slot"] == list(range(2000))


# ---- 4. categories= and the arguments of the host methods -------------------------------------------------------------------
@pytest.fixture(scope="module")
def serving():
    from mmsbm_amd import serving
    return serving


def csr_lists(q):
    return [q.items[q.offsets[g]:q.offsets[g + 1]].tolist() for g in range(len(q.labels))]


def test_every_accepted_form_of_categories(serving):
    labels = np.asarray([f"item-{j}" for j in range(12)], dtype=object)
    side = serving._Side("items", 12, labels)
    table = {"item-3": "b", "item-1": "a", "item-7": "b", "item-0": "a", "item-11": "c", "not-an-item": "a",
             "item-5": None, "item-6": float("nan"), "another": "zzz"}
    want = {"b": [3, 7], "a": [0, 1], "c": [11]}
    forms = {"dict": table, "series": pd.Series(table),
             "frame": pd.DataFrame({"sku": list(table), "brand": list(table.values()), "more": 1})}
    for name, form in forms.items():
        q = serving.shelf_categories(form, side)
        assert q.offsets.dtype == np.int64 and q.items.dtype == np.int32 and q.caps is None
        assert q.labels == ["b", "a", "c"], name                            # the order of first appearance decides ties
        assert dict(zip(q.labels, csr_lists(q))) == want, name             # unknown items ignored, ids ascending
        assert q.label([3, 5, 0, 11, 2]).tolist() == ["b", None, "a", "c", None]
        # the parsing is recommend_quota's: the same labels and the same item -> category table
        cap = serving.quota_categories(form, 1, side)
        assert cap.labels == q.labels and np.array_equal(cap.category_of, q.category_of)
    with pytest.raises(ValueError, match="two different categories.*item-1"):
        serving.shelf_categories(pd.DataFrame({"i": ["item-1", "item-2", "item-1"], "c": ["a", "b", "b"]}), side)
    with pytest.raises(ValueError, match="two columns"):
        serving.shelf_categories(pd.DataFrame({"i": ["item-1"]}), side)
    with pytest.raises(ValueError, match="categories must be"):
        serving.shelf_categories([("item-1", "a")], side)
    q = serving.shelf_categories({3: "x", 4: "x", 99: "x", "5": "x"}, serving._Side("items", 12))
    assert csr_lists(q) == [[3, 4]]
    q = serving.shelf_categories({}, side)
    assert q.labels == [] and q.offsets.tolist() == [0] and len(q.items) == 0 and (q.category_of == -1).all()


def test_the_methods_check_their_arguments(serving):
    import mmsbm_amd
    model = mmsbm_amd.MMSBM(2, 2)
    for call, name in ((model.recommend_shelves, "recommend_shelves"), (model.recommend_categories, "recommend_categories"),
                       (lambda **kw: model.recommend_new_shelves(None, **kw), "recommend_new_shelves")):
        with pytest.raises(TypeError, match=name + " needs categories="):
            call()
    table = {"a": "x"}
    for bad in (True, 0, -1, 1.0, 2.5, "2", None):
        for kw in ({"shelves": bad}, {"per_shelf": bad}, {"min_items": bad}):
            with pytest.raises(ValueError, match=next(iter(kw))):
                model.recommend_shelves(categories=table, **kw)
        for kw in ({"n": bad}, {"depth": bad}, {"min_items": bad}):
            with pytest.raises(ValueError, match=next(iter(kw))):
                model.recommend_categories(categories=table, **kw)
    for bad in (True, 0, -1, 1.0, "2"):
        with pytest.raises(ValueError, match="depth"):
            model.recommend_shelves(categories=table, depth=bad)
    args = serving.Serving._shelves_args
    assert args(5, 10, None, 1) == (5, 10, 10, 1) and args(np.int64(3), 4, 2, 3) == (3, 4, 2, 3) and args(5, None, 7, 1) == (5, 0, 7, 1)
