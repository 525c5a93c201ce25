"""Per-category caps on a top-N list, without a GPU: the reference of test_gpu_quota.py (quota_reference.py) pinned to an
independent statement of the answer; the host plan of the query (serve_plan.hpp: plan_quota) against its rules; the
parsing of MMSBM.recommend_quota's ``categories`` and ``max_per_category`` (serving.quota_categories)."""
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
from conftest import ROOT

VARIANTS = [("mixed", "stars"), ("sorted", "indicator"), ("constant", "indicator")]
SHAPES = [(40, 997, 7, 9, 5, 3), (40, 1021, 9, 5, 4, 4)]     # xm.MANY's catalogues with fewer users: the edge users stay
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]


def same_answer(got, want, what):
    for g, w, nm in zip(got, want, ("items", "scores", "counts")):
        gb, wb = (xm.bits(g), xm.bits(w)) if nm == "scores" else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        assert gb.shape == wb.shape and np.array_equal(gb, wb), (what, nm)


# ---- 1. the walk, its vectorised form and the composition of within_top_n -------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_the_walk_equals_the_composition_of_within_top_n(variant, shape):
    U, I, K, L, R, S = shape
    case = xm.make_case(*variant, shape)
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    rows = np.array([0, 1, 2, 3, 7, 7, U - 1], dtype=np.int32)     # the edge users of make_case, one user twice
    scores = case["scores"][rows]
    extra = [rng.choice(I, (0, 1, 60)[b % 3], replace=False) for b in range(len(rows))]
    lay = qr.layouts(I, rng)
    requests = [(None, None, None), (None, case["seen"], None), (np.arange(0, I, 2), case["seen"], extra),
                (np.arange(70, 199), None, extra)]
    differs = 0
    for name in ("mod2", "mod7", "mod64", "blocks", "all_but_three", "random"):
        category_of, G = lay[name]
        for cand, seen, ex in requests:
            walk = qr.Walk(scores, rows, cand, seen, ex)
            ranks = walk.ranks(category_of)
            plain = cat.within_top_n(scores, rows, 10, cand, seen, ex)
            for n in (1, 10, 257):
                for cname, caps in qr.cap_sets(n, G).items():
                    c_of = qr.mix_absent(category_of, G) if cname == "mix" else category_of
                    what = f"{name} {cname} n={n}"
                    want = qr.walk_top_n(scores, rows, n, c_of, caps, cand, seen, ex)
                    same_answer(walk.top_n(n, c_of, caps, None if cname == "mix" else ranks), want, what)
                    same_answer(qr.composed_top_n(scores, rows, n, c_of, caps, cand, seen, ex), want, what)
                    if caps.min() >= n:                         # a cap >= n has no effect
                        same_answer(want, cat.within_top_n(scores, rows, n, cand, seen, ex), what)
                    if n == 10 and cname in ("cap1", "cap2", "mix"):
                        differs += int(not np.array_equal(want[0], plain[0]))
    assert differs >= 12, differs      # the caps change answers: a mask that does nothing cannot pass test_gpu_quota.py


def test_the_gpu_cases_are_changed_by_their_caps():
    """Every case of test_gpu_quota.py at n = 10: with cap 1 most layouts change a row of the uncapped answer (never the
    singletons: there cap 1 IS the plain query)."""
    for variant in VARIANTS:
        for shape in list(xm.MANY) + [(3, 5000, 4, 6, 5, 2)]:
            U, I, K, L, R, S = shape
            case = xm.make_case(*variant, shape)
            rows = np.arange(min(U, 24), dtype=np.int32)
            walk = qr.Walk(case["scores"][rows], rows, None, case["seen"])
            plain = cat.within_top_n(case["scores"][rows], rows, 10, None, case["seen"])
            changed = []
            for name, (category_of, G) in qr.layouts(I, np.random.default_rng(1)).items():
                got = walk.top_n(10, category_of, np.full(G, 1))
                if name == f"mod{I}":
                    same_answer(got, plain, name)
                elif not np.array_equal(got[0], plain[0]):
                    changed.append(name)
            assert len(changed) >= 6 and {"mod1", "mod2", "mod7", "all_but_three"} <= set(changed), (variant, shape, changed)


# ---- 2. the host plan ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_exe(tmp):
    exe = os.path.join(tmp, "quota_plan_dump")
    src = os.path.join(ROOT, "tests", "native", "quota_plan_dump.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


def device_plan(exe, cand, lists, caps, n, forms=()):
    off, items = cat.csr(lists)
    words = [-1] if cand is None else [len(cand), *np.asarray(cand).tolist()]
    words += [len(lists), *off.tolist(), *items.tolist(), *np.asarray(caps).tolist(), n]
    for t in forms:
        words += list(t)
    run = subprocess.run([exe], input=" ".join(str(int(x)) for x in words), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    out, form = {}, []
    for ln in run.stdout.splitlines():
        name, *vals = ln.split()
        if name == "form":
            form.append((int(vals[0]), int(vals[2])))
        else:
            out[name] = [int(v) for v in vals]
    return out, form


def expected_plan(cand, lists, caps, n):
    """plan_quota's rules, restated: columns under the candidates, the dropped categories, the short ones by width."""
    col_of = None if cand is None else {int(i): c for c, i in enumerate(np.asarray(cand).tolist())}
    cols = [[i if col_of is None else col_of[i] for i in lst if col_of is None or i in col_of] for lst in (np.asarray(x).tolist() for x in lists)]
    kept = [g for g, c in enumerate(cols) if len(c) > caps[g] and caps[g] < n]
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
    return {"cat": order, "off": np.concatenate([[0], np.cumsum([len(cols[g]) for g in order])]).astype(int).tolist(),
            "col": [c for g in order for c in cols[g]], "cap": [int(caps[g]) for g in order], "wave_first": wave_first,
            "wave_info": wave_info, "n_short": [len(short)], "n_long": [len(long_)],
            "long_cap": [max([int(caps[g]) for g in long_] + [0])]}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_host_plan(tmp_path_factory):
    exe = plan_exe(str(tmp_path_factory.mktemp("quota_plan")))
    # the form by (m, q) alone, at the borders of a sub-wave group and of a wave: dropped 0, short 1, long 2
    forms = [(m, q, 10) for m in (1, 2, 3, 63, 64, 65, 1000) for q in (0, 1, 9, 10, 64)]
    I = 700
    sizes = (1, 2, 63, 64, 65, 3, 4, 5, 33, 1, 1, 2, 130, 16, 17, 0)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    lists = [np.arange(starts[g], starts[g + 1]) for g in range(len(sizes))]
    caps = np.array([0, 1, 2, 3, 9, 3, 1, 0, 40, 1, 0, 2, 5, 10, 0, 0])
    for n in (1, 10, 257):
        for cand in (None, np.arange(0, I, 2), np.arange(60, 200), np.array([0, 1, 2, 129, 699]), np.zeros(0, dtype=np.int64)):
            got, form = device_plan(exe, cand, lists, caps, n, forms)
            want = expected_plan(cand, lists, caps, n)
            for name in want:
                assert got[name] == want[name], (n, None if cand is None else len(cand), name, got[name], want[name])
            assert len(got["cat"]) < len(sizes)                                  # some category is always dropped ...
            if cand is None and n == 10:                                         # ... exactly these, for m <= q or q >= n
                assert sorted(got["cat"]) == [0, 1, 2, 3, 4, 6, 7, 10, 12, 14], got["cat"]
    want_form = [(0 if m <= q or q >= 10 else 1 if m <= 64 else 2, 1 << max(0, (m - 1).bit_length())) for m, q, _ in forms]
    assert form == want_form
    assert dict(zip([(m, q) for m, q, _ in forms], [f for f, _ in form]))[(1, 0)] == 1      # m = 1 is kept only when banned
    assert [w for (m, q, _), (_, w) in zip(forms, form) if q == 0] == [1, 2, 4, 64, 64, 128, 1024]
    # 2,000 singleton categories with cap 0: 64 to a wave, the last wave partly filled
    got, _ = device_plan(exe, None, [[g] for g in range(2000)], np.zeros(2000, dtype=int), 10)
    assert got["n_short"] == [2000] and len(got["wave_info"]) == 32 and got["wave_info"][-1] == (1 | (16 << 8))


# ---- 3. categories= and max_per_category= ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def serving():
    from mmsbm_amd import serving
    return serving


def csr_lists(q):
    return [q.items[q.offsets[g]:q.offsets[g + 1]].tolist() for g in range(len(q.caps))]


def test_every_accepted_form_of_categories(serving):
    labels = np.asarray([f"item-{j}" for j in range(12)], dtype=object)
    side = serving._Side("items", 12, labels)
    table = {"item-3": "b", "item-1": "a", "item-7": "b", "item-0": "a", "item-11": "c", "not-an-item": "a",
             "item-5": None, "item-6": float("nan"), "another": "zzz"}
    want = {"a": [0, 1], "b": [3, 7], "c": [11]}
    forms = {"dict": table, "series": pd.Series(table),
             "frame": pd.DataFrame({"sku": list(table), "brand": list(table.values()), "more": 1})}
    for name, form in forms.items():
        q = serving.quota_categories(form, 2, side)
        assert q.offsets.dtype == np.int64 and q.items.dtype == np.int32 and q.caps.dtype == np.int32
        assert dict(zip(q.labels, csr_lists(q))) == want, name              # unknown items ignored, ids ascending
        assert q.caps.tolist() == [2, 2, 2] and "zzz" not in q.labels
        assert q.category_of.tolist() == [q.labels.index(x) if x else -1 for x in
                                          ["a", "a", None, "b", None, None, None, "b", None, None, None, "c"]], name
        assert q.label([3, 5, 0, 11, 2]).tolist() == ["b", None, "a", "c", None]
    # a frame names an item twice with the same category: once; with two categories: refused
    twice = pd.DataFrame({"i": ["item-1", "item-2", "item-1"], "c": ["a", "b", "a"]})
    assert csr_lists(serving.quota_categories(twice, 1, side)) == [[1], [2]]
    with pytest.raises(ValueError, match="two different categories.*item-1"):
        serving.quota_categories(pd.DataFrame({"i": ["item-1", "item-2", "item-1"], "c": ["a", "b", "b"]}), 1, side)
    with pytest.raises(ValueError, match="two columns"):
        serving.quota_categories(pd.DataFrame({"i": ["item-1"]}), 1, side)
    with pytest.raises(ValueError, match="categories must be"):
        serving.quota_categories([("item-1", "a")], 1, side)
    # integer labels of categories and of items (the encoder's labels are their str)
    q = serving.quota_categories({3: 10, "4": 10, 5: 20}, {10: 0, 20: 1}, serving._Side("items", 12, np.asarray([str(j) for j in range(12)], dtype=object)))
    assert dict(zip(q.labels, csr_lists(q))) == {10: [3, 4], 20: [5]} and q.caps.tolist() == [0, 1]
    # after fit_encoded: ids are their own labels
    q = serving.quota_categories({3: "x", 4: "x", 99: "x", "5": "x"}, 1, serving._Side("items", 12))
    assert csr_lists(q) == [[3, 4]]
    # nothing known: no category at all
    q = serving.quota_categories({}, 1, side)
    assert len(q.caps) == 0 and q.offsets.tolist() == [0] and len(q.items) == 0 and (q.category_of == -1).all()


def test_max_per_category(serving):
    side = serving._Side("items", 6, np.asarray(list("abcdef"), dtype=object))
    table = {"a": "x", "b": "y", "c": "x", "d": "z", "e": "y"}
    q = serving.quota_categories(table, {"y": 0, "x": 3, "nobody": 1}, side)          # z is not named: uncapped
    assert dict(zip([q.labels[g] for g in np.flatnonzero(np.isin(q.labels, ["x", "y"]))], csr_lists(q))) == {"x": [0, 2], "y": [1, 4]}
    assert q.caps.tolist() == [3, 0] and q.label([3]).tolist() == ["z"]                # ... but still labelled
    assert serving.quota_categories(table, 0, side).caps.tolist() == [0, 0, 0]
    assert serving.quota_categories(table, np.int64(4), side).caps.tolist() == [4, 4, 4]
    for bad in (True, False, -1, 1.0, 2.5, "2", None, np.bool_(True)):
        with pytest.raises(ValueError, match="max_per_category"):
            serving.quota_categories(table, bad, side)
        with pytest.raises(ValueError, match="max_per_category"):
            serving.quota_categories(table, {"x": bad}, side)


def test_the_methods_require_both_arguments(serving):
    import mmsbm_amd
    model = mmsbm_amd.MMSBM(2, 2)
    for call in (model.recommend_quota, lambda **kw: model.recommend_new_quota(None, **kw)):
        for kw in ({}, {"categories": {}}, {"max_per_category": 1}):
            with pytest.raises(TypeError, match="categories= and max_per_category="):
                call(**kw)
