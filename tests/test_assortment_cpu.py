"""Greedy assortment selection, without a GPU: the numpy reference of test_gpu_assortment.py (assortment_reference.py)
against brute force and against its own identities; its gain sums on exact models in three summation orders; the host
plan of the query (serve_plan.hpp: plan_assortment) through the native checker; MMSBM.assortment / assortment_value over
a stand-in device; header, ctypes signature and wrapper."""
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

import assortment_reference as ar
import exact_models as xm
import fake_device
from conftest import ROOT
from mmsbm_amd.core import HipEM
from test_recommend_cpu import RecommendFakeHipEM, fitted, restate_scores, seen_items, string_frame

MIXED = [("mixed", "stars"), ("mixed", "signed")]
BLOCKS = [("sorted", "indicator"), ("constant", "indicator"), ("interleaved", "stars"), ("rare", "stars")]
OBJECTIVES = ("best_score", "reach")


def numerators(case):
    """The undivided accumulators of every (user, item) pair of an exact_models case: score = A / S, A exact."""
    U, I = case["shape"][:2]
    w = np.asarray(case["w"], dtype=np.float64)
    num = np.zeros((U, I))
    for theta, eta, p in case["params"]:
        num += (theta @ (p @ w)) @ eta.T
    return num + 0.0


@functools.lru_cache(maxsize=None)
def case_of(variant, shape):
    case = xm.make_case(*variant, shape)
    case["A"] = numerators(case)
    case["A"].setflags(write=False)
    return case


def level_of(case, objective):
    """The default floor, or a bar on an occurring score (the upper quartile)."""
    if objective == "best_score":
        return float(np.min(case["w"]))
    return float(np.sort(case["scores"], axis=None)[3 * case["scores"].size // 4])


# ---- 1. the reference against brute force -----------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_the_greedy_against_the_best_set(objective):
    rng = np.random.default_rng(11)
    for trial in range(40):
        U, I = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        A = rng.integers(-3, 9, (U, I)).astype(np.float64) / 2.0
        seen = [set(rng.choice(I, int(rng.integers(0, I)), replace=False).tolist()) for _ in range(U)]
        level = float(rng.integers(-4, 6)) / 2.0
        for c in (1, 2, 3):
            got = ar.greedy(A, c, objective, level, seen=seen)
            total = float(got["gains"].sum())
            best, _ = ar.best_set(A, c, objective, level, seen=seen)
            assert total <= best + 1e-12 and total >= (1.0 - 1.0 / math.e) * best - 1e-12, (trial, c, total, best)
            if c == 1:
                assert total == best
            assert (np.diff(got["gains"]) <= 0).all(), (trial, got["gains"])       # submodular: gains never increase
            assert total == ar.set_value(A, got["items"], objective, level, seen=seen)   # (halves: every sum is exact)
            assert got["stop"] == ("c" if len(got["items"]) == c else "no_gain" if len(got["items"]) < I else "no_candidates")


# ---- 2. identities ---------------------------------------------------------------------------------------------------------------
def test_copies_are_never_taken_twice_while_another_item_gains():
    rng = np.random.default_rng(5)
    base = rng.integers(0, 9, (30, 6)).astype(np.float64)
    A = np.concatenate([base[:, [0]]] * 5 + [base], axis=1)                   # items 0 .. 5: copies of one column
    copies = set(range(6))
    for objective, level in (("best_score", 0.0), ("reach", 6.0)):
        got = ar.greedy(A, 6, objective, level)
        picked = got["items"].tolist()
        assert len(copies & set(picked)) <= 1, picked                         # a second copy gains exactly 0
        first = ar.State(A, np.ones_like(A, dtype=bool), objective, level).gains(np.arange(11))
        assert picked[0] == int(np.flatnonzero(first == first.max())[0])      # equal gains: the smallest item id
        if picked[0] in copies:
            assert picked[0] == 0                                             # ... so of the copies only the first


@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("variant", [MIXED[0], BLOCKS[0]], ids=["mixed", "sorted"])
def test_value_and_given_identities(variant, objective):
    case = case_of(variant, xm.MANY[0])
    A, S, seen = case["A"], case["shape"][5], case["seen"]
    level = level_of(case, objective)
    whole = ar.greedy(A, 12, objective, level, S, seen=seen)
    n = len(whole["items"])
    assert n >= 2
    # assortment_value(chosen) is the greedy's value: c = 0 with the chosen items given
    valued = ar.greedy(A, 0, objective, level, S, seen=seen, given=whole["items"])
    assert valued["stop"] == "c" and len(valued["items"]) == 0
    assert xm.bits(valued["value"]) == xm.bits(whole["value"])
    assert np.array_equal(xm.bits(valued["given_gains"]), xm.bits(whole["gains"]))
    for a, b in zip(valued["served"], whole["served"]):
        assert np.array_equal(xm.bits(a) if a.dtype == np.float64 else a, xm.bits(b) if b.dtype == np.float64 else b)
    # given = the first k chosen, then c - k rounds: the tail
    for k in (1, n // 2):
        tail = ar.greedy(A, 12 - k, objective, level, S, seen=seen, given=whole["items"][:k])
        assert tail["items"].tolist() == whole["items"][k:].tolist() and tail["stop"] == whole["stop"]
        assert np.array_equal(xm.bits(tail["gains"]), xm.bits(whole["gains"][k:]))
        assert tail["start"] == float(np.cumsum(whole["gains"][:k])[-1])


# ---- 3. exact models: the gains do not depend on the order of the sum -----------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.MANY, ids=["U300", "U260"])
@pytest.mark.parametrize("variant", MIXED + BLOCKS, ids=["-".join(v) for v in MIXED + BLOCKS])
def test_gains_on_exact_models_are_the_same_bits_in_three_orders(variant, shape):
    case = case_of(variant, shape)
    A, S = case["A"], case["shape"][5]
    U, I = A.shape
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    orders = (None, np.arange(U)[::-1], rng.permutation(U))
    rounds, ties = {}, 0
    for objective in OBJECTIVES:
        level = level_of(case, objective)
        st = ar.State(A, ar.eligible_mask(U, I, np.arange(U), case["seen"]), objective, level, S)
        left = np.arange(I)
        for k in range(12):
            g = [st.gains(left, order) for order in orders]
            assert np.array_equal(xm.bits(g[0]), xm.bits(g[1])) and np.array_equal(xm.bits(g[0]), xm.bits(g[2])), (objective, k)
            at = int(np.lexsort((left, -g[0]))[0])
            if not g[0][at] > 0:
                break
            ties = max(ties, int((g[0] == g[0][at]).sum()))
            st.take(int(left[at]))
            left = np.delete(left, at)
            rounds[objective] = k + 1
    if variant[0] == "mixed":
        assert rounds["best_score"] == 12                                     # the rounds: mostly unique maxima
    else:
        assert min(rounds.values()) < 12 and ties > 1, (rounds, ties)          # the early stop and the tie rule


# ---- 4. the host plan ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_exe(tmp):
    exe = os.path.join(tmp, "assort_plan_check")
    src = os.path.join(ROOT, "tests", "native", "assort_plan_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


def device_plan(exe, n_rows, C, n_cus=256, run_blocks=0, part_bytes=64 << 20):
    run = subprocess.run([exe, *(str(int(v)) for v in (n_rows, C, n_cus, run_blocks, part_bytes))], capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in run.stdout.splitlines()}
    return {k: (v if k == "batch_blk" else v[0]) for k, v in got.items()}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_host_plan(tmp_path_factory):
    exe = plan_exe(str(tmp_path_factory.mktemp("assort_plan")))
    sweep = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert sweep.returncode == 0 and "assort plan check: ok" in sweep.stdout, (sweep.stdout + sweep.stderr)[-3000:]
    # one user, and either side of a step: the padding is the last run's, a run is whole steps
    for n, blocks in ((1, 1), (127, 16), (128, 16), (129, 17)):
        p = device_plan(exe, n, 997)
        assert p["n_blocks"] == blocks and p["run_rows"] % 128 == 0 and p["runs"] * p["run_rows"] >= n > (p["runs"] - 1) * p["run_rows"]
        assert p["item_tiles"] == 8 and p["batches"] == 1 and p["batch_blk"] == [0, 4] and p["part_doubles"] == p["runs"] * 1024
    assert device_plan(exe, 129, 997)["runs"] == 2                            # (256 tiles' worth of workgroups wanted: the shortest runs)
    # run borders: the library's choice at the largest shape, a forced run length rounded up to whole steps
    big = device_plan(exe, 99997, 100000)
    assert (big["run_blocks"], big["runs"], big["batches"]) == (6256, 2, 1)
    assert device_plan(exe, 300, 997, run_blocks=17)["run_blocks"] == 32
    assert device_plan(exe, 300, 997, run_blocks=16)["runs"] == 3
    assert device_plan(exe, 300, 997, run_blocks=1 << 20)["runs"] == 1
    small = device_plan(exe, 300, 997, run_blocks=16, part_bytes=3 * 256 * 8)
    assert (small["batch_tiles"], small["batches"], small["ld"], small["batch_blk"]) == (2, 4, 256, [0, 1, 2, 3, 4])


# ---- 5. the host method over a stand-in device -----------------------------------------------------------------------------------------
class AssortFakeHipEM(RecommendFakeHipEM):
    """RecommendFakeHipEM with recommend_assortment, answered by the numpy greedy over the restated scores."""
    ASSORT_MODES = HipEM.ASSORT_MODES

    def recommend_assortment(self, users, c, mode, level, given=None, candidates=None):
        assert self._rc["params"], "recommend_assortment before recommend_add"
        u = np.asarray(users)
        given = np.zeros(0, dtype=np.int32) if given is None else np.asarray(given)
        assert u.dtype == np.int32 and given.dtype == np.int32 and 0 <= c <= 1024 and mode in self.ASSORT_MODES
        assert len(set(u.tolist())) == len(u) and len(set(given.tolist())) == len(given)
        if candidates is not None:
            cand = np.asarray(candidates)
            assert cand.dtype == np.int32 and (np.diff(cand) > 0).all()
        fake_device.LOG.append(("recommend_assortment", len(u), c, mode))
        scores = restate_scores(self._rc["params"], np.arange(self.n_users), self.n_items, self._rc["w"])
        rows = np.sort(u)
        got = ar.greedy(scores, c, mode, level, 1, rows, self._rc["seen"], given.tolist(), candidates)
        s_items, s_scores = np.full(len(u), -1, dtype=np.int32), np.full(len(u), -np.inf)
        place = np.searchsorted(rows, u)
        at, it, sc = got["served"]
        back = np.empty(len(u), dtype=np.int64)
        back[place] = np.arange(len(u))
        s_items[back[at]], s_scores[back[at]] = it, sc
        return (got["items"].astype(np.int32), got["gains"], len(got["items"]), got["stop"], s_items, s_scores, got["start"])


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", AssortFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(AssortFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def expected(m, c, objective, level, users=None, given=(), candidates=None, exclude_seen=True):
    enc = m.data_handler
    ul, il = list(enc.user_labels()), list(enc.item_labels())
    params = [(r["theta"], r["eta"], r["pr"]) for r in m.results]
    scores = restate_scores(params, np.arange(m.p + 1), m.m + 1, np.asarray(m.ratings, dtype=np.float64))
    rows = np.arange(m.p + 1) if users is None else np.asarray(sorted({ul.index(u) for u in users}))
    seen = seen_items(m.train, m.p + 1) if exclude_seen else None
    cand = None if candidates is None else np.asarray(sorted({il.index(i) for i in candidates}))
    return ar.greedy(scores, c, objective, level, 1, rows, seen, [il.index(i) for i in given], cand), ul, il, rows


def test_the_host_method(host):
    m = fitted(host, string_frame(), sampling=2)
    items, users = list(m.data_handler.item_labels()), list(m.data_handler.user_labels())
    floor = float(min(m.ratings))
    fake_device.LOG.clear()
    got = m.assortment(c=4)
    kinds = [e[0] for e in fake_device.LOG]
    assert kinds.count("recommend_add") == 2 and kinds.count("recommend_assortment") == 1 and kinds[-1] == "recommend_end"
    want, ul, il, rows = expected(m, 4, "best_score", floor)
    assert list(got.columns) == ["items", "gain", "total", "rank"]
    assert got["gain"].dtype == np.float64 and got["total"].dtype == np.float64 and got["rank"].dtype == np.int64
    assert got["items"].tolist() == [il[i] for i in want["items"]] and got["rank"].tolist() == [1, 2, 3, 4]
    assert np.array_equal(xm.bits(got["gain"]), xm.bits(want["gains"]))
    assert np.array_equal(xm.bits(got["total"]), xm.bits(np.cumsum(want["gains"])))
    a = m.assortment_
    assert set(a) == {"rounds", "stopped", "users", "floor", "start", "value", "served"}
    assert (a["rounds"], a["stopped"], a["users"], a["floor"], a["start"]) == (4, "c", len(users), floor, 0.0)
    assert xm.bits(a["value"]) == xm.bits(want["value"]) and a["value"] > floor
    at, it, sc = want["served"]
    assert list(a["served"].columns) == ["users", "items", "score"]
    assert a["served"]["users"].tolist() == [ul[rows[b]] for b in at] and a["served"]["items"].tolist() == [il[i] for i in it]
    assert np.array_equal(xm.bits(a["served"]["score"]), xm.bits(sc))
    # every accepted form of users / given / candidates; a user and a given item named twice count once
    ask = ["u7", "u1", "u3", "u7", "u0"]
    held = [items[3], items[0], items[3]]
    stock = items[::2]
    for us, gv, cd in ((ask, held, stock), (tuple(ask), np.asarray(held, dtype=object), pd.Series(stock)),
                       (pd.Series(ask), pd.Series(held), set(stock)), (iter(ask), iter(held), iter(stock))):
        got = m.assortment(c=3, users=us, given=gv, candidates=cd, floor=0.5)
        want, ul, il, rows = expected(m, 3, "best_score", 0.5, ask, [items[3], items[0]], stock)
        assert got["items"].tolist() == [il[i] for i in want["items"]] and set(got["items"]) <= set(stock) - set(held)
        assert np.array_equal(xm.bits(got["gain"]), xm.bits(want["gains"]))
        assert m.assortment_["users"] == 4 and m.assortment_["floor"] == 0.5 and m.assortment_["start"] == want["start"] > 0
        assert m.assortment_["served"]["users"].tolist() == [u for u in ["u7", "u1", "u3", "u0"] if ul.index(u) in rows[want["served"][0]]]
    # reach: whole numbers of users, the share reached, the stop reasons
    bar = float(np.median(restate_scores([(r["theta"], r["eta"], r["pr"]) for r in m.results], np.arange(m.p + 1), m.m + 1,
                                         np.asarray(m.ratings, dtype=np.float64))))
    got = m.assortment(c=len(items), objective="reach", bar=bar, exclude_seen=False)
    want, ul, il, rows = expected(m, len(items), "reach", bar, exclude_seen=False)
    assert got["items"].tolist() == [il[i] for i in want["items"]] and (got["gain"] == np.floor(got["gain"])).all()
    assert m.assortment_["stopped"] == want["stop"] == "no_gain" and "bar" in m.assortment_ and "floor" not in m.assortment_
    assert m.assortment_["value"] == got["total"].iloc[-1] / len(users) == len(m.assortment_["served"]) / len(users)
    none = m.assortment(c=3, objective="reach", bar=1e9)
    assert len(none) == 0 and list(none.columns) == ["items", "gain", "total", "rank"] and none["rank"].dtype == np.int64
    assert m.assortment_["stopped"] == "no_gain" and m.assortment_["value"] == 0.0 and len(m.assortment_["served"]) == 0
    assert m.assortment(c=3, candidates=[]).empty and m.assortment_["stopped"] == "no_candidates"
    assert m.assortment(c=3, candidates=items[:2], given=items[:2]).empty and m.assortment_["stopped"] == "no_candidates"
    assert m.assortment(c=0).empty and m.assortment_["stopped"] == "c" and m.assortment_["rounds"] == 0
    assert m.assortment(c=2, users=[]).empty and m.assortment_["users"] == 0 and m.assortment_["value"] == floor
    # assortment_value: the same arithmetic for a set somebody else picked
    greedy = m.assortment(c=3)
    value = m.assortment_["value"]
    worth = m.assortment_value(greedy["items"].tolist())
    assert set(worth) == {"value", "start", "served"} and xm.bits(worth["value"]) == xm.bits(value)
    assert m.assortment_["rounds"] == 0 and m.assortment_value(items[:3])["value"] <= value
    assert m.assortment_value(items[:3], objective="reach", bar=bar)["value"] <= 1.0
    # the refusals, by name
    for kw, name in (({"c": -1}, "c"), ({"c": 1025}, "c"), ({"c": 2.0}, "c"), ({"c": True}, "c"),
                     ({"objective": "coverage"}, "objective"), ({"objective": "reach"}, "bar"),
                     ({"objective": "reach", "bar": np.inf}, "bar"), ({"objective": "reach", "bar": 3.0, "floor": 1.0}, "floor"),
                     ({"bar": 3.0}, "bar"), ({"floor": np.nan}, "floor"), ({"floor": -np.inf}, "floor"), ({"floor": "1"}, "floor"),
                     ({"weights": [1.0, 2.0]}, "weights")):
        with pytest.raises(ValueError, match=name):
            m.assortment(**kw)
    for kw in ({"users": ["nobody"]}, {"given": ["not-an-item"]}, {"candidates": ["not-an-item"]}):
        with pytest.raises(KeyError):
            m.assortment(**kw)
    with pytest.raises(TypeError):
        m.assortment_value()
    with pytest.raises(KeyError):
        m.assortment_value(["not-an-item"])


# ---- 6. header, signature and wrapper agree ---------------------------------------------------------------------------------------------
def test_header_signature_and_wrapper_agree():
    from mmsbm_amd import _lib
    name, n_args = "mmsbm_hip_recommend_assortment", 17
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmsbm_hip.h")).read(), flags=re.S)
    assert "#define MMSBM_HIP_ABI_VERSION 1" in text
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert decl and len(decl.group(1).split(",")) == n_args
    assert len(_lib.SIGNATURES[name][1]) == n_args
    for macro, value in (("ASSORT_BEST", HipEM.ASSORT_MODES["best_score"]), ("ASSORT_REACH", HipEM.ASSORT_MODES["reach"]),
                         ("ASSORT_MAX_C", HipEM.MAX_ASSORT), ("ASSORT_STOP_C", HipEM.ASSORT_STOPS.index("c")),
                         ("ASSORT_STOP_NO_GAIN", HipEM.ASSORT_STOPS.index("no_gain")),
                         ("ASSORT_STOP_NO_CANDIDATES", HipEM.ASSORT_STOPS.index("no_candidates"))):
        assert re.search(rf"#define MMSBM_HIP_{macro} {value}\b", text), macro
    assert callable(HipEM.recommend_assortment)
    assert f'"{name}"' in open(os.path.join(ROOT, "mmsbm_amd", "core.py")).read()
    options = open(os.path.join(ROOT, "mmsbm_amd", "csrc", "tu_options.hip")).read()
    assert all(f'"{o}"' in options for o in ("assortment_ms", "assortment_run_blocks", "assortment_part_bytes"))
    from mmsbm_amd.serving import Serving
    assert Serving.ASSORTMENT_MAX == HipEM.MAX_ASSORT
