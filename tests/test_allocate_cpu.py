"""Capacity-aware allocation, without a GPU: the two references of test_gpu_allocate.py (allocate_reference.py) against
each other and against what defines a stable assignment; the host plan of the query (serve_plan.hpp: plan_allocate);
the parsing of MMSBM.allocate's ``capacity`` (serving.allocate_capacity) and the host method over a stand-in device."""
import functools
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pandas as pd
import pytest

import allocate_reference as ar
import exact_models as xm
import fake_device
from conftest import ROOT
from mmsbm_amd.core import HipEM
from test_recommend_cpu import RecommendFakeHipEM, fitted, restate_scores, string_frame

VARIANTS = [("mixed", "stars"), ("sorted", "indicator"), ("constant", "indicator")]
SHAPES = [(300, 997, 7, 9, 5, 3), (260, 1021, 9, 5, 4, 4), (2500, 40, 4, 6, 5, 2)]
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]


def same_answer(got, want, what):
    for g, w, nm in zip(got, want, ("items", "scores", "counts")):
        gb, wb = (xm.bits(g), xm.bits(w)) if nm == "scores" else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        assert gb.shape == wb.shape and np.array_equal(gb, wb), (what, nm)


def cap_sets(rng, I):
    return [(1, np.full(I, 1)), (3, np.full(I, 2)), (10, np.full(I, 5)), (10, rng.choice(np.array([0, 1, 2, 5, -1]), I))]


# ---- 1. the walk and the threshold rounds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_the_rounds_reach_the_walk(variant, shape):
    U, I, K, L, R, S = shape
    case = xm.make_case(*variant, shape)
    users, scores, seen = case["users"], case["scores"], case["seen"]
    short = 0
    for n, caps in cap_sets(np.random.default_rng(xm.case_seed(*variant, shape)), I):
        what = f"n={n} caps={caps[:4].tolist()}"
        want = ar.greedy(scores, users, n, caps, seen)
        got, rounds, converged, taus = ar.threshold_rounds(scores, users, n, caps, seen)
        same_answer(got, want, what)
        assert converged and rounds == len(taus) >= 2, what
        for (s0, u0), (s1, u1) in zip(taus, taus[1:]):                     # a threshold only rises
            assert ((s1 > s0) | ((s1 == s0) & ((u1 <= u0) | (u0 < 0)))).all(), what
        assert all(np.array_equal(a, b) for a, b in zip(taus[-1], taus[-2])) if rounds > 1 else True
        ar.check_feasible(want, scores, users, n, caps, seen)
        assert len(ar.blocking_pairs(want, scores, users, n, caps, seen)) == 0, what
        short += int((want[2] < n).sum())
        # a cap that binds: some item is used up, and the plain query would overrun it
        plain = xm.exact_top_n(scores, users, n, seen)
        finite = caps >= 0
        assert (ar.loads(plain, I)[finite] > caps[finite]).any() and (ar.loads(want, I)[finite] == caps[finite]).any(), what
    assert short > 0                                                       # short rows and their padding are exercised


def test_a_blocking_pair_is_found():
    """The checks themselves: an answer that gives an item to the wrong user has a blocking pair, one beyond a cap is
    not feasible."""
    scores = np.array([[3.0, 1.0], [2.0, 1.0]])
    users, caps = np.array([0, 1]), np.array([1, 1])
    right = ar.greedy(scores, users, 1, caps)
    assert right[0].tolist() == [[0], [1]] and len(ar.blocking_pairs(right, scores, users, 1, caps)) == 0
    wrong = (np.array([[1], [0]], dtype=np.int32), np.array([[1.0], [2.0]]), np.array([1, 1], dtype=np.int32))
    assert ar.blocking_pairs(wrong, scores, users, 1, caps).tolist() == [[0, 0]]
    over = (np.array([[0], [0]], dtype=np.int32), np.array([[3.0], [2.0]]), np.array([1, 1], dtype=np.int32))
    with pytest.raises(AssertionError):
        ar.check_feasible(over, scores, users, 1, caps)


@pytest.mark.parametrize("variant,shape", CASES[:2] + CASES[-1:], ids=CASE_IDS[:2] + CASE_IDS[-1:])
def test_identities_of_the_references(variant, shape):
    U, I, K, L, R, S = shape
    case = xm.make_case(*variant, shape)
    users, scores, seen = case["users"], case["scores"], case["seen"]
    rng = np.random.default_rng(1)
    for n in (1, 10, 257):
        # nothing binds: recommend_query
        want = xm.exact_top_n(scores, users, n, seen)
        for caps in (np.full(I, -1), np.full(I, U), rng.choice(np.array([-3, U, U + 5]), I)):
            same_answer(ar.greedy(scores, users, n, caps, seen), want, f"unlimited n={n}")
            got, rounds, converged, _ = ar.threshold_rounds(scores, users, n, caps, seen)
            same_answer(got, want, f"unlimited n={n}")
            assert (rounds, converged) == (1, True)
    # candidates: capacity 0 on the rest IS the walk over the candidates' columns alone
    cand = np.sort(rng.choice(I, I // 3, replace=False))
    caps = rng.choice(np.array([1, 2, 5, -1]), I)
    rest0 = np.where(np.isin(np.arange(I), cand), caps, 0)
    column = {int(i): c for c, i in enumerate(cand.tolist())}
    inside = [{column[i] for i in s if i in column} for s in seen]
    sub = ar.greedy(scores[:, cand], users, 10, caps[cand], inside)
    back = (np.where(sub[0] >= 0, cand[np.maximum(sub[0], 0)], -1), sub[1], sub[2])
    same_answer(ar.greedy(scores, users, 10, rest0, seen), back, "candidates")
    # a subset of the users in another order: every user's row is the same
    some = rng.choice(U, min(U, 90), replace=False)
    a = ar.greedy(scores[some], some, 3, np.full(I, 2), seen)
    order = rng.permutation(len(some))
    b = ar.greedy(scores[some[order]], some[order], 3, np.full(I, 2), seen)
    same_answer(tuple(x[order] for x in a), b, "request order")
    # a round limit: feasible, a subset of nothing in particular, flagged
    got, rounds, converged, _ = ar.threshold_rounds(scores, users, 3, np.full(I, 2), seen, max_rounds=2)
    assert (rounds, converged) == (2, False)
    ar.check_feasible(got, scores, users, 3, np.full(I, 2), seen)


# ---- 2. the host plan -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_exe(tmp):
    exe = os.path.join(tmp, "allocate_plan_dump")
    src = os.path.join(ROOT, "tests", "native", "allocate_plan_dump.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


def device_plan(exe, caps, n_users, U, max_n=1024, force_bi=0):
    words = [len(caps), *np.asarray(caps).tolist(), n_users, U, max_n, force_bi]
    run = subprocess.run([exe], input=" ".join(str(int(x)) for x in words), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in run.stdout.splitlines()}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_host_plan(tmp_path_factory):
    exe = plan_exe(str(tmp_path_factory.mktemp("allocate_plan")))
    caps = np.array([0, 1, -1, 5, 299, 300, 301, 2 ** 31 - 1, -(2 ** 31), 0, 7, 1024, 2, 3])
    for n_users in (1, 2, 8, 300, 301, 1025):
        got = device_plan(exe, caps, n_users, 5000)
        binds = (caps > 0) & (caps < n_users)
        assert got["refused"] == [-1]
        assert got["item"] == np.flatnonzero(binds).tolist() and got["cap"] == caps[binds].tolist(), n_users
        assert got["closed"] == [0, 9]
        assert got["most_n"] == [int(caps[binds].max()) if binds.any() else 0]
        assert got["bi"] == [int(binds.sum())] and got["batch_n"] == ([got["most_n"][0]] if binds.any() else [])
    # a cap beyond the selection's list that could bind is refused, with its item; at n_users = cap it cannot bind
    assert device_plan(exe, [3, 1025, 1026], 1026, 5000)["refused"] == [1]
    assert device_plan(exe, [3, 1025, 1026], 1025, 5000)["refused"] == [-1]
    assert device_plan(exe, [3, 20, 11], 30, 5000, max_n=10) == {"item": [], "cap": [], "closed": [], "batch_n": [],
                                                                "refused": [1], "bi": [0], "most_n": [0]}
    # batches of the item pass: each selects with its own largest cap
    caps = np.array([4, 1, 9, -1, 2, 2, 0, 3, 7, 1])
    got = device_plan(exe, caps, 100, 5000, force_bi=3)
    assert got["item"] == [0, 1, 2, 4, 5, 7, 8, 9] and got["bi"] == [3] and got["batch_n"] == [9, 3, 7] and got["most_n"] == [9]
    # ... and by rec_batch_users over the U columns: 128 MB of scores, whole 128-row tiles
    got = device_plan(exe, np.full(20000, 50), 99997, 99997)
    bi = xm.batch_users(99997, 20000)
    assert got["bi"] == [bi] and bi % 128 == 0 and len(got["batch_n"]) == -(-20000 // bi)


# ---- 3. capacity= ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def serving():
    from mmsbm_amd import serving
    return serving


def test_every_accepted_form_of_capacity(serving):
    side = serving._Side("items", 6, np.asarray(list("abcdef"), dtype=object))
    for q in (0, 1, 7, np.int64(3), np.int32(2)):
        caps = serving.allocate_capacity(q, side)
        assert caps.dtype == np.int32 and caps.tolist() == [int(q)] * 6
    table = {"c": 2, "a": 0, "nobody": 5, "f": np.int64(9)}
    for form in (table, pd.Series(table)):
        assert serving.allocate_capacity(form, side).tolist() == [0, -1, 2, -1, -1, 9]      # unnamed: unlimited; unknown: ignored
    assert serving.allocate_capacity({}, side).tolist() == [-1] * 6
    assert serving.allocate_capacity({"a": 2 ** 40}, side).tolist()[0] == 2 ** 31 - 1
    # integer labels (the encoder's labels are their str), and ids as their own labels after fit_encoded
    assert serving.allocate_capacity({3: 1, "4": 2}, serving._Side("items", 6, np.asarray([str(j) for j in range(6)], dtype=object))).tolist() == [-1, -1, -1, 1, 2, -1]
    assert serving.allocate_capacity({3: 1, 99: 2, "4": 2}, serving._Side("items", 6)).tolist() == [-1, -1, -1, 1, -1, -1]
    for bad in (True, False, -1, 1.0, 2.5, "2", None, np.bool_(True), [1, 2]):
        with pytest.raises(ValueError, match="capacity"):
            serving.allocate_capacity(bad, side)
        with pytest.raises(ValueError, match="capacity"):
            serving.allocate_capacity({"a": bad}, side)
        with pytest.raises(ValueError, match="capacity"):
            serving.allocate_capacity({"not-an-item": bad}, side)


def test_item_load(serving):
    recs = pd.DataFrame({"users": list("aabbc"), "items": ["x", "y", "y", "z", "y"], "score": 1.0, "rank": 1})
    load = serving.Serving.item_load(recs)
    assert list(load.columns) == ["items", "count"] and load["items"].tolist() == ["y", "x", "z"] and load["count"].tolist() == [3, 1, 1]
    assert len(serving.Serving.item_load(recs[:0])) == 0


# ---- 4. the host method over a stand-in device ---------------------------------------------------------------------------------------
class AllocateFakeHipEM(RecommendFakeHipEM):
    """RecommendFakeHipEM with recommend_allocate, answered by the threshold rounds over the restated scores."""

    def recommend_allocate(self, users, n, caps, max_rounds=10000):
        assert self._rc["params"], "recommend_allocate before recommend_add"
        u, caps = np.asarray(users), np.asarray(caps)
        assert u.dtype == np.int32 and caps.dtype == np.int32 and caps.shape == (self.n_items,) and 1 <= n <= 1024
        assert len(set(u.tolist())) == len(u) and max_rounds >= 1
        fake_device.LOG.append(("recommend_allocate", len(u), n))
        scores = restate_scores(self._rc["params"], u, self.n_items, self._rc["w"])
        got, rounds, converged, _ = ar.threshold_rounds(scores, u, n, caps, self._rc["seen"], max_rounds)
        return (*got, {"rounds": rounds, "converged": converged})


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", AllocateFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(AllocateFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def test_the_host_method(host):
    m = fitted(host, string_frame(), sampling=2)
    items, users = m.data_handler.item_labels(), m.data_handler.user_labels()
    ask = ["u7", "u1", "u3", "u0"]
    plain = m.recommend(users=ask, n=3)
    fake_device.LOG.clear()
    got = m.allocate(n=3, capacity=1, users=ask)
    kinds = [e[0] for e in fake_device.LOG]
    assert kinds.count("recommend_add") == 2 and kinds.count("recommend_allocate") == 1 and kinds[-1] == "recommend_end"
    assert list(got.columns) == list(plain.columns) == ["users", "items", "score", "rank"]
    assert got["users"].unique().tolist() == ask and got["items"].value_counts().max() == 1
    assert not got["items"].equals(plain["items"]) and plain["items"].value_counts().max() > 1
    for u in ask:
        assert got[got["users"] == u]["rank"].tolist() == list(range(1, 1 + (got["users"] == u).sum()))
    a = m.allocation_
    assert a == {"rounds": a["rounds"], "converged": True, "filled": len(got), "requested": 12} and a["rounds"] > 1
    assert m.item_load(got)["count"].tolist() == [1] * len(got)
    # nothing binds: recommend's frame
    assert m.allocate(n=3, capacity=len(ask), users=ask).equals(plain) and m.allocation_["rounds"] == 1
    assert m.allocate(n=3, capacity={}, users=ask).equals(plain)
    assert m.allocate(n=2, capacity={"nobody": 0}).equals(m.recommend(n=2))
    # candidates: capacity 0 on every other item
    cand = items[::2]
    within = m.allocate(n=3, capacity=2, users=ask, candidates=cand)
    assert within.equals(m.allocate(n=3, capacity={i: (2 if i in cand else 0) for i in items}, users=ask))
    assert set(within["items"]) <= set(cand) and within["items"].value_counts().max() <= 2
    assert len(m.allocate(n=3, capacity=2, users=ask, candidates=[])) == 0 and m.allocation_["filled"] == 0
    # an empty request, a round limit, the refusals
    empty = m.allocate(n=3, capacity=1, users=[])
    assert len(empty) == 0 and list(empty.columns) == list(plain.columns) and m.allocation_["requested"] == 0
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        m.allocate(n=3, capacity=1)
    with pytest.warns(RuntimeWarning, match="max_rounds = 1"):
        cut = m.allocate(n=3, capacity=1, max_rounds=1)
    assert m.allocation_["converged"] is False and cut["items"].value_counts().max() == 1
    with pytest.raises(TypeError, match="capacity="):
        m.allocate(n=3)
    with pytest.raises(ValueError, match="distinct"):
        m.allocate(n=1, capacity=1, users=["u7", "u1", "u7"])
    with pytest.raises(KeyError):
        m.allocate(n=1, capacity=1, users=["nobody"])
    with pytest.raises(KeyError):
        m.allocate(n=1, capacity=1, candidates=["not-an-item"])
    for kw in ({"n": 0}, {"n": True}, {"max_rounds": 0}, {"max_rounds": 2.0}, {"capacity": -1}, {"capacity": 1.5}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            m.allocate(**{"capacity": 1, **kw})


# ---- 5. header, signature and wrapper agree ------------------------------------------------------------------------------------------
def test_header_signature_and_wrapper_agree():
    from mmsbm_amd import _lib
    name, n_args = "mmsbm_hip_recommend_allocate", 11
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmsbm_hip.h")).read(), flags=re.S)
    assert "#define MMSBM_HIP_ABI_VERSION 1" in text
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert decl and len(decl.group(1).split(",")) == n_args
    assert len(_lib.SIGNATURES[name][1]) == n_args
    assert callable(HipEM.recommend_allocate)
    assert f'"{name}"' in open(os.path.join(ROOT, "mmsbm_amd", "core.py")).read()
    options = open(os.path.join(ROOT, "mmsbm_amd", "csrc", "tu_options.hip")).read()
    assert '"allocate_ms"' in options and '"allocate_rounds"' in options
