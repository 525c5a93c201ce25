"""Welfare-maximising assignment, without a GPU: the references of test_gpu_assign.py (assign_reference.py) against brute
force, against each other and against what the auction guarantees; MMSBM.assign over a stand-in device; the header, the
ctypes signature and the wrapper; and the condition on the GPU cases (assign_cases.py) that the reference converges."""
import itertools
import math
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pandas as pd
import pytest

import assign_cases as ac
import assign_reference as ar
import fake_device
from conftest import ROOT
from mmsbm_amd.core import HipEM
from test_recommend_cpu import RecommendFakeHipEM, fitted, restate_scores, string_frame


def random_problems(n=200, seed=20261021):
    """n problems of <= 40 users x 12 items: scores in eighths (ties are common), -inf pairs, caps from {0, 1, 2, 3, 5,
    unlimited}, a reserve below, inside and above the scores, user ids in any order."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        U, I = int(rng.integers(1, 41)), int(rng.integers(1, 13))
        scores = rng.integers(0, 64, (U, I)) / 8.0
        scores[rng.random((U, I)) < 0.2] = -np.inf
        caps = rng.choice(np.array([0, 1, 2, 3, 5, -1]), I)
        reserve = float(rng.choice([-1.0, 2.0, 4.0, 9.0]))
        eps = float(rng.choice([0.5, 2.0 ** -4, 0.01]))
        yield scores, rng.permutation(100)[:U], caps, reserve, eps


# ---- 1. the exact solver ---------------------------------------------------------------------------------------------------
def test_optimum_against_brute_force():
    rng = np.random.default_rng(5)
    for _ in range(120):
        U, I = int(rng.integers(1, 7)), int(rng.integers(1, 4))
        scores = rng.integers(0, 8, (U, I)) / 4.0
        scores[rng.random((U, I)) < 0.25] = -np.inf
        caps = rng.choice(np.array([0, 1, 2, 3, -1]), I)
        reserve = float(rng.choice([-0.5, 0.75, 3.0]))
        users = rng.permutation(20)[:U]
        value, items = ar.optimum(scores, users, caps, reserve)
        assert value == ar.brute(scores, users, caps, reserve), (scores, caps, reserve)
        got = items >= 0
        assert math.fsum(scores[np.flatnonzero(got), items[got]].tolist() + [reserve] * int((~got).sum())) == value
        load = np.bincount(items[got], minlength=I)
        assert (load[caps >= 0] <= caps[caps >= 0]).all()


def test_optimum_against_scipy():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for scores, users, caps, reserve, _ in random_problems():
        M, _, _ = ar._expanded(scores, users, caps, reserve, None)
        cost = np.where(np.isfinite(M), -M, 1e9)
        r, c = lsa(cost)
        assert abs(-cost[r, c].sum() - ar.optimum(scores, users, caps, reserve)[0]) < 1e-9


# ---- 2. the auction: what it guarantees -------------------------------------------------------------------------------------
def test_the_auction_on_random_problems():
    worst = 0.0
    for scores, users, caps, reserve, eps in random_problems():
        best, _ = ar.optimum(scores, users, caps, reserve)
        res = ar.auction(scores, users, caps, reserve, eps)
        assert res["converged"] and res["rounds"] >= 1
        ar.check_feasible(res, scores, users, caps)
        sm = ar.summary(res, reserve, eps)
        tiny = 1e-9                                                  # (sums of a few dozen eighths and bids: far below)
        assert -tiny <= best - sm["value"] <= sm["gap_limit"] + tiny, (best, sm)
        assert sm["bound"] >= best - tiny and sm["bound"] - sm["value"] <= sm["gap_limit"] + tiny, (best, sm)
        got = res["items"] >= 0
        assert (res["score"][got] - res["paid"][got] >= res["pi"][got] - eps - 1e-12).all()      # eps-complementary slackness
        assert (res["pi"][~got] == reserve).all() and res["dropped"][~got].all() and not res["dropped"][got].any()
        free = ar.unlimited(caps, len(users))
        for i, (price, holder) in res["slots"].items():             # slots nobody bid on keep price 0; prices ascend
            assert (np.diff(price) >= 0).all() and (price[holder < 0] == 0).all() and res["p1"][i] == price[0]
        assert (res["p1"][free] == 0).all() and np.isposinf(res["p1"][caps == 0]).all()
        if sm["gap_limit"] > 0:
            worst = max(worst, (best - sm["value"]) / sm["gap_limit"])
    assert worst <= 1.0


def test_the_request_order_does_not_matter():
    for scores, users, caps, reserve, eps in itertools.islice(random_problems(seed=9), 40):
        a = ar.auction(scores, users, caps, reserve, eps)
        order = np.random.default_rng(1).permutation(len(users))
        b = ar.auction(scores[order], users[order], caps, reserve, eps)
        for k in ("items", "score", "paid", "pi"):
            assert np.array_equal(a[k][order], b[k]), k
        for k in ("p1", "price_sum", "load"):
            assert np.array_equal(a[k], b[k]), k
        assert (a["rounds"], a["bids"]) == (b["rounds"], b["bids"])


def test_a_round_limit_is_feasible_and_bounded():
    hit = 0
    for scores, users, caps, reserve, eps in itertools.islice(random_problems(seed=11), 60):
        res = ar.auction(scores, users, caps, reserve, eps, max_rounds=2)
        ar.check_feasible(res, scores, users, caps)
        assert res["rounds"] <= 2
        hit += not res["converged"]
        assert ar.summary(res, reserve, eps)["bound"] >= ar.optimum(scores, users, caps, reserve)[0] - 1e-9
    assert hit > 10


# ---- 3. nothing capped: the per-user arg-max ---------------------------------------------------------------------------------
def test_unlimited_caps_give_the_argmax():
    for scores, users, _, reserve, eps in itertools.islice(random_problems(seed=13), 60):
        U, I = scores.shape
        for caps in (np.full(I, -1), np.full(I, U), np.full(I, 2 ** 31 - 1)):
            res = ar.auction(scores, users, caps, reserve, eps)
            best = scores.max(axis=1)
            want = np.where(best > reserve, np.argmax(scores, axis=1), -1)
            assert np.array_equal(res["items"], want) and res["rounds"] == 1 and res["converged"]
            assert (res["paid"] == 0).all() and (res["p1"] == 0).all() and (res["price_sum"] == 0).all()
            assert np.array_equal(res["pi"], np.maximum(best, reserve))


# ---- 4. the host method over a stand-in device -----------------------------------------------------------------------------------
class AssignFakeHipEM(RecommendFakeHipEM):
    """RecommendFakeHipEM with recommend_assign, answered by the reference over the restated scores."""

    def recommend_assign(self, users, caps, reserve, epsilon, max_rounds=10000):
        assert self._rc["params"], "recommend_assign before recommend_add"
        u, caps = np.asarray(users), np.asarray(caps)
        assert u.dtype == np.int32 and caps.dtype == np.int32 and caps.shape == (self.n_items,)
        assert len(set(u.tolist())) == len(u) and max_rounds >= 1 and epsilon > 0 and reserve < np.inf
        fake_device.LOG.append(("recommend_assign", len(u), float(reserve), float(epsilon)))
        scores = restate_scores(self._rc["params"], u, self.n_items, self._rc["w"])
        res = ar.auction(scores, u, caps, reserve, epsilon, self._rc["seen"], max_rounds)
        return {"items": res["items"], "scores": res["score"], "paid": res["paid"], "pi": res["pi"], "price": res["p1"],
                "price_sum": res["price_sum"], "load": res["load"], "rounds": res["rounds"], "bids": res["bids"],
                "converged": res["converged"]}


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", AssignFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(AssignFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def test_the_host_method(host):
    m = fitted(host, string_frame(), sampling=2)
    items, users = m.data_handler.item_labels(), m.data_handler.user_labels()
    ask = ["u7", "u1", "u3", "u0"]
    plain = m.recommend(users=ask, n=1)
    fake_device.LOG.clear()
    got = m.assign(capacity=1, epsilon=0.125, users=ask)
    kinds = [e[0] for e in fake_device.LOG]
    assert kinds.count("recommend_add") == 2 and kinds.count("recommend_assign") == 1 and kinds[-1] == "recommend_end"
    assert list(got.columns) == ["users", "items", "score", "rank", "price"]
    assert got["users"].tolist() == ask and got["items"].value_counts().max() == 1 and (got["rank"] == 1).all()
    assert (got["price"] >= 0).all()
    # the default reserve: min(weights) - span, handed to the device
    w = np.asarray(m.ratings, dtype=np.float64)
    assert w.max() > w.min()
    assert fake_device.LOG[kinds.index("recommend_assign")][2:] == (float(w.min() - (w.max() - w.min())), 0.125)
    a = m.assignment_
    assert set(a) == {"rounds", "bids", "converged", "assigned", "dropped", "total", "value", "bound", "gap_limit", "prices"}
    assert a["converged"] is True and a["assigned"] == 4 and a["dropped"] == 0 and a["rounds"] >= 1 and a["bids"] >= 4
    assert a["total"] == math.fsum(got["score"].tolist()) == a["value"] and a["gap_limit"] == 4 * 0.125
    assert a["value"] <= a["bound"] <= a["value"] + a["gap_limit"] + 1e-12
    prices = a["prices"]
    assert list(prices.columns) == ["items", "price", "load", "capacity"] and len(prices) == len(items)
    assert prices["load"].sum() == 4 and (prices["capacity"] == 1).all() and (prices["load"] <= 1).all()
    # the three forms of capacity; items a dict does not name are unlimited and carry no price
    table = {lab: 1 for lab in items[::2]}
    for form in (table, pd.Series(table)):
        named = m.assign(capacity=form, epsilon=0.125, users=ask)
        assert len(m.assignment_["prices"]) == len(table) and len(named) == 4
        assert named[named["items"].isin(table)]["items"].value_counts().max() <= 1
    # nothing binds: recommend(n=1)'s frame, price 0
    for capacity in (len(ask), {}, {"nobody": 0}):
        free = m.assign(capacity=capacity, epsilon=0.125, users=ask)
        assert free.drop(columns="price").equals(plain) and (free["price"] == 0).all() and m.assignment_["rounds"] == 1
    # a reserve above every score: nobody is assigned, and the value is the reserves'
    none = m.assign(capacity=1, epsilon=0.125, users=ask, reserve=6.0)
    assert len(none) == 0 and list(none.columns) == list(got.columns)
    a = m.assignment_
    assert (a["assigned"], a["dropped"], a["total"], a["value"], a["bound"], a["gap_limit"]) == (0, 4, 0.0, 24.0, 24.0, 0.0)
    # candidates: capacity 0 on every other item
    cand = items[::2]
    within = m.assign(capacity=2, epsilon=0.125, users=ask, candidates=cand)
    assert within.equals(m.assign(capacity={i: (2 if i in cand else 0) for i in items}, epsilon=0.125, users=ask))
    assert set(within["items"]) <= set(cand) and within["items"].value_counts().max() <= 2
    assert len(m.assign(capacity=2, epsilon=0.125, users=ask, candidates=[])) == 0 and m.assignment_["assigned"] == 0
    # an empty request, a round limit, the refusals
    empty = m.assign(capacity=1, epsilon=0.125, users=[])
    assert len(empty) == 0 and list(empty.columns) == list(got.columns) and m.assignment_["value"] == 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        everyone = m.assign(capacity=1, epsilon=0.125)
    assert len(everyone) == len(users) and everyone["users"].tolist() == list(users)
    assert m.recommend(n=1)["items"].value_counts().max() > 1 and everyone["items"].value_counts().max() == 1
    assert (everyone["price"] > 0).any()
    with pytest.warns(RuntimeWarning, match="max_rounds = 1"):
        cut = m.assign(capacity=1, epsilon=0.125, max_rounds=1)
    assert m.assignment_["converged"] is False and cut["items"].value_counts().max() == 1 and len(cut) < len(users)
    assert m.assignment_["bound"] >= m.assignment_["value"]
    with pytest.raises(TypeError, match="capacity="):
        m.assign(epsilon=0.125)
    with pytest.raises(TypeError, match="epsilon="):
        m.assign(capacity=1)
    with pytest.raises(ValueError, match="distinct"):
        m.assign(capacity=1, epsilon=0.125, users=["u7", "u1", "u7"])
    with pytest.raises(KeyError):
        m.assign(capacity=1, epsilon=0.125, users=["nobody"])
    with pytest.raises(KeyError):
        m.assign(capacity=1, epsilon=0.125, candidates=["not-an-item"])
    for kw in ({"max_rounds": 0}, {"max_rounds": 2.0}, {"capacity": -1}, {"capacity": 1.5}, {"epsilon": 0}, {"epsilon": -1.0},
               {"epsilon": np.inf}, {"epsilon": np.nan}, {"epsilon": "1"}, {"epsilon": True}, {"epsilon": 4.0 * 2.0 ** -41},
               {"reserve": np.inf}, {"reserve": np.nan}, {"reserve": "0"}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            m.assign(**{"capacity": 1, "epsilon": 0.125, **kw})
    m.assign(capacity=1, epsilon=4.0 * 2.0 ** -40, users=ask[:1], reserve=-np.inf)       # the smallest epsilon; no reserve


# ---- 5. header, signature and wrapper agree ------------------------------------------------------------------------------------------
def test_header_signature_and_wrapper_agree():
    from mmsbm_amd import _lib
    name, n_args = "mmsbm_hip_recommend_assign", 16
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmsbm_hip.h")).read(), flags=re.S)
    assert "#define MMSBM_HIP_ABI_VERSION 1" in text
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert decl and len(decl.group(1).split(",")) == n_args
    assert len(_lib.SIGNATURES[name][1]) == n_args
    assert callable(HipEM.recommend_assign)
    assert f'"{name}"' in open(os.path.join(ROOT, "mmsbm_amd", "core.py")).read()
    options = open(os.path.join(ROOT, "mmsbm_amd", "csrc", "tu_options.hip")).read()
    assert all(f'"{o}"' in options for o in ("assign_ms", "assign_rounds", "assign_bids"))


# ---- 5b. the host plan (serve_plan.hpp: plan_assign), as a CPU program under the sanitizers ---------------------------------------------
def device_plan(exe, caps, n_users, max_n=1024):
    words = [len(caps), *np.asarray(caps).tolist(), n_users, max_n]
    run = subprocess.run([exe], input=" ".join(str(int(x)) for x in words), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in run.stdout.splitlines()}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_host_plan(tmp_path):
    exe = str(tmp_path / "assign_plan_dump")
    src = os.path.join(ROOT, "tests", "native", "assign_plan_dump.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    caps = np.array([0, 1, -1, 5, 299, 300, 301, 2 ** 31 - 1, -(2 ** 31), 0, 7, 1024, 2, 3])
    for n_users in (1, 2, 8, 300, 301, 1025):
        got = device_plan(exe, caps, n_users)
        want = np.where(ar.unlimited(caps, n_users), -1, caps)
        assert got["refused"] == [-1] and got["cap"] == want.tolist(), n_users
        assert got["slot_off"] == np.concatenate([[0], np.cumsum(np.maximum(want, 0))]).tolist()
        most = int(want.max())
        assert got["most"] == [max(most, 0)] and got["slots"] == [got["slot_off"][-1]]
        places = got["lds_places"][0]
        assert places >= max(most, 2) and places & (places - 1) == 0 and (places == 2 or places // 2 < most)
    # a cap beyond a slot list that could bind is refused, with its item; at n_users = cap it cannot bind
    assert device_plan(exe, [3, 1025, 1026], 1026)["refused"] == [1]
    assert device_plan(exe, [3, 1025, 1026], 1025)["refused"] == [-1]
    assert device_plan(exe, [3, 20, 11], 30, max_n=10)["refused"] == [1]
    assert device_plan(exe, [], 5) == {"cap": [], "slot_off": [0], "refused": [-1], "most": [0], "lds_places": [2], "slots": [0]}


# ---- 6. the GPU cases: the reference converges, and they exercise what they are there for -------------------------------------------------
@pytest.mark.parametrize("variant,shape", ac.CASES, ids=ac.CASE_IDS)
def test_the_gpu_cases_converge(variant, shape):
    U, I = shape[:2]
    case = ac.case_of(variant, shape)
    seen_rounds = []
    for name, exclude, kind in ac.combos():
        res = ac.expected(variant, shape, name, exclude, kind)
        what = (name, exclude, kind)
        assert res["converged"] and res["rounds"] <= ac.MAX_ROUNDS, what
        caps = ac.caps_of(name, variant, shape)
        ar.check_feasible(res, case["scores"], case["users"], caps, case["seen"] if exclude else None)
        sm = ar.summary(res, ac.reserve_of(kind, variant, shape), ac.epsilon_of(variant))
        assert sm["bound"] - sm["value"] <= sm["gap_limit"] + 1e-9 * max(1, U), (what, sm)
        seen_rounds.append(res["rounds"])
        if name == "cap2of40" and U > 80 and kind == "default":
            assert res["dropped"].sum() == U - 80 and res["bids"] > 10 * U, what       # drop-outs and displacement chains
    if U > 80:
        assert max(seen_rounds) > 50
    assert ac.epsilon_of(variant) >= float(np.max(case["w"]) - np.min(case["w"])) * 2.0 ** -40
