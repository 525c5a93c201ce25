"""Randomised top-N with propensities, without a GPU: the reference of test_gpu_explore.py (explore_reference.py) pinned
to the Plackett-Luce distribution it claims to draw from and to the properties of its propensities; the three C entries
in the binding; the argument checks of MMSBM.recommend_explore / propensities, the temperature floor among them."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import explore_reference as er
from conftest import ROOT

NEW_SYMBOLS = ("mmsbm_hip_recommend_query_explore", "mmsbm_hip_recommend_list_propensity", "mmsbm_hip_explore_noise")


# ---- 1. the reference draws from Plackett-Luce -----------------------------------------------------------------------------
def test_the_reference_is_plackett_luce():
    """4,096 rows with the same eight scores, T = 0.5, seed 0, n = 3: every item's first-place frequency and top-3
    inclusion frequency within 4 standard errors of the exact probabilities (the 336 ordered triples enumerated).  A
    condition on a fixed seed, not a measurement."""
    users = np.arange(er.PL_ROWS)
    scores = np.tile(er.PL_SCORES, (er.PL_ROWS, 1))
    g = er.gumbel(er.uniform_rows(er.PL_SEED, users, len(er.PL_SCORES)))
    items, _, prop, counts = er.explore(scores, users, er.PL_T, g, er.PL_N)
    assert (counts == er.PL_N).all() and er.pl_exact(er.PL_SCORES, er.PL_T, er.PL_N)[2] == 336
    d_first, d_incl = er.pl_deviations(items, er.PL_SCORES, er.PL_T, er.PL_N)
    print(f"largest deviations: first place {d_first:.2f}, top-3 inclusion {d_incl:.2f} standard errors")
    assert d_first <= 4.0 and d_incl <= 4.0, (d_first, d_incl)


def test_the_uniform_is_the_stream_at_its_own_offset():
    """uniform_rows (one advance per user, consecutive draws) is the definition (one advance per pair), beyond 2^32 and
    2^62 too; r = 0 maps to E = 2^-54."""
    users = [0, 1, 2, 65_535, 2 ** 31 - 1]
    rows = er.uniform_rows(7, users, 70)
    for b, u in enumerate(users):
        for i in (0, 1, 63, 64, 69):
            assert rows[b, i] == er.uniform(7, u, i), (u, i)
    assert er.uniform(7, 1, 0) != er.uniform(7, 0, 0) and er.uniform(7, 3, 5) != er.uniform(8, 3, 5)
    g = er.gumbel(np.array([0.0, 0.5, 1.0 - 2.0 ** -53]))
    assert g[0] == -np.log(2.0 ** -54) and np.isfinite(g).all() and g[1] == -np.log(-np.log(0.5))


# ---- 2. the reference's propensities ------------------------------------------------------------------------------------------
def test_the_propensities_of_the_reference():
    rng = np.random.default_rng(3)
    s = er.PL_SCORES
    first, _, _ = er.pl_exact(s, er.PL_T, 3)
    w = np.exp((s - s.max()) / er.PL_T)
    for _ in range(20):
        order = rng.permutation(len(s))
        p = er.row_propensities(s, order, er.PL_T)
        # a row's propensities multiply to the probability of its list, prefix by prefix
        left, pr = w.sum(), 1.0
        for t, i in enumerate(order):
            pr *= w[i] / left
            left -= w[i]
            assert np.prod(p[:t + 1]) == pytest.approx(pr, rel=1e-12)
        assert p[0] == pytest.approx(first[order[0]], rel=1e-13)
        assert p[-1] == 1.0                                             # the last remaining candidate: exactly
    # fewer candidates than n: the row ends in exactly 1.0, the padding is 0
    seen = [set(range(2, 8))]
    items, sc, prop, counts = er.explore(s[None, :], [0], er.PL_T, np.zeros((1, 8)), 5, seen=seen)
    assert counts[0] == 2 and prop[0, 1] == 1.0 and (prop[0, 2:] == 0).all() and (items[0, 2:] == -1).all()
    # a given list with non-candidates: 0 / -inf, and the rest as if they were absent
    ok = np.ones(8, dtype=bool)
    ok[[1, 6]] = False
    got_s, got_p = er.list_propensity(s, ok, er.PL_T, [3, 1, 0, 6, 7])
    want_s, want_p = er.list_propensity(s, ok, er.PL_T, [3, 0, 7])
    assert np.array_equal(got_p[[0, 2, 4]], want_p) and np.array_equal(got_s[[0, 2, 4]], want_s)
    assert (got_p[[1, 3]] == 0).all() and np.isneginf(got_s[[1, 3]]).all()
    # the list of every candidate, in any order, ends in exactly 1.0 and multiplies to a permutation's probability
    full = rng.permutation(np.flatnonzero(ok))
    assert er.list_propensity(s, ok, er.PL_T, full)[1][-1] == 1.0
    # explore's own propensities are list_propensity of its list
    g = er.gumbel(er.uniform_rows(5, [9], 8))
    items, sc, prop, counts = er.explore(s[None, :], [9], er.PL_T, g, 4)
    assert np.array_equal(er.list_propensity(s, np.ones(8, dtype=bool), er.PL_T, items[0])[1], prop[0])


def test_a_difference_loses_the_concentrated_rows():
    """Seven items carry nearly all of the mass (the "rare" family of the GPU test at T = 2^-7): R_t formed as the
    full-row sum minus the head has no correct digit left from position 8 on; accumulated from what remains it agrees
    with extended precision."""
    s = np.full(997, 2.25)
    s[[3, 100, 200, 300, 400, 500, 600]] = 3.0
    order = np.lexsort((np.arange(997), -s))
    T = 2.0 ** -7
    assert (s.max() - s.min()) / T <= er.FLOOR
    good, wide = er.row_propensities(s, order, T)[:10], er.row_propensities(s, order, T, np.longdouble)[:10]
    assert np.allclose(good, wide, rtol=1e-11, atol=0.0) and good[7] == pytest.approx(1.0 / 990, rel=1e-11)
    bad = er.row_propensities_by_difference(s, order, T)[:10]
    assert not np.allclose(bad[7:], wide[7:], rtol=1e-11, atol=0.0, equal_nan=False)


# ---- 3. the binding ---------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_declared_and_bound():
    from mmsbm_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmsbm_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert decl, f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
        assert hasattr(lib, name), f"{name} is not exported"
    from mmsbm_amd.core import HipEM
    for method in ("recommend_query_explore", "recommend_list_propensity", "explore_noise"):
        assert callable(getattr(HipEM, method))


# ---- 4. the host class's argument checks -----------------------------------------------------------------------------------------
@pytest.fixture()
def model():
    """A fitted model's surface without a device: any call that reached one fails the test."""
    from mmsbm_amd import serving

    class Stub(serving.Serving):
        sampling, _restart_ids, data_handler = 1, [0], None
        ratings, p, m = np.arange(1.0, 6.0), 9, 19

        def _check_is_fitted(self):
            pass

        def _restarts(self):
            raise AssertionError("the device was asked")

    return Stub()


def test_temperature_is_required_and_checked(model):
    recs = pd.DataFrame({"users": [0, 0, 1], "items": [3, 4, 3]})
    with pytest.raises(TypeError, match="temperature="):
        model.recommend_explore()
    with pytest.raises(TypeError, match="temperature="):
        model.propensities(recs)
    for call in (lambda t: model.recommend_explore(temperature=t), lambda t: model.propensities(recs, temperature=t)):
        for bad in (-1.0, float("nan"), float("inf"), "1", None, True):
            with pytest.raises(ValueError, match="temperature"):
                call(bad)
    with pytest.raises(ValueError, match="temperature must be > 0"):
        model.propensities(recs, temperature=0)


def test_a_temperature_below_the_floor_names_the_floor(model):
    from mmsbm_amd import serving
    recs = pd.DataFrame({"users": [0, 0, 1], "items": [3, 4, 3]})
    floor = 4.0 / 700.0                                                   # the default weights are the ratings 1 .. 5
    for call in (lambda **kw: model.recommend_explore(**kw), lambda **kw: model.propensities(recs, **kw)):
        with pytest.raises(ValueError, match=re.escape(repr(floor))):
            call(temperature=floor * 0.999)
        with pytest.raises(ValueError, match=re.escape(repr(20.0 / 700.0))):
            call(temperature=0.02, weights=[0, 0, 0, 0, 20])
        with pytest.raises(AssertionError, match="the device was asked"):   # just above the floor the call goes on
            call(temperature=floor * 1.001)
    assert serving.explore_temperature(1e-9, np.ones(5)) == 1e-9          # equal weights: every score ties, no floor
    assert serving.explore_temperature(0, np.arange(5.0)) == 0.0
    assert serving.EXPLORE_FLOOR == er.FLOOR


def test_the_other_arguments(model):
    from mmsbm_amd import serving
    from mmsbm_amd.core import pcg64_words
    with pytest.raises(ValueError, match="n must be"):
        model.recommend_explore(n=0, temperature=1.0)
    with pytest.raises(ValueError, match="PCG64"):
        model.recommend_explore(temperature=1.0, seed=np.random.Generator(np.random.MT19937(1)))
    gen = np.random.default_rng(11)
    before = gen.bit_generator.state
    assert list(serving.explore_stream(gen)) == list(pcg64_words(np.random.default_rng(11).bit_generator))
    assert gen.bit_generator.state == before                               # read, not advanced
    assert list(serving.explore_stream(11)) == list(serving.explore_stream(gen))
    with pytest.raises(ValueError, match="first two columns"):
        model.propensities([(0, 1)], temperature=1.0)
    with pytest.raises(KeyError):
        model.propensities(pd.DataFrame({"users": [0, 99], "items": [1, 1]}), temperature=1.0)
    with pytest.raises(KeyError):
        model.propensities(pd.DataFrame({"users": [0, 1], "items": [1, 20]}), temperature=1.0)
    with pytest.raises(ValueError, match="twice"):
        model.propensities(pd.DataFrame({"users": [0, 1, 0], "items": [1, 1, 1]}), temperature=1.0)
    long = pd.DataFrame({"users": [0] * 20, "items": list(range(20))})
    model.RECOMMEND_MAX = 19
    with pytest.raises(ValueError, match="at most 19"):
        model.propensities(long, temperature=1.0)
