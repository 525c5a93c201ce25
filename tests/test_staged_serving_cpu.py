"""staged_serving.py without a device: the long-double restatement of explain against explain_reference.Restatement on
the friendly models of test_gpu_explain.py, the preconditions of the GPU cases as assertions (which rows are clamped,
the planted degrees, the audience bars and the path of aud_decide each takes), the two mutations the GPU file must
catch evaluated in numpy, and the check functions of test_gpu_staged_serving.py run through the CPU stand-ins of the
*_cpu.py files.  If a precondition fails for a seed, change the seed, not the threshold."""
import functools

import numpy as np
import pytest

import staged_after_fit as saf
import staged_serving as ss
from conftest import ELEMENT_FLOOR
from test_align_cpu import OverlapFakeHipEM
from test_audience_cpu import AudienceFakeHipEM, by_item
from test_diverse_cpu import DiverseFakeHipEM
from test_explain_cpu import ExplainFakeHipEM
from test_recommend_cpu import restate_scores

WEIGHTS = {"plain": ss.W, "down": ss.W_DOWN}
SHAPES = pytest.mark.parametrize("k,l", ss.SHAPES, ids=ss.SHAPE_IDS)


class StagedFakeHipEM(ExplainFakeHipEM, AudienceFakeHipEM, DiverseFakeHipEM, OverlapFakeHipEM):
    """Every stand-in the five entry points have, in one class.  The (U, I) restatement of an open recommend session
    is computed once per (weights, slots added) instead of once per query: the same numbers."""
    _memo = (None, None)

    def _scores(self, users):
        key = (self._rc["w"].tobytes(), len(self._rc["params"]))
        if self._memo[0] != key:
            self._memo = (key, restate_scores(self._rc["params"], np.arange(self.n_users), self.n_items, self._rc["w"]))
        return self._memo[1][np.asarray(users, dtype=np.int64)]

    def _item_side(self):
        assert self._rc["params"] and "new" not in self._rc
        seen = by_item(self._rc["seen"], self.n_items) if self._rc["seen"] is not None else None
        return np.ascontiguousarray(self._scores(np.arange(self.n_users)).T), seen, self.n_items


@functools.lru_cache(maxsize=None)
def restated(k, l, family, weights="plain", n_slots=ss.S):
    """The float64 restatement of the case's (U, I) scores: computed once, never written to."""
    scores = restate_scores(ss.case(k, l, family, n_slots=n_slots).params, np.arange(ss.U), ss.I, WEIGHTS[weights])
    scores.setflags(write=False)
    return scores


def stand_in(c):
    em = StagedFakeHipEM(c.data, c.k, c.l, *c.dims, slots=ss.S)
    for s, p in enumerate(c.params):
        em.select(s).set_params(*p)
    return em


# ---- the long-double restatement against the float64 one -----------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5), (20, 20), (70, 3)], ids=lambda s: f"K{s[0]}L{s[1]}")
def test_the_long_double_restatement_agrees_with_the_reference_on_friendly_models(shape):
    import test_gpu_explain as tge
    K, L = shape
    params, ref = tge.model(K, L, 3)
    users, offsets, items = tge.request()
    long = ss.LongExplain(tge.training_rows(), params, tge.W)
    worst = 0.0
    for u, t in tge.pairs_of(users, offsets, items):
        a, b = ref.pair(u, t), long.pair(u, t)
        assert a["degree"] == b["degree"] and np.array_equal(a["items"], b["items"]) and np.array_equal(a["ratings"], b["ratings"])
        for name, bound in (("a", ss.contribution_bound(K, L)), ("explained", ss.explained_bound(K, L, a["degree"])),
                            ("score", ss.explain_score_bound(K, L))):
            # (the reference adds `explained` row after row: d_u roundings instead of the device's tree)
            extra = a["degree"] * 2.0 ** -52 if name == "explained" else 0.0
            frac, small_ok = saf.score_errors(np.atleast_1d(a[name]), np.atleast_1d(b[name]), bound + extra, ELEMENT_FLOOR)
            worst = max(worst, frac)
            assert small_ok and frac <= 1.0, (shape, u, t, name, frac)
    print(f"{shape}: float64 restatement against long double, worst error / bound {worst:.3f}")


# ---- preconditions of the GPU cases ------------------------------------------------------------------------------------------
@SHAPES
def test_planted_degrees_zeroed_rows_and_duplicates(k, l):
    c = ss.case(k, l, "late")
    deg = ss.degrees(c)
    assert all(deg[u] == d for u, d in ss.PLANTED.items()) and deg.min() >= 1 and deg.max() == ss.ALL_ROWS
    assert 15 <= np.median(deg) <= 35
    assert len(c.data) > len({tuple(r) for r in c.data.tolist()}) + 40                # duplicated triples
    assert c.zero_users[0] in ss.PLANTED and ss.PLANTED[c.zero_users[0]] == 64
    for u in (17, 41, 53):                                                            # a zeroed item in planted histories
        assert np.isin(c.data[c.data[:, 0] == u][:, 1], c.zero_items).any()
    users, offsets, items = ss.explain_request(c)
    assert set(ss.PLANTED) <= set(users.tolist()) and set(c.zero_users) <= set(users.tolist())
    assert len(users) - len(set(users.tolist())) == 1 and np.isin(items, c.zero_items).sum() >= 3
    assert all(2 <= n <= 3 for n in np.diff(offsets))
    for s in range(ss.S):
        assert (c.params[s][0][list(c.zero_users)] == 0).all() and (c.params[s][1][list(c.zero_items)] == 0).all()


@pytest.mark.parametrize("family", ss.FAMILIES)
@SHAPES
def test_which_rows_exp_row_kernel_clamps(k, l, family):
    c = ss.case(k, l, family)
    dots = ss.row_dots(c)
    live = dots > 0
    below = float(np.mean(dots[live] < ss.EPS))
    print(f"K={k} L={l} {family}: {1 - live.mean():.3f} exact zeros, {below:.3f} of the others below eps")
    assert 0.01 <= 1 - live.mean() <= 0.06
    if family == "rowborder":
        assert 0.10 <= below <= 0.90
    elif family == "tiny":
        assert below == 1.0
    # the requested users: both sides of the clamp in the launch that serves them
    users = ss.explain_request(c)[0]
    mine = dots[:, np.isin(c.data[:, 0], users)]
    if family == "rowborder":
        assert ((mine > 0) & (mine < ss.EPS)).any() and (mine >= ss.EPS).any()


@pytest.mark.parametrize("family", ss.FAMILIES)
@SHAPES
def test_the_audience_bars_exist_and_take_the_path_the_test_says(k, l, family):
    for wname in ("plain",) + (("down",) if family == "tiny" else ()):
        w, scores = WEIGHTS[wname], restated(k, l, family, wname)
        bars = ss.audience_bars(scores)
        assert len(set(bars)) == len(bars) and bars[0] > 0
        ss.check_bar_paths(bars, ss.S)
        if w is ss.W_DOWN:
            assert scores.max() < 2.0 ** -1022 / ss.WIDE_S and scores[scores > 0].min() > 100 * ss.UNIT and len(bars) == 9
            between = bars[-1]
            assert not (scores == between).any() and (scores < between).any() and (scores > between).any()
        elif family == "tiny":
            assert ELEMENT_FLOOR < scores[scores > 0].min() and scores.max() < 1e-200


def test_the_wide_case_takes_the_divide_path():
    c = ss.case(7, 33, "tiny", n_slots=ss.WIDE_S)
    assert len(c.params) == ss.WIDE_S
    bars = ss.audience_bars(restated(7, 33, "tiny", "down", ss.WIDE_S))
    ss.check_bar_paths(bars, ss.WIDE_S)
    assert sum(ss.floor_acc(b, ss.WIDE_S) == -np.inf for b in bars) >= 7


def test_the_six_step_search_never_gives_up_with_three_slots():
    """The arithmetic of staged_serving.check_bar_paths, on bars all over the range."""
    rng = np.random.default_rng(5)
    bars = np.concatenate([rng.integers(1, 1 << 40, 2000) * ss.UNIT, 2.0 ** rng.uniform(-1074, 1000, 4000),
                           -(2.0 ** rng.uniform(-1074, 1000, 1000)), [0.0, ss.UNIT, 2.0 ** -1022, 1e308, -5e307, -1e308]])
    for bar in bars.tolist():
        assert ss.floor_acc(bar, ss.S) > -np.inf, bar
        assert ss.same_quotient(bar) <= 3
    assert ss.floor_acc(1e-310, 8) > -np.inf                  # (eight slots: nine accumulators, found in five steps)
    assert ss.floor_acc(1e-310, ss.WIDE_S) == -np.inf


# ---- the mutations the GPU file must catch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,w", [("rowborder", ss.W), ("tiny", ss.W_UP)], ids=["rowborder", "tiny"])
@SHAPES
def test_without_the_clamp_the_contributions_leave_the_bound(k, l, family, w):
    """`fmax(dot, kEps)` replaced by `dot` in exp_row_kernel, evaluated in long double on the committed case: part 1
    of the GPU file compares every contribution with the clamped restatement, so it fails on both families."""
    c = ss.case(k, l, family)
    users, offsets, items = ss.explain_request(c)
    good, bad = ss.LongExplain(c.data, c.params, w), ss.LongExplain(c.data, c.params, w, clamp=False)
    outside = total = 0
    for u, t in ss.pairs_of(users, offsets, items):
        a, b = good.pair(u, t)["a"], bad.pair(u, t)["a"]
        big = a > ELEMENT_FLOOR
        with np.errstate(invalid="ignore"):
            outside += int((~(np.abs(b[big] - a[big]) <= ss.contribution_bound(k, l) * a[big])).sum())
        total += int(big.sum())
    print(f"K={k} L={l} {family}: {outside} of {total} contributions outside the bound without the clamp")
    assert total > 100 and outside >= (total if family == "tiny" else total // 20)


@pytest.mark.parametrize("family", ss.FAMILIES)
def test_a_strict_comparison_in_aud_decide_drops_the_pair_at_the_bar(family):
    """`acc >= lo` replaced by `acc > lo`.  A device score is the quotient acc / 3 of an accumulator; a bar that is
    such a score has lo <= acc, and lo == acc where acc is the only accumulator with that quotient: the pair at the
    bar is then dropped and part 2's audience (offsets, users, scores) differs.  About half of all accumulators are
    alone with their quotient (those whose significand is below 1.5), and every case sets three bars that are scores
    (the smallest positive one, the median, the maximum) for each of 2 x 300 item rows' worth of pairs; here: the
    quotients next to the restatement's scores at those bars."""
    single = total = 0
    for k, l in ss.SHAPES:
        for s in (ss.audience_bars(restated(k, l, family))[i] for i in (0, 3, 4)):
            acc = np.float64(s) * ss.S
            bar = float(acc / ss.S)                              # a quotient, as the device's scores are
            lo = ss.floor_acc(bar, ss.S)
            assert np.float64(lo) / ss.S == bar and lo <= acc
            total += 1
            single += int(ss.same_quotient(bar) == 1 and lo == acc)
    assert total == 9 and single >= 2, single


# ---- the GPU file's check functions through the stand-ins ------------------------------------------------------------------------
@pytest.mark.parametrize("family,w", [("rowborder", ss.W), ("tiny", ss.W), ("tiny", ss.W_UP), ("dead", ss.W)],
                         ids=["rowborder", "tiny", "tiny_up", "dead"])
def test_check_explain_through_the_stand_in(family, w):
    c = ss.case(7, 33, family)
    worst = ss.check_explain(stand_in(c), c, w, ELEMENT_FLOOR, f"stand-in {family}")
    print(f"stand-in {family}: {worst}")
    assert (worst["above"] == 0) == (family == "tiny" and w is ss.W)      # plain tiny: the floor and the order only


@pytest.mark.parametrize("family", ["rowborder", "tiny"])
def test_check_identity_through_the_stand_in(family):
    c = ss.case(20, 20, family)
    w = ss.W_UP if family == "tiny" else ss.W
    print(f"stand-in {family}: identity, worst error / bound {ss.check_identity(stand_in(c), c, w, ELEMENT_FLOOR, family):.3f}")


@pytest.mark.parametrize("family,w", [("late", ss.W), ("tiny", ss.W_DOWN)], ids=["late", "tiny_down"])
def test_check_item_side_through_the_stand_in(family, w):
    c = ss.case(7, 33, family)
    dev, bars = ss.check_item_side(stand_in(c), c, w, f"stand-in {family}")
    assert (dev[list(c.zero_users)] == 0).all() and (dev[:, list(c.zero_items)] == 0).all()


@pytest.mark.parametrize("family", ["rowborder", "tiny"])
def test_check_catalogue_and_diverse_through_the_stand_in(family):
    c = ss.case(20, 20, family)
    em = stand_in(c)
    ss.check_catalogue(em, c, ss.W, f"stand-in {family}")
    ss.check_diverse(em, c, ss.W, f"stand-in {family}", pools=(10,))


@pytest.mark.parametrize("family", ss.OVERLAP_FAMILIES)
def test_check_overlap_through_the_stand_in(family):
    c = ss.overlap_case(family, ss.OVERLAP_SLAB + 1)
    em = stand_in(c)
    for side in ("users", "items"):
        frac = ss.check_overlap(em, c, side, ELEMENT_FLOOR, f"stand-in {family} {side}")
        assert frac <= 2.0 ** -10                                 # the restatement rounded to doubles: half an ulp
