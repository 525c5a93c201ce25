"""MMSBM.top_pairs_bulk() / score_bar() without a GPU: the restatement the device is compared against
(test_top_pairs_cpu.restate_top_pairs, unchanged, with m beyond 1,024, and the bar and counts read off the same
candidates), the conditions the GPU cases of test_gpu_top_pairs_bulk.py rely on, asserted on the restatement alone, the
host class through a CPU stand-in, and the agreement of the header, the ctypes table and the wrappers.

The tie-derived m of a case is chosen from the restatement, not by hand: among the groups of equal scores that lie wholly
beyond rank 1,024, the largest that spans three 128-user tiles (and two item tiles where the family allows), m in its
middle.  In the `constant` family every pair scores the same, so no group lies wholly beyond any rank: there m sits in
the middle of the one group, far beyond 1,024."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import exact_models as xm
import fake_device
from conftest import ROOT
from test_recommend_cpu import fitted, restate_scores, seen_items, string_frame
from test_top_pairs_cpu import TILE, TopPairsFakeHipEM, candidate_mask, global_order, restate_top_pairs, tiles_of

BOUND = 1 << 26
ITEM_TILE_FAMILIES = ("interleaved", "constant", "rare")     # tie groups that cross item tiles by construction
_ORDERS = {}


# ---- the restatement ------------------------------------------------------------------------------------------------
def restate_info(scores, users, seen, m):
    """{"bar", "above", "ties", "candidates"} of the request: the score of pair min(m, candidates) of the order (+0.0
    for a zero of either sign, -inf without candidates) and the candidates strictly above / exactly at it."""
    s = scores[candidate_mask(users, scores.shape[1], seen)]
    count = min(m, len(s))
    if count == 0:
        return {"bar": -np.inf, "above": 0, "ties": 0, "candidates": 0}
    bar = float(np.partition(s, len(s) - count)[len(s) - count]) + 0.0
    return {"bar": bar, "above": int((s > bar).sum()), "ties": int((s == bar).sum()), "candidates": int(len(s))}


def case_order(family, kind, shape, exclude):
    """(case, (users, items, scores) of every candidate in the query's order), computed once per case."""
    key = (family, kind, shape, exclude)
    if key not in _ORDERS:
        case = xm.make_case(family, kind, shape)
        _ORDERS[key] = (case, global_order(case["scores"], case["users"], case["seen"] if exclude else None))
    return _ORDERS[key]


def tie_m(family, kind, shape, exclude):
    """(m, users, items of the tie group m lies strictly inside), or (None, ...) when no score repeats beyond rank
    1,024.  See the module's text."""
    _, (u, i, s) = case_order(family, kind, shape, exclude)
    starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    sizes = np.diff(np.concatenate([starts, [len(s)]]))
    if family == "constant":
        assert len(starts) == 1
        ok = np.array([0])
    else:
        ok = np.flatnonzero((starts >= 1024) & (sizes >= 2))
    best = None
    for j in ok[np.argsort(-sizes[ok], kind="stable")][:64]:
        a, n = int(starts[j]), int(sizes[j])
        good = tiles_of(u[a:a + n]) >= 3 and (family not in ITEM_TILE_FAMILIES or tiles_of(i[a:a + n]) >= 2)
        if best is None or good:
            best = (a, n)
        if good:
            break
    if best is None:
        return None, u[:0], i[:0]
    a, n = best
    m = a + max(1, n // 2)                                   # 1-based rank: pairs m and m + 1 are both inside
    assert a < m and m + 1 <= a + n and m > 1024
    return m, u[a:a + n], i[a:a + n]


def bulk_ms(family, kind, shape, exclude):
    """The m of a GPU case: 1,025; 4,096; the tie-derived m; candidates - 1; candidates; candidates + 7."""
    _, (u, _, _) = case_order(family, kind, shape, exclude)
    m = tie_m(family, kind, shape, exclude)[0]
    return [1025, 4096] + ([m] if m is not None else []) + [len(u) - 1, len(u), len(u) + 7]


def test_the_info_is_read_off_the_order():
    rng = np.random.default_rng(1)
    scores = rng.integers(-3, 4, (9, 31)).astype(np.float64)
    scores[scores == 0] = -0.0                              # zeros of the other sign: one tie group all the same
    scores[2, :5] = 0.0
    users = np.array([4, 0, 7, 1, 2, 8, 3, 6, 5])
    seen = [set(rng.choice(31, 6, replace=False).tolist()) for _ in range(9)]
    for sn in (None, seen):
        u, i, s = global_order(scores, users, sn)
        for m in (1, 2, 17, 100, len(s) - 1, len(s), len(s) + 5):
            info = restate_info(scores, users, sn, m)
            got = restate_top_pairs(None, None, users, m, sn, scores=scores)
            last = got[2][got[3] - 1]
            assert info["candidates"] == len(s) and got[3] == min(m, len(s))
            assert info["bar"] == last and (last != 0 or not np.signbit(info["bar"]))
            assert info["above"] == int((s > last).sum()) and info["ties"] == int((s == last).sum())
            assert info["above"] < got[3] <= info["above"] + info["ties"]
    assert restate_info(scores[:0], users[:0], None, 5) == {"bar": -np.inf, "above": 0, "ties": 0, "candidates": 0}


# ---- the conditions the GPU cases rely on -------------------------------------------------------------------------------
TIE_CASES = [(f, k, s, e) for f in xm.TIE_FAMILIES for k in xm.WEIGHT_KINDS for s in xm.MANY for e in (False, True)]


@pytest.mark.parametrize("family,kind,shape,exclude", TIE_CASES,
                         ids=["{}-{}-U{}I{}-{}".format(f, k, s[0], s[1], "unseen_pairs" if e else "all_pairs") for f, k, s, e in TIE_CASES])
def test_the_tie_derived_m_sits_inside_a_group_that_crosses_tiles(family, kind, shape, exclude):
    m, gu, gi = tie_m(family, kind, shape, exclude)
    _, (u, i, s) = case_order(family, kind, shape, exclude)
    assert m is not None and 1024 < m < len(s)
    assert s[m - 1] == s[m], (family, kind, shape, exclude, m)              # pairs m and m + 1 tie
    assert tiles_of(gu) >= 3, (family, kind, shape, exclude, m, len(gu))    # three 128-user tiles
    if family in ITEM_TILE_FAMILIES:
        assert tiles_of(gi) >= 2, (family, kind, shape, exclude, m, len(gi))
    if family != "constant":
        first = int(np.flatnonzero(s == s[m - 1])[0])
        assert first >= 1024                                                  # the group lies wholly beyond rank 1,024
    info = restate_info(xm.make_case(family, kind, shape)["scores"], np.arange(shape[0]),
                        case_order(family, kind, shape, exclude)[0]["seen"] if exclude else None, m)
    assert info["above"] < m < info["above"] + info["ties"] and info["ties"] == len(gu)   # the cut is inside the ties


@pytest.mark.parametrize("shape", xm.MANY, ids=lambda s: "U{}I{}".format(s[0], s[1]))
def test_every_case_has_its_six_m_and_partial_tiles(shape):
    U, I = shape[:2]
    assert U % TILE and I % TILE and -(-U // TILE) == 3 and U * I in (299_100, 265_460)
    for family, kind in xm.VARIANTS:
        for exclude in (False, True):
            ms = bulk_ms(family, kind, shape, exclude)
            n = len(case_order(family, kind, shape, exclude)[1][0])
            assert ms[:2] == [1025, 4096] and ms[-3:] == [n - 1, n, n + 7] and n > 4096
            assert len(ms) == 6, (family, kind, exclude)     # every family repeats a score beyond rank 1,024
            assert all(1 <= m <= BOUND for m in ms)
            if exclude:
                assert n < U * I                             # seen pairs exist: the histogram of seen pairs matters


def test_signed_weights_give_both_signs_and_exact_zeros():
    signs = set()
    for shape in xm.MANY:
        mixed = xm.make_case("mixed", "signed", shape)["scores"]
        assert (mixed < 0).any() and (mixed > 0).any() and (mixed == 0).any(), shape
        const = xm.make_case("constant", "signed", shape)["scores"]
        assert len(np.unique(const)) == 1                    # one level per case: the sign is the case's
        signs.add(float(np.sign(const[0, 0])))
    assert signs == {-1.0, 1.0}                              # ... and the two shapes have one each
    # families whose signed cases hold exact zeros inside the order: the key's zero is one bin for both signs
    assert (xm.make_case("sorted", "signed", xm.MANY[0])["scores"] == 0).any()
    assert (xm.make_case("rare", "signed", xm.MANY[0])["scores"] == 0).any()


def test_the_meeting_point_and_the_large_shape():
    """m in {1, 10, 300, 1,024} is inside top_pairs' bound; 120,000 x 20,000 passes 2^31 pairs, and a constant model
    there puts all of them into one bin, beyond what 32 bits count."""
    from test_top_pairs_cpu import MS
    assert MS == (1, 10, 300, 1024) and max(MS) == TopPairsFakeHipEM.MAX_TOP_PAIRS
    assert 120_000 * 20_000 > 2 ** 31 and 120_000 * 20_000 - 400_000 > 2 ** 31


# ---- the CPU stand-in ---------------------------------------------------------------------------------------------------
class BulkFakeHipEM(TopPairsFakeHipEM):
    """TopPairsFakeHipEM with the bulk query and the bar, answered by the restatement."""
    MAX_TOP_PAIRS_BULK = BOUND

    def _bulk(self, m, users):
        assert self._rc["params"], "recommend_top_pairs_bulk before recommend_add"
        assert 1 <= m <= self.MAX_TOP_PAIRS_BULK
        ids = np.arange(self.n_users) if users is None else np.asarray(users, dtype=np.int64)
        if len(ids) == 0:
            return ids, np.zeros((0, self.n_items))
        return ids, restate_scores(self._rc["params"], ids, self.n_items, self._rc["w"])

    def recommend_top_pairs_bulk(self, m, users=None):
        ids, scores = self._bulk(m, users)
        fake_device.LOG.append(("recommend_top_pairs_bulk", None if users is None else len(users)))
        return (*restate_top_pairs(None, None, ids, m, self._rc["seen"], scores=scores),
                restate_info(scores, ids, self._rc["seen"], m))

    def recommend_pair_bar(self, m, users=None):
        ids, scores = self._bulk(m, users)
        fake_device.LOG.append(("recommend_pair_bar", None if users is None else len(users)))
        return restate_info(scores, ids, self._rc["seen"], m)


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", BulkFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(BulkFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def expected(model, users, m, exclude_seen=True, weights=None):
    """(frame, info) of the restatement in the host class's format, for encoded user ids (None: all)."""
    enc = model.data_handler
    params = [(r["theta"], r["eta"], r["pr"]) for r in model.results]
    w = np.asarray(model.ratings if weights is None else weights, dtype=np.float64)
    seen = seen_items(model.train, model.p + 1) if exclude_seen else None
    ids = np.arange(model.p + 1) if users is None else np.asarray(users, dtype=np.int64)
    scores = restate_scores(params, ids, model.m + 1, w) if len(ids) else np.zeros((0, model.m + 1))
    u, i, s, count = restate_top_pairs(None, None, ids, m, seen, scores=scores)
    ul, il = enc.user_labels(), enc.item_labels()
    rows = [(ul[u[k]], il[i[k]], s[k], k + 1) for k in range(count)]
    return pd.DataFrame(rows, columns=["users", "items", "score", "rank"]), restate_info(scores, ids, seen, m)


def same(got, want):
    assert list(got.columns) == ["users", "items", "score", "rank"]
    for col in ("users", "items", "rank"):
        assert got[col].tolist() == want[col].tolist(), col
    assert np.array_equal(xm.bits(got["score"].to_numpy(dtype=np.float64)), xm.bits(want["score"].to_numpy(dtype=np.float64)))


def same_info(got, want):
    assert set(got) == {"bar", "above", "ties", "candidates"}
    assert np.array_equal(xm.bits(got["bar"]), xm.bits(want["bar"]))
    for k in ("above", "ties", "candidates"):
        assert got[k] == want[k] and isinstance(got[k], int), k


def test_labels_the_info_and_none_means_every_user(host):
    df = string_frame()
    m = fitted(host, df)
    m.predict(df.iloc[:40])
    before = m.score(silent=True)["stats"]
    got = m.top_pairs_bulk(m=130)
    want, info = expected(m, None, 130)
    same(got, want)
    same_info(m.pairs_bulk_, info)
    assert len(got) == 130 and got["rank"].tolist() == list(range(1, 131)) and got["rank"].dtype == np.int64
    assert not set(zip(df["users"], df["items"])) & set(zip(got["users"], got["items"]))   # no training pair
    assert m.score(silent=True)["stats"] == before
    assert ("recommend_top_pairs_bulk", None) in fake_device.LOG
    events = [e for e, _ in fake_device.LOG if e.startswith("recommend")]
    assert events[0] == "recommend_begin" and events[-1] == "recommend_end"
    same(m.top_pairs(m=130), got)                                            # the two methods meet below 1,024


def test_request_order_subsets_exclusion_and_weights(host):
    m = fitted(host, string_frame())
    labels = m.data_handler.user_labels()
    ask = [labels[7], labels[1], labels[4]]
    got = m.top_pairs_bulk(25, users=ask)
    same(got, expected(m, [7, 1, 4], 25)[0])
    same(m.top_pairs_bulk(25, users=ask[::-1]), got)
    assert set(got["users"]) <= set(ask)
    same(m.top_pairs_bulk(40, exclude_seen=False), expected(m, None, 40, exclude_seen=False)[0])
    w = [0, 0, 0, 0, 1]
    same(m.top_pairs_bulk(40, weights=w), expected(m, None, 40, weights=w)[0])
    same_info(m.pairs_bulk_, expected(m, None, 40, weights=w)[1])


def test_the_frame_is_built_in_batches(host, monkeypatch):
    m = fitted(host, string_frame())
    whole = m.top_pairs_bulk(100)
    for rows in (1, 7, 99, 100, 101):
        monkeypatch.setattr(host.MMSBM, "RECOMMEND_BATCH_ROWS", rows)
        got = m.top_pairs_bulk(100)
        same(got, whole)
        assert got.index.tolist() == list(range(100))


def test_more_than_the_candidates_and_an_empty_request(host):
    m = fitted(host, string_frame())
    want, info = expected(m, None, 10 ** 6)
    got = m.top_pairs_bulk(10 ** 6)
    same(got, want)
    assert len(got) == info["candidates"] == m.pairs_bulk_["candidates"] and info["candidates"] < 10 ** 6
    assert m.pairs_bulk_["above"] + m.pairs_bulk_["ties"] == info["candidates"]          # the bar is the lowest score
    none = m.top_pairs_bulk(5, users=[])
    assert len(none) == 0 and list(none.columns) == ["users", "items", "score", "rank"]
    assert m.pairs_bulk_ == {"bar": -np.inf, "above": 0, "ties": 0, "candidates": 0}
    assert m.score_bar(5, users=[])["candidates"] == 0


def test_score_bar_is_the_bulk_querys_info(host):
    m = fitted(host, string_frame())
    labels = m.data_handler.user_labels()
    for users, ids in ((None, None), ([labels[3], labels[0]], [3, 0])):
        for k in (1, 17, 60, 10 ** 5):
            bar = m.score_bar(k, users=users)
            m.top_pairs_bulk(k, users=users)
            same_info(bar, m.pairs_bulk_)
            same_info(bar, expected(m, ids, k)[1])
    assert "audience(min_score=bar)" in host.MMSBM.score_bar.__doc__ and "above + ties" in host.MMSBM.score_bar.__doc__
    events = [e for e, _ in fake_device.LOG if e.startswith("recommend")]
    assert "recommend_pair_bar" in events and events[-1] == "recommend_end"


def test_refusals_come_before_any_device_call(host):
    m = fitted(host, string_frame())
    labels = m.data_handler.user_labels()
    fake_device.LOG.clear()
    for method in (m.top_pairs_bulk, m.score_bar):
        for bad in (0, -3, 2.5, True, None, "7"):
            with pytest.raises(ValueError, match="positive integer"):
                method(bad)
        with pytest.raises(ValueError, match=f"beyond the {BOUND}"):
            method(BOUND + 1)
        with pytest.raises(ValueError, match="more than once"):
            method(5, users=[labels[3], labels[0], labels[3]])
        with pytest.raises(KeyError, match="nobody"):
            method(5, users=[labels[0], "nobody"])
        with pytest.raises(ValueError, match="weights"):
            method(5, weights=[1.0, 2.0])
    assert not fake_device.LOG
    with pytest.raises(ValueError, match="beyond the 1024"):                 # top_pairs keeps its own bound
        m.top_pairs(m=1025)
    m._restart_ids = m._restart_ids[:1]
    m.results = m.results[:1]
    with pytest.raises(RuntimeError, match="1 of its 2 restarts"):
        m.top_pairs_bulk(5)


# ---- one bound, two symbols, every layer --------------------------------------------------------------------------------
def test_the_header_the_ctypes_table_and_the_wrappers_agree():
    import ctypes as C

    import mmsbm_amd.mmsbm as host
    from mmsbm_amd import _lib
    from mmsbm_amd.core import HipEM
    with open(os.path.join(ROOT, "include", "mmsbm_hip.h")) as fh:
        text = fh.read()
    bound = int(re.search(r"#define MMSBM_HIP_TOP_PAIRS_BULK_MAX_M (\d+)", text).group(1))
    assert bound == BOUND == HipEM.MAX_TOP_PAIRS_BULK == host.MMSBM.TOP_PAIRS_BULK_MAX
    assert int(re.search(r"#define MMSBM_HIP_TOP_PAIRS_MAX_M (\d+)", text).group(1)) == HipEM.MAX_TOP_PAIRS == 1024
    with open(os.path.join(ROOT, "mmsbm_amd", "csrc", "pairs_bulk_plan.hpp")) as fh:
        assert re.search(r"kPbMaxM = int64_t\(1\) << 26;", fh.read())
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("mmsbm_hip_recommend_top_pairs_bulk", 10), ("mmsbm_hip_recommend_pair_bar", 6)):
        decl = re.search(name + r"\s*\(([^)]*)\)", plain)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args and args[3] is C.c_int64, name   # m is 64 bits wide
    assert _lib.SIGNATURES["mmsbm_hip_recommend_top_pairs_bulk"][1][7] is _lib.c_i64p   # count, then bar and counts[3]
    for method in ("recommend_top_pairs_bulk", "recommend_pair_bar"):
        assert callable(getattr(HipEM, method))
    for method in ("top_pairs_bulk", "score_bar"):
        assert callable(getattr(host.MMSBM, method))
