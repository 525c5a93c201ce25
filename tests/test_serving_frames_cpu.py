"""What every public serving method of MMSBM hands back, pinned before the host class was split: the column names and
dtypes of a result with rows and of one without, the keys and value types of the dict-returning methods, and the exact
text of the refusals -- with string labels through fit() ("labels") and integer ids through fit_encoded() ("ids").
CPU only: the device is every feature's stand-in in one class."""
import numpy as np
import pandas as pd
import pytest

import fake_device
from test_align_cpu import OverlapFakeHipEM
from test_audience_cpu import AudienceFakeHipEM
from test_diverse_cpu import DiverseFakeHipEM
from test_explain_cpu import ExplainFakeHipEM
from test_heldout_cpu import HeldoutFakeHipEM
from test_ranking_cpu import RankingFakeHipEM
from test_recommend_cpu import string_frame
from test_top_pairs_cpu import TopPairsFakeHipEM

MODES = ("labels", "ids")


class EveryFakeHipEM(ExplainFakeHipEM, AudienceFakeHipEM, DiverseFakeHipEM, OverlapFakeHipEM, RankingFakeHipEM,
                     TopPairsFakeHipEM, HeldoutFakeHipEM):
    """Every stand-in the serving methods have, in one class."""


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", EveryFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(EveryFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    monkeypatch.setattr(HeldoutFakeHipEM, "SCRIPT", None)
    fake_device.LOG.clear()
    return host


class Case:
    """A fitted model of one mode and requests in that mode's vocabulary."""

    def __init__(self, host, mode):
        df = string_frame()
        self.model = host.MMSBM(2, 3, iterations=3, sampling=2, seed=7)
        enc = host.Encoder()
        train = np.ascontiguousarray(enc.fit_transform(df))
        if mode == "labels":
            self.model.fit(df, silent=True)
            name = (enc.user_labels(), enc.item_labels(), enc.rating_labels())
            self.new_users, self.new_items, self.nobody = ["new-a", "new-b", "new-a"], ["film-a", "film-b", "film-a"], "nobody"
        else:
            self.model.fit_encoded(train)
            name = tuple(list(range(int(train[:, j].max()) + 1)) for j in range(3))
            self.new_users, self.new_items, self.nobody = [100, 101, 100], [50, 51, 50], 999
        self.users = [name[0][3], name[0][1]]
        self.items = [name[1][4], name[1][7], name[1][2]]
        self.pairs = [(name[0][3], name[1][4]), (name[0][3], name[1][7]), (name[0][1], name[1][2])]
        self.held = self.frame([name[0][u] for u in train[:6, 0]], [name[1][i] for i in train[6:12, 1]],
                               [name[2][r] for r in train[:6, 2]])
        self.dropped = self.frame([self.nobody] * 2, self.items[:2], [name[2][0]] * 2)
        self.user_data = self.frame(self.new_users, self.items, [name[2][0], name[2][1], name[2][2]])
        self.item_data = self.frame([name[0][0], name[0][1], name[0][2]], self.new_items, [name[2][0], name[2][1], name[2][2]])
        self.user_data_dropped = self.frame(self.new_users, [self.nobody] * 3, [name[2][0]] * 3)

    @staticmethod
    def frame(users, items, ratings):
        return pd.DataFrame({"users": users, "items": items, "ratings": ratings})


def shape_of(df):
    """Column names and dtypes; for a frame with a named index, that too."""
    out = [(str(c), str(t)) for c, t in df.dtypes.items()]
    return ([("index:" + str(df.index.name), str(df.index.dtype))] if df.index.name else []) + out


FRAMES = {
    "recommend_all": lambda c: c.model.recommend(n=3),
    "recommend": lambda c: c.model.recommend(users=c.users, n=3),
    "recommend_within": lambda c: c.model.recommend(users=c.users, n=3, candidates=c.items, exclude=c.pairs[:1]),
    "rerank": lambda c: c.model.rerank(c.pairs, exclude_seen=False),
    "recommend_users_all": lambda c: c.model.recommend_users(n=3),
    "recommend_users": lambda c: c.model.recommend_users(items=c.items, n=3),
    "audience": lambda c: c.model.audience(items=c.items, min_score=0.0),
    "audience_all": lambda c: c.model.audience(min_score=0.0),
    "audience_count": lambda c: c.model.audience(items=c.items, min_score=0.0, count_only=True),
    "audience_count_all": lambda c: c.model.audience(min_score=0.0, count_only=True),
    "top_pairs": lambda c: c.model.top_pairs(m=5),
    "top_pairs_users": lambda c: c.model.top_pairs(m=5, users=c.users),
    "explain": lambda c: c.model.explain(c.pairs, n=2),
    "similar_items": lambda c: c.model.similar_items(c.items, n=2),
    "similar_items_all": lambda c: c.model.similar_items(n=2),
    "similar_users": lambda c: c.model.similar_users(c.users, n=2),
    "recommend_diverse": lambda c: c.model.recommend_diverse(users=c.users, n=3, diversity=0.5),
    "recommend_diverse_within": lambda c: c.model.recommend_diverse(n=2, diversity=0.5, pool=3, candidates=c.items,
                                                                    exclude=c.pairs[:1]),
    "distances": lambda c: c.model.distances([(c.items[0], c.items[1]), (c.items[2], c.items[2])]),
    "distances_users": lambda c: c.model.distances([(c.users[0], c.users[1])], side="users"),
    "list_diversity": lambda c: c.model.list_diversity(c.model.recommend(users=c.users, n=3, exclude_seen=False)),
    "heldout_positions": lambda c: c.model.heldout_positions(c.held, exclude_seen=False),
    "fold_in": lambda c: c.model.fold_in(c.user_data, iterations=2)[0],
    "fold_in_iterations": lambda c: (c.model.fold_in(c.user_data, iterations=2), c.model.fold_in_iterations)[1],
    "recommend_new": lambda c: c.model.recommend_new(c.user_data, n=3, iterations=2),
    "fold_in_items": lambda c: c.model.fold_in_items(c.item_data, iterations=2)[0],
    "fold_in_items_iterations": lambda c: (c.model.fold_in_items(c.item_data, iterations=2),
                                           c.model.fold_in_items_iterations)[1],
    "recommend_with_new_items": lambda c: c.model.recommend_with_new_items(c.item_data, users=c.users, n=3, iterations=2),
    "recommend_users_new_items": lambda c: c.model.recommend_users_new_items(c.item_data, n=3, iterations=2),
    # ---- without rows
    "empty recommend": lambda c: c.model.recommend(users=[], n=3),
    "empty recommend_candidates": lambda c: c.model.recommend(users=c.users, n=3, candidates=[]),
    "empty rerank": lambda c: c.model.rerank([]),
    "empty recommend_users": lambda c: c.model.recommend_users(items=[], n=3),
    "empty audience": lambda c: c.model.audience(items=[], min_score=0.0),
    "empty audience_bar": lambda c: c.model.audience(items=c.items, min_score=1e9),
    "empty audience_count": lambda c: c.model.audience(items=[], min_score=0.0, count_only=True),
    "empty explain": lambda c: c.model.explain([], n=2),
    "empty similar_items": lambda c: c.model.similar_items([], n=2),
    "empty similar_users": lambda c: c.model.similar_users([], n=2),
    "empty recommend_diverse": lambda c: c.model.recommend_diverse(users=[], n=3, diversity=0.5),
    "empty recommend_diverse_candidates": lambda c: c.model.recommend_diverse(users=c.users, n=3, diversity=0.5, candidates=[]),
    "empty distances": lambda c: c.model.distances([]),
    "empty list_diversity": lambda c: c.model.list_diversity([]),
    "empty heldout_positions": lambda c: c.model.heldout_positions(c.dropped),
    "empty fold_in": lambda c: c.model.fold_in(c.user_data.iloc[:0], iterations=2)[0],
    "dropped fold_in": lambda c: c.model.fold_in(c.user_data_dropped, iterations=2)[0],
}

EMPTY = str(pd.DataFrame({"a": []})["a"].dtype)        # a column made from an empty list
TOP = ["score:float64", "rank:int64"]
EXPLAIN = ["contribution:float64", "share:float64", "rank:int64", "score:float64", "explained:float64"]


def cols(*specs):
    return [tuple(s.rsplit(":", 1)) for group in specs for s in ([group] if isinstance(group, str) else group)]


# what the parent commit returns: (labels mode, ids mode); one entry where the two agree
EXPECTED = {
    "recommend_all": (cols("users:object", "items:object", TOP), cols("users:int32", "items:int64", TOP)),
    "recommend": (cols("users:object", "items:object", TOP), cols("users:object", "items:int64", TOP)),
    "recommend_within": (cols("users:object", "items:object", TOP), cols("users:object", "items:int64", TOP)),
    "rerank": (cols("users:object", "items:object", TOP), cols("users:int32", "items:int64", TOP)),
    "recommend_users_all": (cols("items:object", "users:object", TOP), cols("items:int32", "users:int64", TOP)),
    "recommend_users": (cols("items:object", "users:object", TOP), cols("items:object", "users:int64", TOP)),
    "audience": (cols("items:object", "users:object", TOP), cols("items:object", "users:int64", TOP)),
    "audience_all": (cols("items:object", "users:object", TOP), cols("items:int32", "users:int64", TOP)),
    "audience_count": (cols("items:object", "count:int64"),),
    "audience_count_all": (cols("items:object", "count:int64"), cols("items:int32", "count:int64")),
    "top_pairs": (cols("users:object", "items:object", TOP), cols("users:int64", "items:int64", TOP)),
    "top_pairs_users": (cols("users:object", "items:object", TOP), cols("users:int64", "items:int64", TOP)),
    "explain": (cols("users:object", "items:object", "because:object", "rating:object", EXPLAIN),
                cols("users:object", "items:object", "because:int64", "rating:int64", EXPLAIN)),
    "similar_items": (cols("items:object", "similar:object", "distance:float64", "rank:int64"),
                      cols("items:object", "similar:int64", "distance:float64", "rank:int64")),
    "similar_items_all": (cols("items:object", "similar:object", "distance:float64", "rank:int64"),
                          cols("items:int32", "similar:int64", "distance:float64", "rank:int64")),
    "similar_users": (cols("users:object", "similar:object", "distance:float64", "rank:int64"),
                      cols("users:object", "similar:int64", "distance:float64", "rank:int64")),
    "recommend_diverse": (cols("users:object", "items:object", "score:float64", "distance:float64", "rank:int64"),
                          cols("users:object", "items:int64", "score:float64", "distance:float64", "rank:int64")),
    "recommend_diverse_within": (cols("users:object", "items:object", "score:float64", "distance:float64", "rank:int64"),
                                 cols("users:int32", "items:int64", "score:float64", "distance:float64", "rank:int64")),
    "distances": (cols("a:object", "b:object", "distance:float64"),),
    "distances_users": (cols("a:object", "b:object", "distance:float64"),),
    "list_diversity": (cols("users:object", "n:int64", "diversity:float64"),),
    "heldout_positions": (cols("users:object", "items:object", "ratings:object", "position:int64", "candidates:int64"),
                          cols("users:int64", "items:int64", "ratings:int64", "position:int64", "candidates:int64")),
    "fold_in": (cols("index:users:object", "0:float64", "1:float64"), cols("index:users:int64", "0:float64", "1:float64")),
    "fold_in_iterations": (cols("index:users:object", "0:int32", "1:int32"), cols("index:users:int64", "0:int32", "1:int32")),
    "recommend_new": (cols("users:object", "items:object", TOP), cols("users:int64", "items:int64", TOP)),
    "fold_in_items": (cols("index:items:object", "0:float64", "1:float64", "2:float64"),
                      cols("index:items:int64", "0:float64", "1:float64", "2:float64")),
    "fold_in_items_iterations": (cols("index:items:object", "0:int32", "1:int32"), cols("index:items:int64", "0:int32", "1:int32")),
    "recommend_with_new_items": (cols("users:object", "items:object", TOP), cols("users:object", "items:int64", TOP)),
    "recommend_users_new_items": (cols("items:object", "users:object", TOP), cols("items:int64", "users:int64", TOP)),
    "empty recommend": (cols("users:" + EMPTY, "items:" + EMPTY, TOP),),
    "empty recommend_candidates": (cols("users:" + EMPTY, "items:" + EMPTY, TOP),),
    "empty rerank": (cols("users:" + EMPTY, "items:" + EMPTY, TOP),),
    "empty recommend_users": (cols("items:" + EMPTY, "users:" + EMPTY, TOP),),
    "empty audience": (cols("items:" + EMPTY, "users:" + EMPTY, TOP),),
    "empty audience_bar": (cols("items:object", "users:object", TOP), cols("items:object", "users:int64", TOP)),
    "empty audience_count": (cols("items:object", "count:int64"),),
    "empty explain": (cols("users:" + EMPTY, "items:" + EMPTY, "because:" + EMPTY, "rating:" + EMPTY, EXPLAIN),),
    "empty similar_items": (cols("items:" + EMPTY, "similar:" + EMPTY, "distance:float64", "rank:int64"),),
    "empty similar_users": (cols("users:" + EMPTY, "similar:" + EMPTY, "distance:float64", "rank:int64"),),
    "empty recommend_diverse": (cols("users:" + EMPTY, "items:" + EMPTY, "score:float64", "distance:float64", "rank:int64"),),
    "empty recommend_diverse_candidates": (cols("users:" + EMPTY, "items:" + EMPTY, "score:float64", "distance:float64", "rank:int64"),),
    "empty distances": (cols("a:" + EMPTY, "b:" + EMPTY, "distance:float64"),),
    "empty list_diversity": (cols("users:" + EMPTY, "n:int64", "diversity:float64"),),
    "empty heldout_positions": (cols("users:object", "items:object", "ratings:object", "position:int64", "candidates:int64"),
                                cols("users:int64", "items:int64", "ratings:int64", "position:int64", "candidates:int64")),
    "empty fold_in": (cols("index:users:object", "0:float64", "1:float64"),),
    "dropped fold_in": (cols("index:users:object", "0:float64", "1:float64"), cols("index:users:int64", "0:float64", "1:float64")),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_columns_and_dtypes(host, name, mode):
    got = FRAMES[name](Case(host, mode))
    assert isinstance(got, pd.DataFrame)
    assert (len(got) == 0) == name.startswith("empty"), len(got)
    assert shape_of(got) == EXPECTED[name][MODES.index(mode) % len(EXPECTED[name])], shape_of(got)


# ---- the dict-returning methods -----------------------------------------------------------------------------------------
def kinds(d):
    return {k: type(v).__name__ for k, v in d.items()}


ALIGNMENT = {"reference": "int", **{f"{s}_{what}": "ndarray" for s in ("user", "item")
                                    for what in ("groups", "similarity", "agreement")}}


@pytest.mark.parametrize("mode", MODES)
def test_align_restarts_and_consensus(host, mode):
    c = Case(host, mode)
    got = c.model.align_restarts()
    assert kinds(got) == ALIGNMENT and list(got) == list(ALIGNMENT)
    assert kinds(c.model.align_restarts(reference=1)) == ALIGNMENT
    con = c.model.consensus()
    assert kinds(con) == {"theta": "DataFrame", "eta": "DataFrame", "pr": "dict", "alignment": "dict"}
    assert kinds(con["alignment"]) == ALIGNMENT
    labelled = mode == "labels"
    assert str(con["theta"].index.dtype) == str(con["eta"].index.dtype) == ("object" if labelled else "int64")
    assert con["theta"].shape == (c.model.p + 1, 2) and con["eta"].shape == (c.model.m + 1, 3)
    keys = list(con["pr"])
    assert keys == (c.model.data_handler.rating_labels() if labelled else list(range(len(c.model.ratings))))
    assert {type(k) for k in keys} == {str if labelled else int}
    assert all(isinstance(v, pd.DataFrame) and v.shape == (2, 3) for v in con["pr"].values())
    # predict() stores the same shapes through the same labels
    c.model.data_handler and c.model.predict(c.held)
    if labelled:
        assert list(c.model.pr) == keys and c.model.theta.index.tolist() == con["theta"].index.tolist()
        assert {type(k) for k in c.model.pr} == {str}


@pytest.mark.parametrize("mode", MODES)
def test_log_likelihood_and_ranking_score(host, mode):
    c = Case(host, mode)
    ll = {"rows": "int", "log_likelihood": "float", "per_restart": "list", "perplexity": "float"}
    got = c.model.log_likelihood(c.held)
    assert kinds(got) == ll and list(got) == list(ll) and got["rows"] == 6
    assert [type(v) for v in got["per_restart"]] == [float, float]
    none = c.model.log_likelihood(c.dropped)
    assert kinds(none) == ll and none["rows"] == 0 and np.isnan(none["perplexity"])
    rank = ["users", "skipped_users", "pairs", "not_candidates", "mrr", "auc"]
    at = lambda k: [f"{m}@{k}" for m in ("precision", "recall", "ndcg", "hit_rate")]   # noqa: E731
    got = c.model.ranking_score(c.held, k=[2, 5, 2], exclude_seen=False)
    assert list(got) == rank + at(2) + at(5)
    assert kinds(got) == {**{k: "int" for k in rank[:4]}, **{k: "float" for k in rank[4:] + at(2) + at(5)}}
    rel = [c.held["ratings"].iloc[0]]
    assert list(c.model.ranking_score(c.held, k=3, relevant=rel, exclude_seen=False)) == rank + at(3)
    none = c.model.ranking_score(c.dropped, k=3)
    assert list(none) == rank + at(3) and none["users"] == 0 and np.isnan(none["mrr"])


# ---- the refusals, word for word -----------------------------------------------------------------------------------------
REFUSALS = {
    "n": (ValueError, lambda c: c.model.recommend(n=0), "n must be a positive integer, got 0"),
    "n bool": (ValueError, lambda c: c.model.recommend_users(n=True), "n must be a positive integer, got True"),
    "n float": (ValueError, lambda c: c.model.explain(c.pairs, n=2.0), "n must be a positive integer, got 2.0"),
    "n rerank": (ValueError, lambda c: c.model.rerank(c.pairs, n=-1), "n must be a positive integer, got -1"),
    "n similar": (ValueError, lambda c: c.model.similar_items(n="3"), "n must be a positive integer, got '3'"),
    "m": (ValueError, lambda c: c.model.top_pairs(m=0), "m must be a positive integer, got 0"),
    "m numpy bool": (ValueError, lambda c: c.model.top_pairs(m=np.True_), f"m must be a positive integer, got {np.True_!r}"),
    "m large": (ValueError, lambda c: c.model.top_pairs(m=1025), "m = 1025 is beyond the 1024 pairs a query returns at most"),
    "pool": (ValueError, lambda c: c.model.recommend_diverse(n=2, diversity=1, pool=2.5),
             "pool must be a positive integer, got 2.5"),
    "pool range": (ValueError, lambda c: c.model.recommend_diverse(n=3, diversity=1, pool=2),
                   "pool must lie in [n, 1024], got pool=2 with n=3"),
    "iterations": (ValueError, lambda c: c.model.fold_in(c.user_data, iterations=-1),
                   "iterations must be a non-negative integer, got -1"),
    "iterations items": (ValueError, lambda c: c.model.fold_in_items(c.item_data, iterations=None),
                         "iterations must be a non-negative integer, got None"),
    "k": (ValueError, lambda c: c.model.ranking_score(c.held, k=0), "k must be a positive integer or a list of them, got 0"),
    "k list": (ValueError, lambda c: c.model.ranking_score(c.held, k=[3, True]),
               "k must be a positive integer or a list of them, got [3, True]"),
    "k empty": (ValueError, lambda c: c.model.ranking_score(c.held, k=[]), "k must be a positive integer or a list of them, got []"),
    "k text": (ValueError, lambda c: c.model.ranking_score(c.held, k="10"),
               "k must be a positive integer or a list of them, got '10'"),
    "k bool": (ValueError, lambda c: c.model.ranking_score(c.held, k=True),
               "k must be a positive integer or a list of them, got True"),
    "reference": (ValueError, lambda c: c.model.align_restarts(reference=1.0),
                  "reference must be a position in self.results (an int) or None, got 1.0"),
    "reference range": (ValueError, lambda c: c.model.consensus(reference=2),
                        "reference = 2 is not a position in self.results (0 .. 1)"),
    "reference negative": (ValueError, lambda c: c.model.align_restarts(reference=-1),
                           "reference = -1 is not a position in self.results (0 .. 1)"),
    "patience": (ValueError, lambda c: c.model.fit(c.held, validation=c.held, patience=0),
                 "patience must be a positive integer, got 0"),
    "min_score": (ValueError, lambda c: c.model.audience(), "min_score must be a finite number, got None"),
    "min_score inf": (ValueError, lambda c: c.model.audience(min_score=float("inf")), "min_score must be a finite number, got inf"),
    "min_score bool": (ValueError, lambda c: c.model.audience(min_score=True), "min_score must be a finite number, got True"),
    "diversity": (ValueError, lambda c: c.model.recommend_diverse(diversity=-0.5),
                  "diversity must be a finite number >= 0, got -0.5"),
    "diversity nan": (ValueError, lambda c: c.model.recommend_diverse(diversity=float("nan")),
                      "diversity must be a finite number >= 0, got nan"),
    "diversity missing": (TypeError, lambda c: c.model.recommend_diverse(),
                          "recommend_diverse() needs diversity=: score units per unit of distance (0: plain recommend)"),
    "tol": (ValueError, lambda c: c.model.fold_in(c.user_data, tol="x"), "tol must be None or a finite number, got 'x'"),
    "tol inf": (ValueError, lambda c: c.model.recommend_new(c.user_data, tol=float("inf")),
                "tol must be None or a finite number, got inf"),
    "weights": (ValueError, lambda c: c.model.recommend(weights=[1.0]),
                "weights has shape (1,), expected (5,): one per rating value"),
    "side": (ValueError, lambda c: c.model.distances(c.pairs, side="ratings"), "side must be 'items' or 'users', got 'ratings'"),
    "pairs": (ValueError, lambda c: c.model.explain([(1, 2, 3)]), "pairs must be (user, item) tuples"),
    "users": (KeyError, lambda c: c.model.recommend(users=[c.nobody, c.users[0], c.nobody, "?"]),
              lambda c: f"users not in the training data: {[c.nobody, '?']}"),
    "items": (KeyError, lambda c: c.model.recommend_users(items=[c.nobody]), lambda c: f"items not in the training data: {[c.nobody]}"),
    "candidates": (KeyError, lambda c: c.model.recommend(candidates=[c.items[0], c.nobody]),
                   lambda c: f"items not in the training data: {[c.nobody]}"),
    "pairs user": (KeyError, lambda c: c.model.explain([(c.nobody, c.items[0])]),
                   lambda c: f"users not in the training data: {[c.nobody]}"),
    "similar users": (KeyError, lambda c: c.model.similar_users([c.nobody]), lambda c: f"users not in the training data: {[c.nobody]}"),
    "distances": (KeyError, lambda c: c.model.distances([(c.items[0], c.nobody)]),
                  lambda c: f"items not in the training data: {[c.nobody]}"),
    "list_diversity": (KeyError, lambda c: c.model.list_diversity([("x", c.nobody)]),
                       lambda c: f"items not in the training data: {[c.nobody]}"),
    "top_pairs twice": (ValueError, lambda c: c.model.top_pairs(users=[c.users[0], c.users[1], c.users[0]]),
                        lambda c: f"users named more than once: {[c.users[0]]}"),
    "relevant": (ValueError, lambda c: c.model.ranking_score(c.held, relevant=[c.held["ratings"].iloc[0], 77]),
                 "relevant rating 77 is not a rating of the training data"),
    "relevant text": (ValueError, lambda c: c.model.ranking_score(c.held, relevant="45"),
                      "relevant must be a collection of rating values, got '45'"),
    "clash": (ValueError, lambda c: c.model.recommend_with_new_items(c.item_data.assign(items=c.items)),
              lambda c: "items of data are training items, so the frame would be ambiguous: "
                        f"{[str(x) if isinstance(x, str) else x for x in c.items]}"),
    "clash users": (ValueError, lambda c: c.model.recommend_users_new_items(c.item_data.assign(items=c.items)),
                    lambda c: f"items of data are training items, so the frame would be ambiguous: {c.items}"),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_word_for_word(host, name, mode):
    kind, call, text = REFUSALS[name]
    c = Case(host, mode)
    with pytest.raises(kind) as exc:
        call(c)
    assert exc.value.args[0] == (text(c) if callable(text) else text)


@pytest.mark.parametrize("mode", MODES)
def test_a_share_of_the_restarts_is_refused(host, mode):
    c = Case(host, mode)
    c.model._restart_ids = [0]
    text = ("this model holds 1 of its 2 restarts (restarts.fit_distributed without gather=True): fit with gather=True "
            "to recommend from all of them")
    for call in (lambda: c.model.recommend(), lambda: c.model.audience(min_score=0.0), lambda: c.model.align_restarts(),
                 lambda: c.model.log_likelihood(c.held), lambda: c.model.fold_in(c.user_data)):
        with pytest.raises(RuntimeError) as exc:
            call()
        assert exc.value.args[0] == text


def test_labels_are_looked_up_as_text_and_ids_as_integers(host):
    df = string_frame().assign(users=lambda d: d["users"].str[1:].astype(int))     # users 0 .. 11 as integers
    m = host.MMSBM(2, 3, iterations=3, sampling=2, seed=7)
    m.fit(df, silent=True)
    assert m.recommend(users=[7, "7"], n=1)["users"].tolist() == ["7", "7"]       # the encoder's label, not the caller's
    c = Case(host, "ids")
    with pytest.raises(KeyError) as exc:
        c.model.recommend(users=["3", 3, -1, c.model.p + 1, 2.0, -1])
    assert exc.value.args[0] == f"users not in the training data: {['3', -1, c.model.p + 1, 2.0]}"
