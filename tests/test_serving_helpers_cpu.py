"""The helpers the serving methods share (mmsbm_amd/serving.py): grouped lists, a batch's slice of one, the label table
of a side and the two argument checks, each against a restatement a reader can check by eye."""
import numpy as np
import pytest

from mmsbm_amd.serving import _Side, check_finite, check_integer, group_slice, grouped


def brute(keys, values, n_groups, sort, distinct):
    lists = [[] for _ in range(n_groups)]
    for k, v in zip(keys, values):
        lists[k].append(v)
    if sort:
        lists = [sorted(x) for x in lists]
    if distinct:
        lists = [sorted(set(x)) for x in lists]
    return lists


@pytest.mark.parametrize("sort,distinct", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("n,n_groups", [(0, 0), (0, 3), (1, 1), (40, 7), (200, 5), (30, 60)])
def test_grouped_against_a_loop(n, n_groups, sort, distinct):
    rng = np.random.default_rng(n + n_groups)
    keys = rng.integers(0, max(n_groups, 1), n)
    values = rng.integers(0, 6, n)                                  # few values: duplicates within a group
    if n:
        keys[0] = n_groups - 1                                      # the largest key there can be
    off, got = grouped(keys, values, n_groups, sort=sort, distinct=distinct)
    assert off.dtype == np.int64 and got.dtype == np.int32 and off.shape == (n_groups + 1,)
    assert off[0] == 0 and off[-1] == len(got)
    want = brute(keys.tolist(), values.tolist(), n_groups, sort, distinct)
    assert [got[off[g]:off[g + 1]].tolist() for g in range(n_groups)] == want
    if n_groups > n:
        assert (np.diff(off) == 0).any()                            # empty groups, also behind the last key


def test_grouped_keeps_input_order_and_takes_lists():
    off, got = grouped([2, 0, 2, 0, 2], [9, 8, 7, 8, 9], 4)
    assert off.tolist() == [0, 2, 2, 5, 5] and got.tolist() == [8, 8, 9, 7, 9]
    off, got = grouped([2, 0, 2, 0, 2], [9, 8, 7, 8, 9], 4, sort=True, distinct=True)
    assert off.tolist() == [0, 1, 1, 3, 3] and got.tolist() == [8, 7, 9]
    off, got = grouped([], [], 0)
    assert off.tolist() == [0] and got.tolist() == []


def test_group_slice():
    lists = grouped([0, 0, 1, 3, 3, 3], [5, 6, 7, 8, 9, 10], 4)
    n = 4
    for b, e in [(0, n), (0, 0), (n, n), (2, 2), (1, 3), (0, 1), (3, 4)]:
        off, values = group_slice(lists, b, e)
        assert off.dtype == np.int64 and off[0] == 0 and off.shape == (e - b + 1,)
        assert [values[off[g]:off[g + 1]].tolist() for g in range(e - b)] == \
               [lists[1][lists[0][g]:lists[0][g + 1]].tolist() for g in range(b, e)]
    assert group_slice(lists, 1, 3)[0].tolist() == [0, 1, 1] and group_slice(lists, 1, 3)[1].tolist() == [7]
    assert group_slice(None, 0, 2) is None


def test_side_with_an_encoder():
    side = _Side("users", 4, np.asarray(["10", "7", "ann", "True"], dtype=object))
    assert len(side) == 4
    assert side.ids([7, "7", np.int64(10), "ann", True, 7.0, None, -1, 4]).tolist() == [1, 1, 0, 2, 3, -1, -1, -1, -1]
    assert side.ids([]).dtype == np.int32 and side.ids(["ann"]).dtype == np.int32
    assert side.label(np.array([2, 0], dtype=np.int32)).tolist() == ["ann", "10"] and side.label([]).dtype == object
    assert side.index() == ["10", "7", "ann", "True"]
    ids, labels = side.request(None)
    assert ids.dtype == np.int32 and ids.tolist() == [0, 1, 2, 3] and labels.tolist() == side.index()
    ids, labels = side.request([7, "ann", "7"])
    assert ids.tolist() == [1, 2, 1] and labels.tolist() == ["7", "ann", "7"]        # the encoder's spelling
    ids, labels = side.request([])
    assert ids.dtype == np.int32 and len(ids) == 0 and labels.dtype == object
    with pytest.raises(KeyError) as exc:
        side.request(["bob", 7, "bob", 8, "bob"])
    assert exc.value.args[0] == "users not in the training data: ['bob', 8]"
    more = side.extended(np.asarray(["new"], dtype=object))
    assert len(more) == 5 and more.label([4, 1]).tolist() == ["new", "7"] and more.labels.dtype == object


def test_side_without_an_encoder():
    side = _Side("items", 5)
    asked = [3, np.int32(0), "3", 3.0, -1, 5, True, np.True_, None, 4]
    assert side.ids(asked).tolist() == [3, 0, -1, -1, -1, -1, 1, -1, -1, 4]   # (True is the int 1, as it has always been)
    assert side.label(np.array([4, 2], dtype=np.int32)).dtype == np.int64 and side.index() is None
    ids, labels = side.request(None)
    assert ids.dtype == np.int32 and labels is ids and ids.tolist() == [0, 1, 2, 3, 4]
    ids, labels = side.request([4, 4, 0])
    assert ids.tolist() == [4, 4, 0] and labels.tolist() == [4, 4, 0]
    with pytest.raises(KeyError) as exc:
        side.request([5, 1, -1, 5, "1"])
    assert exc.value.args[0] == "items not in the training data: [5, -1, '1']"
    ratings = _Side("ratings", 3, known=[0, 2, 4])                  # the rating ids in use, not a range
    assert ratings.ids([0, 1, 2, 3, 4, 5]).tolist() == [0, -1, 2, -1, 4, -1] and len(ratings) == 3
    more = side.extended(np.asarray([57, 3], dtype=np.int64))       # new items keep the caller's numbers as labels
    assert more.label([5, 6, 2]).tolist() == [57, 3, 2] and more.labels.dtype == np.int64


def test_a_kept_index_belongs_to_its_encoder(monkeypatch):
    import fake_device
    import mmsbm_amd.mmsbm as host
    from test_recommend_cpu import RecommendFakeHipEM, string_frame
    monkeypatch.setattr(host, "HipEM", RecommendFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(RecommendFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    m = host.MMSBM(2, 3, iterations=2, sampling=1, seed=7)
    m.fit(string_frame(), silent=True)
    first = m._side("users")
    assert m._side("users") is first and "u3" in first.index()
    m.fit(string_frame().assign(users=lambda d: "w" + d["users"]), silent=True)          # a second fit: other labels
    assert m._side("users") is not first and m.recommend(users=["wu3"], n=1)["users"].tolist() == ["wu3"]
    with pytest.raises(KeyError):
        m.recommend(users=["u3"])
    other = host.MMSBM(2, 3, iterations=2, sampling=1, seed=7)                            # tables are per model
    other.fit(string_frame(), silent=True)
    assert other._side("users") is not m._side("users") and "u3" in other._side("users").index()
    m.fit_encoded(np.asarray(m.train))                                                    # no encoder: ids, built afresh
    m.data_handler = None
    assert m._side("users").labels is None and m.recommend(users=[3], n=1)["users"].tolist() == [3]


def test_checks():
    assert check_integer(np.int64(3), "n", 1) == 3 and type(check_integer(np.int64(3), "n", 1)) is int
    assert check_integer(0, "iterations", 0, "a non-negative integer") == 0
    assert check_integer(-5, "reference", None, "a position") == -5
    for bad in (True, np.True_, 2.0, "2", None, 0):
        with pytest.raises(ValueError, match="^n must be a positive integer, got "):
            check_integer(bad, "n", 1)
    with pytest.raises(ValueError) as exc:
        check_integer(True, "k", 1, "a positive integer or a list of them", got=[3, True])
    assert exc.value.args[0] == "k must be a positive integer or a list of them, got [3, True]"
    assert check_finite(2, "tol") == 2.0 and type(check_finite(np.float32(0.5), "tol")) is float
    assert check_finite(True, "tol", bool_too=True) == 1.0
    for bad in (True, "1", None, float("nan"), float("-inf"), np.True_):
        with pytest.raises(ValueError, match="^min_score must be a finite number, got "):
            check_finite(bad, "min_score")
    with pytest.raises(ValueError) as exc:
        check_finite(-0.5, "diversity", 0, "a finite number >= 0")
    assert exc.value.args[0] == "diversity must be a finite number >= 0, got -0.5"
