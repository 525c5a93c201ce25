"""Leave-one-out reliability of the training rows without a GPU: the restatement (tests/reliability_reference.py) against
the EM step it is a downdate of, and the host class's orchestration -- labels, training order, filters, min_ratings,
m=None, unknown labels, the refusal on a partial model -- through a stand-in device answered by the restatement.  The
device itself is checked in test_gpu_reliability.py.

TOL = 1e-12 absolute on probabilities (<= 1): the project's serving tolerance.  Measured here, soft and sharpened
parameters at the shapes of the device tests (printed with -s): the restatement against the brute force differs by at
most 3.1e-16, the restatement summed forwards and backwards by at most 7.8e-16 -- the band leaves three decades to the
device's different summation tree."""
import logging

import numpy as np
import pandas as pd
import pytest

import fake_device
import reliability_reference as rr
from oracle import mmsbm_oracle as orc
from test_recommend_cpu import fitted, string_frame

TOL = 1e-12
COLUMNS = ["users", "items", "rating", "fitted", "reliability", "surprise"]
CPU_SHAPES = [(3, 5), (20, 20), (70, 3), (4, 1)]
SHAPE_ID = lambda s: f"K{s[0]}L{s[1]}"  # noqa: E731


# ---- 1. the numerators are the EM step's -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["soft", "sharp", "zero"])
@pytest.mark.parametrize("shape", CPU_SHAPES, ids=SHAPE_ID)
def test_c_and_e_are_the_em_steps_numerators(shape, kind):
    data = rr.training_rows()
    theta, eta, pr = rr.model(*shape, 1, kind)[0]
    t = rr.slot_terms(data, theta, eta, pr)
    n_theta, n_eta = orc.update_coefficients(data, theta, eta, pr)[0:2]
    print(f"{shape} {kind}: |C - n_theta| {np.abs(t['C'] - n_theta).max():.3e}  |E - n_eta| {np.abs(t['E'] - n_eta).max():.3e}")
    assert np.abs(t["C"] - n_theta).max() <= TOL and np.abs(t["E"] - n_eta).max() <= TOL


# ---- 2. brute force: delete the row, take an EM step ----------------------------------------------------------------------
def sampled_rows(data):
    """About 25 rows: of the heavy user, of the heavy item, of the degree-2 user, of the planted users, the row whose
    user and item both hold nothing else, the lone items' rows, duplicated triples, and random ones."""
    rng = np.random.default_rng(5)
    u, i = data[:, 0], data[:, 1]
    pick = [np.flatnonzero(u == rr.HEAVY)[[0, 7, -1]], np.flatnonzero(i == rr.HEAVY_ITEM)[[0, 11, -1]],
            np.flatnonzero(u == 1), np.flatnonzero(u == 2)[:2], np.flatnonzero(u == 3)[:1], np.flatnonzero(u == 4)[:1],
            np.flatnonzero(i == rr.LONE_ITEM), np.flatnonzero(i == rr.LONE_ITEM_2), rng.integers(0, len(data), 10)]
    return np.unique(np.concatenate(pick))


def brute_force(data, j, theta, eta, pr, whole_table=False):
    """rel_j from an EM step of the reference on the table without row j, from the same (theta, eta, p): theta_u and
    eta_i of that step, the fitted p.  theta_u of the step depends on u's rows alone and eta_i on i's, so unless
    ``whole_table`` the step runs over the rows of u and of i only (the same numbers, a hundredth of the work).  A
    user (item) whose only row was row j has no row left: the mean row, by definition."""
    u, i, r = data[j]
    rest = np.delete(data, j, axis=0)
    if not whole_table:
        rest = rest[(rest[:, 0] == u) | (rest[:, 1] == i)]
    du, di = np.bincount(rest[:, 0], minlength=len(theta)), np.bincount(rest[:, 1], minlength=len(eta))
    if len(rest):
        t2, e2, _ = orc.em_step(rest, theta, eta, pr, np.maximum(du, 1), np.maximum(di, 1))
    tu = t2[u] if du[u] > 0 else theta.sum(axis=0) / len(theta)
    ei = e2[i] if di[i] > 0 else eta.sum(axis=0) / len(eta)
    return float(tu @ pr[:, :, r] @ ei)


@pytest.mark.parametrize("kind", ["soft", "sharp"])
@pytest.mark.parametrize("shape", CPU_SHAPES, ids=SHAPE_ID)
def test_reliability_is_one_em_step_without_the_row(shape, kind):
    data = rr.training_rows()
    theta, eta, pr = rr.model(*shape, 1, kind)[0]
    rel = rr.slot_reliability(data, theta, eta, pr)["rel"]
    rows = sampled_rows(data)
    assert 20 <= len(rows) <= 30
    du, di = np.bincount(data[:, 0]), np.bincount(data[:, 1])
    assert {1, 2, rr.HEAVY_ROWS} <= set(du[data[rows, 0]].tolist()) and {1, rr.HEAVY_ITEM_ROWS} <= set(di[data[rows, 1]].tolist())
    worst = 0.0
    for n, j in enumerate(rows.tolist()):
        want = brute_force(data, j, theta, eta, pr)
        if n < 3 and shape == (3, 5):
            assert want == brute_force(data, j, theta, eta, pr, whole_table=True)
        worst = max(worst, abs(rel[j] - want))
        assert abs(rel[j] - want) <= TOL, (shape, kind, j, rel[j], want)
    print(f"{shape} {kind}: worst |restatement - brute force| over {len(rows)} rows {worst:.3e} (TOL {TOL:.0e})")


@pytest.mark.parametrize("shape", [(3, 5), (20, 20)], ids=SHAPE_ID)
def test_the_order_of_the_sums_moves_the_restatement_far_less_than_the_band(shape):
    data = rr.training_rows()
    flip = np.arange(len(data))[::-1]
    for kind in ("soft", "sharp"):
        params = rr.model(*shape, 1, kind)
        fwd = rr.Restatement(data, params).reliability
        back = rr.Restatement(data[flip], params).reliability[flip]
        print(f"{shape} {kind}: forwards against backwards {np.abs(fwd - back).max():.3e}")
        assert np.abs(fwd - back).max() <= TOL / 100


def test_special_models_of_the_restatement():
    """One-hot theta: theta- is zero outside the user's group, and where every share of the user is exactly 1.0 (c =
    v (1 / v) rounds to 1.0 for most v, not for all) it IS the one-hot row, bit for bit.  An emptied rating tile: fit =
    0, the eps clamp gives shares of 0, reliability exactly 0 and surprise -log eps."""
    data = rr.training_rows()
    K, L = 5, 3
    theta, eta, pr = rr.model(K, L, 1, "onehot")[0]
    s = rr.slot_reliability(data, theta, eta, pr)
    u = data[:, 0]
    du = np.bincount(u, minlength=rr.U)
    many = du[u] > 1
    assert (s["theta_minus"][many][theta[u][many] == 0] == 0).all()
    t = rr.slot_terms(data, theta, eta, pr)
    unit = np.ones(rr.U, dtype=bool)
    np.logical_and.at(unit, u, t["c"].max(axis=1) == 1.0)
    exact = many & unit[u]
    assert exact.sum() > 50
    assert np.array_equal(s["theta_minus"][exact], theta[u][exact])
    assert np.abs(s["theta_minus"][many] - theta[u][many]).max() < 1e-13
    ref = rr.restatement(K, L, 1, "zero")
    gone = data[:, 2] == rr.ZERO_RATING
    assert gone.sum() > 1000 and (ref.fitted[gone] == 0).all() and (ref.reliability[gone] == 0).all()
    # (a row of another rating can reach 0 too: every OTHER row of its user, or of its item, had fit = 0)
    assert (ref.surprise[gone] == -np.log(rr.EPS)).all() and (ref.reliability[~gone] > 0).mean() > 0.99


# ---- 3. the host class through the stand-in --------------------------------------------------------------------------------
class LooFakeHipEM(fake_device.FakeHipEM):
    """FakeHipEM with the loo session, answered by the restatement."""
    _loo = None

    def loo_begin(self):
        self._loo = {"params": []}
        fake_device.LOG.append(("loo_begin", None))

    def loo_add(self):
        self._loo["params"].append(self.get_params())
        fake_device.LOG.append(("loo_add", self._sel))

    def _ref(self):
        assert self._loo["params"], "a loo query before loo_add"
        return rr.Restatement(self.data, self._loo["params"])

    def loo_rows(self, rows=None):
        fake_device.LOG.append(("loo_rows", None if rows is None else len(rows)))
        return self._ref().rows(rows)

    def loo_sides(self):
        fake_device.LOG.append(("loo_sides", None))
        return self._ref().sides()

    def loo_lowest(self, m, user_flags=None, item_flags=None):
        assert 1 <= m <= 1024
        for flags, size in ((user_flags, self.n_users), (item_flags, self.n_items)):
            assert flags is None or np.asarray(flags).shape == (size,)
        fake_device.LOG.append(("loo_lowest", m))
        return self._ref().lowest(m, user_flags, item_flags)

    def loo_end(self):
        self._loo = None
        fake_device.LOG.append(("loo_end", None))


@pytest.fixture
def host(monkeypatch):
    import mmsbm_amd.mmsbm as host
    monkeypatch.setattr(host, "HipEM", LooFakeHipEM)
    monkeypatch.setattr(host, "load_backend", lambda name: (None, None, None, "hip"))
    monkeypatch.setattr(LooFakeHipEM, "MAX_SLOTS", 1 << 20, raising=False)
    fake_device.LOG.clear()
    return host


def reference_of(m):
    return rr.Restatement(m.train, [(r["theta"], r["eta"], r["pr"]) for r in m.results])


def labelled(m, rows, ref):
    enc = m.data_handler
    ul, il, rl = np.asarray(enc.user_labels(), dtype=object), np.asarray(enc.item_labels(), dtype=object), \
        np.asarray(enc.rating_labels(), dtype=object)
    t = np.asarray(m.train)[rows]
    return pd.DataFrame({"users": ul[t[:, 0]], "items": il[t[:, 1]], "rating": rl[t[:, 2]], "fitted": ref.fitted[rows],
                         "reliability": ref.reliability[rows], "surprise": ref.surprise[rows]})


def same(got, want, columns=COLUMNS):
    assert list(got.columns) == columns
    for col in columns:
        if got[col].dtype == np.float64:
            np.testing.assert_array_equal(got[col].to_numpy(), want[col].to_numpy(dtype=np.float64), err_msg=col)
        else:
            assert got[col].tolist() == want[col].tolist(), col


def test_rating_reliability_covers_the_training_rows_in_training_order(host):
    df = string_frame()
    m = fitted(host, df)
    ref = reference_of(m)
    got = m.rating_reliability()
    same(got, labelled(m, np.arange(len(m.train)), ref))
    assert got["users"].tolist() == df["users"].tolist() and got["items"].tolist() == df["items"].tolist()
    assert got["rating"].astype(str).tolist() == df["ratings"].astype(str).tolist()
    assert got["fitted"].dtype == got["reliability"].dtype == got["surprise"].dtype == np.float64
    assert ((got["reliability"] >= 0) & (got["reliability"] <= 1)).all()
    names = [e for e, _ in fake_device.LOG]
    assert names.count("loo_begin") == 1 and names.count("loo_add") == 2 and names[-1] == "loo_end"
    m.predict(df.iloc[:40])
    before = m.score(silent=True)["stats"]
    m.rating_reliability()
    assert m.score(silent=True)["stats"] == before


def test_rating_reliability_of_pairs_and_unknown_labels(host, caplog):
    df = string_frame()
    m = fitted(host, df)
    ref = reference_of(m)
    ul, il = m.data_handler.user_labels(), m.data_handler.item_labels()
    t = np.asarray(m.train)
    pairs = [(int(t[5, 0]), int(t[5, 1])), (int(t[40, 0]), int(t[40, 1])), (int(t[5, 0]), int(t[5, 1]))]
    rows = np.flatnonzero([(int(a), int(b)) in set(pairs) for a, b in t[:, :2]])
    ask = [(ul[a], il[b]) for a, b in pairs]
    got = m.rating_reliability(ask)
    same(got, labelled(m, rows, ref))                                              # training order, every row once
    same(m.rating_reliability(pd.DataFrame({"who": [a for a, _ in ask], "what": [b for _, b in ask], "x": 1})), got)
    with caplog.at_level(logging.WARNING, logger="MMSBM"):
        same(m.rating_reliability(ask + [("nobody", il[0]), (ul[0], "no-such-item"), ("x", il[1])]), got)
    assert "The users nobody, x are in the test set but weren't in the train set so I'll remove them." in caplog.text
    assert "The items no-such-item are in the test set but weren't in the train set so I'll remove them." in caplog.text
    free = next((a, b) for a in range(len(ul)) for b in range(len(il)) if not ((t[:, 0] == a) & (t[:, 1] == b)).any())
    none = m.rating_reliability([(ul[free[0]], il[free[1]])])                      # a known pair nobody rated: no row
    assert len(none) == 0 and list(none.columns) == COLUMNS
    assert len(m.rating_reliability([])) == 0
    with pytest.raises(ValueError):
        m.rating_reliability([(ul[0], il[0], 3)])


def test_spurious_ratings_is_the_head_of_the_sorted_table_with_filters(host):
    m = fitted(host, string_frame())
    ref = reference_of(m)
    ul, il = m.data_handler.user_labels(), m.data_handler.item_labels()
    t = np.asarray(m.train)
    order = np.argsort(ref.reliability, kind="stable")
    for n in (1, 7, 1024):
        got = m.spurious_ratings(n)
        want = labelled(m, order[:n], ref)
        want["rank"] = np.arange(1, len(want) + 1)
        same(got, want, COLUMNS + ["rank"])
        assert got["rank"].dtype == np.int64 and (np.diff(got["reliability"].to_numpy()) >= 0).all()
    assert len(m.spurious_ratings()) == min(100, len(t))
    users, items = [ul[2], ul[5], ul[2]], [il[1], il[3], il[8], il[9]]
    uid, iid = [2, 5], [1, 3, 8, 9]
    for kw, ok in (({"users": users}, np.isin(t[:, 0], uid)), ({"items": items}, np.isin(t[:, 1], iid)),
                   ({"users": users, "items": items}, np.isin(t[:, 0], uid) & np.isin(t[:, 1], iid))):
        got = m.spurious_ratings(5, **kw)
        rows = [j for j in order.tolist() if ok[j]][:5]
        want = labelled(m, np.asarray(rows, dtype=np.int64), ref)
        want["rank"] = np.arange(1, len(rows) + 1)
        same(got, want, COLUMNS + ["rank"])
    for bad in (0, -1, 2.5, True, 1025):
        with pytest.raises(ValueError):
            m.spurious_ratings(bad)
    with pytest.raises(KeyError, match="users not in the training data.*nobody"):
        m.spurious_ratings(3, users=["nobody"])
    with pytest.raises(KeyError, match="items not in the training data"):
        m.spurious_ratings(3, items=["no-such-item"])


@pytest.mark.parametrize("side", ["users", "items"])
def test_misfit_tables(host, side):
    m = fitted(host, string_frame())
    ref = reference_of(m)
    labels = np.asarray((m.data_handler.user_labels if side == "users" else m.data_handler.item_labels)(), dtype=object)
    sur, fsur = ref.sides()[:2] if side == "users" else ref.sides()[2:]
    degree = np.bincount(np.asarray(m.train)[:, 0 if side == "users" else 1], minlength=len(labels))
    call = m.misfit_users if side == "users" else m.misfit_items
    for min_ratings in (1, 2, 5):
        ids = np.flatnonzero(degree >= min_ratings)
        ids = ids[np.lexsort((ids, -sur[ids]))]
        for top in (None, 3):
            got = call(m=top, min_ratings=min_ratings)
            want = ids[:top]
            assert list(got.columns) == [side, "ratings", "surprise", "fitted_surprise"]
            assert got[side].tolist() == labels[want].tolist() and got["ratings"].tolist() == degree[want].tolist()
            assert got["ratings"].dtype == np.int64
            np.testing.assert_array_equal(got["surprise"].to_numpy(), sur[want])
            np.testing.assert_array_equal(got["fitted_surprise"].to_numpy(), fsur[want])
            assert (np.diff(got["surprise"].to_numpy()) <= 0).all()
    assert len(call()) == (degree >= 2).sum()                                      # the defaults: everything, two rows up
    for bad in ({"m": 0}, {"m": 2.5}, {"min_ratings": 0}, {"min_ratings": True}):
        with pytest.raises(ValueError):
            call(**bad)


def test_a_partial_distributed_model_is_refused(host):
    m = fitted(host, string_frame(), sampling=3)
    fake_device.LOG.clear()
    m._restart_ids = m._restart_ids[:1]
    m.results = m.results[:1]
    for call in (m.rating_reliability, m.spurious_ratings, m.misfit_users, m.misfit_items):
        with pytest.raises(RuntimeError, match="1 of its 3 restarts"):
            call()
    assert not [e for e, _ in fake_device.LOG if e.startswith("loo_")]


def test_the_session_ends_when_a_query_fails(host, monkeypatch):
    m = fitted(host, string_frame())

    def broken(self, rows=None):
        raise RuntimeError("the device said no")
    monkeypatch.setattr(LooFakeHipEM, "loo_rows", broken)
    fake_device.LOG.clear()
    with pytest.raises(RuntimeError, match="the device said no"):
        m.rating_reliability()
    assert [e for e, _ in fake_device.LOG][-1] == "loo_end"
