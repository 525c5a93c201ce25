"""pass_dense.hpp, the pair units' own A rows: a unit of the merged launch computes A(t)[q,:] = pT_r eta[i_q,:] of its 64
pairs itself (the A launch's mat-vec, multiply-add for multiply-add) instead of loading the rows from the A table, holds
them transposed in the LDS region that first took the eta rows and later takes the C rows, and so needs lp rows there when
lp > kp.  Nothing may change: the form is forced (`pass_dense` = 1) on small data and compared, bit for bit, with the
separate launches (`pass_dense` = 0, `fused` = 0), whose pair pass reads the A table the A launch wrote.  The cases are the
ones tests/test_gpu_pass_dense.py lacks: lp > kp, L = 1 and 3, last units of one pair and of 63, a rating that never
occurs, an all-zero eta row and zero tile entries, set_params in mid-run, graph replay.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import mmsbm_oracle as orc

import test_gpu_pass_dense as base   # the existing file's helpers: run, assert_same, start_of, LaunchWindow

pytestmark = pytest.mark.gpu

TOL_STEP = base.TOL_STEP   # the suite's bound for one step against the oracle
KERNEL = base.KERNEL
STEPS = (1, 2)             # results after 1 and after 1 + 2 = 3 committed iterations


@pytest.fixture(scope="module")
def hip():
    from mmsbm_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("-m gpu tests need a GPU: no HIP device visible (no CPU fallback exists)")
    import mmsbm_amd
    return mmsbm_amd


def tails():
    """300 users x 130 items.  Rating 0 is given to items 0 .. 64 -- 65 pairs, a full unit and a last unit of ONE pair --,
    rating 1 to items 0 .. 126 -- 127 pairs, a last unit of 63 --, rating 2 to 40 items (one ragged unit), rating 4 to every
    item (two full units and one of two pairs); rating 3 never occurs: its tile has no unit.  Each pair has 2 .. 8 triples.
    The users of one rating are a block of their own, sized by the rating's triples and dealt in turn, so that no
    (user, item) occurs twice and every user has the same number of triples to within one or two: neither side's segment
    lengths stand out (coefficient of variation below 0.5), the layout builds no work list, and the form applies."""
    rng = np.random.default_rng(21)
    plan = [(r, list(items), rng.integers(2, 9, size=len(items))) for r, items in
            ((0, range(65)), (1, range(127)), (2, range(3, 43)), (4, range(130)))]
    total = sum(int(n.sum()) for _, _, n in plan)
    rows, first = [], 0
    for j, (r, items, lens) in enumerate(plan):
        size = 300 - first if j == len(plan) - 1 else int(round(300 * int(lens.sum()) / total))
        nxt = 0
        for i, n in zip(items, lens):
            for _ in range(int(n)):
                rows.append((first + nxt % size, i, r))
                nxt += 1
        first += size
    return np.array(rows, dtype=np.int64)


def make_case(name):
    """(data, K, L).  Base: about 3,000 triples of 300 users x 70 items, R = 5, as in tests/test_gpu_pass_dense.py."""
    data = orc.synthetic_triples(3000, 300, 70, 5, seed=3)
    if name == "k20_l24":    # lp > kp: the first LDS region holds lp = 24 rows of eta before kp = 20 of A and C
        return data, 20, 24
    if name == "k17_l24":    # ... and a padded K beside it (kp = 20, three zero columns of the tile)
        return data, 17, 24
    if name == "l1":         # lp = 4: one chunk of four inputs, three of them padding
        return data, 20, 1
    if name == "l3":
        return data, 20, 3
    if name == "tails":      # last units of one pair and of 63 pairs, and rating 3 absent
        return tails(), 20, 20
    if name == "tails_l24":
        return tails(), 17, 24
    if name == "no_r3":      # the base data without rating 3: R stays 5, the rating has a tile and no unit
        return data[data[:, 2] != 3], 20, 20
    raise KeyError(name)


CASES = ["k20_l24", "k17_l24", "l1", "l3", "tails", "tails_l24", "no_r3"]


def start_of(data, k, l, seed=5, n_r=5):
    dims, deg, start = base.start_of(data, k, l, seed)
    assert dims[2] == n_r
    return dims, deg, start


_separate = {}


def separate(hip, name):
    """The separate launches' run of a case: computed once, shared, never changed."""
    if name not in _separate:
        data, k, l = make_case(name)
        dims, deg, start = start_of(data, k, l)
        _separate[name] = (data, k, l, dims, deg, start, base.run(hip, data, k, l, dims, start, 0, steps=STEPS))
    return _separate[name]


def test_the_tails_data_has_the_units_it_is_for():
    data = tails()
    pairs = {r: len(np.unique(data[data[:, 2] == r, 1])) for r in range(5)}
    assert pairs == {0: 65, 1: 127, 2: 40, 3: 0, 4: 130}
    assert len(np.unique(data[:, 0])) == 300 and len(np.unique(data[:, :2], axis=0)) == len(data)
    for lens in (np.bincount(data[:, 0]), np.unique(data[:, 1:], axis=0, return_counts=True)[1]):
        assert lens.max() <= 16 and lens.std() < 0.5 * lens.mean()    # no cut segment, no work list


@pytest.mark.parametrize("name", CASES)
def test_bitwise_the_separate_launches(hip, name):
    """theta, eta, p and the likelihood after 1 and after 3 committed iterations, bit for bit, and the kernel ran."""
    data, k, l, dims, _, start, want = separate(hip, name)
    with base.LaunchWindow() as lw:
        got = base.run(hip, data, k, l, dims, start, 1, steps=STEPS)
        assert KERNEL in lw.names()
    base.assert_same(got, want, name)


@pytest.mark.parametrize("name", ["k17_l24", "tails", "l3"])
def test_one_step_against_the_oracle(hip, name):
    data, k, l, dims, (d_u, d_i), start, _ = separate(hip, name)
    got = base.run(hip, data, k, l, dims, start, 1, steps=(1,))[0]
    for g, w, nm in zip(got, orc.em_step(data, *start, d_u, d_i), ("theta", "eta", "p")):
        assert rel_err(g, w) < TOL_STEP, nm


def zeroed(start):
    """The start with an all-zero eta row (items 7 and 64: A rows of 0, every triple of theirs at the eps clamp), a zero
    column and a zero row of rating 1's tile, and rating 2's tile all zero."""
    theta, eta, pr = (x.copy() for x in start)
    eta[7, :] = 0.0
    eta[64, :] = 0.0
    pr[:, 2, 1] = 0.0
    pr[3, :, 1] = 0.0
    pr[:, :, 2] = 0.0
    return theta, eta, pr


@pytest.mark.parametrize("name", ["tails", "k17_l24"])
def test_zero_eta_rows_and_zero_tile_entries(hip, name):
    """Staged with set_params, not normalised: the unit's A rows of 0 and the table's are the same zeros, the clamp gives
    the same weights, and everything stays finite."""
    data, k, l, dims, (d_u, d_i), start, _ = separate(hip, name)
    z = zeroed(start)
    want = base.run(hip, data, k, l, dims, z, 0, steps=STEPS)
    with base.LaunchWindow() as lw:
        got = base.run(hip, data, k, l, dims, z, 1, steps=STEPS)
        assert KERNEL in lw.names()
    base.assert_same(got, want, name)
    assert all(np.isfinite(np.asarray(x)).all() for res in got for x in res[:3])
    for g, w, nm in zip(got[0], orc.em_step(data, *z, d_u, d_i), ("theta", "eta", "p")):
        assert rel_err(g, w) < TOL_STEP, nm


def test_set_params_in_mid_run(hip):
    """Two iterations, new parameters, two more: the A table then comes from ensure_a (the user pass reads it) and the
    units' A rows from the same parameters."""
    data, k, l, dims, _, start, _ = separate(hip, "k20_l24")
    other = base.start_of(data, k, l, seed=9)[2]
    outs = []
    for dense in (0, 1):
        with hip.HipEM(data, k, l, *dims) as em:
            em.set_option("fused", 0)
            em.set_option("pass_dense", dense)
            assert em.get_option("pass_dense") == float(dense)
            em.set_params(*start)
            em.iterate(2)
            em.set_params(*other)
            em.iterate(1)
            first = (*em.get_params(), em.likelihood())
            em.set_params(*zeroed(other))
            em.iterate(2)
            outs.append([first, (*em.get_params(), em.likelihood())])
    base.assert_same(outs[1], outs[0], "set_params in mid-run")


@pytest.mark.parametrize("name", ["k20_l24", "tails"])
def test_graph_replay(hip, name):
    """A replayed graph of three iterations gives the separate launches' bits."""
    data, k, l, dims, _, start, want = separate(hip, name)
    with hip.HipEM(data, k, l, *dims) as em:
        em.set_option("fused", 0)
        em.set_option("pass_dense", 1)
        assert em.get_option("pass_dense") == 1.0
        em.set_params(*start)
        em.set_graph_mode(1)
        em.iterate(sum(STEPS))
        em.set_graph_mode(0)
        got = [(*em.get_params(), em.likelihood())]
    base.assert_same(got, want[-1:], "graph")
