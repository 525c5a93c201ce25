"""pass_dense.hpp: the two triple passes and the T + S stage of a committed iteration as ONE launch -- pair units that keep
their C rows in LDS, the user segments' workgroups dealt through the same grid.  The form is forced (`pass_dense` = 1) on
small data and compared, bit for bit, with the same context run with the separate launches (`pass_dense` = 0, `fused` = 0):
arithmetic and association order of every sum are unchanged, so theta, eta and p must be IDENTICAL, not close.  One step is
also checked against the oracle at the suite's TOL_STEP.  Needs a real MI355X: run with ``-m gpu``."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err
from oracle import mmsbm_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402  (demangling + canonical kernel names, shared with the coverage report)

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-12   # the suite's bound for one step against the oracle (tests/test_gpu_parity.py)
KERNEL = "pass_dense_kernel<8,4>"


@pytest.fixture(scope="module")
def hip():
    from mmsbm_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("-m gpu tests need a GPU: no HIP device visible (no CPU fallback exists)")
    import mmsbm_amd
    return mmsbm_amd


class LaunchWindow:
    """Kernels this process launched since __enter__ (the library appends to the log when a context is destroyed)."""

    def __enter__(self):
        self.path = os.environ.get("MMSBM_HIP_LAUNCH_LOG", "")
        self.pos = os.path.getsize(self.path) if self.path and os.path.exists(self.path) else 0
        return self

    def __exit__(self, *exc):
        return False

    def names(self):
        if not self.path:
            pytest.skip("launch log switched off (MMSBM_HIP_LAUNCH_LOG is empty)")
        with open(self.path) as fh:
            fh.seek(self.pos)
            rows = [ln.rstrip("\n").split("\t") for ln in fh]
        mine = [r[2] for r in rows if len(r) >= 4 and r[0] == str(os.getpid())]
        return {kernel_coverage.canon(n) for n in kernel_coverage.demangle(mine)} if mine else set()


def regular(n_u, n_i, n_r, per_user):
    """Every user rates exactly `per_user` items, the items and ratings dealt evenly: no segment length stands out, so the
    layout builds no work list on either side whatever the ratio of users to items."""
    u = np.repeat(np.arange(n_u), per_user)
    j = np.tile(np.arange(per_user), n_u)
    i = (u * 7 + j * 31) % n_i
    r = (u + 3 * j) % n_r
    return np.stack([u, i, r], axis=1).astype(np.int64)


def make_case(name):
    """(data, K, L, the form applies).  Base: about 3,000 triples of 300 users x 70 items, R = 5 -- <= 350 pairs, several
    units per rating, every rating ending in a ragged unit, the unit list padded with empty units."""
    base = orc.synthetic_triples(3000, 300, 70, 5, seed=3)
    if name == "base":
        return base, 20, 20, True
    if name == "k17":        # the first lane of the group's last: one live entry in lane 4
        return base, 17, 17, True
    if name == "k32_l24":    # the last lane of the group, with the longest rows 256 threads take
        return base, 32, 24, True
    if name == "k32":        # L = 32 runs T + S with 512 threads: another split of S's sums -- the form must decline
        return base, 32, 32, False
    if name == "k20_l28":    # ... L = 28 too
        return base, 20, 28, False
    if name == "k28_l20":
        return base, 28, 20, True
    if name == "r1":         # one rating: a single run of units, no padding
        return orc.synthetic_triples(3000, 300, 200, 1, seed=4), 20, 20, True
    if name == "absent":     # user 11 and item 5 never occur: an empty user segment, and no pair of item 5
        return base[(base[:, 0] != 11) & (base[:, 1] != 5)], 20, 20, True
    if name == "lengths":    # a pair with ONE triple, a pair and a user with more than 16 (two index chunks), below the cut at 64
        d = base[~((base[:, 1] == 8) & (base[:, 2] == 2)) & (base[:, 0] != 40)]
        one = np.array([[17, 8, 2]])
        long_pair = np.stack([np.arange(100, 140), np.full(40, 9), np.full(40, 3)], axis=1)
        long_user = np.stack([np.full(37, 40), np.arange(37), np.arange(37) % 5], axis=1)
        return np.concatenate([d, one, long_pair, long_user]).astype(np.int64), 20, 20, True
    if name == "swap":       # fewer users than items: the context swaps the sides
        return base[:, [1, 0, 2]].copy(), 20, 20, True
    if name == "many_users":  # 4 pair units, the last of 8 pairs, and 63 user workgroups (base: 40 units, 30 of them empty,
        return regular(2000, 200, 1, 1), 20, 20, True   # and 10 workgroups); pairs of 10 triples: longer ones of so few are cut
    raise KeyError(name)


def start_of(data, k, l, seed=5):
    n_u, n_i, n_r = (int(data[:, j].max()) + 1 for j in range(3))
    d_u, d_i = orc.degrees(data, n_u, n_i)
    return (n_u, n_i, n_r), (d_u, d_i), orc.init_params(seed, n_u, n_i, n_r, k, l, d_u, d_i)


def run(hip, data, k, l, dims, start, dense, steps=(1, 4), applies=True, **kw):
    """theta, eta, p and the likelihood after each of `steps` further committed iterations."""
    out = []
    with hip.HipEM(data, k, l, *dims, **kw) as em:
        em.set_option("fused", 0)
        em.set_option("pass_dense", dense)
        assert em.get_option("pass_dense") == (1.0 if dense and applies else 0.0)
        assert em.get_option("launches") == 4.0       # the form family: separate stages, with or without pass_dense
        em.set_params(*start)
        for its in steps:
            em.iterate(its)
            out.append((*em.get_params(), em.likelihood()))
    return out


def assert_same(a, b, what):
    assert len(a) == len(b)
    for j, (ra, rb) in enumerate(zip(a, b)):
        for x, y, nm in zip(ra, rb, ("theta", "eta", "p", "likelihood")):
            assert np.array_equal(np.asarray(x), np.asarray(y)), (what, j, nm)


_separate = {}


def separate(hip, name):
    """The separate launches' run of a case: computed once, shared, never changed."""
    if name not in _separate:
        data, k, l, applies = make_case(name)
        dims, _, start = start_of(data, k, l)
        _separate[name] = (data, k, l, applies, dims, start, run(hip, data, k, l, dims, start, 0))
    return _separate[name]


@pytest.mark.parametrize("name", ["base", "k17", "k32_l24", "k32", "k20_l28", "k28_l20", "r1", "absent", "lengths", "swap",
                                  "many_users"])
def test_bitwise_the_separate_launches(hip, name):
    """theta, eta, p and the likelihood after 1 and after 5 committed iterations, bit for bit; where the shape is outside
    the form (512-thread T + S) the option reads 0 when forced and the results are the separate launches' own.  The
    library keeps ONE block order (pair units, then user workgroups); its two ends are `base` -- 40 pair units, 30 of them
    empty, and 10 user workgroups -- and `many_users`, 4 and 63."""
    data, k, l, applies, dims, start, want = separate(hip, name)
    with LaunchWindow() as lw:
        got = run(hip, data, k, l, dims, start, 1, applies=applies)
        assert (KERNEL in lw.names()) == applies
    assert_same(got, want, name)


def test_one_step_against_the_oracle(hip):
    data, k, l, _ = make_case("base")
    dims, (d_u, d_i), start = start_of(data, k, l)
    got = run(hip, data, k, l, dims, start, 1, steps=(1,))[0]
    for g, w, nm in zip(got, orc.em_step(data, *start, d_u, d_i), ("theta", "eta", "p")):
        assert rel_err(g, w) < TOL_STEP, nm


def test_switch_of_forms_in_mid_run(hip):
    """off -> on -> off, two iterations each, equals six iterations of the separate launches."""
    data, k, l, _, dims, start, _ = separate(hip, "base")
    want = run(hip, data, k, l, dims, start, 0, steps=(6,))
    with hip.HipEM(data, k, l, *dims) as em:
        em.set_option("fused", 0)
        em.set_params(*start)
        for dense in (0, 1, 0):
            em.set_option("pass_dense", dense)
            assert em.get_option("pass_dense") == float(dense)
            em.iterate(2)
        got = [(*em.get_params(), em.likelihood())]
    assert_same(got, want, "switch")


def test_graph_replay_and_repeat(hip):
    """A replayed graph of two iterations gives the eager run's bits, and two runs of the form are bitwise equal."""
    data, k, l, _, dims, start, _ = separate(hip, "base")
    eager = run(hip, data, k, l, dims, start, 1, steps=(4,))
    assert_same(run(hip, data, k, l, dims, start, 1, steps=(4,)), eager, "repeat")
    with hip.HipEM(data, k, l, *dims) as em:
        em.set_option("fused", 0)
        em.set_option("pass_dense", 1)
        em.set_params(*start)
        em.set_graph_mode(1)
        em.iterate(4)
        em.set_graph_mode(0)
        got = [(*em.get_params(), em.likelihood())]
    assert_same(got, eager, "graph")


def test_update_coefficients_keeps_the_separate_launches(hip):
    """commit off needs the raw numerators: the same values whether the form is on or off, and the iteration after it too."""
    data, k, l, _, dims, start, _ = separate(hip, "base")
    outs = []
    for dense in (0, 1):
        with hip.HipEM(data, k, l, *dims) as em:
            em.set_option("fused", 0)
            em.set_option("pass_dense", dense)
            em.set_params(*start)
            num = em.update_coefficients()
            em.iterate(2)
            outs.append([(*num, 0.0), (*em.get_params(), em.likelihood())])
    assert_same(outs[1], outs[0], "update_coefficients")


def test_declines_split_segments_and_two_slots(hip):
    """Data with cut segments, and a context with two restart slots: the option reads 0 when forced, results unchanged."""
    rng = np.random.default_rng(11)
    n = 6000
    u_col = np.where(rng.random(n) < 0.3, 5, rng.integers(0, 300, n))       # one user with 30 % of the rows
    cut = np.stack([u_col, rng.integers(0, 70, n), rng.integers(0, 5, n)], axis=1).astype(np.int64)
    dims, _, start = start_of(cut, 20, 20)
    with hip.HipEM(cut, 20, 20, *dims) as em:
        assert em.get_option("splits_users") > 0
    assert_same(run(hip, cut, 20, 20, dims, start, 1, applies=False), run(hip, cut, 20, 20, dims, start, 0), "cut segments")
    data, k, l, _, dims, start, want = separate(hip, "base")
    got = {}
    for dense in (0, 1):
        with hip.HipEM(data, k, l, *dims, slots=2) as em:
            em.set_option("fused", 0)
            em.set_option("pass_dense", dense)
            assert em.get_option("pass_dense") == 0.0
            em.select(0).set_params(*start)
            em.select(1).set_params(start[0] * 0.5 + 0.01, start[1], start[2])
            em.iterate(5)
            got[dense] = [em.select(s).get_params() for s in range(2)]
    for s in range(2):
        for a, b in zip(got[1][s], got[0][s]):
            assert np.array_equal(a, b)
    for a, b in zip(got[1][0], want[1][:3]):    # slot 0: the one-slot run after 1 + 4 iterations
        assert np.array_equal(a, b)


def test_every_compiled_instantiation_is_launched_by_a_parity_case(hip):
    """scripts/kernel_coverage.py's view: the compiled pass_dense_kernel instantiations against what a parity case of this
    file launches."""
    compiled = {k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("pass_dense_kernel")}
    assert compiled == {KERNEL}
    data, k, l, _, dims, start, want = separate(hip, "base")
    with LaunchWindow() as lw:
        assert_same(run(hip, data, k, l, dims, start, 1), want, "coverage")
        assert compiled <= lw.names()
