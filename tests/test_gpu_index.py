"""The index a context holds, read back array by array (mmsbm_hip_index_array, HipEM.index_arrays) and compared by
equality: the sort stage of both builders -- layout.hpp on the host, tu_layout.hip on the device -- against the numpy
restatement of index_reference.py on every table of index_cases.py (sizes around the 256-thread workgroup, id ranges
around the widths of the three radix sorts, (rating, item) key spaces up to 2^31 and beyond, where a context must fall
back to the host builder), the default switch between the builders at 100,000 triples, everything create() derives from
the sorts (chunks, unit lists, work lists, splits, the item grid, the likelihood's units) host-built against
device-built, and the XCD-local work lists cut from positions found on the device (range_cuts_kernel) at range counts
that do not divide the table, exceed its rows, or meet a table of one row.  Integer data: no tolerance anywhere but in
the one EM step on a wide key space, which is held to the oracle at the parity file's 1e-12.

test_index_reference_cpu.py pins the restatement to the host builder without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import border_tables as bt
import index_cases as ic
import index_reference as ir
from conftest import ROOT, rel_err
from oracle import mmsbm_oracle as orc
from test_gpu_instantiations import LaunchWindow, hip  # noqa: F401  (hip: the fixture)

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-12           # one update_coefficients call, relative to max |want| (test_gpu_parity.py)
DEVICE_KEY_SPACE = 2 ** 31     # build_index: ratings x items from which the sorts stay on the host
LAYOUT_KERNELS = ("make_keys", "split_keys", "scatter_heads", "iota", "lower_bounds", "item_degrees", "range_cuts_kernel")
WINDOW = {}
_REFS = {}


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the coverage test)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


def reference(name, swap):
    """index_reference.sort_stage of the columns a context of swap_sides = `swap` sorts: once per (case, swap), read-only."""
    if (name, swap) not in _REFS:
        _, data, *dims = ic.case(name)
        cols, idims = ic.internal(data, tuple(dims), swap)
        ref = ir.sort_stage(cols, *idims)
        for a in ref.values():
            a.setflags(write=False)
        _REFS[name, swap] = (ref, idims)
    return _REFS[name, swap]


def builder(monkeypatch, gpu):
    if gpu is None:
        monkeypatch.delenv("MMSBM_HIP_GPU_LAYOUT", raising=False)
    else:
        monkeypatch.setenv("MMSBM_HIP_GPU_LAYOUT", str(gpu))


def assert_sort_stage(em, ref, idims, data, dims, what):
    """The nine arrays, n_pairs and the degrees of an open context against the restatement."""
    got = em.index_arrays()
    wrong = ir.differing(got, ref)
    assert not wrong, (what, "arrays that differ from the numpy restatement", wrong,
                       {nm: (len(got[nm]), len(ref[nm])) for nm in wrong})
    assert em.n_pairs == len(ref["pair_item"]), what
    d_u, d_i = em.degrees()
    assert np.array_equal(d_u, np.maximum(np.bincount(data[:, 0], minlength=dims[0]), 1)), (what, "d_u")
    assert np.array_equal(d_i, np.maximum(np.bincount(data[:, 1], minlength=dims[1]), 1)), (what, "d_i")
    return got


# ---- a. the sort stage of both builders on every case ----
@pytest.mark.parametrize("gpu", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("name", ic.SORT_NAMES)
def test_sort_stage_equals_the_numpy_restatement(hip, name, swap, gpu, monkeypatch):
    _, data, *dims = ic.case(name)
    ref, idims = reference(name, swap)
    builder(monkeypatch, gpu)
    with hip.HipEM(data, 2, 2, *dims, swap_sides=swap) as em:
        assert em.swapped == bool(swap)
        # (the device sort packs (rating, item) into 31 bits: beyond that the host builder, whatever was asked for)
        want = float(gpu) if idims[1] * idims[2] < DEVICE_KEY_SPACE else 0.0
        assert em.get_option("gpu_layout") == want, (name, swap, gpu, idims)
        assert_sort_stage(em, ref, idims, data, dims, (name, swap, gpu))


def test_empty_training_set_under_both_builders(hip, monkeypatch):
    """No triple at all: both builders give the offsets of layout.hpp (all zero, the right lengths), no pair and degrees
    floored at one.  (The device builder used to launch grids of zero workgroups here, which HIP refuses.)"""
    data, dims = np.zeros((0, 3), dtype=np.int64), (3, 2, 2)
    ref = ir.sort_stage(data, *dims)
    outs = []
    for gpu in (0, 1):
        builder(monkeypatch, gpu)
        with hip.HipEM(data, 2, 2, *dims, swap_sides=0) as em:
            assert em.get_option("gpu_layout") == float(gpu)
            outs.append(assert_sort_stage(em, ref, dims, data, dims, ("empty", gpu)))
    assert not ir.differing(outs[0], outs[1], outs[0].keys())
    assert outs[1]["user_off"].tolist() == [0, 0, 0, 0] and outs[1]["item_off"].tolist() == [0, 0, 0] and outs[1]["pair_off"].tolist() == [0]


# ---- b. the default switch: the host below 100,000 triples, the device from there on ----
@pytest.mark.parametrize("name,want", [("switch-99999", 0.0), ("switch-100000", 1.0)])
def test_default_builder_switches_at_100000_triples(hip, name, want, monkeypatch):
    _, data, *dims = ic.case(name)
    ref, idims = reference(name, 0)
    builder(monkeypatch, None)
    with hip.HipEM(data, 2, 2, *dims, swap_sides=0) as em:
        assert em.get_option("gpu_layout") == want, name
        assert_sort_stage(em, ref, idims, data, dims, name)


# ---- c. everything create() derives from the sorts: host-built against device-built, all 19 arrays ----
def derived_tables():
    """(table, K, L): the two heavy cases of index_cases and one border table each of `segments`, `whole` and `grid`."""
    border = [("segments16-g4", 10, 10), ("whole-fits", 20, 20), ("grid-dense-r9", 10, 10)]
    assert all(n in bt.all_names() for n, _, _ in border)
    return [("n300k", 10, 10), ("dup", 10, 10)] + border


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("name,k,l", derived_tables(), ids=[t[0] for t in derived_tables()])
def test_everything_after_the_sorts_is_the_same_under_both_builders(hip, name, k, l, swap, monkeypatch):
    if name in ic.NAMES:
        _, data, *dims = ic.case(name)
        dims = tuple(dims)
    else:
        data, dims = bt.table(name).form(swap)      # (the designed sides are the INTERNAL ones on either layout)
    cols, idims = ic.internal(data, dims, swap)
    outs = []
    for gpu in (0, 1):
        builder(monkeypatch, gpu)
        with hip.HipEM(data, k, l, *dims, swap_sides=swap) as em:
            assert em.get_option("gpu_layout") == float(gpu)
            outs.append((em.index_arrays(), em.get_option("item_grid")))
    (host, host_grid), (dev, dev_grid) = outs
    assert len(host) == 19 and sorted(host) == sorted(dev)
    wrong = ir.differing(host, dev, sorted(host))
    assert not wrong, (name, swap, "device-built arrays that differ from the host-built ones", wrong)
    assert not ir.differing(dev, ir.sort_stage(cols, *idims)), (name, swap)
    assert host_grid == dev_grid == float(len(dev["item_grid"]) > 0)
    assert len(dev["lik_units"]) > 0 and len(dev["mv_chunks"]) > 0 and len(dev["chunks"]) > 0
    assert len(dev["mv_chunk_off"]) == idims[2] + 1 and dev["mv_chunk_off"][-1] == len(dev["mv_chunks"])
    if name.startswith(("segments", "whole")) or name == "n300k":
        assert len(dev["pair_items"]) > 0 and len(dev["user_items"]) > 0 and len(dev["user_splits"]) > 0, name
    if name.startswith("grid"):
        assert len(dev["item_grid"]) == idims[1] * idims[2], name


# ---- d. range cuts found on the device ----
@pytest.mark.parametrize("table,ranges", ic.RANGE_CASES, ids=[f"{t}-{r.replace(',', 'x')}" for t, r in ic.RANGE_CASES])
def test_range_cuts_of_both_builders_and_the_work_lists_they_give(hip, table, ranges, monkeypatch):
    data, dims = ic.range_table(table)
    rp, ru = (int(x) for x in ranges.split(","))
    monkeypatch.setenv("MMSBM_HIP_RANGES", ranges)
    options = ("items_pairs", "items_users", "splits_pairs", "splits_users")
    outs = []
    for gpu in (0, 1):
        builder(monkeypatch, gpu)
        with hip.HipEM(data, 10, 10, *dims, swap_sides=0) as em:
            assert em.get_option("gpu_layout") == float(gpu)
            assert em.get_option("ranges_pairs") == rp and em.get_option("ranges_users") == ru
            outs.append((em.index_arrays(), [em.get_option(o) for o in options]))
    (host, host_opt), (dev, dev_opt) = outs
    lists = ("pair_items", "user_items", "pair_splits", "user_splits")
    assert not ir.differing(host, dev, lists), (table, ranges, ir.differing(host, dev, lists))
    assert host_opt == dev_opt == [float(len(dev[nm])) for nm in lists]
    assert not ir.differing(dev, ir.sort_stage(data, *dims)), (table, ranges)
    n_pairs = len(dev["pair_item"])
    per_block = 256 // 4          # K = 10: rows of 12 doubles, groups of 4 lanes (shapes.hpp: group_code), 64 items per workgroup
    cut_p = ir.check_work_lists(dev["pair_off"], dev["pair_user"], dims[0], rp, dev["pair_items"], dev["pair_splits"], per_block=per_block)
    cut_u = ir.check_work_lists(dev["user_off"], dev["user_pair"], n_pairs, ru, dev["user_items"], dev["user_splits"], per_block=per_block)
    assert cut_p == dev_opt[2] and cut_u == dev_opt[3]
    assert cut_u > 0, (table, ranges)
    if table == "lognormal":
        assert cut_p > 0, ranges          # (the host builder alone cuts these pairs: test_index_reference_cpu.py)


# ---- e. one EM step on a wide key space ----
def test_one_step_on_a_key_space_of_2p27(hip, monkeypatch):
    """(I, R) = (2^21, 64): R beyond the largest the staged tests reach (33), the pair key 27 bits wide.  The builders
    agree bit for bit and the step agrees with the oracle."""
    _, data, *dims = ic.case("key-2p27")
    assert dims[1:] == [2 ** 21, 64]
    k, l = 6, 4
    d_u, d_i = orc.degrees(data, dims[0], dims[1])
    start = orc.init_params(5, *dims, k, l, d_u, d_i)
    want = orc.update_coefficients(data, *start)
    outs = []
    for gpu in (0, 1):
        builder(monkeypatch, gpu)
        with hip.HipEM(data, k, l, *dims, swap_sides=0) as em:
            assert em.get_option("gpu_layout") == float(gpu)
            em.set_params(*start)
            outs.append(em.update_coefficients())
    for a, b, w, nm in zip(outs[0], outs[1], want, ("n_theta", "n_eta", "n_pr")):
        assert np.array_equal(a, b), (nm, "host-built against device-built index")
        assert np.all(np.isfinite(b)), nm
        err = rel_err(b, w)
        print(f"key-2p27 {nm}: {err:.3e}")
        assert err < TOL_STEP, (nm, err)


# ---- g. the accessor itself ----
def test_accessor_count_query_fill_and_refusals(hip, monkeypatch):
    lib = hip._lib
    _, data, *dims = ic.case("n257")
    builder(monkeypatch, 1)
    with hip.HipEM(data, 2, 2, *dims, swap_sides=0) as em:
        for which, want in ((1, len(data)), (4, dims[0] + 1), (3, dims[2] + 1), (18, dims[2] + 1)):
            cnt = C.c_int64(-1)
            lib.call("mmsbm_hip_index_array", em._h, which, None, 0, C.byref(cnt))       # a count query
            assert cnt.value == want, which
            buf = np.full(want + 3, -7, dtype=np.int32)
            cnt = C.c_int64(-1)
            lib.call("mmsbm_hip_index_array", em._h, which, buf.ctypes.data_as(lib.c_i32p), buf.size, C.byref(cnt))
            assert cnt.value == want and np.all(buf[want:] == -7) and np.all(buf[:want] >= 0), which
            with pytest.raises(lib.HipLibraryError) as exc:                                 # a short capacity
                lib.call("mmsbm_hip_index_array", em._h, which, buf.ctypes.data_as(lib.c_i32p), want - 1, C.byref(cnt))
            assert exc.value.code == lib.E_INVALID, which
        for which in (-1, 19, 1000):
            with pytest.raises(lib.HipLibraryError) as exc:
                lib.call("mmsbm_hip_index_array", em._h, which, None, 0, C.byref(cnt))
            assert exc.value.code == lib.E_INVALID, which
        with pytest.raises(lib.HipLibraryError) as exc:
            lib.call("mmsbm_hip_index_array", em._h, 0, None, 0, None)
        assert exc.value.code == lib.E_INVALID
    with pytest.raises(lib.HipLibraryError) as exc:
        lib.call("mmsbm_hip_index_array", None, 0, None, 0, C.byref(cnt))
    assert exc.value.code == lib.E_INVALID


@pytest.mark.parametrize("gpu", [0, 1], ids=["host", "device"])
def test_accessor_between_two_iterate_calls_changes_no_parameter_bit(hip, gpu, monkeypatch):
    _, data, *dims = ic.case("n257")
    d_u, d_i = orc.degrees(data, dims[0], dims[1])
    start = orc.init_params(7, *dims, 3, 4, d_u, d_i)
    builder(monkeypatch, gpu)
    outs = []
    for read in (False, True):
        with hip.HipEM(data, 3, 4, *dims, swap_sides=0) as em:
            em.set_params(*start)
            em.iterate(2, sync=False)          # (the accessor waits for the context's stream itself)
            if read:
                assert len(em.index_arrays()) == 19
            em.iterate(2)
            outs.append(em.get_params() + (np.float64(em.likelihood()),))
    for a, b, nm in zip(outs[0], outs[1], ("theta", "eta", "pr", "likelihood")):
        assert np.array_equal(np.asarray(a), np.asarray(b)), nm


# ---- f. coverage ----
def compiled_layout_kernels(lib):
    """Every kernel of namespace mmsbm::gpu_layout in the library (rocPRIM's own kernels are not ours to launch)."""
    out = subprocess.run(["nm", lib], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in out.splitlines() if "__device_stub__" in ln})
    full = [d for d in kernel_coverage.demangle(syms) if "mmsbm::gpu_layout::" in d and "rocprim" not in d]
    return sorted({kernel_coverage.canon(d) for d in full})


def test_every_layout_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = compiled_layout_kernels(hip._lib.LIB_PATH)
    for k in LAYOUT_KERNELS:
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
