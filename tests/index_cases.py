"""Triple tables for the index itself (the sort stage of layout.hpp and of tu_layout.hip), shared by
test_index_reference_cpu.py and test_gpu_index.py.  No GPU and no library: numpy only.

A case is (name, data, U, I, R) with `data` an (N, 3) int64 array of (user, item, rating) rows in no particular order.
Every case plants the triple (U - 1, I - 1, R - 1) three times and (0, 0, 0) once, so the top and the bottom key of
every sort is present and the top one duplicated -- as far as the case's own design allows: a table of fewer than four
rows plants what fits (the top triple first), `all-pairs-distinct` plants each of the two once, and `absent-ends` plants
nothing (its point is that the first and last ids never occur).

Families:
  n*            N around the 256-thread workgroup of the kernels of tu_layout.hip, and 300,000 rows with Zipf users and one
                item of more than 40,000 rows (multi-block sorts, the per-item loop of item_degrees);
  one-pair-*    all rows in ONE (item, rating) pair; all-pairs-distinct; dup (60 x 40 x 3 ids, 50,000 rows); absent-ends
                (first, middle and last rating, the first and last 10 users and items never occur: lower_bounds at both ends);
  u* / i* / ri* the widths sort_stage computes (user_bits, item_bits, pk_bits) at 1, 2, 3, 2^k and 2^k + 1;
  key*          large (rating, item) key spaces R x I: 2^26 (the host builder's last counting sort), the first beyond it,
                2^27, 2^31 - 2^20 (the widest device sort: pk_bits 31, end bit 63), 2^31 exactly and 4.1e9 (both builders'
                host path: build_index falls back);
  switch-*      one random table cut to 99,999 and 100,000 rows: the default switch between the builders.
"""
import numpy as np

_CACHE = {}


def plant(data, dims, top=3, bottom=1):
    """The first rows become (U - 1, I - 1, R - 1) `top` times and (0, 0, 0) `bottom` times (what fits)."""
    n_u, n_i, n_r = dims
    rows = [[n_u - 1, n_i - 1, n_r - 1]] * top + [[0, 0, 0]] * bottom
    k = min(len(rows), len(data))
    data[:k] = rows[:k]
    return data


def uniform(rng, n, dims):
    return np.stack([rng.integers(0, d, n) for d in dims], axis=1).astype(np.int64)


def _n_rows(n):
    def make(rng):
        dims = (40, 30, 4) if n > 1 else (5, 4, 3)
        return plant(uniform(rng, n, dims), dims), dims
    return make


def _n300k(rng):
    n, dims = 300_000, (20_000, 3_000, 5)
    users = np.minimum(rng.zipf(1.3, n) - 1, dims[0] - 1)
    items = np.where(rng.random(n) < 0.15, 1234, rng.integers(0, dims[1], n))      # item 1234: ~45,000 rows
    data = np.stack([users, items, rng.integers(0, dims[2], n)], axis=1).astype(np.int64)
    assert np.count_nonzero(data[:, 1] == 1234) > 40_000
    return plant(data, dims), dims


def _one_pair(n_u):
    def make(rng):
        dims = (n_u, 1, 1)                        # one item, one rating: top and bottom triple are in the same pair
        return plant(uniform(rng, 300, dims), dims), dims
    return make


def _all_pairs_distinct(rng):
    dims = (90, 700, 5)
    keys = rng.choice(np.arange(1, dims[1] * dims[2] - 1), 1998, replace=False)
    keys = np.concatenate([[0, dims[1] * dims[2] - 1], keys])
    data = np.stack([rng.integers(0, dims[0], len(keys)), keys % dims[1], keys // dims[1]], axis=1).astype(np.int64)
    data[0, 0], data[1, 0] = 0, dims[0] - 1
    return data, dims


def _dup(rng):
    dims = (60, 40, 3)
    return plant(uniform(rng, 50_000, dims), dims), dims


def _absent_ends(rng):
    dims = (100, 80, 5)
    n = 3_000
    data = np.stack([rng.integers(10, 90, n), rng.integers(10, 70, n), rng.choice([1, 3], n)], axis=1).astype(np.int64)
    return data, dims


def _dims_case(dims, n=2_000):
    def make(rng):
        return plant(uniform(rng, n, dims), dims), dims
    return make


def _switch(n):
    def make(rng):
        dims = (5_000, 800, 5)
        full = plant(uniform(np.random.default_rng(99), 100_000, dims), dims)      # the same table for both cuts
        return np.ascontiguousarray(full[:n]), dims
    return make


_MAKERS = {}
for _n in (1, 255, 256, 257):
    _MAKERS[f"n{_n}"] = _n_rows(_n)
_MAKERS["n300k"] = _n300k
_MAKERS["one-pair-u1"] = _one_pair(1)
_MAKERS["one-pair-u50"] = _one_pair(50)
_MAKERS["all-pairs-distinct"] = _all_pairs_distinct
_MAKERS["dup"] = _dup
_MAKERS["absent-ends"] = _absent_ends
for _u in (1, 2, 3, 256, 257, 65_536, 65_537):
    _MAKERS[f"u{_u}"] = _dims_case((_u, 7, 3))
for _i in (1, 2, 3, 4_096, 4_097):
    _MAKERS[f"i{_i}"] = _dims_case((33, _i, 2))
# R x I = 1, 2, 2^8, 2^8 + 1, 2^16, 2^16 + 1 (257 and 65,537 are primes: one rating)
for _r, _i in ((1, 1), (2, 1), (4, 64), (1, 257), (16, 4_096), (1, 65_537)):
    _MAKERS[f"ri{_r * _i}"] = _dims_case((9, _i, _r))
KEY_SPACES = {"key-2p26": (2 ** 21, 32), "key-2p26-plus": (2 ** 21, 33), "key-2p27": (2 ** 21, 64),
              "key-2p31-minus": (2 ** 20, 2_047), "key-2p31": (2 ** 20, 2_048), "key-4e9": (2 ** 20, 4_000)}
for _name, (_i, _r) in KEY_SPACES.items():
    _MAKERS[_name] = _dims_case((300, _i, _r), n=5_000)
_MAKERS["switch-99999"] = _switch(99_999)
_MAKERS["switch-100000"] = _switch(100_000)

NAMES = list(_MAKERS)
SWITCH = ("switch-99999", "switch-100000")
SORT_NAMES = [n for n in NAMES if n not in SWITCH]      # (the switch tables: the default builder, a test of their own)


def case(name):
    """(name, data, U, I, R), built once (data read-only)."""
    if name not in _CACHE:
        rng = np.random.default_rng([NAMES.index(name), 20])
        data, dims = _MAKERS[name](rng)
        data = np.ascontiguousarray(data, dtype=np.int64)
        for j in range(3):
            assert data[:, j].min() >= 0 and data[:, j].max() < dims[j], (name, j)
        data.setflags(write=False)
        _CACHE[name] = (name, data) + tuple(int(d) for d in dims)
    return _CACHE[name]


# ---- the tables of the range-cut tests (XCD-local work lists, MMSBM_HIP_RANGES) ----
RANGE_TABLES = ("lognormal", "five-users", "one-pair")
# (table, "pairs,users" range counts): counts that do not divide the table's rows (700 users, ~1,300 pairs), more ranges
# than rows, a table of one row
RANGE_CASES = [("lognormal", "8,16"), ("lognormal", "7,7"), ("lognormal", "3,5"), ("lognormal", "512,512"),
               ("five-users", "8,8"), ("one-pair", "2,2")]


def range_table(name):
    """(data, (U, I, R)).  lognormal: 120,000 rows, log-normal user degrees over 700 users of which users 0, 350 and 699
    never occur and user 1 holds a single row; five-users: 5 users of ~4,000 rows; one-pair: one item, one rating."""
    key = ("range", name)
    if key not in _CACHE:
        rng = np.random.default_rng([RANGE_TABLES.index(name), 21])
        if name == "lognormal":
            n, dims = 120_000, (700, 260, 5)
            users = 2 + np.minimum((rng.lognormal(0.0, 1.0, n) * 60).astype(np.int64), dims[0] - 5)      # 2 .. 697
            users[users >= 350] += 1                                                                      # 350 free, 698 the last
            data = np.stack([users, rng.integers(0, dims[1], n), rng.integers(0, dims[2], n)], axis=1).astype(np.int64)
            data[0] = (1, 5, 2)
        elif name == "five-users":
            n, dims = 20_000, (5, 40, 3)
            data = uniform(rng, n, dims)
        else:
            n, dims = 5_000, (50, 1, 1)
            data = uniform(rng, n, dims)
        data = np.ascontiguousarray(data)
        data.setflags(write=False)
        _CACHE[key] = (data, dims)
    return _CACHE[key]


def key_space(name):
    _, _, _, n_i, n_r = case(name)
    return n_i * n_r


def internal(data, dims, swap):
    """The id columns and dims a context of swap_sides = `swap` sorts: its "users" are the caller's items when swapped."""
    if not swap:
        return data, dims
    return np.ascontiguousarray(data[:, [1, 0, 2]]), (dims[1], dims[0], dims[2])
