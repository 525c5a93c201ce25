"""The request checks of the C ABI as a caller meets them -- which request is refused, with which code and text, which
fault is reported first, and what an accepted empty request returns: the cases of tests/test_gpu_abi_requests.py and the
recorder of their expected table.

Over the data of pair_plan_cases.make_data() at shape (3, 2), parameters from init_params(31), one context per session
kind.  A row is [label, code or exception class name, message]:

  a refusal of the library    [label, status code, the text of mmsbm_hip_last_error];
  a refusal of core.py        [label, "ValueError", its text];
  an accepted request         [label, 0, the shapes and dtypes of what the method returned ("" for a raw call)].

A request goes through the HipEM method where the method can express it.  Where it cannot -- a null pointer, a negative
count, n_cand out of range, assortment users out of order -- the symbol is called directly (``raw``): the arguments are
laid out by the parameter names of include/mmsbm_hip.h, DEFAULTS gives a small valid request, the keywords of the call
replace single arguments, and every output pointer not named gets a buffer larger than any request here could fill.
Accepted requests are empty ones only, so nothing is launched beyond init_params, the adds and those.

Left out, because this shape cannot reach them:
  * the refused cap of allocate / assign (a cap above 1,024 and below the users of the request: the data has 64 users);
  * "more than 2^31 - 1 items in the catalogue" of recommend_add_items, "K = ... is beyond" of explain_begin / loo_begin /
    fold_in, "n_obs must be below 2^31" of loo_begin, "too many rows" of predict_begin / heldout_begin: sizes of the
    context or of n_rows that tiny data does not have;
  * the entries of tests/host_layer_cases.py (no session, before any add, an id at row 1, n = 0 / 1025 of the three plain
    top-N entries): that table holds them.

The table a commit gives is recorded with

    python tests/abi_request_cases.py --out tests/gpu_abi_requests_parent.json [--tree DIR]

(--tree: the checkout whose mmsbm_amd and include/mmsbm_hip.h are used, e.g. a build of the parent commit; this file's
own by default).  The committed table is the one of the commit BEFORE the request checks moved to csrc/abi_request.hpp:
the refactor must not move an entry.
"""
import argparse
import ctypes
import json
import os
import re
import sys

import numpy as np

K, L = 3, 2
NAN, INF = float("nan"), float("inf")
BIG = 1 << 16                       # entries of an output buffer of a raw call
DTYPES = {"int32_t": np.int32, "int64_t": np.int64, "double": np.float64, "uint64_t": np.uint64, "uint8_t": np.uint8}
STATE = np.array([1, 2, 3, 5], dtype=np.uint64)         # the four PCG64 words of a raw call ...
WORDS = (ctypes.c_uint64 * 4)(1, 2, 3, 5)                # ... and as a HipEM method takes them


def make_data():
    from pair_plan_cases import make_data as pair_plan_data
    return pair_plan_data()


def prototypes(tree):
    """{symbol without "mmsbm_hip_": [(parameter name, base type, is a pointer, is const), ...]} of the header."""
    text = open(os.path.join(tree, "include", "mmsbm_hip.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for name, params in re.findall(r"\bmmsbm_hip_([a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        plist = []
        for p in " ".join(params.split()).split(","):
            m = re.match(r"\s*(const\s+)?(\w+)\s*(\*?)\s*(\w+)?\s*(\[\d*\])?\s*$", p)
            if m and m.group(4):
                plist.append((m.group(4), m.group(2), bool(m.group(3) or m.group(5)), bool(m.group(1))))
        out[name] = plist
    return out


# a small valid request, by parameter name; an output pointer not listed is a buffer of BIG entries
DEFAULTS = dict(
    n_users=2, users=[0, 1], n=2, n_cand=0, cand_items=None, excl_offsets=None, excl_items=None,
    theta=np.full((1, 2, K), 1.0 / K), seen_offsets=None, seen_items=None, seen_users=None,
    n_cats=2, cat_offsets=[0, 2, 4], cat_items=[0, 1, 2, 3], cat_caps=[1, 1], depth=1, min_items=1, n_shelves=1,
    per_shelf=1, temperature=0.5, pcg64_state=STATE, list_offsets=[0, 1, 2], list_items=[3, 4], offsets=[0, 1, 2],
    items=[3, 4], members=[0, 1], n_groups=2, mode=0, bar=0.0, level=0.0, n_given=0, given_items=None, c=1, risk=0.0,
    pool=4, trade_off=0.5, m=2, caps=np.ones(48, dtype=np.int32), max_rounds=3, reserve=0.0, epsilon=0.01,
    min_score=0.5, capacity=0, n_items=2, n_pairs=2, a=[0, 1], b=[1, 2], n_rows=2, ids=[0, 1], rows=[0, 1],
    user_flags=None, item_flags=None, exclude_train=1, n_new=1, eta=np.full((1, 1, L), 1.0 / L))
ENTRY_DEFAULTS = {"recommend_rank": dict(cand_items=[3, 4])}


def describe(res):
    """The shapes and dtypes of what a method returned."""
    if isinstance(res, np.ndarray):
        return f"{res.dtype}{list(res.shape)}"
    if isinstance(res, dict):
        return "{" + ", ".join(f"{k}: {describe(v)}" for k, v in res.items()) + "}"
    if isinstance(res, (tuple, list)):
        return "(" + ", ".join(describe(v) for v in res) + ")"
    return "None" if res is None else type(res).__name__


class Recorder:
    def __init__(self, pkg, protos):
        self.pkg, self.protos, self.rows = pkg, protos, []

    def note(self, label, fn, *args, **kwargs):
        """A request through a HipEM method."""
        try:
            res = fn(*args, **kwargs)
        except self.pkg._lib.HipLibraryError as exc:
            row = [exc.code, exc.message]
        except ValueError as exc:
            row = ["ValueError", str(exc)]
        else:
            row = [0, describe(res)]
        self.rows.append([label, *row])

    def raw(self, label, em, symbol, **given):
        """A request through the symbol itself: DEFAULTS with ``given`` in place of single arguments."""
        lib = self.pkg._lib.load()
        fn = getattr(lib, "mmsbm_hip_" + symbol)
        args, keep = [em._h], []
        defaults = dict(DEFAULTS, **ENTRY_DEFAULTS.get(symbol, {}))
        for (name, base, pointer, const), ctype in zip(self.protos[symbol][1:], fn.argtypes[1:]):
            if name in given:
                value = given[name]
            elif pointer and not const:
                value = np.zeros(BIG, dtype=DTYPES[base])
            else:
                value = defaults[name]
            if pointer and value is not None:
                arr = np.ascontiguousarray(value, dtype=DTYPES[base])
                keep.append(arr)
                value = arr.ctypes.data_as(ctype)
            args.append(value)
        assert not set(given) - {p[0] for p in self.protos[symbol]}, (symbol, given)
        code = fn(*args)
        self.rows.append([label, code, lib.mmsbm_hip_last_error().decode() if code else ""])


BAD_CANDIDATES = lambda n_i: [("candidate out of range at entry 1", [0, n_i]), ("candidates descending", [3, 2]),   # noqa: E731
                              ("candidate repeated", [2, 2]), ("n_cand = items + 1", np.arange(n_i + 1))]
BAD_CSR = lambda top: [("offsets[0] = 1", ([1, 1, 1], [0])), ("offsets decrease at row 1", ([0, 1, 0], [])),        # noqa: E731
                       ("value out of range", ([0, 1, 2], [0, top]))]
CATS = ([0, 2, 4], [0, 1, 2, 3])
THETA = np.full((1, 2, K), 1.0 / K)
BAD_THETA = [("theta of rank 2", np.zeros((2, K))), ("theta last axis", np.zeros((1, 2, K + 1))),
             ("theta of two blocks", np.full((2, 2, K), 1.0 / K))]


def run_prefix(rec, em, inf, ex, dims):
    """The users / candidate subset / exclusion prefix, entry by entry."""
    n_u, n_i, _ = dims

    def lists(u):
        return np.arange(len(u) + 1), np.arange(len(u)) + 3

    # entry: (context, has n, has a subset, has an exclusion list, call(users, n, candidates, exclude))
    entries = {
        "recommend_query_within": (em, 1, 1, 1, lambda u, n, c, e: em.recommend_query_within(u, n, c, e)),
        "recommend_query_explore": (em, 1, 1, 1, lambda u, n, c, e: em.recommend_query_explore(u, n, 0.5, WORDS, c, e)),
        "recommend_list_propensity": (em, 0, 1, 1, lambda u, n, c, e: em.recommend_list_propensity(u, lists(u), 0.5, c, e)),
        "recommend_query_quota": (em, 1, 1, 1, lambda u, n, c, e: em.recommend_query_quota(u, n, *CATS, [1, 1], c, e)),
        "recommend_query_shelves": (em, 0, 1, 1, lambda u, n, c, e: em.recommend_query_shelves(u, *CATS, 1, 1, 1, 1, c, e)),
        "recommend_diverse": (em, 1, 1, 1, lambda u, n, c, e: em.recommend_diverse(u, n, 4, 0.5, c, e)),
        "recommend_query_ensemble": (em, 1, 1, 1, lambda u, n, c, e: em.recommend_query_ensemble(u, n, "min", 0.0, c, e)),
        "inform_query": (inf, 1, 1, 1, lambda u, n, c, e: inf.inform_query(u, n, c, e)),
        "recommend_rank": (em, 1, 0, 0, lambda u, n, c, e: em.recommend_rank(u, *lists(u), n)),
        "explain_query": (ex, 1, 0, 0, lambda u, n, c, e: ex.explain_query(u, *lists(u), n)),
        "recommend_positions": (em, 0, 0, 0, lambda u, n, c, e: em.recommend_positions(u, *lists(u))),
    }
    for name, (ctx, has_n, has_subset, has_excl, call) in entries.items():
        if has_n:
            for n in (0, 1025):
                rec.note(f"{name}: n = {n}", call, [0, 1], n, None, None)
        rec.note(f"{name}: user id = n_users at row 1", call, [0, n_u], 2, None, None)
        rec.note(f"{name}: user id = -1 at row 1", call, [0, -1], 2, None, None)
        rec.raw(f"{name}: n_users = -1", ctx, name, n_users=-1)
        rec.raw(f"{name}: null users", ctx, name, users=None)
        if has_subset:
            for what, cand in BAD_CANDIDATES(n_i):
                rec.note(f"{name}: {what}", call, [0, 1], 2, cand, None)
            rec.raw(f"{name}: n_cand = -1", ctx, name, n_cand=-1, cand_items=[0, 1])
            rec.raw(f"{name}: no users, n_cand = -1 without candidates", ctx, name, n_users=0, users=None, n_cand=-1)
        if has_excl:
            for what, excl in BAD_CSR(n_i):
                rec.note(f"{name}: exclusion {what}", call, [0, 1], 2, None, excl)
            rec.raw(f"{name}: exclusion total 2^31", ctx, name, excl_offsets=[0, 0, 2 ** 31])
            rec.raw(f"{name}: exclusion without values", ctx, name, excl_offsets=[0, 1, 2])
            rec.raw(f"{name}: no users, exclusion offsets given", ctx, name, n_users=0, users=None, excl_offsets=[0])
        rec.note(f"{name}: no users", call, [], 2, None, None)
        outs = {p[0]: None for p in rec.protos[name] if p[2] and not p[3]}
        ins = {p[0]: None for p in rec.protos[name] if p[2] and p[3] and p[0] not in ("pcg64_state", "cat_offsets",
                                                                                     "cat_items", "cat_caps")}
        rec.raw(f"{name}: no users, null arrays", ctx, name, n_users=0, **ins, **outs)

    # the entries that take the candidates or the queried items as a CSR of their own
    for name, ctx, val in (("recommend_rank", em, "cand_items"), ("explain_query", ex, "items"),
                           ("recommend_positions", em, "items")):
        call = {"recommend_rank": lambda o, v: em.recommend_rank([0, 1], o, v, 2),
                "explain_query": lambda o, v: ex.explain_query([0, 1], o, v, 2),
                "recommend_positions": lambda o, v: em.recommend_positions([0, 1], o, v)}[name]
        for what, (off, values) in BAD_CSR(n_i):
            rec.note(f"{name}: {what}", call, off, values)
        rec.note(f"{name}: offsets of the wrong length", call, [0, 1], [3])
        rec.note(f"{name}: offsets end elsewhere", call, [0, 1, 3], [3, 4])
        rec.raw(f"{name}: null offsets", ctx, name, offsets=None)
        rec.raw(f"{name}: total 2^31", ctx, name, offsets=[0, 0, 2 ** 31], **{val: None})
        rec.raw(f"{name}: without values", ctx, name, **{val: None})
    rec.note("recommend_rank: not ascending in the second row", em.recommend_rank, [0, 1], [0, 2, 4], [0, 1, 3, 2], 2)
    rec.note("recommend_rank: repeated in the second row", em.recommend_rank, [0, 1], [0, 2, 4], [0, 1, 3, 3], 2)
    rec.raw("recommend_positions: null positions", em, "recommend_positions", positions=None)
    rec.raw("explain_query: null hist_items", ex, "explain_query", hist_items=None)
    rec.raw("explain_query: 2^31 entries", ex, "explain_query", offsets=[0, 0, 2 ** 21],
            items=np.zeros(2 ** 21, dtype=np.int32), n=1024)


def run_theta(rec, em, inf, dims):
    """The theta-rows prefix."""
    n_u, n_i, _ = dims
    entries = {
        "recommend_query_theta": (em, 1, lambda t, n, s, c: em.recommend_query_theta(t, n, s, None)),
        "recommend_query_theta_within": (em, 1, lambda t, n, s, c: em.recommend_query_theta(
            t, n, s, np.arange(n_i) if c is None else c)),
        "recommend_query_theta_quota": (em, 1, lambda t, n, s, c: em.recommend_query_theta_quota(t, n, *CATS, [1, 1], s, c)),
        "recommend_query_theta_shelves": (em, 0, lambda t, n, s, c: em.recommend_query_theta_shelves(
            t, *CATS, 1, 1, 1, 1, s, c)),
        "inform_query_theta": (inf, 1, lambda t, n, s, c: inf.inform_query_theta(t, n, s, c)),
    }
    for name, (ctx, has_n, call) in entries.items():
        for what, theta in BAD_THETA:
            rec.note(f"{name}: {what}", call, theta, 2, None, None)
        if has_n:
            for n in (0, 1025):
                rec.note(f"{name}: n = {n}", call, THETA, n, None, None)
        for what, seen in BAD_CSR(n_i):
            rec.note(f"{name}: seen {what}", call, THETA, 2, seen, None)
        rec.raw(f"{name}: seen total 2^31", ctx, name, seen_offsets=[0, 0, 2 ** 31])
        rec.raw(f"{name}: seen without values", ctx, name, seen_offsets=[0, 1, 2])
        if name != "recommend_query_theta":
            for what, cand in BAD_CANDIDATES(n_i):
                rec.note(f"{name}: {what}", call, THETA, 2, None, cand)
            rec.raw(f"{name}: n_cand = -1", ctx, name, n_cand=-1, cand_items=[0, 1])
        rec.raw(f"{name}: n_users = -1", ctx, name, n_users=-1)
        rec.raw(f"{name}: null theta", ctx, name, theta=None)
        rec.note(f"{name}: no users", call, np.zeros((1, 0, K)), 2, None, None)
        outs = {p[0]: None for p in rec.protos[name] if p[2] and not p[3]}
        rec.raw(f"{name}: no users, null arrays", ctx, name, n_users=0, theta=None, **outs)
    bad = THETA.copy()
    bad[0, 1, 1] = -0.25
    rec.note("inform_query_theta: a negative theta entry", inf.inform_query_theta, bad, 2)
    bad[0, 1, 1] = NAN
    rec.note("inform_query_theta: a NaN theta entry", inf.inform_query_theta, bad, 2)
    rec.note("inform_query_theta: a NaN theta entry and a bad candidate", inf.inform_query_theta, bad, 2, None, [3, 2])
    rec.note("recommend_query_theta_within: a bad candidate and a bad seen list", em.recommend_query_theta, THETA, 2,
             ([1, 1, 1], [0]), [3, 2])


def run_categories(rec, em, dims):
    """The categories of the quota entries and the ask of the shelves entries."""
    n_u, n_i, _ = dims
    bad_cats = [("category not ascending", ([0, 2, 4], [1, 0, 2, 3])), ("item in two categories", ([0, 2, 4], [0, 1, 1, 2])),
                ("cat_offsets[0] = 1", ([1, 2, 4], [0, 1, 2, 3])), ("cat_offsets decrease", ([0, 2, 1], [0])),
                ("category item out of range", ([0, 2, 4], [0, 1, 2, n_i]))]
    for name, call in (("recommend_query_quota", lambda cats, caps: em.recommend_query_quota([0, 1], 2, *cats, caps)),
                       ("recommend_query_theta_quota", lambda cats, caps: em.recommend_query_theta_quota(THETA, 2, *cats, caps))):
        rec.note(f"{name}: a negative cap", call, CATS, [1, -1])
        for what, cats in bad_cats:
            rec.note(f"{name}: {what}", call, cats, [1, 1])
        rec.note(f"{name}: category offsets of the wrong length", call, ([0, 4], [0, 1, 2, 3]), [1, 1])
        rec.raw(f"{name}: n_cats = -1", em, name, n_cats=-1)
        rec.raw(f"{name}: null cat_offsets", em, name, cat_offsets=None)
        rec.raw(f"{name}: null cat_caps", em, name, cat_caps=None)
        rec.raw(f"{name}: null cat_items", em, name, cat_items=None)
    rec.note("recommend_query_quota: no users, no categories", em.recommend_query_quota, [], 2, [0], [], [])
    rec.note("recommend_query_theta_quota: no users, no categories", em.recommend_query_theta_quota, np.zeros((1, 0, K)), 2,
             [0], [], [])
    ask = dict(depth=1, min_items=1, n_shelves=1, per_shelf=1)
    for name, call in (("recommend_query_shelves", lambda cats, a: em.recommend_query_shelves([0, 1], *cats, **a)),
                       ("recommend_query_theta_shelves", lambda cats, a: em.recommend_query_theta_shelves(THETA, *cats, **a))):
        for what, cats in bad_cats:
            rec.note(f"{name}: {what}", call, cats, ask)
        for key, value in (("depth", 0), ("min_items", 0), ("n_shelves", 0), ("per_shelf", -1), ("depth", 1025),
                           ("n_shelves", 1025), ("per_shelf", 1025)):
            rec.note(f"{name}: {key} = {value}", call, CATS, dict(ask, **{key: value}))
        rec.note(f"{name}: depth = 0 and a category not ascending", call, bad_cats[0][1], dict(ask, depth=0))
        rec.raw(f"{name}: n_cats = -1", em, name, n_cats=-1)
        rec.raw(f"{name}: n_cats = 2^31", em, name, n_cats=2 ** 31)
        rec.raw(f"{name}: null cat_offsets", em, name, cat_offsets=None)
        rec.raw(f"{name}: null shelf_cats", em, name, shelf_cats=None)
        rec.raw(f"{name}: null items at per_shelf 1", em, name, items=None)
    rec.note("recommend_query_shelves: depth = 0 and a bad user id", em.recommend_query_shelves, [0, n_u], *CATS, 0, 1, 1, 1)
    rec.note("recommend_query_quota: a bad exclusion and a bad category", em.recommend_query_quota, [0, 1], 2,
             [0, 2, 4], [1, 0, 2, 3], [1, 1], None, ([1, 1, 1], [0]))


def run_explore(rec, em, bare, dims):
    n_u, n_i, _ = dims
    lists = ([0, 1, 2], [3, 4])
    # the session's weights are 0, 1, 2: the floor is 2 / 700 = 0.002857...
    for t in (0.0, NAN, INF, -1.0, 0.002857):
        rec.note(f"recommend_query_explore: temperature {t}", em.recommend_query_explore, [0, 1], 2, t, WORDS)
        rec.note(f"recommend_list_propensity: temperature {t}", em.recommend_list_propensity, [0, 1], lists, t)
    rec.note("recommend_query_explore: temperature 0 and n = 0", em.recommend_query_explore, [0, 1], 0, 0.0, WORDS)
    rec.note("recommend_query_explore: temperature 0 and a bad user id", em.recommend_query_explore, [0, n_u], 2, 0.0, WORDS)
    rec.note("recommend_query_explore: null state", em.recommend_query_explore, [0, 1], 2, 0.5, None)
    rec.raw("recommend_list_propensity: temperature 0 and null users", em, "recommend_list_propensity", temperature=0.0,
            users=None)
    rec.note("recommend_list_propensity: an item twice in a list", em.recommend_list_propensity, [0, 1], ([0, 2, 2], [3, 3]), 0.5)
    rec.note("recommend_list_propensity: a list of 1025 items", em.recommend_list_propensity, [0, 1],
             ([0, 1025, 1025], np.arange(1025) % n_i), 0.5)
    for what, lst in BAD_CSR(n_i):
        rec.note(f"recommend_list_propensity: list {what}", em.recommend_list_propensity, [0, 1], lst, 0.5)
    rec.raw("recommend_list_propensity: null list_offsets", em, "recommend_list_propensity", list_offsets=None)
    rec.raw("recommend_list_propensity: null propensity", em, "recommend_list_propensity", propensity=None)
    rec.note("explore_noise: a negative user id", bare.explore_noise, WORDS, [0, -1], [0, 1])
    rec.note("explore_noise: a negative item id", bare.explore_noise, WORDS, [0, 1], [-1, 1])
    rec.note("explore_noise: null state", bare.explore_noise, None, [0, 1], [0, 1])
    rec.note("explore_noise: two lengths", bare.explore_noise, WORDS, [0, 1], [0])
    rec.note("explore_noise: no pairs", bare.explore_noise, WORDS, [], [])
    rec.raw("explore_noise: n_pairs = -1", bare, "explore_noise", n_pairs=-1)
    rec.raw("explore_noise: null users", bare, "explore_noise", users=None)
    rec.raw("explore_noise: no pairs, null arrays", bare, "explore_noise", n_pairs=0, users=None, items=None, r=None, g=None)


def run_user_sets(rec, em, dims):
    n_u, n_i, _ = dims
    beyond = {"recommend_top_pairs": 1025, "recommend_top_pairs_bulk": 2 ** 26 + 1, "recommend_pair_bar": 2 ** 26 + 1}
    for name, first in beyond.items():
        call = getattr(em, name)
        rec.note(f"{name}: a repeated id", call, 2, [1, 0, 1])
        rec.note(f"{name}: user id = n_users at row 1", call, 2, [0, n_u])
        rec.note(f"{name}: m = 0", call, 0, [0, 1])
        rec.raw(f"{name}: m = {first}", em, name, m=first)
        rec.raw(f"{name}: m = 0 and a repeated id", em, name, m=0, users=[1, 1])
        rec.raw(f"{name}: n_users = -1", em, name, n_users=-1)
        rec.raw(f"{name}: null counts or count", em, name, **{"count" if name == "recommend_top_pairs" else "counts": None})
        rec.note(f"{name}: no users", call, 2, [])
    caps = np.ones(n_i, dtype=np.int32)
    for name, call in (("recommend_allocate", lambda u, **kw: em.recommend_allocate(u, kw.pop("n", 2), caps, **kw)),
                       ("recommend_assign", lambda u, **kw: em.recommend_assign(
                           u, caps, kw.pop("reserve", 0.0), kw.pop("epsilon", 0.01), **kw))):
        rec.note(f"{name}: a user asked twice", call, [1, 0, 1])
        rec.note(f"{name}: user id = n_users at row 1", call, [0, n_u])
        rec.note(f"{name}: max_rounds = 0", call, [0, 1], max_rounds=0)
        rec.note(f"{name}: max_rounds = 0 and a user asked twice", call, [1, 1], max_rounds=0)
        rec.raw(f"{name}: users left out, n_users = 3", em, name, users=None, n_users=3)
        rec.raw(f"{name}: n_users = -1", em, name, n_users=-1)
        rec.raw(f"{name}: null caps", em, name, caps=None)
        rec.raw(f"{name}: null rounds", em, name, rounds=None)
        rec.note(f"{name}: no users", call, [])
    for n in (0, 1025):
        rec.note(f"recommend_allocate: n = {n}", em.recommend_allocate, [0, 1], n, caps)
    # the largest minus the smallest weight is 2: epsilon must be at least 2^-39 = 1.8e-12
    for eps in (0.0, NAN, INF, -1.0, 1e-12):
        rec.note(f"recommend_assign: epsilon = {eps}", em.recommend_assign, [0, 1], caps, 0.0, eps)
    for reserve in (NAN, INF):
        rec.note(f"recommend_assign: reserve = {reserve}", em.recommend_assign, [0, 1], caps, reserve, 0.01)
    rec.note("recommend_assign: epsilon = 0 and max_rounds = 0", em.recommend_assign, [0, 1], caps, 0.0, 0.0, 0)
    rec.note("recommend_assign: caps too short", em.recommend_assign, [0, 1], caps[:-1], 0.0, 0.01)
    rec.raw("recommend_assign: null price", em, "recommend_assign", price=None)


def run_groups_assortment_ensemble(rec, em, dims):
    n_u, n_i, _ = dims
    g = em.recommend_query_groups
    rec.note("recommend_query_groups: an unknown mode", g, [0, 1, 2], [0, 1], 2, 7)
    rec.note("recommend_query_groups: a NaN bar with count", g, [0, 1, 2], [0, 1], 2, "count", NAN)
    rec.note("recommend_query_groups: no groups, a NaN bar with min", g, [0], [], 2, "min", NAN)
    rec.note("recommend_query_groups: a member repeated in a group", g, [0, 1, 3], [0, 1, 1], 2, "min")
    for what, (off, members) in BAD_CSR(n_u):
        rec.note(f"recommend_query_groups: {what}", g, off, members, 2, "min")
    for n in (0, 1025):
        rec.note(f"recommend_query_groups: n = {n}", g, [0, 1, 2], [0, 1], n, "min")
    for what, cand in BAD_CANDIDATES(n_i):
        rec.note(f"recommend_query_groups: {what}", g, [0, 1, 2], [0, 1], 2, "min", 0.0, cand)
    rec.note("recommend_query_groups: offsets of rank 2", g, [[0, 1]], [0], 2, "min")
    rec.note("recommend_query_groups: offsets end elsewhere", g, [0, 1, 3], [0, 1], 2, "min")
    rec.note("recommend_query_groups: an unknown mode and n = 0", g, [0, 1, 2], [0, 1], 0, 7)
    rec.note("recommend_query_groups: a repeated member and a bad candidate", g, [0, 2], [1, 1], 2, "min", 0.0, [3, 2])
    rec.raw("recommend_query_groups: n_groups = -1", em, "recommend_query_groups", n_groups=-1)
    rec.raw("recommend_query_groups: null offsets", em, "recommend_query_groups", offsets=None)
    rec.raw("recommend_query_groups: n_cand = -1", em, "recommend_query_groups", n_cand=-1, cand_items=[0, 1])
    rec.note("recommend_query_groups: no groups", g, [0], [], 2, "min")
    rec.raw("recommend_query_groups: no groups, null arrays", em, "recommend_query_groups", n_groups=0, offsets=None,
            members=None, items=None, scores=None, counts=None)

    a = em.recommend_assortment
    rec.note("recommend_assortment: an unknown mode", a, [0, 1], 1, 5, 0.0)
    rec.note("recommend_assortment: a NaN floor", a, [0, 1], 1, "best_score", NAN)
    rec.note("recommend_assortment: a NaN bar", a, [0, 1], 1, "reach", NAN)
    rec.note("recommend_assortment: c = -1", a, [0, 1], -1, "reach", 0.5)
    rec.note("recommend_assortment: c = 1025", a, [0, 1], 1025, "reach", 0.5)
    rec.note("recommend_assortment: user id = n_users", a, [0, n_u], 1, "reach", 0.5)
    rec.note("recommend_assortment: a given item out of range", a, [0, 1], 1, "reach", 0.5, [0, n_i])
    for what, cand in BAD_CANDIDATES(n_i):
        rec.note(f"recommend_assortment: {what}", a, [0, 1], 1, "reach", 0.5, None, cand)
    rec.note("recommend_assortment: an unknown mode and c = -1", a, [0, 1], -1, 5, 0.0)
    rec.raw("recommend_assortment: n_given = -1", em, "recommend_assortment", n_given=-1)
    rec.raw("recommend_assortment: n_users = -1", em, "recommend_assortment", n_users=-1)
    rec.raw("recommend_assortment: users not ascending", em, "recommend_assortment", users=[1, 0])
    rec.raw("recommend_assortment: users repeated", em, "recommend_assortment", users=[1, 1])
    rec.raw("recommend_assortment: users not ascending and a bad candidate", em, "recommend_assortment", users=[1, 0],
            n_cand=2, cand_items=[3, 2])
    rec.raw("recommend_assortment: null count", em, "recommend_assortment", count=None)
    rec.raw("recommend_assortment: null given_items", em, "recommend_assortment", n_given=1)
    rec.raw("recommend_assortment: n_cand = -1", em, "recommend_assortment", n_cand=-1, cand_items=[0, 1])
    rec.note("recommend_assortment: no users, c = 0", a, [], 0, "reach", 0.5)

    e = em.recommend_query_ensemble
    rec.note("recommend_query_ensemble: an unknown mode", e, [0, 1], 2, 9)
    rec.note("recommend_query_ensemble: a NaN risk with lcb", e, [0, 1], 2, "lcb", NAN)
    rec.note("recommend_query_ensemble: no users, a NaN risk with min", e, [], 2, "min", NAN)
    rec.note("recommend_query_ensemble: an unknown mode and n = 0", e, [0, 1], 0, 9)


def run_pairs_items(rec, em, sim_items, sim_users, dims):
    n_u, n_i, _ = dims
    s = em.recommend_pair_spread
    rec.note("recommend_pair_spread: user id out of range", s, [0, n_u], [0, 1])
    rec.note("recommend_pair_spread: item id out of range", s, [0, 1], [0, n_i])
    rec.note("recommend_pair_spread: both out of range at row 1", s, [0, n_u], [0, n_i])
    rec.note("recommend_pair_spread: two lengths", s, [0, 1], [0])
    rec.note("recommend_pair_spread: no pairs", s, [], [], True)
    rec.raw("recommend_pair_spread: n_pairs = -1", em, "recommend_pair_spread", n_pairs=-1)
    rec.raw("recommend_pair_spread: null stats", em, "recommend_pair_spread", stats=None)
    for sim, top, side in ((sim_items, n_i, "items"), (sim_users, n_u, "users")):
        rec.note(f"similar_pairs, {side}: a out of range", sim.similar_pairs, [0, top], [0, 1])
        rec.note(f"similar_pairs, {side}: b out of range", sim.similar_pairs, [0, 1], [0, -1])
        rec.note(f"similar_pairs, {side}: no pairs", sim.similar_pairs, [], [])
        rec.raw(f"similar_query, {side}: n_rows = -1", sim, "similar_query", n_rows=-1)
        rec.raw(f"similar_query, {side}: null ids", sim, "similar_query", ids=None)
        rec.note(f"similar_query, {side}: no rows", sim.similar_query, [], 2)
    rec.note("similar_pairs: two lengths", sim_items.similar_pairs, [0, 1], [0])
    rec.raw("similar_pairs: n_pairs = -1", sim_items, "similar_pairs", n_pairs=-1)
    rec.raw("similar_pairs: null distance", sim_items, "similar_pairs", distance=None)
    rec.note("similar_begin: side 2", sim_items.similar_begin, 2)

    rec.note("recommend_audience: a NaN min_score", em.recommend_audience, [0, 1], NAN)
    rec.note("recommend_audience: item id out of range", em.recommend_audience, [0, n_i], 0.5)
    rec.note("recommend_audience: no items", em.recommend_audience, [], 0.5)
    rec.raw("recommend_audience: a negative capacity", em, "recommend_audience", capacity=-1)
    rec.raw("recommend_audience: n_items = -1", em, "recommend_audience", n_items=-1)
    rec.raw("recommend_audience: null offsets", em, "recommend_audience", offsets=None)
    rec.raw("recommend_audience: users without scores", em, "recommend_audience", scores=None)
    rec.raw("recommend_query_items: n_items = -1", em, "recommend_query_items", n_items=-1)
    rec.raw("recommend_query_items: null items", em, "recommend_query_items", items=None)
    rec.note("recommend_query_items: no items", em.recommend_query_items, [], 2)
    rec.raw("recommend_query: n_users = -1", em, "recommend_query", n_users=-1)
    rec.raw("recommend_query: null users", em, "recommend_query", users=None)
    rec.raw("recommend_query: n_users = -1 and n = 0", em, "recommend_query", n_users=-1, n=0)
    rec.note("recommend_query: n = 0 and a bad user id", em.recommend_query, [0, n_u], 0)
    rec.note("recommend_query: no users", em.recommend_query, [], 2)


def run_diverse_and_added_items(rec, em, dims):
    """The session pairing of recommend_diverse and recommend_add_items; leaves ``em`` with added items."""
    n_u, n_i, _ = dims
    d = em.recommend_diverse
    rec.note("recommend_diverse: no similarity session", d, [0, 1], 2, 4, 0.5)
    em.similar_begin("users")
    em.similar_add()
    rec.note("recommend_diverse: a similarity session over the users", d, [0, 1], 2, 4, 0.5)
    em.similar_begin("items")
    rec.note("recommend_diverse: a similarity session without slots", d, [0, 1], 2, 4, 0.5)
    em.similar_add()
    em.similar_add()
    rec.note("recommend_diverse: two slots against one", d, [0, 1], 2, 4, 0.5)
    em.similar_begin("items")
    em.similar_add()
    rec.note("recommend_diverse: pool < n", d, [0, 1], 5, 4, 0.5)
    rec.note("recommend_diverse: pool = 1025", d, [0, 1], 2, 1025, 0.5)
    rec.note("recommend_diverse: trade_off = -1", d, [0, 1], 2, 4, -1.0)
    rec.note("recommend_diverse: trade_off NaN", d, [0, 1], 2, 4, NAN)
    rec.note("recommend_diverse: pool < n and trade_off NaN", d, [0, 1], 5, 4, NAN)
    rec.note("recommend_diverse: n = 0 and a bad user id", d, [0, n_u], 0, 4, 0.5)


def run_add_items(rec, em, dims):
    n_u, n_i, _ = dims
    eta = np.full((1, 2, L), 1.0 / L)
    rec.note("recommend_add_items: eta of rank 2", em.recommend_add_items, np.zeros((2, L)))
    rec.note("recommend_add_items: eta last axis", em.recommend_add_items, np.zeros((1, 2, L + 1)))
    rec.note("recommend_add_items: eta of two blocks", em.recommend_add_items, np.zeros((2, 2, L)))
    for what, seen in BAD_CSR(n_u):
        rec.note(f"recommend_add_items: seen {what}", em.recommend_add_items, eta, seen)
    rec.raw("recommend_add_items: n_new = -1", em, "recommend_add_items", n_new=-1)
    rec.raw("recommend_add_items: null eta", em, "recommend_add_items", eta=None)
    rec.raw("recommend_add_items: seen without values", em, "recommend_add_items", seen_offsets=[0, 1])
    rec.note("recommend_add_items: two items", em.recommend_add_items, eta, ([0, 1, 2], [0, 1]))
    rec.note("recommend_add_items: a second call", em.recommend_add_items, eta)
    rec.raw("recommend_add_items: a second call with n_new = -1", em, "recommend_add_items", n_new=-1)
    rec.note("recommend_add after recommend_add_items", em.recommend_add)
    rec.note("recommend_diverse: a catalogue with added items", em.recommend_diverse, [0, 1], 2, 4, 0.5)
    # the catalogue now holds n_items + 2 items: the bound of a candidate moves with it
    rec.note("recommend_query_within: no users, candidate n_items + 1 after add_items", em.recommend_query_within, [], 2, [0, n_i + 1])
    rec.note("recommend_query_within: candidate n_items + 2 after add_items", em.recommend_query_within, [0, 1], 2, [0, n_i + 2])
    rec.note("recommend_query_items: item n_items + 2 after add_items", em.recommend_query_items, [0, n_i + 2], 2)


def run_loo(rec, loo, n_obs):
    rec.note("loo_rows: a position out of range", loo.loo_rows, [0, n_obs])
    rec.note("loo_rows: a negative position", loo.loo_rows, [0, -1])
    rec.note("loo_rows: no rows", loo.loo_rows, [])
    rec.raw("loo_rows: n_rows = -1", loo, "loo_rows", n_rows=-1)
    for m in (0, 1025):
        rec.note(f"loo_lowest: m = {m}", loo.loo_lowest, m)
    rec.note("loo_lowest: user_flags of the wrong length", loo.loo_lowest, 2, [1, 0])
    rec.raw("loo_lowest: null rows", loo, "loo_lowest", rows=None)


# every query entry this table adds to the ones of host_layer_cases.py, for "no session" and "before any add"
NEW_QUERIES = ["recommend_query_within", "recommend_query_theta_within", "recommend_rank", "recommend_query_quota",
               "recommend_query_theta_quota", "recommend_query_shelves", "recommend_query_theta_shelves",
               "recommend_query_explore", "recommend_list_propensity", "recommend_allocate", "recommend_assign",
               "recommend_top_pairs_bulk", "recommend_pair_bar", "recommend_diverse", "recommend_query_groups",
               "recommend_assortment", "recommend_query_ensemble", "recommend_pair_spread", "similar_pairs",
               "inform_query", "inform_query_theta", "inform_mean_theta", "explain_query", "loo_rows", "loo_sides",
               "loo_lowest"]


def run(pkg, protos, data, dims):
    """[[label, code or exception class name, message], ...]"""
    n_u, n_i, n_r = dims
    w = np.arange(n_r, dtype=np.float64)
    rec = Recorder(pkg, protos)

    def context():
        em = pkg.HipEM(data, K, L, n_u, n_i, n_r, swap_sides=0)
        em.init_params(31)
        return em

    with context() as bare:
        for name in NEW_QUERIES:
            rec.raw(f"no session: {name}", bare, name)
        bare.recommend_begin(w, True)
        bare.similar_begin("items")
        bare.inform_begin()
        bare.explain_begin(w)
        bare.loo_begin()
        for name in NEW_QUERIES:
            rec.raw(f"no add: {name}", bare, name)
        with context() as em, context() as inf, context() as ex:
            em.recommend_begin(w, True)
            em.recommend_add()
            inf.inform_begin()
            inf.inform_add()
            ex.explain_begin(w)
            ex.explain_add()
            run_diverse_and_added_items(rec, em, dims)      # opens the similarity session recommend_diverse needs
            run_prefix(rec, em, inf, ex, dims)
            run_theta(rec, em, inf, dims)
            run_categories(rec, em, dims)
            run_explore(rec, em, bare, dims)
            run_user_sets(rec, em, dims)
            run_groups_assortment_ensemble(rec, em, dims)
            with context() as sim_items, context() as sim_users:
                sim_items.similar_begin("items")
                sim_items.similar_add()
                sim_users.similar_begin("users")
                sim_users.similar_add()
                run_pairs_items(rec, em, sim_items, sim_users, dims)
            run_add_items(rec, em, dims)
    with context() as loo:
        loo.loo_begin()
        loo.loo_add()
        run_loo(rec, loo, len(data))
    labels = [row[0] for row in rec.rows]
    assert len(set(labels)) == len(labels), sorted(l for l in set(labels) if labels.count(l) > 1)
    return rec.rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import mmsbm_amd
    data, dims = make_data()
    rows = run(mmsbm_amd, prototypes(tree), data, dims)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as fh:     # one line per row
        fh.write("[\n" + ",\n".join(" " + json.dumps(row) for row in rows) + "\n]\n")
    print(f"{len(rows)} requests from {os.path.dirname(mmsbm_amd.__file__)} -> {args.out}")


if __name__ == "__main__":
    main()
