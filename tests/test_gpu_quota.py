"""Per-category caps on a top-N list on the device (quota.hpp: mmsbm_hip_recommend_query_quota, _query_theta_quota;
MMSBM.recommend_quota, recommend_new_quota) against the exact reference: models whose scores carry no rounding
(exact_models.py) and the numpy restatement of the walk (quota_reference.py, pinned in test_quota_cpu.py).

Everything is compared by EQUALITY -- items, counts, the padding, and the scores by their bits -- with no tie band and
no case left out: the answer is the row's full order walked with a counter per category, whatever form a category's
(m, q) selects, whatever column an item gets under a candidate list, whatever the split of the selection across waves.
"""
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

import catalogue_reference as cat
import exact_models as xm
import quota_reference as qr
from conftest import ROOT
from test_gpu_recommend import LaunchWindow, context, hip, problem  # noqa: F401  (hip: the fixture)

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_coverage  # noqa: E402

pytestmark = pytest.mark.gpu

SPLIT = (3, 5000, 4, 6, 5, 2)                                 # the selection is split across waves at column 1,000
assert SPLIT in xm.SPLIT
SHAPES = list(xm.MANY) + [SPLIT]
VARIANTS = [("mixed", "stars"), ("sorted", "indicator"), ("constant", "indicator")]
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]
NS = (1, 10, 257)
WINDOW = {}


@pytest.fixture(scope="module", autouse=True)
def _launches_of_this_file():
    """The launch log from the first test of this file on (read by the last one)."""
    WINDOW["lw"] = LaunchWindow().__enter__()
    yield


@functools.lru_cache(maxsize=None)
def case_of(variant, shape):
    """The session's inputs and exact scores: computed once, shared by the tests, never written to."""
    case = xm.make_case(*variant, shape)
    case["scores"].setflags(write=False)
    return case


def open_session(em, n_slots, w, exclude):
    em.recommend_begin(w, exclude)
    for s in range(n_slots):
        em.select(s).recommend_add()


def same_answer(got, want, what):
    """(items, scores, counts) equal in every entry, the padding included, scores by their bits."""
    for g, w, nm in zip(got, want, ("items", "scores", "counts")):
        gb, wb = (xm.bits(g), xm.bits(w)) if nm == "scores" else (np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
        assert gb.shape == wb.shape, (what, nm, gb.shape, wb.shape)
        if not np.array_equal(gb, wb):
            row = int(np.argwhere(gb != wb)[0][0])
            raise AssertionError(f"{what}: {nm} differ in {int((gb != wb).sum())} entries, first in row {row}: "
                                 f"device {np.asarray(g)[row]}, exact {np.asarray(w)[row]}")


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def every_cap(category_of, G, n):
    """(name, category_of, (offsets, items), caps) of every cap set of a layout; the mix also takes categories out."""
    csr = qr.categories_csr(category_of, G)
    for cname, caps in qr.cap_sets(n, G).items():
        if cname == "mix":
            absent = qr.mix_absent(category_of, G)
            yield cname, absent, qr.categories_csr(absent, G), caps
        else:
            yield cname, category_of, csr, caps


# ---- 1. every layout, cap and list length -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_layouts_and_caps_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users, scores = case["users"], case["scores"]
    lay = qr.layouts(I, np.random.default_rng(xm.case_seed(*variant, shape)))
    assert ("straddle" in lay) == (shape == SPLIT)
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            walk = qr.Walk(scores, users, None, case["seen"] if exclude else None)
            open_session(em, S, case["w"], exclude)
            for name, (category_of, G) in lay.items():
                ranks = {}
                for n in NS:
                    for cname, c_of, (off, items), caps in every_cap(category_of, G, n):
                        key = cname == "mix"
                        if key not in ranks:
                            ranks[key] = walk.ranks(c_of)
                        got = em.recommend_query_quota(users, n, off, items, caps)
                        same_answer(got, walk.top_n(n, c_of, caps, ranks[key]), f"{name} {cname} n={n} exclude={exclude}")
            em.recommend_end()
    finally:
        em.close()


# ---- 2. candidate subsets and the query's own exclusions ------------------------------------------------------------------------
def own_lists(rng, users, I, pool):
    """One list per request row, by the row's place: empty; one candidate; many items of the whole catalogue, shuffled,
    one repeated; all candidates but three."""
    out = []
    for b in range(len(users)):
        kind = b % 4
        if kind == 0:
            lst = []
        elif kind == 1:
            lst = [int(pool[b % len(pool)])]
        elif kind == 2:
            lst = rng.choice(I, min(I, 200), replace=False).tolist()
            lst = lst + lst[:1]
        else:
            lst = rng.permutation(pool)[3:].tolist()
        out.append(lst)
    return out


@pytest.mark.parametrize("variant,shape", CASES, ids=CASE_IDS)
def test_candidates_and_own_exclusions_are_exact(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(xm.case_seed(*variant, shape))
    again = np.arange(min(U, 7))[::-1]                        # a user asked twice carries two different lists
    users = i32(np.concatenate([case["users"], again]))
    scores = case["scores"][users]
    lay = qr.layouts(I, rng)
    # every other item; a block across column 128 of the compact table; a set that leaves most of mod64's categories empty
    # or within their cap (m <= q) and a few above it
    subsets = {"every_other": np.arange(0, I, 2), "block": np.arange(70, 70 + 300),
               "sparse": np.unique(np.concatenate([rng.choice(I, 40, replace=False), np.arange(5, I, 64)[:6], np.arange(9, I, 128)[:4]]))}
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            for sname, cand in subsets.items():
                lists = own_lists(rng, users, I, cand)
                walk = qr.Walk(scores, users, cand, case["seen"] if exclude else None, lists)
                for name in ("mod7", "mod64", "blocks", "random", "all_but_three"):
                    category_of, G = lay[name]
                    ranks = walk.ranks(category_of)
                    csr = qr.categories_csr(category_of, G)
                    m = np.array([np.isin(csr[1][csr[0][g]:csr[0][g + 1]], cand).sum() for g in range(G)])
                    if (sname, name) == ("sparse", "mod64"):
                        assert (m == 0).any() and (m == 1).any() and (m > 2).any()
                    for n in NS:
                        for cname in ("cap0", "cap1", "cap2", f"cap{n + 1}"):
                            caps = qr.cap_sets(n, G)[cname]
                            got = em.recommend_query_quota(users, n, *csr, caps, i32(cand), cat.csr(lists))
                            same_answer(got, walk.top_n(n, category_of, caps, ranks), f"{sname} {name} {cname} n={n} exclude={exclude}")
            em.recommend_end()
    finally:
        em.close()


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(VARIANTS[0], xm.MANY[0]), (VARIANTS[2], xm.MANY[1]), (VARIANTS[1], SPLIT)],
                         ids=["mixed-K7L9", "constant-K9L5", "sorted-split"])
def test_identities(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    users = case["users"]
    rng = np.random.default_rng(3)
    lay = qr.layouts(I, rng)
    cand = i32(np.arange(1, I, 3))
    extra = cat.csr([rng.choice(I, 30, replace=False) for _ in users])
    none = (np.zeros(1, dtype=np.int64), i32([]), i32([]))
    sample = i32([0, 1, 2, U - 1, 2][:max(3, min(U, 5))])
    thetas = np.stack([case["params"][s][0][sample] for s in range(S)])
    own = cat.csr([sorted(case["seen"][u]) for u in sample.tolist()])
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        for exclude in (True, False):
            open_session(em, S, case["w"], exclude)
            for n in NS:
                plain = em.recommend_query(users, n)
                what = f"n={n} exclude={exclude}"
                # no categories, and categories that cannot change the answer: recommend_query_within
                within = em.recommend_query_within(users, n, cand, extra)
                same_answer(em.recommend_query_quota(users, n, *none), plain, "no categories " + what)
                same_answer(em.recommend_query_quota(users, n, *none, cand, extra), within, "no categories, within " + what)
                csr7 = qr.categories_csr(*lay["mod7"])
                same_answer(em.recommend_query_quota(users, n, *csr7, i32(np.full(7, n)), cand, extra), within, "caps = n " + what)
                # all singletons with cap 1: the plain query
                singles = (np.arange(I + 1, dtype=np.int64), i32(np.arange(I)))
                same_answer(em.recommend_query_quota(users, n, *singles, i32(np.ones(I))), plain, "singletons " + what)
                # one category of everything with cap c: the first c of the plain list
                for c in (0, 1, 3, 256):
                    if c >= n:
                        continue
                    got = em.recommend_query_quota(users, n, np.array([0, I], dtype=np.int64), i32(np.arange(I)), i32([c]))
                    want = (plain[0].copy(), plain[1].copy(), np.minimum(plain[2], c))
                    want[0][:, c:], want[1][:, c:] = -1, -np.inf
                    same_answer(got, want, f"everything cap {c} " + what)
                # cap 0: the same query with the category taken out of the candidates
                for name in ("blocks", "mod7"):
                    category_of, G = lay[name]
                    banned = [g for g in range(G) if g % 2 == 0]
                    caps = i32([0 if g in banned else n for g in range(G)])
                    left = i32(np.flatnonzero(~np.isin(category_of, banned)))
                    same_answer(em.recommend_query_quota(users, n, *qr.categories_csr(category_of, G), caps),
                                em.recommend_query_within(users, n, left), f"cap 0 {name} " + what)
                # a user alone: the same user inside the full request
                category_of, G = lay["random"]
                csr, caps = qr.categories_csr(category_of, G), qr.cap_sets(n, G)["mix"]
                full = em.recommend_query_quota(users, n, *csr, caps, cand)
                for b in sorted({0, 1, U // 2, U - 1}):
                    same_answer(em.recommend_query_quota(users[b:b + 1], n, *csr, caps, cand), tuple(a[b:b + 1] for a in full), f"alone {b} " + what)
                # the theta entry with a slot's own theta: the user entry (the session's seen lists given as the rows' own)
                if exclude:
                    for cd in (None, cand):
                        same_answer(em.recommend_query_theta_quota(thetas, n, *csr, caps, own, cd),
                                    em.recommend_query_quota(sample, n, *csr, caps, cd), f"theta {cd is None} " + what)
                    same_answer(em.recommend_query_theta_quota(thetas, n, *none, own, cand),
                                em.recommend_query_theta(thetas, n, own, candidates=cand), "theta, no categories " + what)
            em.recommend_end()
    finally:
        em.close()


def test_added_items_belong_to_the_catalogue(hip):
    """Categories may name the items of recommend_add_items; one category straddles the training and the added ids."""
    variant, shape = VARIANTS[0], xm.MANY[0]
    U, I, K, L, R, S = shape
    n_new = 70
    case = case_of(variant, shape)
    rng = np.random.default_rng(11)
    src = rng.integers(0, I, n_new)                          # added item j duplicates training item src[j]'s eta rows
    new_eta = np.stack([case["params"][s][1][src] for s in range(S)])
    ext = [(t, np.vstack([e, new_eta[s]]), p) for s, (t, e, p) in enumerate(case["params"])]
    NI = I + n_new
    scores = xm.exact_scores(ext, case["users"], NI, case["w"])
    category_of = np.full(NI, -1, dtype=np.int64)
    category_of[I - 30:I + 40] = 0                           # 70 columns: the long form
    category_of[I + 40:] = 1                                 # 30 columns: a short one
    category_of[np.arange(0, I - 30, 2)] = 2
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        em.recommend_add_items(new_eta)
        walk = qr.Walk(scores, case["users"], None, case["seen"])
        for n in NS:
            for caps in ([1, 1, 1], [0, 2, 3], [5, 0, n + 1]):
                got = em.recommend_query_quota(case["users"], n, *qr.categories_csr(category_of, 3), i32(caps))
                same_answer(got, walk.top_n(n, category_of, caps), f"added items {caps} n={n}")
        em.recommend_end()
    finally:
        em.close()


# ---- 4. swapped sides ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", [(("mixed", "stars"), xm.MANY[1]), (("sorted", "indicator"), SPLIT)],
                         ids=["mixed-K9L5", "sorted-split"])
def test_swapped_contexts_answer_bitwise_the_same(hip, variant, shape):
    U, I, K, L, R, S = shape
    case = case_of(variant, shape)
    rng = np.random.default_rng(7)
    users = i32(np.arange(max(U, 9)) % U)
    cand = np.arange(0, I, 2)
    lists = [rng.choice(I, 40, replace=False) for _ in users]
    lay = qr.layouts(I, rng)
    thetas = np.stack([p[0][users] for p in case["params"]])
    asked = {name: (lay[name][0], qr.categories_csr(*lay[name]), qr.cap_sets(10, lay[name][1])["mix"]) for name in ("mod7", "blocks", "random")}
    answers = []
    for swap in (0, 1):
        em = context(hip, case["data"], case["params"], U, I, R, swap=swap)
        try:
            assert em.swapped == bool(swap)
            open_session(em, S, case["w"], True)
            got = {}
            for name, (_, csr, caps) in asked.items():
                got[name] = em.recommend_query_quota(users, 10, *csr, caps, i32(cand), cat.csr(lists))
                got["theta " + name] = em.recommend_query_theta_quota(thetas, 10, *csr, caps, None, i32(cand))
            answers.append(got)
            em.recommend_end()
        finally:
            em.close()
    scores = case["scores"][users]
    for name, (category_of, _, caps) in asked.items():
        same_answer(answers[0][name], qr.quota_top_n(scores, users, 10, category_of, caps, cand, case["seen"], lists), name)
        same_answer(answers[0]["theta " + name], qr.quota_top_n(scores, users, 10, category_of, caps, cand), "theta " + name)
    for what in answers[0]:
        same_answer(answers[1][what], answers[0][what], f"swapped {what}")


# ---- 5. users beyond one batch of scores --------------------------------------------------------------------------------------------
def test_batches_of_users(hip):
    """300 users over 100,003 items: three batches (128 + 128 + 44 rows), so the mask runs at a row offset of the request;
    a layout of short categories and one of long ones."""
    U, I, K, L, R, S = xm.BATCHES
    case = xm.make_case("mixed", "stars", xm.BATCHES, n_random=3000)
    users = case["users"]
    assert xm.batch_users(I, U) == 128
    blocks = np.arange(I) // 1000                             # blocks of 1,000 columns; the last three items uncategorised
    blocks[blocks == 100] = -1
    # (neighbouring ids share a category: in these models equal scores are common and ties go by id, so a row's best
    # items are often neighbours -- a layout that scatters a category over the row, item % G, changes no row here)
    layouts = {"short": (np.arange(I) // 25, (I + 24) // 25, 1),   # 25 columns each, two categories to a wave
               "long": (blocks, 100, 2)}
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        walk = qr.Walk(case["scores"], users, None, case["seen"], top=20000)
        plain = em.recommend_query(users, 10)
        for name, (category_of, G, q) in layouts.items():
            caps = np.full(G, q)
            got = em.recommend_query_quota(users, 10, *qr.categories_csr(category_of, G), i32(caps))
            same_answer(got, walk.top_n(10, category_of, caps), name)
            changed = (got[0] != plain[0]).any(axis=1)
            assert changed[:128].any() and changed[128:256].any() and changed[256:].any(), name    # every batch is masked
        em.recommend_end()
    finally:
        em.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_requests_are_refused_before_any_launch(hip):
    U, I, K, L, R, S = xm.MANY[0]
    case = case_of(("mixed", "stars"), xm.MANY[0])
    E = hip._lib.HipLibraryError
    users = i32([0, 1])
    off = np.array([0, 2, 3], dtype=np.int64)
    good = (off, i32([3, 5, 8]), i32([1, 0]))
    thetas = np.stack([p[0][users] for p in case["params"]])
    bad = {"unsorted": (off, i32([5, 3, 8]), i32([1, 1])), "repeated": (off, i32([3, 3, 8]), i32([1, 1])),
           "negative id": (off, i32([-1, 5, 8]), i32([1, 1])), "beyond": (off, i32([3, I, 8]), i32([1, 1])),
           "two categories": (off, i32([3, 5, 5]), i32([1, 1])), "negative cap": (off, i32([3, 5, 8]), i32([1, -1])),
           "offsets from 1": (np.array([1, 2, 3], dtype=np.int64), i32([3, 5, 8]), i32([1, 1])),
           "offsets decrease": (np.array([0, 3, 2], dtype=np.int64), i32([3, 5]), i32([1, 1]))}

    def refused(call, code=None):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == (hip._lib.E_INVALID if code is None else code), e.value

    with LaunchWindow() as lw:
        em = context(hip, case["data"], case["params"], U, I, R)
        try:
            refused(lambda: em.recommend_query_quota(users, 3, *good))                       # no session
            em.recommend_begin(case["w"], True)
            refused(lambda: em.recommend_query_quota(users, 3, *good))                       # a session without a slot
            refused(lambda: em.recommend_query_theta_quota(thetas[:0], 3, *good))
            for s in range(S):
                em.select(s).recommend_add()
            for name, cats in bad.items():
                refused(lambda: em.recommend_query_quota(users, 3, *cats))
                refused(lambda: em.recommend_query_theta_quota(thetas, 3, *cats))
            # what recommend_query_within / _query_theta_within refuse
            refused(lambda: em.recommend_query_quota(i32([0, U]), 3, *good))
            refused(lambda: em.recommend_query_quota(users, 3, *good, i32([5, 3, 8])))
            refused(lambda: em.recommend_query_quota(users, 3, *good, i32([3, 5, I])))
            refused(lambda: em.recommend_query_quota(users, 3, *good, None, (np.array([0, 2, 1], dtype=np.int64), i32([1]))))
            refused(lambda: em.recommend_query_quota(users, 3, *good, None, (off, i32([1, 2, I]))))
            refused(lambda: em.recommend_query_theta_quota(thetas, 3, *good, None, i32([3, 3])))
            refused(lambda: em.recommend_query_theta_quota(thetas, 3, *good, (off, i32([1, 2, I]))))
            for call in (lambda n: em.recommend_query_quota(users, n, *good),
                         lambda n: em.recommend_query_theta_quota(thetas, n, *good)):
                refused(lambda: call(0))
                refused(lambda: call(1025), hip._lib.E_UNSUPPORTED)
        finally:
            em.close()
        names = lw.names()
        assert not [k for k in names if k.startswith(("quota_", "cat_", "rec_score", "rec_select", "rec_exclude"))], names
    em = context(hip, case["data"], case["params"], U, I, R)
    try:
        open_session(em, S, case["w"], True)
        before = em.recommend_query(case["users"], 10)
        for cats in bad.values():
            with pytest.raises(E):
                em.recommend_query_quota(users, 3, *cats)
        em.recommend_query_quota(users, 3, *good)
        same_answer(em.recommend_query(case["users"], 10), before, "the plain query afterwards")   # the session still answers
        em.recommend_end()
    finally:
        em.close()


# ---- 7. the host class ------------------------------------------------------------------------------------------------------------------
def test_the_host_class_with_string_ids(hip):
    rng = np.random.default_rng(12)
    n_u, n_i, n_obs = 60, 150, 1500
    df = pd.DataFrame({"users": [f"u{x}" for x in rng.integers(0, n_u, n_obs)],
                       "items": [f"item-{x}" for x in rng.integers(0, n_i, n_obs)],
                       "ratings": rng.integers(1, 6, n_obs)})
    model = hip.MMSBM(4, 6, iterations=8, sampling=2, seed=5)
    model.fit(df, silent=True)
    items = list(model.data_handler.item_labels())
    code = {lab: j for j, lab in enumerate(items)}
    brands = {lab: f"brand-{int(lab.split('-')[1]) % 9}" for lab in items if int(lab.split("-")[1]) % 5}
    brands.update({"not-in-the-model": "brand-0", items[3]: None})
    caps = {"brand-0": 0, "brand-1": 1, "brand-2": 2, "brand-3": 3, "brand-4": 1, "brand-5": 40, "brand-6": 1}   # 7, 8: uncapped
    ask = ["u7", "u1", "u7", "u30"]
    pairs = [("u7", items[0]), ("u1", items[5]), ("u2", items[3]), ("nobody", items[0])]
    cand = [items[j] for j in rng.choice(len(items), 90, replace=False)]

    def composed(call, who, n, cap_of, pool):
        """The composition of existing calls: call(candidates, n) per category with n = cap, plus the uncapped candidates,
        merged by (score descending, encoded item id), cut to n."""
        members, once = {}, list(dict.fromkeys(who))
        for lab in pool:
            c = brands.get(lab)
            members.setdefault(c if c is not None and cap_of(c) is not None else None, []).append(lab)
        parts = []
        for c, labs in members.items():
            q = len(items) if c is None else cap_of(c)
            if q > 0:
                parts.append(call(once, labs, q))
        every = pd.concat(parts, ignore_index=True)
        out = []
        for u in who:
            block = every[every["users"] == u].copy()
            block["id"] = [code[i] for i in block["items"]]
            block = block.sort_values(["score", "id"], ascending=[False, True], kind="stable").head(n)
            block["rank"] = np.arange(1, len(block) + 1)
            block["category"] = [brands.get(i) for i in block["items"]]
            out.append(block.drop(columns="id"))
        return pd.concat(out, ignore_index=True)

    def same(got, want):
        assert list(got.columns) == ["users", "items", "score", "rank", "category"]
        for col in ("users", "items", "rank", "category"):
            assert got[col].tolist() == want[col].tolist(), col
        assert np.array_equal(xm.bits(got["score"].to_numpy()), xm.bits(want["score"].to_numpy()))

    for n in (5, 12):
        for mpc, cap_of in ((caps, caps.get), (1, lambda c: 1), (0, lambda c: 0)):
            for kw, pool in (({}, items), ({"candidates": cand, "exclude": pairs}, cand)):
                got = model.recommend_quota(users=ask, n=n, categories=brands, max_per_category=mpc, **kw)
                same(got, composed(lambda us, labs, q: model.recommend(users=us, n=q, candidates=labs, exclude=kw.get("exclude")),
                                   ask, n, cap_of, pool))
    capped = model.recommend_quota(users=ask, n=12, categories=brands, max_per_category=1)
    assert capped.groupby(["users", "category"]).size().max() <= 2          # (u7 is asked twice: two lists of at most one)
    assert not capped["items"].equals(model.recommend(users=ask, n=12)["items"])
    assert capped["category"].isna().any() and capped["category"].notna().any()
    frame = pd.DataFrame({"sku": list(brands), "brand": list(brands.values())})
    for form in (pd.Series(brands), frame):
        assert model.recommend_quota(users=ask, n=12, categories=form, max_per_category=1).equals(capped)
    empty = model.recommend_quota(users=ask, n=5, categories=brands, max_per_category=1, candidates=[])
    assert len(empty) == 0 and list(empty.columns) == list(capped.columns)
    with pytest.raises(ValueError, match="max_per_category"):
        model.recommend_quota(users=ask, categories=brands, max_per_category=True)

    new = pd.DataFrame({"users": [f"new{x}" for x in rng.integers(0, 5, 60)],
                        "items": [f"item-{x}" for x in rng.integers(0, n_i, 60)], "ratings": rng.integers(1, 6, 60)})
    new = new[new["items"].isin(items)]
    who = list(new["users"].drop_duplicates())
    for kw, pool in (({}, items), ({"candidates": cand}, cand)):
        got = model.recommend_new_quota(new, n=6, categories=brands, max_per_category=caps, **kw)
        same(got, composed(lambda us, labs, q: model.recommend_new(new, n=q, candidates=labs), who, 6, caps.get, pool))


# ---- 8. the launch log: these cases reach every kernel of quota.hpp ---------------------------------------------------------------------
def test_every_quota_kernel_was_launched_by_this_file(hip):
    names = WINDOW["lw"].names()
    compiled = [k for k in kernel_coverage.compiled_kernels(hip._lib.LIB_PATH) if k.startswith("quota_")]
    for k in ("quota_short_kernel", "quota_long_kernel"):
        assert k in compiled, (k, compiled)
    missing = [k for k in compiled if k not in names]
    assert not missing, (missing, sorted(names))
