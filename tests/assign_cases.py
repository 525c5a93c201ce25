"""The cases test_gpu_assign.py runs on the device, and test_assign_cpu.py checks for convergence without one: exact
models (exact_models.py), three capacity sets, with and without the exclusions, the default reserve and one that occurs
as a score.  Every reference is computed once and shared."""
import functools

import numpy as np

import assign_reference as ar
import exact_models as xm

SMALL = (7, 130, 4, 6, 5, 2)            # <= 8 users: fewer users than any cap set's items, one partial tile
SHAPES = list(xm.MANY) + [SMALL]        # 300 x 997 and 260 x 1,021: partial 128-tiles on both sides, three row tiles
VARIANTS = [("mixed", "stars"), ("sorted", "indicator"), ("constant", "indicator")]
CASES = [(v, s) for v in VARIANTS for s in SHAPES]
CASE_IDS = ["{}-{}-U{}I{}K{}L{}R{}S{}".format(*v, *s) for v, s in CASES]
SETS = ("cap1", "cap2of40", "drawn")
RESERVES = ("default", "occurring")
MAX_ROUNDS = 2000                       # every case converges within these (test_assign_cpu.py)
# epsilon per weight kind: 2^-4 where that converges within MAX_ROUNDS, else the next power of two that does
EPS = {"stars": 2.0 ** -4, "indicator": 2.0 ** -4}


@functools.lru_cache(maxsize=None)
def case_of(variant, shape):
    """The session's inputs and exact scores: computed once, shared by the tests, never written to."""
    case = xm.make_case(*variant, shape)
    case["scores"].setflags(write=False)
    return case


def caps_of(name, variant, shape):
    """int32 caps per item: all 1; 2 on a 40-item subset and 0 elsewhere (fewer slots than users on the large shapes:
    drop-outs and displacement chains); drawn from {0, 1, 2, 5, unlimited}."""
    I = shape[1]
    rng = np.random.default_rng(xm.case_seed(*variant, shape) + [SETS.index(name)])
    if name == "cap1":
        return np.full(I, 1, dtype=np.int32)
    if name == "cap2of40":
        caps = np.zeros(I, dtype=np.int32)
        caps[rng.choice(I, 40, replace=False)] = 2
        return caps
    assert name == "drawn", name
    return rng.choice(np.array([0, 1, 2, 5, -1]), I).astype(np.int32)


def default_reserve(w):
    span = float(np.max(w) - np.min(w))
    return float(np.min(w)) - (span if span > 0 else 1.0)


def reserve_of(kind, variant, shape):
    """The default (below every score), or a score that occurs: the median of user 3's row (user 3 has seen nothing)."""
    case = case_of(variant, shape)
    if kind == "default":
        return default_reserve(case["w"])
    return float(np.median(case["scores"][min(3, shape[0] - 1)]))


def epsilon_of(variant):
    return EPS[variant[1]]


@functools.lru_cache(maxsize=None)
def expected(variant, shape, name, exclude, reserve_kind, max_rounds=MAX_ROUNDS):
    """The reference's answer for all users of the case."""
    case = case_of(variant, shape)
    return ar.auction(case["scores"], case["users"], caps_of(name, variant, shape),
                      reserve_of(reserve_kind, variant, shape), epsilon_of(variant), case["seen"] if exclude else None,
                      max_rounds)


def combos():
    return [(name, exclude, kind) for name in SETS for exclude in (True, False) for kind in RESERVES]
