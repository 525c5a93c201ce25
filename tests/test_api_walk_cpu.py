"""The harness of tests/api_walk.py without a GPU: every walk test_gpu_api_walk.py runs passes on the stand-in device
(the reference alone), the committed seeds reach what the walks are for, and the harness can fail -- three planted state
bugs are each caught."""
import numpy as np
import pytest

import api_walk
import fake_device


@pytest.fixture(scope="module")
def fake():
    return fake_device.full_fake_module()


@pytest.mark.parametrize("shape,seed", api_walk.CASES, ids=[f"{sh}-{sd}" for sh, sd in api_walk.CASES])
def test_the_reference_alone_passes_every_walk(fake, shape, seed):
    ops = api_walk.walk(seed, shape)
    done = api_walk.run(fake, shape, ops, seed)
    assert done["ops"] == len(ops) >= 40 and done["checks"] >= 40


def test_walks_are_deterministic_valid_literals_with_few_refused_calls():
    import ast
    for shape, seed in api_walk.CASES:
        ops = api_walk.walk(seed, shape)
        assert ops == api_walk.walk(seed, shape) and ops != api_walk.walk(seed + 1, shape)
        assert ast.literal_eval(repr(ops)) == ops                       # what a failure prints is what run() accepts
        refused = [op for op in ops if op[0] == "refused"]
        assert len(refused) * api_walk.REFUSED_SHARE <= len(ops)            # at most 10 % of a walk
        assert all(op[0] != "iterate" or 1 <= op[1][0] <= api_walk.SPAN for op in ops)
        # no slot ever goes beyond SPAN iterations from its origin: the oracle comparison stays inside its bound
        sh = api_walk.Shadow(api_walk.START_SLOTS, api_walk.SHAPES[shape]["fused"])
        for i, op in enumerate(ops):
            if op[0] == "refused":
                assert api_walk.refusal_kind(sh, op[1]) is not None, (shape, seed, i, op)
                continue
            sh.apply(i, op)
            assert all(x is None or x[1] <= api_walk.SPAN for x in sh.slot), (shape, seed, i)


@pytest.mark.parametrize("shape", list(api_walk.SHAPES))
def test_the_seed_set_of_every_shape_reaches_what_the_walks_are_for(shape):
    """Every operation kind, every kind of refusal and every order of api_walk.PATTERNS, from the sequences alone."""
    walks = [api_walk.walk(seed, shape) for seed in api_walk.SEEDS[shape]]
    assert len(walks) >= 3 and all(len(ops) >= 40 for ops in walks)
    assert api_walk.missing(walks, shape) == []


def test_the_pattern_detectors_see_a_pattern_and_its_absence():
    start = [("set_params", (1,)), ("select", (1,)), ("set_params", (2,)), ("select", (2,)), ("init_params", (3,)),
             ("select", (0,))]
    ops = [("iterate", (1,)), ("snapshot_save", ()), ("select", (1,)), ("get_params", ()),
           ("iterate", (2,)), ("select", (0,)), ("restore", ()), ("iterate", (1,)), ("result", ()), ("iterate", (1,))]
    assert api_walk.patterns_in(start + ops, "fused") == {api_walk.PATTERNS[2], api_walk.PATTERNS[7]}
    even = start + [("iterate", (2,))] + ops[1:]                          # an even total at the save
    assert api_walk.patterns_in(even, "fused") == {api_walk.PATTERNS[7]}
    other = start + [("select", (1,)), ("snapshot_save", ()), ("select", (0,))] + ops[:5] + ops[6:]   # ... on another slot
    assert api_walk.patterns_in(other, "fused") == {api_walk.PATTERNS[7], api_walk.PATTERNS[8]}   # (two snapshots at it)
    eager = [("update_coefficients", ()), ("iterate", (2,))]
    assert api_walk.patterns_in(start + eager, "fused") == set()
    assert api_walk.patterns_in(start + [("set_graph_mode", (1,))] + eager, "fused") == {api_walk.PATTERNS[1]}


# ---- the harness can fail: three planted state bugs ----------------------------------------------------------------------
def planted(name):
    Full = fake_device.full_fake()

    class StaleLikelihood(Full):
        """A likelihood cached per slot that iterate does not drop."""

        def set_slots(self, n):
            super().set_slots(n)
            self._lik = {}

        def set_params(self, theta, eta, pr):
            super().set_params(theta, eta, pr)
            self._lik.pop(self._sel, None)

        def likelihood(self):
            if self._sel not in self._lik:
                self._lik[self._sel] = super().likelihood()
            return self._lik[self._sel]

    class QueryReadsTheSlot(Full):
        """A recommend_query that reads the slots' current parameters instead of those at their adds."""

        def recommend_begin(self, rating_weights, exclude_seen=True):
            super().recommend_begin(rating_weights, exclude_seen)
            self._rc["slots"] = []

        def recommend_add(self):
            super().recommend_add()
            self._rc["slots"].append(self._sel)

        def recommend_query(self, users, n):
            kept = self._rc["params"]
            if kept:
                self._rc["params"] = [self._params[s] if s < self.slots and self._params[s] is not None else k
                                      for s, k in zip(self._rc["slots"], kept)]
            try:
                return super().recommend_query(users, n)
            finally:
                self._rc["params"] = kept

    class SnapshotOfSlotZero(Full):
        """A restore that hands every slot the snapshot of slot 0."""

        def snapshot_get(self):
            own = super().snapshot_get()
            return own if self._snap[0] is None else tuple(a.copy() for a in self._snap[0])

    return {"likelihood": StaleLikelihood, "recommend_query": QueryReadsTheSlot, "restore": SnapshotOfSlotZero}[name]


@pytest.mark.parametrize("fault", ["likelihood", "recommend_query", "restore"])
def test_a_planted_state_bug_is_caught_by_a_walk_of_the_seed_set(fault):
    hip = fake_device.full_fake_module(planted(fault))
    caught = []
    for shape in ("fused", "one_rating"):                                  # (the two cheapest shapes on the CPU)
        for seed in api_walk.SEEDS[shape]:
            try:
                api_walk.run(hip, shape, api_walk.walk(seed, shape), seed)
            except api_walk.WalkFailure as exc:
                text = str(exc)
                assert f"shape {shape!r}, seed {seed}, operation" in text and "api_walk.run(hip" in text
                caught.append((shape, seed, text.split("\n")[0]))
    print(*caught, sep="\n")
    assert caught, f"no walk notices the planted {fault} bug"
    where = {"likelihood": ("likelihood", "result"), "recommend_query": ("recommend_query",),
             "restore": ("snapshot_get", "get_params", "result", "every slot", "likelihood", "update_coefficients",
                         "heldout", "recommend", "similar", "predict", "fold")}[fault]
    assert all(any(w in line for w in where) for _, _, line in caught), caught
