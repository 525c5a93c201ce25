"""Seeded random walks through the ``HipEM`` surface against a shadow model of the context (plain Python and numpy).

Every other GPU test is one call sequence written for one feature.  A context keeps state from call to call -- the
double-buffer index, "A is current" per slot, the captured graphs, which slots have parameters, the two-launch / four-
launch choice, sessions that hold copies made at their ``*_add``, snapshots -- and a stale table or a wrong parity shows
only in an order nobody wrote down.  ``walk`` generates such orders, ``Shadow`` tracks what the state should be, and
``run`` checks every step that observes something against

  * the oracle (``orc.em_step`` over spans of at most 3 iterations, ``orc.update_coefficients``,
    ``orc.compute_likelihood``, the restatements of the ``*_cpu.py`` files), within bounds other tests already hold, and
  * a canonical replay: a fresh one-slot context, default options, ``set_params(origin)`` and ONE ``iterate(total)``
    (``replay_state``), or a fresh context loaded with the arrays a session saw at its adds (``replay_session``) --
    bit for bit.  Two-launch == four-launch, graph == eager, ``nt_out``, chunked ``iterate``, slot s of n == a one-slot
    context and "an evaluation changes no slot and no session" are each asserted alone elsewhere; here in combination.

An operation is ``(name, args)``, a Python literal; arrays (rows, users, starting parameters) are derived from the seeds
in ``args`` and the shape, so a printed walk replays as it stands: ``api_walk.run(hip, shape, ops)``.
``("refused", (name, args))`` is a call the library must refuse with MMSBM_E_INVALID in host code, before any launch.

``hip`` is the ``mmsbm_amd`` module, or any object with ``HipEM`` and ``_lib`` (tests/fake_device.full_fake_module()).
"""
import numpy as np
import pytest

from conftest import assert_elementwise, rel_err
from oracle import mmsbm_oracle as orc

SPAN = 3            # iterations from an origin the oracle comparison covers (check_step_and_loop, test_restart_slots_in_super_groups)
REFUSED_SHARE = 10  # at most one call in REFUSED_SHARE is one that must be refused

# name -> U, I, R, K, L; "fused": option at the start (None: the library's choice); "both": the library allows both
# forms of the iteration for the shape (the walk toggles "fused" only there); "data": the recipe
SHAPES = {
    "fused": dict(dims=(70, 50, 4, 5, 6), fused=1, swap=0, both=True, data="fused"),
    "four_launch": dict(dims=(70, 50, 4, 5, 6), fused=0, swap=0, both=True, data="four_launch"),
    "matrix_core": dict(dims=(60, 50, 3, 40, 30), fused=None, swap=0, both=False, data="matrix_core"),
    "side80": dict(dims=(60, 50, 3, 80, 6), fused=None, swap=0, both=False, data="side80"),
    "one_rating": dict(dims=(50, 40, 1, 3, 4), fused=None, swap=0, both=False, data="one_rating"),
    "skewed": dict(dims=(None, None, None, 10, 10), fused=1, swap=0, both=True, data="skewed"),
    "fused_swapped": dict(dims=(70, 50, 4, 5, 6), fused=1, swap=1, both=True, data="fused"),
    "matrix_core_swapped": dict(dims=(60, 50, 3, 40, 30), fused=None, swap=1, both=False, data="matrix_core"),
}
START_SLOTS = 3
LENGTH = 64
# the first three walks of every shape were chosen (on the CPU, by missing() below) so that each shape's set reaches every
# operation kind, every kind of refusal and every pattern of PATTERNS: test_api_walk_cpu.py fails if a set stops doing
# so.  The shapes whose walks cost the stand-in device next to nothing have three more, taken as they come.
SEEDS = {"fused": (253, 125, 186, 1, 2, 3), "four_launch": (214, 14, 3, 1, 2, 4), "matrix_core": (61, 111, 50),
         "side80": (38, 261, 65), "one_rating": (23, 7, 18, 1, 2, 3), "skewed": (233, 216, 10),
         "fused_swapped": (80, 55, 240, 1, 2, 3), "matrix_core_swapped": (50, 30, 10)}
CASES = [(shape, seed) for shape in SHAPES for seed in SEEDS[shape]]
_PROBLEMS = {}


def problem(shape):
    """{"data", "U", "I", "R", "K", "L", "d_u", "d_i", ...} of a shape, built once."""
    if shape in _PROBLEMS:
        return _PROBLEMS[shape]
    spec = SHAPES[shape]
    U, I, R, K, L = spec["dims"]
    if spec["data"] == "skewed":
        # the `skew` data of test_two_launch_iteration_is_chosen_by_size_and_refused_where_it_does_not_apply: one very
        # busy user, whose segment is cut into work items that sit in one workgroup of the two-launch tail
        rng = np.random.default_rng(0)
        n = 9_000
        data = np.stack([np.where(rng.random(n) < 0.3, 3, rng.integers(0, 900, n)), rng.integers(0, 400, n),
                         rng.integers(0, 5, n)], axis=1).astype(np.int64)
        U, I, R = (int(data[:, j].max()) + 1 for j in range(3))
    else:
        from test_gpu_heldout import SHAPES as recipes, em_problem      # 12 U rows, every id present
        data = em_problem(next(s for s in recipes if s[0] == spec["data"]), 1)[0]
    d_u, d_i = orc.degrees(data, U, I)
    _PROBLEMS[shape] = dict(spec, name=shape, data=data, U=U, I=I, R=R, K=K, L=L, d_u=d_u, d_i=d_i)
    return _PROBLEMS[shape]


# ---- arrays from the seeds an operation carries ------------------------------------------------------------------------
def start_params(prob, seed):
    return orc.init_params(seed, prob["U"], prob["I"], prob["R"], prob["K"], prob["L"], prob["d_u"], prob["d_i"])


def rows_of(prob, seed, m):
    rng = np.random.default_rng([11, seed])
    return np.stack([rng.integers(0, prob["U"], m), rng.integers(0, prob["I"], m), rng.integers(0, prob["R"], m)], 1)


def weights_of(prob, kind):
    """kind 0: the expected rating (1 .. R); kind k > 0: one-hot on rating (k - 1) mod R."""
    if kind == 0:
        return np.arange(1.0, prob["R"] + 1)
    w = np.zeros(prob["R"])
    w[(kind - 1) % prob["R"]] = 1.0
    return w


def ids_of(seed, top, m, distinct=False):
    rng = np.random.default_rng([13, seed])
    return rng.choice(top, min(m, top), replace=False) if distinct else rng.integers(0, top, m)


def positions_request(prob, seed, m):
    rng = np.random.default_rng([17, seed])
    users = rng.integers(0, prob["U"], m)
    offsets = np.concatenate([[0], np.cumsum(rng.integers(0, 5, m))]).astype(np.int64)
    return users, offsets, rng.integers(0, prob["I"], int(offsets[-1]))


def fold_rows(prob, seed, n_new, n_rows, items_side):
    rng = np.random.default_rng([19, seed])
    new = rng.integers(0, n_new, n_rows)
    if items_side:
        return np.stack([rng.integers(0, prob["U"], n_rows), new, rng.integers(0, prob["R"], n_rows)], 1)
    return np.stack([new, rng.integers(0, prob["I"], n_rows), rng.integers(0, prob["R"], n_rows)], 1)


# ---- the shadow ---------------------------------------------------------------------------------------------------------
class Shadow:
    """What a context should hold after a sequence of operations.  A slot's lineage is (origin key, iterations since),
    None without parameters; an origin key names a set of host arrays: ("seed", s) = orc.init_params(s, ...), ("read", i)
    = what the get_params at operation i returned.  A session keeps the lineages as they were at each add, a snapshot
    the lineage at its save.  set_slots drops parameters and snapshots, selects slot 0 and leaves every session as it
    is (include/mmsbm_hip.h); `total` counts the iterations since the tables were allocated: its parity is the double
    buffer's."""

    def __init__(self, n_slots, fused):
        self.graph, self.fused = 0, fused
        self.pred = self.rec = self.sim = self.ho = None
        self._slots(n_slots)

    def _slots(self, n):
        self.n, self.sel, self.total = n, 0, 0
        self.slot, self.snap = [None] * n, [None] * n

    def ready(self):
        return all(x is not None for x in self.slot)

    @property
    def cur(self):
        return self.slot[self.sel]

    def apply(self, i, op):
        name, a = op
        if name == "select":
            self.sel = a[0]
        elif name in ("set_params", "init_params"):
            self.slot[self.sel] = (("seed", a[0]), 0)
        elif name == "iterate":
            self.slot = [(o, n + a[0]) for o, n in self.slot]
            self.total += a[0]
        elif name == "get_params":
            self.slot[self.sel] = (("read", i), 0)
        elif name == "set_graph_mode":
            self.graph = a[0]
        elif name == "set_option":
            if a[0] == "fused":
                self.fused = a[1]
        elif name == "set_slots":
            total = self.total if a[0] == self.n else 0       # (the same count keeps the tables and their parity)
            self._slots(a[0])
            self.total = total
        elif name == "snapshot_save":
            self.snap[self.sel] = self.cur
        elif name == "restore":
            self.slot[self.sel] = self.snap[self.sel]
        elif name in ("predict_begin", "recommend_begin", "similar_begin", "heldout_begin"):
            setattr(self, _SESSION[name.split("_")[0]], dict(args=a, adds=[]))
        elif name in ("predict_add", "recommend_add", "similar_add", "heldout_add"):
            getattr(self, _SESSION[name.split("_")[0]])["adds"].append(self.cur)
        elif name in ("predict_finish", "recommend_end", "similar_end", "heldout_end"):
            setattr(self, _SESSION[name.split("_")[0]], None)
        # everything else observes and changes nothing


_SESSION = {"predict": "pred", "recommend": "rec", "similar": "sim", "heldout": "ho"}


# ---- the generator ------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, rng, shape):
        self.rng, self.spec, self.prob_dims = rng, SHAPES[shape], SHAPES[shape]["dims"]
        self.sh = Shadow(START_SLOTS, self.spec["fused"])
        self.ops, self.n_refused, self.done, self.refused_kinds = [], 0, set(), set()

    # -- plumbing
    def emit(self, name, *args):
        self.ops.append((name, tuple(args)))
        self.sh.apply(len(self.ops) - 1, self.ops[-1])

    def refuse(self, name, *args):
        self.ops.append(("refused", (name, tuple(args))))
        self.n_refused += 1
        self.refused_kinds.add(refusal_kind(self.sh, (name, tuple(args))))

    def can_refuse(self):
        return (self.n_refused + 1) * REFUSED_SHARE <= len(self.ops) + 1

    def r(self, lo, hi):
        return int(self.rng.integers(lo, hi + 1))

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def select(self, s):
        if self.sh.sel != s:
            self.emit("select", s)

    # -- building blocks
    def fill(self, s):
        self.select(s)
        self.emit(self.pick(["set_params", "init_params"]), self.r(1, 999))

    def rebase_for(self, n):
        """The reads that keep every slot within SPAN iterations of its origin through an iterate(n)."""
        for s in range(self.sh.n):
            if self.sh.slot[s][1] + n > SPAN:
                self.select(s)
                self.emit("get_params")

    def iterate(self, n=None):
        n = self.r(1, 4) if n is None else n
        n = min(n, SPAN)                        # (an iterate(4) would leave every span the oracle comparison covers)
        self.rebase_for(n)
        self.emit("iterate", n)

    def open_heldout(self):
        self.emit("heldout_begin", self.r(1, 999), self.pick([1, 300, 700]))

    def open_recommend(self):
        self.emit("recommend_begin", self.r(0, 4), self.r(0, 1))

    # -- the orders the walk is for (each also arises by chance; these make sure)
    def m_toggle(self):
        self.iterate()
        self.emit("set_option", "fused", 1 - self.sh.fused)
        self.iterate()

    def m_graph(self):
        if not self.sh.graph:
            self.emit("set_graph_mode", 1)
        self.rebase_for(SPAN)
        self.emit("update_coefficients")
        self.iterate(self.r(2, SPAN))

    def m_snapshot(self):
        if self.sh.total % 2 == 0:
            self.iterate(1)
        s = self.r(0, self.sh.n - 1)
        if self.sh.n > 1 and self.rng.random() < 0.5:       # another slot's snapshot beside it
            self.select(self.pick([o for o in range(self.sh.n) if o != s]))
            self.emit("snapshot_save")
        self.rebase_for(2)
        self.select(s)
        self.emit("snapshot_save")
        self.iterate(self.r(1, 2))
        self.select(s)
        self.emit("restore")
        self.iterate(self.r(1, 2))

    def m_eval(self):
        if self.sh.ho is None:
            self.open_heldout()
        self.iterate()
        self.emit("heldout_eval")
        self.iterate()

    def m_slots(self):
        self.emit("set_slots", self.pick([n for n in (1, 2, 3) if n != self.sh.n]))
        for s in range(self.sh.n):
            self.select(s)
            self.emit("set_params", self.r(1, 999))
        self.iterate()

    def m_recommend(self):
        if self.sh.rec is None:
            self.open_recommend()
        self.emit("recommend_add")
        self.iterate()
        self.emit("recommend_query", self.r(1, 999), 9, 5)

    def m_predict(self):
        a = self.r(0, self.sh.n - 1)
        b = self.pick([s for s in range(self.sh.n) if s != a])
        self.emit("predict_begin", self.r(1, 999), self.pick([1, 200]))
        self.select(a)
        self.emit("predict_add")
        self.iterate()
        self.select(b)
        self.emit("predict_add")
        self.emit("predict_finish")

    def m_result(self):
        n = self.r(1, SPAN)
        self.rebase_for(n)
        self.emit("result")
        self.emit("iterate", n)

    # -- one step
    def refusal(self):
        sh = self.sh
        c = [("select", self.pick([sh.n, sh.n + 3, -1]))]
        if sh.rec is None:
            c += [("recommend_query", 1, 3, 2), ("recommend_positions", 1, 2), ("recommend_top_pairs", 1, 0, 4)]
        if sh.sim is None:
            c.append(("similar_query", 0, 1, 3, 2))
        if sh.ho is None:
            c += [("heldout_eval",), ("heldout_add",), ("heldout_mean",)]
        elif not sh.ho["adds"]:
            c.append(("heldout_mean",))
        if sh.snap[sh.sel] is None:
            c.append(("snapshot_get",))
        fresh = [x for x in c if refusal_kind(sh, (x[0], x[1:])) not in self.refused_kinds]
        self.refuse(*self.pick(fresh or c))

    def step(self):
        sh = self.sh
        if not sh.ready():
            if self.can_refuse() and self.rng.random() < 0.5:
                self.refuse(*self.pick([("iterate", 2), ("heldout_eval",)]))
            else:
                self.fill(self.pick([s for s in range(sh.n) if sh.slot[s] is None]))
            return
        U, I = self.prob_dims[0] or 900, self.prob_dims[1] or 400
        one = lambda name, *args: (name, lambda: self.emit(name, *args))  # noqa: E731
        c = [(6, "iterate", self.iterate), (4,) + one("select", self.r(0, sh.n - 1)),
             (1, "set_params", lambda: self.emit("set_params", self.r(1, 999))),
             (1, "init_params", lambda: self.emit("init_params", self.r(1, 999))),
             (2,) + one("update_coefficients"), (2,) + one("likelihood"), (2,) + one("get_params"), (2,) + one("result"),
             (2,) + one("set_graph_mode", 1 - sh.graph),
             (1, "nt_out", lambda: self.emit("set_option", "nt_out", self.r(0, 7))),
             (1, "top_pairs_groups", lambda: self.emit("set_option", "top_pairs_groups", self.pick([0, 1, 3, 16]))),
             (1,) + one("set_slots", self.r(1, 3)), (2,) + one("snapshot_save"),
             (1,) + one("fold_in", self.r(1, 999), self.pick([1, 7]), self.pick([5, 60]), self.r(1, 6)),
             (1,) + one("fold_in_items", self.r(1, 999), self.pick([1, 7]), self.pick([5, 60]), self.r(1, 6)),
             (1, "m_graph", self.m_graph), (1, "m_snapshot", self.m_snapshot), (1, "m_eval", self.m_eval),
             (1, "m_slots", self.m_slots), (1, "m_recommend", self.m_recommend), (1, "m_result", self.m_result)]
        if self.spec["both"]:
            c += [(1, "fused", lambda: self.emit("set_option", "fused", 1 - sh.fused)), (1, "m_toggle", self.m_toggle)]
        if sh.n > 1:
            c.append((1, "m_predict", self.m_predict))
        if sh.snap[sh.sel] is not None:
            c += [(1,) + one("snapshot_get"), (1,) + one("restore")]
        if self.can_refuse():
            c.append((2, "refused", self.refusal))
        if sh.pred is None:
            c.append((1,) + one("predict_begin", self.r(1, 999), self.pick([1, 200])))
        else:
            c.append((2,) + one("predict_add"))
            if sh.pred["adds"]:
                c.append((1,) + one("predict_finish"))
        if sh.rec is None:
            c.append((2, "recommend_begin", self.open_recommend))
        else:
            c += [(2,) + one("recommend_add"), (1,) + one("recommend_end")]
            if sh.rec["adds"]:
                c += [(2,) + one("recommend_query", self.r(1, 999), self.pick([1, 9, 40]), self.pick([1, 5, I + 3])),
                      (2,) + one("recommend_positions", self.r(1, 999), self.pick([1, 12])),
                      (2,) + one("recommend_top_pairs", self.r(1, 999), self.pick([0, 1, 20]), self.pick([1, 10, 300]))]
        if sh.sim is None:
            c.append((2,) + one("similar_begin", self.r(0, 1)))
        else:
            side = sh.sim["args"][0]
            c += [(2,) + one("similar_add"), (1,) + one("similar_end")]
            if sh.sim["adds"]:
                c.append((2,) + one("similar_query", side, self.r(1, 999), self.pick([1, 10]),
                                    self.pick([1, 4, (U if side else I) + 2])))
        if sh.ho is None:
            c.append((2, "heldout_begin", self.open_heldout))
        else:
            c += [(2,) + one("heldout_eval"), (2,) + one("heldout_add"), (1,) + one("heldout_end")]
            if sh.ho["adds"]:
                c.append((2,) + one("heldout_mean"))
        # what this walk has not done yet comes first: a walk of a few dozen calls reaches most of the surface
        w = np.array([x[0] * (1 if x[1] in self.done else 6) for x in c], dtype=np.float64)
        _, label, fn = c[int(self.rng.choice(len(c), p=w / w.sum()))]
        self.done.add(label)
        fn()


def walk(seed, shape, length=LENGTH):
    """The operations of walk `seed` on `shape`: at least `length` of them, deterministic in (seed, shape, length).
    Every call is valid but for the ("refused", ...) ones, at most one in REFUSED_SHARE."""
    g = _Gen(np.random.default_rng([seed, sorted(SHAPES).index(shape), length]), shape)
    while len(g.ops) < length:
        g.step()
    return g.ops


# ---- what a set of walks reaches (from the sequences alone) --------------------------------------------------------------
OP_KINDS = ["select", "set_params", "init_params", "iterate", "update_coefficients", "likelihood", "get_params", "result",
            "set_graph_mode", "set_option:nt_out", "set_option:top_pairs_groups", "set_slots", "predict_begin",
            "predict_add", "predict_finish", "recommend_begin", "recommend_add", "recommend_query",
            "recommend_positions", "recommend_top_pairs", "recommend_end", "similar_begin", "similar_add",
            "similar_query", "similar_end", "heldout_begin", "heldout_eval", "heldout_add", "heldout_mean",
            "heldout_end", "snapshot_save", "snapshot_get", "restore", "fold_in", "fold_in_items", "refused"]
REFUSED_KINDS = ["a query without a session", "heldout_mean before an add", "snapshot_get without a save",
                 "iterate / heldout_eval while a slot has no parameters", "select out of range"]
PATTERNS = ["iterate, toggle fused, iterate", "update_coefficients, iterate with the graph on",
            "odd total, snapshot_save, iterate, restore, iterate", "iterate, heldout_eval, iterate",
            "set_slots, set_params, iterate", "recommend_add, iterate, recommend_query",
            "predict_add on a, iterate, predict_add on b, predict_finish", "result immediately followed by iterate",
            "restore or snapshot_get beside another slot's different snapshot"]
_READS = ("select", "get_params")      # what the generator puts in front of an iterate; they change no state


def kind(op):
    return f"set_option:{op[1][0]}" if op[0] == "set_option" else op[0]


def refusal_kind(sh, call):
    """Which of REFUSED_KINDS the refused `call` is in the state `sh` -- None if the library would accept it."""
    name, a = call
    session = {"recommend_query": sh.rec, "recommend_positions": sh.rec, "recommend_top_pairs": sh.rec,
               "similar_query": sh.sim, "heldout_add": sh.ho, "heldout_eval": sh.ho, "heldout_mean": sh.ho}
    if name == "select":
        return REFUSED_KINDS[4] if not 0 <= a[0] < sh.n else None
    if name in ("iterate", "heldout_eval") and not sh.ready():
        return REFUSED_KINDS[3]
    if name == "snapshot_get":
        return REFUSED_KINDS[2] if sh.snap[sh.sel] is None else None
    if name in session and session[name] is None:
        return REFUSED_KINDS[0]
    if name == "heldout_mean" and not sh.ho["adds"]:
        return REFUSED_KINDS[1]
    return None


def _chain(ops, i, names):
    """ops[i] is a names[0]: the index of the operation that completes `names`, in order, with nothing but _READS in
    between -- or None."""
    at, j = 1, i + 1
    while at < len(names) and j < len(ops):
        k = kind(ops[j])
        if k == names[at]:
            at += 1
        elif k not in _READS:
            return None
        j += 1
    return j - 1 if at == len(names) else None


def patterns_in(ops, shape):
    """The PATTERNS and REFUSED_KINDS a walk holds, found by running the shadow over it."""
    found = set()
    sh = Shadow(START_SLOTS, SHAPES[shape]["fused"])
    sel, total, graph, others = [], [], [], []              # before each operation
    for i, op in enumerate(ops):
        sel.append(sh.sel), total.append(sh.total), graph.append(sh.graph)
        others.append(any(x is not None and x != sh.snap[sh.sel] for x in sh.snap) if sh.sel < sh.n else False)
        if op[0] == "refused":
            found.add(refusal_kind(sh, op[1]))
        else:
            sh.apply(i, op)
    for i, op in enumerate(ops):
        k = kind(op)
        if k == "iterate":
            if _chain(ops, i, ["iterate", "set_option:fused", "iterate"]) is not None:
                found.add(PATTERNS[0])
            if _chain(ops, i, ["iterate", "heldout_eval", "iterate"]) is not None:
                found.add(PATTERNS[3])
        elif k == "update_coefficients":
            j = _chain(ops, i, ["update_coefficients", "iterate"])
            if j is not None and graph[j] == 1 and ops[j][1][0] >= 2:      # (a replay takes two iterations)
                found.add(PATTERNS[1])
        elif k == "snapshot_save" and total[i] % 2 == 1:
            j = _chain(ops, i, ["snapshot_save", "iterate", "restore"])
            if j is not None and sel[j] == sel[i] and _chain(ops, j, ["restore", "iterate"]) is not None:
                found.add(PATTERNS[2])
        elif k == "set_slots":
            j = i + 1
            while j < len(ops) and kind(ops[j]) in _READS + ("set_params", "init_params"):
                j += 1
            if j < len(ops) and ops[j][0] == "iterate" and any(o[0] == "set_params" for o in ops[i:j]):
                found.add(PATTERNS[4])
        elif k == "recommend_add":
            if _chain(ops, i, ["recommend_add", "iterate", "recommend_query"]) is not None:
                found.add(PATTERNS[5])
        elif k == "predict_add":
            j = _chain(ops, i, ["predict_add", "iterate", "predict_add"])
            if j is not None and sel[j] != sel[i] and ops[j + 1:j + 2] and ops[j + 1][0] == "predict_finish":
                found.add(PATTERNS[6])
        elif k == "result" and ops[i + 1:i + 2] and ops[i + 1][0] == "iterate":
            found.add(PATTERNS[7])
        elif k in ("restore", "snapshot_get") and others[i]:
            found.add(PATTERNS[8])
    return found


def missing(walks, shape):
    """What the walks of a shape's seed set leave out: operation kinds, refusal kinds, PATTERNS."""
    kinds = {kind(op) for ops in walks for op in ops}
    pats = set().union(*(patterns_in(ops, shape) for ops in walks))
    assert None not in pats, "a call that the library accepts was generated as one it refuses"
    both = SHAPES[shape]["both"]
    want_k = OP_KINDS + (["set_option:fused"] if both else [])
    want_p = PATTERNS if both else PATTERNS[1:]
    return [k for k in want_k if k not in kinds] + [p for p in REFUSED_KINDS + want_p if p not in pats]


# ---- the canonical replays ---------------------------------------------------------------------------------------------
def _context(hip, prob, slots):
    return hip.HipEM(prob["data"], prob["K"], prob["L"], n_users=prob["U"], n_items=prob["I"], n_ratings=prob["R"],
                     swap_sides=prob["swap"], slots=slots)


def replay_state(hip, shape, lineage):
    """(theta, eta, pr, likelihood) a lineage = (origin arrays, iterations) reaches without detours: a fresh one-slot
    context with the same data, K, L and swap_sides, default options, set_params(origin), one iterate(total)."""
    origin, total = lineage
    em = _context(hip, problem(shape), 1)
    try:
        em.set_params(*origin)
        if total:
            em.iterate(total)
        return em.get_params() + (em.likelihood(),)
    finally:
        em.close()


def replay_session(hip, shape, kind, added_params, query):
    """What `query` (a dict) returns in a fresh context whose slots hold `added_params`, every slot added in order to a
    fresh session of `kind`: "predict", "recommend", "similar", "heldout" or "fold" (no session: slot 0 answers)."""
    prob = problem(shape)
    S = len(added_params)
    em = _context(hip, prob, S)
    try:
        for s, prm in enumerate(added_params):
            em.select(s).set_params(*prm)
        ask = query["ask"]
        if kind == "fold":
            call = em.select(0).fold_in_items if query["items_side"] else em.select(0).fold_in
            return call(query["rows"], query["n_new"], query["iters"])
        if kind == "heldout":
            em.heldout_begin(query["rows"])
            if ask == "eval":
                return em.heldout_eval()
            lls = [em.select(s).heldout_add() for s in range(S)]
            return lls[-1] if ask == "add" else em.heldout_mean()
        if kind == "predict":
            em.predict_begin(query["rows"], query["weights"])
            stats = [em.select(s).predict_add() for s in range(S)]
            return stats[-1] if ask == "add" else em.predict_finish()
        if kind == "similar":
            em.similar_begin(query["side"])
            for s in range(S):
                em.select(s).similar_add()
            return em.similar_query(query["ids"], query["n"])
        assert kind == "recommend", kind
        em.recommend_begin(query["weights"], query["exclude"])
        for s in range(S):
            em.select(s).recommend_add()
        if ask == "query":
            return em.recommend_query(query["users"], query["n"])
        if ask == "positions":
            return em.recommend_positions(query["users"], query["offsets"], query["items"])
        return em.recommend_top_pairs(query["m"], query["users"])
    finally:
        em.close()


# ---- the runner ----------------------------------------------------------------------------------------------------------
class WalkFailure(AssertionError):
    """A step of a walk failed; `fault`: the library reported a HIP runtime error (nothing more should run)."""
    fault = False


def _flat(x):
    """The arrays and numbers of a result, in order."""
    if isinstance(x, (tuple, list)):
        return [y for part in x for y in _flat(part)]
    return [] if x is None else [np.asarray(x)]


def same_bits(got, want):
    a, b = _flat(got), _flat(want)
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
                                    for x, y in zip(a, b))


class _Run:
    def __init__(self, hip, shape):
        self.hip, self.shape, self.prob = hip, shape, problem(shape)
        self.sh = Shadow(START_SLOTS, self.prob["fused"])
        self.origins, self.states, self.oracle = {}, {}, {}
        self.checks = 0

    # -- what a lineage is
    def origin(self, key):
        if key not in self.origins:
            assert key[0] == "seed", key
            self.origins[key] = start_params(self.prob, key[1])
        return self.origins[key]

    def state(self, lineage):
        """(theta, eta, pr, likelihood) of a lineage by the canonical replay, once per lineage."""
        if lineage not in self.states:
            self.states[lineage] = replay_state(self.hip, self.shape, (self.origin(lineage[0]), lineage[1]))
        return self.states[lineage]

    def params(self, lineage):
        return self.state(lineage)[:3]

    def check(self, ok, what):
        self.checks += 1
        assert ok, what

    def check_state(self, got, lineage, what):
        """Bits of the replay; and the span from the lineage's own origin against the oracle."""
        self.check(same_bits(got, self.params(lineage)), f"{what}: not the bits of set_params(origin); iterate({lineage[1]})")
        assert lineage[1] <= SPAN, lineage
        if lineage not in self.oracle:
            t, e, p = self.origin(lineage[0])
            for _ in range(lineage[1]):
                t, e, p = orc.em_step(self.prob["data"], t, e, p, self.prob["d_u"], self.prob["d_i"])
            self.oracle[lineage] = (t, e, p)
        for g, w, nm in zip(got, self.oracle[lineage], ("theta", "eta", "pr")):   # check_step_and_loop's bounds
            self.check(rel_err(g, w) < 1e-11, f"{what}: {nm} against {lineage[1]} oracle steps: {rel_err(g, w):.3e}")
            assert_elementwise(g, w, f"{what} {nm}")

    def check_likelihood(self, got, lineage, what):
        t, e, p, lik = self.state(lineage)
        self.check(same_bits(got, lik), f"{what}: {got!r} is not the replay's {lik!r}")
        self.check(got == pytest.approx(float(orc.compute_likelihood(self.prob["data"], t, e, p)), rel=1e-11), what)

    # -- one operation on the device
    def call(self, em, name, a):
        prob = self.prob
        if name in ("select", "iterate", "set_graph_mode", "set_slots", "similar_begin"):
            return getattr(em, name)(a[0])
        if name == "set_option":
            return em.set_option(a[0], a[1])
        if name == "set_params":
            return em.set_params(*self.origin(("seed", a[0])))
        if name == "init_params":
            return em.init_params(a[0])
        if name == "restore":
            return em.set_params(*em.snapshot_get())
        if name == "predict_begin":
            return em.predict_begin(rows_of(prob, a[0], a[1]), weights_of(prob, 0))
        if name == "recommend_begin":
            return em.recommend_begin(weights_of(prob, a[0]), bool(a[1]))
        if name == "recommend_query":
            return em.recommend_query(ids_of(a[0], prob["U"], a[1]), a[2])
        if name == "recommend_positions":
            return em.recommend_positions(*positions_request(prob, a[0], a[1]))
        if name == "recommend_top_pairs":
            return em.recommend_top_pairs(a[2], None if a[1] == 0 else ids_of(a[0], prob["U"], a[1], distinct=True))
        if name == "similar_query":
            return em.similar_query(ids_of(a[1], prob["U"] if a[0] else prob["I"], a[2]), a[3])
        if name == "heldout_begin":
            return em.heldout_begin(rows_of(prob, a[0], a[1]))
        if name in ("fold_in", "fold_in_items"):
            return getattr(em, name)(fold_rows(prob, a[0], a[1], a[2], name == "fold_in_items"), a[1], a[3])
        return getattr(em, name)()        # the calls without arguments

    # -- one step: the call, then what it must have returned
    def step(self, em, i, op):
        from test_heldout_cpu import ll_bound, restate_heldout, restate_ll, restate_p
        hip, shape, sh, prob = self.hip, self.shape, self.sh, self.prob
        name, a = op
        K, L = prob["K"], prob["L"]
        if name == "refused":
            with pytest.raises(hip._lib.HipLibraryError) as e:
                self.call(em, *a)
            self.check(e.value.code == hip._lib.E_INVALID, (e.value.code, e.value.message))
            return
        got = self.call(em, name, a)
        before = sh.cur if sh.sel < sh.n else None
        sh.apply(i, op)
        if name == "get_params":
            self.check_state(got, before, "get_params")
            self.origins[("read", i)] = tuple(got)       # the slot goes on from what the device returned
        elif name == "result":
            self.check_state(got[1:], before, "result")
            self.check_likelihood(got[0], before, "result's likelihood")
        elif name == "snapshot_get":
            self.check_state(got, sh.snap[sh.sel], "snapshot_get")
        elif name == "likelihood":
            self.check_likelihood(got, before, "likelihood")
        elif name == "update_coefficients":
            want = orc.update_coefficients(prob["data"], *self.params(before))
            for g, w, nm in zip(got, want, ("n_theta", "n_eta", "n_pr")):         # TOL_STEP
                self.check(rel_err(g, w) < 1e-12, f"update_coefficients {nm}: {rel_err(g, w):.3e}")
        elif name == "set_option" and a[0] == "fused":
            self.check(em.get_option("launches") == (2 if a[1] else 4), "the option did not switch the form")
        elif name in ("heldout_eval", "heldout_add", "heldout_mean"):
            rows = rows_of(prob, *sh.ho["args"])
            ask = name.split("_")[1]
            prm = [self.params(x) for x in (sh.slot if ask == "eval" else sh.ho["adds"])]
            self.check(same_bits(got, replay_session(hip, shape, "heldout", prm, dict(ask=ask, rows=rows))), name)
            if ask == "mean":
                want = restate_heldout(prm, rows)
                self.check(abs(got[1] - want["mean_ll"]) <= ll_bound(K, L, want["mean_p"]), name)
            else:
                for g, x in zip(np.atleast_1d(got), prm if ask == "eval" else prm[-1:]):
                    p = restate_p(x, rows)
                    self.check(abs(g - restate_ll(p)) <= ll_bound(K, L, p), f"{name}: {g!r} against {restate_ll(p)!r}")
        elif name in ("recommend_query", "recommend_positions", "recommend_top_pairs"):
            prm = [self.params(x) for x in sh.rec["adds"]]
            w, excl = weights_of(prob, sh.rec["args"][0]), bool(sh.rec["args"][1])
            q = dict(ask=name.split("_", 1)[1], weights=w, exclude=excl)
            if name == "recommend_query":
                q.update(ask="query", users=ids_of(a[0], prob["U"], a[1]), n=a[2])
            elif name == "recommend_positions":
                q.update(zip(("users", "offsets", "items"), positions_request(prob, a[0], a[1])))
            else:
                q.update(m=a[2], users=None if a[1] == 0 else ids_of(a[0], prob["U"], a[1], distinct=True))
            self.check(same_bits(got, replay_session(hip, shape, "recommend", prm, q)), name)
            if name == "recommend_query":
                from test_gpu_recommend import check_rows
                from test_recommend_cpu import restate_scores, seen_items
                ref = restate_scores(prm, q["users"], prob["I"], w)
                check_rows(got, ref, np.arange(len(q["users"])), a[2],
                           seen_items(prob["data"], prob["U"]) if excl else None, q["users"])
                self.checks += 1
        elif name == "similar_query":
            prm = [self.params(x) for x in sh.sim["adds"]]
            q = dict(ask="query", side=a[0], ids=ids_of(a[1], prob["U"] if a[0] else prob["I"], a[2]), n=a[3])
            self.check(same_bits(got, replay_session(hip, shape, "similar", prm, q)), name)
        elif name == "predict_add":
            prm = [self.params(x) for x in sh.pred["adds"]]
            q = dict(ask="add", rows=rows_of(prob, *sh.pred["args"]), weights=weights_of(prob, 0))
            self.check(same_bits(got, replay_session(hip, shape, "predict", prm, q)), name)
        elif name in ("fold_in", "fold_in_items"):
            q = dict(ask=name, items_side=name == "fold_in_items", n_new=a[1], iters=a[3],
                     rows=fold_rows(prob, a[0], a[1], a[2], name == "fold_in_items"))
            self.check(same_bits(got, replay_session(hip, shape, "fold", [self.params(before)], q)), name)

    def finish_predict(self, em, i, op, session):
        got = self.call(em, "predict_finish", ())
        self.sh.apply(i, op)
        prm = [self.params(x) for x in session["adds"]]
        q = dict(ask="finish", rows=rows_of(self.prob, *session["args"]), weights=weights_of(self.prob, 0))
        self.check(same_bits(got, replay_session(self.hip, self.shape, "predict", prm, q)), "predict_finish")


def run(hip, shape, ops, seed=None):
    """Run `ops` on a fresh context of `shape` and check every step that observes something; at the end every slot.
    Returns {"ops", "checks"}.  A failure names the shape, the seed, the operation and the walk up to it, as a literal
    this function accepts -- to be replayed and cut down by hand."""
    r = _Run(hip, shape)
    prob = r.prob
    em = _context(hip, prob, START_SLOTS)
    i, op = -1, ("create", ())
    try:
        if prob["fused"] is not None:
            em.set_option("fused", prob["fused"])
            assert em.get_option("launches") == (2 if prob["fused"] else 4)
        if shape.startswith("matrix_core"):
            assert em.get_option("mfma") > 0
        if shape == "skewed":
            assert em.get_option("splits_users") > 0 and em.get_option("fused_split") == 2.0
        assert em.swapped == bool(prob["swap"])
        for i, op in enumerate(ops):
            if op[0] == "predict_finish":
                r.finish_predict(em, i, op, r.sh.pred)
            else:
                r.step(em, i, op)
        i, op = len(ops), ("every slot at the end", ())
        for s in range(r.sh.n):
            if r.sh.slot[s] is not None:
                r.check_state(em.select(s).get_params(), r.sh.slot[s], f"slot {s} at the end")
    except BaseException as exc:  # noqa: BLE001  (re-raised below with the walk)
        if isinstance(exc, (KeyboardInterrupt, SystemExit)):
            raise
        fail = WalkFailure(f"shape {shape!r}, seed {seed}, operation {i} {op!r}: {type(exc).__name__}: {exc}\n"
                           f"replay with api_walk.run(hip, {shape!r}, ops), ops =\n{list(ops[:i + 1])!r}")
        fail.fault = getattr(exc, "code", None) == getattr(hip._lib, "E_HIP", 2) and hasattr(exc, "func")
        raise fail from exc
    finally:
        em.close()
    return {"ops": len(ops), "checks": r.checks}
