"""What the engine entries of the C ABI launch and return -- the cases of tests/test_gpu_engine_entries.py and the
recorder of their expected table.

The engine entries are everything that is not a serving query: creating a context, parameters in and out, the EM
iteration in its forms, the likelihood, prod_dist / predict, compute_omegas, restart slots, snapshots, the index
read-back and the timers.  A case opens ONE context of a shape and form, walks the whole sequence of run_case() on it
and closes it (the library appends its launch counts to MMSBM_HIP_LAUNCH_LOG when a context is destroyed).  Recorded
per case: the launch count per kernel name of this process since the case began, and per step of the sequence the
SHA-256 of every array and the hexadecimal form of every scalar the step returned.  The EM step uses no atomics, so on
one device type both are a function of the library alone.

The data, all tiny: "uniform", the 3,000 uniform ratings of 64 x 48 x 3 of pair_plan_cases.make_data() -- segments of
some 47 and 21 triples, long enough at this size to be cut, so its contexts carry work lists and whole-segment lists;
"short", 3,000 ratings of 300 x 70 x 5 (test_gpu_pass_dense.py's base) -- ten triples a user, no work lists at all; and
border_tables' "whole-fits" -- one user of 614 pieces and a pair of 64 among short segments, the heavy-tailed table at
the limits of the whole-segment lists.  The shapes are the smallest that reach each form of the iteration:

  two-launch          10 x 10  "short": the two launches of fused_small.hpp over whole, uncut segments
  two-launch-lists    10 x 10  "uniform": the same form with whole-segment lists (and once with the sides swapped)
  whole-segments      20 x 20  "whole-fits": the same form, lists at their limits
  four-launch         10 x 10  "uniform", option fused = 0: the separate stages on the vector ALUs, work lists and combine
  pass-dense          20 x 20  "short", option pass_dense = 1: the form needs rows of 17 .. 32 on the K side, at most 24
                               on the L side and data without work lists -- no shape of pair_plan_cases.SHAPES over
                               "uniform" has all three; 20 x 20 over "short" is what test_gpu_pass_dense.py starts from
  matrix-cores        64 x 64  "uniform": the pair stage on the matrix cores, and option a_units = 3
  wide-rows         1100 x 4   "uniform": the wide-row plan

The table a commit gives is recorded with

    python tests/engine_cases.py --out tests/gpu_engine_entries_parent.json [--tree DIR]

(--tree: the directory whose mmsbm_amd is imported, e.g. a build of the parent commit; this file's own checkout by
default).  The committed table is the one of the commit BEFORE the engine moved out of mmsbm_hip.hip into units of its
own: the refactor must not move an entry.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (table, K, L, swap_sides, options set right after the creation)
CASES = {
    "two-launch": ("short", 10, 10, 0, ()),
    "two-launch-lists": ("uniform", 10, 10, 0, ()),
    "two-launch-swapped": ("uniform", 10, 10, 1, ()),
    "whole-segments": ("whole-fits", 20, 20, 0, ()),
    "four-launch": ("uniform", 10, 10, 0, (("fused", 0),)),
    "pass-dense": ("short", 20, 20, 0, (("pass_dense", 1),)),
    "matrix-cores": ("uniform", 64, 64, 0, ()),
    "wide-rows": ("uniform", 1100, 4, 0, ()),
}
# what the form of a case shows as (read after the options are set)
FORM_OPTIONS = ("launches", "pass_dense", "mfma", "wide", "fused_split", "splits_users", "splits_pairs", "item_grid",
                "gpu_layout", "a_units", "a_chunks", "chunk_pairs", "n_chunks")
OMEGAS_MAX = 1024        # K x L up to which compute_omegas is part of the sequence (N K L doubles come back)
N_INDEX_ARRAYS = 19
_DATA = {}


def table(name):
    """(data, (n_users, n_items, n_ratings)) of a table.  Built once."""
    if name not in _DATA:
        if name == "uniform":
            import pair_plan_cases
            _DATA[name] = pair_plan_cases.make_data()
        elif name == "short":
            from oracle import mmsbm_oracle as orc
            data = orc.synthetic_triples(3000, 300, 70, 5, seed=3)
            _DATA[name] = (data, tuple(int(data[:, j].max()) + 1 for j in range(3)))
        else:
            import border_tables
            t = border_tables.table(name)
            _DATA[name] = (t.data, t.dims)
    return _DATA[name]


def start_params(shapes, seed):
    """(theta, eta, pr) of the given shapes: rows that sum to 1, nothing zero."""
    rng = np.random.default_rng([seed, *shapes[0], *shapes[1]])
    simplex = lambda shape: (lambda a: a / a.sum(axis=-1, keepdims=True))(rng.random(shape) + 0.01)  # noqa: E731
    pr = rng.random(shapes[2]) + 0.01
    return simplex(shapes[0]), simplex(shapes[1]), pr / pr.sum(axis=2, keepdims=True)


def _value(v):
    if v is None:
        return None
    if isinstance(v, str):
        return v
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if isinstance(v, (int, np.integer)):
        return int(v)
    from serving_launch_cases import _digest
    return _digest(v)


def _index_array(pkg, em, which):
    """mmsbm_hip_index_array(which) by its number (HipEM.index_arrays names them; here every number is asked)."""
    return pkg.core._fetch_i32("mmsbm_hip_index_array", em._h, which)


def _kernel_bytes(pkg, em, index):
    rd, wr = C.c_int64(0), C.c_int64(0)
    pkg._lib.call("mmsbm_hip_kernel_bytes", em._h, index, C.byref(rd), C.byref(wr))
    return [int(rd.value), int(wr.value)]


def _refused(fn):
    """What fn() raises, as text -- or "ran"."""
    try:
        fn()
    except Exception as e:   # noqa: BLE001  (the message is what is recorded)
        return f"{type(e).__name__}: {e}"
    return "ran"


def run_sequence(pkg, em, data, rec):
    """The engine entries over one open context, in an order in which every step's state is the steps' before it.
    rec(label, *values) records what a step returned."""
    n_r = em.n_ratings
    start = start_params(em._shapes(), 3)
    n_kernels = pkg._lib.load().mmsbm_hip_kernel_count()

    # -- the index and the byte model
    for which in range(N_INDEX_ARRAYS):
        rec(f"index_array {which}", _index_array(pkg, em, which))
    rec("index_array 19", _refused(lambda: _index_array(pkg, em, N_INDEX_ARRAYS)))
    rec("degrees", *em.degrees())
    for index in range(n_kernels):
        rec(f"kernel_bytes {index}", *_kernel_bytes(pkg, em, index))

    # -- parameters in and out
    rec("get_params before any", _refused(em.get_params))
    rec("init_params", em.init_params(41), *em.get_params())
    em.set_params(*start)
    rec("set_params", *em.get_params())

    # -- the iteration: uncommitted before and after committed ones, odd and even counts, eager and replayed
    rec("update_coefficients first", *em.update_coefficients())
    em.iterate(3)
    rec("iterate 3 eager", *em.get_params())
    rec("update_coefficients after a commit", *em.update_coefficients())
    em.iterate(2)
    rec("iterate 2 eager", *em.get_params())
    em.set_graph_mode(1)
    em.iterate(5)                                   # two replays and one eager iteration
    rec("iterate 5 graph", *em.get_params())
    em.iterate(4)
    rec("iterate 4 graph", *em.get_params())
    rec("update_coefficients after a replay", *em.update_coefficients())
    em.iterate(1)
    rec("iterate 1 graph mode", *em.get_params())
    if em.get_option("launches") == 2.0:            # A is stale after a two-launch commit: the four-launch capture needs
        em.set_option("fused", 0)                   # it made outside the capture
        em.iterate(4)
        rec("iterate 4 graph after fused = 0", *em.get_params())
        em.set_option("fused", 1)
        em.iterate(2)
        rec("iterate 2 graph after fused = 1", *em.get_params())
    em.set_graph_mode(0)
    if em.get_option("a_units") > 0:
        em.set_option("a_units", 3)
        rec("a_units = 3", em.get_option("a_units"), em.get_option("a_chunks"))
        em.iterate(2)
        rec("iterate 2 a_units = 3", *em.get_params())
        em.set_option("a_units", 0)
        rec("a_units = 0", em.get_option("a_units"), em.get_option("a_chunks"))

    # -- once-per-run entries
    rec("likelihood", em.likelihood())
    rec("result", *em.result())
    for rows, what in ((5, "few rows"), (300, "many rows")):     # the per-row kernels; the B table (rows >= items / 4)
        rec(f"prod_dist {what}", em.prod_dist(data[:rows]))
        em.predict_begin(data[:rows], np.arange(1.0, n_r + 1))
        rec(f"predict_add {what}", em.predict_add())
        em.iterate(1)
        rec(f"predict_add again {what}", em.predict_add())
        rec(f"predict_finish {what}", *em.predict_finish())
    em.set_option("predict_fast", 0)
    rec("prod_dist many rows, predict_fast = 0", em.prod_dist(data[:300]))
    em.set_option("predict_fast", 1)
    if em.k * em.l <= OMEGAS_MAX:
        rec("compute_omegas", em.compute_omegas())

    # -- restart slots and snapshots
    rec("snapshot_get before any", _refused(em.snapshot_get))
    em.set_slots(3)
    rec("set_slots 3", em.slots, em.selected, em.bytes_per_slot, _refused(em.get_params))
    rec("iterate without every slot", _refused(lambda: em.iterate(1)))
    for s in range(3):
        rec(f"slot {s} init_params", em.select(s).init_params(50 + s))
    em.iterate(3)
    for s in (0, 2):
        em.select(s).snapshot_save()
    rec("likelihood slot 2", em.likelihood())
    em.set_graph_mode(1)
    em.iterate(3)
    em.set_graph_mode(0)
    for s in range(3):
        rec(f"slot {s} after 6", *em.select(s).get_params())
    rec("update_coefficients slot 2", *em.update_coefficients())
    for s in (0, 2):
        rec(f"slot {s} snapshot_get", *em.select(s).snapshot_get())
    rec("slot 1 snapshot_get", _refused(em.select(1).snapshot_get))
    rec("result slot 1", *em.result())
    em.set_slots(3)                                 # the same count: parameters and snapshots dropped, slot 0 selected
    rec("set_slots 3 again", em.slots, em.selected, _refused(em.get_params), _refused(em.snapshot_get))
    for s in range(3):
        em.select(s).set_params(*start_params(em._shapes(), 60 + s))
    em.iterate(2)
    rec("slot 1 after set_slots 3 again", *em.select(1).get_params())
    rec("select_slot 3", _refused(lambda: em.select(3)))
    em.set_slots(1)
    rec("set_slots 1", em.slots, em.selected, em.bytes_per_slot, _refused(em.get_params))
    em.set_params(*start)
    em.iterate(1)
    rec("iterate 1 after set_slots 1", *em.get_params())

    # -- the timers: only what they launch (the launch log) and whether they ran; time_stage clobbers the state
    rec("time_iterations", "ran" if em.time_iterations(3) >= 0 else "negative")
    prof = em.profile_iterations(2)
    rec("profile_iterations", json.dumps({name: list(v[1:]) for name, v in sorted(prof.items())}))
    for stage in range(n_kernels):
        rec(f"time_stage {stage}", _refused(lambda: em.time_stage(stage, reps=2)))
    rec("time_stage out of range", _refused(lambda: em.time_stage(n_kernels, reps=2)))


def run_case(pkg, name):
    """{"launches": {kernel: count}, "form": {option: value}, "steps": [[label, value, ...], ...]} of one case."""
    from serving_launch_cases import _launches
    tab, k, l, swap, options = CASES[name]
    data, (n_u, n_i, n_r) = table(tab)
    if swap:
        data, n_u, n_i = np.ascontiguousarray(data[:, [1, 0, 2]]), n_i, n_u
    path = os.environ["MMSBM_HIP_LAUNCH_LOG"]
    pos = os.path.getsize(path) if os.path.exists(path) else 0
    steps = []
    em = pkg.HipEM(data, k, l, n_users=n_u, n_items=n_i, n_ratings=n_r, swap_sides=swap)
    try:
        for option, value in options:
            em.set_option(option, value)
        form = {option: em.get_option(option) for option in FORM_OPTIONS}
        form["swapped"] = bool(em.swapped)
        run_sequence(pkg, em, data, lambda label, *values: steps.append([label] + [_value(v) for v in values]))
    finally:
        em.close()
    return {"launches": dict(sorted(_launches(path, pos).items())), "form": form, "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if not os.environ.get("MMSBM_HIP_LAUNCH_LOG"):   # (the library reads it when it is loaded)
        os.environ["MMSBM_HIP_LAUNCH_LOG"] = os.path.join(tempfile.mkdtemp(), "launch_log.tsv")
    sys.path.insert(0, ROOT)                         # the oracle, whatever --tree holds
    sys.path.insert(0, os.path.abspath(args.tree))
    import mmsbm_amd
    out = {name: run_case(mmsbm_amd, name) for name in CASES}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as fh:     # one line per step
        cases = []
        for name, got in out.items():
            steps = ",\n".join("   " + json.dumps(row) for row in got["steps"])
            cases.append(f' "{name}": {{\n  "launches": {json.dumps(got["launches"])},\n  "form": {json.dumps(got["form"])},\n'
                         f'  "steps": [\n{steps}\n  ]\n }}')
        fh.write("{\n" + ",\n".join(cases) + "\n}\n")
    print(f"{len(out)} cases from {os.path.dirname(mmsbm_amd.__file__)} -> {args.out}")


if __name__ == "__main__":
    main()
