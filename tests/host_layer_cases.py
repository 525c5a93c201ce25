"""The host layer above the kernels as the public API shows it -- option values, refusal texts, which call feeds which
timer: the cases of tests/test_gpu_host_layer.py and the recorder of their expected table.

Over the data of pair_plan_cases.make_data() three things are recorded:

  options   per shape (K, L) -- the two-launch form, the matrix-core form, the wide form -- the value of every option
            name after create, then after each of STEPS (every settable name with a valid value, every bound's first
            invalid value, a read-only name and an unknown one passed to set_option): [step, code, message, values];
  refusals  on (3, 2) with parameters set: every session entry without a session, every query entry before any add,
            an id out of range at row 1 of a two-row request for every entry that checks ids, n = 0 and n = 1025 for
            the three top-N entries: [label, code, message] (code 0: accepted);
  timers    on (3, 2): after each of nine timed calls which of the eight "<name>_ms" options are non-zero.

The table a commit gives is recorded with

    python tests/host_layer_cases.py --out tests/gpu_host_layer_parent.json [--tree DIR]

(--tree: the checkout whose mmsbm_amd is imported, e.g. a build of the parent commit; this file's own by default).  The
committed table is the one of the commit BEFORE sessions, options and timers got one shape each: the refactor must not
move an entry.
"""
import argparse
import json
import os
import sys

import numpy as np

OPTIONS = ("graph", "quad", "mfma", "predict_fast", "fused", "nt_out", "recommend_ms", "fold_in_ms", "position_ms",
           "similar_ms", "top_pairs_ms", "overlap_ms", "heldout_ms", "top_pairs_groups", "audience_ms", "audience_rows",
           "audience_entries", "launches", "wide", "lik_fast", "lik_g", "ranges_pairs", "ranges_users", "chunk_pairs",
           "n_chunks", "a_units", "a_chunks", "items_pairs", "items_users", "splits_pairs", "splits_users", "fused_split",
           "item_grid", "gpu_layout")
TIMERS = ("recommend_ms", "fold_in_ms", "position_ms", "top_pairs_ms", "audience_ms", "similar_ms", "overlap_ms",
          "heldout_ms")

SHAPES = [(3, 2),        # two launches per iteration
          (64, 64),      # the matrix cores: a_units means something
          (1100, 4)]     # the wide form

# (name, value); "graph_mode" is mmsbm_hip_set_graph_mode.  The valid ones end on the vector ALUs with predict_fast on,
# where every shape can run; then every bound's first invalid value, a read-only name and an unknown one.
STEPS = [("graph", 1), ("graph_mode", 0), ("graph_mode", 1), ("lik_fast", 1), ("lik_g", 4), ("quad", 1), ("quad", 0),
         ("fused", 0), ("nt_out", 5), ("predict_fast", 0), ("predict_fast", 1), ("top_pairs_groups", 7),
         ("audience_rows", 3), ("audience_entries", 1000), ("a_units", 3), ("mfma", 2), ("mfma", 1), ("mfma", 0),
         ("lik_fast", 3), ("lik_g", 3), ("nt_out", 16), ("nt_out", -1), ("top_pairs_groups", 4097),
         ("top_pairs_groups", 1.5), ("audience_rows", -1), ("audience_rows", 2.0 ** 31), ("audience_entries", -1),
         ("a_units", 17), ("fused", 1), ("wide", 1), ("no_such_option", 1)]


def shape_id(shape):
    return f"{shape[0]}x{shape[1]}"


def make_data():
    from pair_plan_cases import make_data as pair_plan_data
    return pair_plan_data()


def attempt(pkg, fn, *args, **kwargs):
    """[status code, message] of a call through the handle: [0, ""] when the library accepts it."""
    try:
        fn(*args, **kwargs)
    except pkg._lib.HipLibraryError as exc:
        return [exc.code, exc.message]
    return [0, ""]


def read_options(em):
    return {name: em.get_option(name) for name in OPTIONS}


def run_options(pkg, shape, data, dims, created=None, stepped=None):
    """[[step, code, message, {option: value}], ...] of one shape: step "created", then one entry per STEPS.
    created(em) runs on the new context, stepped(em) after the last step."""
    n_u, n_i, n_r = dims
    with pkg.HipEM(data, shape[0], shape[1], n_u, n_i, n_r, swap_sides=0) as em:
        if created:
            created(em)
        rows = [["created", 0, "", read_options(em)]]
        for name, value in STEPS:
            if name == "graph_mode":
                status = attempt(pkg, em.set_graph_mode, value)
            else:
                status = attempt(pkg, em.set_option, name, value)
            rows.append([f"{name}={value}", *status, read_options(em)])
        if stepped:
            stepped(em)
    return rows


def run_refusals(pkg, data, dims):
    """[[label, code, message], ...] on (3, 2) with parameters set."""
    n_u, n_i, n_r = dims
    k, l = SHAPES[0]
    w = np.arange(n_r, dtype=np.float64)
    out = []
    with pkg.HipEM(data, k, l, n_u, n_i, n_r, swap_sides=0) as em:
        em.init_params(31)

        def note(label, fn, *args, **kwargs):
            out.append([label, *attempt(pkg, fn, *args, **kwargs)])

        def queries(tag):   # every query entry; no session, or none added to it
            note(f"{tag}: predict_finish", em.predict_finish, want_matrix=False)
            note(f"{tag}: recommend_query", em.recommend_query, [0, 1], 2)
            note(f"{tag}: recommend_query_theta", em.recommend_query_theta, np.zeros((0, 2, k)), 2)
            note(f"{tag}: recommend_positions", em.recommend_positions, [0, 1], [0, 0, 0], [])
            note(f"{tag}: recommend_add_items", em.recommend_add_items, np.zeros((0, 1, l)))
            note(f"{tag}: recommend_top_pairs", em.recommend_top_pairs, 2)
            note(f"{tag}: recommend_query_items", em.recommend_query_items, [0, 1], 2)
            note(f"{tag}: recommend_audience", em.recommend_audience, [0, 1], 0.5)
            note(f"{tag}: similar_query", em.similar_query, [0, 1], 2)
            note(f"{tag}: overlap_query", em.overlap_query)
            note(f"{tag}: heldout_mean", em.heldout_mean)

        queries("no session")
        note("no session: predict_add", em.predict_add)
        note("no session: recommend_add", em.recommend_add)
        note("no session: similar_add", em.similar_add)
        note("no session: overlap_add", em.overlap_add)
        note("no session: heldout_eval", em.heldout_eval)
        note("no session: heldout_add", em.heldout_add)
        for kind in ("recommend", "similar", "overlap", "heldout"):
            note(f"no session: {kind}_end", getattr(em, kind + "_end"))

        em.predict_begin(data[:8], w)
        em.recommend_begin(w, True)
        em.similar_begin("items")
        em.overlap_begin("items")
        em.heldout_begin(data[:8])
        queries("no add")

        em.recommend_add()
        em.similar_add()
        for n in (0, 1025):
            note(f"n = {n}: recommend_query", em.recommend_query, [0, 1], n)
            note(f"n = {n}: recommend_query_items", em.recommend_query_items, [0, 1], n)
            note(f"n = {n}: similar_query", em.similar_query, [0, 1], n)
        note("row 1: recommend_query", em.recommend_query, [0, n_u], 2)
        note("row 1, negative: recommend_query", em.recommend_query, [0, -1], 2)
        note("row 1: recommend_positions", em.recommend_positions, [0, n_u], [0, 0, 0], [])
        note("row 1: recommend_top_pairs", em.recommend_top_pairs, 2, [0, n_u])
        note("row 1: recommend_query_items", em.recommend_query_items, [0, n_i], 2)
        note("row 1: recommend_audience", em.recommend_audience, [0, n_i], 0.5)
        note("row 1: similar_query, items", em.similar_query, [0, n_i], 2)
        em.similar_begin("users")
        em.similar_add()
        note("row 1: similar_query, users", em.similar_query, [0, n_u], 2)
        note("row 1: prod_dist", em.prod_dist, [[0, 0], [n_u, 0]])
        note("row 1: predict_begin", em.predict_begin, [[0, 0, 0], [0, n_i, 0]], w)
        note("row 1: heldout_begin", em.heldout_begin, [[0, 0, 0], [0, 0, n_r]])
        note("row 1: fold_in", em.fold_in, [[0, 0, 0], [1, 0, 0]], 1, 2)
        note("row 1: fold_in_items", em.fold_in_items, [[0, 0, 0], [0, 1, 0]], 1, 2)
        for kind in ("recommend", "similar", "overlap", "heldout"):
            note(f"open: {kind}_end", getattr(em, kind + "_end"))
    return out


def run_timers(pkg, data, dims):
    """[[call, {timer: non-zero}], ...] on (3, 2): "created", then one entry per timed call."""
    n_u, n_i, n_r = dims
    k, l = SHAPES[0]
    w = np.arange(n_r, dtype=np.float64)
    with pkg.HipEM(data, k, l, n_u, n_i, n_r, swap_sides=0) as em:
        em.init_params(31)
        out = []

        def note(call):
            out.append([call, {name: em.get_option(name) != 0.0 for name in TIMERS}])

        note("created")
        em.recommend_begin(w, True)
        em.recommend_add()
        em.recommend_query([0, 1], 2)
        note("recommend_query")
        em.recommend_query_items([0, 1], 2)
        note("recommend_query_items")
        em.recommend_positions([0, 1], [0, 1, 2], [3, 4])
        note("recommend_positions")
        em.recommend_top_pairs(4)
        note("recommend_top_pairs")
        em.recommend_audience([0, 1], 0.0)
        note("recommend_audience")
        em.recommend_end()
        em.similar_begin("items")
        em.similar_add()
        em.similar_query([0, 1], 2)
        note("similar_query")
        em.similar_end()
        em.overlap_begin("items")
        em.overlap_add()
        em.overlap_query()
        note("overlap_query")
        em.overlap_end()
        em.heldout_begin(data[:8])
        em.heldout_add()
        note("heldout_add")
        em.heldout_end()
        em.fold_in([[0, 0, 0], [0, 1, 1]], 1, 2)
        note("fold_in")
    return out


# (call, the timer it feeds) in the order of run_timers
TIMED_CALLS = [("recommend_query", "recommend_ms"), ("recommend_query_items", "recommend_ms"),
               ("recommend_positions", "position_ms"), ("recommend_top_pairs", "top_pairs_ms"),
               ("recommend_audience", "audience_ms"), ("similar_query", "similar_ms"), ("overlap_query", "overlap_ms"),
               ("heldout_add", "heldout_ms"), ("fold_in", "fold_in_ms")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import mmsbm_amd
    data, dims = make_data()
    table = {"options": {shape_id(s): run_options(mmsbm_amd, s, data, dims) for s in SHAPES},
             "refusals": run_refusals(mmsbm_amd, data, dims),
             "timers": run_timers(mmsbm_amd, data, dims)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)

    def block(rows, pad):   # one line per entry
        return "[\n" + ",\n".join(pad + " " + json.dumps(row) for row in rows) + "\n" + pad + "]"

    with open(args.out, "w") as fh:
        shapes = ",\n".join(f'  "{sid}": {block(rows, "  ")}' for sid, rows in table["options"].items())
        fh.write('{\n "options": {\n' + shapes + '\n },\n "refusals": ' + block(table["refusals"], " ") +
                 ',\n "timers": ' + block(table["timers"], " ") + "\n}\n")
    print(f"{len(SHAPES)} shapes, {len(table['refusals'])} refusals, {len(table['timers']) - 1} timed calls from "
          f"{os.path.dirname(mmsbm_amd.__file__)} -> {args.out}")


if __name__ == "__main__":
    main()
