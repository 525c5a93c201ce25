"""The transitions between the forms of an EM iteration -- two, three or four launches (mmsbm_amd/csrc/step_plan.hpp) --
that tests/engine_cases.py does not walk: the cases of tests/test_gpu_step_forms.py and the recorder of their expected
table.

A case opens one context over a tiny table of engine_cases.py and walks run_sequence() on it.  After every step it
records what shows the form and what the form did: the options "launches", "pass_dense" and "fused"; the byte model of
every kernel id; the launches per iteration of every kernel id over two profiled iterations; and the SHA-256 of the
parameters after them.  The EM step uses no atomics, so on one device type all of it is a function of the library alone.

  three   20 x 20 "short": no work lists, rows of 17 .. 24 groups -- the three-launch form is reachable
  two     10 x 10 "short": two launches over whole, uncut segments; three launches never apply
  lists   10 x 10 "uniform": two launches with whole-segment lists; the separate form runs work lists and a combine

The table a commit gives is recorded with

    python tests/step_form_cases.py --out tests/gpu_step_forms_parent.json [--tree DIR]

(--tree: the directory whose mmsbm_amd is imported, e.g. a build of the parent commit; this file's own checkout by
default).  The committed table is the one of the commit BEFORE the form moved into StepPlan: the refactor must not
move an entry.
"""
import argparse
import json
import os
import sys

import engine_cases as ec

ROOT = ec.ROOT

# name -> (table, K, L)
CASES = {
    "three": ("short", 20, 20),
    "two": ("short", 10, 10),
    "lists": ("uniform", 10, 10),
}
FORM_OPTIONS = ("launches", "pass_dense", "fused")


def run_sequence(pkg, em, rec):
    """rec(label, *values) records what a step returned; state(label) what shows the form after it."""
    n_kernels = pkg._lib.load().mmsbm_hip_kernel_count()

    def state(label):
        rec(label + ": options", *(em.get_option(o) for o in FORM_OPTIONS))
        rec(label + ": kernel_bytes", json.dumps([ec._kernel_bytes(pkg, em, j) for j in range(n_kernels)]))
        prof = em.profile_iterations(2)
        rec(label + ": launches per iteration", json.dumps({name: v[1] for name, v in sorted(prof.items())}))
        rec(label + ": params", *em.get_params())

    def option(step, name, value):
        rec(f"{step} {name} = {value}", ec._refused(lambda: em.set_option(name, value)))
        state(f"{step} {name} = {value}")

    em.set_params(*ec.start_params(em._shapes(), 3))
    state("created")
    # 1. the three settings of "pass_dense" at the ask create() left
    for v in (1, 0, -1):
        option("1", "pass_dense", v)
    # 2. a forced "fused" wins over "pass_dense" = 1; 3. and gives way again
    em.set_option("pass_dense", 1)
    option("2", "fused", 1)
    option("3", "fused", 0)
    # 4. the blocked matrix-core pair stage takes the two-launch form away, and "mfma" = 0 brings it back
    option("4a", "mfma", 2)
    option("4b", "fused", 1)
    option("4c", "mfma", 0)
    option("4d", "fused", 1)
    option("4e", "fused", 0)
    # 5. an uncommitted iteration between two committed ones under "pass_dense" = 1
    em.iterate(1)
    rec("update_coefficients between commits", *em.update_coefficients())
    em.iterate(1)
    state("after update_coefficients")
    # 6. new parameters in the middle of a run, then replayed graphs
    em.set_params(*ec.start_params(em._shapes(), 7))
    em.set_graph_mode(1)
    em.iterate(4)
    em.set_graph_mode(0)
    state("set_params, iterate 4 graph")
    # 7. two restart slots per launch (three launches need one), and one again
    em.set_slots(2)
    for s in range(2):
        em.select(s).set_params(*ec.start_params(em._shapes(), 20 + s))
    em.select(0)
    state("set_slots 2")
    rec("set_slots 2: slot 1", *em.select(1).get_params())
    em.set_slots(1)
    em.set_params(*ec.start_params(em._shapes(), 3))
    state("set_slots 1")


def run_case(pkg, name):
    """[[label, value, ...], ...] of one case."""
    tab, k, l = CASES[name]
    data, (n_u, n_i, n_r) = ec.table(tab)
    steps = []
    em = pkg.HipEM(data, k, l, n_users=n_u, n_items=n_i, n_ratings=n_r)
    try:
        run_sequence(pkg, em, lambda label, *values: steps.append([label] + [ec._value(v) for v in values]))
    finally:
        em.close()
    return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)                         # the oracle, whatever --tree holds
    sys.path.insert(0, os.path.abspath(args.tree))
    import mmsbm_amd
    out = {name: run_case(mmsbm_amd, name) for name in CASES}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as fh:     # one line per step
        cases = []
        for name, steps in out.items():
            rows = ",\n".join("  " + json.dumps(row) for row in steps)
            cases.append(f' "{name}": [\n{rows}\n ]')
        fh.write("{\n" + ",\n".join(cases) + "\n}\n")
    print(f"{len(out)} cases from {os.path.dirname(mmsbm_amd.__file__)} -> {args.out}")


if __name__ == "__main__":
    main()
