"""The pair stage's launch plan as the public API shows it: the cases of tests/test_gpu_pair_plan.py and the recorder of
their expected table.

A case is a shape (K, L) -- the smallest that reaches each plan of mmsbm_amd/csrc/pair_plan.hpp -- and the creation knob
set around HipEM(); over tiny data it creates one context per option sequence, applies the sequence and reads the
options that show the plan after every step.  The table a commit gives is recorded with

    python tests/pair_plan_cases.py --out tests/gpu_pair_plan_parent.json [--tree DIR]

(--tree: the checkout whose mmsbm_amd is imported, e.g. a build of the parent commit; this file's own by default).  The
committed table is the one of the commit BEFORE the plan became one value: the refactor must not move an entry.
"""
import argparse
import json
import os
import sys

OPTIONS = ("mfma", "quad", "wide", "chunk_pairs", "n_chunks", "a_units", "a_chunks", "fused", "launches")

SHAPES = [(10, 10), (28, 28),          # block, small tile
          (32, 32),                    # largest tile still in the scalar cache
          (28, 40),                    # smallest with the tile in LDS + quad
          (52, 20), (20, 52),          # block, 256/512-thread mixes
          (64, 64),                    # mfma
          (64, 68),                    # just past mfma's 64 limit: blocked mfma
          (264, 16),                   # two slots per thread
          (100, 164),                  # four slots per thread
          (600, 5), (3, 1024),         # skinny
          (1100, 4)]                   # wide


def padded(d):
    return -(-d // 4) * 4 if d <= 256 else -(-d // 8) * 8 if d <= 512 else -(-d // 16) * 16 if d <= 1024 else -(-d // 32) * 32


# (K, L, environment variable set around the creation or None): every shape; the big-tile shapes (more than 1,024 padded
# entries) without the matrix cores as well; (28, 40) through the wide-row kernels
CASES = ([(k, l, None) for k, l in SHAPES] +
         [(k, l, "MMSBM_HIP_NO_MFMA") for k, l in SHAPES if padded(k) * padded(l) > 1024] +
         [(28, 40, "MMSBM_HIP_FORCE_WIDE")])

SEQUENCES = {"mfma": [("mfma", 0), ("mfma", 1), ("mfma", 2), ("mfma", 0)],
             "quad": [("quad", 0), ("quad", 1)],
             "fused": [("fused", 0)],
             "a_units": [("a_units", 3)]}


def case_id(case):
    k, l, env = case
    return f"{k}x{l}" + (f"-{env[len('MMSBM_HIP_'):].lower()}" if env else "")


def make_data():
    """About 3,000 uniform ratings of 64 users x 48 items x 3 ratings."""
    from oracle import mmsbm_oracle as orc
    data = orc.synthetic_triples(3000, 64, 48, 3, seed=17)
    return data, tuple(int(data[:, j].max()) + 1 for j in range(3))


def read_options(em):
    return {name: em.get_option(name) for name in OPTIONS}


def run_case(hip_em, case, data, dims, prepare=None, after_sequence=None):
    """{sequence: [[step, {option: value}], ...]} of one case: step "created", then one entry per option set.
    prepare(em) runs on every new context, after_sequence(em, sequence) once its last option is set."""
    k, l, env = case
    n_u, n_i, n_r = dims
    table = {}
    for name, steps in SEQUENCES.items():
        if env:
            os.environ[env] = "1"
        try:
            em = hip_em(data, k, l, n_u, n_i, n_r, swap_sides=0)
        finally:
            if env:
                del os.environ[env]
        with em:
            if prepare:
                prepare(em)
            rows = [["created", read_options(em)]]
            for option, value in steps:
                em.set_option(option, value)
                rows.append([f"{option}={value}", read_options(em)])
            if after_sequence:
                after_sequence(em, name)
        table[name] = rows
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import mmsbm_amd
    data, dims = make_data()
    table = {case_id(c): run_case(mmsbm_amd.HipEM, c, data, dims) for c in CASES}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as fh:     # one line per step
        cases = []
        for cid, seqs in table.items():
            body = ",\n".join(f'  "{name}": [\n' + ",\n".join("   " + json.dumps(row) for row in rows) + "\n  ]"
                              for name, rows in seqs.items())
            cases.append(f' "{cid}": {{\n{body}\n }}')
        fh.write("{\n" + ",\n".join(cases) + "\n}\n")
    print(f"{len(table)} cases from {os.path.dirname(mmsbm_amd.__file__)} -> {args.out}")


if __name__ == "__main__":
    main()
