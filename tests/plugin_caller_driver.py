"""Child process of tests/test_plugin_caller_cpu.py: a caller that resolves the HIP backend the way the reference's
``load_backend`` does (``import_module("kernels_" + name)`` with mmsbm_amd/plugin on PYTHONPATH) and runs its
``fit`` -> ``predict`` -> ``score`` order -- each restart in a worker of ``Pool(processes=sampling)`` from a spawn
context, which imports ``kernels_hip`` afresh -- restated here with the oracle's start and scores (nothing of the
reference is imported).  tests/fake_site puts the oracle-backed stand-in behind ``mmsbm_amd.core.HipEM`` in every
process, the spawned workers included."""
import multiprocessing
import os
import sys
from importlib import import_module

import numpy as np

EPS = np.finfo(float).eps


def backend():
    return import_module("kernels_" + "hip")


def run_restart(task):
    """One restart in a worker: the three callables of the freshly imported plugin, the numpy normalisations."""
    train, theta, eta, pr, d_u, d_i, iterations = task
    kernels_hip = backend()
    for _ in range(iterations):
        n_theta, n_eta, n_pr = kernels_hip.update_coefficients(train, theta, eta, pr)
        theta = n_theta / d_u[:, None]
        eta = n_eta / d_i[:, None]
        s = n_pr.sum(axis=2, keepdims=True)
        s[s == 0] = 1
        pr = n_pr / s
    om = kernels_hip.compute_omegas(train, theta, eta, pr)
    w = np.maximum(om, EPS)
    tot = np.maximum(om.sum(axis=(1, 2)), EPS)
    lik = float(np.sum(w * np.log(w) - w * np.log(tot)[:, None, None]))
    owners = sorted({f.__module__ for f in (kernels_hip.compute_omegas, kernels_hip.update_coefficients,
                                            kernels_hip.prod_dist)})
    return {"theta": theta, "eta": eta, "pr": pr, "likelihood": lik, "pid": os.getpid(),
            "plugin_file": os.path.abspath(kernels_hip.__file__), "kernel_modules": owners}


def main(golden, out_path, k, l, sampling, seed):
    from oracle import mmsbm_oracle as orc
    g = np.load(golden)
    train, test = g["train"], g["test"]
    n_u, n_i, n_r = (int(train[:, j].max()) + 1 for j in range(3))
    d_u, d_i = orc.degrees(train, n_u, n_i)
    tasks = []
    for child in orc.child_seeds(seed, sampling):
        theta, eta, pr = orc.init_params(child, n_u, n_i, n_r, k, l, d_u, d_i)
        tasks.append((train, theta, eta, pr, d_u.astype(np.float64), d_i.astype(np.float64), 10))
    kernels_hip = backend()      # the parent resolves the backend too
    with multiprocessing.get_context("spawn").Pool(processes=sampling, maxtasksperchild=1) as pool:
        res = pool.map(run_restart, tasks, chunksize=1)
    pm = sum(kernels_hip.prod_dist(test, r["theta"], r["eta"], r["pr"]) for r in res) / sampling
    best = res[int(np.argmax([r["likelihood"] for r in res]))]
    stats = orc.score_stats(pm, test[:, 2], list(range(n_r)))
    stats["likelihood"] = best["likelihood"]
    out = {"prediction_matrix": pm, "stats_keys": np.array(list(stats)),
           "stats_vals": np.array([float(v) for v in stats.values()]),
           "likelihoods": np.array([r["likelihood"] for r in res]), "pids": np.array([r["pid"] for r in res]),
           "pid": np.array(os.getpid()), "plugin_files": np.array([r["plugin_file"] for r in res]),
           "kernel_modules": np.array(sorted({m for r in res for m in r["kernel_modules"]}))}
    for s, r in enumerate(res):
        out[f"theta_{s}"], out[f"eta_{s}"], out[f"pr_{s}"] = r["theta"], r["eta"], r["pr"]
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], *(int(x) for x in sys.argv[3:7]))
