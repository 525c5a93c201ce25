"""The plugin (``mmsbm_amd/plugin/kernels_hip.py``) under the reference's calling convention, without a GPU.

A child process (tests/plugin_caller_driver.py) with ``mmsbm_amd/plugin`` and ``tests/fake_site`` on PYTHONPATH
resolves the backend the way the reference's ``load_backend('hip')`` does (``import_module("kernels_hip")``), runs
every restart in a spawned ``Pool(processes=sampling)`` worker that imports the plugin afresh, then predicts through
the plugin's ``prod_dist`` and scores.  ``tests/fake_site`` puts the oracle-backed stand-in behind
``mmsbm_amd.core.HipEM`` in every process.  The numbers must be those of fixtures G1 / G2, which the reference's own
class produced (tests/golden/make_golden.py)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PLUGIN = os.path.join(ROOT, "mmsbm_amd", "plugin")


def run_caller(tmp_path, golden, k, l, sampling, seed=1):
    out = tmp_path / "out.npz"
    log = tmp_path / "pids.log"
    env = dict(os.environ)
    env.update(PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests", "fake_site"), PLUGIN, ROOT]),
               PYTHONDONTWRITEBYTECODE="1", MMSBM_FAKE_SITE_ROOT=ROOT, MMSBM_FAKE_SITE_LOG=str(log))
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plugin_caller_driver.py"),
                           os.path.join(GOLD, golden + ".npz"), str(out), str(k), str(l), str(sampling), str(seed)],
                          cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout + done.stderr
    pids = [int(x) for x in log.read_text().split()]
    return np.load(out), pids


def _common(got, pids, sampling):
    # the callables are this repo's, reached through the plugin file, in fresh interpreters with the stand-in installed
    assert list(got["plugin_files"]) == [os.path.join(PLUGIN, "kernels_hip.py")] * sampling
    assert list(got["kernel_modules"]) == ["mmsbm_amd.kernels_hip"]
    workers = set(int(p) for p in got["pids"])
    assert len(workers) == sampling and int(got["pid"]) not in workers
    assert int(got["pid"]) in pids and workers <= set(pids)


def test_the_plugin_in_a_spawned_worker_gives_g1(tmp_path):
    got, pids = run_caller(tmp_path, "g1_c1_mock", 2, 2, 1)
    g = np.load(os.path.join(GOLD, "g1_c1_mock.npz"))
    _common(got, pids, 1)
    for name in ("theta", "eta", "pr"):
        assert np.array_equal(got[name + "_0"], g["t_" + name]), name
    assert float(got["likelihoods"][0]) == float(g["t_likelihood"])
    assert np.array_equal(got["prediction_matrix"], g["t_prediction_matrix"])
    assert list(got["stats_keys"]) == list(g["t_stats_keys"])
    assert np.array_equal(got["stats_vals"], g["t_stats_vals"])


def test_three_restarts_in_three_spawned_workers_give_g2(tmp_path):
    got, pids = run_caller(tmp_path, "g2_c1_sampling3", 2, 2, 3)
    g = np.load(os.path.join(GOLD, "g2_c1_sampling3.npz"))
    _common(got, pids, 3)
    assert len(set(pids)) >= 4                                              # parent + Pool(processes=3)
    for s in range(3):
        for name in ("theta", "eta", "pr"):
            assert np.array_equal(got[f"{name}_{s}"], g[f"{name}_{s}"]), (name, s)
    assert np.array_equal(got["likelihoods"], g["likelihoods"])
    assert np.array_equal(got["prediction_matrix"], g["prediction_matrix"])
