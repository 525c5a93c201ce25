"""Seeded random walks through the HipEM surface on the device (tests/api_walk.py): after every step that observes
something, the result against the oracle -- within the bounds check_step_and_loop, the parity tests and the held-out
and recommend files already hold -- and, bit for bit, against a canonical replay in a fresh context.

The shapes are the smallest at which each family of state exists (the recipes of test_gpu_heldout.py; `skewed`: the one
busy user of test_two_launch_iteration_is_chosen_by_size_and_refused_where_it_does_not_apply); every shape starts with 3
slots and three to six walks of 64 operations or a few more (api_walk.SEEDS, whose reach test_api_walk_cpu.py asserts).
Measured on an MI355X: 0.2 to 0.7 s a walk, 1.0 to 1.7 s a shape, 11 s for the 36 walks.  The
file runs as one process, in order; a failing walk prints itself as a literal for api_walk.run -- nothing is re-run.
"""
import time

import pytest

import api_walk
from test_gpu_recommend import LaunchWindow, hip  # noqa: F401  (hip: the module fixture)

pytestmark = pytest.mark.gpu

WINDOWS, NAMES, TIMES = {}, {}, {}


@pytest.mark.parametrize("shape,seed", api_walk.CASES, ids=[f"{sh}-{sd}" for sh, sd in api_walk.CASES])
def test_walk(hip, shape, seed):
    WINDOWS.setdefault(shape, LaunchWindow().__enter__())
    ops = api_walk.walk(seed, shape)
    assert len(ops) >= 40
    t0 = time.perf_counter()
    try:
        done = api_walk.run(hip, shape, ops, seed)
    except api_walk.WalkFailure as exc:
        if exc.fault:                       # a HIP runtime error: nothing more runs on the device in this process
            pytest.exit(f"HIP runtime error in a walk; the run ends here.\n{exc}", returncode=1)
        raise
    TIMES[(shape, seed)] = time.perf_counter() - t0
    print(f"{shape} seed {seed}: {done['ops']} operations, {done['checks']} checks, {TIMES[(shape, seed)]:.2f} s")
    assert done["ops"] == len(ops) and done["checks"] >= 40
    if seed == api_walk.SEEDS[shape][-1] and WINDOWS[shape].path:      # the shape's walks are over: what they launched
        NAMES[shape] = WINDOWS[shape].names()


def test_the_toggles_took_effect():
    """The launch log of the walks above: the `fused` shape ran both forms of the iteration, `matrix_core` the
    matrix-core pair stage."""
    if "fused" not in WINDOWS or "matrix_core" not in WINDOWS:
        pytest.fail("the walks of this file have not run in this process")
    if not NAMES:
        LaunchWindow().names()              # (skips, as everywhere, where the launch log is switched off)
    names = NAMES["fused"]
    assert [n for n in names if "_fused_kernel" in n], sorted(names)
    assert [n for n in names if n.startswith(("seg_pass_kernel", "seg_pass_slots_kernel"))], sorted(names)
    assert [n for n in NAMES["matrix_core"] if n.startswith("pair_mfma_kernel")], sorted(NAMES["matrix_core"])
    if TIMES:
        print("wall time per shape:", {sh: round(sum(t for (s, _), t in TIMES.items() if s == sh), 2)
                                       for sh in api_walk.SHAPES}, "total", round(sum(TIMES.values()), 2))
