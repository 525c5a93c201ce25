"""The serving side's build rule, read from csrc/ as text: one unit per query family behind serve_frame.hpp, and every
kernel of the serving headers launched from exactly one unit."""
import os
import re

from mmsbm_amd import build

SERVING_UNITS = ("tu_serve_frame", "tu_recommend", "tu_rerank", "tu_pairs", "tu_market", "tu_similar")


def read(name):
    with open(os.path.join(build.CSRC, name)) as fh:
        return fh.read()


def code(text):
    """The text without its // comments: a comment may name a kernel or a macro, only code uses one."""
    return re.sub(r"//[^\n]*", "", text)


def includes(text):
    return re.findall(r'^#include "([a-z_0-9]+\.hpp)"', text, flags=re.M)


def kernels(header_text):
    """The __global__ names a header defines."""
    return re.findall(r"__global__\s+(?:__launch_bounds__\s*\((?:[^()]|\([^()]*\))*\)\s*)?void\s+(\w+)\s*\(",
                      code(header_text))


def test_the_frame_header_launches_nothing_and_includes_no_kernel_header():
    text = read("serve_frame.hpp")
    assert "LAUNCH(" not in text
    for header in includes(text):
        assert not kernels(read(header)), header


def test_every_serving_kernel_is_launched_from_exactly_one_unit():
    """The headers are those the six serving units and tu_explain.hip include.  A unit launches a kernel where its code
    (comments apart) names it: that covers `LAUNCH(<name>`, `LAUNCH((<name><` and the instantiations a unit hands to a
    generic launching lambda (`tile(grp_tile_kernel<kGrpMin>)`), and it asks more than a search for the macro alone
    would -- a kernel is not even named in a second unit."""
    hips = {f: code(read(f)) for f in os.listdir(build.CSRC) if f.endswith(".hip") and f != "unity.hip"}
    headers = sorted({h for u in SERVING_UNITS + ("tu_explain",) for h in includes(read(u + ".hip"))})
    names = {k: h for h in headers for k in kernels(read(h))}
    assert len(names) > 60, len(names)           # (the serving headers hold some ninety kernels)
    for must in ("rec_w_kernel", "rec_fold_kernel", "rec_select_kernel", "cat_exclude_kernel", "grp_tile_kernel", "sim_mass_kernel"):
        assert must in names, must
    for kernel, header in sorted(names.items()):
        users = sorted(f for f, text in hips.items() if re.search(r"\b%s\b" % kernel, text))
        assert len(users) == 1, (header, kernel, users)
    # what several families share is the frame unit's
    for kernel in ("rec_w_kernel", "rec_fold_kernel", "rec_score_kernel", "rec_exclude_kernel", "rec_select_kernel",
                   "cat_exclude_kernel", "cat_gather_kernel", "cat_cols_kernel"):
        assert re.search(r"\bLAUNCH\(\(?%s\b" % kernel, hips["tu_serve_frame.hip"]), kernel


def test_the_units_on_disk_are_the_units_the_build_compiles():
    on_disk = sorted(f[:-4] for f in os.listdir(build.CSRC) if f.endswith(".hip") and f != "unity.hip")
    assert on_disk == sorted(build.UNITS)
    assert len(set(build.UNITS)) == len(build.UNITS)


def test_the_recommend_unit_includes_only_its_own_kernel_headers():
    mine = includes(read("tu_recommend.hip"))
    for other in ("similar", "overlap", "top_pairs", "pairs_bulk", "audience", "allocate", "assign", "assortment", "inform",
                  "explore", "ensemble", "group", "diverse"):
        assert other + ".hpp" not in mine, other
    for unit in SERVING_UNITS[1:]:               # every query unit starts from the prelude and the frame
        assert includes(read(unit + ".hip"))[:2] == ["prelude.hpp", "serve_frame.hpp"], unit


def test_a_request_crosses_into_the_units_as_values():
    """The runs of loose pointers and counts end at the C ABI: as function parameters -- a type, the name,
    then `,` or `)` -- their spellings occur in mmsbm_hip.hip (the ABI's own signatures) and in the two factory
    functions of abi_request.hpp (user_query, theta_query), nowhere else under csrc/.  serve_plan.hpp stands alone for
    its native dump programs and keeps plain arguments (n_cand, cat_off); the kernel headers are not host seams (one
    kernel of diverse.hpp names an argument n_cand)."""
    names = r"(?:int(?:32_t)?\s+n_cand|\*\s*(?:excl_offsets|seen_offsets|cat_offsets|list_offsets))\s*[,)]"
    factories = r"inline \w+Query (?:user|theta)_query\([^)]*\)"
    found = {}
    for f in sorted(os.listdir(build.CSRC)):
        if not f.endswith((".hip", ".hpp")) or f in ("mmsbm_hip.hip", "unity.hip"):
            continue
        text = code(read(f))
        if kernels(read(f)):                     # (a kernel header: device code, where a kernel names its own arguments)
            continue
        if f == "abi_request.hpp":
            assert len(re.findall(factories, text)) == 2
            text = re.sub(factories, "", text)
        if f == "serve_plan.hpp":
            text = re.sub(r"int(?:32_t)?\s+n_cand\s*[,)]", "", text)
        hits = re.findall(names, text)
        if hits:
            found[f] = hits
    assert not found, found
    assert re.search(names, code(read("mmsbm_hip.hip")))     # (the pattern does find the ABI's signatures)
    for f in os.listdir(build.CSRC):
        if f.endswith(".hip"):
            assert "offsets_of(" not in code(read(f)), f
    for f in os.listdir(build.CSRC):
        assert "QuotaCats" not in read(f), f
    assert "AssignOut" in code(read("abi_request.hpp"))
    assert not re.search(r"struct\s+AssignOut", code(read("launch.hpp")))


def test_the_build_runs_no_more_compilers_than_the_job_may_use(monkeypatch):
    """MAX_JOBS, then CMAKE_BUILD_PARALLEL_LEVEL, cap the compilers build_library starts side by side when set to a
    positive integer; anything else leaves the machine's core count in charge."""
    n = len(build.UNITS)
    monkeypatch.setattr(os, "cpu_count", lambda: 192)
    monkeypatch.delenv("MAX_JOBS", raising=False)
    monkeypatch.delenv("CMAKE_BUILD_PARALLEL_LEVEL", raising=False)
    assert build.build_workers(n) == n
    monkeypatch.setenv("CMAKE_BUILD_PARALLEL_LEVEL", "5")
    assert build.build_workers(n) == 5
    monkeypatch.setenv("MAX_JOBS", "3")
    assert build.build_workers(n) == 3           # (MAX_JOBS first)
    assert build.build_workers(2) == 2
    for junk in ("0", "-4", "many", ""):
        monkeypatch.setenv("MAX_JOBS", junk)
        assert build.build_workers(n) == 5, junk  # (not a positive integer: the next one decides)
    monkeypatch.delenv("CMAKE_BUILD_PARALLEL_LEVEL")
    assert build.build_workers(n) == n
    monkeypatch.setattr(os, "cpu_count", lambda: None)
    assert build.build_workers(n) == 1
