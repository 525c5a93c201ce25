"""The C-ABI library loads and exports every symbol include/mmsbm_hip.h declares."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mmsbm_amd import _lib


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mmsbm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mmsbm_hip_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    names = declared_symbols()
    assert len(names) >= 20
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for nm in names:
        assert hasattr(lib, nm), f"{nm} declared in the header but not exported"
        assert nm in _lib.SIGNATURES, f"{nm} has no ctypes signature in mmsbm_amd/_lib.py"
    assert sorted(_lib.SIGNATURES) == names


C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
             "uint8_t": ctypes.c_uint8, "double": ctypes.c_double, "float": ctypes.c_float}


def ctype_of(decl):
    """The ctypes type of one C return or parameter declaration of the header (its name, if any, is dropped)."""
    decl = re.sub(r"\[\s*\d*\s*\]", " *", decl)                 # T name[k] is T *
    stars = decl.count("*")
    words = [w for w in decl.replace("*", " ").split() if w not in ("const", "struct", "unsigned")]
    base = words[0]
    if "unsigned" in decl.split():                              # (unsigned long long of the diagnostic build only)
        raise AssertionError(f"no mapping for {decl!r}")
    if base.startswith("mmsbm_hip_"):                           # an opaque handle
        assert stars in (1, 2), decl
        return ctypes.c_void_p if stars == 1 else ctypes.POINTER(ctypes.c_void_p)
    if base == "char":
        assert stars == 1, decl
        return ctypes.c_char_p
    assert stars <= 1, decl
    return ctypes.POINTER(C_SCALARS[base]) if stars else C_SCALARS[base]


def declared_prototypes():
    """{name: (restype, [argtypes])} of every prototype of include/mmsbm_hip.h."""
    text = open(os.path.join(ROOT, "include", "mmsbm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#[^\n]*(\\\n[^\n]*)*", "", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(mmsbm_hip_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        args = [] if params == "void" else [ctype_of(p) for p in params.split(",")]
        assert name not in out, f"{name} is declared twice"
        out[name] = (ctype_of(ret), args)
    return out


def test_ctypes_signatures_equal_the_header_position_by_position():
    """Every prototype of the header against _lib.SIGNATURES: the return type and each argument type, in order -- a
    miscounted or mistyped argument in a long signature shows here, without a GPU."""
    protos = declared_prototypes()
    assert sorted(protos) == declared_symbols() == sorted(_lib.SIGNATURES)
    assert len(protos) >= 106
    for name, (res, args) in protos.items():
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res, (name, "return", got_res, res)
        assert len(got_args) == len(args), (name, len(got_args), len(args))
        for pos, (got, want) in enumerate(zip(got_args, args)):
            assert got is want, (name, pos, got, want)


def test_abi_version_and_kernel_names():
    lib = _lib.load()
    assert lib.mmsbm_hip_abi_version() == 1
    n = lib.mmsbm_hip_kernel_count()
    names = [lib.mmsbm_hip_kernel_name(j).decode() for j in range(n)]
    assert n == 6 and names[0] == "seg_pass_kernel" and names[4] == "pairs_fused_kernel" and all(names)
    assert lib.mmsbm_hip_kernel_name(99) == b""


def test_no_device_means_loud_failure_not_fallback():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    from mmsbm_amd.core import HipEM
    data = np.array([[0, 0, 0], [1, 1, 1]], dtype=np.int64)
    with pytest.raises(_lib.HipLibraryError) as exc:
        HipEM(data, 2, 2)
    assert exc.value.code == _lib.E_NODEVICE
    with pytest.raises(ImportError):
        import mmsbm_amd.kernels_hip  # noqa: F401
    from mmsbm_amd import load_backend
    with pytest.raises(ImportError, match="Could not load any backend"):
        load_backend("auto")
    with pytest.raises(ImportError, match="Could not load any backend"):
        load_backend("numpy")  # this package has no numpy fallback


def test_nothing_thrown_crosses_the_abi():
    """whatever is thrown inside an entry point -- also a type that is not a std::exception --
    comes back as a status and a message, never as a dead process."""
    lib = _lib.load()
    assert lib.mmsbm_hip_selftest_throw(0) == _lib.OK
    for kind, code, text in ((1, _lib.E_INVALID, "invalid argument"), (2, _lib.E_INTERNAL, "runtime error"),
                             (3, _lib.E_INTERNAL, "allocation"), (4, _lib.E_INTERNAL, "unknown exception"),
                             (5, _lib.E_INTERNAL, "unknown exception")):
        assert lib.mmsbm_hip_selftest_throw(kind) == code
        assert text in lib.mmsbm_hip_last_error().decode()
    with pytest.raises(_lib.HipLibraryError, match="unknown exception"):
        _lib.call("mmsbm_hip_selftest_throw", 4)


def test_product_code_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "mmsbm_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("the oracle", ""), f


def _build_demo(tmp_path):
    import shutil, subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe = tmp_path / "abi_demo"
    lib_dir = os.path.join(ROOT, "mmsbm_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-O2",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "abi_demo.c"),
           "-o", str(exe), "-L" + lib_dir, "-lmmsbm_hip", "-Wl,-rpath," + lib_dir,
           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def test_header_is_plain_c99_and_demo_links(tmp_path):
    """include/mmsbm_hip.h compiles as pedantic C99 (-Werror) and a C program links against the
    library; without a GPU the program stops at the first call with the library's message."""
    import subprocess
    exe = _build_demo(tmp_path)
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: the run is checked by the gpu test")
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 1 and "mmsbm_hip_device_count" in run.stderr


def test_pcg64_stream_matches_numpy_at_any_offset():
    """The generator behind mmsbm_hip_init_params (device-side theta0 / eta0) against numpy's
    default_rng: same doubles, from the start and after a jump-ahead."""
    import numpy as np
    from mmsbm_amd.core import pcg64_doubles
    for seed in (0, 1, 12345, np.random.SeedSequence(1).spawn(3)[2]):
        want = np.random.default_rng(seed).random(5000)
        assert np.array_equal(pcg64_doubles(seed, 0, 5000), want)
        for off in (1, 7, 64, 1023, 4097):
            assert np.array_equal(pcg64_doubles(seed, off, 300), want[off:off + 300])
        big = 2_000_000_123                      # far beyond anything that is drawn sequentially here
        bg = np.random.PCG64(seed)
        bg.advance(big)
        assert np.array_equal(pcg64_doubles(seed, big, 64), np.random.Generator(bg).random(64))


def test_build_id_is_the_hash_of_the_sources_and_staleness_goes_by_content(tmp_path, monkeypatch):
    """bench.py and the tests must never measure a binary built from other sources than the tree
    holds.  The library carries mmsbm_hip_build_id() = the hash mmsbm_amd.build.source_id() computes over csrc/;
    is_stale() compares CONTENT (a sidecar with that hash next to the .so), not time stamps -- a copy of the tree
    does not keep those."""
    from mmsbm_amd import build
    assert _lib.build_id() == build.source_id() == build.built_id()
    assert not build.is_stale()
    # another set of sources (one byte more in a copy of csrc/): a different id, and the library counts as stale
    import shutil
    copy = tmp_path / "csrc"
    shutil.copytree(build.CSRC, copy)
    with open(copy / "common.hpp", "a") as fh:
        fh.write("\n")
    monkeypatch.setattr(build, "CSRC", str(copy))
    assert build.source_id() != _lib.build_id()
    assert build.is_stale()
    # touching a file without changing it does NOT make the library stale
    monkeypatch.undo()
    os.utime(os.path.join(build.CSRC, "common.hpp"))
    assert not build.is_stale()


def test_the_units_compile_as_one_with_the_diagnostic_switches():
    """csrc/unity.hip -- every translation unit as ONE, which the diagnostic builds (-DMMSBM_STAMPS, -DMMSBM_ABLATE) and
    scripts/kernel_resources.sh use -- goes through the compiler's front end for host and device (-fsyntax-only: no
    code generation, about ten seconds) with both switches on: the product never carries either, so nothing else in
    the suite would notice if that code rotted."""
    import subprocess
    from mmsbm_amd.build import CSRC, UNITS, hipcc_path
    with open(os.path.join(CSRC, "unity.hip")) as fh:
        text = fh.read()
    for unit in UNITS:                       # the list build.py compiles side by side is the list unity.hip includes
        assert f'#include "{unit}.hip"' in text, unit
    res = subprocess.run([hipcc_path(), "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-Wall",
                          "-Wno-unused-function", "-Wno-unused-command-line-argument", "-DMMSBM_STAMPS", "-DMMSBM_ABLATE",
                          os.path.join(CSRC, "unity.hip")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "warning" not in res.stderr, res.stderr[-3000:]


def test_the_product_has_no_ablation_switch_in_its_kernel_arguments():
    """VERDICT r5 (weak 8): `abl` exists only under -DMMSBM_ABLATE."""
    import re
    from mmsbm_amd.build import CSRC
    for name in ("pair_block.hpp", "eta_p.hpp", "context.hpp", "mmsbm_hip.hip", "tu_iterate.hip"):
        with open(os.path.join(CSRC, name)) as fh:
            text = fh.read()
        # every line that mentions the switch sits between `#ifdef MMSBM_ABLATE` and its `#else` / `#endif`,
        # or is the compile-time zero of the product
        inside, bad = False, []
        for ln in text.splitlines():
            if ln.startswith("#ifdef MMSBM_ABLATE"):
                inside = True
            elif inside and ln.startswith(("#else", "#endif")):
                inside = False
            elif not inside and re.search(r"\b(pa|a|c|ctx)(\.|->)(abl|ablate)\b", ln):
                bad.append(ln)
        assert not bad, (name, bad)
