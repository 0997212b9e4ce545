"""The checked library (make -C jaybenne_amd/csrc checked) without a GPU: the transport-invariant predicates
of jb_invariants.hpp on hand-written states (tests/invariants_test.cpp, host compiler), the checked and the
release library's answers to the three invariant entry points, and the release code object without any of
the checked build's kernels."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jaybenne_amd", "csrc")
RELEASE = os.path.join(ROOT, "jaybenne_amd", "libjaybenne_amd.so")
CHECKED = os.path.join(ROOT, "jaybenne_amd", "libjaybenne_amd_checked.so")
# names only the checked build has: its two sweep kernels and its counting buffer
CHECK_SYMBOLS = (b"k_inv_swarm", b"k_inv_ddmc_class", b"jb_inv_buf")


def _make(target):
    """make <target> in jaybenne_amd/csrc (one translation unit: ~3 min when it has to compile)."""
    res = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True, timeout=1200)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]


@pytest.fixture(scope="module")
def libraries():
    _make("all")
    _make("checked")
    return RELEASE, CHECKED


def test_predicates_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "invariants_test")
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                          os.path.join(ROOT, "tests", "invariants_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout + run.stderr


_PROBE = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from jaybenne_amd import _lib
lib = _lib.load()
r = _lib.InvariantReport()
print(json.dumps({"path": _lib.LIB_PATH, "enabled": lib.jb_invariants_enabled(),
                  "report": lib.jb_invariant_report_get(None, C.byref(r), 0),
                  "verify": lib.jb_verify_swarm(None, None, None, 0.0, 1.0, None),
                  "error": lib.jb_last_error().decode()}))
"""


def _probe(path):
    """The three entry points, asked in a child process that loads `path` through JAYBENNE_AMD_LIB."""
    env = dict(os.environ, JAYBENNE_AMD_LIB=path)
    res = subprocess.run([sys.executable, "-c", _PROBE, ROOT], capture_output=True, text=True, env=env,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-4000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_checked_library_reports_enabled(libraries):
    from jaybenne_amd import _lib
    got = _probe(CHECKED)
    assert got["path"] == CHECKED
    assert got["enabled"] == 1
    # (a null context is an argument error in the checked build)
    assert got["report"] == _lib.JB_ERR_INVALID and got["verify"] == _lib.JB_ERR_INVALID


def test_release_library_has_no_checks(libraries):
    from jaybenne_amd import _lib
    got = _probe(RELEASE)
    assert got["enabled"] == 0
    assert got["report"] == _lib.JB_ERR_UNSUPPORTED and got["verify"] == _lib.JB_ERR_UNSUPPORTED
    assert "checked" in got["error"]


def _llvm_tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    tool = shutil.which(name)
    assert tool, f"{name} (ROCm's LLVM) is needed"
    return tool


def _code_object(lib, tmp_path):
    """The gfx950 code object embedded in a library: its .hip_fatbin section, unbundled."""
    base = tmp_path / os.path.basename(lib)
    fatbin, co = str(base) + ".fatbin", str(base) + ".gfx950.co"
    res = subprocess.run([_llvm_tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fatbin}", lib, str(base) + ".o"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fatbin}",
                          "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and os.path.getsize(co) > 0, res.stderr
    return open(co, "rb").read()


def test_release_code_object_has_none_of_the_check_kernels(libraries, tmp_path):
    release = _code_object(RELEASE, tmp_path)
    checked = _code_object(CHECKED, tmp_path)
    for name in CHECK_SYMBOLS:
        assert name in checked, name        # (the search finds them where they exist)
        assert name not in release, name
