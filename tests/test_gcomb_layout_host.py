"""Where the global comb keeps its arrays in the library's scratch memory (jaybenne_amd/csrc/jb_scratch_layout.hpp:
gcomb_layout) without a GPU: tests/gcomb_layout_test.cpp -- a stand-alone program -- holds its offsets, that nothing
overlaps and that everything the comb's layout has stays where comb_layout puts it, once plainly and once under the
address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


@pytest.mark.parametrize("sanitize", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "sanitized"])
def test_gcomb_layout_on_the_host(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "gcomb_layout_test")
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *sanitize,
                          os.path.join(ROOT, "tests", "gcomb_layout_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout + run.stderr


def test_the_gcomb_header_is_a_dependency_of_the_library():
    text = open(os.path.join(ROOT, "jaybenne_amd", "csrc", "Makefile")).read()
    hdr = next(line for line in text.splitlines() if line.startswith("HDR"))
    assert "jb_kernel_gcomb.hpp" in hdr.split()
