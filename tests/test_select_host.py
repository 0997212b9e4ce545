"""The transport kernel selection (jaybenne_amd/csrc/jb_select.hpp) without a GPU: tests/select_test.cpp walks
select_transport and variant_name over every threshold with a host compiler, once plainly and once under the
address and undefined-behaviour sanitizers (a stand-alone program: the name buffer is what they watch)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "sanitized"])
def test_selection_truth_table_on_the_host(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "select_test")
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *sanitize,
                          os.path.join(ROOT, "tests", "select_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout + run.stderr
