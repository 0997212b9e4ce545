"""k_imc_cell's unit-cell form without a GPU.

* tests/unit_cell_select_test.cpp walks `select_transport` (jaybenne_amd/csrc/jb_select.hpp) over every combination of
  the inputs that bear on the new plan fields, once plainly and once under the address and undefined-behaviour
  sanitizers (a stand-alone program): `unit_cell` exactly on a gray IMC call in lean arithmetic on a uniform mesh with
  power-of-two widths that the cell-local kernel takes, and `variant_name` the same with or without it.
* the kernel the headline mesh then runs, `k_imc_cell_unit<3, true, true, true>`, in the gfx950 assembly of the library's own source file:
  at most 128 vector registers and no scratch memory (four waves per SIMD), as tests/test_cabi.py asks of
  `k_imc_cell<3, true, true, true>`; the same for the other forms a mesh can select.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "sanitized"])
def test_unit_cell_selection_on_the_host(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "unit_cell_select_test")
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *sanitize,
                          os.path.join(ROOT, "tests", "unit_cell_select_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout + run.stderr


def _makefile_flags():
    """The library's own compile flags, as its Makefile states them (`make print-flags`)."""
    res = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "jaybenne_amd", "csrc"), "print-flags", "ARCH=gfx950"],
                         capture_output=True, text=True)
    assert res.returncode == 0 and "--offload-arch=gfx950" in res.stdout, res.stdout + res.stderr
    return [f for f in res.stdout.split() if f not in ("-fPIC", "-Wall")]


# NDIM, TALLY, NOABS, EQUALH: the headline form first; unequal widths; an absorbing material; 2-D; 1-D
FORMS = ["3, true, true, true", "3, true, true, false", "3, true, false, true", "3, true, false, false",
         "2, true, true, true", "2, true, true, false", "1, true, true, true"]


def test_unit_cell_kernels_keep_four_waves_per_simd(tmp_path):
    """The library's own translation unit to gfx950 assembly, as tests/test_cabi.py compiles it: the register count and
    scratch use of every k_imc_cell_unit a launch can select, read from the kernel descriptors."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / "jb.s"
    res = subprocess.run([hipcc] + _makefile_flags() + ["-S", "--cuda-device-only",
                                                        os.path.join(ROOT, "jaybenne_amd", "csrc", "jb_api.hip"),
                                                        "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = out.read_text()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        name, body = m.group(1), m.group(2)
        if "k_imc_cell_unit" in name:
            found[name] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))
    # NDIM, TALLY, NOABS, EQUALH as the mangled names spell them
    for form in FORMS:
        n, t, a, e = [f.strip() for f in form.split(",")]
        key = "k_imc_cell_unitILi%sE%sE" % (n, "E".join("Lb%d" % (v == "true") for v in (t, a, e)))
        names = [k for k in found if key in k]
        assert len(names) == 1, (form, key, sorted(found))
        vgpr, scratch = found[names[0]]
        print(f"k_imc_cell_unit<{form}>: {vgpr} vector registers, {scratch} bytes of scratch")
        assert vgpr <= 128 and scratch == 0, (form, vgpr, scratch)
