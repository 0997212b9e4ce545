"""The radiation spectrum on the CPU (tests/spectrum_model.py: a numpy restatement of include/jaybenne_amd.h,
jb_evaluate_radiation_spectrum): counts that show the crafted swarms of tests/test_gpu_spectrum.py hold what they claim,
the equivalence of skipping a photon and adding +0.0, the one-group spectrum against the moments model's E, the table of
edges the library must refuse, the series of the Planck law, and the library's symbols."""
import os
import re

import numpy as np
import pytest

import moments_model as mm
import spectrum_model as sm
import swarm_ops_model as som
from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "jaybenne_amd.h")
SPECTRUM_SYMBOLS = ("jb_spectrum_words", "jb_evaluate_radiation_spectrum", "jb_evaluate_radiation_spectrum_host")

# what the library must refuse: (name, edges or None, ngroups)
BAD_EDGES = [
    ("unsorted", [1.0, 3.0, 2.0, 4.0], 3),
    ("equal neighbours", [1.0, 2.0, 2.0, 4.0], 3),
    ("decreasing pair", [2.0, 1.0], 1),
    ("NaN", [1.0, float("nan"), 3.0], 2),
    ("inf", [1.0, 2.0, float("inf")], 2),
    ("-inf", [float("-inf"), 2.0, 3.0], 2),
    ("ngroups 0", [1.0], 0),
    ("ngroups 65", list(range(1, 67)), 65),
    ("ngroups -1", [1.0], -1),
]


@pytest.fixture(scope="module")
def geoms():
    return {name: som.host_view(case)[1] for name, case in mm.mesh_cases().items()}


# ---- the bins -----------------------------------------------------------------------------------------
def test_the_bin_rule_on_edges_and_odd_values():
    edges = sm.edges_for(7)
    ng = 7
    assert sm.check_edges(edges)
    assert sm.bins(edges, edges).tolist() == list(range(1, ng + 2))                     # on edge j: bin j + 1
    assert sm.bins(edges, np.nextafter(edges, -np.inf)).tolist() == list(range(0, ng + 1))
    assert sm.bins(edges, np.nextafter(edges, np.inf)).tolist() == list(range(1, ng + 2))
    odd = sm.SPECIALS
    assert np.isnan(odd[-2:]).all() and odd[-2:].view(np.uint64).tolist() == [0x7FF8000000C0FFEE, 0xFFF400000000BEEF]
    assert np.signbit(odd[1]) and odd[1] == 0 and 0 < odd[2] < 2.3e-308
    # NaN, negative, zero, -inf: below; +inf: above
    assert sm.bins(edges, odd).tolist() == [0, 0, 0, 0, 0, ng + 1, 0, 0, 0]
    # the widest edges take every positive finite double into bin 1, the smallest denormal included
    e = np.array([4.9e-324, 1.0, np.finfo(np.float64).max, 0.0, np.inf])
    assert sm.bins(sm.WIDEST, e).tolist() == [1, 1, 2, 0, 2]


@pytest.mark.parametrize("name,edges,ngroups", BAD_EDGES, ids=[b[0] for b in BAD_EDGES])
def test_bad_edges_are_not_edges(name, edges, ngroups):
    from jaybenne_amd import _lib
    assert len(edges) == max(ngroups, 0) + 1 and not sm.check_edges(edges)
    lib = _lib.load()
    if not 1 <= ngroups <= sm.MAX_GROUPS:
        assert lib.jb_spectrum_words(None, ngroups) == 0
    # without a context nothing can be evaluated: null pointers are turned down first
    arr = np.asarray(edges, dtype=np.float64)
    for f in (lib.jb_evaluate_radiation_spectrum, lib.jb_evaluate_radiation_spectrum_host):
        assert f(None, None, None, arr.ctypes.data, ngroups, None, None) == _lib.JB_ERR_INVALID


def test_good_edges_are_edges():
    for ng in sm.NGROUPS:
        edges = sm.edges_for(ng)
        assert len(edges) == ng + 1 and sm.check_edges(edges)
        assert len(set(np.diff(edges).tolist())) == ng                 # no two widths alike: no formula to invert
    assert sm.check_edges(sm.WIDEST) and sm.WIDEST[0] == 5e-324


# ---- the sums -----------------------------------------------------------------------------------------
def _run(L, ng, salt):
    ids = som._hash(np.arange(L), salt) >> np.uint64(1)
    sw = sm.craft_e(mm._physical({"id": ids}, salt), sm.edges_for(ng), salt)
    return sw["w"], sm.bins(sm.edges_for(ng), sw["e"])


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 700, 4096, 4097, 2 * 4096 + 1])
def test_skipping_equals_adding_plus_zero(L):
    """per bin: walking the run and adding only the bin's photons gives the bits of adding +0.0 for all the others"""
    for ng in (1, 7, 64):
        w, b = _run(L, ng, 17 + L + ng)
        assert mm.same_bits(sm.run_sums(w, b, ng + 2), sm.run_sums_skipping(w, b, ng + 2)), (L, ng)


def test_a_bin_without_photons_is_plus_zero_and_the_order_shows():
    w, b = _run(4097, 2, 5)
    b = np.where(b == 3, 2, b)                                          # nothing above
    s = sm.run_sums(w, b, 4)
    assert s[3] == 0.0 and not np.signbit(s[3])
    # another order gives other bits in a bin that holds 60 binary orders of w
    sel = b == 1
    assert sel.sum() > 500 and np.log2(w[sel].max() / w[sel].min()) > 59
    assert s[1] != np.add.accumulate(w[sel])[-1] or s[2] != np.add.accumulate(w[b == 2])[-1]


def test_one_group_with_the_widest_edges_is_the_moments_e(geoms):
    """ngroups = 1, edges {4.9e-324, DBL_MAX}, every e positive and finite: bin 1 is the moments model's E bit for
    bit, bins 0 and 2 are +0.0"""
    g = geoms["2d"]
    sw, _ = mm.run_swarm(g, [65, 4097, 1, 2 * mm.CHUNK + 1, 64, 700, 2, 63])
    n = len(sw["id"])
    sw = mm.canonical(g, sw, n)
    sw["e"] = np.ldexp(1.0 + som._unit(sw["id"], 3), (som._mod(sw["id"], 4, 2000) - 1000).astype(np.int32))
    sw["e"][::501] = 4.9e-324
    assert np.all(sw["e"] > 0) and np.all(np.isfinite(sw["e"]))
    spec, rep = sm.spectrum(g, sw, n, sm.WIDEST)
    fields, mrep = mm.moments(g, sw, n)
    assert mm.same_bits(spec[1], fields[1]) and not spec[0].any() and not spec[2].any()
    assert rep == dict(mrep, n_below=0, n_above=0) and rep["n_counted"] > 10000


# ---- the crafted swarms hold what they claim ---------------------------------------------------------------
def test_run_plans_hold_every_case(geoms):
    """per plan: the report's counts; per cell and bin the number of photons; every bin occupied in one chunk of one
    run (short plans: over the plan); photons on every edge and one ulp either side of it, and every special value,
    among the counted ones"""
    seen_groups = {}
    for p, (name, mesh, lengths) in enumerate(mm.run_plans()):
        g = geoms[mesh]
        ng = sm.plan_groups(p)
        nb = ng + 2
        edges = sm.edges_for(ng)
        sw, cells = sm.run_swarm(g, lengths, edges)
        n = len(sw["id"])
        assert not mm.in_order(g, sw, n), name
        srt = mm.canonical(g, sw, n)
        key = som.sort_key(g, srt, n)
        counted = key < g.nkeys
        assert int((~counted).sum()) == mm.EXTRAS
        b = sm.bins(edges, srt["e"])
        e = srt["e"][counted]
        spec, rep = sm.spectrum(g, srt, n, edges)
        assert rep["n_counted"] == sum(lengths) and rep["n_skipped"] == mm.EXTRAS and rep["longest_run"] == max(lengths)
        assert rep["n_below"] == int((b[counted] == 0).sum()) and rep["n_above"] == int((b[counted] == nb - 1).sum())
        assert rep["n_below"] > 0 and rep["n_above"] > 0
        # per cell and bin: a bin is nonzero exactly where it holds a photon (w > 0 everywhere)
        flat = spec.reshape(nb, -1)
        count = np.zeros((nb, flat.shape[1]), dtype=np.int64)
        np.add.at(count, (b[counted], np.repeat(cells, lengths)), 1)
        assert np.array_equal(count.sum(0)[cells], np.asarray(lengths)) and np.array_equal(flat > 0, count > 0)
        if max(lengths) >= 4095:                                    # one chunk of one run holds every bin
            head = int(np.flatnonzero(counted & (np.concatenate(([True], key[1:] != key[:-1]))))[np.argmax(lengths)])
            assert set(b[head:head + min(max(lengths), mm.CHUNK)].tolist()) == set(range(nb)), (name, ng)
        else:
            assert set(b[counted].tolist()) == set(range(nb)), (name, ng)
        if sum(lengths) > 10000:
            for j in range(ng + 1):
                for v in (edges[j], np.nextafter(edges[j], -np.inf), np.nextafter(edges[j], np.inf)):
                    assert (e == v).any(), (name, j)
            bits = set(e.view(np.uint64).tolist())
            assert set(sm.SPECIALS.view(np.uint64).tolist()) <= bits, name
        seen_groups.setdefault(ng, set()).add(max(lengths) > mm.CHUNK)
    assert set(seen_groups) == set(sm.NGROUPS)
    assert all(True in v for v in seen_groups.values())             # every width meets a run of several chunks
    # w spans 60 binary orders within one bin of the one-cell run
    name, mesh, lengths = mm.run_plans()[-1]
    assert lengths == [mm.ONE_CELL]
    ng = sm.plan_groups(len(mm.run_plans()) - 1)
    sw, _ = sm.run_swarm(geoms[mesh], lengths, sm.edges_for(ng))
    act = (sw["status"] == som.ST_ACTIVE) & (sw["blk"] >= 0) & (sw["blk"] < geoms[mesh].nblocks)
    b = sm.bins(sm.edges_for(ng), sw["e"])
    spans = [np.log2(sw["w"][act & (b == q)].max() / sw["w"][act & (b == q)].min()) for q in range(ng + 2)]
    assert max(spans) > 59, spans


def test_hashed_swarms_and_halo_copies(geoms):
    g = geoms["3d"]
    edges = sm.edges_for(7)
    sw = mm.canonical(g, sm.hashed_swarm(g, 6000, edges), 6000)
    spec, rep = sm.spectrum(g, sw, 6000, edges)
    _, mrep = mm.moments(g, sw, 6000)
    assert {k: rep[k] for k in mrep} == mrep and 0 < rep["n_below"] < rep["n_counted"] and rep["n_above"] > 0
    _, h = som.host_view(som.RANK_MESH, 1, 2)
    sw = mm.canonical(h, sm.hashed_swarm(h, 3000, edges), 3000)
    spec, rep = sm.spectrum(h, sw, 3000, edges)
    assert h.nowned < h.nblocks and not spec[:, h.nowned:].any() and spec[:, :h.nowned].any() and rep["n_counted"] > 500


# ---- the Planck law ---------------------------------------------------------------------------------------
def test_planck_fractions_from_the_series():
    """the shares sum to one; the tail from 0 is one to the series' truncation; against a midpoint rule on [0, 0.5] and [0.5, 1]"""
    import math
    x = (0.5, 1, 2, 3, 4, 6, 8, 12)
    p = sm.planck_fractions(x)
    assert len(p) == len(x) + 1 and all(v > 0 for v in p) and abs(math.fsum(p) - 1.0) < 1e-15
    assert abs(sm.planck_tail(0.0) - 1.0) < 1e-7
    m = 20000
    mid = 0.5 + (np.arange(m) + 0.5) * (0.5 / m)
    quad = 15.0 / math.pi ** 4 * float(np.sum(mid ** 3 / np.expm1(mid)) * (0.5 / m))
    assert abs(quad - p[1]) < 1e-10
    mid = (np.arange(m) + 0.5) * (0.5 / m)
    quad = 15.0 / math.pi ** 4 * float(np.sum(mid ** 3 / np.expm1(mid)) * (0.5 / m))
    assert abs(quad - p[0]) < 1e-10


# ---- the library ------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    from jaybenne_amd import _lib
    lib = _lib.load()
    text = open(HEADER).read()
    for name in SPECTRUM_SYMBOLS:
        assert name in _lib.PROTOTYPES, name
        assert getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\(", text), name
    assert int(re.search(r"#define JB_SPECTRUM_MAX_GROUPS (\d+)", text).group(1)) == sm.MAX_GROUPS == _lib.JB_SPECTRUM_MAX_GROUPS
    assert "THE NUMBER OF EDGES j WITH edges[j] <= e" in text
    assert lib.jb_spectrum_words(None, 1) == 0
    import ctypes as C
    assert C.sizeof(_lib.SpectrumReport) == 56


@pytest.mark.parametrize("sanitize", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "sanitized"])
def test_the_scratch_layout_on_the_host(tmp_path, sanitize):
    """tests/spectrum_layout_test.cpp, a stand-alone program: spectrum_layout() behind the sort's arrays -- order,
    alignment, bounds, and the partials the kernels index"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "spectrum_layout_test")
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *sanitize,
                          os.path.join(ROOT, "tests", "spectrum_layout_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout + run.stderr
    hdr = next(line for line in open(os.path.join(ROOT, "jaybenne_amd", "csrc", "Makefile")) if line.startswith("HDR"))
    assert "jb_kernel_spectrum.hpp" in hdr.split()


# texts of `spectrum_edges`: numbers to both hosts, or an error to both, in the same words
EDGE_TEXTS = [" 0.1, 1e-3,2.5 ,4.9e-324 ", "1,2", "+1.,.5E+1,,3e0,", "-2.5e-3,\t0,1E2", "1.7976931348623157e308,1e-400",
              "0.1,0.30000000000000004,2.2250738585072011e-308", ",".join(str(j) for j in range(65)),
              # not decimal numbers: to float() or to strtod alone these would be numbers
              "1_0,2", "0x1p-3,1", "inf,1", "1,nan", "1,infinity", "1e,2", "1,.", "1,2e+", "1 2,3", "1,2x", "--1,2", "1;2",
              # too few, too many
              "", "1", " , ", ",".join(str(j) for j in range(66))]


def test_both_hosts_parse_the_same_edge_texts(tmp_path):
    """one decimal grammar: examples/mcblock_amd's parser (include/jaybenne_amd.hpp: ParseSpectrumEdges, through
    tests/spectrum_edges_test.cpp, a stand-alone program) and the Python host's give the same doubles or the same
    error for every text"""
    import shutil
    import subprocess
    from jaybenne_amd.__main__ import parse_spectrum_edges
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "spectrum_edges_test")
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "spectrum_edges_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    errors = 0
    for text in EDGE_TEXTS:
        run = subprocess.run([exe, text], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, (text, run.stderr)
        try:
            want = "".join("%.17g\n" % e for e in parse_spectrum_edges(text))
        except ValueError as e:
            want = f"error: {e}\n"
            errors += 1
        assert run.stdout == want, (text, run.stdout, want)
    assert errors == 16 and parse_spectrum_edges(EDGE_TEXTS[2]) == [1.0, 5.0, 3.0]


def test_the_python_host_prints_fixed_characters():
    """the Python host's line against fixed characters (examples/mcblock_amd is held to the same lines on the GPU)"""
    from jaybenne_amd.__main__ import parse_spectrum_edges, spectrum_integrals, spectrum_json
    edges = parse_spectrum_edges(" 0.1, 1e-3,2.5 ,4.9e-324 ")
    assert edges == [0.1, 1e-3, 2.5, 5e-324]
    rep = dict(n_counted=3, n_skipped=1, cells_nonempty=2, longest_run=2, n_below=1, n_above=0, sorted=1)
    line = spectrum_json(2, 0.5, rep, [0.1, 2.5], [1.0, 0.25, 0.0])
    assert line == ('{"cycle": 2, "time": 0.5, "n_counted": 3, "n_skipped": 1, "cells_nonempty": 2, "longest_run": 2, '
                    '"n_below": 1, "n_above": 0, "sorted": 1, "ngroups": 1, "edges": [0.10000000000000001, 2.5], '
                    '"e": [1, 0.25, 0]}')
    spec = np.arange(2 * 2 * 3, dtype=np.float64).reshape(2, 2, 1, 1, 3)
    dx = np.array([[0.5, 1.0, 1.0], [0.25, 1.0, 1.0]])
    assert spectrum_integrals(spec, dx) == sm.integrals(spec, dx) == [0.5 * 3 + 0.25 * 12, 0.5 * 21 + 0.25 * 30]
