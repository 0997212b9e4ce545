"""The canonical order within cells (include/jaybenne_amd.h: jb_set_cell_order) without a GPU: the pass planning of
the sort on the host (tests/order_test.cpp, once plainly and once under the address and undefined-behaviour
sanitizers -- a stand-alone program), the deck key, the exports, and the order photons are sourced in."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cell_order_model as om
import comb_model as cm
from helpers import ROOT, load_deck, make_oracle, run_oracle_cycles

HEADER = os.path.join(ROOT, "include", "jaybenne_amd.h")


@pytest.mark.parametrize("sanitize", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "sanitized"])
def test_pass_planning_on_the_host(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "order_test")
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *sanitize,
                          os.path.join(ROOT, "tests", "order_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout + run.stderr


# ---- the deck key ---------------------------------------------------------------------------------
@pytest.mark.parametrize("value, want", [("id", "id"), ("any", "any"), (None, "any")])
def test_deck_key_sets_the_mode(value, want):
    from jaybenne_amd import jaybenne as jb, mcblock, _lib
    pin = load_deck("stepdiff", {} if value is None else {"jaybenne_amd/cell_order": value})
    assert mcblock.deck_cell_order(pin) == want
    assert jb.cell_order_code(want) == {"any": _lib.CELL_ORDER_ANY, "id": _lib.CELL_ORDER_BY_ID}[want]


@pytest.mark.parametrize("value", ["ID", "by_id", "1", "none"])
def test_a_wrong_value_names_the_key(value):
    from jaybenne_amd import jaybenne as jb, mcblock
    with pytest.raises(ValueError, match="jaybenne_amd/cell_order"):
        mcblock.deck_cell_order(load_deck("stepdiff", {"jaybenne_amd/cell_order": value}))
    with pytest.raises(ValueError, match="cell_order"):
        jb.cell_order_code(value)


def test_the_cpp_host_reads_the_same_key():
    """include/jaybenne_amd.hpp: CellOrderOf -- compiled alone (it needs no library) and asked the same questions."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    src = r'''
#include <cstdio>
#include <cstring>
#include "jaybenne_amd.hpp"
int main() {
  int bad = 0;
  for (const char *v : {"ID", "by_id", "1", ""}) {
    try { (void)jaybenne_amd::CellOrderOf(v); } catch (const std::invalid_argument &e) {
      bad += std::strstr(e.what(), "jaybenne_amd/cell_order") != nullptr;
    }
  }
  std::printf("%d %d %d\n", jaybenne_amd::CellOrderOf("any"), jaybenne_amd::CellOrderOf("id"), bad);
}
'''
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "t.cpp"), "w") as f:
            f.write(src)
        exe = os.path.join(tmp, "t")
        res = subprocess.run([cxx, "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.cpp"),
                              "-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and run.stdout.split() == ["0", "1", "4"], run.stdout + run.stderr


# ---- the library ------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    from jaybenne_amd import _lib
    lib = _lib.load()
    text = open(HEADER).read()
    for name in ("jb_set_cell_order", "jb_get_cell_order"):
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\(", text), name
    assert (_lib.CELL_ORDER_ANY, _lib.CELL_ORDER_BY_ID) == (0, 1)
    assert re.search(r"enum \{ JB_CELL_ORDER_ANY = 0, JB_CELL_ORDER_BY_ID = 1 \}", text)
    # no context exists without a GPU: null pointers are turned down before anything is touched
    assert lib.jb_set_cell_order(None, _lib.CELL_ORDER_BY_ID) == _lib.JB_ERR_INVALID
    assert b"jb_set_cell_order" in lib.jb_last_error()
    assert lib.jb_get_cell_order(None) == _lib.CELL_ORDER_ANY


# ---- the order photons are sourced in ---------------------------------------------------------------
def test_the_model_orders_by_key_then_id_then_slot():
    """The model itself, on a swarm small enough to read: ids as unsigned words (bit 63 sorts last), dead slots behind
    all cells, equal (key, id) in input order."""
    from test_gpu_comb import MESHES
    from jaybenne_amd.mesh import Mesh
    deck, ov = MESHES["1d"]
    mesh = Mesh.from_deck(load_deck(deck, ov))
    gids = np.arange(mesh.nblocks)
    n = 7
    sw = {k: np.zeros(n, dtype=np.int32 if k in ("ip", "jp", "kp", "blk", "status") else np.float64) for k in cm.SWARM_KEYS}
    sw["id"] = np.array([5, (1 << 63) + 1, 3, 9, 9, 1 << 40, 2], dtype=np.uint64)
    sw["rng"] = np.zeros(n, dtype=np.uint64)
    cell = np.array([1, 1, 1, 0, 0, 0, 0])
    sw["x"] = mesh.blk_xmin[0, 0] + (cell + 0.5) * mesh.blk_dx[0, 0]
    sw["status"][[3, 4]] = 1          # two dead slots with one id
    order, key = om.canonical_order(mesh, gids, sw, n)
    assert order.tolist() == [6, 5, 2, 0, 1, 3, 4]
    assert key[3] == key[4] == mesh.nblocks * int(np.prod(mesh.field_shape[1:]))
    assert not om.is_canonical(mesh, gids, sw, n)
    assert om.is_canonical(mesh, gids, om.canonical_sort(mesh, gids, sw, n), n)


@pytest.mark.parametrize("name", ["1d", "3d"])
def test_a_freshly_sourced_swarm_is_in_canonical_order(name):
    """Photons are sourced block by block, cell by cell, with rising ids: the initial swarm of the CPU oracle is in
    canonical order, so the first sort of a run in this mode moves nothing it need not."""
    from oracle import orc
    from test_gpu_comb import MESHES
    deck, ov = MESHES[name]
    ov = dict(ov, **{"jaybenne/num_particles": 4000})
    O, mesh, _ = make_oracle(load_deck(deck, ov), orc.MATH_PORTABLE, capacity_factor=4.0)
    gids = np.arange(mesh.nblocks)
    sw = {k: O.sw[k] for k in cm.SWARM_KEYS}
    if O.n == 0:            # (a deck without initial radiation: the photons of the first cycle's source)
        run_oracle_cycles(O, load_deck(deck, ov), 1)
        act = np.flatnonzero(O.sw["status"][:O.n] == cm.ST_ACTIVE)
        assert len(act) > 0 and np.all(np.diff(O.sw["id"][:O.n][act].astype(np.uint64).astype(np.int64)) > 0)
        return
    assert O.n > 0 and len(np.unique(O.sw["id"][:O.n])) == O.n
    key, _, nkeys, _ = cm.cell_keys(mesh, gids, sw, O.n)
    assert key.max() < nkeys and len(np.unique(key)) > 1
    assert om.is_canonical(mesh, gids, sw, O.n)
