"""The energy ledger without a GPU: the conditions the cases of tests/test_gpu_ledger.py must meet, checked on the
CPU oracle alone (tests/ledger_cases.py), and what the library and its bindings promise a host before any kernel
runs -- the struct, the symbols, the argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ledger_cases as lc
from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "jaybenne_amd.h")


# ---- the cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,bset", lc.PAIRS, ids=[f"{c}-{s}" for c, s in lc.PAIRS])
def test_cases_send_energy_through_every_open_face(cid, bset):
    """First cycle of the oracle: every escaped slot is classified by the face rule to exactly one face, that face
    is outflow, no escaped slot lies outside on more than one axis, every outflow face receives at least 50
    escapes, and the energy identity holds to 1e-12."""
    led = lc.oracle_ledgers(cid, bset, 1)[0]
    geom = lc.case_of(cid).geom
    mesh = lc.ax.mesh_of(geom, lc.ax.boundary_sets(geom)[bset])
    esc = led["escaped"]
    assert len(esc["id"]) > 0
    assert led["n_escaped_unclassified"] == 0 and np.all(esc["face"] < 6)
    assert np.all(esc["outside"] == 1)
    bc = np.asarray(mesh.swarm_bc)
    assert np.all(bc[esc["face"]] == lc.BC_OUTFLOW)
    open_faces = [f for f in range(2 * mesh.ndim) if bc[f] == lc.BC_OUTFLOW]
    assert open_faces
    for f in range(6):
        if f in open_faces:
            assert led["n_escaped"][f] >= 50, (lc.FACES[f], led["n_escaped"])
            assert led["e_escaped"][f] > 0.0
        else:
            assert led["n_escaped"][f] == 0 and led["e_escaped"][f] == 0.0
    assert sum(led["n_escaped"]) == len(esc["id"])
    assert led["residual"] <= 1e-12, led["residual"]
    assert abs(led["e_tally"] - led["e_census"]) <= 1e-12 * led["e_census"]
    if cid == "G3S-hot":
        assert led["n_absorbed"] > 500 and led["n_sourced"] > 100
    else:
        assert led["n_absorbed"] == 0 and led["n_sourced"] == 0


def test_face_rule_on_constructed_positions():
    """classify(): below / above every axis in turn, inside, outside a face that is not outflow, and outside on
    two axes (the first axis decides)."""
    mesh = lc.ax.mesh_of("G3U", lc.ax.boundary_sets("G3U")["S1"])        # R O | O R | P P
    lo, hi = np.asarray(mesh.gmin), np.asarray(mesh.gmax)
    mid = 0.5 * (lo + hi)
    pts = {"in": mid.copy()}
    for d in range(3):
        for side, v in (("lo", lo[d] - 1e-3), ("hi", hi[d] + 1e-3)):
            p = mid.copy()
            p[d] = v
            pts[f"{d}{side}"] = p
    both = mid.copy()
    both[0], both[1] = hi[0] + 1e-3, lo[1] - 1e-3
    pts["two"] = both
    names = list(pts)
    xyz = np.array([pts[k] for k in names])
    face, outside = lc.classify(mesh, xyz[:, 0], xyz[:, 1], xyz[:, 2])
    got = dict(zip(names, face.tolist()))
    assert got == {"in": 6, "0lo": 6, "0hi": 1, "1lo": 2, "1hi": 6, "2lo": 6, "2hi": 6, "two": 1}
    assert dict(zip(names, outside.tolist()))["two"] == 2
    on_face = mid.copy()
    on_face[0] = hi[0]                       # ON the face is not outside: strictly
    assert lc.classify(mesh, on_face[:1], on_face[1:2], on_face[2:3])[0][0] == 6


# ---- the library, no GPU -----------------------------------------------------------------------
def _header_struct():
    text = open(HEADER).read()
    body = re.search(r"typedef struct jb_energy_ledger \{(.*?)\} jb_energy_ledger;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for name in rest.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", name)
            fields.append((m.group(1), ctype, int(m.group(2) or 1)))
    return fields


def test_struct_matches_the_ctypes_mirror():
    from jaybenne_amd import _lib
    fields = _header_struct()
    want = [(n, {"double": C.c_double, "int64_t": C.c_int64}[t], k) for n, t, k in fields]
    got = [(n, getattr(t, "_type_", t) if hasattr(t, "_length_") else t, getattr(t, "_length_", 1))
           for n, t in _lib.EnergyLedger._fields_]
    assert got == want
    assert C.sizeof(_lib.EnergyLedger) == 8 * sum(k for _, _, k in fields) == 208
    assert [n for n, _, _ in fields] == [
        "e_sourced", "n_sourced", "e_escaped", "n_escaped", "e_escaped_unclassified", "n_escaped_unclassified",
        "e_absorbed", "n_absorbed", "e_census", "n_census", "e_tally", "e_delta", "e_material", "t_start", "dt", "cycle"]
    assert (_lib.JB_LEDGER_SOURCED, _lib.JB_LEDGER_TRANSPORTED) == (0, 1)
    assert re.search(r"enum \{ JB_LEDGER_SOURCED = 0, JB_LEDGER_TRANSPORTED = 1 \}", open(HEADER).read())
    d = _lib.EnergyLedger(e_sourced=1.5, n_sourced=3, cycle=7).as_dict()
    assert d["e_sourced"] == 1.5 and d["n_sourced"] == 3 and d["cycle"] == 7 and d["e_escaped"] == [0.0] * 6
    assert d["n_escaped"] == [0] * 6 and all(isinstance(v, int) for v in d["n_escaped"])


LEDGER_SYMBOLS = ("jb_ledger_enable", "jb_ledger_enabled", "jb_ledger_accumulate", "jb_ledger_close",
                  "jb_ledger_reduce", "jb_ledger_last")


def test_symbols_are_exported_and_declared():
    from jaybenne_amd import _lib
    lib = _lib.load()
    text = open(HEADER).read()
    for name in LEDGER_SYMBOLS:
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\(", text), name


def test_null_arguments_are_invalid():
    """No context exists without a GPU: every entry point must turn null pointers down before it touches one."""
    from jaybenne_amd import _lib
    lib = _lib.load()
    led = _lib.EnergyLedger()
    sv = _lib.SwarmView()
    bad = _lib.JB_ERR_INVALID
    assert lib.jb_ledger_enable(None, 1) == bad and b"null" in lib.jb_last_error()
    assert lib.jb_ledger_enabled(None) == 0
    assert lib.jb_ledger_accumulate(None, None, C.byref(sv), 0, 0, _lib.JB_LEDGER_SOURCED) == bad
    assert b"jb_ledger_accumulate" in lib.jb_last_error()
    assert lib.jb_ledger_close(None, None, C.byref(sv), 0.0, 1.0, C.byref(led)) == bad
    assert b"jb_ledger_close" in lib.jb_last_error()
    assert lib.jb_ledger_reduce(None, None, 0, 1, 0, C.byref(led)) == bad
    assert b"jb_ledger_reduce" in lib.jb_last_error()
    assert lib.jb_ledger_last(None, C.byref(led)) == bad and b"jb_ledger_last" in lib.jb_last_error()


def test_residual_helper():
    from jaybenne_amd import _lib
    led = dict(e_sourced=2.0, e_census=5.0, e_absorbed=1.0, e_escaped=[0.5, 0.0, 0.25, 0.0, 0.0, 0.0],
               e_escaped_unclassified=0.25)
    assert _lib.ledger_residual(led, 5.0) == 0.0
    assert _lib.ledger_residual(led, 5.5) == pytest.approx(0.5 / 7.5)
    assert _lib.ledger_residual(dict(led, e_sourced=0.0), 0.0) == 0.0
