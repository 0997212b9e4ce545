"""Expected values of the energy ledger (include/jaybenne_amd.h: jb_energy_ledger), from the CPU oracle alone.

``oracle_cycle`` restates one radiation cycle on the oracle task by task, as ``Oracle.RadiationStep`` does, and reads
the oracle's swarm after TransportPhotons and BEFORE RemoveMarkedParticles: there the escaped and absorbed slots still
exist, with their weights and positions.  Every sum is ``math.fsum``.  tests/test_ledger_host.py (CPU) checks the
conditions the cases must meet; tests/test_gpu_ledger.py holds the library to these terms.
"""
from __future__ import annotations

import math

import numpy as np

import axis_cases as ax
import hetero_states as hs
from helpers import load_deck

FACES = ax.FACES
BC_OUTFLOW = 2          # enum of include/jaybenne_amd.h (JB_BC_OUTFLOW)
ST_ACTIVE, ST_ABSORBED, ST_ESCAPED = 0, 1, 2

# the (case, boundary set) pairs the GPU tests run
PAIRS = [("G1-imc", "RO"), ("G1-imc", "OR"), ("G1-ddmc", "RO"), ("G1-ddmc", "OR"),
         ("G2S-imc", "S1"), ("G2S-imc", "S2"), ("G2S-imc", "S3"),
         ("G3U-imc", "S1"), ("G3U-imc", "S2"), ("G3U-imc", "S3"), ("G3O-imc", "S2"), ("G3S-imc", "S3"),
         ("G2S-ddmc", "S1"), ("G3S-ddmc", "S1"), ("G3S-ddmc", "S2"), ("G3S-ddmc", "S3"),
         ("G2S-hybrid", "S1"), ("G2S-hybrid", "S3"), ("G3S-hybrid", "S2"), ("G3S-hot", "S1")]


def case_of(cid):
    return ax.HOT_CASE if cid == ax.HOT_CASE.id else ax.BY_ID[cid]


def setup_of(cid, bset):
    """(case, deck overrides, pattern, capacity factor) of a pair."""
    case = case_of(cid)
    return case, ax.overrides(case, bset), ax.DDMC_PALETTE.get((cid, bset), case.pattern), (8.0 if cid == "G3S-hot" else 1.3)


def oracle_of(cid, bset):
    case, ov, pattern, cf = setup_of(cid, bset)
    O, mesh, pkg = hs.oracle_on(case.deck, ov, pattern, capacity_factor=cf)
    return O, mesh, load_deck(case.deck, ov)


def classify(mesh, x, y, z):
    """The face rule of jb_energy_ledger on arrays of positions: (face, axes outside).  face: the first active
    axis d on which the position lies strictly outside -- below gmin[d]: 2 d, above gmax[d]: 2 d + 1 -- if that
    face is outflow, else 6 (unclassified); axes outside: on how many active axes the position lies outside."""
    pos = (np.asarray(x), np.asarray(y), np.asarray(z))
    face = np.full(pos[0].shape, -1, dtype=np.int64)
    outside = np.zeros(pos[0].shape, dtype=np.int64)
    for d in range(mesh.ndim):
        lo, hi = pos[d] < mesh.gmin[d], pos[d] > mesh.gmax[d]
        outside += (lo | hi)
        face = np.where((face < 0) & lo, 2 * d, face)
        face = np.where((face < 0) & hi, 2 * d + 1, face)
    bc = np.asarray(mesh.swarm_bc)
    ok = (face >= 0) & (bc[np.maximum(face, 0)] == BC_OUTFLOW)
    return np.where(ok, face, 6), outside


def census_energy(O):
    n = O.n
    act = O.sw["status"][:n] == ST_ACTIVE
    return math.fsum(O.sw["w"][:n][act]), int(act.sum())


def oracle_cycle(O, pin, t):
    """One cycle of the oracle, task by task (oracle/orc.py: Oracle.RadiationStep), then the host's update as
    oracle/harness.py: run_oracle_cycles makes it.  Returns the ledger's terms as a dict, with ``e_start`` and
    ``residual``, and under ``escaped`` the escaped slots themselves (id, w, x, y, z, face, axes outside)."""
    from oracle import orc
    dt = pin.GetReal("jaybenne", "dt")
    mesh = O.mesh
    e_start, _ = census_energy(O)
    O.cycle += 1
    O.UpdateDerivedTransportFields(dt)
    n0 = O.n
    O.SourcePhotons(orc.SRC_EMISSION, t, dt, getattr(O, "emission_blocks_in_call", None))
    led = {"cycle": O.cycle, "t_start": t, "dt": dt, "e_start": e_start,
           "e_sourced": math.fsum(O.sw["w"][n0:O.n]), "n_sourced": O.n - n0}
    O.TransportPhotons(t, dt)
    n = O.n
    st, w = O.sw["status"][:n], O.sw["w"][:n]
    esc = st == ST_ESCAPED
    face, outside = classify(mesh, O.sw["x"][:n][esc], O.sw["y"][:n][esc], O.sw["z"][:n][esc])
    led["e_escaped"] = [math.fsum(w[esc][face == f]) for f in range(6)]
    led["n_escaped"] = [int((face == f).sum()) for f in range(6)]
    led["e_escaped_unclassified"] = math.fsum(w[esc][face == 6])
    led["n_escaped_unclassified"] = int((face == 6).sum())
    led["e_absorbed"] = math.fsum(w[st == ST_ABSORBED])
    led["n_absorbed"] = int((st == ST_ABSORBED).sum())
    led["escaped"] = {"id": O.sw["id"][:n][esc].copy(), "w": w[esc].copy(), "face": face, "outside": outside,
                      **{k: O.sw[k][:n][esc].copy() for k in ("x", "y", "z")}}
    assert int(((st != ST_ACTIVE) & (st != ST_ABSORBED) & ~esc).sum()) == 0
    O.RemoveMarkedParticles()
    assert O.CheckCompletion(t + dt) == 0
    O.EvaluateRadiationEnergy()
    O.UpdateFluid()
    led["e_census"], led["n_census"] = census_energy(O)
    vol = np.array([mesh.cell_volume(b) for b in range(mesh.nblocks)])[:, None, None, None]
    sl = mesh.interior()
    led["e_tally"] = math.fsum((O.fields["tally"] * vol)[sl].ravel())
    led["e_delta"] = math.fsum(O.fields["edelta"][sl].ravel())
    led["e_material"] = math.fsum((O.fields["u"] * vol)[sl].ravel())
    led["residual"] = residual(led)
    if pin.GetOrAddBoolean("jaybenne", "do_feedback", True):
        mesh.fill_ghosts(O.fields["u"])
    O.fields["sie"][...] = O.fields["u"] / O.fields["rho"]
    return led


def residual(led):
    """Of e_start + e_sourced = e_census + e_absorbed + escaped, relative to the left-hand side."""
    lhs = math.fsum([led["e_start"], led["e_sourced"]])
    return abs(math.fsum([led["e_start"], led["e_sourced"], -led["e_census"], -led["e_absorbed"],
                          -led["e_escaped_unclassified"]] + [-e for e in led["e_escaped"]])) / lhs


_CACHE = {}


def oracle_ledgers(cid, bset, cycles):
    """The oracle's ledgers of the first ``cycles`` cycles of a pair, computed once per process and shared: a
    tuple of dicts that nobody changes."""
    key = (cid, bset)
    if key not in _CACHE or len(_CACHE[key]) < cycles:
        O, mesh, pin = oracle_of(cid, bset)
        dt, t, out = pin.GetReal("jaybenne", "dt"), 0.0, []
        for _ in range(cycles):
            out.append(oracle_cycle(O, pin, t))
            t += dt
        _CACHE[key] = tuple(out)
    return _CACHE[key][:cycles]
