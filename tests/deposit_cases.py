"""The (deck, overrides) pairs the exact-deposition tests run (tests/test_gpu_deposit.py), and what one cycle of the
CPU oracle absorbs on each: tests/test_deposit_host.py holds every pair to the conditions under which a GPU case
proves something -- enough absorbed photons, enough cells with several addends, nothing truncated."""
from __future__ import annotations

import numpy as np

import deposit_model as dm
import axis_cases as ax
import hetero_states as hs
import ledger_cases as lc
from helpers import load_deck, make_oracle

# emission and feedback on, absorption as strong as the scattering of the IMC deck is weak: the material state of
# the next cycle depends on every deposit
HOT = {"mcblock/opacity_model": "constant", "mcblock/opacity_constant_value": 100.0,
       "jaybenne/do_emission": "true", "jaybenne/do_feedback": "true"}
ONE_D = dict({"parthenon/mesh/nx1": 16, "parthenon/meshblock/nx1": 8, "jaybenne/num_particles": 20000}, **HOT)

# name -> ("deck", deck, overrides), ("ledger", case id, boundary set) of tests/ledger_cases.py, or ("hetero", case id
# of tests/axis_cases.py, boundary set): that case with the absorption of hetero_states.ABSORBING added
CASES = {
    "hybrid-2d": ("hetero", "G2S-hybrid", "S1"),
    "imc-1d": ("deck", "stepdiff", ONE_D),
    "ddmc-1d": ("deck", "stepdiff_ddmc", ONE_D),
    "imc-3d-smr": ("ledger", "G3S-hot", "S1"),
    "imc-3d": ("deck", "inf", {"jaybenne/num_particles": 20000}),
}


def setup_of(name):
    """(deck, overrides, initial state or None, capacity factor) of a case."""
    kind, a, b = CASES[name]
    if kind == "deck":
        return a, b, None, 2.0
    if kind == "ledger":
        case, ov, pattern, cf = lc.setup_of(a, b)
    else:
        case = ax.BY_ID[a]
        ov, pattern, cf = dict(ax.overrides(case, b), **hs.ABSORBING), case.pattern, 2.0
    return case.deck, ov, hs.state_for(case.deck, ov, pattern), cf


def pin_of(name):
    deck, ov, _, _ = setup_of(name)
    return load_deck(deck, ov)


def oracle_of(name):
    """(oracle, mesh, deck) of a case, before its first cycle."""
    from oracle import orc
    deck, ov, state, cf = setup_of(name)
    kw = {} if state is None else {"initial_state": state}
    O, mesh, _ = make_oracle(load_deck(deck, ov), orc.MATH_PORTABLE, capacity_factor=max(cf, 2.0), **kw)
    return O, mesh, load_deck(deck, ov)


def oracle_absorbed(name, cycles=1):
    """Per cycle of the oracle: the absorbed slots as they stand after TransportPhotons and before the compaction
    -- (flat interior cell index, w) -- and the weights of the whole swarm at that moment (the scale's range)."""
    O, mesh, pin = oracle_of(name)
    from oracle import orc
    dt, t, out = pin.GetReal("jaybenne", "dt"), 0.0, []
    for _ in range(cycles):
        O.cycle += 1
        O.UpdateDerivedTransportFields(dt)
        O.SourcePhotons(orc.SRC_EMISSION, t, dt, getattr(O, "emission_blocks_in_call", None))
        w_before = O.sw["w"][:O.n].copy()
        O.TransportPhotons(t, dt)
        n = O.n
        sel = O.sw["status"][:n] == dm.ST_ABSORBED
        cell = dm.cell_index(mesh, O.sw, n)[sel]
        out.append(dict(cell=cell, w=O.sw["w"][:n][sel].copy(), w_all=w_before, ncells=mesh.nblocks * mesh.ncell))
        O.RemoveMarkedParticles()
        O.EvaluateRadiationEnergy()
        O.UpdateFluid()
        if pin.GetOrAddBoolean("jaybenne", "do_feedback", True):
            mesh.fill_ghosts(O.fields["u"])
        O.fields["sie"][...] = O.fields["u"] / O.fields["rho"]
        t += dt
    return out


def conditions(rec):
    """(absorbed photons, cells with >= 2 addends, n_truncated of the model at the scale of the swarm)."""
    E = dm.scale(rec["w_all"])
    _, n_add, n_trunc, n_rej = dm.accumulate(rec["w"], rec["cell"], rec["ncells"], E)
    per = np.bincount(rec["cell"], minlength=rec["ncells"])
    assert n_rej == 0 and n_add == len(rec["w"])
    return n_add, int((per >= 2).sum()), n_trunc
