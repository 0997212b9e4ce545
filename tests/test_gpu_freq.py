"""k_transport<NDIM, DDMC, TALLY, GRAY = 0> -- the opacities evaluated at every event from the cell's rho and sie and the
photon's own frequency -- where the temperature and the frequency act, against the CPU oracle.

Under the gray models both inputs are dead (tests/test_freq_host.py::test_c: exactly 0.000 of the photons notice a
shifted sie or their neighbour's frequency), so the heterogeneous, axis-asymmetric and lane-reuse suites cannot see a
``sie`` gathered from the wrong cell, block or axis, or a refill that keeps the previous photon's frequency.  The rows of
tests/freq_cases.py run EPBremss on material whose rho AND sie differ in every cell, on meshes whose axes all differ,
with every boundary kind on every axis; a one-cell shift of sie changes 7 .. 100 % of their photons, the neighbour's
frequency 12 .. 100 %, and with ``use_ddmc`` 24 .. 68 % of the photons start on the DDMC side in cells they share with
photons of the other regime: the regime interface runs through frequency (tests/test_freq_host.py holds all of this on
the CPU).

All tests run exact arithmetic -- GRAY = 0 has no lean form, which the variant string says -- and first check that they
ran what they say: ``jb_last_transport_variant`` is ``k_transport<N, true, 0, false, false>`` behind the entry point the
row names, and under a cap ``jb_last_transport_grid`` equals it.  Then photons bit for bit by creation id, tally, fleck,
src_num and src_ew to 1e-12, energy_delta to 1e-12 of the emitted energy, events and the four outcome counters equal.
(Several resident blocks beyond kLdsBlocks need no case: GRAY = 0 never takes the LDS-table branch.)

Wall time on the MI355X (pytest's ``--durations``, the whole file 5.4 s for 30 tests): every call 0.01 .. 0.20 s (the
slowest: the F3S-imc and F3S-hybrid rows, 4e6 and 2e6 events a cycle, on the default grid, with one workgroup and on
the threshold; one workgroup follows a cycle of F3S-imc in under 0.2 s), the first test's set-up, which loads the
library, 1.7 s.  No row's photon count had to be lowered.
"""
import types

import numpy as np
import pytest

import axis_cases as ax
import freq_cases as fc
import hetero_states as hs
import lane_reuse_cases as lr
from helpers import load_deck, run_oracle_cycles
from test_gpu_hetero import _compare_start, _variant
from test_gpu_lane_reuse import COUNTERS, FIELDS, KNOB, SWITCHES, _emitted, _grid
from test_gpu_parity import _compare_fields, _compare_swarm_by_id

pytestmark = pytest.mark.gpu

IDS = [c.id for c in fc.CASES]


def _ndim(case):
    return len(ax.GEOMETRIES[case.geom].nx)


def _driver(case, device, monkeypatch, G=None):
    """The device problem of a row under the cap G (None: the knob unset).  The switches are read when the driver is
    made."""
    from jaybenne_amd import mcblock
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if G is not None:
        monkeypatch.setenv(KNOB, str(G))
    ov = fc.overrides(case)
    drv = mcblock.McblockDriver(load_deck(case.deck, ov), device=device, initial_state=hs.state_for(case.deck, ov, fc.PATTERN),
                                capacity_factor=fc.CAPACITY_FACTOR)
    assert drv.pkg.arithmetic() == "exact" and _grid(drv) == 0
    return drv


_REFERENCE = {}


def _reference(cid, cycles, threshold=False):
    """The oracle's run of a row, computed once and only read afterwards: ``cycles`` cycles with ``watch`` on its
    transport calls; ``threshold``: every 5th starting photon on e_lo or e_hi of its cell (``e0``: the frequencies the
    run started from, ``ids0`` their photons)."""
    key = (cid, cycles, threshold)
    if key not in _REFERENCE:
        case = fc.BY_ID[cid]
        pin, O, mesh, pkg = fc.oracle_of(case)
        r = types.SimpleNamespace(pin=pin, O=O, mesh=mesh, pkg=pkg, ids0=O.sw["id"][:O.n].copy(), sides=None)
        if threshold:
            e, low, high = fc.on_the_threshold(O, mesh, fc.model_params(pin, pkg))
            O.sw["e"][:O.n] = e
            r.sides = (int(low.sum()), int(high.sum()))
        r.e0 = O.sw["e"][:O.n].copy()
        r.log = lr.watch(O)
        run_oracle_cycles(O, pin, cycles)
        r.outcomes = lr.outcomes(r.log)
        _REFERENCE[key] = r
    return _REFERENCE[key]


def _ran_what_it_says(drv, case, G=None):
    nd = _ndim(case)
    entry = "TransportPhotons_DDMC: " if drv.pkg.Param("use_ddmc") else "TransportPhotons: "
    want = ("TransportPhotons_DDMC: " if case.ddmc else "TransportPhotons: ") + f"k_transport<{nd}, true, 0, false, false>"
    assert entry + _variant(drv) == want, entry + _variant(drv)
    if G is None:
        assert _grid(drv) > 3, _grid(drv)                 # one lane per photon, or the chip's fill
    else:
        assert _grid(drv) == G, _grid(drv)


def _equals_the_oracle(drv, ref):
    """Photons bit for bit by creation id, fields to 1e-12 (energy_delta: of the emitted energy), events and the four
    outcome counters."""
    O = ref.O
    _compare_swarm_by_id(drv.md, O)
    _compare_fields(drv.md, O, tuple(k for k in FIELDS if k != "edelta"))
    _compare_fields(drv.md, O, ("edelta",), scale=_emitted(O, ref.mesh))
    assert drv.md.events == O.events
    got = drv.md.stats()
    assert {k: got[k] for k in COUNTERS} == {k: ref.outcomes[k] for k in COUNTERS}
    assert all(ref.outcomes[k] >= lr.FLOOR for k in ("n_census", "n_absorbed", "n_escaped"))


# ---- a. before the first step ------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_sourcing_and_derived_fields_before_the_first_step(gpu_device, monkeypatch, cid):
    """The swarm bit for bit; fleck, src_num, src_ew and P1 .. P3 (k_face_prob evaluates EPBremss at nu = 1 from two
    neighbouring cells' rho and sie) as test_gpu_axes holds them."""
    case = fc.BY_ID[cid]
    drv = _driver(case, gpu_device, monkeypatch)
    pin, O, mesh, pkg = fc.oracle_of(case)
    _compare_start(drv, O, case.ddmc)
    f = O.fields["fleck"][mesh.interior()]
    assert len(np.unique(f)) > 0.4 * f.size               # a Fleck factor of its own in (nearly) every cell


# ---- b. every row on the default grid ----------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_every_row_on_the_default_grid(gpu_device, monkeypatch, cid):
    case = fc.BY_ID[cid]
    ref = _reference(cid, case.cycles)
    drv = _driver(case, gpu_device, monkeypatch)
    for _ in range(case.cycles):
        drv.Step()
    _ran_what_it_says(drv, case)
    _equals_the_oracle(drv, ref)


# ---- c. many photons per lane ------------------------------------------------------------------
CAPPED = [(c.id, G) for c in fc.CASES for G in c.grids]
assert any(G == 3 and fc.BY_ID[c].ddmc for c, G in CAPPED) and any(G == 3 and not fc.BY_ID[c].ddmc for c, G in CAPPED)
assert {c for c, G in CAPPED if G == 1} == set(IDS)


@pytest.mark.parametrize("cid,G", CAPPED, ids=[f"{c}-G{G}" for c, G in CAPPED])
def test_many_photons_per_lane(gpu_device, monkeypatch, cid, G):
    """One cycle under JB_TRANSPORT_MAX_BLOCKS = G: a lane that takes its next photon must take that photon's
    frequency, and gather the temperature of the cell, block and level that photon is in."""
    case = fc.BY_ID[cid]
    ref = _reference(cid, 1)
    drv = _driver(case, gpu_device, monkeypatch, G)
    assert drv.md.n >= lr.reuse_floor(G), (drv.md.n, G)
    drv.Step()
    _ran_what_it_says(drv, case, G)
    _equals_the_oracle(drv, ref)


# ---- d. photons on the threshold ---------------------------------------------------------------
THRESHOLD = [(c, G) for c in ("F2S-hybrid", "F3S-hybrid") for G in (None, 1)]


@pytest.mark.parametrize("cid,G", THRESHOLD, ids=[f"{c}-" + ("default" if G is None else f"G{G}") for c, G in THRESHOLD])
def test_photons_on_the_regime_threshold(gpu_device, monkeypatch, cid, G):
    """Every 5th starting photon carries e_lo or e_hi of the cell it starts in: neighbouring doubles of which the
    oracle's expression calls the first DDMC and the second not.  The kernel must decide as the oracle does."""
    import torch
    case = fc.BY_ID[cid]
    ref = _reference(cid, 1, threshold=True)
    assert ref.sides[0] > lr.FLOOR and ref.sides[1] > lr.FLOOR, ref.sides
    drv = _driver(case, gpu_device, monkeypatch, G)
    n = drv.md.n
    assert n == len(ref.ids0) and np.array_equal(drv.md.get_swarm()["id"], ref.ids0)
    if G is not None:
        assert n >= lr.reuse_floor(G)
    drv.md.swarm["e"][:n] = torch.from_numpy(ref.e0).to(gpu_device)
    drv.Step()
    _ran_what_it_says(drv, case, G)
    _equals_the_oracle(drv, ref)
