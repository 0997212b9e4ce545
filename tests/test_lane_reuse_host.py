"""CPU conditions on the rows of tests/lane_reuse_cases.py -- what keeps tests/test_gpu_lane_reuse.py from passing
vacuously.  Everything here is the oracle's: one cycle of each row, with ``watch`` on its transport call.

* reuse is forced: the photons at the transport call number at least 8 x 256 x G for G = 1 workgroup and
  4 x 256 x G for G = 3, so some lane follows at least 8 (4) of them and the average lane does;
* the awkward predecessors are common: at least 256 histories end escaped or absorbed (a lane then starts its next
  photon from an absolute position, a block id of another meaning, a cleared run bit) and at least 256 end at census;
* on the two-level meshes at least 256 survivors end on a block of another level than they started on (the per-lane
  geometry of the lane's next photon is then another one);
* the hybrid rows have both regimes on both levels, and at least 256 survivors end in a cell of the other regime
  than they started in, so they took steps of both kinds (the oracle keeps no per-history count of them).

These are conditions, not measurements: a row that falls under a floor gets another boundary set or scattering value.
"""
import numpy as np
import pytest

import axis_cases as ax
import hetero_states as hs
import lane_reuse_cases as lr
from helpers import load_deck, run_oracle_cycles
from test_axis_host import test_hybrid_cases_have_both_regimes_on_both_levels as _both_regimes_on_both_levels

RUNS = [(r, p) for r in lr.ROWS for p in r.patterns]


def _one_cycle(row, pattern):
    case = lr.case_of(row)
    ov = ax.overrides(case, row.bset)
    pin = load_deck(case.deck, ov)
    O, mesh, pkg = hs.oracle_on(case.deck, ov, pattern, capacity_factor=row.capacity_factor)
    ddmc = hs.regime_map(mesh, pkg, O.fields["rho"], pin.GetOrAddReal("jaybenne", "tau_ddmc", 5.0))
    log = lr.watch(O)
    run_oracle_cycles(O, pin, 1)
    assert len(log) == 1
    return O, mesh, ddmc, log[0], lr.outcomes(log)


@pytest.mark.parametrize("row,pattern", RUNS, ids=[f"{r.cid}-{r.bset}-{p}" for r, p in RUNS])
def test_every_row_forces_reuse_behind_awkward_predecessors(row, pattern):
    O, mesh, ddmc, call, out = _one_cycle(row, pattern)
    gone = out["n_escaped"] + out["n_absorbed"]
    levels = lr.changed_level(call, mesh)
    regimes = lr.changed_regime(call, ddmc)
    print(f"{row.cid} {row.bset} {pattern}: {out['live']} at the transport call, {gone} gone ({out['n_escaped']} escaped, "
          f"{out['n_absorbed']} absorbed), {out['n_census']} to census, {levels} changed level, {regimes} changed regime, "
          f"{O.events} events")
    for G in lr.GRIDS:
        assert out["live"] >= lr.reuse_floor(G), (G, out)
    assert gone >= lr.FLOOR and out["n_census"] >= lr.FLOOR, out
    assert out["n_census"] == O.n
    if lr.two_levels(row):
        assert levels >= lr.FLOOR, levels
    else:
        assert set(mesh.blk_level) == {0} and levels == 0
    family = lr.case_of(row).family
    if family == "hybrid":
        assert regimes >= lr.FLOOR, regimes
    elif family == "ddmc":
        assert ddmc[mesh.interior()].all()
    if row.cid == ax.HOT_CASE.id:
        assert out["n_absorbed"] >= lr.FLOOR, out         # the !NOABS forms end histories inside the loop


@pytest.mark.parametrize("row", [r for r in lr.ROWS if lr.case_of(r).family == "hybrid"], ids=lambda r: r.cid)
def test_hybrid_rows_have_both_regimes_on_both_levels(row):
    for pattern in row.patterns:
        _both_regimes_on_both_levels(lr.case_of(row), pattern)


def test_the_rank_row_hands_photons_over():
    """The two-rank run of test_gpu_lane_reuse: under the ``blocks`` decomposition of two ranks at least 256
    histories of each rank's first transport call end on a block of the other rank (``n_outgoing`` there)."""
    row = lr.RANK_ROW
    case = lr.case_of(row)
    ov = ax.overrides(case, row.bset)
    pin = load_deck(case.deck, ov)
    O, mesh, _ = hs.oracle_on(case.deck, ov, row.patterns[0], capacity_factor=row.capacity_factor)
    owner = _owners(pin, 2)
    assert set(owner) == {0, 1}
    log = lr.watch(O)
    run_oracle_cycles(O, pin, 1)
    call = log[0]
    from oracle import orc
    alive = call["status"] == orc.ST_ACTIVE
    start, end = owner[call["cell0"][0][alive]], owner[call["cell1"][0][alive]]
    for rank in (0, 1):
        at_call = int(np.count_nonzero(owner[call["cell0"][0]] == rank))
        leaving = int(np.count_nonzero((start == rank) & (end != rank)))
        print(f"rank {rank}: {at_call} photons at the transport call, {leaving} end on the other rank")
        assert at_call >= lr.reuse_floor(1)
        assert leaving >= lr.FLOOR


def _owners(pin, nranks):
    """Owner rank of every block under the ``blocks`` decomposition, as ``McblockDriver`` deals them (on a mesh of
    its own: ``Mesh.partition`` writes into it)."""
    from jaybenne_amd import mcblock
    from jaybenne_amd.mesh import Mesh
    mesh = Mesh.from_deck(pin)
    mesh.partition(nranks, cost=mcblock.block_costs(mesh, pin, mcblock.Initialize(pin)))
    return np.asarray(mesh.owner)
