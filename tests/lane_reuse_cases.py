"""The cases that put many photons through every lane of a tracking kernel, and what the CPU oracle says about them.

A lane of a tracking kernel is persistent: it finishes a history, writes it back, claims the next slot
(jb_scaffold.hpp: claim_exact, refill_chunk) and goes on with whatever of its state the refill did not set again.
``launch_persistent`` sizes the grid to the chip, so on the small swarms the oracle can follow every lane gets one
photon; ``JB_TRANSPORT_MAX_BLOCKS=G`` caps the grid at G workgroups of 256 lanes and the same swarms then put tens
of photons through every lane.  The rows below are cases of tests/axis_cases.py (outflow faces, two levels, unequal
axes, boundary kinds that differ per face) on ``hetero_states`` material, one boundary set each.

tests/test_lane_reuse_host.py (CPU) checks on the oracle alone that every row forces the reuse and makes the awkward
predecessors common; tests/test_gpu_lane_reuse.py runs the kernels.  Both import the table and ``watch`` below.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import axis_cases as ax
import hetero_states as hs

BLOCK = 256                       # lanes of a workgroup (jb_limits.hpp: kBlock)
GRIDS = (1, 3)                    # the caps the GPU tests run
PER_LANE = {1: 8, 3: 4}           # photons per lane a row must force at each cap
FLOOR = 256                       # histories of a kind: one per lane of a workgroup on average

# (case of axis_cases, boundary set, patterns the GPU tests run it on, capacity factor of swarm and oracle)
Row = namedtuple("Row", "cid bset patterns capacity_factor")
ROWS = [
    Row("G1-imc", "RO", ("smooth",), 1.3),
    Row("G2S-imc", "S1", ("smooth",), 1.3),
    Row("G3U-imc", "S3", ("smooth",), 1.3),
    Row("G3S-imc", "S3", ("smooth",), 1.3),
    Row("G3S-hot", "S1", ("hot_spots",), 8.0),
    Row("G3O-imc", "S3", ("smooth",), 1.3),
    Row("G1-ddmc", "OR", ("palette3",), 1.3),
    Row("G2S-ddmc", "S1", ("palette2", "smooth_dense"), 1.3),
    Row("G3S-ddmc", "S3", ("stripes3", "smooth_dense"), 1.3),
    Row("G2S-hybrid", "S1", ("islands",), 1.3),
    Row("G3S-hybrid", "S3", ("islands",), 1.3),
    Row("G2O-hybrid", "S1", ("islands",), 1.3),
]
BY_ID = {r.cid: r for r in ROWS}
for _r in ROWS:
    if (_r.cid, _r.bset) in ax.DDMC_PALETTE:
        assert _r.patterns[0] == ax.DDMC_PALETTE[_r.cid, _r.bset], _r
# the two-rank run: a lane that last held a photon on its way to the other rank
RANK_ROW = Row("G3S-hybrid", "S1", ("islands",), 2.0)


def case_of(row):
    return ax.HOT_CASE if row.cid == ax.HOT_CASE.id else ax.BY_ID[row.cid]


def two_levels(row):
    return ax.GEOMETRIES[case_of(row).geom].refine is not None


def reuse_floor(G):
    """Photons at the transport call from which on G workgroups must follow PER_LANE[G] of them per lane."""
    return PER_LANE[G] * BLOCK * G


def watch(O):
    """Have the oracle keep, for every TransportPhotons call from now on, who went in and what became of them:
    a list of {"id", "status", "cell0", "cell1"} per call (cell: (blk, kp, jp, ip), as
    ``hetero_states.swarm_cells``; the end values of a history that did not reach census mean nothing).  The
    tracking loop works in place and compaction comes behind it, so slot q is the same photon on both sides."""
    log = []
    inner = O.TransportPhotons

    def transport(t_start, dt, first=0, last=None):
        n = O.n
        ids = O.sw["id"][:n].copy()
        cell0 = tuple(a.copy() for a in hs.swarm_cells(O.mesh, O.sw, n))
        ev = inner(t_start, dt, first, last)
        assert O.n == n and np.array_equal(O.sw["id"][:n], ids)
        cell1 = tuple(a.copy() for a in hs.swarm_cells(O.mesh, O.sw, n))
        log.append(dict(id=ids, status=O.sw["status"][:n].copy(), cell0=cell0, cell1=cell1))
        return ev

    O.TransportPhotons = transport
    return log


def outcomes(log):
    """{"live": photons at the transport calls, "n_census", "n_absorbed", "n_escaped", "n_outgoing"} summed over
    the calls: the names of ``MeshData.stats()``; the oracle holds the whole mesh, nothing is outgoing."""
    from oracle import orc
    out = dict(live=0, n_census=0, n_absorbed=0, n_escaped=0, n_outgoing=0)
    for call in log:
        st = call["status"]
        out["live"] += len(st)
        out["n_census"] += int(np.count_nonzero(st == orc.ST_ACTIVE))
        out["n_absorbed"] += int(np.count_nonzero(st == orc.ST_ABSORBED))
        out["n_escaped"] += int(np.count_nonzero(st == orc.ST_ESCAPED))
    assert out["live"] == out["n_census"] + out["n_absorbed"] + out["n_escaped"]
    return out


def changed_level(call, mesh):
    """Survivors of a transport call that ended on a block of another level than they started on."""
    from oracle import orc
    alive = call["status"] == orc.ST_ACTIVE
    lev = np.asarray(mesh.blk_level)
    return int(np.count_nonzero(lev[call["cell0"][0][alive]] != lev[call["cell1"][0][alive]]))


def changed_regime(call, ddmc):
    """Survivors that started in a DDMC cell and ended in an IMC cell or the reverse (``ddmc``:
    ``hetero_states.regime_map``): each took steps of both kinds."""
    from oracle import orc
    alive = call["status"] == orc.ST_ACTIVE
    a = ddmc[tuple(c[alive] for c in call["cell0"])]
    b = ddmc[tuple(c[alive] for c in call["cell1"])]
    return int(np.count_nonzero(a != b))
