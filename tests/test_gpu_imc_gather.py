"""k_imc_cell gathers a photon's mean free paths only when the photon changes cell.

A lane that scatters, is absorbed or reaches census inside its cell keeps the `lam_s` (and `lam_a`) it holds;
only a step that puts the photon through a cell face -- and the ghost, wall, level-change, relocation and refill
paths, each of which sets the cell offset itself -- requests the new cell's values.  A fetch that does not follow
the offset leaves a stale mean free path in the lane, i.e. a wrong collision distance in the next cell, so every
case here runs on material that differs from cell to cell: rho and sie are drawn per interior cell from a seeded
generator (ghost cells filled from their owners), which makes `lam_s`, and `lam_a` where the material absorbs,
different between neighbouring cells and between the ghost-adjacent cells of neighbouring blocks.

Each case runs the lean kernel and the exact variant (`k_transport<..., false>`, held bit for bit to the oracle by
tests/test_gpu_parity.py and tests/test_gpu_hetero.py) from the same state on the same streams for two cycles
and applies the tolerance tests/test_gpu_lean.py states: integer attributes and stream states equal,
floating-point attributes and the tally (and `edelta` where the material absorbs) within 1e-9 after one cycle and
1e-8 after two.

The thin and the thick deck are the two extremes of the predicate: sigma dx = 0.05 (nearly every event is a
crossing: the fetch is issued nearly every pass) and sigma dx = 50 (nearly every event is a same-cell scatter:
the held value is used ~50 times between fetches).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import load_deck
from test_gpu_invariants import CHECKED, ROOT, TESTS, _clean, checked_lib  # noqa: F401  (checked_lib: fixture)
from test_gpu_lean import _compare_within_tolerance
from test_gpu_parity import SMR3D, SMR_OVERRIDES

pytestmark = [pytest.mark.gpu, pytest.mark.lean]

SCAT = "mcblock/scattering_constant_value"


class SeededMaterial:
    """``initial_state=`` for ``McblockDriver``: the problem generator's rho and sie times a factor drawn per cell
    from a seeded generator (rho in [0.6, 1.4], sie in [0.8, 1.2] of the deck's), ghosts from their owners."""

    def __init__(self, seed):
        self.seed = seed

    def __call__(self, mesh, pkg, gids=None):
        from jaybenne_amd import mcblock
        ic = mcblock.ProblemGenerator(mesh, pkg)
        rng = np.random.default_rng(self.seed)
        rho = ic["rho"] * rng.uniform(0.6, 1.4, ic["rho"].shape)
        sie = ic["sie"] * rng.uniform(0.8, 1.2, ic["sie"].shape)
        mesh.fill_ghosts(rho)
        mesh.fill_ghosts(sie)
        out = {"rho": rho, "sie": sie, "u": rho * sie}
        if gids is not None:
            out = {k: np.ascontiguousarray(v[np.asarray(gids)]) for k, v in out.items()}
        return out


def _mesh(nx, bx):
    out = {}
    for d, (n, b) in enumerate(zip(nx, bx)):
        out[f"parthenon/mesh/nx{d + 1}"] = n
        out[f"parthenon/meshblock/nx{d + 1}"] = b
    return out


# 16^3 cells on [-0.5, 0.5]^3 in 8 blocks of 8^3: dx = 1 / 16; reflecting walls in x, periodic in y and z (the deck's)
CUBE16 = _mesh((16, 16, 16), (8, 8, 8))
OUTFLOW_1D = {"parthenon/swarm/ix1_bc": "outflow", "parthenon/swarm/ox1_bc": "outflow"}
# (id, deck, overrides, kernel dimension, NOABS)
CASES = [
    # sigma dx = 4, as the headline workload: same-cell scatters and crossings both frequent
    ("3d-scatter", "stepdiff", dict(CUBE16, **{"jaybenne/num_particles": 20000, SCAT: 64.0}), 3, True),
    # ... with absorption (sigma_a dx = 1 / 16: about a third of the photons survive a cycle): lam_a is held too
    ("3d-absorb", "stepdiff", dict(CUBE16, **{"jaybenne/num_particles": 20000, SCAT: 63.0,
                                              "mcblock/opacity_model": "constant",
                                              "mcblock/opacity_constant_value": 1.0,
                                              "mcblock/initial_temperature": 1.0e6}), 3, False),
    # two levels: cross_level changes the offset and the geometry
    ("2d-smr", "stepdiff_smr", dict(SMR_OVERRIDES, **{"jaybenne/num_particles": 20000, SCAT: 100.0}), 2, True),
    ("3d-smr", "stepdiff_smr", dict(SMR3D, **{"jaybenne/num_particles": 20000, SCAT: 50.0}), 3, True),
    # 1-D, 64 cells in 2 blocks, both ends open (sigma dx = 1): escapes and the general relocation
    ("1d-outflow", "stepdiff", dict(_mesh((64,), (32,)), **OUTFLOW_1D, **{"jaybenne/num_particles": 10000, SCAT: 64.0}),
     1, True),
    ("3d-thin", "stepdiff", dict(CUBE16, **{"jaybenne/num_particles": 20000, SCAT: 0.8}), 3, True),      # sigma dx = 0.05
    ("3d-thick", "stepdiff", dict(CUBE16, **{"jaybenne/num_particles": 20000, SCAT: 800.0}), 3, True),   # sigma dx = 50
]
SEED = 20240611
CYCLES = 2
TOL = (1e-9, 1e-8)      # after one / two cycles (tests/test_gpu_lean.py)


def _run(case, mode, device):
    """Two cycles of one case in one arithmetic variant: a snapshot after each."""
    from jaybenne_amd import mcblock
    cid, deck, ov, ndim, noabs = case
    drv = mcblock.McblockDriver(load_deck(deck, ov), device=device, initial_state=SeededMaterial(SEED))
    drv.pkg.set_arithmetic(mode)
    sl = drv.mesh.interior()
    snaps = []
    for _ in range(CYCLES):
        drv.Step()
        v = drv.md.lib.jb_last_transport_variant(drv.md.handle).decode()
        if mode == "lean":
            assert v.startswith(f"k_imc_cell<{ndim}, true, {'true' if noabs else 'false'}, lean>"), v
        else:
            assert f"k_transport<{ndim}," in v and v.endswith("false>"), v
        snaps.append({"sw": drv.md.get_swarm(), "n": drv.md.n, "events": drv.md.events, "stats": drv.md.stats(),
                      "tally": drv.md.get_field("tally")[sl].copy(), "edelta": drv.md.get_field("edelta")[sl].copy()})
    return drv, snaps


def _material_differs(drv):
    """Every interior cell's density differs from its neighbour's along every active axis."""
    sl = drv.mesh.interior()
    rho = drv.md.get_field("rho")[sl]
    for ax in range(1, 1 + 3):
        if rho.shape[ax] > 1:
            assert np.all(np.diff(rho, axis=ax) != 0.0)


def _compare(case, drv, lean, exact, dt):
    cid, deck, ov, ndim, noabs = case
    for cyc, (a, b) in enumerate(zip(lean, exact)):
        tol = TOL[cyc]
        print(f"{cid} cycle {cyc + 1}: {a['n']} photons, {a['events']} events, stats {a['stats']}")
        assert a["n"] == b["n"] and a["events"] == b["events"], (cyc, a["n"], b["n"], a["events"], b["events"])
        _compare_within_tolerance(a["sw"], b["sw"], b["n"], drv.mesh, dt, by_id=True, tol=tol)
        for k in ("tally",) if noabs else ("tally", "edelta"):
            scale = np.abs(b[k]).max()
            assert scale > 0.0, k
            err = np.abs(a[k] - b[k]).max()
            print(f"  {k}: largest difference {err / scale:.2e} of the largest entry")
            assert err <= tol * scale, (k, cyc, err, scale)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_lean_kernel_follows_the_cell_on_random_material(gpu_device, case):
    cid, deck, ov, ndim, noabs = case
    drv, lean = _run(case, "lean", gpu_device)
    _material_differs(drv)
    _, exact = _run(case, "exact", gpu_device)
    n0 = int(ov["jaybenne/num_particles"])
    ev = lean[0]["events"] / max(n0, 1)
    if cid == "3d-thin":
        assert ev < 40            # ~16 crossings and ~1 scatter per history and cycle
    elif cid == "3d-thick":
        assert ev > 600           # ~800 scatters per history and cycle
    else:
        assert ev > 20            # collisions and crossings, not one event per history
    if cid == "1d-outflow":
        assert lean[-1]["stats"]["n_escaped"] > 100
    if not noabs:
        assert lean[0]["stats"]["n_absorbed"] > 1000 and lean[-1]["n"] > 1000
    _compare(case, drv, lean, exact, load_deck(deck, ov).GetReal("jaybenne", "dt"))


# ---- one case under the checked library --------------------------------------------------------
def child_case():
    import torch
    case = CASES[0]
    dev = torch.device("cuda", 0)
    drv, lean = _run(case, "lean", dev)
    assert drv.md.invariants_enabled()
    rep = drv.md.invariant_report()
    _, exact = _run(case, "exact", dev)
    _compare(case, drv, lean, exact, load_deck(case[1], case[2]).GetReal("jaybenne", "dt"))
    return rep


@pytest.mark.timeout(900, method="thread")
def test_checked_library_sees_no_violation(gpu_device, checked_lib):
    """The 3-D scattering case with the transport invariants evaluated on every pass: position inside the cell,
    offset naming an interior cell, no collision in the step that left the block."""
    res = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True,
                         env=dict(os.environ, JAYBENNE_AMD_LIB=CHECKED), timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    rep = json.loads(res.stdout.strip().splitlines()[-1])
    _clean(rep)
    assert rep["passes"]["imc_cell"] > 0, rep
    assert rep["evaluated"]["INDEX"] >= rep["passes"]["imc_cell"], rep
    assert rep["evaluated"]["EVENT_OFF_BLOCK"] > 0, rep


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    print(json.dumps(child_case()))
