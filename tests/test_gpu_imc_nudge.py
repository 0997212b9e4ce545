"""k_imc_cell nudges a photon through a cell face, and re-indexes its cell, under exec masks.

Per axis the step's comparison `|p| > m` is left by the hardware as a wave mask; with that mask in `exec` the
crossing lanes alone move the byte offset by the stride (with the sign of p) and store `-copysign(m, p)`
(`nudge_reindex_masked`, jaybenne_amd/csrc/jb_physics.hpp).  The select form it replaces stays in the source
behind `-DJB_NO_ASM_NUDGE`, in plain C++, and is what the masked form is compared with here:

* bit equality: every case runs two cycles of lean arithmetic under the release library and under a second library
  built with `-DJB_NO_ASM_NUDGE` (`make -C jaybenne_amd/csrc select_nudge`), each in a fresh child process; every
  swarm attribute and the stream state must be equal bit for bit, the tally within 1e-15 of its largest entry
  (atomics add to it in any order);
* both sides of every axis: photons placed by hand within eps_imc dx of each of the six faces of an interior
  cell, moving outward, and one at a cell edge (two axes hit in one step), against the exact variant within the
  lean tolerance (tests/test_gpu_lean.py);
* the 3-D case under the checked library: no invariant violation.

The meshes are small and thin (sigma dx = 0.5 to 1, c dt = the domain): a photon's path of one domain length crosses
a dozen cells -- block faces, the reflecting x walls and the periodic y / z faces, in both directions.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import load_deck
from test_gpu_invariants import CHECKED, RELEASE, ROOT, TESTS, _clean, checked_lib  # noqa: F401  (checked_lib: fixture)
from test_gpu_lean import _compare_within_tolerance
from test_gpu_parity import SMR_OVERRIDES

pytestmark = [pytest.mark.gpu, pytest.mark.lean, pytest.mark.timeout(900, method="thread")]

SELECT = os.path.join(ROOT, "jaybenne_amd", "libjaybenne_amd_select_nudge.so")
SCAT = "mcblock/scattering_constant_value"
N = "jaybenne/num_particles"
EPS_IMC = 1.0e6 * 10.0 * np.finfo(np.float64).eps      # transport_utils.hpp:24 (kEpsImc, jb_physics.hpp)
C_LIGHT = 2.99792458e10


def _mesh(nx, bx):
    out = {}
    for d, (n, b) in enumerate(zip(nx, bx)):
        out[f"parthenon/mesh/nx{d + 1}"] = n
        out[f"parthenon/meshblock/nx{d + 1}"] = b
    return out


CUBE8 = _mesh((8, 8, 8), (4, 4, 4))          # dx = 1 / 8: 8 blocks of 4^3; sigma dx = 0.5 with SCAT = 4
# id -> (deck, overrides, kernel dimension, NOABS)
CASES = {
    "1d": ("stepdiff", dict(_mesh((16,), (8,)), **{N: 20000, SCAT: 16.0}), 1, True),
    "2d": ("stepdiff", dict(_mesh((16, 16), (8, 8)), **{N: 20000, SCAT: 16.0}), 2, True),
    "3d": ("stepdiff", dict(CUBE8, **{N: 20000, SCAT: 4.0}), 3, True),
    "3d-absorb": ("stepdiff", dict(CUBE8, **{N: 20000, SCAT: 3.0, "mcblock/opacity_model": "constant",
                                             "mcblock/opacity_constant_value": 1.0,
                                             "mcblock/initial_temperature": 1.0e6}), 3, False),
    "2d-smr": ("stepdiff_smr", dict(SMR_OVERRIDES, **{N: 20000, SCAT: 100.0}), 2, True),   # per-lane geometry
}
CYCLES = 2
INT_KEYS = ("id", "rng", "ip", "jp", "kp", "blk", "status")
FLT_KEYS = ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e")


@pytest.fixture(scope="module")
def select_lib():
    """The select form of the nudge in every kernel: built once (a no-op when it is up to date)."""
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "jaybenne_amd", "csrc"), "select_nudge"],
                         capture_output=True, text=True, timeout=840)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return SELECT


# ---- in the child process ----------------------------------------------------------------------
def child_cycles(cid, out):
    """Two cycles of one case in lean arithmetic under the library JAYBENNE_AMD_LIB names: a snapshot after each."""
    import torch
    from jaybenne_amd import mcblock
    deck, ov, ndim, noabs = CASES[cid]
    drv = mcblock.McblockDriver(load_deck(deck, ov), device=torch.device("cuda", 0))
    assert drv.pkg.arithmetic() == "lean"
    sl = drv.mesh.interior()
    n0 = drv.md.n
    g = drv.md.get_swarm()
    save = {"init_blk": g["blk"][np.argsort(g["id"])]}
    for cyc in range(CYCLES):
        drv.Step()
        v = drv.md.lib.jb_last_transport_variant(drv.md.handle).decode()
        assert v.startswith(f"k_imc_cell<{ndim}, true, {'true' if noabs else 'false'}, lean>"), v
        g = drv.md.get_swarm()
        for k in INT_KEYS + FLT_KEYS:
            save[f"c{cyc}_{k}"] = g[k]
        save[f"c{cyc}_tally"] = drv.md.get_field("tally")[sl]
        save[f"c{cyc}_edelta"] = drv.md.get_field("edelta")[sl]
        save[f"c{cyc}_events"] = np.array([drv.md.events, drv.md.n])
    np.savez(out, **save)
    rep = drv.md.invariant_report() if drv.md.invariants_enabled() else {}
    return {"n0": n0, "events": int(drv.md.events), "stats": drv.md.stats(), "report": rep}


def _child(lib, *args, timeout=280):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), *map(str, args)], capture_output=True,
                         text=True, env=dict(os.environ, JAYBENNE_AMD_LIB=lib), timeout=timeout, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


# ---- the tests ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASES))
def test_masked_form_equals_the_select_form_bit_for_bit(gpu_device, select_lib, tmp_path, cid):
    outs = {}
    for name, lib in (("masked", RELEASE), ("select", select_lib)):
        info = _child(lib, "cycles", cid, tmp_path / f"{name}.npz")
        outs[name] = (np.load(tmp_path / f"{name}.npz"), info)
    (a, ia), (b, ib) = outs["masked"], outs["select"]
    deck, ov, ndim, noabs = CASES[cid]
    print(f"{cid}: {ia['n0']} photons, {ia['events']} events in {CYCLES} cycles, stats {ia['stats']}")
    assert ia["events"] == ib["events"]
    for k in ("n_census", "n_absorbed", "n_escaped", "n_outgoing", "n_events"):
        assert ia["stats"][k] == ib["stats"][k], k     # (wave passes and services depend on the scheduling)
    assert ia["events"] > 10 * ia["n0"]            # collisions and crossings, not one event per history
    if not noabs:
        assert ia["stats"]["n_absorbed"] > 1000
    for cyc in range(CYCLES):
        assert np.array_equal(a[f"c{cyc}_events"], b[f"c{cyc}_events"]), cyc
        # (by id: the slot order moves with DefragParticles, whose schedule depends on timing)
        oa, ob = np.argsort(a[f"c{cyc}_id"]), np.argsort(b[f"c{cyc}_id"])
        assert oa.shape == ob.shape
        for k in INT_KEYS:
            assert np.array_equal(a[f"c{cyc}_{k}"][oa], b[f"c{cyc}_{k}"][ob]), (cyc, k)
        for k in FLT_KEYS:      # bit for bit (NaN-proof: compared as integers)
            x, y = a[f"c{cyc}_{k}"][oa], b[f"c{cyc}_{k}"][ob]
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (cyc, k)
        for k in ("tally",) if noabs else ("tally", "edelta"):
            x, y = a[f"c{cyc}_{k}"], b[f"c{cyc}_{k}"]
            scale = np.abs(y).max()
            assert scale > 0.0, k
            err = np.abs(x - y).max()
            print(f"  cycle {cyc + 1} {k}: largest difference {err / scale:.2e} of the largest entry")
            assert err <= 1e-15 * scale, (k, cyc, err, scale)
    if cid == "3d":
        # the photons of the case really cross: a path of 4 mean free paths of 0.25 displaces a photon by ~0.5
        # (0.29 per axis) in blocks 0.5 wide -- well over half of them end the first cycle in another block
        assert np.array_equal(a["init_blk"], b["init_blk"])
        moved = a["c0_blk"][np.argsort(a["c0_id"])] != a["init_blk"]
        print(f"  photons in another block after one cycle: {moved.mean():.2f}")
        assert moved.mean() > 0.5


def _place(drv):
    """Seven photons of the 3-D case moved, inside their own (interior) cell, to within eps_imc dx of a face and
    pointed outward: one per face, and one at the +x / +y edge.  Returns their slots."""
    import torch
    md, mesh = drv.md, drv.mesh
    g = md.get_swarm()
    nx = np.asarray(mesh.nx)
    first = np.array([mesh.is_[0], mesh.is_[1], mesh.is_[2]])
    loc = np.stack([g["ip"], g["jp"], g["kp"]], axis=1) - first
    inner = np.flatnonzero(np.all((loc >= 1) & (loc <= nx - 2), axis=1) & (g["status"] == 0))
    assert inner.size >= 7
    slots = [int(s) for s in inner[:7]]
    faces = [(0, +1), (0, -1), (1, +1), (1, -1), (2, +1), (2, -1), None]
    keys = ("x", "y", "z")
    for s, face in zip(slots, faces):
        gid = int(md.gids[g["blk"][s]])
        dx = np.asarray(mesh.blk_dx[gid], dtype=np.float64)
        lo = np.asarray(mesh.blk_xmin[gid], dtype=np.float64) + loc[s] * dx      # the cell's lower corner
        pos = lo + 0.5 * dx
        omega = np.array([0.14, 0.14, 0.14])
        hits = [face] if face is not None else [(0, +1), (1, +1)]
        for d, sgn in hits:
            # 0.25 eps_imc dx inside the face: within the nudge width, still in the cell
            pos[d] = (lo[d] + dx[d]) - 0.25 * EPS_IMC * dx[d] if sgn > 0 else lo[d] + 0.25 * EPS_IMC * dx[d]
            omega[d] = sgn * (0.98 if face is not None else 0.7)
        omega /= np.linalg.norm(omega)
        for d, k in enumerate(keys):
            md.swarm[k][s] = float(pos[d])
            md.swarm["v" + k][s] = float(C_LIGHT * omega[d])
    torch.cuda.synchronize()
    return slots


def test_both_sides_of_every_axis_and_a_cell_edge(gpu_device):
    from jaybenne_amd import mcblock
    deck, ov, ndim, noabs = CASES["3d"]
    out = {}
    for mode in ("lean", "exact"):
        drv = mcblock.McblockDriver(load_deck(deck, ov), device=gpu_device)
        drv.pkg.set_arithmetic(mode)
        slots = _place(drv)
        before = drv.md.get_swarm()
        drv.Step()
        v = drv.md.lib.jb_last_transport_variant(drv.md.handle).decode()
        assert v.startswith("k_imc_cell<3, true, true, lean>") if mode == "lean" else v.endswith("false>"), v
        out[mode] = (drv.md.get_swarm(), drv.md.n, drv.md.events, drv.mesh, slots, before)
    (g, n, ev, mesh, slots, before), (h, m, ev2, _, slots2, before2) = out["lean"], out["exact"]
    assert slots == slots2 and n == m and ev == ev2
    for k in ("x", "y", "z", "vx", "vy", "vz", "id"):
        assert np.array_equal(before[k], before2[k]), k          # the same hand-placed start
    _compare_within_tolerance(g, h, n, mesh, load_deck(deck, ov).GetReal("jaybenne", "dt"), by_id=True, tol=1e-9)
    for k in ("ip", "jp", "kp", "blk", "status"):
        assert np.array_equal(g[k], h[k]), k


def test_checked_library_sees_no_violation(gpu_device, checked_lib, tmp_path):
    """The 3-D case with the transport invariants evaluated on every pass: position inside the cell, offset naming
    an interior cell, no collision in the step that left the block."""
    info = _child(CHECKED, "cycles", "3d", tmp_path / "checked.npz")
    rep = info["report"]
    _clean(rep)
    assert rep["passes"]["imc_cell"] > 0, rep
    assert rep["evaluated"]["INDEX"] >= rep["passes"]["imc_cell"], rep


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    print(json.dumps(child_cycles(sys.argv[2], sys.argv[3])))
