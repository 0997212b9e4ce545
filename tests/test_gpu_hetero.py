"""Every tracking kernel on material that differs from cell to cell (tests/hetero_states.py), against the CPU
oracle started from the same arrays.  On the parity decks rho is one number, so a gather from the wrong cell
returns the right bits; here a one-cell shift of the state changes at least 5 % of the photons
(tests/test_hetero_host.py), and the comparisons are the project's own: bit-equality in exact arithmetic, 1e-12
on fields, 1e-9 / 1e-8 for lean after one / two cycles, 1e-11 after feedback."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hetero_states as hs
from helpers import load_deck, make_oracle, run_oracle_cycles
from test_gpu_invariants import CHECKED, ROOT, TESTS, _clean, checked_lib  # noqa: F401  (checked_lib: fixture)
from test_gpu_parity import _compare_fields, _compare_swarm, _compare_swarm_by_id

pytestmark = pytest.mark.gpu


def _pair(deck, ov, pattern, device, salt=0, capacity_factor=1.3):
    """The device problem and the oracle from the same heterogeneous state."""
    from jaybenne_amd import mcblock
    from oracle import orc
    st = hs.state_for(deck, ov, pattern, salt=salt)
    pin = load_deck(deck, ov)
    drv = mcblock.McblockDriver(pin, device=device, initial_state=st, capacity_factor=capacity_factor)
    O, mesh, pkg = make_oracle(load_deck(deck, ov), orc.MATH_PORTABLE, initial_state=st,
                               capacity_factor=capacity_factor)
    return pin, drv, O, mesh, pkg


def _variant(drv):
    return drv.md.lib.jb_last_transport_variant(drv.md.handle).decode()


def _compare_start(drv, O, use_ddmc):
    """Sourcing and the derived fields before the first step."""
    from jaybenne_amd import jaybenne as jb
    m = drv.mesh
    _compare_swarm(drv.md, O)
    jb.UpdateDerivedTransportFields(drv.md, drv.dt)
    O.UpdateDerivedTransportFields(drv.dt)
    _compare_fields(drv.md, O, ("fleck", "src_num", "src_ew"))
    if use_ddmc:
        for d, name in enumerate(("P1", "P2", "P3")[:m.ndim]):
            sl = tuple([slice(None)] + [slice(m.is_[dd], m.is_[dd] + m.nx[dd] + (1 if dd == d else 0))
                                        for dd in (2, 1, 0)])
            a, b = drv.md.get_field(name)[sl], O.fields[name][sl]
            assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), name
            assert len(np.unique(b)) > 2, name       # (the field really varies)


def _steps(drv, O, pin, cycles):
    for _ in range(cycles):
        drv.Step()
    run_oracle_cycles(O, pin, cycles)


def _compare_end(drv, O):
    _compare_swarm(drv.md, O)
    _compare_fields(drv.md, O)
    assert drv.md.events == O.events


def _compare_lean(drv, O, mesh, pin, cycles, by_id=False):
    from test_gpu_lean import _compare_within_tolerance
    assert drv.md.n == O.n and drv.md.events == O.events
    _compare_within_tolerance(drv.md.get_swarm(), O.sw, O.n, mesh, pin.GetReal("jaybenne", "dt"), by_id=by_id,
                              tol=1e-9 if cycles == 1 else 1e-8)
    sl = mesh.interior()
    a, b = drv.md.get_field("tally")[sl], O.fields["tally"][drv.md.gids][sl]
    assert np.abs(a - b).max() <= (1e-9 if cycles == 1 else 1e-8) * np.abs(b).max()


# ---- a. pure IMC, exact arithmetic -------------------------------------------------------------
@pytest.mark.parametrize("cid,deck,ov,pattern,ndim", hs.IMC_CASES, ids=[c[0] for c in hs.IMC_CASES])
def test_imc_exact_on_smooth_density(gpu_device, cid, deck, ov, pattern, ndim):
    pin, drv, O, mesh, _ = _pair(deck, ov, pattern, gpu_device)
    _compare_start(drv, O, False)
    _steps(drv, O, pin, 1)
    v = _variant(drv)
    assert f"k_transport<{ndim}," in v and v.endswith("false>"), v
    assert 20 * O.n < O.events        # collisions and crossings, not one event per history
    _compare_end(drv, O)


def test_imc_exact_on_hot_spots_with_absorption(gpu_device):
    cid, deck, ov, pattern, ndim = hs.IMC_HOT_CASE
    pin, drv, O, mesh, _ = _pair(deck, ov, pattern, gpu_device, capacity_factor=8.0)
    _compare_start(drv, O, False)
    _steps(drv, O, pin, 1)
    assert f"k_transport<{ndim}," in _variant(drv)
    assert drv.md.stats()["n_absorbed"] > 500 and O.n > 500
    _compare_swarm_by_id(drv.md, O)
    _compare_fields(drv.md, O, ("tally", "fleck", "src_num", "src_ew"))
    f = O.fields["fleck"][mesh.interior()]
    assert len(np.unique(f)) > 0.4 * f.size       # a Fleck factor of its own in (nearly) every cell
    assert drv.md.events == O.events


# ---- b. pure IMC, lean -------------------------------------------------------------------------
LEAN_IMC = [(c, None) for c in hs.IMC_CASES] + [(hs.IMC_CASES[3], "1")]


@pytest.mark.lean
@pytest.mark.parametrize("case,no_cell", LEAN_IMC, ids=[c[0] + ("-x-space" if e else "") for c, e in LEAN_IMC])
def test_imc_lean_on_smooth_density(gpu_device, case, no_cell, monkeypatch):
    cid, deck, ov, pattern, ndim = case
    if no_cell:
        monkeypatch.setenv("JB_NO_IMC_CELL", no_cell)
    pin, drv, O, mesh, _ = _pair(deck, ov, pattern, gpu_device)
    assert drv.pkg.arithmetic() == "lean"
    _steps(drv, O, pin, 1)
    v = _variant(drv)
    if no_cell:
        assert f"k_transport<{ndim}," in v and v.endswith("true>"), v
    else:
        assert f"k_imc_cell<{ndim}," in v, v
    _compare_lean(drv, O, mesh, pin, 1)


# ---- c. all-DDMC -------------------------------------------------------------------------------
GATHERS = [(m, f) for m in hs.DDMC_MESHES for f in hs.DDMC_GATHERS] + [(hs.DDMC_MESHES[0], "lds")]


@pytest.mark.parametrize("mesh_case,form", GATHERS, ids=[f"{m[0]}-{f}" for m, f in GATHERS])
def test_ddmc_64_byte_gathers_on_smooth_density(gpu_device, mesh_case, form, monkeypatch):
    name, deck, ov, ndim = mesh_case
    monkeypatch.delenv("JB_COOP_GATHER", raising=False)
    if form in ("0", "1", "2"):
        monkeypatch.setenv("JB_COOP_GATHER", form)
    elif form == "lds":
        monkeypatch.setenv("JB_DDMC_QUEUES", "0")
    pin, drv, O, mesh, pkg = _pair(deck, ov, "smooth_dense", gpu_device)
    _compare_start(drv, O, True)
    ncpu = hs.class_count(mesh, pkg, O)
    _steps(drv, O, pin, 2)
    v = _variant(drv)
    ndev = drv.md.lib.jb_mesh_ddmc_classes(drv.md.handle)
    assert f"k_ddmc_all<{ndim}, true" in v, v
    if ncpu <= 256:
        assert ndev == ncpu, (ndev, ncpu)
    else:
        assert ndev > 256, ndev
    if form == "0":
        assert v.endswith(f"k_ddmc_all<{ndim}, true>"), v
    elif form in ("1", "2"):
        assert "quad gather" in v, v
    elif form == "lds":
        assert "records in LDS" in v, v
    else:       # the library's choice: codes where the classes fit the table, a 64-byte form where they do not
        assert ("cell codes" in v) == (ncpu <= 256), v
    _compare_end(drv, O)


CODES = [(m, c) for m in hs.DDMC_MESHES for c in hs.DDMC_CODES]


@pytest.mark.parametrize("mesh_case,mode", CODES, ids=[f"{m[0]}-{c}" for m, c in CODES])
def test_ddmc_cell_codes_on_palettes(gpu_device, mesh_case, mode, monkeypatch):
    """The switches of test_cell_codes_on_all_ddmc_meshes, on many classes."""
    name, deck, ov, ndim = mesh_case
    monkeypatch.delenv("JB_COOP_GATHER", raising=False)
    if mode == "forced":
        monkeypatch.setenv("JB_COOP_GATHER", "4")
    elif mode.startswith("queues"):
        monkeypatch.setenv("JB_DDMC_QUEUES", "1")
        monkeypatch.setenv("JB_DDMC_LDS_CODES", "1" if mode == "queues" else "0")
    else:
        monkeypatch.setenv("JB_DDMC_MAX_CLASSES", "1" if mode == "one class allowed" else "0")
    pin, drv, O, mesh, pkg = _pair(deck, ov, hs.DDMC_PALETTE[name], gpu_device)
    ncpu = None
    if mode == "forced":
        _compare_start(drv, O, True)
        ncpu = hs.class_count(mesh, pkg, O)
    _steps(drv, O, pin, 2)
    v = _variant(drv)
    if mode == "forced":
        assert "cell codes" in v and "queues" not in v, v
        assert drv.md.lib.jb_mesh_ddmc_classes(drv.md.handle) == ncpu
    elif mode.startswith("queues"):
        assert "cell codes" in v and ("queues" in v) == (drv.md.nblocks <= 64), v
        small = drv.md.nblocks <= 64 and drv.md.nblocks * mesh.ntot <= 1024
        assert ("codes in LDS" in v) == (mode == "queues" and small), v
    else:
        assert "k_ddmc_all" in v and "cell codes" not in v, v
    _compare_end(drv, O)


# ---- d. re-dealt classes -----------------------------------------------------------------------
REDEAL = (("palette2", 0), ("palette2", 1), ("stripes3", 0))


def _redealt(device):
    """3-D all-DDMC mesh on k_ddmc_q: another deal of the densities before every cycle, so every class number
    changes its meaning while the class table is never cleared."""
    name, deck, ov, ndim = hs.DDMC_MESHES[2]
    pin, drv, O, mesh, pkg = _pair(deck, ov, REDEAL[0][0], device, salt=REDEAL[0][1])
    dt = pin.GetReal("jaybenne", "dt")
    t = 0.0
    seen = []
    for cyc, (pattern, salt) in enumerate(REDEAL):
        if cyc > 0:
            ic = hs.initial_state(mesh, pkg, pattern, salt=salt, tau_ddmc=pin.GetOrAddReal("jaybenne", "tau_ddmc", 5.0))
            for k in ("rho", "sie", "u"):
                O.fields[k][...] = ic[k]
                drv.md.set_field(k, ic[k])
        drv.Step()
        O.RadiationStep(t, dt)
        t += dt
        v = _variant(drv)
        assert "cell codes, queues" in v, v
        seen.append(drv.md.lib.jb_mesh_ddmc_classes(drv.md.handle))
        _compare_end(drv, O)
    assert len(set(seen)) > 1 or seen[0] > 64, seen
    return drv


def test_ddmc_classes_dealt_again_every_cycle(gpu_device, monkeypatch):
    monkeypatch.delenv("JB_COOP_GATHER", raising=False)
    monkeypatch.setenv("JB_DDMC_QUEUES", "1")
    _redealt(gpu_device)


# ---- e. hybrid ---------------------------------------------------------------------------------
HYB = [pytest.param(m, p, a, marks=[pytest.mark.lean] if a == "lean" else [], id=f"{m[0]}-{p}-{a}")
       for m in hs.HYBRID_MESHES for p in hs.HYBRID_PATTERNS for a in ("exact", "lean")]


@pytest.mark.parametrize("mesh_case,pattern,arith", HYB)
def test_hybrid_with_interfaces_inside_blocks(gpu_device, mesh_case, pattern, arith):
    name, deck, ov, cycles = mesh_case
    pin, drv, O, mesh, pkg = _pair(deck, ov, pattern, gpu_device)
    assert drv.pkg.arithmetic() == arith
    if arith == "exact":
        _compare_start(drv, O, True)
    ddmc = hs.regime_map(mesh, pkg, O.fields["rho"], pin.GetOrAddReal("jaybenne", "tau_ddmc", 5.0))
    g0 = drv.md.get_swarm()
    drv.Step()
    g1 = drv.md.get_swarm()
    # the interface is crossed, in both directions, on the device too
    to_ddmc, to_imc = hs.regime_crossings(ddmc, hs.swarm_cells(mesh, g0, len(g0["id"])),
                                          hs.swarm_cells(mesh, g1, len(g1["id"])))
    assert to_ddmc >= 0.02 and to_imc >= 0.02, (to_ddmc, to_imc)
    for _ in range(cycles - 1):
        drv.Step()
    run_oracle_cycles(O, pin, cycles)
    v = _variant(drv)
    assert f"k_hybrid<{mesh.ndim}, {arith}" in v, v
    if arith == "exact":
        _compare_end(drv, O)
    else:
        _compare_lean(drv, O, mesh, pin, cycles)


def test_hybrid_islands_with_per_event_opacities(gpu_device, monkeypatch):
    name, deck, ov, _ = hs.HYBRID_MESHES[0]
    monkeypatch.setenv("JB_PER_EVENT_OPACITY", "1")
    pin, drv, O, mesh, _ = _pair(deck, ov, "islands", gpu_device)
    monkeypatch.delenv("JB_PER_EVENT_OPACITY")
    _steps(drv, O, pin, 1)
    assert "k_transport<2," in _variant(drv), _variant(drv)
    _compare_end(drv, O)


def test_general_kernel_on_an_all_ddmc_mesh_with_smooth_density(gpu_device, monkeypatch):
    name, deck, ov, ndim = hs.DDMC_MESHES[1]
    monkeypatch.setenv("JB_NO_DDMC_ALL", "1")
    pin, drv, O, mesh, _ = _pair(deck, ov, "smooth_dense", gpu_device)
    _steps(drv, O, pin, 2)
    assert f"k_hybrid<{ndim}" in _variant(drv), _variant(drv)
    _compare_end(drv, O)


# ---- f. feedback in 2-D ------------------------------------------------------------------------
def test_feedback_on_hot_islands_in_2d(gpu_device):
    """Absorption, emission and feedback on the 2-D hybrid deck: the device's ghost refresh of u runs on a field
    that varies across a level boundary; u is compared ghost cells included after every cycle."""
    deck, ov, pattern, cycles = hs.FEEDBACK_CASE
    pin, drv, O, mesh, _ = _pair(deck, ov, pattern, gpu_device, capacity_factor=8.0)
    dt = pin.GetReal("jaybenne", "dt")
    t = 0.0
    for cyc in range(cycles):
        drv.Step()
        O.RadiationStep(t, dt)
        mesh.fill_ghosts(O.fields["u"])
        O.fields["sie"][...] = O.fields["u"] / O.fields["rho"]
        t += dt
        _compare_swarm_by_id(drv.md, O, exact=cyc == 0)
        sl = mesh.interior()
        emitted = np.where(O.fields["src_num"][sl] > 0, O.fields["src_num"][sl] * O.fields["src_ew"][sl], 0.0)
        _compare_fields(drv.md, O, ("tally", "fleck", "u"))
        _compare_fields(drv.md, O, ("edelta",), scale=emitted)
        u = drv.md.fields["u"].cpu().numpy()
        assert np.all(np.abs(u - O.fields["u"]) <= 1e-12 * np.abs(O.fields["u"])), cyc
    assert "k_hybrid<2" in _variant(drv)
    assert drv.md.stats()["n_absorbed"] > 1000


# ---- g. several ranks --------------------------------------------------------------------------
def _rank_worker(rank, world, port, case, outdir, decomposition, handoff, halo_rings):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_HANDOFF=handoff)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import mcblock
        from jaybenne_amd.comm import Comm
        cid, deck, ov, pattern, cycles = hs.RANK_CASES[case]
        drv = mcblock.McblockDriver(load_deck(deck, ov), rank=rank, nranks=world, comm=Comm(),
                                    device=torch.device("cuda", 0), capacity_factor=2.0, halo_rings=halo_rings,
                                    decomposition=decomposition, initial_state=hs.state_for(deck, ov, pattern))
        assert drv.decomposition == decomposition
        for _ in range(cycles):
            drv.Step()
        g = drv.md.get_swarm()
        g["gblk"] = drv.md.gids[g["blk"]]
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), tally=drv.md.get_field("tally"), gids=drv.md.gids,
                 resident=drv.md.resident_gids, rho=drv.md.fields["rho"].cpu().numpy(),
                 events=np.array([drv.md.events]), **g)
    finally:
        dist.destroy_process_group()


RANKS = [(0, 2, "blocks", "c", 1), (0, 4, "blocks", "step", 2), (1, 2, "blocks", "step", 2), (1, 4, "blocks", "c", 1),
         (1, 2, "replicated", "c", 1), (2, 4, "blocks", "c", 1), (2, 2, "blocks", "step", 1),
         (3, 2, "blocks", "c", 1), (3, 4, "replicated", "c", 1), (3, 4, "blocks", "step", 1)]


@pytest.mark.parametrize("case,world,decomposition,handoff,halo_rings", RANKS)
def test_ranks_on_heterogeneous_material(gpu_device, case, world, decomposition, handoff, halo_rings, tmp_path):
    """Halo copies of a field that is not constant: the union of the ranks' swarms is the oracle's."""
    import torch.multiprocessing as mp
    from oracle import orc
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, TESTS)
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, case, str(tmp_path), decomposition, handoff,
                                                    halo_rings)) for r in range(world)]
    _run_workers(procs)
    cid, deck, ov, pattern, cycles = hs.RANK_CASES[case]
    pin = load_deck(deck, ov)
    O, mesh, _ = hs.oracle_on(deck, ov, pattern)
    rho0 = O.fields["rho"].copy()
    run_oracle_cycles(O, pin, cycles)
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    ids = np.concatenate([p["id"] for p in parts])
    order = np.argsort(ids)
    oo = np.argsort(O.sw["id"][:O.n])
    assert len(ids) == O.n and np.array_equal(ids[order], O.sw["id"][:O.n][oo])
    for k in ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e", "ip", "jp", "kp", "rng"):
        assert np.array_equal(np.concatenate([p[k] for p in parts])[order], O.sw[k][:O.n][oo]), k
    assert np.array_equal(np.concatenate([p["gblk"] for p in parts])[order], O.sw["blk"][:O.n][oo])
    sl = mesh.interior()
    for p in parts:
        if decomposition == "blocks":
            assert len(p["resident"]) > len(p["gids"])               # halo copies in use
        assert np.array_equal(p["rho"], rho0[p["resident"]])         # ... holding their owner's cells, ghosts too
        np.testing.assert_allclose(p["tally"][sl], O.fields["tally"][p["gids"]][sl], rtol=1e-12, atol=0)
    assert sum(int(p["events"][0]) for p in parts) == O.events


# ---- h. (and d.) under the checked library -----------------------------------------------------
def child_case(kind):
    import torch
    dev = torch.device("cuda", 0)
    if kind == "redeal":
        drv = _redealt(dev)
    else:
        if kind == "hybrid":
            _, deck, ov, _ = hs.HYBRID_MESHES[0]
            pattern = "islands"
        else:
            _, deck, ov, pattern, _ = hs.IMC_CASES[2]
        pin, drv, O, mesh, _ = _pair(deck, ov, pattern, dev)
        _steps(drv, O, pin, 1)
        _compare_end(drv, O)
    assert drv.md.invariants_enabled()
    rep = drv.md.invariant_report()
    rep["variant"] = _variant(drv)
    return rep


def _child(kind, env=None):
    e = dict(os.environ, JAYBENNE_AMD_LIB=CHECKED, **(env or {}))
    e.pop("JB_COOP_GATHER", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), kind], capture_output=True, text=True, env=e,
                         timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.timeout(900, method="thread")
@pytest.mark.parametrize("kind,family", [("hybrid", "hybrid"), ("imc3d", "transport")])
def test_checked_library_on_heterogeneous_material(gpu_device, checked_lib, kind, family):
    rep = _child(kind)
    _clean(rep)
    assert rep["passes"][family] > 0, rep
    assert rep["evaluated"]["INDEX"] >= rep["passes"][family], rep


@pytest.mark.timeout(900, method="thread")
def test_dealt_again_classes_equal_the_cells_own_records(gpu_device, checked_lib):
    """DDMC_CLASS on every interior cell in each of the three cycles, zero violations: the check the stale-class
    finding asked for, on a mesh whose class numbers change meaning every cycle."""
    rep = _child("redeal", env={"JB_DDMC_QUEUES": "1"})
    _clean(rep)
    assert rep["passes"]["ddmc_q"] > 0, rep
    assert rep["evaluated"]["DDMC_CLASS"] == rep["passes"]["ddmc_class"] > 0, rep


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    print(json.dumps(child_case(sys.argv[1])))
