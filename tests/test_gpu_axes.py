"""Every tracking kernel on meshes whose per-axis numbers all differ and whose six faces carry different boundary
kinds (tests/axis_cases.py), against the CPU oracle started from the same arrays.  On the decks of
tests/test_gpu_parity.py and tests/test_gpu_hetero.py dy == dz, nj == nk, nleaf[1] == nleaf[2], gmin == -gmax and x2 /
x3 are periodic, so a kernel that exchanges the second and third axes, the two faces of an axis or the sign of an
origin computes the same bits there; here at least 100 histories touch every face (tests/test_axis_host.py) and the
comparisons are the project's own: bit-equality in exact arithmetic, 1e-12 on fields, 1e-9 / 1e-8 for lean after
one / two cycles.  Photons escape in every case, so swarms are compared by creation id."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import axis_cases as ax
import hetero_states as hs
from helpers import load_deck, run_oracle_cycles
from test_gpu_hetero import _compare_lean, _compare_start, _pair, _steps, _variant
from test_gpu_invariants import CHECKED, ROOT, TESTS, _clean, checked_lib  # noqa: F401  (checked_lib: fixture)
from test_gpu_parity import _compare_fields, _compare_swarm_by_id

pytestmark = pytest.mark.gpu


def _case_pair(case, bset, device, pattern=None, capacity_factor=1.3):
    ov = ax.overrides(case, bset)
    return _pair(case.deck, ov, pattern or case.pattern, device, capacity_factor=capacity_factor)


def _compare_end(drv, O, names=("tally", "edelta", "fleck", "src_num", "src_ew")):
    """test_gpu_hetero._compare_end for swarms that compaction has reordered, and: photons did escape."""
    assert drv.md.stats()["n_escaped"] > 0
    _compare_swarm_by_id(drv.md, O)
    _compare_fields(drv.md, O, names)
    assert drv.md.events == O.events


def _ids(pairs):
    return [f"{c}-{s}" for c, s in pairs]


def _uniform(mesh):
    """The library's condition for k_imc_cell<.., UNIFORM> (jb_mesh_create): every block has block 0's widths."""
    return bool(np.all(mesh.blk_dx == mesh.blk_dx[0]))


# ---- a. pure IMC, exact arithmetic on exact geometry -------------------------------------------
EXACT_IMC = [(c, s) for c in ("G1-imc", "G2S-imc", "G3U-imc", "G3S-imc") for s in ax.boundary_sets(ax.BY_ID[c].geom)]


@pytest.mark.parametrize("cid,bset", EXACT_IMC, ids=_ids(EXACT_IMC))
def test_imc_exact(gpu_device, cid, bset):
    case = ax.BY_ID[cid]
    pin, drv, O, mesh, _ = _case_pair(case, bset, gpu_device)
    assert drv.md.lib.jb_mesh_exact_geometry(drv.md.handle) == 1
    _compare_start(drv, O, False)
    _steps(drv, O, pin, case.cycles)
    v = _variant(drv)
    assert f"k_transport<{mesh.ndim}," in v and v.endswith("true, false>"), v      # EXACT geometry, not LEAN
    assert 10 * O.n < O.events
    _compare_end(drv, O)


# ---- b. pure IMC, lean, in cell-local coordinates ----------------------------------------------
@pytest.mark.lean
@pytest.mark.parametrize("cid,bset", EXACT_IMC, ids=_ids(EXACT_IMC))
def test_imc_lean_cell_local(gpu_device, cid, bset):
    case = ax.BY_ID[cid]
    pin, drv, O, mesh, _ = _case_pair(case, bset, gpu_device)
    assert drv.pkg.arithmetic() == "lean"
    _steps(drv, O, pin, case.cycles)
    v = _variant(drv)
    assert f"k_imc_cell<{mesh.ndim}, true, true, lean>" == v, v                  # TALLY, NOABS
    assert _uniform(mesh) == (ax.GEOMETRIES[case.geom].refine is None)             # UNIFORM on one level only
    assert drv.md.stats()["n_escaped"] > 0
    _compare_lean(drv, O, mesh, pin, case.cycles, by_id=True)


@pytest.mark.lean
def test_imc_lean_cell_local_with_absorption(gpu_device):
    case = ax.HOT_CASE
    pin, drv, O, mesh, _ = _case_pair(case, "S1", gpu_device, capacity_factor=8.0)
    _steps(drv, O, pin, 1)
    v = _variant(drv)
    assert v == "k_imc_cell<3, true, false, lean>", v                              # !NOABS
    assert drv.md.stats()["n_absorbed"] > 500 and drv.md.stats()["n_escaped"] > 0
    _compare_lean(drv, O, mesh, pin, 1, by_id=True)


# ---- c. pure IMC, lean, in the swarm's coordinates ---------------------------------------------
@pytest.mark.lean
def test_imc_lean_x_space(gpu_device, monkeypatch):
    case = ax.BY_ID["G3S-imc"]
    monkeypatch.setenv("JB_NO_IMC_CELL", "1")
    pin, drv, O, mesh, _ = _case_pair(case, "S3", gpu_device)
    _steps(drv, O, pin, 1)
    v = _variant(drv)
    assert "k_transport<3," in v and v.endswith("true, true>"), v                  # EXACT geometry, LEAN
    assert drv.md.stats()["n_escaped"] > 0
    _compare_lean(drv, O, mesh, pin, 1, by_id=True)


# ---- d. general geometry -----------------------------------------------------------------------
GENERAL = [(c, s) for c in ("G3O-imc", "G3X-imc") for s in ("S1", "S2", "S3")]


@pytest.mark.parametrize("cid,bset", GENERAL, ids=_ids(GENERAL))
def test_imc_exact_arithmetic_on_general_geometry(gpu_device, cid, bset):
    """G3O: widths that are no powers of two; G3X: powers of two from an origin that is no whole number of them --
    jb_mesh_create's x0 / dx test must turn exact geometry off."""
    case = ax.BY_ID[cid]
    pin, drv, O, mesh, _ = _case_pair(case, bset, gpu_device)
    assert drv.md.lib.jb_mesh_exact_geometry(drv.md.handle) == 0
    _compare_start(drv, O, False)
    _steps(drv, O, pin, case.cycles)
    v = _variant(drv)
    assert "k_transport<3," in v and v.endswith("false, false>"), v               # not EXACT, not LEAN
    _compare_end(drv, O)


LEAN_GENERAL = [("G3O-imc", "S2", None), ("G3X-imc", "S3", None), ("G3O-imc", "S3", "1"), ("G3X-imc", "S1", "1")]


@pytest.mark.lean
@pytest.mark.parametrize("cid,bset,no_cell", LEAN_GENERAL,
                         ids=[f"{c}-{s}" + ("-x-space" if e else "") for c, s, e in LEAN_GENERAL])
def test_imc_lean_on_general_geometry(gpu_device, cid, bset, no_cell, monkeypatch):
    case = ax.BY_ID[cid]
    if no_cell:
        monkeypatch.setenv("JB_NO_IMC_CELL", no_cell)
    pin, drv, O, mesh, _ = _case_pair(case, bset, gpu_device)
    assert drv.md.lib.jb_mesh_exact_geometry(drv.md.handle) == 0
    _steps(drv, O, pin, case.cycles)
    v = _variant(drv)
    if no_cell:
        assert "k_transport<3," in v and v.endswith("false, true>"), v            # not EXACT, LEAN
    else:
        assert v == "k_imc_cell<3, true, true, lean>", v
    _compare_lean(drv, O, mesh, pin, case.cycles, by_id=True)


@pytest.mark.parametrize("arith", ["exact", pytest.param("lean", marks=pytest.mark.lean)])
def test_general_kernels_on_the_exact_mesh(gpu_device, arith, monkeypatch):
    case = ax.BY_ID["G3U-imc"]
    monkeypatch.setenv("JB_NO_EXACT_GEOM", "1")
    monkeypatch.setenv("JB_NO_IMC_CELL", "1")
    pin, drv, O, mesh, _ = _case_pair(case, "S1" if arith == "exact" else "S2", gpu_device)
    assert drv.md.lib.jb_mesh_exact_geometry(drv.md.handle) == 0
    _steps(drv, O, pin, case.cycles)
    v = _variant(drv)
    assert "k_transport<3," in v and v.endswith("false, false>" if arith == "exact" else "false, true>"), v
    if arith == "exact":
        _compare_end(drv, O)
    else:
        _compare_lean(drv, O, mesh, pin, case.cycles, by_id=True)


# ---- e. all-DDMC -------------------------------------------------------------------------------
DDMC_CASES = ("G3S-ddmc", "G2S-ddmc")
SETS = ("S1", "S2", "S3")
# (the forms and the sets rotate against each other: every form meets every set on one of the two meshes or the
# other, and each mesh runs every set)
GATHERS = [(c, f, SETS[(q + 2 * m) % 3]) for m, c in enumerate(DDMC_CASES) for q, f in enumerate(hs.DDMC_GATHERS)] + \
          [("G3S-ddmc", "0", "S3"), ("G3S-ddmc", "1", "S1"), ("G3S-ddmc", "2", "S2")]


@pytest.mark.parametrize("cid,form,bset", GATHERS, ids=[f"{c}-{f}-{s}" for c, f, s in GATHERS])
def test_ddmc_64_byte_gathers(gpu_device, cid, form, bset, monkeypatch):
    case = ax.BY_ID[cid]
    monkeypatch.delenv("JB_COOP_GATHER", raising=False)
    if form in ("0", "1", "2"):
        monkeypatch.setenv("JB_COOP_GATHER", form)
    pin, drv, O, mesh, pkg = _case_pair(case, bset, gpu_device, pattern="smooth_dense")
    nd = mesh.ndim
    _compare_start(drv, O, True)
    ncpu = hs.class_count(mesh, pkg, O)
    assert ncpu > 256
    _steps(drv, O, pin, case.cycles)
    v = _variant(drv)
    assert f"k_ddmc_all<{nd}, true" in v, v
    assert drv.md.lib.jb_mesh_ddmc_classes(drv.md.handle) > 256
    if form == "0":
        assert v.endswith(f"k_ddmc_all<{nd}, true>"), v
    elif form in ("1", "2"):
        assert "quad gather" in v, v
    else:
        assert "cell codes" not in v, v          # more classes than the table holds: a 64-byte form
    _compare_end(drv, O)


CODES = [(c, mode, SETS[(q + m) % 3]) for m, c in enumerate(DDMC_CASES) for q, mode in enumerate(hs.DDMC_CODES)] + \
        [("G3S-ddmc", "queues", "S3"), ("G3S-ddmc", "queues, codes gathered", "S1"), ("G3S-ddmc", "forced", "S2"),
         ("G1-ddmc", "queues", "RO"), ("G1-ddmc", "queues", "OR"), ("G1-ddmc", "queues, codes gathered", "OR"),
         ("G1-ddmc", "forced", "RO")]


@pytest.mark.parametrize("cid,mode,bset", CODES, ids=[f"{c}-{m}-{s}" for c, m, s in CODES])
def test_ddmc_cell_codes(gpu_device, cid, mode, bset, monkeypatch):
    """The switches of test_gpu_hetero.test_ddmc_cell_codes_on_palettes; k_ddmc_q keeps its codes in LDS on the 1-D
    mesh, gathers them on the others."""
    case = ax.BY_ID[cid]
    monkeypatch.delenv("JB_COOP_GATHER", raising=False)
    if mode == "forced":
        monkeypatch.setenv("JB_COOP_GATHER", "4")
    elif mode.startswith("queues"):
        monkeypatch.setenv("JB_DDMC_QUEUES", "1")
        monkeypatch.setenv("JB_DDMC_LDS_CODES", "1" if mode == "queues" else "0")
    else:
        monkeypatch.setenv("JB_DDMC_MAX_CLASSES", "1" if mode == "one class allowed" else "0")
    pin, drv, O, mesh, pkg = _case_pair(case, bset, gpu_device, pattern=ax.DDMC_PALETTE[cid, bset])
    ncpu = None
    if mode == "forced":
        _compare_start(drv, O, True)
        ncpu = hs.class_count(mesh, pkg, O)
        lo, hi = ax.DDMC_CLASS_BRACKET[cid]
        assert lo < ncpu <= hi
    _steps(drv, O, pin, case.cycles)
    v = _variant(drv)
    if mode == "forced":
        assert "cell codes" in v and "queues" not in v, v
        assert drv.md.lib.jb_mesh_ddmc_classes(drv.md.handle) == ncpu
    elif mode.startswith("queues"):
        assert "cell codes, queues" in v, v
        small = drv.md.nblocks * mesh.ntot <= 1024 and ax.DDMC_CLASS_BRACKET[cid][1] <= 64
        assert small == (mesh.ndim == 1)
        assert ("codes in LDS" in v) == (mode == "queues" and small), v
    else:
        assert "k_ddmc_all" in v and "cell codes" not in v, v
    _compare_end(drv, O)


# ---- f. hybrid ---------------------------------------------------------------------------------
HYB = []
for _m, _cid in enumerate(("G3S-hybrid", "G2S-hybrid")):
    for _q, (_p, _a) in enumerate((p, a) for p in ax.HYBRID_PATTERNS for a in ("exact", "lean")):
        HYB.append((_cid, _p, _a, SETS[(_q + _m) % 3]))
HYB += [("G3S-hybrid", "islands", "exact", "S3"), ("G3S-hybrid", "islands", "lean", "S1"),
        ("G3S-hybrid", "islands", "exact", "S2"), ("G3S-hybrid", "islands", "lean", "S3"),
        ("G2O-hybrid", "islands", "exact", "S1"), ("G2O-hybrid", "islands", "exact", "S2"),
        ("G2O-hybrid", "islands", "exact", "S3"), ("G2O-hybrid", "threshold", "lean", "S3"),
        ("G2O-hybrid", "islands", "lean", "S2")]
HYB = [pytest.param(c, p, a, s, marks=[pytest.mark.lean] if a == "lean" else [], id=f"{c}-{p}-{a}-{s}")
       for c, p, a, s in HYB]


@pytest.mark.parametrize("cid,pattern,arith,bset", HYB)
def test_hybrid(gpu_device, cid, pattern, arith, bset):
    case = ax.BY_ID[cid]
    pin, drv, O, mesh, pkg = _case_pair(case, bset, gpu_device, pattern=pattern)
    assert drv.pkg.arithmetic() == arith
    if arith == "exact":
        _compare_start(drv, O, True)
    _steps(drv, O, pin, case.cycles)
    v = _variant(drv)
    exact_geom = ax.GEOMETRIES[case.geom].exact
    assert drv.md.lib.jb_mesh_exact_geometry(drv.md.handle) == int(exact_geom)
    want = "exact>" if arith == "exact" else ("lean, cell-local>" if exact_geom else "lean>")
    assert v == f"k_hybrid<{mesh.ndim}, {want}", v
    if arith == "exact":
        _compare_end(drv, O)
    else:
        assert drv.md.stats()["n_escaped"] > 0
        _compare_lean(drv, O, mesh, pin, case.cycles, by_id=True)


def test_general_kernel_on_the_all_ddmc_mesh(gpu_device, monkeypatch):
    case = ax.BY_ID["G3S-ddmc"]
    monkeypatch.setenv("JB_NO_DDMC_ALL", "1")
    pin, drv, O, mesh, _ = _case_pair(case, "S2", gpu_device, pattern="smooth_dense")
    _steps(drv, O, pin, case.cycles)
    assert "k_hybrid<3" in _variant(drv), _variant(drv)
    _compare_end(drv, O)


# ---- g. derived fields before the first step ---------------------------------------------------
@pytest.mark.parametrize("bset", SETS)
@pytest.mark.parametrize("cid,pattern", [("G3S-hybrid", "islands"), ("G3S-ddmc", "smooth_dense")])
def test_derived_fields_before_the_first_step(gpu_device, cid, pattern, bset):
    """fleck, src_num, src_ew and P1 .. P3 (k_face_prob, k_ddmc_pack: per-axis code) with walls, open faces and
    level boundaries on every axis in turn."""
    pin, drv, O, mesh, _ = _case_pair(ax.BY_ID[cid], bset, gpu_device, pattern=pattern)
    _compare_start(drv, O, True)


# ---- h. PhotonReflectBC as a task of its own ---------------------------------------------------
def test_photon_reflect_bc_task_on_every_face(gpu_device):
    """Photons pushed beyond all six faces of G3U under S1 (ix1 and ox2 reflect).  First as a host schedules the
    task -- on the reflecting faces only: what lies beyond the other four faces stays untouched; then on every
    face, one at a time: each call mirrors exactly the photons beyond its face about gmin[d] / gmax[d] (no origin
    is minus the other bound here), flips that velocity component and changes nothing else, as the oracle."""
    import torch
    from jaybenne_amd import jaybenne as jb
    from jaybenne_amd.mesh import BC_REFLECT
    case = ax.BY_ID["G3U-imc"]
    pin, drv, O, mesh, _ = _case_pair(case, "S1", gpu_device)
    n = drv.md.n
    rng = np.random.default_rng(3)
    ext = mesh.gmax - mesh.gmin
    keys = ("x", "y", "z", "vx", "vy", "vz", "ip", "jp", "kp")
    for q, k in enumerate(("x", "y", "z")):
        new = O.sw[k][:n] + rng.uniform(-0.7, 0.7, size=n) * ext[q]      # a good fraction beyond every face
        O.sw[k][:n] = new
        drv.md.swarm[k][:n] = torch.from_numpy(new).to(gpu_device)
    start = {k: O.sw[k][:n].copy() for k in keys}
    reflecting = [f for f in range(6) if mesh.swarm_bc[f] == BC_REFLECT]
    assert reflecting == [0, 3]
    for face in reflecting:
        jb.PhotonReflectBC(drv.md, face)
        O.PhotonReflectBC(face)
    g = drv.md.get_swarm()
    for k in keys:
        assert np.array_equal(g[k], O.sw[k][:n]), k
    beyond = {0: start["x"] < mesh.gmin[0], 1: start["x"] > mesh.gmax[0], 2: start["y"] < mesh.gmin[1],
              3: start["y"] > mesh.gmax[1], 4: start["z"] < mesh.gmin[2], 5: start["z"] > mesh.gmax[2]}
    assert all(int(b.sum()) > 100 for b in beyond.values())
    touched = beyond[0] | beyond[3]
    for k in keys:
        assert np.array_equal(g[k][~touched], start[k][~touched]), k
    assert np.array_equal(g["x"][beyond[1]], start["x"][beyond[1]])               # still beyond the open faces
    assert np.array_equal(g["y"][beyond[2]], start["y"][beyond[2]])
    assert np.array_equal(g["z"], start["z"]) and np.array_equal(g["vz"], start["vz"])
    # every face in turn, from the pushed state again
    for k in keys:
        O.sw[k][:n] = start[k]
        drv.md.swarm[k][:n] = torch.from_numpy(start[k]).to(gpu_device)
    for face in range(6):
        before = drv.md.get_swarm()
        jb.PhotonReflectBC(drv.md, face)
        O.PhotonReflectBC(face)
        g = drv.md.get_swarm()
        for k in keys:
            assert np.array_equal(g[k], O.sw[k][:n]), (face, k)
        d, outer = face >> 1, face & 1
        pos, vel = "xyz"[d], "v" + "xyz"[d]
        wall = mesh.gmax[d] if outer else mesh.gmin[d]
        hit = before[pos] > wall if outer else before[pos] < wall
        assert int(hit.sum()) > 100
        assert np.array_equal(g[pos][hit], wall + (wall - before[pos][hit]) if not outer
                              else wall - (before[pos][hit] - wall)), face
        assert np.array_equal(g[vel][hit], -before[vel][hit]), face
        for k in keys:
            if k in (pos, vel):
                assert np.array_equal(g[k][~hit], before[k][~hit]), (face, k)
            elif k not in ("ip", "jp", "kp"):
                assert np.array_equal(g[k], before[k]), (face, k)
            else:
                assert np.array_equal(g[k][~hit], before[k][~hit]), (face, k)


# ---- i. DefragParticles ------------------------------------------------------------------------
def test_defrag_particles_with_unequal_block_sides(gpu_device):
    """The sort key is built from (blk, k, j, i) with nj != nk: after a cycle on the G3S hybrid case the particle
    set is the oracle's and the swarm is ordered by (block, cell)."""
    case = ax.BY_ID["G3S-hybrid"]
    pin, drv, O, mesh, _ = _case_pair(case, "S2", gpu_device)
    drv.md.defrag_interval = 1
    _steps(drv, O, pin, 2)
    assert drv.md.defrags == 2
    _compare_end(drv, O)
    g = drv.md.get_swarm()
    m = drv.mesh
    assert m.ntot_dim[1] != m.ntot_dim[2] and m.ntot_dim[0] != m.ntot_dim[1]
    b = g["blk"].astype(np.int64)
    cell = np.zeros(len(b), dtype=np.int64)
    stride = 1
    for d, name in enumerate("xyz"):
        idx = np.floor((g[name] - m.blk_xmin[b, d]) * (1.0 / m.blk_dx[b, d])).astype(np.int64) + m.is_[d]
        cell += stride * idx
        stride *= m.field_shape[3 - d]
    key = b * int(np.prod(m.field_shape[1:])) + cell
    assert np.all(np.diff(key) >= 0)
    assert len(np.unique(key)) > 1000


# ---- j. several ranks --------------------------------------------------------------------------
RANKS = [("G3S-hybrid", "S1", 2, "blocks", "step"), ("G3S-ddmc", "S3", 4, "blocks", "step"),
         ("G3S-hybrid", "S2", 2, "replicated", "c")]


def _rank_worker(rank, world, port, cid, bset, outdir, decomposition, handoff):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_HANDOFF=handoff)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import mcblock
        from jaybenne_amd.comm import Comm
        case = ax.BY_ID[cid]
        ov = ax.overrides(case, bset)
        pattern = ax.DDMC_PALETTE.get((cid, bset), case.pattern)
        drv = mcblock.McblockDriver(load_deck(case.deck, ov), rank=rank, nranks=world, comm=Comm(),
                                    device=torch.device("cuda", 0), capacity_factor=2.0,
                                    decomposition=decomposition, initial_state=hs.state_for(case.deck, ov, pattern))
        assert drv.decomposition == decomposition
        for _ in range(case.cycles):
            drv.Step()
        if decomposition == "blocks":
            assert drv.md.handoff_path().startswith("c: jb_radiation_step_ranks"), drv.md.handoff_path()
        g = drv.md.get_swarm()
        g["gblk"] = drv.md.gids[g["blk"]]
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), tally=drv.md.get_field("tally"), gids=drv.md.gids,
                 resident=drv.md.resident_gids, rho=drv.md.fields["rho"].cpu().numpy(),
                 events=np.array([drv.md.events]), **g)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("cid,bset,world,decomposition,handoff", RANKS,
                         ids=[f"{c}-{s}-{w}-{d}" for c, s, w, d, _ in RANKS])
def test_ranks(gpu_device, cid, bset, world, decomposition, handoff, tmp_path):
    """The union of the ranks' swarms is the oracle's: hand-overs across block faces of unequal sides, walls and
    open faces on ranks of their own."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, TESTS)
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, cid, bset, str(tmp_path), decomposition, handoff))
             for r in range(world)]
    _run_workers(procs)
    case = ax.BY_ID[cid]
    ov = ax.overrides(case, bset)
    pin = load_deck(case.deck, ov)
    O, mesh, _ = hs.oracle_on(case.deck, ov, ax.DDMC_PALETTE.get((cid, bset), case.pattern))
    rho0 = O.fields["rho"].copy()
    n0 = O.n
    run_oracle_cycles(O, pin, case.cycles)
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    ids = np.concatenate([p["id"] for p in parts])
    order = np.argsort(ids)
    oo = np.argsort(O.sw["id"][:O.n])
    assert len(ids) == O.n and np.array_equal(ids[order], O.sw["id"][:O.n][oo])
    for k in ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e", "ip", "jp", "kp", "rng"):
        assert np.array_equal(np.concatenate([p[k] for p in parts])[order], O.sw[k][:O.n][oo]), k
    assert np.array_equal(np.concatenate([p["gblk"] for p in parts])[order], O.sw["blk"][:O.n][oo])
    assert O.n < n0                  # photons left through the open faces
    sl = mesh.interior()
    for p in parts:
        if decomposition == "blocks":
            assert len(p["resident"]) > len(p["gids"])
        assert np.array_equal(p["rho"], rho0[p["resident"]])
        np.testing.assert_allclose(p["tally"][sl], O.fields["tally"][p["gids"]][sl], rtol=1e-12, atol=0)
    assert sum(int(p["events"][0]) for p in parts) == O.events


# ---- k. under the checked library --------------------------------------------------------------
def child_case(kind):
    import torch
    dev = torch.device("cuda", 0)
    cid, bset = {"hybrid": ("G3S-hybrid", "S3"), "imc3d": ("G3U-imc", "S2")}[kind]
    case = ax.BY_ID[cid]
    pin, drv, O, mesh, _ = _case_pair(case, bset, dev)
    _steps(drv, O, pin, case.cycles)
    _compare_end(drv, O)
    assert drv.md.invariants_enabled()
    rep = drv.md.invariant_report()
    rep["variant"] = _variant(drv)
    return rep


def _child(kind):
    e = dict(os.environ, JAYBENNE_AMD_LIB=CHECKED)
    e.pop("JB_COOP_GATHER", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), kind], capture_output=True, text=True, env=e,
                         timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.timeout(900, method="thread")
@pytest.mark.parametrize("kind,family", [("hybrid", "hybrid"), ("imc3d", "transport")])
def test_checked_library(gpu_device, checked_lib, kind, family):
    rep = _child(kind)
    _clean(rep)
    assert rep["passes"][family] > 0, rep
    assert rep["evaluated"]["INDEX"] >= rep["passes"][family], rep


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    print(json.dumps(child_case(sys.argv[1])))
