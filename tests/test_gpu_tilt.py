"""The source tilt (include/jaybenne_amd.h: jb_set_source_tilt) on the GPU.  The reference is tests/tilt_model.py, the
slopes and the sampling restated in numpy: slopes are read back through jb_source_tilt_slopes and compared bit for
bit, positions are compared bit for bit by creation id, and every other attribute must be the untilted run's.

Meshes: 1-D, 2 blocks of 8 cells; the two-level 2-D mesh G2S of tests/axis_cases.py; 3-D, 2 x 2 x 2 blocks of 4^3
with a different width and origin on every axis.  States differ in every cell (tests/hetero_states.py: hot_spots on
the stepdiff step, so that slopes vary smoothly, clamp at the step and vanish nowhere).  About 2e4 photons."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import axis_cases as ax
import hetero_states as hs
import tilt_model as tm
from helpers import load_deck
from test_gpu_invariants import _clean, checked_lib  # noqa: F401  (checked_lib: fixture)

pytestmark = pytest.mark.gpu

R_, O_, P_ = ax.R, ax.O, ax.P
NP, SCAT = ax.NP, ax.SCAT
TILT = "jaybenne_amd/source_tilt"
BOX_EXT = ((-0.25, 0.75), (0.5, 2.0), (-1.0, -0.75))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometry(name, kinds):
    if name == "1d":
        return "stepdiff", ax.deck_overrides((16,), (8,), ((-0.25, 0.75),), kinds)
    if name == "2d-smr":
        return "stepdiff_smr", ax.geometry_overrides("G2S", kinds)
    return "stepdiff", ax.deck_overrides((8, 8, 8), (4, 4, 4), BOX_EXT, kinds)


SETS_1D = {"RO": (R_, O_) + (P_,) * 4, "OR": (O_, R_) + (P_,) * 4, "PP": (P_,) * 6}
SLOPE_CASES = ([("1d", k, v) for k, v in SETS_1D.items()] +
               [("2d-smr", k, v[:4] + (P_,) * 2) for k, v in ax.BOUNDARY_SETS.items()] +
               [("3d", k, v) for k, v in ax.BOUNDARY_SETS.items()])


def _driver(deck, ov, pattern, device, **kw):
    from jaybenne_amd import mcblock
    state = hs.state_for(deck, ov, pattern) if pattern else None
    return mcblock.McblockDriver(load_deck(deck, ov), device=device, initial_state=state, **kw)


def _count(md, source_type, dt, epoch=1):
    from jaybenne_amd import _lib
    nper = np.zeros(md.nblocks, dtype=np.int32)
    md._sync_stream()
    _lib.check(md.lib.jb_source_photons_count(md.pkg.ctx, md.handle, int(source_type), dt, md.nowned, epoch,
                                              nper.ctypes.data, md.prefix.data_ptr()))
    return nper


def _model_slopes(drv):
    md = drv.md
    sie = md.fields["sie"][:md.nowned].cpu().numpy()
    return tm.slopes(drv.mesh, sie, drv.mcb.eos.cv, blocks=md.gids)


# ---- 1. slopes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,bset,kinds", SLOPE_CASES, ids=[f"{g}-{b}" for g, b, _ in SLOPE_CASES])
def test_slopes_equal_the_model(gpu_device, geom, bset, kinds):
    from jaybenne_amd import _lib, jaybenne as jb
    deck, ov = _geometry(geom, kinds)
    drv = _driver(deck, dict(ov, **{NP: 2000, TILT: "linear"}), "hot_spots", gpu_device)
    md, mesh = drv.md, drv.mesh
    assert md.source_tilt == "linear" and md.lib.jb_get_source_tilt(md.pkg.ctx) == _lib.TILT_LINEAR
    _count(md, jb.SourceType.thermal, drv.dt)
    got, want = md.source_tilt_slopes(), _model_slopes(drv)
    assert got.shape == want.shape == (mesh.nblocks, 3, mesh.nx[2], mesh.nx[1], mesh.nx[0])
    bad = np.nonzero(got.view(np.int64) != want.view(np.int64))
    assert bad[0].size == 0, (bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5])
    # the state exercises the definition: clamped cells at the step, smooth ones elsewhere, nothing on inactive axes
    act = got[:, :mesh.ndim]
    assert (np.abs(act) == 1.0).any() and ((np.abs(act) > 0.0) & (np.abs(act) < 1.0)).mean() > 0.5
    assert not got[:, mesh.ndim:].any()
    if (geom, bset) in (("3d", "S1"), ("2d-smr", "S3"), ("1d", "RO")):
        # the ghost cells behind a reflecting or outflow domain face are not read
        host = md.fields["sie"].cpu().numpy()
        md.set_field("sie", tm.nan_behind_walls(mesh, host, blocks=md.resident_gids), local=True)
        assert np.isnan(md.fields["sie"].cpu().numpy()).any()
        _count(md, jb.SourceType.thermal, drv.dt)
        assert np.array_equal(md.source_tilt_slopes().view(np.int64), want.view(np.int64))


def test_slopes_need_a_tilted_count(gpu_device):
    from jaybenne_amd import _lib, jaybenne as jb
    deck, ov = _geometry("1d", SETS_1D["RO"])
    drv = _driver(deck, dict(ov, **{NP: 2000}), "hot_spots", gpu_device)
    md = drv.md
    out = np.zeros(3 * drv.mesh.ncell)
    assert md.source_tilt == "none"
    assert md.lib.jb_source_tilt_slopes(md.pkg.ctx, md.handle, 0, out.ctypes.data) == _lib.JB_ERR_INVALID
    assert md.lib.jb_set_source_tilt(md.pkg.ctx, 2) == _lib.JB_ERR_INVALID and md.source_tilt == "none"
    jb.SetSourceTilt(md, "linear")
    nper = _count(md, jb.SourceType.thermal, drv.dt)
    assert md.lib.jb_source_tilt_slopes(md.pkg.ctx, md.handle, 0, out.ctypes.data) == 0
    assert md.lib.jb_source_tilt_slopes(md.pkg.ctx, md.handle, md.nblocks, out.ctypes.data) == _lib.JB_ERR_INVALID
    jb.SetSourceTilt(md, "none")                 # a count in the other mode: the slopes are no longer the last call's
    _count(md, jb.SourceType.thermal, drv.dt)
    assert md.lib.jb_source_tilt_slopes(md.pkg.ctx, md.handle, 0, out.ctypes.data) == _lib.JB_ERR_INVALID
    jb.SetSourceTilt(md, "linear")               # ... and a fill in the mode without its count is refused
    slot = np.zeros(md.nblocks, dtype=np.int64)
    ids = np.zeros(md.nblocks, dtype=np.uint64)
    md.reserve(int(nper.sum()))
    st = md.lib.jb_source_photons_fill(md.pkg.ctx, md.handle, C.byref(md.sv), int(jb.SourceType.thermal), 0.0, drv.dt,
                                       nper.ctypes.data, md.prefix.data_ptr(), slot.ctypes.data, ids.ctypes.data)
    assert st == _lib.JB_ERR_INVALID and b"tilt" in md.lib.jb_last_error()


# ---- 2. photons ------------------------------------------------------------------------------------
HOT3D = dict(ax.deck_overrides((8, 8, 8), (4, 4, 4), BOX_EXT, ax.BOUNDARY_SETS["S1"]), **hs.ABSORBING,
             **{NP: 20000, SCAT: 20.0})


def _source(drv, source_type, mode):
    """SourcePhotons into an empty swarm, ids from 0, under the tilt ``mode``."""
    jb, md = drv.jb, drv.md
    md.sv.n, md.next_id, md.cycle = 0, 0, 1
    md.source_tilt = mode
    jb.SourcePhotons(md, source_type, 0.125, drv.dt)
    return md.get_swarm()


def _check_tilted_against(drv, lin, none, seed):
    """Everything but x, y, z equal to the untilted photons; x, y, z the model's by id; every position in its cell."""
    md, mesh = drv.md, drv.mesh
    assert len(lin["id"]) == len(none["id"]) > 0
    for k in none:
        if k not in ("x", "y", "z"):
            assert np.array_equal(lin[k], none[k]), k
    blk = lin["blk"].astype(np.int64)
    want = tm.photon_positions(mesh, seed, _model_slopes(drv), lin["id"], md.gids[blk], blk, lin["kp"], lin["jp"], lin["ip"])
    moved = 0
    for d, k in enumerate(("x", "y", "z")):
        bad = np.nonzero(lin[k].view(np.int64) != want[d].view(np.int64))[0]
        assert bad.size == 0, (k, bad[:5], lin[k][bad[:5]], want[d][bad[:5]])
        idx = lin[("ip", "jp", "kp")[d]].astype(np.int64)
        dx = mesh.blk_dx[md.gids[blk], d]
        xc = (mesh.blk_xmin[md.gids[blk], d] - mesh.is_[d] * dx) + (idx + 0.5) * dx
        assert np.all(lin[k] >= xc - 0.5 * dx) and np.all(lin[k] < xc + 0.5 * dx), k
        if d < mesh.ndim:
            moved += int((lin[k] != none[k]).sum())
        else:
            assert np.array_equal(lin[k], none[k]), k       # inactive axis: slope 0, the untilted bits
    assert moved > 0.5 * mesh.ndim * len(lin["id"])


@pytest.mark.parametrize("source", ["thermal", "emission"])
def test_tilt_moves_positions_and_nothing_else(gpu_device, source):
    # (a source call of a MeshData of 8 blocks makes num_particles / 8 photons: sourcing.cpp:68-69)
    drv = _driver("stepdiff", dict(HOT3D, **{NP: 160000}), "hot_spots", gpu_device, capacity_factor=1.2)
    jb = drv.jb
    jb.UpdateDerivedTransportFields(drv.md, drv.dt)
    st = jb.SourceType[source]
    none = _source(drv, st, "none")
    lin = _source(drv, st, "linear")
    assert abs(len(lin["id"]) - 20000) < 2000
    _check_tilted_against(drv, lin, none, drv.pin.GetOrAddInteger("jaybenne", "seed", 123))
    assert np.array_equal(_source(drv, st, "none")["x"], none["x"])       # and back


SLAB_HOT = dict(ax.deck_overrides((16,), (8,), ((-0.25, 0.75),), SETS_1D["RO"]), **hs.ABSORBING, **{NP: 4000, SCAT: 150.0})


def test_the_library_step_calls_pick_the_mode_up(gpu_device, monkeypatch):
    """One cycle of the 1-D case under linear: the Python task loop, jb_radiation_step_ranks (JB_HANDOFF=step) and
    jb_radiation_step give the same photons by id, and not the untilted ones."""
    from jaybenne_amd import _lib
    from test_gpu_bsource import _by_id_equal
    ov = dict(SLAB_HOT, **{TILT: "linear"})
    py = _driver("stepdiff", ov, "hot_spots", gpu_device, capacity_factor=3.0)
    assert py.Step() == py.jb.TaskStatus.complete
    want = py.md.get_swarm()
    monkeypatch.setenv("JB_HANDOFF", "step")
    st = _driver("stepdiff", ov, "hot_spots", gpu_device, capacity_factor=3.0)
    assert st.md.handoff == "step" and st.Step() == st.jb.TaskStatus.complete
    assert st.md.handoff_path().startswith("c: jb_radiation_step_ranks")
    _by_id_equal(st.md.get_swarm(), want)
    monkeypatch.delenv("JB_HANDOFF")
    cc = _driver("stepdiff", ov, "hot_spots", gpu_device, capacity_factor=3.0)
    md = cc.md
    next_id, cycle = C.c_uint64(md.next_id), C.c_uint32(0)
    md.reserve(md.n + 8000)
    md._sync_stream()
    _lib.check(md.lib.jb_radiation_step(md.pkg.ctx, md.handle, C.byref(md.sv), 0.0, cc.dt, C.byref(next_id),
                                        C.byref(cycle), md.prefix.data_ptr()))
    _by_id_equal(md.get_swarm(), want)
    plain = _driver("stepdiff", SLAB_HOT, "hot_spots", gpu_device, capacity_factor=3.0)
    assert plain.md.source_tilt == "none" and plain.Step() == plain.jb.TaskStatus.complete
    g = plain.md.get_swarm()
    assert len(g["id"]) != len(want["id"]) or not np.array_equal(np.sort(g["x"]), np.sort(want["x"]))


def test_environment_sets_the_initial_mode(gpu_device, monkeypatch):
    monkeypatch.setenv("JB_SOURCE_TILT", "linear")
    deck, ov = _geometry("1d", SETS_1D["RO"])
    drv = _driver(deck, dict(ov, **{NP: 2000}), None, gpu_device)
    assert drv.md.source_tilt == "linear"
    drv = _driver(deck, dict(ov, **{NP: 2000, TILT: "none"}), None, gpu_device)
    assert drv.md.source_tilt == "none"


def test_checked_library_accepts_tilted_photons(gpu_device, checked_lib):
    """One cycle of the 1-D case under linear with the checked library: its SWARM sweep behind the fill (positions
    inside the cells the indices name) and every other invariant hold."""
    env = dict(os.environ, JAYBENNE_AMD_LIB=checked_lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "checked-1d"], capture_output=True, text=True,
                         env=env, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    _clean(out["report"])
    assert out["tilt"] == "linear" and out["clamped"] > 0 and out["n"] > 1000


# ---- 3. uniform temperature ------------------------------------------------------------------------
def test_uniform_temperature_gives_the_untilted_cycle(gpu_device):
    """The inf deck (one temperature, periodic, emission on): every slope is zero and the whole swarm after one full
    cycle -- initial thermal photons, emission photons, transport -- has the bits of the untilted run."""
    ov = {NP: 4000, "parthenon/meshblock/nx1": 2, "parthenon/meshblock/nx2": 2, "parthenon/meshblock/nx3": 2}
    out = {}
    for mode in ("none", "linear"):
        drv = _driver("inf", dict(ov, **{TILT: mode}), None, gpu_device, capacity_factor=4.0)
        assert drv.md.source_tilt == mode and drv.mesh.nblocks == 8
        assert drv.Step() == drv.jb.TaskStatus.complete
        out[mode] = drv.md.get_swarm()
        if mode == "linear":
            s = drv.md.source_tilt_slopes()
            assert s.shape[0] == 8 and not s.any()
    from test_gpu_bsource import _by_id_equal
    assert len(out["none"]["id"]) > 4000
    _by_id_equal(out["linear"], out["none"])        # (by id: the compaction behind the transport orders the slots)


# ---- 4. two ranks ----------------------------------------------------------------------------------
def _sourced(drv, nowned=None):
    """The photons of the initial thermal source (made by the driver) and of one emission source behind them, not
    transported; block indices global.  ``nowned``: the block count the emission source scales its photons per cell
    with (sourcing.cpp:68-69: the blocks of the calling rank's MeshData)."""
    jb, md = drv.jb, drv.md
    md.cycle = 1
    jb.UpdateDerivedTransportFields(md, drv.dt)
    keep = md.nowned
    md.nowned = keep if nowned is None else nowned
    try:
        jb.SourcePhotons(md, jb.SourceType.emission, 0.0, drv.dt)
    finally:
        md.nowned = keep
    g = md.get_swarm()
    g["blk"] = md.resident_gids[g["blk"]]
    return g


def _rank_worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_EXACT_ARITH="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd.comm import Comm
        for decomposition in ("blocks", "replicated"):
            drv = _driver("stepdiff", dict(HOT3D, **{TILT: "linear"}), "hot_spots", torch.device("cuda", 0), rank=rank,
                          nranks=world, comm=Comm(), capacity_factor=3.0, decomposition=decomposition)
            assert drv.md.source_tilt == "linear" and drv.md.replicated == (decomposition == "replicated")
            g = _sourced(drv)
            np.savez(os.path.join(outdir, f"{decomposition}{rank}.npz"), nowned=np.array([drv.md.nowned]),
                     next_id=np.array([drv.md.next_id]), **g)
            drv.md.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_source_the_photons_of_one(gpu_device, tmp_path):
    import torch.multiprocessing as mp
    from test_gpu_bsource import _by_id_equal
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)])
    for decomposition in ("blocks", "replicated"):
        parts = [np.load(tmp_path / f"{decomposition}{r}.npz") for r in range(2)]
        nowned = [int(p["nowned"][0]) for p in parts]
        assert nowned == ([4, 4] if decomposition == "blocks" else [8, 8])
        one = _driver("stepdiff", dict(HOT3D, **{TILT: "linear"}), "hot_spots", gpu_device, capacity_factor=3.0)
        want = _sourced(one, nowned[0])
        assert all(len(p["id"]) > 5000 for p in parts)
        _by_id_equal({k: np.concatenate([p[k] for p in parts]) for k in want}, want)
        assert all(int(p["next_id"][0]) == one.md.next_id for p in parts)
    # ... and those are tilted photons
    plain = _sourced(_driver("stepdiff", HOT3D, "hot_spots", gpu_device, capacity_factor=3.0), 8)
    assert np.array_equal(np.sort(plain["id"]), np.sort(want["id"])) and not np.array_equal(np.sort(plain["x"]), np.sort(want["x"]))


# ---- 5. the physics --------------------------------------------------------------------------------
SLAB_CELLS, SLAB_FINE, SLAB_K, SLAB_DT, SLAB_NP, SLAB_KAPPA, SLAB_COLD = 16, 8, 60, 1.0e-12, 20000, 64.0, 0.01
SLAB_SEEDS = (11, 12, 13, 14)


def hot_slab(mesh, pkg, gids=None):
    """The left quarter of the domain at the deck's temperature, the rest at SLAB_COLD of it; ghost cells mirrored
    at the walls."""
    from jaybenne_amd import mcblock
    ic = mcblock.ProblemGenerator(mesh, pkg, gids)
    lo, hi = mesh.gmin[0], mesh.gmax[0]
    for n, b in enumerate(np.arange(mesh.nblocks) if gids is None else np.asarray(gids)):
        x = mesh.cell_centers(int(b), 0)
        x = np.where(x < lo, 2 * lo - x, np.where(x > hi, 2 * hi - x, x))
        ic["sie"][n][:, :, x >= lo + 0.25 * (hi - lo)] *= SLAB_COLD
    ic["u"] = ic["rho"] * ic["sie"]
    return ic


def _slab_profile(device, cells, seed, tilt):
    """Material energy density per cell after SLAB_K cycles of the slab on ``cells`` cells."""
    from jaybenne_amd import mcblock
    ov = {"parthenon/job/problem_id": "slab", "parthenon/mesh/nx1": cells, "parthenon/meshblock/nx1": cells,
          NP: SLAB_NP, "jaybenne/dt": SLAB_DT, "jaybenne/seed": seed, "jaybenne/do_emission": "true",
          "jaybenne/do_feedback": "true", "jaybenne/use_ddmc": "false", "mcblock/opacity_model": "constant",
          "mcblock/opacity_constant_value": SLAB_KAPPA, "mcblock/scattering_model": "none", TILT: tilt}
    drv = mcblock.McblockDriver(load_deck("stepdiff", ov), device=device, capacity_factor=8.0, initial_state=hot_slab)
    assert drv.md.source_tilt == tilt and drv.dt == SLAB_DT
    assert 3.0 <= SLAB_KAPPA * drv.mesh.blk_dx[0, 0] * (cells // SLAB_CELLS) <= 5.0
    for _ in range(SLAB_K):
        assert drv.Step() == drv.jb.TaskStatus.complete
    u = drv.md.get_field("u")[drv.mesh.interior()][0, 0, 0].copy()
    drv.md.close()
    return u


def test_tilt_brings_a_coarse_slab_closer_to_the_fine_one(gpu_device):
    """A hot slab in 1-D: reflecting walls, no DDMC, absorption opacity 64 (4 mean free paths per coarse cell), emission
    and feedback on, the left quarter at 1e5, the rest at 1e3; 16 cells, dt = 1e-12 (c dt = 0.48 cells), 60 cycles,
    2e4 photons per cycle.  The yardstick is the same deck, untilted, on 128 cells, averaged onto the coarse cells
    and over its four seeds.  err = sum |u - u_fine| / sum u_fine; the assertion is the ordering with three
    seed-to-seed deviations on either side.  Measured: untilted 0.0722 +- 0.0041, linear 0.0242 +- 0.0036."""
    runs = {"none": [], "linear": [], "fine": []}
    for seed in SLAB_SEEDS:
        runs["none"].append(_slab_profile(gpu_device, SLAB_CELLS, seed, "none"))
        runs["linear"].append(_slab_profile(gpu_device, SLAB_CELLS, seed, "linear"))
        fine = _slab_profile(gpu_device, SLAB_CELLS * SLAB_FINE, seed + 100, "none")
        runs["fine"].append(fine.reshape(SLAB_CELLS, SLAB_FINE).mean(axis=1))
    yard = np.mean(runs["fine"], axis=0)
    err = {k: np.array([np.abs(u - yard).sum() / yard.sum() for u in runs[k]]) for k in runs}
    mean = {k: float(v.mean()) for k, v in err.items()}
    sd = {k: float(v.std(ddof=1)) for k, v in err.items()}
    print("slab errors", {k: (mean[k], sd[k], v.tolist()) for k, v in err.items()})
    assert mean["none"] >= 5.0 * sd["none"], (mean, sd)          # the untilted error is no noise
    assert mean["linear"] + 3.0 * sd["linear"] < mean["none"] - 3.0 * sd["none"], (mean, sd)


# ---- in the child process ------------------------------------------------------------------------------
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ["JB_EXACT_ARITH"] = "1"
    import torch
    assert sys.argv[1] == "checked-1d"
    drv = _driver("stepdiff", dict(SLAB_HOT, **{TILT: "linear"}), "hot_spots", torch.device("cuda", 0), capacity_factor=3.0)
    assert drv.md.invariants_enabled()
    assert drv.Step() == drv.jb.TaskStatus.complete
    print(json.dumps({"report": drv.md.invariant_report(), "tilt": drv.md.source_tilt, "n": drv.md.n,
                      "clamped": int((np.abs(drv.md.source_tilt_slopes()) == 1.0).sum())}))
