"""The boundary source (include/jaybenne_amd.h: jb_source_boundary_count / _fill) on the GPU.  The reference is
tests/bsource_model.py -- the semantics restated in numpy from the CPU oracle's primitives -- and, behind the source,
the CPU oracle itself, which transports the model's photons like any other: photons are compared by creation id.

Meshes: 1-D, 8 cells in one block; the two-level 2-D mesh G2S of tests/axis_cases.py (the ix2 face carries cells of two
areas); the 3-D mesh G3U (2 x 3 x 4 blocks, every per-axis number different), every non-periodic face outflow.  About
2 000 boundary photons per cycle."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import axis_cases as ax
import bsource_model as bm
import hetero_states as hs
from helpers import load_deck
from test_gpu_invariants import _clean, checked_lib  # noqa: F401  (checked_lib: fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_B = 2000
O_, P_ = ax.O, ax.P
BOX = ax.geometry_overrides("G3U", (O_,) * 6)
SMR2 = ax.geometry_overrides("G2S", (O_,) * 4 + (P_,) * 2)
SLAB = {"parthenon/mesh/nx1": 8, "parthenon/meshblock/nx1": 8, "parthenon/swarm/ix1_bc": O_, "parthenon/swarm/ox1_bc": O_}
NP, SCAT, TAU = ax.NP, ax.SCAT, ax.TAU

# id: (deck, overrides, pattern, {face: temperature}, capacity factor)
CASES = {
    # (the all-DDMC cases: a scattering opacity at which every cell is a DDMC cell -- dx_push sigma > tau_ddmc = 5 --
    # and the albedo still admits a fair share of the photons)
    "imc-3d": ("stepdiff", dict(BOX, **{NP: 3000, SCAT: 20.0}), "smooth", {0: 1.0e5, 5: 1.2e5}, 4.0),
    # with absorption and emission: per block the emission ids first, then the boundary ids
    "imc-3d-hot": ("stepdiff", dict(BOX, **hs.ABSORBING, **{NP: 3000, SCAT: 20.0}), "hot_spots", {1: 1.0e6, 2: 0.9e6}, 8.0),
    "ddmc-1d": ("stepdiff_ddmc", dict(SLAB, **{NP: 4000, SCAT: 60.0}), "palette3", {0: 1.0e5}, 4.0),
    "ddmc-3d": ("stepdiff_ddmc", dict(BOX, **{NP: 6000, SCAT: 200.0}), None, {1: 1.0e5, 2: 1.1e5}, 4.0),
    "hybrid-2d": ("stepdiff_smr_hybrid", dict(SMR2, **{NP: 8000, TAU: 10.0}), "islands", {2: 1.0e5, 1: 1.1e5}, 4.0),
}


def _temps(faces):
    t = [0.0] * 6
    for f, v in faces.items():
        t[f] = v
    return t


def _deck(cid, source=True):
    deck, ov, pattern, faces, cf = CASES[cid]
    ov = dict(ov)
    if source:
        ov["jaybenne_amd/bsource_num_particles"] = N_B
        for f, v in faces.items():
            ov[f"jaybenne_amd/bsource_{bm.FACES[f]}_temperature"] = v
    state = hs.state_for(deck, ov, pattern) if pattern else None
    return load_deck(deck, ov), state, _temps(faces), cf


def _driver(cid, device, source=True, **kw):
    from jaybenne_amd import mcblock
    pin, state, temps, cf = _deck(cid, source)
    kw.setdefault("ledger", True)
    return mcblock.McblockDriver(pin, device=device, capacity_factor=cf, initial_state=state, **kw), pin, temps


def _oracle(cid):
    from helpers import make_oracle
    from oracle import orc
    pin, state, temps, cf = _deck(cid)
    O, mesh, pkg = make_oracle(pin, orc.MATH_PORTABLE, capacity_factor=cf + 2.0, initial_state=state)
    return O, mesh, pin, temps


_REFERENCE = {}


def _reference(cid, cycles):
    """The oracle + model run of a case, once per process and shared: per cycle (swarm, tally, ledger) that nobody
    changes, and the swarm before the first cycle."""
    if cid not in _REFERENCE or len(_REFERENCE[cid][1]) < cycles:
        O, mesh, pin, temps = _oracle(cid)
        start = {k: v[:O.n].copy() for k, v in O.sw.items()}
        dt, t, out = pin.GetReal("jaybenne", "dt"), 0.0, []
        for _ in range(cycles):
            led = bm.oracle_cycle(O, pin, t, temps, N_B)
            t += dt
            out.append(({k: v[:O.n].copy() for k, v in O.sw.items()}, O.fields["tally"].copy(), led))
        _REFERENCE[cid] = (start, out, mesh)
    start, out, mesh = _REFERENCE[cid]
    return start, out[:cycles], mesh


def _by_id_equal(g, ref):
    og, orf = np.argsort(g["id"]), np.argsort(ref["id"])
    assert len(g["id"]) == len(ref["id"])
    for k in ref:
        a, b = g[k][og], ref[k][orf]
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (k, bad[:5], a[bad[:5]], b[bad[:5]])


# ---- 1. sourcing -----------------------------------------------------------------------------------
def _source_once(md, jb, t_start, dt):
    n0, id0 = md.n, md.next_id
    jb.SourceBoundaryPhotons(md, t_start, dt)
    g = md.get_swarm()
    return n0, id0, {k: v[n0:].copy() for k, v in g.items()}


def _model_photons(mesh, pin, temps, epoch, id0, t_start, dt):
    sb, c, seed = _constants(pin)
    cells, rec = bm.count(mesh, sb, seed, temps, N_B, dt, epoch)
    parts, base = [], id0
    for b in sorted(cells):
        parts.append(bm.photons(mesh, sb, c, seed, temps, cells[b], b, base, t_start, dt))
        base += len(parts[-1]["id"])
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}, rec


def _constants(pin):
    from jaybenne_amd import mcblock
    pkg = mcblock.Initialize(pin)
    return pkg.opacity.sb, pkg.opacity.c, pin.GetOrAddInteger("jaybenne", "seed", 123)


SOURCING = ([("imc-3d", {f: 1.0e5 * (1.0 + 0.1 * f)}) for f in range(6)] +
            [("hybrid-2d", {2: 1.0e5, 1: 1.1e5}), ("ddmc-1d", {0: 1.0e5})])


@pytest.mark.parametrize("cid,faces", SOURCING, ids=[f"{c}-{'+'.join(bm.FACES[f] for f in fs)}" for c, fs in SOURCING])
def test_sourced_photons_equal_the_model(gpu_device, cid, faces):
    """After jb_source_boundary_count / _fill every attribute of every new photon is the model's, bit for bit, in slot
    order; e_face / n_face are the model's; the same call gives the same bits."""
    from jaybenne_amd import jaybenne as jb
    drv, pin, _ = _driver(cid, gpu_device, source=False)
    md, mesh = drv.md, drv.mesh
    temps = _temps(faces)
    md.bsource_num_particles = N_B
    for f, v in faces.items():
        jb.SetBoundarySource(md, f, v)
    got = C.c_double(0.0)
    assert md.lib.jb_get_boundary_source(md.pkg.ctx, next(iter(faces)), C.byref(got)) == 0
    assert got.value == temps[next(iter(faces))]
    assert md.lib.jb_boundary_face_cells(md.pkg.ctx, md.handle) == bm.face_cells_total(mesh, temps) \
        == jb.boundary_face_cells_total(md)
    md.cycle = 1
    t_start, dt = 0.125, drv.dt
    n0, id0, new = _source_once(md, jb, t_start, dt)
    want, rec = _model_photons(mesh, pin, temps, 1, id0, t_start, dt)
    assert md.n - n0 == len(want["id"]) == sum(rec["n_face"]) and abs(md.n - n0 - N_B) < 0.1 * N_B
    assert md.next_id == id0 + len(want["id"])
    for k in want:
        bad = np.nonzero(new[k] != want[k])[0]
        assert bad.size == 0, (k, bad[:5], new[k][bad[:5]], want[k][bad[:5]])
    hist = md.boundary_source_history[-1]
    assert hist["n_face"] == rec["n_face"]
    for f in range(6):
        assert abs(hist["e_face"][f] - rec["e_face"][f]) <= 1e-12 * rec["e_face"][f], (f, hist["e_face"], rec["e_face"])
    if cid == "hybrid-2d":      # the ix2 face carries cells of two areas: two weights per photon count
        assert len({float(mesh.blk_dx[b, 0]) for b, f in bm.source_faces(mesh, temps) if f == 2}) == 2
    # the same call again, from the same state: the same bits (photons and record)
    md.sv.n, md.next_id = n0, id0
    _, _, again = _source_once(md, jb, t_start, dt)
    for k in new:
        assert np.array_equal(new[k], again[k]), k
    assert md.boundary_source_history[-1] == hist


# ---- 2. two full cycles against the oracle + model ---------------------------------------------------
def _cycles_equal_the_reference(drv, cid, cycles, exact=True):
    from test_gpu_hetero import _variant
    from test_gpu_ledger import _compare_ledger
    from test_gpu_lean import _compare_within_tolerance
    start, ref, mesh = _reference(cid, cycles)
    md = drv.md
    _by_id_equal({k: v for k, v in md.get_swarm().items() if k != "status"},
                 {k: v for k, v in start.items() if k != "status"})
    variants = []
    for cycle in range(cycles):
        assert drv.Step() == drv.jb.TaskStatus.complete
        variants.append(_variant(drv))
        sw, tally, led = ref[cycle]
        g = md.get_swarm()
        assert md.n == len(sw["id"])
        if exact:
            _by_id_equal(g, sw)
        else:
            _compare_within_tolerance(g, sw, len(sw["id"]), mesh, drv.dt, by_id=True)
        sl = mesh.interior()
        np.testing.assert_allclose(md.get_field("tally")[sl], tally[sl], rtol=1e-12 if exact else 1e-9, atol=0)
        _compare_ledger(md.ledger, led, 1e-12 if exact else 1e-9)
        hist = md.boundary_source_history[-1]
        assert hist["cycle"] == cycle + 1 and hist["n_face"] == led["n_sourced_face"]
        for f in range(6):
            assert abs(hist["e_face"][f] - led["e_sourced_face"][f]) <= 1e-12 * led["e_sourced_face"][f]
        assert sum(led["n_sourced_face"]) > 0.9 * N_B
    return variants


@pytest.mark.parametrize("cid", ["imc-3d-hot", "imc-3d"])
def test_two_cycles_k_transport(gpu_device, cid):
    drv, _, _ = _driver(cid, gpu_device)
    variants = _cycles_equal_the_reference(drv, cid, 2)
    assert all(v.startswith("k_transport<3") for v in variants), variants


@pytest.mark.parametrize("cid", ["ddmc-1d", "ddmc-3d"])
@pytest.mark.parametrize("queues", ["k_ddmc_q", "k_ddmc_all"])
def test_two_cycles_all_ddmc(gpu_device, monkeypatch, cid, queues):
    if queues == "k_ddmc_all":
        monkeypatch.setenv("JB_DDMC_QUEUES", "0")
    drv, _, _ = _driver(cid, gpu_device)
    variants = _cycles_equal_the_reference(drv, cid, 2)
    assert all(v.startswith("k_ddmc_all<") and ("queues" in v) == (queues == "k_ddmc_q") for v in variants), variants
    # the albedo admitted some and sent some back through the face they came from
    led = _reference(cid, 2)[1][0][2]
    for f, t in enumerate(_temps(CASES[cid][3])):
        if t > 0.0:
            assert 0 < led["n_escaped"][f] < led["n_sourced_face"][f]


def test_two_cycles_k_hybrid(gpu_device):
    drv, _, _ = _driver("hybrid-2d", gpu_device)
    variants = _cycles_equal_the_reference(drv, "hybrid-2d", 2)
    assert all(v.startswith("k_hybrid<2") for v in variants), variants


@pytest.mark.lean
@pytest.mark.parametrize("cid", ["imc-3d", "hybrid-2d"])
def test_one_cycle_lean_arithmetic(gpu_device, cid):
    """The library's default arithmetic: within the stated 1e-9 of the oracle after one cycle, integer attributes and
    stream states equal."""
    drv, _, _ = _driver(cid, gpu_device)
    assert drv.pkg.arithmetic() == "lean"
    _cycles_equal_the_reference(drv, cid, 1, exact=False)


# ---- 3. one rank against several ---------------------------------------------------------------------
def _rank_worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_EXACT_ARITH="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import mcblock
        from jaybenne_amd.comm import Comm
        for handoff in ("c", "step"):
            os.environ["JB_HANDOFF"] = handoff
            pin, state, temps, cf = _deck("imc-3d")
            drv = mcblock.McblockDriver(pin, rank=rank, nranks=world, comm=Comm(), device=torch.device("cuda", 0),
                                        capacity_factor=cf, initial_state=state, ledger=True)
            md = drv.md
            for _ in range(2):
                assert drv.Step() == drv.jb.TaskStatus.complete
            assert md.handoff_path().startswith("c: jb_radiation_step_ranks" if handoff == "step" else "c: jb_exchange")
            g = md.get_swarm()
            g["blk"] = md.gids[g["blk"]]
            np.savez(os.path.join(outdir, f"{handoff}{rank}.npz"), next_id=np.array([md.next_id]),
                     e_face=np.array([h["e_face"] for h in md.boundary_source_history]),
                     n_face=np.array([h["n_face"] for h in md.boundary_source_history]),
                     e_sourced=np.array([h["e_sourced"] for h in md.ledger_history]),
                     residual=np.array([h["residual"] for h in md.ledger_history]), **g)
            md.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_give_the_photons_of_one(gpu_device, tmp_path):
    """The 3-D case on two gloo ranks sharing the card -- through the Python loop and through JB_HANDOFF=step -- gives
    the photons of one rank by id, the same next_id, and the same per-face record on every rank."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _run_workers
    drv, _, _ = _driver("imc-3d", gpu_device)
    for _ in range(2):
        assert drv.Step() == drv.jb.TaskStatus.complete
    one = drv.md.get_swarm()
    hist = drv.md.boundary_source_history
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)])
    for handoff in ("c", "step"):
        parts = [np.load(tmp_path / f"{handoff}{r}.npz") for r in range(2)]
        assert all(len(p["id"]) > 0 for p in parts)
        got = {k: np.concatenate([p[k] for p in parts]) for k in one}
        _by_id_equal(got, one)
        for p in parts:
            assert int(p["next_id"][0]) == drv.md.next_id
            assert np.array_equal(p["n_face"], np.array([h["n_face"] for h in hist]))
            want = np.array([h["e_face"] for h in hist])
            assert np.all(np.abs(p["e_face"] - want) <= 1e-12 * want)
            assert np.all(p["residual"] <= 1e-12)
        assert np.array_equal(parts[0]["e_face"], parts[1]["e_face"])        # reduced in rank order: the same bits


# ---- 4. the C path and the checked library -----------------------------------------------------------
def test_c_path_gives_the_photons_of_the_python_path(gpu_device):
    """jb_radiation_step on the 1-D case: the library runs the boundary source behind the emission source itself."""
    from jaybenne_amd import _lib
    py, _, _ = _driver("ddmc-1d", gpu_device)
    for _ in range(2):
        assert py.Step() == py.jb.TaskStatus.complete
    drv, _, temps = _driver("ddmc-1d", gpu_device)
    md = drv.md
    _lib.check(md.lib.jb_set_boundary_source_count(md.pkg.ctx, N_B, bm.face_cells_total(drv.mesh, temps)))
    next_id, cycle, t = C.c_uint64(md.next_id), C.c_uint32(0), 0.0
    for _ in range(2):
        md.reserve(md.n + 2 * N_B)
        md._sync_stream()
        _lib.check(md.lib.jb_radiation_step(md.pkg.ctx, md.handle, C.byref(md.sv), t, drv.dt, C.byref(next_id),
                                            C.byref(cycle), md.prefix.data_ptr()))
        t += drv.dt
        last = _lib.BoundarySourceRecord()
        _lib.check(md.lib.jb_boundary_source_last(md.pkg.ctx, C.byref(last)))
        want = py.md.boundary_source_history[cycle.value - 1]
        assert list(last.n_face) == want["n_face"] and list(last.e_face) == want["e_face"]
    assert next_id.value == py.md.next_id
    _by_id_equal(md.get_swarm(), py.md.get_swarm())
    led = _lib.EnergyLedger()
    _lib.check(md.lib.jb_ledger_last(md.pkg.ctx, C.byref(led)))
    assert led.as_dict()["e_sourced"] == py.md.ledger["e_sourced"] and led.n_sourced == py.md.ledger["n_sourced"]


def test_checked_library_one_cycle_without_violations(gpu_device, checked_lib):
    env = dict(os.environ, JAYBENNE_AMD_LIB=checked_lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "checked-1d"], capture_output=True, text=True,
                         env=env, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    _clean(out["report"])
    assert out["n_sourced"] > 0.9 * N_B and out["launches"] == 2


def test_both_command_line_hosts_write_the_per_face_sourced_energy(gpu_device, tmp_path):
    """``python -m jaybenne_amd`` and the native ``examples/mcblock_amd`` on the stepdiff deck with the ix1 face open
    and hot: every ``--ledger`` line carries ``e_sourced_face`` = sb T^4 A dt, both hosts write the same source terms,
    and the balance closes at rounding level."""
    from helpers import DECK_DIR
    exe = os.path.join(ROOT, "examples", "mcblock_amd")
    assert os.path.exists(exe), "examples/mcblock_amd has not been built (__graft_entry__.build())"
    temp = 1.0e5
    ov = {"parthenon/swarm/ix1_bc": O_, NP: 4000, "jaybenne_amd/bsource_ix1_temperature": temp,
          "jaybenne_amd/bsource_num_particles": N_B}
    pin = load_deck("stepdiff", ov)
    dt = pin.GetReal("jaybenne", "dt")
    ov["parthenon/time/tlim"] = 1.5 * dt                    # two cycles on either host
    args = ["-i", os.path.join(DECK_DIR, "stepdiff.in")] + [f"{k}={v}" for k, v in ov.items()]
    env = dict(os.environ, JB_EXACT_ARITH="1")
    env.pop("JB_LEDGER", None)
    lines = {}
    for name, cmd in (("py", [sys.executable, "-m", "jaybenne_amd"]), ("cc", [exe])):
        res = subprocess.run(cmd + args + ["--ledger", str(tmp_path / f"{name}.jsonl")], capture_output=True, text=True,
                             env=env, timeout=240, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        lines[name] = [json.loads(line) for line in open(tmp_path / f"{name}.jsonl")]
    sb, _, _ = _constants(pin)
    want = sb * temp ** 4 * 1.0 * dt                        # the ix1 face of the 1-D deck: area 1
    assert len(lines["py"]) == len(lines["cc"]) == 2
    for a, b in zip(lines["py"], lines["cc"]):
        assert a.keys() == b.keys()
        for got in (a, b):
            assert abs(got["e_sourced_face"][0] - want) <= 1e-12 * want and not any(got["e_sourced_face"][1:])
            assert abs(got["n_sourced_face"][0] - N_B) <= 1 and got["n_sourced"] == got["n_sourced_face"][0]
            assert abs(got["e_sourced"] - want) <= 1e-12 * want and got["residual"] <= 1e-12
        for k in ("e_sourced_face", "n_sourced_face", "e_sourced", "n_sourced", "n_escaped", "n_census"):
            assert a[k] == b[k], (k, a[k], b[k])


# ---- 5. off path and errors --------------------------------------------------------------------------
def test_every_face_off_launches_nothing_and_changes_nothing(gpu_device):
    from helpers import make_oracle, run_oracle_cycles
    from jaybenne_amd import _lib, mcblock
    from oracle import orc
    from test_gpu_parity import _compare_swarm_by_id
    ov = {"jaybenne/num_particles": 2000}
    drv = mcblock.McblockDriver(load_deck("stepdiff", ov), device=gpu_device, ledger=True)
    for _ in range(2):
        assert drv.Step() == drv.jb.TaskStatus.complete
    last = _lib.BoundarySourceRecord()
    _lib.check(drv.md.lib.jb_boundary_source_last(drv.md.pkg.ctx, C.byref(last)))
    assert last.kernel_launches == 0 and sum(last.n_face) == 0 and not any(last.e_face)
    assert drv.md.lib.jb_boundary_source_enabled(drv.md.pkg.ctx) == 0 and drv.md.boundary_source_history == []
    assert "e_sourced_face" not in drv.md.ledger
    O, _, _ = make_oracle(load_deck("stepdiff", ov), orc.MATH_PORTABLE)
    run_oracle_cycles(O, load_deck("stepdiff", ov), 2)
    _compare_swarm_by_id(drv.md, O)


def test_error_paths(gpu_device):
    from jaybenne_amd import _lib
    drv, _, _ = _driver("imc-3d", gpu_device, source=False)       # x3 is not periodic here ...
    md, lib, ctx = drv.md, drv.md.lib, drv.md.pkg.ctx
    assert lib.jb_set_boundary_source(ctx, 6, 1.0) == _lib.JB_ERR_INVALID
    assert lib.jb_set_boundary_source(ctx, -1, 1.0) == _lib.JB_ERR_INVALID
    assert lib.jb_set_boundary_source(ctx, 0, -1.0) == _lib.JB_ERR_INVALID
    assert lib.jb_set_boundary_source(ctx, 0, float("nan")) == _lib.JB_ERR_INVALID
    assert lib.jb_set_boundary_source(ctx, 0, float("inf")) == _lib.JB_ERR_INVALID
    assert lib.jb_boundary_source_enabled(ctx) == 0

    def count(d, num_particles, cells):
        m = d.md
        words = int(m.lib.jb_boundary_prefix_words(m.handle))
        import torch
        prefix = torch.zeros(words, dtype=torch.int32, device=gpu_device)
        nper = np.zeros(m.nblocks, dtype=np.int32)
        plan = _lib.BoundarySourcePlan(nper_block=nper.ctypes.data)
        m._sync_stream()
        return m.lib.jb_source_boundary_count(m.pkg.ctx, m.handle, d.dt, cells, num_particles, 1, C.byref(plan),
                                              prefix.data_ptr())

    assert lib.jb_set_boundary_source(ctx, 0, 1.0e5) == 0
    cells = bm.face_cells_total(drv.mesh, [1.0e5, 0, 0, 0, 0, 0])
    assert count(drv, cells - 1, cells) == _lib.JB_ERR_INVALID and b"fewer than one" in lib.jb_last_error()   # npc < 1
    assert count(drv, cells, cells) == 0
    slab, _, _ = _driver("ddmc-1d", gpu_device, source=False)
    assert slab.md.lib.jb_set_boundary_source(slab.md.pkg.ctx, 2, 1.0e5) == 0
    assert count(slab, N_B, 1) == _lib.JB_ERR_INVALID and b"not active" in lib.jb_last_error()              # inactive axis
    from jaybenne_amd import mcblock
    per = mcblock.McblockDriver(load_deck("stepdiff", dict(ax.geometry_overrides("G3U", ax.BOUNDARY_SETS["S1"]),
                                                           **{NP: 2000})), device=gpu_device)
    assert per.md.lib.jb_set_boundary_source(per.md.pkg.ctx, 4, 1.0e5) == 0
    assert count(per, N_B, 192) == _lib.JB_ERR_INVALID and b"periodic" in lib.jb_last_error()               # periodic face
    with pytest.raises(_lib.JaybenneError):        # ... and the host raises what the library answers
        per.md.bsource_num_particles = N_B
        per.jb.SetBoundarySource(per.md, 4, 1.0e5)
        per.md.cycle = 1
        per.jb.SourceBoundaryPhotons(per.md, 0.0, per.dt)


# ---- in the child process ------------------------------------------------------------------------------
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ["JB_EXACT_ARITH"] = "1"
    import torch
    from jaybenne_amd import _lib
    assert sys.argv[1] == "checked-1d"
    drv, _, _ = _driver("ddmc-1d", torch.device("cuda", 0))
    assert drv.md.invariants_enabled()
    assert drv.Step() == drv.jb.TaskStatus.complete
    last = _lib.BoundarySourceRecord()
    _lib.check(drv.md.lib.jb_boundary_source_last(drv.md.pkg.ctx, C.byref(last)))
    print(json.dumps({"report": drv.md.invariant_report(), "n_sourced": drv.md.ledger["n_sourced"],
                      "launches": int(last.kernel_launches)}))
