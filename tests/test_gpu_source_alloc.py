"""Energy-proportional source allocation (include/jaybenne_amd.h: jb_set_source_allocation) on the GPU.  The
reference is tests/source_alloc_model.py, steps 1-4 of the contract restated in numpy and Python floats: block sums,
E_tot, src_num, src_ew, the per-block counts and the prefix are compared bit for bit, photons bit for bit by creation
id.

Meshes: 1-D with blocks of 50, 257 and 513 cells (fewer cells than threads; the scan's carry and the strided sum's
tail); the two-level 2-D and 3-D meshes of tests/axis_cases.py (dv differs by level) with temperature and density
different in every cell; a view with a halo copy; crafted 1-D states."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import axis_cases as ax
import hetero_states as hs
import source_alloc_model as sam
import tilt_model as tm
from helpers import load_deck
from jaybenne_amd._lib import ALLOC_ENERGY, ALLOC_UNIFORM  # noqa: F401  (the mode's symbols: without it nothing here runs)
from test_gpu_invariants import _clean, checked_lib  # noqa: F401  (checked_lib: fixture)

pytestmark = pytest.mark.gpu

NP, SCAT = ax.NP, ax.SCAT
ALLOC = "jaybenne_amd/source_allocation"
TILT = "jaybenne_amd/source_tilt"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECKS = os.path.join(ROOT, "jaybenne_amd", "decks")
R_, O_, P_ = ax.R, ax.O, ax.P
BOX_EXT = ((-0.25, 0.75), (0.5, 2.0), (-1.0, -0.75))


class BothState:
    """Temperature AND density different in every cell: hetero_states' ``smooth`` factor on rho, ``hot_spots`` on
    sie (picklable: the rank workers receive it through spawn)."""

    def __call__(self, mesh, pkg, gids=None):
        from jaybenne_amd import mcblock
        ic = mcblock.ProblemGenerator(mesh, pkg)
        rho, sie = ic["rho"].copy(), ic["sie"].copy()
        for b in range(mesh.nblocks):
            rho[b] *= hs.rho_factor(mesh, pkg, "smooth", b)[0]
            sie[b] *= hs.rho_factor(mesh, pkg, "hot_spots", b)[1]
        mesh.fill_ghosts(rho)
        mesh.fill_ghosts(sie)
        out = {"rho": rho, "sie": sie, "u": rho * sie}
        if gids is not None:
            out = {k: np.ascontiguousarray(v[np.asarray(gids)]) for k, v in out.items()}
        return out


def _geometry(name):
    if name.startswith("1d-"):
        cells = int(name[3:])
        return "stepdiff", ax.deck_overrides((2 * cells,), (cells,), ((-0.5, 0.5),), (R_, R_) + (P_,) * 4)
    if name == "2d-smr":
        return "stepdiff_smr", ax.geometry_overrides("G2S", ax.BOUNDARY_SETS["S1"][:4] + (P_,) * 2)
    if name == "3d-smr":
        return "stepdiff_smr", ax.geometry_overrides("G3S", ax.BOUNDARY_SETS["S1"])
    return "stepdiff", ax.deck_overrides((8, 8, 8), (4, 4, 4), BOX_EXT, ax.BOUNDARY_SETS["S1"])


def _driver(deck, ov, device, state=BothState(), **kw):
    from jaybenne_amd import mcblock
    return mcblock.McblockDriver(load_deck(deck, ov), device=device, initial_state=state, **kw)


def _par(drv):
    from jaybenne_amd import mcblock
    o = drv.mcb.opacity
    par = dict(cv=drv.mcb.eos.cv, sb=o.sb, c=o.c, kappa=o.kappa, seed=drv.pin.GetOrAddInteger("jaybenne", "seed", 123))
    if o.model == mcblock.OPAC_EPBREMSS:     # (the library's coefficients are the oracle's: test_gpu_parity)
        from oracle import orc
        par["ep_E"] = orc.model_coefficients(o.time_scale, o.mass_scale, o.length_scale, o.temperature_scale)["ep_E"]
    return par


def _host(md, name):
    """A field of the resident blocks with ghosts, [nblocks, nk, nj, ni]."""
    md._sync_stream()
    return md.fields[name].cpu().numpy()


def _two_phase(md, source_type, dt, epoch, e_total=None):
    """jb_source_energy_sums, the total, jb_source_photons_count_energy: (e_local, E_tot, nper)."""
    from jaybenne_amd import _lib, jaybenne as jb
    e_local = np.full(md.nblocks, -1.0)
    md._sync_stream()
    _lib.check(md.lib.jb_source_energy_sums(md.pkg.ctx, md.handle, int(source_type), dt, e_local.ctypes.data))
    staged = _host(md, "src_ew").copy()
    if e_total is None:
        e_gid = np.ascontiguousarray(jb.gather_block_energies(md, e_local))
        e_total = float(md.lib.jb_source_energy_total(e_gid.ctypes.data, md.mesh.nblocks))
    nper = np.full(md.nblocks, -1, dtype=np.int32)
    _lib.check(md.lib.jb_source_photons_count_energy(md.pkg.ctx, md.handle, int(source_type), dt, epoch, e_total,
                                                     nper.ctypes.data, md.prefix.data_ptr()))
    return e_local, e_total, nper, staged


def _model(drv, source_type, dt, epoch, n_target=None, blocks=None):
    md = drv.md
    rows = slice(None) if blocks is None else [int(md.local_index[b]) for b in blocks]
    return sam.source_call(drv.mesh, _host(md, "rho")[rows], _host(md, "sie")[rows], _host(md, "fleck")[rows], _par(drv),
                           int(source_type), dt, drv.pkg.Param("num_particles") if n_target is None else n_target,
                           epoch, blocks=blocks)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _compare(drv, call, e_local, e_total, nper, staged=None):
    """The library's block sums, total, fields, counts and prefix against the model's, bit for bit, for the blocks
    this MeshData owns."""
    md, mesh = drv.md, drv.mesh
    sl = mesh.interior()[1:]
    assert _bits([e_total]) == _bits([call.e_total]), (e_total, call.e_total)
    num, ew = _host(md, "src_num"), _host(md, "src_ew")
    prefix = md.prefix.cpu().numpy().reshape(md.nblocks, mesh.ncell)
    for row, b in enumerate(md.gids):
        b = int(b)
        assert _bits([e_local[row]]) == _bits([call.e_block[b]]), (b, e_local[row], call.e_block[b])
        if staged is not None:
            assert np.array_equal(_bits(staged[row][sl]), _bits(call.erad[b])), b
        bad = np.nonzero(num[row][sl] != call.n[b])
        assert bad[0].size == 0, (b, bad, num[row][sl][bad][:5], call.n[b][bad][:5])
        bad = np.nonzero(_bits(ew[row][sl]) != _bits(call.ew[b]))
        assert bad[0].size == 0, (b, bad, ew[row][sl][bad][:5], call.ew[b][bad][:5])
        assert int(nper[row]) == call.nper[b], (b, nper[row], call.nper[b])
        assert np.array_equal(prefix[row], call.prefix[b]), b
    assert not nper[md.nowned:].any() and not e_local[md.nowned:].any()       # halo copies


# ---- 1. the count against the model ---------------------------------------------------------------------------
COUNT_CASES = [("1d-50", 3000), ("1d-257", 6000), ("1d-513", 9000), ("2d-smr", 6000), ("3d-smr", 20000)]


@pytest.mark.parametrize("source", ["thermal", "emission"])
@pytest.mark.parametrize("geom,n", COUNT_CASES, ids=[g for g, _ in COUNT_CASES])
def test_count_equals_the_model(gpu_device, geom, n, source):
    from jaybenne_amd import _lib, jaybenne as jb
    deck, ov = _geometry(geom)
    drv = _driver(deck, dict(ov, **hs.ABSORBING, **{NP: n, ALLOC: "energy"}), gpu_device, capacity_factor=2.0)
    md = drv.md
    assert md.source_allocation == "energy" and md.lib.jb_get_source_allocation(md.pkg.ctx) == _lib.ALLOC_ENERGY
    st = jb.SourceType[source]
    dt = drv.dt if source == "emission" else 0.0
    jb.UpdateDerivedTransportFields(md, drv.dt)
    e_local, e_total, nper, staged = _two_phase(md, st, dt, 5)
    call = _model(drv, st, dt, 5)
    _compare(drv, call, e_local, e_total, nper, staged)
    # the state exercises the definition: cells with several photons, cells whose fraction decides, cells with none
    n_all = np.concatenate([call.n[b].reshape(-1) for b in range(drv.mesh.nblocks)])
    assert (n_all >= 2).any() and (n_all == 0).any() and abs(int(n_all.sum()) - n) <= n_all.size
    # ... and jb_source_photons_count runs the three in a row on this wholly resident mesh: the same bits
    nper2 = np.zeros(md.nblocks, dtype=np.int32)
    _lib.check(md.lib.jb_source_photons_count(md.pkg.ctx, md.handle, int(st), dt, 1, 5, nper2.ctypes.data,
                                              md.prefix.data_ptr()))
    _compare(drv, call, e_local, e_total, nper2)


@pytest.mark.parametrize("source", ["thermal", "emission"])
def test_count_equals_the_model_under_epbremss(gpu_device, source):
    """k_salloc_energy's emission branch forms fleck * opac_emissivity * dv * dt: with EPBremss the emissivity is
    (E (rho rho)) sqrt(T).  The 3-D two-level row of tests/freq_cases.py (rho and sie different in every cell, the
    Fleck factor from the frequency-integrated emissivity), under source_allocation = energy."""
    import freq_cases as fc
    from jaybenne_amd import _lib, jaybenne as jb, mcblock
    case = fc.BY_ID["F3S-hybrid"]
    ov = fc.overrides(case, **{ALLOC: "energy"})
    drv = _driver(case.deck, ov, gpu_device, state=hs.state_for(case.deck, ov, fc.PATTERN), capacity_factor=fc.CAPACITY_FACTOR)
    md = drv.md
    assert md.source_allocation == "energy" and md.lib.jb_get_source_allocation(md.pkg.ctx) == _lib.ALLOC_ENERGY
    assert drv.mcb.opacity.model == mcblock.OPAC_EPBREMSS and _par(drv)["ep_E"] > 0.0 and _par(drv)["kappa"] == 0.0
    st = jb.SourceType[source]
    dt = drv.dt if source == "emission" else 0.0
    jb.UpdateDerivedTransportFields(md, drv.dt)
    e_local, e_total, nper, staged = _two_phase(md, st, dt, 5)
    call = _model(drv, st, dt, 5)
    _compare(drv, call, e_local, e_total, nper, staged)
    n_all = np.concatenate([call.n[b].reshape(-1) for b in range(drv.mesh.nblocks)])
    assert (n_all >= 2).any() and (n_all == 0).any() and abs(int(n_all.sum()) - case.photons) <= n_all.size
    f = _host(md, "fleck")[drv.mesh.interior()]
    assert len(np.unique(f)) > 0.4 * f.size              # a Fleck factor of its own in (nearly) every cell


def test_view_with_a_halo_copy(gpu_device):
    """Rank 0 of a two-rank block partition: the halo copies give a block sum of 0, get no count, and none of their
    fields is written; the owned blocks equal the model's, with E_tot taken over the whole mesh."""
    from jaybenne_amd import jaybenne as jb
    deck, ov = _geometry("2d-smr")
    drv = _driver(deck, dict(ov, **hs.ABSORBING, **{NP: 6000}), gpu_device, rank=0, nranks=2, capacity_factor=2.0)
    md = drv.md
    assert md.nblocks > md.nowned > 0 and md.nowned < drv.mesh.nblocks
    md.source_allocation = "energy"
    jb.UpdateDerivedTransportFields(md, drv.dt)
    whole = _driver(deck, dict(ov, **hs.ABSORBING, **{NP: 6000, ALLOC: "energy"}), gpu_device, capacity_factor=2.0)
    jb.UpdateDerivedTransportFields(whole.md, whole.dt)
    call = _model(whole, jb.SourceType.emission, whole.dt, 2)
    for name in ("src_ew", "src_num"):
        md.fields[name][md.nowned:] = -7.0
    e_local, e_total, nper, _ = _two_phase(md, jb.SourceType.emission, drv.dt, 2, e_total=call.e_total)
    _compare(drv, call, e_local, e_total, nper)
    for name in ("src_ew", "src_num"):
        assert bool((md.fields[name][md.nowned:] == -7.0).all()), name


# ---- 2. crafted states ------------------------------------------------------------------------------------------
def _crafted(device, n):
    deck, ov = _geometry("1d-50")
    return _driver(deck, dict(ov, **{NP: n, ALLOC: "energy"}), device, state=None, capacity_factor=1.5)


def _set_temperature(drv, temp):
    """temp: [nblocks, ncell] interior temperatures; ghosts 0."""
    md, mesh = drv.md, drv.mesh
    sie = np.zeros(mesh.field_shape)
    sie[mesh.interior()] = (np.asarray(temp) * drv.mcb.eos.cv).reshape((mesh.nblocks,) + tuple(mesh.nx[::-1]))
    md.set_field("sie", sie)


def _thermal_count(drv, epoch=7):
    from jaybenne_amd import jaybenne as jb
    e_local, e_total, nper, staged = _two_phase(drv.md, jb.SourceType.thermal, 0.0, epoch)
    call = _model(drv, jb.SourceType.thermal, 0.0, epoch)
    _compare(drv, call, e_local, e_total, nper, staged)
    return call, nper


def test_one_hot_cell_takes_every_photon(gpu_device):
    from jaybenne_amd import jaybenne as jb
    drv = _crafted(gpu_device, 100000)
    temp = np.zeros((2, 50))
    temp[1, 37] = 1.0e5
    _set_temperature(drv, temp)
    call, nper = _thermal_count(drv, epoch=0)
    assert nper.tolist() == [0, call.nper[1]] and abs(call.nper[1] - 100000) <= 1
    assert int((call.n[1] > 0).sum()) == 1 and call.e_block[0] == 0.0 and not call.ew[0].any()
    md = drv.md
    md.sv.n, md.next_id, md.cycle = 0, 0, 0
    jb.SourcePhotons(md, jb.SourceType.thermal, 0.0, 0.0, per_block=True)
    g = md.get_swarm()
    assert len(g["id"]) == call.nper[1] and np.array_equal(np.sort(g["id"]), np.arange(call.nper[1], dtype=np.uint64))
    assert (g["blk"] == 1).all() and (g["ip"] == 37 + drv.mesh.is_[0]).all()
    assert (g["w"] == call.ew[1].reshape(-1)[37]).all()
    assert math.fsum(g["w"]) == pytest.approx(call.e_total, rel=1e-12)


def test_fractional_cells_and_empty_cells(gpu_device):
    """Three quarters of the cells with nu between 5 and 30, a quarter with nu in (0.1, 0.9) -- roulette: no photon,
    or one of weight erad / nu --, and every tenth cell at temperature 0."""
    nu = 5.0 + 25.0 * ((np.arange(100) * 37) % 100) / 100.0
    nu[::4] = 0.1 + 0.8 * ((np.arange(25) * 7) % 25 + 0.5) / 25.0
    nu[5::10] = 0.0
    n = int(round(nu.sum()))
    drv = _crafted(gpu_device, n)
    _set_temperature(drv, (1.0e5 * nu ** 0.25).reshape(2, 50))
    call, nper = _thermal_count(drv)
    erad = np.concatenate([call.erad[b].reshape(-1) for b in (0, 1)])
    got = erad * call.scale
    cnt = np.concatenate([call.n[b].reshape(-1) for b in (0, 1)])
    ew = np.concatenate([call.ew[b].reshape(-1) for b in (0, 1)])
    frac = (got > 0.1) & (got < 0.9)
    assert frac.sum() >= 20 and np.allclose(got, nu, rtol=1e-2)
    assert set(cnt[frac].tolist()) == {0.0, 1.0}                        # both outcomes occur
    one = frac & (cnt == 1.0)
    assert np.array_equal(ew[one], erad[one] / got[one]) and not ew[frac & (cnt == 0.0)].any()
    assert np.allclose(ew[one], call.e_total / n, rtol=2e-2)           # about E_tot / N
    zero = erad == 0.0
    assert zero.sum() == 10 and not cnt[zero].any() and not ew[zero].any()
    assert abs(int(nper.sum()) - n) <= 90


def test_exact_integer_nu_is_never_rounded_up(gpu_device):
    """32 equal cells per block hold the energy, so every block sum and E_tot are exact (the tree only ever adds equal
    numbers).  For a target of 64 k, nu = erad (64 k / E_tot) is k up to two roundings; the k at which the model's nu
    are whole numbers are used: there the fraction is 0, no draw can exceed it, n = nu and ew = erad / n."""
    drv = _crafted(gpu_device, 64)
    temp = np.zeros((2, 50))
    temp[:, :32] = 1.0e5
    _set_temperature(drv, temp)
    from jaybenne_amd import jaybenne as jb
    par, used = _par(drv), 0
    e0 = float(sam.erad_thermal(np.array([1.0e5 * par["cv"]]), par["cv"], par["sb"], par["c"],
                                (drv.mesh.blk_dx[0, 0] * drv.mesh.blk_dx[0, 1]) * drv.mesh.blk_dx[0, 2])[0])
    for k in range(1, 40):
        if e0 * (64.0 * k / (64.0 * e0)) != float(k):
            continue
        used += 1
        if used > 6:
            break
        drv = _crafted(gpu_device, 64 * k)
        _set_temperature(drv, temp)
        call, nper = _thermal_count(drv, epoch=k)
        assert call.e_total == 64.0 * e0
        for b in (0, 1):
            assert (call.n[b].reshape(-1)[:32] == float(k)).all() and not call.n[b].reshape(-1)[32:].any()
            assert np.array_equal(call.ew[b].reshape(-1)[:32], np.full(32, e0 / k))
        assert nper.tolist() == [32 * k, 32 * k]
    assert used >= 3


# ---- 3. photons ---------------------------------------------------------------------------------------------------
def _local_swarm(md, g, lo=0):
    g = {k: v[lo:].copy() for k, v in g.items()}
    g["blk"] = md.resident_gids[g["blk"]].astype(np.int32)
    return g


def _by_id_bits(got, want, skip=()):
    og, ow = np.argsort(got["id"]), np.argsort(want["id"])
    assert len(got["id"]) == len(want["id"]) > 0
    for k in want:
        if k in skip:
            continue
        a, b = got[k][og], want[k][ow]
        if a.dtype == np.float64:
            a, b = _bits(a), _bits(b)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (k, bad[:5], got[k][og][bad[:5]], want[k][ow][bad[:5]])


@pytest.mark.parametrize("geom,n,tilt", [("1d-50", 1500, "none"), ("2d-smr", 2500, "none"), ("3d", 2500, "linear")],
                         ids=["1d", "2d-smr", "3d-tilted"])
def test_photons_equal_the_model(gpu_device, geom, n, tilt):
    """The initial thermal source (made by the driver) and one emission source behind it: by id every attribute is the
    model's -- the photon numbered p of block b lies in the cell the prefix bisection names, carries that cell's
    src_ew and has the position, direction, frequency and time the fill draws for that id in that cell.  Under
    source_tilt = linear the positions are the tilt model's for the same cells and ids, everything else unchanged."""
    from jaybenne_amd import jaybenne as jb
    deck, ov = _geometry(geom)
    drv = _driver(deck, dict(ov, **hs.ABSORBING, **{NP: n, ALLOC: "energy", TILT: tilt, SCAT: 20.0}), gpu_device,
                  capacity_factor=3.0)
    md, mesh, par = drv.md, drv.mesh, _par(drv)
    sie = _host(md, "sie")
    skip = ("x", "y", "z") if tilt == "linear" else ()

    def positions(g):
        if tilt != "linear":
            return
        blk = g["blk"].astype(np.int64)
        want = tm.photon_positions(mesh, par["seed"], tm.slopes(mesh, sie, par["cv"]), g["id"], blk, blk, g["kp"],
                                   g["jp"], g["ip"])
        for d, k in enumerate(("x", "y", "z")):
            assert np.array_equal(_bits(g[k]), _bits(want[d])), k

    # the initial source: epoch 0, dt 0, ids from 0
    call0 = _model(drv, jb.SourceType.thermal, 0.0, 0)
    n0 = md.n
    assert n0 == sum(call0.nper.values()) and abs(n0 - n) <= mesh.nblocks * mesh.ncell and md.next_id == n0
    assert md.source_e_total == call0.e_total
    got = _local_swarm(md, md.get_swarm())
    _by_id_bits(got, sam.photons(mesh, call0, par, sam.THERMAL, 0.0, 0.0, 0, sie), skip)
    positions(got)
    assert not _host(md, "edelta").any()
    # one emission source behind it: epoch = the cycle, ids behind the thermal photons
    md.cycle = 1
    jb.UpdateDerivedTransportFields(md, drv.dt)
    call1 = _model(drv, jb.SourceType.emission, drv.dt, 1)
    jb.SourcePhotons(md, jb.SourceType.emission, 0.125, drv.dt)
    assert md.n == n0 + sum(call1.nper.values()) and md.next_id == md.n
    got = _local_swarm(md, md.get_swarm(), n0)
    _by_id_bits(got, sam.photons(mesh, call1, par, sam.EMISSION, 0.125, drv.dt, n0, sie), skip)
    positions(got)
    sl = mesh.interior()
    edelta = _host(md, "edelta")[sl]
    for b in range(mesh.nblocks):
        assert np.array_equal(edelta[b], sam.energy_delta(call1.n[b], call1.ew[b], sam.EMISSION)), b
    assert (edelta < 0.0).any()


def test_library_step_gives_the_photons_of_the_python_tasks(gpu_device):
    """jb_radiation_step sources through jb_source_photons_count, which runs the three phases in a row: one cycle
    gives the photons of the Python task list by id."""
    from jaybenne_amd import _lib
    from test_gpu_bsource import _by_id_equal
    deck, ov = _geometry("1d-50")
    ov = dict(ov, **hs.ABSORBING, **{NP: 4000, ALLOC: "energy", SCAT: 150.0})
    py = _driver(deck, ov, gpu_device, capacity_factor=4.0)
    assert py.Step() == py.jb.TaskStatus.complete
    want = py.md.get_swarm()
    cc = _driver(deck, ov, gpu_device, capacity_factor=4.0)
    md = cc.md
    next_id, cycle = C.c_uint64(md.next_id), C.c_uint32(0)
    md.reserve(md.n + 8000)
    md._sync_stream()
    _lib.check(md.lib.jb_radiation_step(md.pkg.ctx, md.handle, C.byref(md.sv), 0.0, cc.dt, C.byref(next_id),
                                        C.byref(cycle), md.prefix.data_ptr()))
    _by_id_equal(md.get_swarm(), want)
    assert int(next_id.value) == py.md.next_id > 7000


def test_uniform_is_untouched_and_the_environment_sets_the_default(gpu_device, monkeypatch):
    """Under uniform the count is the parent's (the model of sourcing.cpp:99-103: every cell floor(npc) or one more)
    and no phase call is accepted; JB_SOURCE_ALLOCATION=energy makes energy the default of jb_initialize, the deck key
    wins."""
    from jaybenne_amd import _lib, jaybenne as jb
    deck, ov = _geometry("1d-50")
    drv = _driver(deck, dict(ov, **{NP: 1000}), gpu_device)
    md = drv.md
    assert md.source_allocation == "uniform" and md.n in range(900, 1101)
    assert set(np.unique(_host(md, "src_num")[drv.mesh.interior()]).tolist()) <= {10.0, 11.0}
    e = np.zeros(md.nblocks)
    assert md.lib.jb_source_energy_sums(md.pkg.ctx, md.handle, 0, 0.0, e.ctypes.data) == _lib.JB_ERR_INVALID
    nper = np.zeros(md.nblocks, dtype=np.int32)
    assert md.lib.jb_source_photons_count_energy(md.pkg.ctx, md.handle, 0, 0.0, 1, 1.0, nper.ctypes.data,
                                                 md.prefix.data_ptr()) == _lib.JB_ERR_INVALID
    assert md.lib.jb_set_source_allocation(md.pkg.ctx, 2) == _lib.JB_ERR_INVALID and md.source_allocation == "uniform"
    jb.SetSourceAllocation(md, "energy")
    assert md.source_allocation == "energy"
    monkeypatch.setenv("JB_SOURCE_ALLOCATION", "energy")
    assert _driver(deck, dict(ov, **{NP: 1000}), gpu_device).md.source_allocation == "energy"
    assert _driver(deck, dict(ov, **{NP: 1000, ALLOC: "uniform"}), gpu_device).md.source_allocation == "uniform"


# ---- 4. ledger and counts -----------------------------------------------------------------------------------------
def test_ledger_sources_the_total(gpu_device):
    """stepdiff (hot half nu = 40, cold half 1e-20 of the energy) with absorption and emission on: the cycle's
    e_sourced is E_tot to 1e-12, n_sourced within the number of sourcing cells of N; so is the initial source."""
    ov = dict(hs.ABSORBING, **{NP: 2000, ALLOC: "energy", SCAT: 150.0})
    drv = _driver("stepdiff", ov, gpu_device, state=None, capacity_factor=4.0, ledger=True)
    md = drv.md
    cells = drv.mesh.nblocks * drv.mesh.ncell
    assert abs(md.n - 2000) <= cells
    assert math.fsum(md.get_swarm()["w"]) == pytest.approx(md.source_e_total, rel=1e-12)
    assert drv.Step() == drv.jb.TaskStatus.complete
    led = md.ledger
    print("ledger", led["e_sourced"], md.source_e_total, led["n_sourced"])
    assert led["e_sourced"] == pytest.approx(md.source_e_total, rel=1e-12) and md.source_e_total > 0.0
    assert abs(led["n_sourced"] - 2000) <= cells
    erad = _host(md, "src_ew")[drv.mesh.interior()] * _host(md, "src_num")[drv.mesh.interior()]
    assert (erad[erad > 0] > 1e-3 * erad.max()).all()          # only cells with nu >= 1 sourced


# ---- 5. yield -----------------------------------------------------------------------------------------------------
def _n_eff(drv):
    fields, rep = drv.jb.EvaluateRadiationMoments(drv.md)
    f = fields.cpu().numpy()
    dv = np.array([drv.mesh.cell_volume(int(b)) for b in drv.md.gids])[:, None, None, None]
    sw, sw2 = math.fsum((f[1][:drv.md.nowned] * dv).reshape(-1)), math.fsum(f[2][:drv.md.nowned].reshape(-1))
    return sw * sw / sw2, int(rep["n_counted"])


def test_stepdiff_census_is_worth_its_photons(gpu_device):
    """stepdiff at N = 2e4 (no absorption, reflecting walls: the census keeps every photon): the census' global
    N_eff = (sum w)^2 / sum w^2 from the moments call's E dv and W2, after the initial source and after the deck's ten
    cycles.  Under energy the 50 hot cells have nu = 400 and weights equal to within 1/400, the cold cells have
    nu ~ 4e-18, below the smallest uniform 2^-53, and source nothing: N_eff >= 0.99 N.  Under uniform half the photons
    sit in the cold half with 1e-20 of the weight: N_eff <= 0.51 N -- the yardstick."""
    n = 20000
    out = {}
    for mode in ("energy", "uniform"):
        drv = _driver("stepdiff", {NP: n, ALLOC: mode}, gpu_device, state=None)
        assert drv.md.source_allocation == mode
        first = _n_eff(drv)
        for _ in range(10):
            assert drv.Step() == drv.jb.TaskStatus.complete
        out[mode] = (first, _n_eff(drv))
        assert drv.md.n == first[1] == out[mode][1][1]            # nothing absorbed, nothing escaped
    print("N_eff", out)
    for neff, counted in out["energy"]:
        assert neff >= 0.99 * n and abs(counted - n) <= 50
    for neff, counted in out["uniform"]:
        assert neff <= 0.51 * n and abs(counted - n) <= 100


# ---- 6. ranks -----------------------------------------------------------------------------------------------------
RANK_OV = dict(ax.deck_overrides((8, 8, 8), (4, 4, 4), BOX_EXT, ax.BOUNDARY_SETS["S1"]), **hs.ABSORBING,
               **{NP: 20000, SCAT: 20.0, ALLOC: "energy"})


def _sourced(drv):
    """The photons of the initial thermal source and of one emission source behind it, not transported; block indices
    global; with the fields of the emission count by global block id."""
    jb, md = drv.jb, drv.md
    e0 = md.source_e_total
    md.cycle = 1
    jb.UpdateDerivedTransportFields(md, drv.dt)
    jb.SourcePhotons(md, jb.SourceType.emission, 0.0, drv.dt)
    g = _local_swarm(md, md.get_swarm())
    sl = drv.mesh.interior()
    g["gids"] = md.gids.copy()
    g["src_num"], g["src_ew"] = md.get_field("src_num")[sl], md.get_field("src_ew")[sl]
    g["e_total"] = np.array([e0, md.source_e_total])
    g["next_id"] = np.array([md.next_id])
    return g


def _rank_worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_EXACT_ARITH="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd.comm import Comm
        for decomposition in ("blocks", "replicated"):
            drv = _driver("stepdiff", RANK_OV, torch.device("cuda", 0), rank=rank, nranks=world, comm=Comm(),
                          capacity_factor=3.0, decomposition=decomposition)
            assert drv.md.source_allocation == "energy" and drv.md.replicated == (decomposition == "replicated")
            np.savez(os.path.join(outdir, f"{decomposition}{rank}.npz"), **_sourced(drv))
            drv.md.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_source_the_photons_of_one(gpu_device, tmp_path):
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)])
    want = _sourced(_driver("stepdiff", RANK_OV, gpu_device, capacity_factor=3.0))
    photon_keys = [k for k in want if k not in ("gids", "src_num", "src_ew", "e_total", "next_id")]
    assert len(want["id"]) > 30000
    for decomposition in ("blocks", "replicated"):
        parts = [np.load(tmp_path / f"{decomposition}{r}.npz") for r in range(2)]
        assert [len(p["gids"]) for p in parts] == ([4, 4] if decomposition == "blocks" else [8, 8])
        for p in parts:
            assert np.array_equal(_bits(p["e_total"]), _bits(want["e_total"])), decomposition      # both calls' E_tot
            assert int(p["next_id"][0]) == int(want["next_id"][0])
            for k in ("src_num", "src_ew"):
                assert np.array_equal(_bits(p[k]), _bits(want[k][p["gids"]])), (decomposition, k)
        assert all(len(p["id"]) > 5000 for p in parts)
        _by_id_bits({k: np.concatenate([p[k] for p in parts]) for k in photon_keys}, {k: want[k] for k in photon_keys})


# ---- 7. the physics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deck,overrides,tol", [
    ("stepdiff", ["parthenon/mesh/nx1=128", "parthenon/meshblock/nx1=128"], 0.05),
    ("stepdiff_smr", ["parthenon/mesh/nx1=64", "parthenon/mesh/nx2=32", "parthenon/meshblock/nx1=16",
                      "parthenon/meshblock/nx2=16"], 0.3)])
def test_reference_gates_under_energy(gpu_device, deck, overrides, tol, capsys):
    from jaybenne_amd.__main__ import main
    rc = main(["-i", os.path.join(DECKS, deck + ".in"), "--tolerance", str(tol), ALLOC + "=energy"] + overrides)
    out = capsys.readouterr().out
    assert rc == 0 and "TEST PASSED" in out, out


def test_infinite_medium_under_energy(gpu_device):
    """inputs/inf.in with emission and feedback on (100 cycles): the domain-mean radiation energy density stays at
    a T0^4 (the gate of tests/test_gpu_regression.py: 0.03)."""
    from jaybenne_amd import constants, mcblock
    pin = load_deck("inf", {ALLOC: "energy", "jaybenne/do_feedback": "true"})
    drv = mcblock.McblockDriver(pin, device=gpu_device)
    assert drv.md.source_allocation == "energy" and drv.pkg.Param("do_emission") and drv.pkg.Param("do_feedback")
    ur = 4.0 * constants.STEFAN_BOLTZMANN / constants.SPEED_OF_LIGHT * drv.mcb.initial_temperature ** 4
    sl = drv.mesh.interior()
    ratio = []
    while drv.time < drv.tlim:
        drv.Step()
        ratio.append(float(drv.md.get_field("tally")[sl].mean()) / ur)
    print("inf ratio", np.mean(ratio))
    assert abs(np.mean(ratio) - 1.0) < 0.03, ratio


def test_native_host_passes_the_gate_under_energy(gpu_device):
    """examples/mcblock_amd with the deck key: stepdiff's gate (0.05), evaluated by the host itself; a bad value of
    the key ends it with the key named."""
    exe = os.path.join(ROOT, "examples", "mcblock_amd")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], check=True, capture_output=True)
    ov = ["parthenon/mesh/nx1=128", "parthenon/meshblock/nx1=64"]
    res = subprocess.run([exe, "-i", os.path.join(DECKS, "stepdiff.in"), "--tolerance", "0.05", ALLOC + "=energy"] + ov,
                         capture_output=True, text=True, timeout=280)
    assert res.returncode == 0 and "TEST PASSED" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    # (energy sources num_particles per call: the census holds the deck's 100000 photons, to the rounding of 64 cells)
    last = [ln for ln in res.stdout.splitlines() if ln.startswith("cycle=")][-1]
    photons = int(last.split("photons=")[1].split()[0])
    assert abs(photons - 100000) <= 128, last
    bad = subprocess.run([exe, "-i", os.path.join(DECKS, "stepdiff.in"), ALLOC + "=proportional"] + ov,
                         capture_output=True, text=True, timeout=280)
    assert bad.returncode != 0 and "source_allocation" in bad.stdout + bad.stderr


# ---- 8. errors ----------------------------------------------------------------------------------------------------
def test_error_paths(gpu_device, monkeypatch):
    from jaybenne_amd import _lib, jaybenne as jb
    deck, ov = _geometry("2d-smr")
    # jb_source_photons_count on a partial mesh: JB_ERR_INVALID that names the two-phase calls
    part = _driver(deck, dict(ov, **{NP: 2000}), gpu_device, rank=0, nranks=2)
    md = part.md
    md.source_allocation = "energy"
    nper = np.zeros(md.nblocks, dtype=np.int32)
    st = md.lib.jb_source_photons_count(md.pkg.ctx, md.handle, 0, 0.0, 1, 1, nper.ctypes.data, md.prefix.data_ptr())
    msg = md.lib.jb_last_error()
    assert st == _lib.JB_ERR_INVALID and b"jb_source_energy_sums" in msg and b"jb_source_photons_count_energy" in msg
    # the count pass without its energy pass, and with a total that is not finite
    e = np.zeros(md.nblocks)
    args = (md.pkg.ctx, md.handle, 0, 0.0, 1)
    assert md.lib.jb_source_photons_count_energy(*args, 1.0, nper.ctypes.data, md.prefix.data_ptr()) == _lib.JB_ERR_INVALID
    for bad in (math.inf, math.nan, -1.0):
        _lib.check(md.lib.jb_source_energy_sums(md.pkg.ctx, md.handle, 0, 0.0, e.ctypes.data))
        assert md.lib.jb_source_photons_count_energy(*args, bad, nper.ctypes.data, md.prefix.data_ptr()) == _lib.JB_ERR_INVALID
    # E_tot == 0 sources nothing and completes
    _lib.check(md.lib.jb_source_energy_sums(md.pkg.ctx, md.handle, 0, 0.0, e.ctypes.data))
    nper[:] = -1
    _lib.check(md.lib.jb_source_photons_count_energy(*args, 0.0, nper.ctypes.data, md.prefix.data_ptr()))
    assert not nper.any() and not _host(md, "src_num")[:md.nowned][part.mesh.interior()].any()
    assert not _host(md, "src_ew")[:md.nowned][part.mesh.interior()].any() and not md.prefix.cpu().numpy().any()
    # an N for which a block's count could pass 2^31 - 1 is rejected before any launch
    from jaybenne_amd import mcblock
    from jaybenne_amd.mesh import Mesh
    for n_ok in (True, False):
        pin = load_deck(deck, dict(ov, **{NP: 2 ** 31 - 1 - part.mesh.ncell + (0 if n_ok else 1)}))
        mcb = mcblock.Initialize(pin)
        pkg = jb.Initialize(pin, mcb.opacity, mcb.scattering, mcb.eos, device=gpu_device)
        mdb = jb.MeshData(pkg, Mesh.from_deck(pin), 1024)
        mdb.source_allocation = "energy"
        if n_ok:      # the largest target a block's count can hold passes the check (the fields are zero: E_tot = 0)
            eb = np.ones(mdb.nblocks)
            _lib.check(mdb.lib.jb_source_energy_sums(pkg.ctx, mdb.handle, 0, 0.0, eb.ctypes.data))
            assert not eb.any()
    mdb.source_allocation = "energy"
    mdb.fields["src_ew"].fill_(-3.0)
    nb = np.zeros(mdb.nblocks, dtype=np.int32)
    eb = np.zeros(mdb.nblocks)
    assert mdb.lib.jb_source_energy_sums(pkg.ctx, mdb.handle, 0, 0.0, eb.ctypes.data) == _lib.JB_ERR_INVALID
    assert b"2^31" in mdb.lib.jb_last_error()
    assert mdb.lib.jb_source_photons_count(pkg.ctx, mdb.handle, 0, 0.0, 1, 1, nb.ctypes.data,
                                           mdb.prefix.data_ptr()) == _lib.JB_ERR_INVALID
    assert bool((mdb.fields["src_ew"] == -3.0).all())                  # nothing was launched
    # jb_radiation_step_ranks is outside the mode
    monkeypatch.setenv("JB_HANDOFF", "step")
    d1, o1 = _geometry("1d-50")
    stp = _driver(d1, dict(o1, **hs.ABSORBING, **{NP: 1000, ALLOC: "energy"}), gpu_device, capacity_factor=4.0)
    assert stp.md.handoff == "step"
    n0 = stp.md.n
    with pytest.raises(_lib.JaybenneError) as exc:
        stp.Step()
    assert exc.value.status == _lib.JB_ERR_UNSUPPORTED and stp.md.n == n0


# ---- 9. the checked library ---------------------------------------------------------------------------------------
def test_checked_library_accepts_a_cycle(gpu_device, checked_lib):
    env = dict(os.environ, JAYBENNE_AMD_LIB=checked_lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "checked-stepdiff"], capture_output=True, text=True,
                         env=env, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    _clean(out["report"])
    assert out["allocation"] == "energy" and abs(out["n"] - 20000) <= 100


# ---- in the child process -------------------------------------------------------------------------------------------
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ["JB_EXACT_ARITH"] = "1"
    import torch
    assert sys.argv[1] == "checked-stepdiff"
    drv = _driver("stepdiff", {NP: 20000, ALLOC: "energy"}, torch.device("cuda", 0), state=None)
    assert drv.md.invariants_enabled()
    assert drv.Step() == drv.jb.TaskStatus.complete
    print(json.dumps({"report": drv.md.invariant_report(), "allocation": drv.md.source_allocation, "n": drv.md.n}))
