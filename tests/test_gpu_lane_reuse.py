"""Every tracking kernel with tens of photons per lane, against the CPU oracle.

A lane of k_transport, k_imc_cell, k_hybrid, k_ddmc_all or k_ddmc_q is persistent: it writes a finished history
back, claims the next slot and goes on, carrying whatever the refill did not set again (an absolute position, a
global block id, the per-lane cell geometry, the held mean free paths, a run-mask bit, a parked or virtual lane's
budget, a queue entry in LDS).  The other parity suites launch at least as many lanes as they have photons, so a
lane takes a second photon only by accident of timing.  Here ``JB_TRANSPORT_MAX_BLOCKS`` caps every persistent launch
at G = 1 or 3 workgroups, so the rows of tests/lane_reuse_cases.py put 8 .. 117 photons through every lane behind
predecessors that escaped, were absorbed, changed level or changed regime (tests/test_lane_reuse_host.py holds the
counts on the CPU).  With one workgroup a wave walks through all eight particle queues; with three the queues are
entered from three starts and ``QueueCursor::next`` wraps.

Every test first checks that it ran what it says: ``jb_last_transport_grid`` == G, the kernel
``jb_last_transport_variant`` names, and enough photons in the swarm before the call.  Then

* exact arithmetic: photons bit for bit by creation id, fields to 1e-12, events and the four outcome counters equal
  to the oracle's;
* lean arithmetic: the project's tolerance against the oracle (1e-9 after one cycle), and -- the sharp check -- every
  photon attribute bit-identical to the same lean run on the default grid, events equal, tally and energy_delta
  within 1e-12: a photon's arithmetic depends on its own stream and its cells' data only, so any difference is
  state that leaked from a lane's earlier photon.  (The default-grid run is held to the oracle by
  tests/test_gpu_axes.py.)

Wall time on the MI355X (pytest's ``--durations``, the whole file 16 s for 62 tests): every exact, lean, budget and
grid case 0.01 .. 0.45 s (the slowest: G3S-hybrid with budgets of 2^20, 0.44 s; the G3S-hybrid and G3S-imc lean cases,
which run the default grid too, 0.3 .. 0.4 s; one workgroup follows the 1.0e7 events of G2O-hybrid in 0.15 s); the
two-rank run 2.9 s; the child under the checked library 2.5 s.  No row's photon count had to be lowered.
"""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import axis_cases as ax
import hetero_states as hs
import lane_reuse_cases as lr
from helpers import load_deck, run_oracle_cycles
from test_gpu_axes import _case_pair
from test_gpu_hetero import _compare_lean, _steps, _variant
from test_gpu_invariants import CHECKED, ROOT, TESTS, _clean, checked_lib  # noqa: F401  (checked_lib: fixture)
from test_gpu_parity import _compare_fields, _compare_swarm_by_id

pytestmark = pytest.mark.gpu

KNOB = "JB_TRANSPORT_MAX_BLOCKS"
COUNTERS = ("n_census", "n_absorbed", "n_escaped", "n_outgoing")
FIELDS = ("tally", "edelta", "fleck", "src_num", "src_ew")
SWITCHES = ("JB_COOP_GATHER", "JB_DDMC_QUEUES", "JB_DDMC_LDS_CODES", "JB_NO_IMC_CELL", "JB_NO_DDMC_ALL",
            "JB_PER_EVENT_OPACITY", "JB_NO_EXACT_GEOM", "JB_HYBRID_IMC_BUDGET", "JB_HYBRID_PARK_BUDGET",
            "JB_TRANSPORT_BLOCKS_PER_CU", KNOB)


def _grid(drv):
    return drv.md.lib.jb_last_transport_grid(drv.md.handle)


def _run(cid, pattern, device, monkeypatch, G, env=None):
    """One cycle of a row on the device under ``env`` and the cap G (None: the knob unset), and on the oracle with
    ``watch`` on its transport call.  The switches are read when the driver is made."""
    row = lr.BY_ID[cid]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if G is not None:
        monkeypatch.setenv(KNOB, str(G))
    pin, drv, O, mesh, pkg = _case_pair(lr.case_of(row), row.bset, device, pattern=pattern or row.patterns[0],
                                        capacity_factor=row.capacity_factor)
    assert _grid(drv) == 0                                   # no transport call yet
    if G is not None:
        assert drv.md.n >= lr.reuse_floor(G), (drv.md.n, G)  # at least 8 (G = 1) or 4 (G = 3) photons per lane
    log = lr.watch(O)
    _steps(drv, O, pin, 1)
    if G is not None:
        assert _grid(drv) == G, _grid(drv)
    return types.SimpleNamespace(pin=pin, drv=drv, O=O, mesh=mesh, pkg=pkg, log=log, variant=_variant(drv))


def _emitted(O, mesh):
    """The energy a cell emitted: what energy_delta = absorbed - emitted is measured against where it cancels."""
    sl = mesh.interior()
    with np.errstate(invalid="ignore"):
        return np.where(O.fields["src_num"][sl] > 0, O.fields["src_num"][sl] * O.fields["src_ew"][sl], 0.0)


def _equals_the_oracle(r):
    """Photons bit for bit by creation id, fields to 1e-12, events and the four outcome counters."""
    drv, O = r.drv, r.O
    _compare_swarm_by_id(drv.md, O)
    _compare_fields(drv.md, O, tuple(k for k in FIELDS if k != "edelta"))
    _compare_fields(drv.md, O, ("edelta",), scale=_emitted(O, r.mesh))
    assert drv.md.events == O.events
    want = lr.outcomes(r.log)
    got = drv.md.stats()
    assert {k: got[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}
    assert want["n_escaped"] + want["n_absorbed"] >= lr.FLOOR and want["n_census"] >= lr.FLOOR


def _as_reference(drv):
    """A finished device run in the shape the comparison helpers take the oracle in."""
    g = drv.md.get_swarm()
    return types.SimpleNamespace(sw=g, n=drv.md.n, events=drv.md.events, status=g["status"],
                                 fields={k: drv.md.get_field(k) for k in FIELDS},
                                 stats={k: drv.md.stats()[k] for k in COUNTERS})


_DEFAULT_GRID = {}


def _default_grid_run(cid, pattern, device, monkeypatch, env=None):
    """The lean run of a row with the knob unset (and the hybrid budgets at their defaults): computed once."""
    key = (cid, pattern, tuple(sorted((env or {}).items())))
    if key not in _DEFAULT_GRID:
        r = _run(cid, pattern, device, monkeypatch, None, env)
        assert _grid(r.drv) > 3, _grid(r.drv)                # really another grid: one lane per photon or the chip's fill
        _DEFAULT_GRID[key] = (_as_reference(r.drv), r.variant)
    return _DEFAULT_GRID[key]


def _same_bits(r, ref):
    """The sharp check: every photon attribute bit-identical by creation id, events and counters equal, tally and
    energy_delta within 1e-12 (the order of the atomic additions into a cell differs between the grids)."""
    drv = r.drv
    _compare_swarm_by_id(drv.md, ref)
    g = drv.md.get_swarm()
    assert np.array_equal(g["status"][np.argsort(g["id"])], ref.status[np.argsort(ref.sw["id"])])
    assert drv.md.events == ref.events
    assert {k: drv.md.stats()[k] for k in COUNTERS} == ref.stats
    _compare_fields(drv.md, ref, ("tally", "fleck", "src_num", "src_ew"))
    sl = r.mesh.interior()
    with np.errstate(invalid="ignore"):
        emitted = np.where(ref.fields["src_num"][sl] > 0, ref.fields["src_num"][sl] * ref.fields["src_ew"][sl], 0.0)
    _compare_fields(drv.md, ref, ("edelta",), scale=emitted)


def _lean_checks(r, ref, ref_variant):
    assert r.drv.pkg.arithmetic() == "lean" and ref_variant == r.variant
    assert r.drv.md.stats()["n_escaped"] >= lr.FLOOR
    _compare_lean(r.drv, r.O, r.mesh, r.pin, 1, by_id=True)
    _same_bits(r, ref)


# ---- a. exact arithmetic against the oracle ----------------------------------------------------
# (row, pattern (None: the row's first), switches, what the variant must say, grids)
def _tr(nd, gray, exact):
    return lambda v: v == f"k_transport<{nd}, true, {gray}, {'true' if exact else 'false'}, false>"


def _has(*parts):
    return lambda v: all(p in v for p in parts)


Q, QG = {"JB_DDMC_QUEUES": "1", "JB_DDMC_LDS_CODES": "1"}, {"JB_DDMC_QUEUES": "1", "JB_DDMC_LDS_CODES": "0"}
EXACT = [
    # k_transport, exact geometry: 1-D, per-lane geometry in 2-D and 3-D, one level, absorption
    ("G1-imc", None, {}, _tr(1, 2, True), (1, 3)),
    ("G2S-imc", None, {}, _tr(2, 2, True), (1,)),
    ("G3U-imc", None, {}, _tr(3, 2, True), (1,)),
    ("G3S-imc", None, {}, _tr(3, 2, True), (1, 3)),
    ("G3S-hot", None, {}, _tr(3, 1, True), (1, 3)),
    # ... general geometry, by its widths and by the switch; per-event opacities on the hybrid deck
    ("G3O-imc", None, {}, _tr(3, 2, False), (1,)),
    ("G3U-imc", None, {"JB_NO_EXACT_GEOM": "1", "JB_NO_IMC_CELL": "1"}, _tr(3, 2, False), (1,)),
    ("G2S-hybrid", None, {"JB_PER_EVENT_OPACITY": "1"}, _has("k_transport<2, true, 0,"), (1,)),
    # k_ddmc_q: records and codes in LDS (1-D), codes gathered; k_ddmc_all: records in LDS, forced codes
    ("G1-ddmc", None, Q, _has("cell codes, queues, codes in LDS"), (1, 3)),
    ("G1-ddmc", None, QG, lambda v: v.endswith("cell codes, queues>"), (1,)),
    ("G1-ddmc", None, {"JB_DDMC_QUEUES": "0"}, _has("k_ddmc_all<1, true, records in LDS>"), (1,)),
    ("G1-ddmc", None, {"JB_COOP_GATHER": "4"}, lambda v: v.endswith("cell codes>"), (1,)),
    ("G2S-ddmc", None, Q, lambda v: v.endswith("cell codes, queues>"), (1,)),
    ("G2S-ddmc", None, {"JB_COOP_GATHER": "4"}, lambda v: v.endswith("cell codes>"), (1,)),
    ("G2S-ddmc", "smooth_dense", {"JB_COOP_GATHER": "0"}, _has("k_ddmc_all<2, true>"), (1, 3)),
    ("G2S-ddmc", "smooth_dense", {"JB_COOP_GATHER": "1"}, _has("k_ddmc_all<2, true, quad gather>"), (1,)),
    ("G2S-ddmc", "smooth_dense", {"JB_COOP_GATHER": "2"}, _has("k_ddmc_all<2, true, quad gather>"), (1,)),
    ("G3S-ddmc", None, Q, lambda v: v.endswith("cell codes, queues>"), (1, 3)),
    ("G3S-ddmc", None, QG, lambda v: v.endswith("cell codes, queues>"), (1,)),
    ("G3S-ddmc", None, {"JB_DDMC_QUEUES": "0"}, lambda v: v.endswith("k_ddmc_all<3, true, cell codes>"), (1,)),
    ("G3S-ddmc", "smooth_dense", {"JB_COOP_GATHER": "0"}, _has("k_ddmc_all<3, true>"), (1,)),
    ("G3S-ddmc", "smooth_dense", {"JB_COOP_GATHER": "1"}, _has("k_ddmc_all<3, true, quad gather>"), (1,)),
    ("G3S-ddmc", "smooth_dense", {"JB_COOP_GATHER": "2"}, _has("k_ddmc_all<3, true, quad gather>"), (1,)),
    ("G3S-ddmc", "smooth_dense", {}, lambda v: "k_ddmc_all<3, true" in v and "cell codes" not in v, (1,)),
    ("G3S-ddmc", "smooth_dense", {"JB_NO_DDMC_ALL": "1"}, _has("k_hybrid<3, exact>"), (1,)),
    # k_hybrid, exact arithmetic: exact and general geometry
    ("G2S-hybrid", None, {}, _has("k_hybrid<2, exact>"), (1, 3)),
    ("G3S-hybrid", None, {}, _has("k_hybrid<3, exact>"), (1, 3)),
    ("G2O-hybrid", None, {}, _has("k_hybrid<2, exact>"), (1,)),
]
EXACT_RUNS = [pytest.param(c, p, e, w, G, id="-".join([c, lr.BY_ID[c].bset, p or lr.BY_ID[c].patterns[0]] +
                                                      [f"{k[3:].lower()}={v}" for k, v in e.items()] + [f"G{G}"]))
              for c, p, e, w, grids in EXACT for G in grids]


@pytest.mark.parametrize("cid,pattern,env,want,G", EXACT_RUNS)
def test_exact_arithmetic_with_many_photons_per_lane(gpu_device, monkeypatch, cid, pattern, env, want, G):
    r = _run(cid, pattern, gpu_device, monkeypatch, G, env)
    assert r.drv.pkg.arithmetic() == "exact"
    assert want(r.variant), r.variant
    if "JB_PER_EVENT_OPACITY" not in env:
        exact_geom = ax.GEOMETRIES[lr.case_of(lr.BY_ID[cid]).geom].exact and "JB_NO_EXACT_GEOM" not in env
        assert r.drv.md.lib.jb_mesh_exact_geometry(r.drv.md.handle) == int(exact_geom)
    _equals_the_oracle(r)


# ---- b. the lean kernels, one workgroup --------------------------------------------------------
X = {"JB_NO_IMC_CELL": "1"}
LEAN = [
    # k_imc_cell<NDIM, TALLY, NOABS>: UNIFORM on one level, per-lane geometry on two; with absorption; on general
    # geometry (the cell-local step does not care what the widths are)
    ("G1-imc", {}, "k_imc_cell<1, true, true, lean>", True),
    ("G2S-imc", {}, "k_imc_cell<2, true, true, lean>", False),
    ("G3U-imc", {}, "k_imc_cell<3, true, true, lean>", True),
    ("G3S-imc", {}, "k_imc_cell<3, true, true, lean>", False),
    ("G3S-hot", {}, "k_imc_cell<3, true, false, lean>", False),
    ("G3O-imc", {}, "k_imc_cell<3, true, true, lean>", None),    # (widths 1 / 24 ..: the blocks' differ in the last place)
    # the lean step in the swarm's coordinates: exact and general geometry
    ("G3S-imc", X, "k_transport<3, true, 2, true, true>", None),
    ("G3O-imc", X, "k_transport<3, true, 2, false, true>", None),
    # k_hybrid, lean: cell-local on exact geometry, in the swarm's coordinates with the switch and on general geometry
    ("G2S-hybrid", {}, "k_hybrid<2, lean, cell-local>", None),
    ("G3S-hybrid", {}, "k_hybrid<3, lean, cell-local>", None),
    ("G3S-hybrid", X, "k_hybrid<3, lean, exact geometry>", None),
    ("G2O-hybrid", {}, "k_hybrid<2, lean>", None),
]


@pytest.mark.lean
@pytest.mark.parametrize("cid,env,want,uniform", LEAN,
                         ids=["-".join([c, lr.BY_ID[c].bset] + (["x-space"] if e else [])) for c, e, _, _ in LEAN])
def test_lean_kernels_with_many_photons_per_lane(gpu_device, monkeypatch, cid, env, want, uniform):
    ref, ref_variant = _default_grid_run(cid, None, gpu_device, monkeypatch, env)
    r = _run(cid, None, gpu_device, monkeypatch, 1, env)
    assert r.variant == want, r.variant
    if uniform is not None:      # the library's condition for k_imc_cell<.., UNIFORM>: every block has block 0's widths
        assert bool(np.all(r.mesh.blk_dx == r.mesh.blk_dx[0])) == uniform
    if cid == ax.HOT_CASE.id:
        assert r.drv.md.stats()["n_absorbed"] >= lr.FLOOR
    _lean_checks(r, ref, ref_variant)


# ---- c. the hybrid kernel's scheduling budgets -------------------------------------------------
BUDGETS = [pytest.param(c, a, b, marks=[pytest.mark.lean] if a == "lean" else [], id=f"{c}-{a}-{b}")
           for c in ("G2S-hybrid", "G3S-hybrid") for a in ("exact", "lean") for b in (1, 1048576)]


@pytest.mark.parametrize("cid,arith,budget", BUDGETS)
def test_hybrid_budgets_never_change_results(gpu_device, monkeypatch, cid, arith, budget):
    """JB_HYBRID_IMC_BUDGET and JB_HYBRID_PARK_BUDGET are tuning aids: how many passes a wave spends in its IMC
    loop, and how many parked lanes it lets collect, before it turns to the other loop.  Both extremes end by
    construction, as the kernel reads: its IMC and DDMC loops run ``while (nrun >= thresh)`` with ``thresh`` = 1
    until a budget raises it to 65 (no ballot has 65 lanes, so the loop is left), and the DDMC loop is entered when
    ``n_imc == 0`` whatever the park budget -- a budget of 1 leaves a loop after every pass, one of 2^20 never does
    before the loop has run dry.  One workgroup; exact arithmetic equals the oracle bit for bit, lean arithmetic the
    lean run on the default grid with the default budgets."""
    env = {"JB_HYBRID_IMC_BUDGET": str(budget), "JB_HYBRID_PARK_BUDGET": str(budget)}
    if arith == "lean":
        ref, ref_variant = _default_grid_run(cid, None, gpu_device, monkeypatch, {})
    r = _run(cid, None, gpu_device, monkeypatch, 1, env)
    assert r.drv.pkg.arithmetic() == arith
    assert r.variant == f"k_hybrid<{r.mesh.ndim}, " + ("exact>" if arith == "exact" else "lean, cell-local>"), r.variant
    if arith == "exact":
        _equals_the_oracle(r)
    else:
        _lean_checks(r, ref, ref_variant)


# ---- d. a lane that last held a photon on its way to another rank ------------------------------
def _rank_worker(rank, world, port, outdir):
    """As test_gpu_axes._rank_worker, and: one workgroup, enough photons for it, photons handed over."""
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_HANDOFF="step")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import mcblock
        from jaybenne_amd.comm import Comm
        row = lr.RANK_ROW
        case = lr.case_of(row)
        ov = ax.overrides(case, row.bset)
        drv = mcblock.McblockDriver(load_deck(case.deck, ov), rank=rank, nranks=world, comm=Comm(),
                                    device=torch.device("cuda", 0), capacity_factor=row.capacity_factor,
                                    decomposition="blocks", initial_state=hs.state_for(case.deck, ov, row.patterns[0]))
        assert os.environ[KNOB] == "1" and drv.md.n >= lr.reuse_floor(1), drv.md.n
        drv.Step()
        assert drv.md.handoff_path().startswith("c: jb_radiation_step_ranks"), drv.md.handoff_path()
        assert drv.md.lib.jb_last_transport_grid(drv.md.handle) == 1
        assert _variant(drv) == "k_hybrid<3, exact>", _variant(drv)
        assert drv.md.stats()["n_outgoing"] >= lr.FLOOR, drv.md.stats()
        g = drv.md.get_swarm()
        g["gblk"] = drv.md.gids[g["blk"]]
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), tally=drv.md.get_field("tally"), gids=drv.md.gids,
                 events=np.array([drv.md.events]), **g)
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_one_workgroup_each(gpu_device, monkeypatch, tmp_path):
    """G3S-hybrid S1 dealt to two ranks by blocks, the step in the library: a lane's previous photon may have left
    for the other rank (a global block id in the lane's block register).  The union of the ranks' swarms is the
    oracle's, bit for bit."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, TESTS)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(KNOB, "1")                                        # (the workers inherit the environment)
    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_rank_worker, args=(r, world, port, str(tmp_path))) for r in range(world)])
    row = lr.RANK_ROW
    case = lr.case_of(row)
    ov = ax.overrides(case, row.bset)
    pin = load_deck(case.deck, ov)
    O, mesh, _ = hs.oracle_on(case.deck, ov, row.patterns[0])
    n0 = O.n
    run_oracle_cycles(O, pin, 1)
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    ids = np.concatenate([p["id"] for p in parts])
    order = np.argsort(ids)
    oo = np.argsort(O.sw["id"][:O.n])
    assert len(ids) == O.n < n0 and np.array_equal(ids[order], O.sw["id"][:O.n][oo])
    for k in ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e", "ip", "jp", "kp", "rng"):
        assert np.array_equal(np.concatenate([p[k] for p in parts])[order], O.sw[k][:O.n][oo]), k
    assert np.array_equal(np.concatenate([p["gblk"] for p in parts])[order], O.sw["blk"][:O.n][oo])
    sl = mesh.interior()
    for p in parts:
        np.testing.assert_allclose(p["tally"][sl], O.fields["tally"][p["gids"]][sl], rtol=1e-12, atol=0)
    assert sum(int(p["events"][0]) for p in parts) == O.events


# ---- e. under the checked library --------------------------------------------------------------
def child_case():
    """G3S-imc S3, lean, one workgroup: the invariants of k_imc_cell (position inside the cell, the offset names an
    interior cell, no collision in the step that left the block) on every pass of every lane that is used again."""
    import torch
    mp = pytest.MonkeyPatch()
    try:
        r = _run("G3S-imc", None, torch.device("cuda", 0), mp, 1, {})
        _compare_lean(r.drv, r.O, r.mesh, r.pin, 1, by_id=True)
        assert r.drv.md.invariants_enabled()
        rep = r.drv.md.invariant_report()
        rep["variant"] = r.variant
        rep["grid"] = _grid(r.drv)
        return rep
    finally:
        mp.undo()


@pytest.mark.lean
@pytest.mark.timeout(900, method="thread")
def test_checked_library_with_many_photons_per_lane(gpu_device, checked_lib):
    e = dict(os.environ, JAYBENNE_AMD_LIB=CHECKED)
    for k in SWITCHES:
        e.pop(k, None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=e,
                         timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    rep = json.loads(res.stdout.strip().splitlines()[-1])
    _clean(rep)
    assert rep["grid"] == 1 and rep["variant"] == "k_imc_cell<3, true, true, lean>", rep
    assert rep["passes"]["imc_cell"] > 0, rep
    assert rep["evaluated"]["INDEX"] >= rep["passes"]["imc_cell"], rep


# ---- f. the knob unset -------------------------------------------------------------------------
@pytest.mark.parametrize("knob", [None, "0", "-3", "1000000"])
def test_grid_without_the_knob_is_the_launch_policy(gpu_device, monkeypatch, knob):
    """``jb_last_transport_grid`` with the knob unset, or set to something that is no cap (<= 0, above the policy's
    grid): min(ceil(n / 256), compute units x workgroups per unit) under JB_TRANSPORT_BLOCKS_PER_CU=2, on a swarm
    that does not fill the chip and on one that does (G1-ddmc: one persistent launch over the swarm, then the eight
    workgroups of the hand-over launch)."""
    import torch
    from jaybenne_amd import mcblock
    num_cu = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    row = lr.BY_ID["G1-ddmc"]
    case = lr.case_of(row)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JB_TRANSPORT_BLOCKS_PER_CU", "2")
    if knob is not None:
        monkeypatch.setenv(KNOB, knob)
    grids = []
    for photons in (20000, 2 * num_cu * lr.BLOCK + 20000):
        ov = dict(ax.overrides(case, row.bset), **{ax.NP: photons})
        drv = mcblock.McblockDriver(load_deck(case.deck, ov), device=gpu_device,
                                    initial_state=hs.state_for(case.deck, ov, row.patterns[0]))
        n = drv.md.n                                         # (no emission on this deck: the swarm of the transport call)
        assert abs(n - photons) < 100
        drv.Step()
        assert "k_ddmc_all<1" in _variant(drv)
        assert _grid(drv) == min(-(-n // lr.BLOCK), 2 * num_cu), (_grid(drv), n, num_cu)
        grids.append(_grid(drv))
    assert 8 < grids[0] < grids[1] == 2 * num_cu


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    print(json.dumps(child_case()))
