"""The census comb (include/jaybenne_amd.h: jb_comb_census_plan / jb_comb_census_apply) on the GPU.  Expected values
come from tests/comb_model.py -- the rule restated in numpy over the CPU oracle's generator -- and from math.fsum,
never from the library.  Synthetic swarms first, on the smallest shapes where the kernels can go wrong (empty cells,
cells of 1, T and T + 1 photons, a cell longer than three scan tiles, combed cells at the first and the last key);
then whole runs."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import comb_model as cm
from helpers import load_deck, make_oracle, run_oracle_cycles

from test_gpu_invariants import checked_lib  # noqa: E402,F401  (fixture: the checked library, built once)

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048          # kScanTile of jb_kernels.hpp: 256 threads x 8 slots
T_SYN = 70                # more than a wave: a cell of T + 1 straddles a wave boundary wherever it starts
EPOCH, ID_BASE = 5, 1 << 33
MESHES = {
    "1d": ("stepdiff", {"parthenon/mesh/nx1": 16, "parthenon/meshblock/nx1": 8, "jaybenne/num_particles": 64}),
    "3d": ("inf", {"parthenon/meshblock/nx1": 2, "parthenon/meshblock/nx2": 2, "parthenon/meshblock/nx3": 2,
                   "jaybenne/num_particles": 64}),
}


def _hash(i, salt):
    x = (np.asarray(i).astype(np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    return x


def _unit(i, salt):
    return ((_hash(i, salt) >> np.uint64(11)) % np.uint64(1 << 20)).astype(np.float64) / float(1 << 20)


def _driver(name, device, **kw):
    from jaybenne_amd import mcblock
    deck, ov = MESHES[name]
    return mcblock.McblockDriver(load_deck(deck, ov), device=device, **kw)


def _layout(ncells):
    """photons per interior cell (cells numbered block by block) and the cells with a special weight pattern"""
    pattern = [0, 1, T_SYN, 0, 5, SCAN_TILE + 52, 0, 64, 3, 129]
    per = [pattern[c % len(pattern)] for c in range(ncells)]
    per[0] = T_SYN + 1                     # a combed cell at the first key
    per[1], per[2], per[3] = 0, 1, T_SYN
    per[4] = 3 * SCAN_TILE + 5             # spans four tiles
    per[5] = 0
    per[6] = 300                           # all weights equal
    per[7] = 200                           # one photon holds 99.9 % of W
    per[ncells - 2] = 0
    per[ncells - 1] = 500                  # a combed cell at the last key
    return per, 6, 7


def _synthetic(mesh, salt):
    """The swarm: the layout's photons at hashed positions inside their cells, 37 slots that are not ACTIVE mixed in,
    all in a hashed slot order; weights over 1e-17 .. 1e7."""
    nx = [int(v) for v in mesh.nx]
    ncell = nx[0] * nx[1] * nx[2]
    per, equal, dominant = _layout(mesh.nblocks * ncell)
    cell_of = np.repeat(np.arange(len(per)), per)
    n_act = len(cell_of)
    n = n_act + 37
    cell_of = np.concatenate([cell_of, _hash(np.arange(37), salt + 9) % np.uint64(len(per))]).astype(np.int64)
    i = np.arange(n)
    blk = cell_of // ncell
    c = cell_of % ncell
    ijk = [c % nx[0], (c // nx[0]) % nx[1], c // (nx[0] * nx[1])]
    sw = {}
    for d, name in enumerate(("x", "y", "z")):
        if d < mesh.ndim:
            sw[name] = mesh.blk_xmin[blk, d] + (ijk[d] + 0.05 + 0.9 * _unit(i, salt + 31 + d)) * mesh.blk_dx[blk, d]
        else:
            sw[name] = np.zeros(n)
    for q, name in enumerate(("vx", "vy", "vz", "t", "e")):
        sw[name] = _unit(i, salt + 50 + q) - 0.5
    w = 10.0 ** (-17.0 + 24.0 * _unit(i, salt + 70))
    w[cell_of == equal] = 0.37
    dom = np.flatnonzero(cell_of[:n_act] == dominant)
    w[dom] = 1.0
    w[dom[17]] = 999.0 * (len(dom) - 1)
    sw["w"] = w
    ng = mesh.ng
    sw["ip"] = (ijk[0] + ng).astype(np.int32)
    sw["jp"] = (ijk[1] + (ng if mesh.ndim >= 2 else 0)).astype(np.int32)
    sw["kp"] = (ijk[2] + (ng if mesh.ndim >= 3 else 0)).astype(np.int32)
    sw["blk"] = blk.astype(np.int32)
    status = np.zeros(n, dtype=np.int32)
    status[n_act:] = 1 + (np.arange(37) % 2)            # ABSORBED / ESCAPED
    sw["status"] = status
    sw["id"] = (i + 1000).astype(np.uint64)
    sw["rng"] = _hash(i, salt + 99)
    order = np.argsort(_hash(i, salt + 123))
    return {k: np.ascontiguousarray(v[order]) for k, v in sw.items()}, per


def _upload(md, sw, device):
    import torch
    n = len(sw["w"])
    md.reserve(n)
    for k, v in sw.items():
        md.swarm[k][:n] = torch.from_numpy(v.view(np.int64) if k in ("id", "rng") else v).to(device)
    md.sv.n = n
    torch.cuda.synchronize(device)


def _plan(md, T, K, epoch=EPOCH):
    from jaybenne_amd import _lib
    md._sync_stream()
    plan = _lib.CombPlan()
    st = md.lib.jb_comb_census_plan(md.pkg.ctx, md.handle, C.byref(md.sv), T, K, epoch, C.byref(plan))
    return st, plan


def _apply(md, id_base=ID_BASE):
    from jaybenne_amd import _lib
    rep = _lib.CombReport()
    st = md.lib.jb_comb_census_apply(md.pkg.ctx, md.handle, C.byref(md.sv), id_base, C.byref(rep))
    return st, rep


def _same(a, b, names=cm.SWARM_KEYS):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in names)


def _by_id(sw):
    o = np.argsort(sw["id"])
    return {k: v[o] for k, v in sw.items()}


@pytest.mark.parametrize("K", [1, T_SYN], ids=["K=1", "K=T"])
@pytest.mark.parametrize("name", ["1d", "3d"])
def test_comb_on_synthetic_swarms(gpu_device, name, K):
    from jaybenne_amd import _lib
    drv = _driver(name, gpu_device)
    md, mesh = drv.md, drv.mesh
    seed = int(drv.pin.GetOrAddInteger("jaybenne", "seed", 123))
    T = T_SYN
    sw, per = _synthetic(mesh, salt=17)
    n = len(sw["w"])
    _upload(md, sw, gpu_device)

    # ---- the plan: sorts, decides, changes nothing a photon carries
    st, plan = _plan(md, T, K)
    assert st == _lib.JB_COMPLETE, md.lib.jb_last_error()
    assert plan.sorted == 1 and plan.n_before == n == md.n
    g0 = md.get_swarm()
    assert _same(_by_id(g0), _by_id(sw))
    want, info = cm.comb_swarm(mesh, md.resident_gids, g0, n, T, K, seed, EPOCH, ID_BASE, sort=False)
    combed_cells = [c for c, m in enumerate(per) if m > T]
    assert info["cells_combed"] == len(combed_cells) >= 6 and info["max_per_cell"] == 3 * SCAN_TILE + 5
    assert (plan.n_after, plan.n_new_ids, plan.cells_combed, plan.max_per_cell) == \
        (n - sum(per[c] - K for c in combed_cells), info["n_new_ids"], len(combed_cells), info["max_per_cell"])
    act = g0["status"] == cm.ST_ACTIVE
    assert abs(plan.e_before - math.fsum(g0["w"][act])) <= 1e-13 * math.fsum(g0["w"][act])
    if K == 1:
        assert plan.n_new_ids == 0
    else:
        assert plan.n_new_ids > 0

    # ---- the move
    st, rep = _apply(md)
    assert st == _lib.JB_COMPLETE, md.lib.jb_last_error()
    assert (rep.n_after, rep.n_new_ids) == (plan.n_after, plan.n_new_ids) and md.n == plan.n_after
    g1 = md.get_swarm()
    act1 = g1["status"] == cm.ST_ACTIVE
    assert abs(rep.e_after - math.fsum(g1["w"][act1])) <= 1e-13 * math.fsum(g1["w"][act1])
    key0, _, nkeys, _ = cm.cell_keys(mesh, md.resident_gids, g0, n)
    key1, _, _, _ = cm.cell_keys(mesh, md.resident_gids, g1, md.n)
    assert np.all(np.diff(key1) >= 0)                       # still in (block, cell) order, the others behind
    in_id = {int(v): q for q, v in enumerate(g0["id"])}
    is_new = g1["id"] >= np.uint64(ID_BASE)
    # the original of every output slot: itself by id, or (a further copy) that of the first copy before it
    first_slot = np.maximum.accumulate(np.where(is_new, -1, np.arange(md.n)))
    assert first_slot.min() >= 0
    origin = np.array([in_id[int(v)] for v in g1["id"][first_slot]])
    carried = [k for k in cm.SWARM_KEYS if k not in ("w", "id", "rng")]
    assert _same({k: g1[k] for k in carried}, {k: g0[k][origin] for k in carried}, carried)
    assert _same({k: g1[k][~is_new] for k in ("id", "rng")}, {k: g0[k][origin][~is_new] for k in ("id", "rng")},
                 ("id", "rng"))                              # first copies keep id and stream state
    new_ids = g1["id"][is_new]
    assert np.array_equal(new_ids, np.uint64(ID_BASE) + np.arange(plan.n_new_ids, dtype=np.uint64))   # slot order
    for q in np.flatnonzero(is_new):
        state = C.c_uint64(0)
        _lib.check(md.lib.jb_debug_stream_start(md.pkg.ctx, seed, int(g1["id"][q]), C.byref(state)))
        assert int(g1["rng"][q]) == state.value
    # per cell: count, energy, and the cells that are not combed bit for bit
    skipped = 0
    got_k = np.bincount(origin, minlength=n)
    want_key, _, _, _ = cm.cell_keys(mesh, md.resident_gids, want, info["n_after"])
    for k in np.unique(key0):
        sel0, sel1 = key0 == k, key1 == k
        m = int(sel0.sum())
        if k == nkeys or m <= T:
            assert int(sel1.sum()) == m
            assert _same(_by_id({q: g1[q][sel1] for q in cm.SWARM_KEYS}), _by_id({q: g0[q][sel0] for q in cm.SWARM_KEYS}))
            continue
        assert int(sel1.sum()) == K
        e_in = math.fsum(g0["w"][sel0])
        assert abs(math.fsum(g1["w"][sel1]) - e_in) <= 1e-13 * e_in
        assert len(set(g1["w"][sel1].tolist())) == 1
        # k_j against the model, unless the last bit of a running sum decides one
        if info["margins"][int(k)] < 1e-9:
            skipped += 1
            continue
        assert np.array_equal(got_k[sel0], info["counts"][sel0]), int(k)
        # (W by two orders of summation: each within m eps of the exact sum, 7e-13 at m = 6149 in the worst case and
        # far less for these weights; the bound the per-cell energy is held to above)
        assert np.allclose(g1["w"][sel1], want["w"][want_key == k], rtol=1e-13, atol=0)
        assert _same({q: g1[q][sel1] for q in carried}, {q: want[q][want_key == k] for q in carried}, carried)
    assert skipped <= 0.01 * len(combed_cells)
    if skipped == 0:      # then the whole output is the model's, new ids and their streams included
        assert _same(g1, want, [q for q in cm.SWARM_KEYS if q != "w"])

    # ---- the same sorted swarm, twice: the same bits (and those of the first run, which sorted into this order)
    runs = []
    for _ in range(2):
        _upload(md, g0, gpu_device)
        st, p2 = _plan(md, T, K)
        assert st == _lib.JB_COMPLETE and p2.sorted == 0
        assert bytes(p2)[:48] == bytes(plan)[:48]
        st, r2 = _apply(md)
        assert st == _lib.JB_COMPLETE and bytes(r2) == bytes(rep)
        runs.append(md.get_swarm())
    assert _same(runs[0], runs[1]) and _same(runs[0], g1)


def test_nothing_to_comb_and_argument_errors(gpu_device):
    from jaybenne_amd import _lib
    drv = _driver("1d", gpu_device)
    md, mesh = drv.md, drv.mesh
    sw, per = _synthetic(mesh, salt=3)
    n = len(sw["w"])
    _upload(md, sw, gpu_device)
    # apply without a plan
    st, _ = _apply(md)
    assert st == _lib.JB_ERR_INVALID and b"no plan" in md.lib.jb_last_error()
    for T, K, epoch in ((10, 0, 1), (10, 11, 1), (10, -3, 1), (10, 5, 1 << 20), (1 << 32, 5, 1)):
        st, _ = _plan(md, T, K, epoch)
        assert st == _lib.JB_ERR_INVALID, (T, K, epoch)
        assert _apply(md)[0] == _lib.JB_ERR_INVALID          # a failed plan is no plan
    assert md.n == n
    # no cell above the trigger: the plan says so, the swarm (sorted now) holds the same photons
    st, plan = _plan(md, max(per), max(per))
    assert st == _lib.JB_COMPLETE
    assert (plan.n_after, plan.n_new_ids, plan.cells_combed, plan.max_per_cell) == (n, 0, 0, max(per))
    assert _same(_by_id(md.get_swarm()), _by_id(sw))
    # a plan made for another swarm length does not apply
    md.sv.n = n - 1
    assert _apply(md)[0] == _lib.JB_ERR_INVALID
    md.sv.n = n
    # an empty swarm
    md.sv.n = 0
    st, plan = _plan(md, 4, 2)
    assert st == _lib.JB_COMPLETE and (plan.n_before, plan.n_after, plan.cells_combed) == (0, 0, 0)


# ---- whole runs ---------------------------------------------------------------------------------
INF_K, INF_T, INF_CYCLES = 32, 64, 40
# (inf.in sources num_particles per cycle into 64 cells and absorbs 3 % of the census per cycle: at the deck's 200
# the first cell passes 64 photons after some twenty cycles; at 2000 the comb works from the second cycle on)
INF = {"jaybenne/num_particles": 2000, "jaybenne_amd/census_per_cell_max": INF_K, "jaybenne_amd/ledger": "true"}


@pytest.mark.lean
def test_inf_census_stays_bounded(gpu_device):
    from jaybenne_amd import jaybenne as jb, mcblock
    drv = mcblock.McblockDriver(load_deck("inf", INF), device=gpu_device)
    md, mesh = drv.md, drv.mesh
    assert (md.comb_target, md.comb_trigger) == (INF_K, INF_T)
    sl = mesh.interior()
    for cycle in range(INF_CYCLES):
        drv.Step()
        assert md.n <= INF_T * 64, (cycle, md.n)
        assert md.ledger["residual"] <= 1e-12, (cycle, md.ledger["residual"])
        if md.comb_history and md.comb_history[-1]["cycle"] == md.cycle:
            h = md.comb_history[-1]
            assert h["n_after"] == md.n < h["n_before"] and h["cells_combed"] > 0
            assert abs(h["e_after"] - h["e_before"]) <= 1e-13 * h["e_before"]
            before = md.get_field("tally")[sl].copy()         # the census tally of the cycle's transport
            jb.EvaluateRadiationEnergy(md)                     # ... and that of the combed census
            np.testing.assert_allclose(md.get_field("tally")[sl], before, rtol=1e-12, atol=0)
    assert len(md.comb_history) >= INF_CYCLES // 2     # (a cell gains ~31 photons per cycle: no cell goes two cycles uncombed)
    g = md.get_swarm()
    assert len(np.unique(g["id"])) == md.n and int(g["id"].max()) < md.next_id
    key, _, nkeys, _ = cm.cell_keys(mesh, md.resident_gids, g, md.n)
    assert np.bincount(key, minlength=nkeys).max() <= INF_T


def test_without_the_keys_nothing_changes(gpu_device):
    """The deck without the comb's keys: no comb runs, and the photons are the CPU oracle's bit for bit, by id."""
    from jaybenne_amd import mcblock
    from oracle import orc
    ov = {"jaybenne/num_particles": 2000}
    drv = mcblock.McblockDriver(load_deck("inf", ov), device=gpu_device)
    assert drv.md.comb_target == 0
    O, _, _ = make_oracle(load_deck("inf", ov), orc.MATH_PORTABLE, capacity_factor=5.0)   # (2000 more every cycle)
    run_oracle_cycles(O, load_deck("inf", ov), 3)
    for _ in range(3):
        drv.Step()
    assert drv.md.comb_history == [] and drv.md.n == O.n
    g, o = _by_id(drv.md.get_swarm()), np.argsort(O.sw["id"][:O.n])
    for k in ("id", "x", "y", "z", "vx", "vy", "vz", "t", "w", "rng"):
        assert np.array_equal(g[k], O.sw[k][:O.n][o]), k


STEPDIFF = {"parthenon/mesh/nx1": 128, "parthenon/meshblock/nx1": 64, "jaybenne/num_particles": 400000,
            "jaybenne_amd/census_per_cell_max": 781}


@pytest.mark.lean
@pytest.mark.parametrize("host", ["python", "cpp"])
def test_stepdiff_acceptance(gpu_device, host):
    """stepdiff at nx1 = 128 with 4e5 photons, combed to K = 781 per cell (T = 1562) after every cycle, through
    ``python -m jaybenne_amd`` and through examples/mcblock_amd: the reference's gate (0.05), and 128 x 781 photons
    at the end."""
    import subprocess
    from helpers import DECK_DIR, ROOT
    args = ["-i", os.path.join(DECK_DIR, "stepdiff.in")] + [f"{k}={v}" for k, v in STEPDIFF.items()] + ["--tolerance", "0.05"]
    cmd = [sys.executable, "-m", "jaybenne_amd"] if host == "python" else [os.path.join(ROOT, "examples", "mcblock_amd")]
    res = subprocess.run(cmd + args, cwd=ROOT, capture_output=True, text=True, timeout=280)
    print(res.stdout[-1500:])
    assert res.returncode == 0 and "TEST PASSED" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
    cycles = [ln for ln in res.stdout.splitlines() if ln.startswith("cycle=")]
    assert len(cycles) == 10 and " photons=99968 " in cycles[-1] + " ", cycles[-1]
    assert " combed=128 " in cycles[0] + " ", cycles[0]


# ---- the checked library ------------------------------------------------------------------------------
def child_checked():
    """(in a child process under the checked library) two cycles with the comb on, then a sweep of the combed swarm"""
    import torch
    from jaybenne_amd import mcblock
    ov = {"parthenon/mesh/nx1": 16, "parthenon/meshblock/nx1": 8, "jaybenne/num_particles": 8000,
          "jaybenne_amd/census_per_cell_max": 100, "jaybenne_amd/census_comb_trigger": 1.5}
    drv = mcblock.McblockDriver(load_deck("stepdiff", ov), device=torch.device("cuda", 0))
    assert drv.md.invariants_enabled()
    for _ in range(2):
        drv.Step()       # (raises on a violation)
    return dict(report=drv.md.invariant_report(), sweep=drv.md.verify_swarm(drv.time, drv.time + drv.dt),
                combs=len(drv.md.comb_history), n=drv.md.n)


def test_a_comb_cycle_runs_clean_under_the_checked_library(gpu_device, checked_lib):
    from test_gpu_invariants import CHECKED
    import json
    import subprocess
    from helpers import ROOT
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "checked"], capture_output=True, text=True,
                         env=dict(os.environ, JAYBENNE_AMD_LIB=CHECKED), timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["combs"] >= 1 and out["n"] <= 16 * 150
    for rep in (out["report"], out["sweep"]):
        assert sum(rep["violated"].values()) == 0 and rep["first"] is None, rep
        assert rep["evaluated"]["SWARM"] > 0, rep


# ---- two ranks ------------------------------------------------------------------------------------
TWO_RANK = {"parthenon/mesh/nx1": 32, "parthenon/meshblock/nx1": 8, "jaybenne/num_particles": 16000,
            "jaybenne_amd/census_per_cell_max": 100, "jaybenne_amd/census_comb_trigger": 1.5}


def _rank_worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import mcblock
        from jaybenne_amd.comm import Comm
        drv = mcblock.McblockDriver(load_deck("stepdiff", TWO_RANK), rank=rank, nranks=world, comm=Comm(),
                                    device=torch.device("cuda", 0), capacity_factor=2.0)
        next0 = drv.md.next_id
        for _ in range(2):
            drv.Step()
        g = drv.md.get_swarm()
        key, _, nkeys, _ = cm.cell_keys(drv.mesh, drv.md.resident_gids, g, drv.md.n)
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), id=g["id"], w=g["w"], key=key, nkeys=np.array([nkeys]),
                 next_id=np.array([drv.md.next_id]), next0=np.array([next0]), new=np.array([h["n_new_ids"] for h in drv.md.comb_history]),
                 base=np.array([h["id_base"] for h in drv.md.comb_history]),
                 e=np.array([[h["e_before"], h["e_after"]] for h in drv.md.comb_history]).reshape(-1, 2))
    finally:
        dist.destroy_process_group()


@pytest.mark.lean
def test_two_ranks_comb_their_own_cells(gpu_device, tmp_path):
    """stepdiff in four blocks of eight cells over two gloo ranks on one card, 500 photons per cell combed to 100
    (T = 150): ids unique across the ranks, next_id equal on both, every owned cell at K or at most T."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)])
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    ids = np.concatenate([p["id"] for p in parts])
    assert len(np.unique(ids)) == len(ids)
    assert int(parts[0]["next_id"][0]) == int(parts[1]["next_id"][0]) > int(ids.max())
    assert len(parts[0]["new"]) == len(parts[1]["new"]) >= 1
    # first cycle: every cell holds 500 > T; rank 1's ids follow rank 0's
    assert int(parts[1]["base"][0]) == int(parts[0]["base"][0]) + int(parts[0]["new"][0])
    assert int(parts[0]["next0"][0]) + sum(int(p["new"].sum()) for p in parts) == int(parts[0]["next_id"][0])
    for p in parts:
        counts = np.bincount(p["key"], minlength=int(p["nkeys"][0]) + 1)[:int(p["nkeys"][0])]
        assert counts.max() <= 150 and counts.sum() == len(p["id"])
        assert np.all(np.abs(p["e"][:, 1] - p["e"][:, 0]) <= 1e-13 * p["e"][:, 0])
    assert sum(len(p["id"]) for p in parts) <= 32 * 150


if __name__ == "__main__":
    import json
    print(json.dumps(globals()["child_" + sys.argv[1]](*sys.argv[2:])))
