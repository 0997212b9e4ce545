"""The global census comb (include/jaybenne_amd.h: jb_comb_census_weigh / _plan_global / _apply) on the GPU.  Expected
values come from tests/gcomb_model.py -- the rule restated in numpy over the CPU oracle's generator -- never from the
library.  The crafted swarms of tests/gcomb_cases.py first (tests/test_gcomb_host.py counts their cases), then errors,
sequencing and whole runs."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import axis_cases as ax
import cell_order_model as om
import comb_model as cm
import gcomb_cases as gc
import gcomb_model as gm
from helpers import load_deck, make_oracle, run_oracle_cycles

from test_gpu_invariants import checked_lib  # noqa: E402,F401  (fixture: the checked library, built once)

pytestmark = pytest.mark.gpu

EPOCH, ID_BASE = 5, 1 << 33
GEOMS = {"1d": "G1", "2d": "G2S", "3d": "G3S"}
SALT = {"1d": 5, "2d": 6, "3d": 7}


def _driver(name, device, **kw):
    from jaybenne_amd import mcblock
    geom = GEOMS[name]
    g = ax.GEOMETRIES[geom]
    kinds = next(iter(ax.boundary_sets(geom).values()))
    ov = dict(ax.geometry_overrides(geom, kinds), **{ax.NP: 64})
    return mcblock.McblockDriver(load_deck("stepdiff_smr" if g.refine else "stepdiff", ov), device=device, **kw)


def _upload(md, sw, device, room=0):
    import torch
    n = len(sw["w"])
    md.reserve(max(n, room))
    for k, v in sw.items():
        md.swarm[k][:n] = torch.from_numpy(v.view(np.int64) if k in ("id", "rng") else v).to(device)
    md.sv.n = n
    torch.cuda.synchronize(device)


def _weigh(md, n_room):
    from jaybenne_amd import _lib
    md._sync_stream()
    plan = _lib.CombGlobalPlan()
    e = np.full(md.nblocks, -7.0)
    st = md.lib.jb_comb_census_weigh(md.pkg.ctx, md.handle, C.byref(md.sv), int(n_room), e.ctypes.data, C.byref(plan))
    return st, plan, e


def _total(md, e_local):
    from jaybenne_amd import jaybenne as jb
    e_gid = np.ascontiguousarray(jb.gather_block_energies(md, e_local), dtype=np.float64)
    return float(md.lib.jb_source_energy_total(e_gid.ctypes.data, int(md.mesh.nblocks)))


def _plan(md, w_total, N, r=gc.R_BAND, S=gc.S_MAX, epoch=EPOCH):
    from jaybenne_amd import _lib
    plan = _lib.CombGlobalPlan()
    st = md.lib.jb_comb_census_plan_global(md.pkg.ctx, md.handle, C.byref(md.sv), float(w_total), int(N), float(r), int(S),
                                           int(epoch), C.byref(plan))
    return st, plan


def _apply(md, id_base=ID_BASE):
    from jaybenne_amd import _lib
    rep = _lib.CombReport()
    st = md.lib.jb_comb_census_apply(md.pkg.ctx, md.handle, C.byref(md.sv), id_base, C.byref(rep))
    return st, rep


def _same(a, b, names=cm.SWARM_KEYS):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in names)


def _differing(a, b, names=cm.SWARM_KEYS):
    return [k for k in names if not np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8))]


def _by_id(sw):
    o = np.argsort(sw["id"], kind="stable")
    return {k: v[o] for k, v in sw.items()}


def _seed(drv):
    return int(drv.pin.GetOrAddInteger("jaybenne", "seed", 123))


def _whole_call(md, mesh, sw, device, N, r, S, seed, by_id, expect_sorted=1, owned=None):
    """upload, weigh, plan, apply against the model; returns (sorted input, output, plan bytes, report bytes, info)"""
    from jaybenne_amd import _lib
    n = len(sw["w"])
    n_room = min(n + N, S * n)
    _upload(md, sw, device, room=n_room)
    st, wrep, e_local = _weigh(md, n_room)
    assert st == _lib.JB_COMPLETE, md.lib.jb_last_error()
    assert (wrep.n_before, wrep.n_after, wrep.sorted) == (n, n, expect_sorted)
    g0 = md.get_swarm()
    assert md.n == n and _same(_by_id(g0), _by_id(sw))              # the weigh changes nothing a photon carries
    if by_id:
        assert _same(g0, om.canonical_sort(mesh, md.resident_gids, sw, n))
    owned = np.ones(md.nblocks) if owned is None else owned
    want, info = gm.gcomb_swarm(mesh, md.resident_gids, owned, g0, n, N, r, S, seed, EPOCH, ID_BASE,
                                exact=by_id, sort=False)
    # the block sums and the total, bit for bit
    assert np.array_equal(e_local.view(np.uint64), info["e_block"].view(np.uint64)), (e_local, info["e_block"])
    if owned.all():
        w_total = _total(md, e_local)
        assert w_total == info["w_total"]
    else:       # (one rank of two, on its own: the total of its blocks alone, added as the library's helper adds)
        w_total = info["w_total"]
    act = g0["status"] == cm.ST_ACTIVE
    e_sum = math.fsum(g0["w"][act & np.isfinite(g0["w"])])          # (the cell with an inf is left alone)
    st, plan = _plan(md, w_total, N, r, S)
    assert st == _lib.JB_COMPLETE, md.lib.jb_last_error()
    got = (plan.n_before, plan.n_after, plan.n_new_ids, plan.cells_thinned, plan.cells_split, plan.max_per_cell,
           plan.max_target, plan.sorted)
    assert got == (n, info["n_after"], info["n_new_ids"], info["cells_thinned"], info["cells_split"],
                   info["max_per_cell"], info["max_target"], expect_sorted), got
    assert plan.e_before == wrep.e_before
    assert _same(md.get_swarm(), g0)                                  # nothing a photon carries has changed yet
    st, rep = _apply(md)
    assert st == _lib.JB_COMPLETE, md.lib.jb_last_error()
    assert (rep.n_after, rep.n_new_ids) == (info["n_after"], info["n_new_ids"]) and md.n == info["n_after"]
    g1 = md.get_swarm()
    return g0, g1, want, info, plan, rep, e_sum


# ---- 1, 2: bit for bit against the model on the crafted swarms ------------------------------------------------------
@pytest.mark.parametrize("weights,order", [("crafted", "any"), ("crafted", "id"), ("hashed", "id"), ("hashed", "any")])
@pytest.mark.parametrize("name", ["1d", "2d", "3d"])
def test_comb_equals_the_model_bit_for_bit(gpu_device, name, weights, order):
    drv = _driver(name, gpu_device)
    md, mesh = drv.md, drv.mesh
    md.cell_order = order
    by_id = order == "id"
    sw, N, placed = gc.crafted(mesh, md.resident_gids, SALT[name], weights)
    r, S = (gc.R_BAND, gc.S_MAX) if weights == "crafted" else (gc.R_BAND, 64)
    g0, g1, want, info, plan, rep, e_sum = _whole_call(md, mesh, sw, gpu_device, N, r, S, _seed(drv), by_id)
    assert info["cells_thinned"] > 0 and info["cells_split"] > 0
    skipped = [k for k, v in info["margins"].items() if v < 1e-9]
    if weights == "crafted":
        # every sum is exact in any order: the energies too
        assert info["scale"] == 16.0
    if weights == "crafted" or by_id:
        skipped = []                                                            # exact sums: no margin, no skips
    assert len(skipped) <= 0.01 * len(info["margins"])
    if not skipped:
        assert _differing(g1, want) == []
    else:       # (a last bit of the running sums may decide: those cells are left out, every other cell is the model's)
        key1 = cm.cell_keys(mesh, md.resident_gids, g1, md.n)[0]
        keyw = cm.cell_keys(mesh, md.resident_gids, want, info["n_after"])[0]
        carried = [k for k in cm.SWARM_KEYS if k not in ("id", "rng")]
        for k in info["cells"]:
            if k not in skipped:
                assert _same({q: g1[q][key1 == k] for q in carried}, {q: want[q][keyw == k] for q in carried}, carried), k
    act1 = g1["status"] == cm.ST_ACTIVE
    fin = np.isfinite(g1["w"])
    e1 = math.fsum(g1["w"][act1 & fin])
    assert abs(e1 - e_sum) <= 1e-13 * e_sum
    if math.isfinite(rep.e_after):
        assert abs(rep.e_after - e1) <= 1e-13 * e1

    # ---- the same sorted swarm, twice: the same bits
    for _ in range(2):
        g0b, g1b, _, _, plan2, rep2, _ = _whole_call(md, mesh, g0, gpu_device, N, r, S, _seed(drv), by_id, expect_sorted=0)
        assert _same(g0b, g0) and _same(g1b, g1)
        assert bytes(plan2)[:56] == bytes(plan)[:56] and bytes(rep2)[:16] == bytes(rep)[:16]


@pytest.mark.parametrize("pad", gc.TILE_PADS)
@pytest.mark.parametrize("name,weights,order", [("1d", "crafted", "any"), ("2d", "crafted", "any"), ("1d", "hashed", "id")])
def test_cells_of_2049_at_every_lane_offset(gpu_device, name, weights, order, pad):
    """gcomb_cases.tile_specs: 22 cells of 2049 photons behind 0, 22 and 44 padding photons -- over the three swarms one
    starts at every lane offset (tests/test_gcomb_host.py counts them) --, thinned, left alone and split in turn."""
    drv = _driver(name, gpu_device)
    md, mesh = drv.md, drv.mesh
    md.cell_order = order
    sw, N, placed = gc.crafted(mesh, md.resident_gids, SALT[name], weights, pad)
    S = gc.S_MAX if weights == "crafted" else 64
    g0, g1, want, info, plan, rep, _ = _whole_call(md, mesh, sw, gpu_device, N, gc.R_BAND, S, _seed(drv), order == "id")
    starts = {info["cells"][k][0] % 64 for s, k in placed if s.tag == "tile-2049"}
    assert starts == {(pad + q) % 64 for q in range(gc.TILE_CELLS)}
    if weights == "crafted":
        assert info["cells_thinned"] >= 7 and info["cells_split"] >= 7
    assert _differing(g1, want) == []


@pytest.mark.parametrize("name", ["1d", "3d"])
def test_band_one_combs_every_cell_off_its_target(gpu_device, name):
    """r = 1 on the crafted swarm: the one-photon cell with nu = 2 is split in two (inside the band at r = 2), and every
    cell whose target is not its count is combed."""
    drv = _driver(name, gpu_device)
    md, mesh = drv.md, drv.mesh
    sw, N, placed = gc.crafted(mesh, md.resident_gids, SALT[name])
    g0, g1, want, info, plan, rep, _ = _whole_call(md, mesh, sw, gpu_device, N, 1.0, gc.S_MAX, _seed(drv), False)
    k2 = next(k for s, k in placed if s.tag == "one-to-2")
    assert info["combed"][k2] == 2
    assert all((k in info["combed"]) == (K != info["cells"][k][1] - info["cells"][k][0]) for k, K in info["targets"].items())
    assert _differing(g1, want) == []


def test_an_empty_swarm_and_a_swarm_without_weight(gpu_device):
    from jaybenne_amd import _lib
    drv = _driver("1d", gpu_device)
    md, mesh = drv.md, drv.mesh
    md.sv.n = 0
    st, wrep, e = _weigh(md, 0)
    assert st == _lib.JB_COMPLETE and np.all(e == 0.0) and (wrep.n_before, wrep.n_after) == (0, 0)
    st, plan = _plan(md, 0.0, 100)
    assert st == _lib.JB_COMPLETE and (plan.n_before, plan.n_after, plan.n_new_ids) == (0, 0, 0)
    assert _apply(md)[0] == _lib.JB_ERR_INVALID               # nothing is combed: there is no plan to apply
    # every weight zero: W_tot = 0, nothing is combed
    sw, N, _ = gc.crafted(mesh, md.resident_gids, 3)
    sw["w"][:] = 0.0
    _upload(md, sw, gpu_device)
    st, wrep, e = _weigh(md, len(sw["w"]))
    assert st == _lib.JB_COMPLETE and np.all(e == 0.0)
    st, plan = _plan(md, _total(md, e), N)
    assert st == _lib.JB_COMPLETE and plan.n_after == plan.n_before and plan.cells_thinned == plan.cells_split == 0
    assert _same(_by_id(md.get_swarm()), _by_id(sw))


# ---- 3: errors, each with the swarm byte-identical behind it --------------------------------------------------------
def test_errors_leave_the_swarm_as_it_was(gpu_device):
    from jaybenne_amd import _lib
    drv = _driver("1d", gpu_device)
    md, mesh = drv.md, drv.mesh
    sw, N, _ = gc.crafted(mesh, md.resident_gids, SALT["1d"])
    n = len(sw["w"])
    _upload(md, sw, gpu_device, room=n + N)
    # plan without weigh
    st, _ = _plan(md, 1.0, N)
    assert st == _lib.JB_ERR_INVALID and b"weigh" in md.lib.jb_last_error()
    assert _same(md.get_swarm(), sw)
    # n_room outside [n, capacity]
    for room in (n - 1, md.capacity + 1):
        assert _weigh(md, room)[0] == _lib.JB_ERR_INVALID
        assert _plan(md, 1.0, N)[0] == _lib.JB_ERR_INVALID
    assert _same(md.get_swarm(), sw)
    # the comb needs more slots than n_room: JB_ERR_CAPACITY before any record is written
    st, wrep, e = _weigh(md, n)
    assert st == _lib.JB_COMPLETE
    g0 = md.get_swarm()
    w_total = _total(md, e)
    st, plan = _plan(md, w_total, N)
    assert st == _lib.JB_ERR_CAPACITY, md.lib.jb_last_error()
    assert plan.n_after > n and md.n == n
    assert _apply(md)[0] == _lib.JB_ERR_INVALID                  # a failed plan is no plan
    assert _same(md.get_swarm(), g0)
    # bad arguments (each behind a fresh weigh); a failed plan is no plan, and its weigh is spent
    for args in (dict(N=0), dict(N=-5), dict(N=1 << 31), dict(r=0.5), dict(r=float("nan")), dict(r=float("inf")),
                 dict(S=0), dict(S=-1), dict(epoch=1 << 20)):
        assert _weigh(md, n + N)[0] == _lib.JB_COMPLETE
        kw = dict(dict(N=N), **args)
        st, _ = _plan(md, w_total, **kw)
        assert st == _lib.JB_ERR_INVALID, args
        assert _apply(md)[0] == _lib.JB_ERR_INVALID
        assert _plan(md, w_total, N)[0] == _lib.JB_ERR_INVALID, args
    assert _same(md.get_swarm(), g0)
    # the swarm changed between weigh and plan, and between plan and apply
    assert _weigh(md, n + N)[0] == _lib.JB_COMPLETE
    md.sv.n = n - 1
    assert _plan(md, w_total, N)[0] == _lib.JB_ERR_INVALID
    md.sv.n = n
    assert _weigh(md, n + N)[0] == _lib.JB_COMPLETE
    st, plan = _plan(md, w_total, N)
    assert st == _lib.JB_COMPLETE and plan.n_after > n
    md.sv.n = n - 1
    assert _apply(md)[0] == _lib.JB_ERR_INVALID
    md.sv.n = n
    assert _same(md.get_swarm(), g0)
    # a w_total that is not the total, with a split limit to match: the copies pass 2^32, which the 32-bit scans
    # cannot count -- the plan counts them in 64 bits and refuses before any record is written
    assert _weigh(md, n + N)[0] == _lib.JB_COMPLETE
    st, plan = _plan(md, w_total * 1e-12, N, S=1 << 31)
    assert st == _lib.JB_ERR_CAPACITY and plan.n_after >= 1 << 32, (st, plan.n_after)
    assert _apply(md)[0] == _lib.JB_ERR_INVALID
    assert _same(md.get_swarm(), g0)
    # a per-cell plan between weigh and the global plan takes the scratch: the weigh is spent
    assert _weigh(md, n + N)[0] == _lib.JB_COMPLETE
    per_cell = _lib.CombPlan()
    assert md.lib.jb_comb_census_plan(md.pkg.ctx, md.handle, C.byref(md.sv), 1 << 20, 1 << 20, 1, C.byref(per_cell)) == _lib.JB_COMPLETE
    assert _plan(md, w_total, N)[0] == _lib.JB_ERR_INVALID
    assert _same(md.get_swarm(), g0)


# ---- 4: sequencing -------------------------------------------------------------------------------------------------
def test_unsorted_equals_sorted_and_the_per_cell_comb_still_works(gpu_device):
    from jaybenne_amd import _lib
    drv = _driver("2d", gpu_device)
    md, mesh = drv.md, drv.mesh
    seed = _seed(drv)
    md.cell_order = "id"
    sw, N, _ = gc.crafted(mesh, md.resident_gids, SALT["2d"], "hashed")
    n = len(sw["w"])
    g0, g1, want, info, plan, rep, _ = _whole_call(md, mesh, sw, gpu_device, N, gc.R_BAND, 64, seed, True)
    perm = np.argsort(gc._hash(np.arange(n), 777))
    sw2 = {k: np.ascontiguousarray(v[perm]) for k, v in sw.items()}
    _, g2, _, _, plan2, rep2, _ = _whole_call(md, mesh, sw2, gpu_device, N, gc.R_BAND, 64, seed, True)
    _, g3, _, _, plan3, rep3, _ = _whole_call(md, mesh, g0, gpu_device, N, gc.R_BAND, 64, seed, True, expect_sorted=0)
    assert _same(g1, g2) and _same(g1, g3) and bytes(rep) == bytes(rep2) == bytes(rep3)
    assert bytes(plan)[:56] == bytes(plan2)[:56] == bytes(plan3)[:56]
    # the per-cell plan and apply on the same context: comb_model's bits (crafted weights: its sums are exact too)
    md.cell_order = "any"
    swc, _, _ = gc.crafted(mesh, md.resident_gids, SALT["2d"])
    keep = np.isfinite(swc["w"]) & (swc["w"] >= 0.0)
    swc = {k: np.ascontiguousarray(v[keep]) for k, v in swc.items()}
    nc = len(swc["w"])
    _upload(md, swc, gpu_device)
    T, K = 70, 16
    md._sync_stream()
    p = _lib.CombPlan()
    assert md.lib.jb_comb_census_plan(md.pkg.ctx, md.handle, C.byref(md.sv), T, K, EPOCH, C.byref(p)) == _lib.JB_COMPLETE
    s0 = md.get_swarm()
    wantc, infoc = cm.comb_swarm(mesh, md.resident_gids, s0, nc, T, K, seed, EPOCH, ID_BASE, sort=False)
    st, r2 = _apply(md)
    assert st == _lib.JB_COMPLETE and (r2.n_after, r2.n_new_ids) == (infoc["n_after"], infoc["n_new_ids"])
    assert infoc["cells_combed"] >= 4 and _differing(md.get_swarm(), wantc) == []


# ---- 5: whole runs -------------------------------------------------------------------------------------------------
RUN_N = 20000
RUNS = {
    "inf": ("inf", {"jaybenne/num_particles": 20000}),
    "stepdiff": ("stepdiff", {"parthenon/mesh/nx1": 32, "parthenon/meshblock/nx1": 16, "jaybenne/num_particles": 30000,
                              "jaybenne/do_emission": "true", "jaybenne/do_feedback": "true"}),
}
RUN_KEYS = {"jaybenne_amd/census_total_target": RUN_N, "jaybenne_amd/deposition": "exact", "jaybenne_amd/cell_order": "id",
            "jaybenne_amd/ledger": "true"}


@pytest.mark.parametrize("deck", ["inf", "stepdiff"])
def test_two_cycles_hold_the_population_and_the_energy(gpu_device, deck):
    from jaybenne_amd import jaybenne as jb, mcblock
    import moments_model as mm
    name, ov = RUNS[deck]
    finals = []
    for resort in (False, True):
        drv = mcblock.McblockDriver(load_deck(name, dict(ov, **RUN_KEYS)), device=gpu_device, capacity_factor=4.0)
        md, mesh = drv.md, drv.mesh
        assert (md.census_total_target, md.census_total_band, md.census_split_max) == (RUN_N, 2.0, 64)
        r = md.census_total_band
        for cycle in range(2):
            if resort:
                jb.DefragParticles(md)                            # sorted just now | last sorted a cycle ago
            drv.Step()
            key = cm.cell_keys(mesh, md.resident_gids, md.get_swarm(), md.n)[0]
            occupied = len(np.unique(key))
            print(deck, "cycle", cycle, "n =", md.n, "occupied cells", occupied, "residual", md.ledger["residual"],
                  md.comb_history[-1:] if md.comb_history else None)
            assert RUN_N / r <= md.n <= r * RUN_N + occupied, (cycle, md.n)
            assert md.ledger["residual"] <= 1e-12, (cycle, md.ledger["residual"])
            for h in md.comb_history:
                assert h["mode"] == "global" and abs(h["e_after"] - h["e_before"]) <= 1e-13 * h["e_before"]
                assert h["scale"] == RUN_N / h["w_total"]
        fields, rep = jb.EvaluateRadiationMoments(md)
        integ = mm.integrals(fields.cpu().numpy(), np.asarray(mesh.blk_dx)[md.resident_gids])
        e_census = md.ledger["e_census"]
        assert abs(integ[1] - e_census) <= 1e-12 * e_census
        g = md.get_swarm()
        assert len(np.unique(g["id"])) == md.n and int(g["id"].max()) < md.next_id
        finals.append((_by_id(g), [dict(h) for h in md.comb_history]))
    assert len(finals[0][1]) >= 1
    assert _differing(finals[0][0], finals[1][0]) == []
    for a, b in zip(finals[0][1], finals[1][1]):
        assert a == b


def test_both_hosts_write_the_same_comb_history_and_ledger(gpu_device, tmp_path):
    """``python -m jaybenne_amd`` and examples/mcblock_amd on the stepdiff run above: the same lines of
    ``--comb-history`` and ``--ledger``, number for number."""
    import json
    import subprocess
    from helpers import DECK_DIR, ROOT
    name, ov = RUNS["stepdiff"]
    keys = dict(ov, **RUN_KEYS)
    keys["parthenon/time/tlim"] = 6.0e-11          # two cycles of dt = 3.335641e-11
    lines = {}
    for host in ("python", "cpp"):
        files = {k: str(tmp_path / f"{host}_{k}.jsonl") for k in ("ledger", "comb")}
        args = ["-i", os.path.join(DECK_DIR, name + ".in")] + [f"{k}={v}" for k, v in keys.items()] + \
            ["--ledger", files["ledger"], "--comb-history", files["comb"]]
        cmd = [sys.executable, "-m", "jaybenne_amd"] if host == "python" else [os.path.join(ROOT, "examples", "mcblock_amd")]
        res = subprocess.run(cmd + args, cwd=ROOT, capture_output=True, text=True, timeout=280)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        lines[host] = {k: [json.loads(ln) for ln in open(f)] for k, f in files.items()}
    assert len(lines["python"]["comb"]) >= 1 and len(lines["python"]["ledger"]) == 2
    assert all(rec["mode"] == "global" and rec["cells_thinned"] + rec["cells_split"] == rec["cells_combed"] > 0
               for rec in lines["python"]["comb"])
    assert lines["python"]["comb"] == lines["cpp"]["comb"]
    assert len(lines["cpp"]["ledger"]) == 2 and lines["python"]["ledger"] == lines["cpp"]["ledger"]


def test_without_the_keys_nothing_changes(gpu_device):
    """The deck without the global comb's keys: no comb runs, and the photons are the CPU oracle's bit for bit, by id."""
    from jaybenne_amd import mcblock
    from oracle import orc
    ov = {"jaybenne/num_particles": 2000}
    drv = mcblock.McblockDriver(load_deck("inf", ov), device=gpu_device)
    assert drv.md.census_total_target == 0 and drv.md.comb_target == 0
    O, _, _ = make_oracle(load_deck("inf", ov), orc.MATH_PORTABLE, capacity_factor=5.0)
    run_oracle_cycles(O, load_deck("inf", ov), 3)
    for _ in range(3):
        drv.Step()
    assert drv.md.comb_history == [] and drv.md.n == O.n
    assert drv.md.lib.jb_gcomb_kernel_launches(drv.md.pkg.ctx) == 0       # none of the new kernels was launched
    g, o = _by_id(drv.md.get_swarm()), np.argsort(O.sw["id"][:O.n])
    for k in ("id", "x", "y", "z", "vx", "vy", "vz", "t", "w", "rng"):
        assert np.array_equal(g[k], O.sw[k][:O.n][o]), k
    # ... nor under the per-cell comb; with the key, weigh, targets, decide and pack are
    drv = mcblock.McblockDriver(load_deck("inf", dict(ov, **{"jaybenne_amd/census_per_cell_max": 8})), device=gpu_device)
    for _ in range(2):
        drv.Step()
    assert len(drv.md.comb_history) >= 1 and drv.md.lib.jb_gcomb_kernel_launches(drv.md.pkg.ctx) == 0
    drv = mcblock.McblockDriver(load_deck("inf", dict(ov, **{"jaybenne_amd/census_total_target": 1000})), device=gpu_device)
    drv.Step()
    assert len(drv.md.comb_history) == 1 and drv.md.lib.jb_gcomb_kernel_launches(drv.md.pkg.ctx) == 4


def test_both_combs_at_once_and_a_replicated_mesh_are_errors(gpu_device):
    from jaybenne_amd import jaybenne as jb, mcblock
    with pytest.raises(ValueError) as err:
        mcblock.McblockDriver(load_deck("inf", {"jaybenne_amd/census_total_target": 100,
                                                "jaybenne_amd/census_per_cell_max": 10}), device=gpu_device)
    assert "census_total_target" in str(err.value) and "census_per_cell_max" in str(err.value)
    drv = mcblock.McblockDriver(load_deck("inf", {"jaybenne_amd/census_total_target": 100}), device=gpu_device)
    drv.md.replicated = True
    with pytest.raises(ValueError):
        jb.CombCensusGlobal(drv.md)


# ---- 6: the checked library ----------------------------------------------------------------------------------------
def child_checked():
    """(in a child process under the checked library) a cycle with the global comb on, then a sweep of the swarm"""
    import torch
    from jaybenne_amd import mcblock
    ov = {"parthenon/mesh/nx1": 16, "parthenon/meshblock/nx1": 8, "jaybenne/num_particles": 8000,
          "jaybenne_amd/census_total_target": 3000, "jaybenne_amd/census_total_band": 1.5}
    drv = mcblock.McblockDriver(load_deck("stepdiff", ov), device=torch.device("cuda", 0))
    assert drv.md.invariants_enabled()
    drv.Step()           # (raises on a violation)
    return dict(report=drv.md.invariant_report(), sweep=drv.md.verify_swarm(drv.time, drv.time + drv.dt),
                combs=len(drv.md.comb_history), n=drv.md.n)


def test_a_global_comb_cycle_runs_clean_under_the_checked_library(gpu_device, checked_lib):
    from test_gpu_invariants import CHECKED
    import json
    import subprocess
    from helpers import ROOT
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "checked"], capture_output=True, text=True,
                         env=dict(os.environ, JAYBENNE_AMD_LIB=CHECKED), timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["combs"] == 1 and 2000 <= out["n"] <= 4500 + 16
    for rep in (out["report"], out["sweep"]):
        assert sum(rep["violated"].values()) == 0 and rep["first"] is None, rep
        assert rep["evaluated"]["SWARM"] > 0, rep


# ---- 7: two ranks --------------------------------------------------------------------------------------------------
TWO_RANK = {"parthenon/mesh/nx1": 32, "parthenon/meshblock/nx1": 8, "jaybenne/num_particles": 16000,
            "jaybenne_amd/census_total_target": 24000, "jaybenne_amd/census_total_band": 1.25,
            "jaybenne_amd/cell_order": "id", "jaybenne_amd/deposition": "exact"}


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
        assert int((np.asarray(drv.md.owned_flags) == 0).sum()) >= 1       # a halo copy in the view
        for _ in range(2):
            drv.Step()
        g = drv.md.get_swarm()
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), next_id=np.array([drv.md.next_id]),
                 new=np.array([h["n_new_ids"] for h in drv.md.comb_history]),
                 w_total=np.array([h["w_total"] for h in drv.md.comb_history]), **{k: g[k] for k in cm.SWARM_KEYS})
    finally:
        dist.destroy_process_group()


HALO_DECK = {"parthenon/mesh/nx1": 64, "parthenon/meshblock/nx1": 16, "jaybenne/num_particles": 64}


def _halo_worker(rank, world, port, outdir):
    """One rank of two, each on its own (no collective inside): the crafted swarm laid over ALL resident blocks of
    the rank's view, halo copies included, against the model with the view's owned flags."""
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import mcblock
        from jaybenne_amd.comm import Comm
        device = torch.device("cuda", 0)
        drv = mcblock.McblockDriver(load_deck("stepdiff", HALO_DECK), rank=rank, nranks=world, comm=Comm(), device=device,
                                    capacity_factor=2.0)
        md, mesh = drv.md, drv.mesh
        owned = np.asarray(md.owned_flags).astype(np.float64)
        res = dict(halo_blocks=np.array([int((owned == 0).sum())]))
        for order in ("any", "id"):
            md.cell_order = order
            sw, N, placed = gc.crafted(mesh, md.resident_gids, 11 + rank)
            ntot = int(np.prod(mesh.field_shape[1:]))
            in_halo = sum(s.m for s, k in placed if owned[k // ntot] == 0)
            g0, g1, want, info, plan, rep, _ = _whole_call(md, mesh, sw, device, N, gc.R_BAND, gc.S_MAX, _seed(drv),
                                                           order == "id", owned=owned)
            combed_in_halo = sum(1 for k in info["combed"] if owned[k // ntot] == 0)
            res[order] = np.array([in_halo, combed_in_halo, len(_differing(g1, want)),
                                   int(np.all(info["e_block"][owned == 0] == 0.0)), int(np.all(info["e_block"][owned == 1] > 0.0))])
        np.savez(os.path.join(outdir, f"halo{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


def test_a_halo_copy_in_the_view(gpu_device, tmp_path):
    """Two gloo ranks on one card, each with two owned blocks and a halo copy that HOLDS photons: the block sums -- 0
    for the halo copy, whose cells are combed all the same --, the report and every swarm attribute equal the model
    with the view's owned flags, bit for bit (the assertions of _whole_call run inside the ranks)."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_halo_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)])
    for r in range(2):
        res = np.load(tmp_path / f"halo{r}.npz")
        assert int(res["halo_blocks"][0]) >= 1
        for order in ("any", "id"):
            in_halo, combed_in_halo, differing, halo_zero, owned_positive = (int(v) for v in res[order])
            assert in_halo > 0 and combed_in_halo > 0 and differing == 0 and halo_zero == 1 and owned_positive == 1


def test_two_ranks_give_the_photons_of_one(gpu_device, tmp_path):
    """stepdiff in four blocks over two gloo ranks on one card, block partition, cell_order = id: survivors, weights
    and new ids are those of one rank."""
    import torch.multiprocessing as mp
    from jaybenne_amd import mcblock
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)])
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    drv = mcblock.McblockDriver(load_deck("stepdiff", TWO_RANK), device=gpu_device, capacity_factor=2.0)
    for _ in range(2):
        drv.Step()
    one = _by_id(drv.md.get_swarm())
    assert len(drv.md.comb_history) >= 1 and sum(h["n_new_ids"] for h in drv.md.comb_history) > 0
    assert int(parts[0]["next_id"][0]) == int(parts[1]["next_id"][0]) == drv.md.next_id
    assert np.array_equal(parts[0]["w_total"], np.array([h["w_total"] for h in drv.md.comb_history]))
    both = {k: np.concatenate([p[k] for p in parts]) for k in cm.SWARM_KEYS}
    two = _by_id(both)
    assert len(two["id"]) == len(one["id"])
    assert _differing(two, one, [k for k in cm.SWARM_KEYS if k != "blk"]) == []     # (blk: an index into the rank's view)


if __name__ == "__main__":
    import json
    print(json.dumps(globals()["child_" + sys.argv[1]](*sys.argv[2:])))
