"""The canonical order within cells (include/jaybenne_amd.h: jb_set_cell_order, JB_CELL_ORDER_BY_ID) on the GPU: the
sort against tests/cell_order_model.py slot for slot, the census comb against tests/comb_model.py whatever slots the
photons came in, and whole runs that do not depend on when the swarm was sorted or on how many ranks hold it.
Expected values come from the numpy models, never from the library.

The synthetic swarm is that of tests/test_gpu_comb.py with other ids: distinct hashed values, a third of the slots
in the lowest class, a third between 2^16 and 2^33, the rest between 2^33 and 2^62.  (Only 256 distinct ids exist
below 2^8: the lowest class takes all of them and fills up between 2^8 and 2^16, so that every digit boundary of the
low word is still crossed.)  Some ids differ only above bit 32, one cell's ids are all multiples of 256 (a pass
that sees one digit value), the dead slots have ids of their own, three of them with bit 63 set."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cell_order_model as om
import comb_model as cm
from helpers import DECK_DIR, ROOT, load_deck

from test_gpu_comb import (EPOCH, MESHES, SCAN_TILE, T_SYN, _apply, _by_id, _driver, _hash, _plan, _same,
                           _synthetic, _unit, _upload)
from test_gpu_invariants import checked_lib  # noqa: E402,F401  (fixture: the checked library, built once)

pytestmark = pytest.mark.gpu

EDGE_SIZES = (1, 63, 64, 65, 2047, 2048, 2049)
# the first id the comb hands out: above every live id of the swarm (< 2^62), as a host's next_id always is
NEW_IDS = 1 << 62
# the salts of the synthetic swarm per mesh: chosen on the CPU so that no combed cell of the MODEL has a count that
# the last bit of a running sum decides (comb_model.comb_margin >= 1e-9 for K = 1 and K = T; the margins depend on
# the order within the cell, so they were looked at again for this order) -- test_comb_does_not_depend_on_slot_order
# asserts it
SALT = {"1d": 23, "3d": 5}


def _distinct(m, lo, hi, salt):
    """m distinct hashed values in [lo, hi)"""
    span = hi - lo
    if span <= (1 << 16):
        assert m <= span
        return (np.argsort(_hash(np.arange(span), salt), kind="stable")[:m] + lo).astype(np.uint64)
    v = np.uint64(lo) + _hash(np.arange(m), salt) % np.uint64(span)
    assert len(np.unique(v)) == m
    return v


def _hashed_ids(n, salt):
    """n distinct ids over the three classes, dealt to the slots by a hashed permutation"""
    n_low = (n + 2) // 3
    n_mid = (n - n_low + 1) // 2
    n_top = n - n_low - n_mid
    n_byte = min(n_low, 256)
    ids = np.concatenate([_distinct(n_byte, 0, 1 << 8, salt + 1), _distinct(n_low - n_byte, 1 << 8, 1 << 16, salt + 2),
                          _distinct(n_mid, 1 << 16, 1 << 33, salt + 3), _distinct(n_top, 1 << 33, 1 << 62, salt + 4)])
    top = n_low + n_mid
    for j in range(min(n_top // 2, 24)):           # pairs that differ in bit 50 alone
        ids[top + 2 * j] &= ~np.uint64(1 << 50)
        ids[top + 2 * j + 1] = ids[top + 2 * j] | np.uint64(1 << 50)
    assert np.all(ids[top:] >= np.uint64(1 << 33)) and np.all(ids[top:] < np.uint64(1 << 62))
    return ids[np.argsort(_hash(np.arange(n), salt + 5), kind="stable")]


def _swarm(mesh, gids, salt):
    """_synthetic of tests/test_gpu_comb.py with the ids of the module docstring"""
    sw, per = _synthetic(mesh, salt)
    n = len(sw["w"])
    ids = _hashed_ids(n, salt + 200)
    key, _, nkeys, _ = cm.cell_keys(mesh, gids, sw, n)
    counts = np.bincount(key, minlength=nkeys + 1)
    (k300,) = np.flatnonzero(counts[:nkeys] == 300)          # the cell of 300 photons: ids that are multiples of 256
    sel = np.flatnonzero(key == k300)
    ids[sel] = _distinct(300, 1 << 8, 1 << 25, salt + 300) << np.uint64(8)
    dead = np.flatnonzero(key == nkeys)
    assert len(dead) == 37
    ids[dead[:3]] |= np.uint64(1 << 63)
    assert len(np.unique(ids)) == n
    low, mid = ids < np.uint64(1 << 16), (ids >= np.uint64(1 << 16)) & (ids < np.uint64(1 << 33))
    assert 200 <= int((ids < np.uint64(1 << 8)).sum()) <= 256          # (the cell of 300 and the holes took some)
    assert 0.28 * n < low.sum() < 0.37 * n and 0.3 * n < mid.sum() < 0.4 * n
    sw["id"] = ids
    return sw, per


def _edge_swarm(mesh, n, spread, salt):
    """n ACTIVE photons in the first cell, or spread over all cells; hashed ids"""
    nx = [int(v) for v in mesh.nx]
    ncell = nx[0] * nx[1] * nx[2]
    i = np.arange(n)
    cell_of = (_hash(i, salt) % np.uint64(mesh.nblocks * ncell)).astype(np.int64) if spread else np.zeros(n, dtype=np.int64)
    blk, c = cell_of // ncell, cell_of % ncell
    ijk = [c % nx[0], (c // nx[0]) % nx[1], c // (nx[0] * nx[1])]
    sw = {}
    for d, name in enumerate(("x", "y", "z")):
        sw[name] = (mesh.blk_xmin[blk, d] + (ijk[d] + 0.05 + 0.9 * _unit(i, salt + 31 + d)) * mesh.blk_dx[blk, d]
                    if d < mesh.ndim else np.zeros(n))
    for q, name in enumerate(("vx", "vy", "vz", "t", "e", "w")):
        sw[name] = _unit(i, salt + 50 + q) + 0.25
    ng = mesh.ng
    sw["ip"] = (ijk[0] + ng).astype(np.int32)
    sw["jp"] = (ijk[1] + (ng if mesh.ndim >= 2 else 0)).astype(np.int32)
    sw["kp"] = (ijk[2] + (ng if mesh.ndim >= 3 else 0)).astype(np.int32)
    sw["blk"] = blk.astype(np.int32)
    sw["status"] = np.zeros(n, dtype=np.int32)
    sw["id"] = _hashed_ids(n, salt + 200)
    sw["rng"] = _hash(i, salt + 99)
    return sw


def _permuted(sw, salt):
    n = len(sw["w"])
    perm = np.argsort(_hash(np.arange(n), salt), kind="stable")
    return {k: np.ascontiguousarray(v[perm]) for k, v in sw.items()}


def _defrag(md):
    from jaybenne_amd import _lib
    md._sync_stream()
    st = md.lib.jb_defrag_particles(md.pkg.ctx, md.handle, C.byref(md.sv))
    assert st == _lib.JB_COMPLETE, md.lib.jb_last_error()
    return md.get_swarm()


# ---- 10: the default ------------------------------------------------------------------------------
def test_the_default_is_any_and_a_wrong_mode_is_refused(gpu_device):
    from jaybenne_amd import _lib
    drv = _driver("1d", gpu_device)
    md = drv.md
    assert md.lib.jb_get_cell_order(md.pkg.ctx) == _lib.CELL_ORDER_ANY and md.cell_order == "any"
    for mode in (7, -1, 2):
        assert md.lib.jb_set_cell_order(md.pkg.ctx, mode) == _lib.JB_ERR_INVALID
        assert b"jb_set_cell_order" in md.lib.jb_last_error()
        assert md.lib.jb_get_cell_order(md.pkg.ctx) == _lib.CELL_ORDER_ANY
    md.cell_order = "id"
    assert md.lib.jb_get_cell_order(md.pkg.ctx) == _lib.CELL_ORDER_BY_ID and md.cell_order == "id"
    assert md.lib.jb_set_cell_order(md.pkg.ctx, 7) == _lib.JB_ERR_INVALID
    assert md.lib.jb_get_cell_order(md.pkg.ctx) == _lib.CELL_ORDER_BY_ID
    md.cell_order = "any"
    assert md.cell_order == "any"
    with pytest.raises(ValueError, match="cell_order"):
        md.cell_order = "sorted"
    deck, ov = MESHES["1d"]
    from jaybenne_amd import mcblock
    drv2 = mcblock.McblockDriver(load_deck(deck, dict(ov, **{"jaybenne_amd/cell_order": "id"})), device=gpu_device)
    assert drv2.md.cell_order == "id"


# ---- 5: the sort against the model ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1d", "3d"])
def test_sort_equals_the_model_slot_for_slot(gpu_device, name):
    from jaybenne_amd import _lib
    drv = _driver(name, gpu_device)
    md, mesh = drv.md, drv.mesh
    md.cell_order = "id"
    sw, _ = _swarm(mesh, md.resident_gids, SALT[name])
    n = len(sw["w"])
    want = om.canonical_sort(mesh, md.resident_gids, sw, n)
    assert not om.is_canonical(mesh, md.resident_gids, sw, n)
    outs = []
    for salt in (1001, 1002):
        _upload(md, _permuted(sw, salt), gpu_device)
        got = _defrag(md)
        assert md.n == n
        for k in cm.SWARM_KEYS:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (salt, k)
        outs.append(got)
        # in canonical order now: a plan does not sort, and a second sort moves nothing
        st, plan = _plan(md, T_SYN, T_SYN)
        assert st == _lib.JB_COMPLETE and plan.sorted == 0, md.lib.jb_last_error()
        assert _same(_defrag(md), want)
    assert _same(outs[0], outs[1])
    _upload(md, _permuted(sw, 1003), gpu_device)
    st, plan = _plan(md, T_SYN, T_SYN)
    assert st == _lib.JB_COMPLETE and plan.sorted == 1
    assert _same(md.get_swarm(), want)                       # the plan's sort is the same sort

    # every edge size, in one cell and spread over all cells
    for n in EDGE_SIZES:
        for spread in (False, True):
            e = _edge_swarm(mesh, n, spread, salt=7 * n + int(spread))
            want = om.canonical_sort(mesh, md.resident_gids, e, n)
            _upload(md, e, gpu_device)
            got = _defrag(md)
            assert md.n == n
            for k in cm.SWARM_KEYS:
                assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (n, spread, k)
            st, plan = _plan(md, T_SYN, T_SYN)
            assert st == _lib.JB_COMPLETE and plan.sorted == 0, (n, spread)
            if n > 1:
                _upload(md, _permuted(e, 5), gpu_device)
                assert _same(_defrag(md), want), (n, spread)


# ---- 6: the comb does not depend on the slots the photons came in -----------------------------------------
@pytest.mark.parametrize("K", [1, T_SYN], ids=["K=1", "K=T"])
@pytest.mark.parametrize("name", ["1d", "3d"])
def test_comb_does_not_depend_on_slot_order(gpu_device, name, K):
    from jaybenne_amd import _lib
    drv = _driver(name, gpu_device)
    md, mesh = drv.md, drv.mesh
    md.cell_order = "id"
    seed = int(drv.pin.GetOrAddInteger("jaybenne", "seed", 123))
    T = T_SYN
    sw, per = _swarm(mesh, md.resident_gids, SALT[name])
    n = len(sw["w"])
    canon = om.canonical_sort(mesh, md.resident_gids, sw, n)
    want, info = cm.comb_swarm(mesh, md.resident_gids, canon, n, T, K, seed, EPOCH, NEW_IDS, sort=False)
    assert info["cells_combed"] == sum(m > T for m in per) >= 6
    assert min(info["margins"].values()) >= 1e-9           # the model alone leaves no cell out (the choice of SALT)

    runs = []
    for salt in (2001, 2002):
        _upload(md, _permuted(sw, salt), gpu_device)
        st, plan = _plan(md, T, K)
        assert st == _lib.JB_COMPLETE and plan.sorted == 1, md.lib.jb_last_error()
        st, rep = _apply(md, NEW_IDS)
        assert st == _lib.JB_COMPLETE, md.lib.jb_last_error()
        runs.append((md.get_swarm(), bytes(plan), bytes(rep)))
    (g1, plan_b, rep_b), (g2, plan_b2, rep_b2) = runs
    assert _same(g1, g2) and plan_b == plan_b2 and rep_b == rep_b2
    assert (plan.n_after, plan.n_new_ids, plan.cells_combed, plan.max_per_cell) == \
        (info["n_after"], info["n_new_ids"], info["cells_combed"], 3 * SCAN_TILE + 5)
    assert md.n == info["n_after"] == rep.n_after

    # against the model on the model's canonical input: counts per combed cell, unless a last bit decides one
    key0 = info["key"]
    in_slot = {int(v): q for q, v in enumerate(canon["id"])}
    is_new = (g1["id"] >= np.uint64(NEW_IDS)) & (g1["id"] < np.uint64(NEW_IDS + info["n_new_ids"]))
    assert int(is_new.sum()) == info["n_new_ids"]
    first_slot = np.maximum.accumulate(np.where(is_new, -1, np.arange(md.n)))
    assert first_slot.min() >= 0
    origin = np.array([in_slot[int(v)] for v in g1["id"][first_slot]])
    got_k = np.bincount(origin, minlength=n)
    skipped = [k for k, m in info["margins"].items() if m < 1e-9]
    assert len(skipped) <= 0.01 * len(info["margins"])
    for k in info["margins"]:
        if k not in skipped:
            assert np.array_equal(got_k[key0 == k], info["counts"][key0 == k]), int(k)
    if not skipped:      # then the whole output is the model's: survivors, new ids and their streams included
        assert _same(g1, want, [q for q in cm.SWARM_KEYS if q != "w"])
        assert np.allclose(g1["w"], want["w"], rtol=1e-13, atol=0)
    # the survivors are in canonical order again; a further copy sits behind its original (its id is above every
    # old one, so the next sort moves it behind the cell's older photons -- the same way in every run)
    old = {k: g1[k][~is_new] for k in cm.SWARM_KEYS}
    assert om.is_canonical(mesh, md.resident_gids, old, len(old["id"]))
    st, p3 = _plan(md, T, K)
    assert st == _lib.JB_COMPLETE and p3.sorted == (0 if info["n_new_ids"] == 0 else 1)
    assert om.is_canonical(mesh, md.resident_gids, md.get_swarm(), md.n)


# ---- 7: whole runs ----------------------------------------------------------------------------------
# stepdiff in two blocks of eight cells, 20 000 photons (1250 per cell), combed to 32 per cell.  The deck has neither
# emission nor feedback (set again here), so the fields do not depend on the order of the tally's atomic adds.  The
# trigger factor is 1: a cell is combed as soon as it holds MORE than 32 -- after the first comb every cell holds
# exactly 32 and ~10 % of them cross a cell face per cycle (diffusion length sqrt(c dt / 3 sigma) = 0.018 against
# cells of 0.0625), so that some cell gains one in every cycle; with the default factor of 2 only the first cycle
# would comb.
RUN = {"parthenon/mesh/nx1": 16, "parthenon/meshblock/nx1": 8, "jaybenne/num_particles": 20000,
       "jaybenne/do_emission": "false", "jaybenne/do_feedback": "false",
       "jaybenne_amd/census_per_cell_max": 32, "jaybenne_amd/census_comb_trigger": 1.0, "jaybenne_amd/cell_order": "id"}


def _run(device, cycles, **ov):
    from jaybenne_amd import mcblock
    drv = mcblock.McblockDriver(load_deck("stepdiff", dict(RUN, **ov)), device=device)
    drv.pkg.set_arithmetic("exact")
    assert drv.md.cell_order == "id" and (drv.md.comb_target, drv.md.comb_trigger) == (32, 32)
    for _ in range(cycles):
        drv.Step()
    return drv


def _active_global(md, g):
    """the ACTIVE photons of the swarm, the resident block index replaced by the block's global id"""
    act = g["status"] == cm.ST_ACTIVE
    out = {k: g[k][act] for k in cm.SWARM_KEYS}
    out["blk"] = np.asarray(md.resident_gids)[out["blk"]].astype(np.int32)
    return out


def test_runs_do_not_depend_on_when_the_swarm_was_sorted(gpu_device):
    finals = []
    for interval in (0, 1):
        drv = _run(gpu_device, 3, **{"jaybenne/defrag_interval": interval})
        md = drv.md
        assert md.defrag_interval == interval
        assert len(md.comb_history) == 3, md.comb_history          # every cycle combed
        assert all(h["cells_combed"] >= 1 for h in md.comb_history)
        g = md.get_swarm()
        assert len(np.unique(g["id"])) == md.n
        finals.append(_by_id(g))
    assert np.array_equal(finals[0]["id"], finals[1]["id"])
    assert _same(finals[0], finals[1])


# ---- 8: one rank against two ------------------------------------------------------------------------
def _rank_worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import mcblock
        from jaybenne_amd.comm import Comm
        drv = mcblock.McblockDriver(load_deck("stepdiff", RUN), rank=rank, nranks=world, comm=Comm(),
                                    device=torch.device("cuda", 0), capacity_factor=2.0)
        drv.pkg.set_arithmetic("exact")
        assert drv.md.cell_order == "id"
        for _ in range(2):
            drv.Step()
        g = _active_global(drv.md, drv.md.get_swarm())
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), resident=np.asarray(drv.md.resident_gids),
                 owner=np.asarray(drv.mesh.owner), combs=np.array([h["cells_combed"] for h in drv.md.comb_history]),
                 **{k: g[k] for k in cm.SWARM_KEYS})
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_one(gpu_device, tmp_path):
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)])
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    # the precondition: a rank's owned blocks in ascending global id in its resident list, the ranks' id ranges
    # contiguous and in rank order
    owner = parts[0]["owner"]
    assert np.array_equal(owner, parts[1]["owner"]) and np.all(np.diff(owner) >= 0) and set(owner.tolist()) == {0, 1}
    for r, p in enumerate(parts):
        owned = [int(g) for g in p["resident"] if owner[g] == r]
        assert owned == sorted(owned) == np.flatnonzero(owner == r).tolist()
        assert np.all(owner[p["blk"]] == r)                 # census photons live in owned blocks
        assert len(p["combs"]) == 2
    one = _run(gpu_device, 2)
    assert len(one.md.comb_history) == 2
    g = _active_global(one.md, one.md.get_swarm())
    both = {k: np.concatenate([p[k] for p in parts]) for k in cm.SWARM_KEYS}
    assert len(np.unique(both["id"])) == len(both["id"]) == len(g["id"])
    a, b = _by_id(both), _by_id(g)
    assert np.array_equal(a["id"], b["id"])
    for k in cm.SWARM_KEYS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ---- the C++ host -----------------------------------------------------------------------------------
def test_the_cpp_host_honours_the_key(gpu_device, tmp_path):
    """examples/mcblock_amd on the deck of the whole-run tests, the key given on the command line: the photons of
    its final swarm are the Python host's, by id."""
    exe = os.path.join(ROOT, "examples", "mcblock_amd")
    dump = tmp_path / "native.bin"
    args = [f"{k}={v}" for k, v in RUN.items()] + ["parthenon/time/nlim=3", "jaybenne/defrag_interval=0"]
    res = subprocess.run([exe, "-i", os.path.join(DECK_DIR, "stepdiff.in"), "--dump", str(dump)] + args,
                         capture_output=True, text=True, timeout=280, env=dict(os.environ, JB_EXACT_ARITH="1"))
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    cycles = [ln for ln in res.stdout.splitlines() if ln.startswith("cycle=")]
    assert len(cycles) == 3 and all(" combed=0 " not in ln + " " for ln in cycles), cycles
    raw = dump.read_bytes()
    ncell, n, _ = np.frombuffer(raw, dtype=np.int64, count=3)
    off = 24 + 8 * int(ncell)
    ids = np.frombuffer(raw, dtype=np.uint64, count=n, offset=off)
    xs = np.frombuffer(raw, dtype=np.float64, count=n, offset=off + 8 * int(n))
    drv = _run(gpu_device, 3, **{"jaybenne/defrag_interval": 0})
    g = _by_id(drv.md.get_swarm())
    assert n == drv.md.n and np.array_equal(np.sort(ids), g["id"])
    assert np.array_equal(xs[np.argsort(ids)], g["x"])
    res = subprocess.run([exe, "-i", os.path.join(DECK_DIR, "stepdiff.in"), "jaybenne_amd/cell_order=sorted"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and "jaybenne_amd/cell_order" in res.stdout + res.stderr


# ---- 9: the checked library -------------------------------------------------------------------------
def child_checked():
    """(in a child process under the checked library) one comb cycle in the canonical order, then a sweep"""
    import torch
    drv = _run(torch.device("cuda", 0), 1)
    assert drv.md.invariants_enabled()
    return dict(report=drv.md.invariant_report(), sweep=drv.md.verify_swarm(drv.time, drv.time + drv.dt),
                combs=len(drv.md.comb_history), n=drv.md.n, order=drv.md.cell_order)


def test_a_canonical_comb_cycle_runs_clean_under_the_checked_library(gpu_device, checked_lib):
    from test_gpu_invariants import CHECKED
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "checked"], capture_output=True, text=True,
                         env=dict(os.environ, JAYBENNE_AMD_LIB=CHECKED), timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["combs"] == 1 and out["n"] == 16 * 32 and out["order"] == "id"
    for rep in (out["report"], out["sweep"]):
        assert sum(rep["violated"].values()) == 0 and rep["first"] is None, rep
        assert rep["evaluated"]["SWARM"] > 0, rep


if __name__ == "__main__":
    print(json.dumps(globals()["child_" + sys.argv[1]](*sys.argv[2:])))
