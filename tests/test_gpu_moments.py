"""Radiation moments on the GPU (jb_evaluate_radiation_moments: k_mom_chunks, k_mom_cells) against
tests/moments_model.py bit for bit on crafted swarms -- tests/test_moments_host.py shows that the swarms hold the
cases --, the call's invariances (slot order, a second call, everything else untouched), deck runs against the
energy tally, the ledger and the identities of an isotropic field, the two command-line hosts, and two ranks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import moments_model as mm
import swarm_ops_model as som
from helpers import DECK_DIR, ROOT, load_deck

from test_gpu_comb import _upload
from test_gpu_swarm_ops import _check, _download

pytestmark = pytest.mark.gpu

NP = "jaybenne/num_particles"
PLANS = mm.run_plans()
GROUPS = ("1", "8", "64")          # JB_MOMENTS_GROUP: lanes per cell of k_mom_cells, beside the host's own choice


@pytest.fixture(scope="module")
def views(gpu_device):
    """(driver, Geom) per (mesh, rank, nranks), made once"""
    from jaybenne_amd import mcblock
    made = {}

    def get(case, rank=0, nranks=1):
        key = (repr(case), rank, nranks)
        if key not in made:
            drv = mcblock.McblockDriver(load_deck(*case), rank=rank, nranks=nranks, comm=None, device=gpu_device)
            md = drv.md
            assert md.cell_order == "any" and md.deposition == "atomic"
            g = som.Geom(drv.mesh, md.resident_gids, md.field_owner, md.nowned)
            _, h = som.host_view(case, rank, nranks)
            assert np.array_equal(g.gids, h.gids) and g.nowned == h.nowned and np.array_equal(g.dx, h.dx)
            made[key] = (drv, g)
        return made[key]

    yield get
    for drv, _ in made.values():
        drv.md.cell_order = "any"
        drv.md.close()
    made.clear()


def _moments(md, group=None, report=True):
    """(fields [12, nblocks, nx3, nx2, nx1] on the host, report) of one call; the output array is filled with NaN
    first: every word must be written"""
    import torch
    from jaybenne_amd import _lib
    nx = md.mesh.nx
    out = torch.full((_lib.JB_MOMENTS, md.nblocks, int(nx[2]), int(nx[1]), int(nx[0])), float("nan"),
                     dtype=torch.float64, device=md.device)
    assert out.numel() == md.lib.jb_moments_words(md.handle)
    rep = _lib.MomentsReport()
    md._sync_stream()
    if group is None:
        os.environ.pop("JB_MOMENTS_GROUP", None)
    else:
        os.environ["JB_MOMENTS_GROUP"] = group
    try:
        st = md.lib.jb_evaluate_radiation_moments(md.pkg.ctx, md.handle, C.byref(md.sv), out.data_ptr(),
                                                  C.byref(rep) if report else None)
    finally:
        os.environ.pop("JB_MOMENTS_GROUP", None)
    _check(md, st)
    torch.cuda.synchronize(md.device)
    return out.cpu().numpy(), rep.as_dict()


def _against_the_model(md, g, sw, what):
    """uploads sw, calls, and holds fields and report to the model on the swarm as the call left it"""
    n = len(sw["id"])
    _upload(md, sw, md.device)
    got, rep = _moments(md)
    after = _download(md, n)
    assert som.sorted_failures(g, sw, after, n) == [], what          # the same photons, in key order
    want, want_rep = mm.moments(g, after, n)
    assert mm.differing_components(got, want) == [], what
    assert rep == dict(want_rep, sorted=0 if mm.in_order(g, sw, n) else 1), (what, rep, want_rep)
    return got, after


# ---- crafted swarms, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("plan", range(len(PLANS)), ids=[f"{p[0]}-{p[1]}" for p in PLANS])
def test_runs_equal_the_model(gpu_device, views, plan):
    """runs of 1, 2, 63, 64, 65, 4095, 4096, 4097, 2 x 4096 + 1 slots at every lane offset and one cell of
    3 x 4096 + 5, given unsorted with other statuses and bad blks among them; then the sorted swarm again under
    every group width: the same bits, and the call does not sort"""
    name, mesh, lengths = PLANS[plan]
    drv, g = views(mm.mesh_cases()[mesh])
    sw, _ = mm.run_swarm(g, lengths)
    got, after = _against_the_model(drv.md, g, sw, name)
    assert np.nanmax(got[0]) == max(lengths)
    for group in GROUPS:
        again, rep = _moments(drv.md, group)
        assert mm.differing_components(again, got) == [] and rep["sorted"] == 0, (name, group)
    assert som.differing(_download(drv.md, len(sw["id"])), after) == []        # a sorted swarm is not moved


@pytest.mark.parametrize("mesh", ["1d", "2d", "3d"])
def test_hashed_swarm_equals_the_model(gpu_device, views, mesh):
    """hashed cells, photons clamped into ghost cells, hashed statuses and bad blks"""
    drv, g = views(mm.mesh_cases()[mesh])
    for n in (1, 65, 20011):
        got, _ = _against_the_model(drv.md, g, mm.hashed_swarm(g, n, mm.SALT + n), (mesh, n))
    for group in GROUPS:
        again, _ = _moments(drv.md, group)
        assert mm.differing_components(again, got) == [], (mesh, group)


def test_halo_copies_get_zeros(gpu_device, views):
    drv, g = views(som.RANK_MESH, 1, 2)
    assert g.nowned < g.nblocks
    got, after = _against_the_model(drv.md, g, mm.hashed_swarm(g, 3000), "halo")
    assert not got[:, g.nowned:].any() and got[0].sum() > 500
    assert int(((after["status"] == som.ST_ACTIVE) & (after["blk"] >= g.nowned) & (after["blk"] < g.nblocks)).sum()) > 10


def test_empty_swarm_and_one_photon_in_the_last_cell(gpu_device, views):
    drv, g = views(mm.mesh_cases()["3d"])
    md = drv.md
    md.sv.n = 0
    got, rep = _moments(md)
    assert not got.any() and not np.isnan(got).any()
    assert rep == dict(n_counted=0, n_skipped=0, cells_nonempty=0, longest_run=0, sorted=0)
    got, rep = _moments(md, report=False)
    assert not got.any() and not np.isnan(got).any()
    sw, cells = mm.run_swarm(g, [1], extras=0, first_cell=g.nblocks * g.ncell - 1)
    got, _ = _against_the_model(md, g, sw, "one photon")
    assert got[0, -1, -1, -1, -1] == 1.0 and got[0].sum() == 1.0 and got[1, -1, -1, -1, -1] > 0


def test_null_arguments_are_refused(gpu_device, views):
    from jaybenne_amd import _lib
    drv, g = views(mm.mesh_cases()["1d"])
    md = drv.md
    md._sync_stream()
    rep = _lib.MomentsReport()
    f = md.lib.jb_evaluate_radiation_moments
    assert f(md.pkg.ctx, md.handle, C.byref(md.sv), None, C.byref(rep)) == _lib.JB_ERR_INVALID
    assert f(md.pkg.ctx, None, C.byref(md.sv), None, C.byref(rep)) == _lib.JB_ERR_INVALID
    assert f(None, md.handle, C.byref(md.sv), None, None) == _lib.JB_ERR_INVALID
    assert md.lib.jb_moments_words(md.handle) == 12 * g.nblocks * g.ncell


# ---- the sort, the comb and the moments in one scratch memory ---------------------------------------------
# One context runs a defrag sort, a comb plan + apply and a moments evaluation: the three share the library's scratch
# memory (jaybenne_amd/csrc/jb_scratch_layout.hpp).  A mesh of 13 histogram bins and one of 2054 -- more than a scan
# tile of 2048 --, swarm sizes on both sides of a scan tile and of a moments chunk, odd and even (the 4-byte arrays
# are packed in pairs), both cell orders: each call against its numpy model.
NX1, MB1 = "parthenon/mesh/nx1", "parthenon/meshblock/nx1"
TILE_MESHES = {"8 cells": ("stepdiff", {NX1: 8, MB1: 8, NP: 64}), "2049 cells": ("stepdiff", {NX1: 2049, MB1: 2049, NP: 64})}
TILE_COMB = {"8 cells": (70, 32), "2049 cells": (3, 2)}          # (T, K): some 260 | 1 .. 2 photons per cell
TILE_N = (2047, 2048, 2049, 4097)


def _tile_swarm(mesh, n):
    """n ACTIVE photons with hashed ids in hashed cells (tests/test_gpu_cell_order.py), one in 97 forty times as
    heavy: on the coarse mesh the comb keeps several copies of some"""
    from test_gpu_cell_order import _edge_swarm
    sw = _edge_swarm(mesh, n, True, salt=11 * n)
    sw["w"][::97] *= 40.0
    return sw


def _sort_comb_moments(drv, g, name, n, order, device):
    import comb_model as cm
    from jaybenne_amd import _lib
    from test_gpu_cell_order import NEW_IDS
    from test_gpu_comb import EPOCH, _apply, _plan, _same
    from test_gpu_swarm_ops import _defrag
    md, mesh = drv.md, drv.mesh
    what = (name, n, order)
    T, K = TILE_COMB[name]
    seed = int(drv.pin.GetOrAddInteger("jaybenne", "seed", 123))
    sw = _tile_swarm(mesh, n)
    canon = mm.canonical(g, sw, n)
    assert not mm.in_order(g, sw, n)
    # the sort
    _upload(md, sw, device)
    _defrag(md)
    got = _download(md, n)
    assert md.n == n and som.sorted_failures(g, sw, got, n) == [], what
    if order == "id":
        assert som.differing(got, canon) == [], what
    # the comb: the plan sorts; the model works on the swarm as the plan left it
    _upload(md, mm.shuffle(sw, 3), device)
    st, plan = _plan(md, T, K)
    assert st == _lib.JB_COMPLETE and plan.sorted == 1, (what, md.lib.jb_last_error())
    g0 = _download(md, n)
    assert som.sorted_failures(g, sw, g0, n) == [], what
    if order == "id":
        assert som.differing(g0, canon) == [], what
    want, info = cm.comb_swarm(mesh, md.resident_gids, g0, n, T, K, seed, EPOCH, NEW_IDS, sort=False)
    assert info["cells_combed"] > 0 and min(info["margins"].values()) >= 1e-9, what
    assert (plan.n_before, plan.n_after, plan.n_new_ids, plan.cells_combed, plan.max_per_cell) == \
        (n, info["n_after"], info["n_new_ids"], info["cells_combed"], info["max_per_cell"]), what
    st, rep = _apply(md, NEW_IDS)
    assert st == _lib.JB_COMPLETE and (rep.n_after, rep.n_new_ids) == (plan.n_after, plan.n_new_ids), what
    assert md.n == info["n_after"]
    g1 = _download(md, md.n)
    assert _same(g1, want, [q for q in cm.SWARM_KEYS if q != "w"]), what
    assert np.allclose(g1["w"], want["w"], rtol=1e-13, atol=0), what     # (W of a cell by two orders of summation)
    # the moments: the call sorts
    _, after = _against_the_model(md, g, mm.shuffle(sw, 5), what)
    if order == "id":
        assert som.differing(after, canon) == [], what


@pytest.mark.parametrize("order", ["any", "id"])
@pytest.mark.parametrize("n", TILE_N)
@pytest.mark.parametrize("name", list(TILE_MESHES))
def test_sort_comb_and_moments_share_one_scratch(gpu_device, views, name, n, order):
    drv, g = views(TILE_MESHES[name])
    drv.md.cell_order = order
    try:
        _sort_comb_moments(drv, g, name, n, order, gpu_device)
    finally:
        drv.md.cell_order = "any"


def test_the_scratch_changes_hands(gpu_device, views):
    """A comb plan lies in the scratch memory until it is applied: a moments evaluation in between, or
    jb_release_scratch, takes the memory -- the apply then finds no plan.  After the release the three calls work
    as before."""
    from jaybenne_amd import _lib
    from test_gpu_comb import _apply, _plan
    name, n = "8 cells", 2049
    drv, g = views(TILE_MESHES[name])
    md = drv.md
    T, K = TILE_COMB[name]
    for taker in ("moments", "release"):
        _upload(md, _tile_swarm(drv.mesh, n), gpu_device)
        st, plan = _plan(md, T, K)
        assert st == _lib.JB_COMPLETE and plan.n_after < n, md.lib.jb_last_error()
        if taker == "moments":
            _moments(md)
        else:
            md._sync_stream()
            _check(md, md.lib.jb_release_scratch(md.pkg.ctx))
        st, _ = _apply(md)
        assert st == _lib.JB_ERR_INVALID and b"no plan for this swarm" in md.lib.jb_last_error(), taker
        assert md.n == n
    _sort_comb_moments(drv, g, name, n, "any", gpu_device)


# ---- slot order -------------------------------------------------------------------------------------------
def _mixed(g):
    return mm.run_swarm(g, [65, 4097, 1, 2 * mm.CHUNK + 1, 64, 700, 2, 63], extras=mm.EXTRAS)


def test_any_order_two_slot_orders_that_keep_each_cells_order(gpu_device, views):
    """JB_CELL_ORDER_ANY: the same photons in key order with the slots that are not counted arranged in two ways,
    and with photons put into an earlier cell (every later cell then starts at another slot): the same bits cell by
    cell, and neither call sorts"""
    drv, g = views(mm.mesh_cases()["1d"])
    md = drv.md
    assert md.cell_order == "any"
    sw, cells = _mixed(g)
    n = len(sw["id"])
    a = mm.canonical(g, sw, n)
    tail = n - mm.EXTRAS
    b = som.take(a, np.concatenate((np.arange(tail), np.arange(n - 1, tail - 1, -1))))
    assert som.differing(a, b) != [] and mm.in_order(g, a, n) and mm.in_order(g, b, n)
    out = []
    for s in (a, b):
        _upload(md, s, gpu_device)
        got, rep = _moments(md)
        assert rep["sorted"] == 0 and som.differing(_download(md, n), s) == []
        out.append(got)
    assert mm.differing_components(out[0], out[1]) == []
    assert mm.differing_components(out[0], mm.moments(g, a, n)[0]) == []
    for extra in (1, 63, 1000):
        more, _ = mm.run_swarm(g, [extra], salt=mm.SALT + extra, extras=0, first_cell=1)
        both = mm.canonical(g, {k: np.concatenate((more[k], a[k])) for k in som.KEYS}, n + extra)
        _upload(md, both, gpu_device)
        got, rep = _moments(md)
        flat_a, flat_g = out[0].reshape(12, -1), got.reshape(12, -1)
        assert rep["sorted"] == 0 and flat_g[0, 1] == extra
        assert mm.same_bits(flat_a[:, cells], flat_g[:, cells]), extra


def test_by_id_any_permutation_gives_the_same_bits(gpu_device, views):
    drv, g = views(mm.mesh_cases()["2d"])
    md = drv.md
    sw, _ = _mixed(g)
    n = len(sw["id"])
    want, want_rep = mm.moments(g, mm.canonical(g, sw, n), n)
    md.cell_order = "id"
    try:
        for salt in (1, 2, 3):
            _upload(md, mm.shuffle(sw, salt), gpu_device)
            got, rep = _moments(md)
            assert mm.differing_components(got, want) == [], salt
            assert rep == dict(want_rep, sorted=1)
            assert som.differing(_download(md, n), mm.canonical(g, sw, n)) == []
        got, rep = _moments(md)                                            # in canonical order already
        assert mm.differing_components(got, want) == [] and rep["sorted"] == 0
    finally:
        md.cell_order = "any"


def test_everything_else_is_untouched(gpu_device, views):
    """energy_tally, energy_delta and the multiset of photons by id are bit-identical before and after"""
    import torch
    drv, g = views(mm.mesh_cases()["3d"])
    md = drv.md
    sw = mm.hashed_swarm(g, 20011, mm.SALT + 5)
    _upload(md, sw, gpu_device)
    marks = {}
    for q, name in enumerate(("tally", "edelta")):
        base = som.edelta_base(g, 11 + q)
        md.set_field(name, base, local=True)
        marks[name] = base
    _moments(md)
    torch.cuda.synchronize(md.device)
    for name, base in marks.items():
        assert np.array_equal(md.fields[name].cpu().numpy().view(np.uint64), base.view(np.uint64)), name
    assert md.n == 20011 and som.same_multiset(_download(md, 20011), sw) == []


# ---- deck runs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deck", ["inf", "stepdiff", "stepdiff_smr"])
def test_deck_run_agrees_with_tally_ledger_and_isotropy(gpu_device, deck):
    from jaybenne_amd import jaybenne as jb, mcblock
    from test_moments_host import domain_isotropy
    drv = mcblock.McblockDriver(load_deck(deck, {NP: 20000}), device=gpu_device, ledger=True, capacity_factor=4.0)
    md = drv.md
    try:
        drv.pkg.set_arithmetic("exact")
        for _ in range(2):
            drv.Step()
        c = drv.pkg.Param("speed_of_light")
        fields, rep = jb.EvaluateRadiationMoments(md)
        assert fields is md.moments and rep == md.moments_report
        m = fields.cpu().numpy()
        sw = md.get_swarm()
        act = sw["status"] == som.ST_ACTIVE
        assert m[0].sum() == act.sum() == rep["n_counted"] > 10000 and rep["n_skipped"] == md.n - rep["n_counted"]
        tally = np.asarray(md.get_field("tally"))[drv.mesh.interior()]
        assert tally.shape == m[1].shape
        assert np.abs(m[1] - tally).max() <= 1e-12 * tally.max()
        dx = np.asarray(drv.mesh.blk_dx)[md.resident_gids]
        integ = mm.integrals(m, dx)
        e_census = md.ledger["e_census"]
        print(deck, "sum E dv / e_census - 1 =", integ[1] / e_census - 1.0)
        assert abs(integ[1] - e_census) <= 1e-12 * e_census
        if not drv.pkg.Param("use_ddmc"):                      # |v| = c in every photon: the trace of Q is c^2 E
            E, trace = m[1], m[6] + m[9] + m[11]
            full = m[0] > 0
            assert full.sum() == rep["cells_nonempty"]
            assert np.all(np.abs(trace[full] - c * c * E[full]) <= 1e-12 * c * c * E[full])
        print(deck, end=" ")
        assert domain_isotropy(sw, act, c, report=True)
        # N_eff of the domain from the fields is that of the photons
        neff = integ[1] ** 2 / integ[2]
        w = sw["w"][act]
        assert abs(neff - w.sum() ** 2 / (w * w).sum()) <= 1e-9 * neff
    finally:
        md.close()


# ---- the command-line hosts ---------------------------------------------------------------------------------------
def test_both_hosts_write_the_same_lines(gpu_device, tmp_path):
    """``--moments FILE`` on one short inf run, in the canonical cell order and with exact deposition so that the run
    is a function of the deck alone: the files agree line for line; the deck key alone writes moments.jsonl"""
    import json
    exe = os.path.join(ROOT, "examples", "mcblock_amd")
    assert os.path.exists(exe), "examples/mcblock_amd has not been built (__graft_entry__.build())"
    ov = {NP: 4000, "parthenon/time/tlim": 2.5e-12, "jaybenne_amd/cell_order": "id", "jaybenne_amd/deposition": "exact"}
    args = ["-i", os.path.join(DECK_DIR, "inf.in")] + [f"{k}={v}" for k, v in ov.items()]
    env = dict(os.environ, JB_EXACT_ARITH="1")
    runs = {"py": [sys.executable, "-m", "jaybenne_amd"], "cc": [exe]}
    for name, cmd in runs.items():
        res = subprocess.run(cmd + args + ["--moments", str(tmp_path / f"{name}.jsonl")], capture_output=True, text=True,
                             env=env, timeout=240, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        assert res.stdout.count(" eddington=[") == 3, res.stdout
    py, cc = (open(tmp_path / f"{name}.jsonl").read().splitlines() for name in runs)
    assert len(py) == 3 and py == cc, (py, cc)
    for q, line in enumerate(py):
        rec = json.loads(line)
        assert rec["cycle"] == q + 1 and rec["n"] == rec["n_counted"] > 4000 and rec["sorted"] == 1
        assert all(abs(e - 1 / 3) < 0.05 for e in rec["eddington"]) and abs(sum(rec["eddington"]) - 1) < 1e-12
    # off by default, and on by the deck key
    res = subprocess.run(runs["cc"] + args + ["jaybenne_amd/moments=true"], capture_output=True, text=True, env=env,
                         timeout=240, cwd=str(tmp_path))
    assert res.returncode == 0 and open(tmp_path / "moments.jsonl").read().splitlines() == cc
    res = subprocess.run(runs["cc"] + args, capture_output=True, text=True, env=env, timeout=240, cwd=str(tmp_path))
    assert res.returncode == 0 and " eddington=[" not in res.stdout


# ---- two ranks ------------------------------------------------------------------------------------------------------
RUN = {"parthenon/mesh/nx1": 16, "parthenon/meshblock/nx1": 8, NP: 20000, "jaybenne/do_emission": "false",
       "jaybenne/do_feedback": "false", "jaybenne_amd/cell_order": "id"}


def _rank_worker(rank, world, port, outdir, decomposition):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import jaybenne as jb, mcblock
        from jaybenne_amd.comm import Comm
        drv = mcblock.McblockDriver(load_deck("stepdiff", RUN), rank=rank, nranks=world, comm=Comm(),
                                    device=torch.device("cuda", 0), capacity_factor=2.0, decomposition=decomposition)
        drv.pkg.set_arithmetic("exact")
        for _ in range(2):
            drv.Step()
        fields, rep = jb.EvaluateRadiationMoments(drv.md)
        np.savez(os.path.join(outdir, f"{decomposition}{rank}.npz"), resident=np.asarray(drv.md.resident_gids),
                 owner=np.asarray(drv.mesh.owner), nowned=drv.md.nowned, fields=fields.cpu().numpy(),
                 counted=rep["n_counted"])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("decomposition", ["blocks", "replicated"])
def test_two_ranks_equal_one(gpu_device, tmp_path, decomposition):
    """stepdiff in two blocks, canonical cell order.  Block partition: each rank's owned cells have the one-rank
    run's bits (and its halo copy zeros).  Replicated mesh: the ranks' sums agree with it to 1e-12 of a component's
    largest entry, the counts exactly."""
    import torch.multiprocessing as mp
    from jaybenne_amd import jaybenne as jb, mcblock
    from test_gpu_multirank import _free_port, _run_workers
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path), decomposition)) for r in range(2)])
    parts = [np.load(tmp_path / f"{decomposition}{r}.npz") for r in range(2)]
    drv = mcblock.McblockDriver(load_deck("stepdiff", RUN), device=gpu_device)
    try:
        drv.pkg.set_arithmetic("exact")
        for _ in range(2):
            drv.Step()
        fields, rep = jb.EvaluateRadiationMoments(drv.md)
        one = fields.cpu().numpy()
    finally:
        drv.md.close()
    assert one.shape[1] == 2 and rep["n_counted"] > 10000
    if decomposition == "blocks":
        assert sum(int(p["counted"]) for p in parts) == rep["n_counted"]
        for r, p in enumerate(parts):
            nowned, resident = int(p["nowned"]), p["resident"]
            assert nowned == 1 and len(resident) == 2 and p["owner"][resident[0]] == r
            assert mm.differing_components(p["fields"][:, :1], one[:, resident[:1]]) == [], r
            assert not p["fields"][:, 1:].any()
    else:
        for p in parts:
            assert int(p["counted"]) == rep["n_counted"] and np.array_equal(p["fields"][0], one[0])
            for q in range(12):
                assert np.abs(p["fields"][q] - one[q]).max() <= 1e-12 * np.abs(one[q]).max(), mm.NAMES[q]
        assert mm.differing_components(parts[0]["fields"], parts[1]["fields"]) == []
