"""JB_HANDOFF=step on the GPU: RadiationStep of a block-partitioned mesh as ONE library call per cycle,
jb_radiation_step_ranks (include/jaybenne_amd.h) -- the iterate-sublist of reference jaybenne.cpp:113-131
inside the library.  The ranks share cuda:0 and talk over gloo, as in test_gpu_multirank.py; the union
of their photons must equal the single-process CPU oracle bit for bit, and the step must take the
transport iterations the hand-off driven from Python (JB_HANDOFF=c) takes."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from helpers import load_deck, make_oracle, run_oracle_cycles
from test_gpu_multirank import CASES, FEEDBACK, _deck, _free_port, _read_photon_dumps, _run_workers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_PATH = "c: jb_radiation_step_ranks"


def _driver(pin, rank, world, capacity_factor=2.0, halo_rings=1):
    import torch
    from jaybenne_amd import mcblock
    from jaybenne_amd.comm import Comm
    return mcblock.McblockDriver(pin, rank=rank, nranks=world, comm=Comm(), device=torch.device("cuda", 0),
                                 capacity_factor=capacity_factor, halo_rings=halo_rings)


def _step_worker(rank, world, port, case, outdir, compare_c=False, min_records=None, tight=False):
    """Runs CASES[case] with JB_HANDOFF=step (after a run with JB_HANDOFF=c when compare_c) and saves the
    photons.  tight: the swarm starts with 64 free slots, so the hand-off has to call reserve."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if min_records is not None:
        os.environ["JB_HANDOFF_MIN_RECORDS"] = str(min_records)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c_iterations = -1
        if compare_c:
            os.environ["JB_HANDOFF"] = "c"
            pin, cycles = _deck(case)
            drv = _driver(pin, rank, world)
            for _ in range(cycles):
                assert drv.Step() == drv.jb.TaskStatus.complete
            assert drv.md.handoff_path().startswith("c: jb_exchange"), drv.md.handoff_path()
            c_iterations = drv.md.transport_iterations_total
            drv.md.close()
        os.environ["JB_HANDOFF"] = "step"
        pin, cycles = _deck(case)
        drv = _driver(pin, rank, world)
        md = drv.md
        n0 = md.n
        reserves = []
        if tight:
            md.capacity = md.sv.capacity = md.n + 64      # (the arrays are larger: the library uses less of them)
            grow = md.reserve

            def counting(nslots):
                reserves.append(int(nslots))
                grow(nslots)
            md.reserve = counting
        capacity_rounds = 0
        for _ in range(cycles):
            assert drv.Step() == drv.jb.TaskStatus.complete
            capacity_rounds += md.step_report.capacity_rounds
        assert md.handoff_path().startswith(STEP_PATH), md.handoff_path()
        g = md.get_swarm()
        g["gblk"] = md.gids[g["blk"]]
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), tally=md.get_field("tally"), gids=md.gids,
                 events=np.array([md.events]), sourced=np.array([n0]), outgoing=np.array([md.stats()["n_outgoing"]]),
                 iterations=np.array([md.transport_iterations_total]), c_iterations=np.array([c_iterations]),
                 records=np.array([md.handoff_records]), capacity_rounds=np.array([capacity_rounds]),
                 reserves=np.array([len(reserves)]), **g)
    finally:
        dist.destroy_process_group()


def _step_equals_the_oracle(case, world, tmp_path, **kw):
    from oracle import orc
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_step_worker, args=(r, world, port, case, str(tmp_path)), kwargs=kw)
             for r in range(world)]
    _run_workers(procs)
    pin, cycles = _deck(case)
    O, mesh, _ = make_oracle(pin, orc.MATH_PORTABLE)
    run_oracle_cycles(O, pin, cycles)
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    assert sum(int(p["outgoing"][0]) for p in parts) > 0, "the case must exercise the hand-off"
    assert sum(int(p["records"][0]) for p in parts) > 0
    ids = np.concatenate([p["id"] for p in parts])
    order = np.argsort(ids)
    oo = np.argsort(O.sw["id"][:O.n])
    assert len(ids) == O.n and np.array_equal(ids[order], O.sw["id"][:O.n][oo])
    for k in ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e", "ip", "jp", "kp", "rng"):
        got = np.concatenate([p[k] for p in parts])[order]
        assert np.array_equal(got, O.sw[k][:O.n][oo]), k
    got_blk = np.concatenate([p["gblk"] for p in parts])[order]
    assert np.array_equal(got_blk, O.sw["blk"][:O.n][oo])
    sl = mesh.interior()
    for p in parts:
        np.testing.assert_allclose(p["tally"][sl], O.fields["tally"][p["gids"]][sl], rtol=1e-12, atol=0)
    assert sum(int(p["events"][0]) for p in parts) == O.events
    # moved_anywhere is global: every rank takes the same number of transport iterations
    assert len({int(p["iterations"][0]) for p in parts}) == 1
    return parts


@pytest.mark.parametrize("case", [0, 2, 3, 5, 6, 7, 8, 9])
def test_two_ranks_one_call_per_cycle_equal_the_oracle(gpu_device, case, tmp_path):
    """Two ranks, JB_HANDOFF=step: the photons are the oracle's, and the library's iterate-sublist takes as
    many transport iterations as the hand-off driven from Python (JB_HANDOFF=c, run first in the same ranks)."""
    parts = _step_equals_the_oracle(case, 2, tmp_path, compare_c=True)
    for p in parts:
        assert int(p["iterations"][0]) == int(p["c_iterations"][0]) > 0


@pytest.mark.parametrize("case,world", [(3, 4), (6, 4), (9, 4), (3, 8), (5, 8), (6, 8)])
def test_four_and_eight_ranks_one_call_per_cycle_equal_the_oracle(gpu_device, case, world, tmp_path):
    """4 ranks on the hybrid SMR decks, 8 ranks -- the reference CI's rank count (its SMR decks run on 8 MPI
    ranks) -- on stepdiff_smr_hybrid, the 3-D SMR DDMC mesh of 72 blocks and stepdiff_smr (one card, gloo:
    8 rank processes and the test runner have the GPU open)."""
    _step_equals_the_oracle(case, world, tmp_path)


def test_eight_ranks_with_the_c_hand_off(gpu_device, tmp_path):
    """The existing hand-off (JB_HANDOFF=c: jb_exchange per transport iteration, driven from Python) at 8 ranks."""
    from test_gpu_multirank import _ranks_equal_the_oracle
    _ranks_equal_the_oracle(6, 8, tmp_path)


@pytest.mark.parametrize("case,world", [(3, 2), (6, 4)])
def test_step_grows_its_record_buffers_and_the_swarm(gpu_device, case, world, tmp_path):
    """Record buffers of 16 entries to start with (JB_HANDOFF_MIN_RECORDS) and a swarm with 64 free slots:
    jb_exchange says JB_ERR_CAPACITY on every rank in the same call, the step grows its own buffers, closes
    the holes, calls reserve (md.reserve) and repeats -- the photons are still the oracle's."""
    parts = _step_equals_the_oracle(case, world, tmp_path, min_records=16, tight=True)
    assert all(int(p["capacity_rounds"][0]) > 0 for p in parts)
    assert len({int(p["capacity_rounds"][0]) for p in parts}) == 1       # the same verdicts on every rank
    assert sum(int(p["reserves"][0]) for p in parts) > 0


def _feedback_step_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_HANDOFF="step")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        drv = _driver(load_deck("stepdiff_smr_hybrid", FEEDBACK), rank, world, capacity_factor=8.0)
        assert len(drv.md.resident_gids) > drv.md.nowned        # halo copies are in use
        for _ in range(3):
            assert drv.Step() == drv.jb.TaskStatus.complete
        assert drv.md.handoff_path().startswith(STEP_PATH)
        g = drv.md.get_swarm()
        g["gblk"] = drv.md.gids[g["blk"]]
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), gids=drv.md.gids, u=drv.md.fields["u"].cpu().numpy(),
                 resident=drv.md.resident_gids, tally=drv.md.get_field("tally"), fleck=drv.md.get_field("fleck"), **g)
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_call_per_cycle_with_material_feedback(gpu_device, tmp_path):
    """test_two_ranks_with_material_feedback with JB_HANDOFF=step: emission (blocks_in_call = the blocks a
    rank owns, the oracle's emission_blocks_in_call), stream ids over both ranks' counts, feedback into u and
    the halo refresh between the library calls; the same tolerances."""
    from oracle import orc
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_feedback_step_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    _run_workers(procs)
    pin = load_deck("stepdiff_smr_hybrid", FEEDBACK)
    O, mesh, _ = make_oracle(pin, orc.MATH_PORTABLE, capacity_factor=8.0)
    O.emission_blocks_in_call = mesh.nblocks // 2
    run_oracle_cycles(O, pin, 3)
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    assert all(len(p["gids"]) == mesh.nblocks // 2 for p in parts)
    ids = np.concatenate([p["id"] for p in parts])
    order = np.argsort(ids)
    oo = np.argsort(O.sw["id"][:O.n])
    assert len(ids) == O.n and np.array_equal(ids[order], O.sw["id"][:O.n][oo])
    for k in ("ip", "jp", "kp", "rng"):
        assert np.array_equal(np.concatenate([p[k] for p in parts])[order], O.sw[k][:O.n][oo]), k
    for k in ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e"):
        got = np.concatenate([p[k] for p in parts])[order]
        np.testing.assert_allclose(got, O.sw[k][:O.n][oo], rtol=1e-11, atol=0, err_msg=k)
    sl = mesh.interior()
    for p in parts:
        np.testing.assert_allclose(p["u"], O.fields["u"][p["resident"]], rtol=1e-12, atol=0)
        np.testing.assert_allclose(p["fleck"][sl], O.fields["fleck"][p["gids"]][sl], rtol=1e-12)
        np.testing.assert_allclose(p["tally"][sl], O.fields["tally"][p["gids"]][sl], rtol=1e-11)


def _iterate_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_HANDOFF="step")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pin = load_deck(CASES[3][0], dict(CASES[3][1], **{"jaybenne/max_transport_iterations": 1}))
        drv = _driver(pin, rank, world, halo_rings=0)
        assert len(drv.md.resident_gids) == drv.md.nowned       # no halo copies: every crossing is a hand-off
        n_before, id_before, cycle_before = drv.md.n, drv.md.next_id, drv.md.cycle
        st = drv.Step()
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), status=np.array([int(st)]),
                 iterations=np.array([drv.md.transport_iterations]), events=np.array([drv.md.events]),
                 cycle=np.array([drv.md.cycle - cycle_before]), next_id=np.array([drv.md.next_id - id_before]),
                 n=np.array([n_before]))
    finally:
        dist.destroy_process_group()


def test_iteration_limit_returns_iterate_on_every_rank(gpu_device, tmp_path):
    """max_transport_iterations = 1 without halo copies: the first pass hands photons over, the sublist is
    not done, and EVERY rank gets TaskStatus.iterate from the same call (moved_anywhere is global) -- none is
    left waiting in a collective (the workers would time out)."""
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_iterate_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    _run_workers(procs, timeout=240)
    from jaybenne_amd import jaybenne as jb
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    for p in parts:
        assert int(p["status"][0]) == int(jb.TaskStatus.iterate)
        assert int(p["iterations"][0]) == 1
        assert int(p["events"][0]) == 0            # neither tallied nor counted: the cycle did not finish
        assert int(p["cycle"][0]) == 1


def _one_rank_runs(gpu_device):
    """run(handoff, release=False): two cycles of stepdiff_smr_hybrid on one rank, by jb_radiation_step_ranks
    ("step") or by jb_radiation_step ("c"); release: jb_release_scratch between the two cycles"""
    from jaybenne_amd import _lib, mcblock
    over = dict(CASES[3][1])

    def run(handoff, release=False):
        os.environ["JB_HANDOFF"] = handoff
        try:
            drv = mcblock.McblockDriver(load_deck("stepdiff_smr_hybrid", over), device=gpu_device, capacity_factor=2.0)
        finally:
            os.environ.pop("JB_HANDOFF", None)
        drv.md.defrag_interval = 0
        md = drv.md
        for cycle in range(2):
            if release and cycle == 1:
                md._sync_stream()
                _lib.check(md.lib.jb_release_scratch(md.pkg.ctx))
            if handoff == "step":
                assert drv.Step() == drv.jb.TaskStatus.complete
                assert md.step_report.transport_iterations == 1
                continue
            md._sync_stream()
            nid, cyc = C.c_uint64(md.next_id), C.c_uint32(md.cycle)
            _lib.check(md.lib.jb_radiation_step(md.pkg.ctx, md.handle, C.byref(md.sv), drv.time, drv.dt,
                                                C.byref(nid), C.byref(cyc), md.prefix.data_ptr()))
            md.next_id, md.cycle = int(nid.value), int(cyc.value)
            drv.HostUpdateTasks()
            drv.time += drv.dt
        assert md.handoff_path().startswith(STEP_PATH) == (handoff == "step")
        fields = {k: v.cpu().numpy() for k, v in md.fields.items()}
        return md.get_swarm(), fields, md.next_id, md.cycle

    return run


def test_one_rank_equals_jb_radiation_step(gpu_device):
    """nranks = 1, transport = NULL: jb_radiation_step_ranks is jb_radiation_step -- two cycles of
    stepdiff_smr_hybrid, photons bit for bit (by id), every field to the order of the tally atomics."""
    run = _one_rank_runs(gpu_device)
    sa, fa, ida, ca = run("step")
    sb, fb, idb, cb = run("c")
    assert (ida, ca) == (idb, cb) and ca == 2
    oa, ob = np.argsort(sa["id"]), np.argsort(sb["id"])
    assert len(oa) == len(ob) and np.array_equal(sa["id"][oa], sb["id"][ob])
    for k in sa:
        assert np.array_equal(sa[k][oa], sb[k][ob]), k
    for k in fa:
        np.testing.assert_allclose(fa[k], fb[k], rtol=1e-12, atol=0, err_msg=k)


def test_one_rank_step_after_release_scratch(gpu_device):
    """jb_release_scratch between two cycles lets go of the scratch memory and the step's own buffers: the next
    jb_radiation_step_ranks takes them again and gives the photons of the run that kept them, bit for bit (by id)."""
    run = _one_rank_runs(gpu_device)
    sa, fa, ida, ca = run("step")
    sb, fb, idb, cb = run("step", release=True)
    assert (ida, ca) == (idb, cb) and ca == 2
    oa, ob = np.argsort(sa["id"]), np.argsort(sb["id"])
    assert len(oa) == len(ob) > 0 and np.array_equal(sa["id"][oa], sb["id"][ob])
    for k in sa:
        assert np.array_equal(sa[k][oa], sb[k][ob]), k
    for k in fa:
        np.testing.assert_allclose(fa[k], fb[k], rtol=1e-12, atol=0, err_msg=k)


def test_replicated_view_is_refused_before_any_collective(gpu_device):
    """A replicated mesh (every rank holds every block: one owner in the view) is not driven by the call:
    JB_ERR_INVALID with nranks = 2, and neither collective of the transport is entered."""
    from jaybenne_amd import _lib, mcblock
    from jaybenne_amd import jaybenne as jb
    from jaybenne_amd.mesh import Mesh
    pin = load_deck("stepdiff_smr_hybrid", CASES[3][1])
    mcb = mcblock.Initialize(pin)
    pkg = jb.Initialize(pin, mcb.opacity, mcb.scattering, mcb.eos, device=gpu_device)
    md = jb.MeshData(pkg, Mesh.from_deck(pin), 4096, rank=0, nranks=2, replicated=True)
    calls = []
    tr = _lib.ExchangeTransport()
    tr.all_gather_u64 = _lib.ALL_GATHER_FN(lambda *a: calls.append("all_gather") or 1)
    tr.all_to_all_v = _lib.ALL_TO_ALL_V_FN(lambda *a: calls.append("all_to_all_v") or 1)
    comm = _lib.RankComm(rank=0, nranks=2, transport=C.pointer(tr))
    nid, cyc = C.c_uint64(0), C.c_uint32(0)
    st = md.lib.jb_radiation_step_ranks(pkg.ctx, md.handle, C.byref(md.sv), 0.0, 1e-12, C.byref(nid), C.byref(cyc),
                                        md.prefix.data_ptr(), C.byref(comm), None)
    assert st == _lib.JB_ERR_INVALID
    assert "replicated" in md.lib.jb_last_error().decode()
    assert calls == [] and cyc.value == 0
    md.close()
    pkg.close()


def test_c_level_mpi_one_call_per_cycle(gpu_device, tmp_path):
    """examples/handoff_mpi.cpp with exchange = step: each cycle is ONE call of the C++ mirror,
    jaybenne_amd::RadiationStep(md, t, dt, &transport, rank, nranks), over the program's MPI transport --
    three ranks, with halo copies (2 transport iterations per cycle) and without (dozens); the photons are
    the single-process oracle's bit for bit."""
    from oracle import orc
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec) or not os.path.exists("/opt/conda/lib/libmpi.so"):
        pytest.skip("no MPI installation in this image")
    build = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "mpi"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    ov = {"parthenon/mesh/nx1": 128, "parthenon/meshblock/nx1": 16, "jaybenne/num_particles": 200000}
    O, mesh, _ = make_oracle(load_deck("stepdiff", ov), orc.MATH_PORTABLE)
    run_oracle_cycles(O, load_deck("stepdiff", ov), 3)
    order = np.argsort(O.sw["id"][:O.n])
    per_cycle = {}
    for rings in (1, 0):
        prefix = str(tmp_path / f"photons{rings}")
        run = subprocess.run([mpiexec, "-n", "3", os.path.join(ROOT, "examples", "handoff_mpi"), "16", "8",
                              "200000", "3", str(rings), prefix, "step"], capture_output=True, text=True, timeout=240)
        assert run.returncode == 0 and "HANDOFF OK" in run.stdout, run.stdout + run.stderr
        assert run.stdout.count(" ok") == 3
        per_cycle[rings] = float(re.search(r"\(([0-9.]+) per cycle\)", run.stdout).group(1))
        g = _read_photon_dumps(prefix, 3)
        assert len(g) == O.n
        assert np.array_equal(g["id"], O.sw["id"][:O.n][order])
        for k in ("x", "vx", "t", "w", "rng", "ip"):
            assert np.array_equal(g[k], O.sw[k][:O.n][order]), (rings, k)
        assert np.array_equal(g["gblk"], O.sw["blk"][:O.n][order])
    assert per_cycle[1] == 2.0
    assert per_cycle[0] > 20.0
