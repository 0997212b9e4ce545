"""The checked library on the GPU: libjaybenne_amd_checked.so (make -C jaybenne_amd/csrc checked), the same
sources as the release library with the reference's debug-build transport invariants evaluated on every pass
(jaybenne_amd/csrc/jb_invariants.hpp).  Every run happens in a child process that selects the library through
JAYBENNE_AMD_LIB; clean runs must give the oracle's bits with zero violations, and the SWARM sweep must find
corruptions written through the swarm view.  No transport task ever runs on a corrupted swarm."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900, method="thread")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
CHECKED = os.path.join(ROOT, "jaybenne_amd", "libjaybenne_amd_checked.so")
RELEASE = os.path.join(ROOT, "jaybenne_amd", "libjaybenne_amd.so")
N_PARITY_CASES = 13   # len(test_gpu_parity.CASES), checked by test_parity_case_count


@pytest.fixture(scope="module")
def checked_lib():
    """Built once per session (a no-op when it is up to date); a failed build fails the tests."""
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "jaybenne_amd", "csrc"), "checked"],
                         capture_output=True, text=True, timeout=840)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return CHECKED


def _child(scenario, *args, lib=CHECKED, env=None, timeout=280):
    e = dict(os.environ, JAYBENNE_AMD_LIB=lib)
    for k, v in (env or {}).items():
        if v is None:
            e.pop(k, None)
        else:
            e[k] = v
    res = subprocess.run([sys.executable, os.path.abspath(__file__), scenario, *map(str, args)],
                         capture_output=True, text=True, env=e, timeout=timeout, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def _clean(rep):
    assert sum(rep["violated"].values()) == 0, rep
    assert rep["first"] is None, rep
    assert rep["evaluated"]["SWARM"] > 0, rep


# ---- in the child process ----------------------------------------------------------------------
def _driver(pin):
    import torch
    from jaybenne_amd import mcblock
    drv = mcblock.McblockDriver(pin, device=torch.device("cuda", 0))
    assert drv.md.invariants_enabled() == (os.environ["JAYBENNE_AMD_LIB"] == CHECKED)
    return drv


def _run_against_the_oracle(deck, ov, cycles, compare=True, rho_ramp=False):
    from helpers import load_deck, make_oracle, run_oracle_cycles
    from oracle import orc
    from test_gpu_parity import _compare_fields, _compare_swarm
    pin = load_deck(deck, ov)
    drv = _driver(pin)
    O, mesh, _ = make_oracle(load_deck(deck, ov), orc.MATH_PORTABLE)
    if rho_ramp:   # (as test_gpu_parity: a step record of its own in every cell)
        rho = O.fields["rho"]
        rho *= 1.0 + 0.003 * np.arange(rho.shape[-1])[None, None, None, :]
        O.fields["u"][...] = rho * O.fields["sie"]
        drv.md.set_field("rho", rho)
        drv.md.set_field("u", O.fields["u"])
    for _ in range(cycles):
        drv.Step()       # (raises on a violation under the checked library)
    if compare:
        run_oracle_cycles(O, pin, cycles)
        _compare_swarm(drv.md, O)
        _compare_fields(drv.md, O)
        assert drv.md.events == O.events
    rep = drv.md.invariant_report()
    rep["variant"] = drv.md.lib.jb_last_transport_variant(drv.md.handle).decode()
    return rep


def child_ncases():
    from test_gpu_parity import CASES
    return len(CASES)


def child_deck(i, compare):
    from test_gpu_parity import CASES
    deck, ov, cycles = CASES[int(i)]
    return _run_against_the_oracle(deck, ov, cycles, compare=compare == "1")


def child_class():
    return _run_against_the_oracle("stepdiff_ddmc", {"jaybenne/num_particles": 20000}, 2, rho_ramp=True)


def child_detect():
    import torch
    from helpers import load_deck
    drv = _driver(load_deck("stepdiff_smr", {"jaybenne/num_particles": 6000}))   # (2-D, 2 levels)
    md, mesh = drv.md, drv.mesh
    t0, t1 = drv.time, drv.time + drv.dt
    fill = md.invariant_report()         # the source fill has been swept already
    clean = md.verify_swarm(t0, t1)
    g = md.get_swarm()
    slots = [int(s) for s in np.flatnonzero(g["status"] == 0)[[3, 50, 400, 2000]]]
    a, b, c, d = slots
    saved = {k: md.swarm[k].clone() for k in ("x", "ip", "w", "status")}
    gid = int(md.gids[g["blk"][a]])
    md.swarm["x"][a] = float(mesh.blk_xmax[gid, 0] + 0.5 * mesh.blk_dx[gid, 0])   # outside, blk / ip valid
    ie = mesh.is_[0] + mesh.nx[0] - 1
    md.swarm["ip"][b] = ie + 1                                                     # a ghost cell
    md.swarm["w"][c] = float("nan")
    md.swarm["status"][d] = 7                                                      # undefined
    torch.cuda.synchronize()
    bad = md.verify_swarm(t0, t1)        # (only the sweep: no transport task sees this swarm)
    for k, v in saved.items():
        md.swarm[k].copy_(v)
    torch.cuda.synchronize()
    again = md.verify_swarm(t0, t1)
    return {"fill": fill, "clean": clean, "bad": bad, "again": again, "slots": slots, "n": md.n,
            "ip_b": ie + 1}


def child_c2(cycles):
    import torch
    import bench
    drv = _driver(bench.make_deck(1, 10_000_000))
    times = []
    for _ in range(int(cycles)):
        torch.cuda.synchronize()
        t = time.perf_counter()
        drv.Step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    rep = drv.md.invariant_report() if drv.md.invariants_enabled() else {}
    return {"times": times, "report": rep, "n": drv.md.n}


# ---- the tests ---------------------------------------------------------------------------------
def test_parity_case_count(gpu_device, checked_lib):
    assert _child("ncases", lib=RELEASE) == N_PARITY_CASES


@pytest.mark.parametrize("case", range(N_PARITY_CASES))
def test_parity_cases_bit_exact_with_zero_violations(gpu_device, checked_lib, case):
    """Every deck of test_gpu_parity.CASES, exact arithmetic, under the checked library: the oracle's bits and
    not one violation (SWARM swept at the source fill and on entry to every transport task; DDMC_CLASS after
    every k_ddmc_pack)."""
    rep = _child("deck", case, "1")
    _clean(rep)
    if "cell codes" in rep["variant"]:
        assert rep["evaluated"]["DDMC_CLASS"] > 0, rep
    if rep["variant"].startswith("TransportPhotons: k_transport") or "k_transport<" in rep["variant"]:
        assert rep["passes"]["transport"] > 0, rep


def _families(variant):
    """The kernel families a transport variant string names (jb_last_transport_variant)."""
    fam = set()
    if "k_transport" in variant:
        fam.add("transport")
    if "k_imc_cell" in variant:
        fam.add("imc_cell")
    if "k_hybrid" in variant:
        fam.add("hybrid")
    if "k_ddmc_all" in variant:
        fam.add("ddmc_q" if "queues" in variant else "ddmc_all")
    return fam


VARIANTS = [
    # (CASES index, environment, compare with the oracle (False: lean arithmetic, held to its tolerance elsewhere),
    #  the family that must have run checked)
    (0, {"JB_NO_IMC_CELL": "1"}, True, "transport"),                     # exact x-space IMC kernel
    (7, {"JB_NO_IMC_CELL": "1"}, True, "transport"),                     # ... 3-D
    (0, {"JB_NO_IMC_CELL": "1", "JB_EXACT_ARITH": None}, False, "transport"),   # lean arithmetic, x-space
    (0, {"JB_EXACT_ARITH": None}, False, "imc_cell"),                    # lean: the cell-local IMC kernel
    (7, {"JB_EXACT_ARITH": None}, False, "imc_cell"),                    # ... 3-D
    (2, {"JB_NO_DDMC_ALL": "1"}, True, "hybrid"),                        # all-DDMC mesh on k_hybrid
    (4, {"JB_DDMC_QUEUES": "0"}, True, "ddmc_all"),
    (4, {"JB_COOP_GATHER": "1"}, True, None),
    (4, {"JB_COOP_GATHER": "2"}, True, None),
    (4, {}, True, None),
    (2, {}, True, None),
    (5, {}, True, "hybrid"),                                             # 2-D hybrid
    (5, {"JB_EXACT_ARITH": None}, False, "hybrid"),                      # ... lean: its cell-local IMC loop
]


@pytest.mark.parametrize("case,env,compare,family", VARIANTS)
def test_kernel_selection_variants_with_zero_violations(gpu_device, checked_lib, case, env, compare, family):
    """Zero violations, and every kernel family the launch names ran its per-pass checks (pass counts > 0)."""
    rep = _child("deck", case, "1" if compare else "0", env=env)
    _clean(rep)
    fams = _families(rep["variant"])
    assert fams, rep["variant"]
    if family is not None:
        assert family in fams, rep["variant"]
    for f in fams:
        assert rep["passes"][f] > 0, (f, rep)
    assert rep["evaluated"]["INDEX"] >= sum(rep["passes"][f] for f in fams), rep


def test_every_tracking_family_runs_checked(gpu_device, checked_lib):
    """Over a handful of decks and switches, each of the five tracking families ran checked at least once."""
    seen = set()
    for case, env in ((0, {"JB_NO_IMC_CELL": "1"}), (0, {"JB_EXACT_ARITH": None}), (2, {"JB_NO_DDMC_ALL": "1"}),
                      (4, {"JB_DDMC_QUEUES": "0"}), (4, {}), (2, {})):
        rep = _child("deck", case, "0", env=env)
        _clean(rep)
        seen |= {f for f in ("transport", "imc_cell", "ddmc_all", "ddmc_q", "hybrid") if rep["passes"][f] > 0}
    assert seen == {"transport", "imc_cell", "ddmc_all", "ddmc_q", "hybrid"}, seen


@pytest.mark.parametrize("max_classes", [None, "64"])
def test_ddmc_class_records_equal_the_cells_own(gpu_device, checked_lib, max_classes):
    """A step record of its own in every cell (128 classes), with and without JB_DDMC_MAX_CLASSES overflow:
    every cell whose code is a class number has that class's record bit for bit."""
    rep = _child("class", env={"JB_DDMC_MAX_CLASSES": max_classes})
    _clean(rep)
    assert rep["evaluated"]["DDMC_CLASS"] > 0, rep
    if max_classes is not None:    # (the cells past the 64th class carry the overflow code: not evaluated)
        assert rep["evaluated"]["DDMC_CLASS"] < rep["passes"]["ddmc_class"], rep
    else:
        assert rep["evaluated"]["DDMC_CLASS"] == rep["passes"]["ddmc_class"], rep


def test_swarm_sweep_finds_corruptions(gpu_device, checked_lib):
    """Four photons corrupted through the swarm view after a clean source fill -- x outside its block, ip one
    past the interior (a ghost cell), w = NaN, an undefined status -- are four SWARM violations of
    jb_verify_swarm, the first record names one of them, and the restored swarm is clean again."""
    r = _child("detect")
    _clean(r["fill"])
    _clean(r["clean"])
    assert r["clean"]["evaluated"]["SWARM"] == r["n"]
    bad = r["bad"]
    assert bad["violated"]["SWARM"] == 4, bad
    assert sum(bad["violated"].values()) == 4, bad
    assert bad["evaluated"]["SWARM"] == r["n"]
    # (the record is the violation that won the claim -- one of the four, not necessarily the lowest slot)
    first = bad["first"]
    assert first is not None and first["kind"] == "SWARM" and first["family"] == "swarm", bad
    assert first["slot"] in r["slots"], bad
    if first["slot"] == r["slots"][1]:
        assert first["ijk"][0] == r["ip_b"], bad
    again = r["again"]
    assert sum(again["violated"].values()) == 0 and again["first"] is None, again


def _rank_worker(rank, world, port, case, outdir, corrupt):
    """One rank of a JB_HANDOFF=step run under the checked library: statuses of its steps and its report.
    corrupt: rank 0 moves one resident photon's time past the end of the cycle before the first step -- a SWARM
    violation on that rank only, harmless to track (the photon is at census at once)."""
    import torch.distributed as dist
    from jaybenne_amd import _lib
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_HANDOFF="step")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from test_gpu_multirank import _deck
        from test_gpu_rank_step import _driver
        pin, cycles = _deck(case)
        drv = _driver(pin, rank, world)
        md = drv.md
        out = {"enabled": md.invariants_enabled(), "path": _lib.LIB_PATH, "status": []}
        if corrupt and rank == 0:
            g = md.get_swarm()
            s = int(np.flatnonzero(g["status"] == 0)[0])
            md.swarm["t"][s] = drv.time + 2.0 * drv.dt
        for _ in range(cycles):
            try:
                out["status"].append(int(drv.Step()))
            except _lib.JaybenneError as e:
                out["status"].append(int(e.status))
                out["error"] = str(e)
                break
        out["report"] = md.invariant_report()
        with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
            json.dump(out, f)
    finally:
        dist.destroy_process_group()


def _run_ranks(tmp_path, corrupt, monkeypatch):
    import torch.multiprocessing as mp
    monkeypatch.setenv("JAYBENNE_AMD_LIB", CHECKED)
    sys.path.insert(0, TESTS)
    from test_gpu_multirank import CASES, _free_port, _run_workers
    case = next(i for i, c in enumerate(CASES) if c[0] == "stepdiff_smr_hybrid")
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, case, str(tmp_path), corrupt)) for r in range(2)]
    _run_workers(procs)
    return [json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)]


def test_two_rank_step_run_with_the_checked_library(gpu_device, checked_lib, tmp_path, monkeypatch):
    """JB_HANDOFF=step on stepdiff_smr_hybrid, two ranks under the checked library: every step completes on both
    ranks with zero violations, SampleDDMCBlockFace ran its FACE_SAMPLE check, and the photons are the oracle's."""
    parts = _run_ranks(tmp_path, False, monkeypatch)
    for p in parts:
        assert p["enabled"] and p["path"] == CHECKED, p
        assert p["status"] and all(s == 0 for s in p["status"]), p
        rep = p["report"]
        assert sum(rep["violated"].values()) == 0 and rep["first"] is None, rep
    assert sum(p["report"]["passes"]["block_face"] for p in parts) > 0, parts
    assert sum(p["report"]["evaluated"]["FACE_SAMPLE"] for p in parts) > 0, parts
    from test_gpu_rank_step import _step_equals_the_oracle
    (tmp_path / "oracle").mkdir()
    _step_equals_the_oracle(next(i for i, c in enumerate(__import__("test_gpu_multirank").CASES)
                                 if c[0] == "stepdiff_smr_hybrid"), 2, tmp_path / "oracle")


def test_a_violation_on_one_rank_stops_both_in_the_same_call(gpu_device, checked_lib, tmp_path, monkeypatch):
    """A SWARM violation on rank 0 only: jb_exchange carries it in rank 0's row of its all-gather, and both ranks
    return JB_ERR_INVARIANT from the same step -- neither is left waiting in a collective."""
    from jaybenne_amd import _lib
    parts = _run_ranks(tmp_path, True, monkeypatch)
    assert parts[0]["status"] == parts[1]["status"] == [_lib.JB_ERR_INVARIANT], parts
    assert parts[0]["report"]["violated"]["SWARM"] >= 1, parts[0]
    assert sum(parts[1]["report"]["violated"].values()) == 0, parts[1]


def test_c2_one_cycle_of_ten_million_photons(gpu_device, checked_lib):
    """BASELINE configs[1] (C2) at 1e7 photons, one cycle: zero violations.  The cycle time is printed next
    to the release library's, not asserted."""
    lean = {"JB_EXACT_ARITH": None}
    chk = _child("c2", 1, env=lean)
    rel = _child("c2", 1, lib=RELEASE, env=lean)
    rep = chk["report"]
    assert sum(rep["violated"].values()) == 0 and rep["first"] is None, rep
    assert rep["evaluated"]["SWARM"] >= chk["n"]
    print(f"C2 1e7 photons, one cycle: checked {chk['times'][0] * 1e3:.1f} ms, "
          f"release {rel['times'][0] * 1e3:.1f} ms")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    print(json.dumps(globals()["child_" + sys.argv[1]](*sys.argv[2:])))
