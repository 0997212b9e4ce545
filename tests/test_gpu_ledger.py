"""The energy ledger (include/jaybenne_amd.h: jb_energy_ledger) on the GPU.  Expected values come from the CPU oracle,
never from the library: tests/ledger_cases.py restates a cycle on the oracle task by task and sums what its swarm
holds between TransportPhotons and RemoveMarkedParticles with math.fsum.  The sweep kernel itself runs on synthetic
swarms first, on the smallest shapes where it can go wrong."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import hetero_states as hs
import ledger_cases as lc
from helpers import load_deck
from test_gpu_hetero import _variant
from test_gpu_invariants import CHECKED, ROOT, TESTS, _clean, checked_lib  # noqa: F401  (checked_lib: fixture)

pytestmark = pytest.mark.gpu

SWARM_TERMS = ("e_sourced", "e_absorbed", "e_census", "e_escaped_unclassified")
COUNTS = ("n_sourced", "n_absorbed", "n_census", "n_escaped_unclassified")


def _driver(cid, bset, device, **kw):
    from jaybenne_amd import mcblock
    case, ov, pattern, cf = lc.setup_of(cid, bset)
    kw.setdefault("ledger", True)
    return mcblock.McblockDriver(load_deck(case.deck, ov), device=device, capacity_factor=cf,
                                 initial_state=hs.state_for(case.deck, ov, pattern), **kw), case


def _close(a, b, tol):
    return abs(a - b) <= tol * abs(b)


def _compare_ledger(got, want, tol):
    """Counts equal; every term within tol (relative) of the oracle's own term, per face; nothing unclassified; the
    tally holds the census energy; the energy balance closes."""
    for k in COUNTS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["n_escaped"] == want["n_escaped"], (got["n_escaped"], want["n_escaped"])
    assert got["n_escaped_unclassified"] == 0 and got["e_escaped_unclassified"] == 0.0
    for k in SWARM_TERMS:
        if want[k] != 0.0:
            assert _close(got[k], want[k], tol), (k, got[k], want[k])
        else:
            assert got[k] == 0.0, (k, got[k])
    for f in range(6):
        if want["e_escaped"][f] != 0.0:
            assert _close(got["e_escaped"][f], want["e_escaped"][f], tol), (lc.FACES[f], got["e_escaped"], want["e_escaped"])
        else:
            assert got["e_escaped"][f] == 0.0
    for k in ("e_tally", "e_delta", "e_material"):
        if want[k] != 0.0:
            assert _close(got[k], want[k], tol), (k, got[k], want[k])
        else:
            assert got[k] == 0.0, (k, got[k])
    assert _close(got["e_tally"], got["e_census"], 1e-12), (got["e_tally"], got["e_census"])
    assert _close(got["e_start"], want["e_start"], tol)
    assert got["residual"] <= 1e-12, got["residual"]
    assert (got["cycle"], got["t_start"], got["dt"]) == (want["cycle"], want["t_start"], want["dt"])


# ---- 1. the sweep itself -----------------------------------------------------------------------
def _hash(i, salt):
    x = (i.astype(np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    return x


def _synthetic(mesh, n, salt):
    """n slots: the five statuses mixed by a hash of the slot, weights over 1e-17 .. 1e7, every position inside the
    domain but those of the escaped slots -- outside exactly one outflow face, every such face in turn, or (one
    in five) with no outflow face: inside, or outside a face of another kind.  Some absorbed slots are the holes
    arrivals absorbed on another rank become (bit 63 of the id): not this rank's to count."""
    i = np.arange(n)
    h = _hash(i, salt)
    status = (h % np.uint64(5)).astype(np.int32)
    u = ((h >> np.uint64(11)) % np.uint64(1 << 20)).astype(np.float64) / float(1 << 20)
    w = 10.0 ** (-17.0 + 24.0 * u)
    lo, hi = np.asarray(mesh.gmin, dtype=np.float64), np.asarray(mesh.gmax, dtype=np.float64)
    ext = hi - lo
    pos = np.empty((3, n))
    for d in range(3):
        ud = ((_hash(i, salt + 101 + d) >> np.uint64(7)) % np.uint64(1 << 20)).astype(np.float64) / float(1 << 20)
        pos[d] = lo[d] + (0.01 + 0.98 * ud) * ext[d]
    bc = np.asarray(mesh.swarm_bc)
    open_faces = [f for f in range(2 * mesh.ndim) if bc[f] == lc.BC_OUTFLOW]
    other_faces = [f for f in range(2 * mesh.ndim) if bc[f] != lc.BC_OUTFLOW]
    pick = ((h >> np.uint64(40)) % np.uint64(5 * len(open_faces))).astype(np.int64)
    beyond = 1e-3 + 0.3 * u
    for q, f in enumerate(open_faces):
        m = (status == lc.ST_ESCAPED) & (pick % 5 != 4) & ((pick // 5) == q)
        d = f >> 1
        pos[d][m] = (hi[d] + beyond[m] * ext[d]) if f & 1 else (lo[d] - beyond[m] * ext[d])
    m = (status == lc.ST_ESCAPED) & (pick % 5 == 4) & ((pick // 5) % 2 == 1)      # outside a wall or a periodic face
    f = other_faces[salt % len(other_faces)]
    d = f >> 1
    pos[d][m] = (hi[d] + beyond[m] * ext[d]) if f & 1 else (lo[d] - beyond[m] * ext[d])
    ids = i.astype(np.uint64) + np.uint64(1000)
    deposited = (status == lc.ST_ABSORBED) & (((h >> np.uint64(50)) % np.uint64(4)) == 0)
    ids[deposited] |= np.uint64(1 << 63)
    return dict(status=status, w=w, x=pos[0], y=pos[1], z=pos[2], id=ids), deposited


def _expected(mesh, sw, deposited, first, last):
    r = slice(first, last)
    st, w = sw["status"][r], sw["w"][r]
    out = {}
    act = st == lc.ST_ACTIVE
    out["active"] = (math.fsum(w[act]), int(act.sum()))
    ab = ((st == lc.ST_ABSORBED) & ~deposited[r]) | (st == 4)
    out["absorbed"] = (math.fsum(w[ab]), int(ab.sum()))
    esc = st == lc.ST_ESCAPED
    face, _ = lc.classify(mesh, sw["x"][r][esc], sw["y"][r][esc], sw["z"][r][esc])
    out["faces"] = [(math.fsum(w[esc][face == f]), int((face == f).sum())) for f in range(7)]
    return out


def _upload(md, sw, n, device):
    import torch
    md.reserve(max(n, 1))
    for k, v in sw.items():
        t = torch.from_numpy(v.view(np.int64) if k == "id" else v).to(device)
        md.swarm[k][:n] = t
    md.sv.n = n
    torch.cuda.synchronize(device)


def _sweep(md, first, last, what):
    """accumulate over [first, last), then close: the cycle's ledger as the struct."""
    from jaybenne_amd import _lib
    md._sync_stream()
    _lib.check(md.lib.jb_ledger_accumulate(md.pkg.ctx, md.handle, C.byref(md.sv), first, last, what))
    led = _lib.EnergyLedger()
    _lib.check(md.lib.jb_ledger_close(md.pkg.ctx, md.handle, C.byref(md.sv), 0.0, 1.0, C.byref(led)))
    return led


def _within(got, want, scale):
    """the project's tolerance for sums whose order is not that of math.fsum: 1e-12 of the sum of all weights"""
    return abs(got - want) <= 1e-12 * scale


SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 100003)   # the wave, the workgroup, its tile of 4 x 256, many workgroups


@pytest.mark.parametrize("cid,bset", [("G1-imc", "RO"), ("G2S-imc", "S3"), ("G3U-imc", "S1"), ("G3U-imc", "S2"),
                                      ("G3U-imc", "S3")], ids=["1d-RO", "2d-S3", "3d-S1", "3d-S2", "3d-S3"])
def test_sweep_on_synthetic_swarms(gpu_device, cid, bset):
    from jaybenne_amd import _lib
    drv, _ = _driver(cid, bset, gpu_device)
    md, mesh = drv.md, drv.mesh
    assert md.ledger_enabled()
    checked_faces = set()
    for n in SIZES:
        sw, deposited = _synthetic(mesh, n, salt=n)
        _upload(md, sw, n, gpu_device)
        total = math.fsum(sw["w"]) if n else 0.0
        ranges = [(0, n)] + [(f, l) for f in (0, 1, 37) for l in (n - 1, n - 29) if 0 <= f <= l]
        for first, last in ranges:
            want = _expected(mesh, sw, deposited, first, last)
            whole = _expected(mesh, sw, deposited, 0, n)
            for what in (_lib.JB_LEDGER_SOURCED, _lib.JB_LEDGER_TRANSPORTED):
                led = _sweep(md, first, last, what)
                again = _sweep(md, first, last, what)
                assert bytes(led) == bytes(again), (n, first, last, what)       # the same call, the same bits
                assert led.cycle == 0                                           # (the host's to set)
                where = (n, first, last, what)
                # the close's own census sweep: the ACTIVE slots of the whole swarm
                assert led.n_census == whole["active"][1] and _within(led.e_census, whole["active"][0], total), where
                if what == _lib.JB_LEDGER_SOURCED:
                    assert led.n_sourced == want["active"][1] and _within(led.e_sourced, want["active"][0], total), where
                    assert led.n_absorbed == 0 and led.e_absorbed == 0.0 and sum(led.n_escaped) == 0
                    assert led.n_escaped_unclassified == 0
                    continue
                assert led.n_sourced == 0 and led.e_sourced == 0.0
                assert led.n_absorbed == want["absorbed"][1], where
                assert _within(led.e_absorbed, want["absorbed"][0], total), where
                for f in range(6):
                    assert led.n_escaped[f] == want["faces"][f][1], (where, f)
                    assert _within(led.e_escaped[f], want["faces"][f][0], total), (where, f)
                    if want["faces"][f][1]:
                        checked_faces.add(f)
                    if mesh.swarm_bc[f] != lc.BC_OUTFLOW:
                        assert led.n_escaped[f] == 0 and led.e_escaped[f] == 0.0
                assert led.n_escaped_unclassified == want["faces"][6][1], where
                assert _within(led.e_escaped_unclassified, want["faces"][6][0], total), where
                if n >= 1023 and (first, last) == (0, n):
                    assert want["faces"][6][1] > 0 and want["absorbed"][1] > 0 and int(deposited.sum()) > 0
    assert checked_faces == {f for f in range(2 * mesh.ndim) if mesh.swarm_bc[f] == lc.BC_OUTFLOW}
    # argument checks of the task form
    st = md.lib.jb_ledger_accumulate(md.pkg.ctx, md.handle, C.byref(md.sv), 0, md.n + 1, _lib.JB_LEDGER_SOURCED)
    assert st == _lib.JB_ERR_INVALID and b"outside the swarm" in md.lib.jb_last_error()
    assert md.lib.jb_ledger_accumulate(md.pkg.ctx, md.handle, C.byref(md.sv), 0, 1, 7) == _lib.JB_ERR_INVALID


# ---- 2. every tracking family against the oracle -----------------------------------------------
def _run_with_escaped(drv, cycles, monkeypatch):
    """drv.Step() on the task-driven path, with the swarm's escaped slots read before each compaction."""
    from jaybenne_amd import jaybenne as jb
    seen = []
    remove = jb.RemoveMarkedParticles

    def spy(md):
        g = md.get_swarm()
        m = g["status"] == lc.ST_ESCAPED
        seen.append({k: g[k][m] for k in ("id", "w", "x", "y", "z")})
        return remove(md)

    monkeypatch.setattr(jb, "RemoveMarkedParticles", spy)
    for _ in range(cycles):
        drv.Step()
    return seen


def _compare_escaped(seen, want):
    """id, w and the position on the escape axis, by creation id."""
    a, b = np.argsort(seen["id"]), np.argsort(want["id"])
    assert np.array_equal(seen["id"][a], want["id"][b])
    assert np.array_equal(seen["w"][a], want["w"][b])
    face = want["face"][b]
    for d, k in enumerate(("x", "y", "z")):
        m = (face >> 1) == d
        assert np.array_equal(seen[k][a][m], want[k][b][m]), k


def _family(gpu_device, monkeypatch, cid, bset, variant_ok, tol, exact, cycles=None):
    drv, case = _driver(cid, bset, gpu_device)
    assert drv.pkg.arithmetic() == ("exact" if exact else "lean")
    cycles = cycles or case.cycles
    want = lc.oracle_ledgers(cid, bset, cycles)
    seen = _run_with_escaped(drv, cycles, monkeypatch)
    v = _variant(drv)
    assert variant_ok(v, drv.mesh.ndim), v
    assert len(drv.md.ledger_history) == cycles and drv.md.ledger is drv.md.ledger_history[-1]
    for c in range(cycles):
        print(f"{cid} {bset} cycle {c + 1}: residual {drv.md.ledger_history[c]['residual']:.3e} "
              f"n_escaped {drv.md.ledger_history[c]['n_escaped']}")
        _compare_ledger(drv.md.ledger_history[c], want[c], tol)
        if exact:
            _compare_escaped(seen[c], want[c]["escaped"])
    assert sum(sum(h["n_escaped"]) for h in drv.md.ledger_history) == drv.md.stats()["n_escaped"] > 0
    return drv


@pytest.mark.parametrize("cid,bset", [("G3U-imc", "S1"), ("G3U-imc", "S3")])
def test_k_transport_exact(gpu_device, monkeypatch, cid, bset):
    _family(gpu_device, monkeypatch, cid, bset, lambda v, nd: f"k_transport<{nd}," in v and v.endswith("true, false>"),
            1e-12, True)


def test_k_transport_general_geometry(gpu_device, monkeypatch):
    _family(gpu_device, monkeypatch, "G3O-imc", "S2", lambda v, nd: "k_transport<3," in v and v.endswith("false, false>"),
            1e-12, True)


@pytest.mark.lean
@pytest.mark.parametrize("cid,bset", [("G3U-imc", "S2"), ("G2S-imc", "S1")])
def test_k_imc_cell_lean(gpu_device, monkeypatch, cid, bset):
    """Lean arithmetic, one cycle: terms to 1e-9, the lean tolerance after one cycle; counts equal."""
    _family(gpu_device, monkeypatch, cid, bset, lambda v, nd: v == f"k_imc_cell<{nd}, true, true, lean>",
            1e-9, False, cycles=1)


@pytest.mark.parametrize("arith", ["exact", pytest.param("lean", marks=pytest.mark.lean)])
def test_with_absorption_and_emission(gpu_device, monkeypatch, arith):
    ok = {"exact": lambda v, nd: "k_transport<3," in v, "lean": lambda v, nd: v == "k_imc_cell<3, true, false, lean>"}[arith]
    drv = _family(gpu_device, monkeypatch, "G3S-hot", "S1", ok, 1e-12 if arith == "exact" else 1e-9, arith == "exact")
    led = drv.md.ledger
    assert led["n_absorbed"] > 500 and led["n_sourced"] > 100 and led["e_delta"] != 0.0


DDMC = [("G1-ddmc", "RO", "queues"), ("G3S-ddmc", "S2", "queues"), ("G3S-ddmc", "S3", "all"),
        ("G1-ddmc", "RO", "no class allowed"), ("G3S-ddmc", "S2", "all")]


@pytest.mark.parametrize("cid,bset,mode", DDMC, ids=[f"{c}-{s}-{m.replace(' ', '_')}" for c, s, m in DDMC])
def test_ddmc(gpu_device, monkeypatch, cid, bset, mode):
    """k_ddmc_q (the default where it applies) and k_ddmc_all, behind the switches of tests/test_gpu_axes.py."""
    monkeypatch.delenv("JB_COOP_GATHER", raising=False)
    if mode == "queues":
        monkeypatch.setenv("JB_DDMC_QUEUES", "1")
        ok = lambda v, nd: "cell codes, queues" in v                                     # noqa: E731
    elif mode == "all":
        monkeypatch.setenv("JB_DDMC_QUEUES", "0")
        ok = lambda v, nd: f"k_ddmc_all<{nd}, true" in v and "queues" not in v           # noqa: E731
    else:
        monkeypatch.setenv("JB_DDMC_MAX_CLASSES", "0")
        ok = lambda v, nd: "k_ddmc_all" in v and "cell codes" not in v                   # noqa: E731
    _family(gpu_device, monkeypatch, cid, bset, ok, 1e-12, True)


@pytest.mark.parametrize("cid,bset", [("G2S-hybrid", "S1"), ("G3S-hybrid", "S2")])
def test_k_hybrid(gpu_device, monkeypatch, cid, bset):
    _family(gpu_device, monkeypatch, cid, bset, lambda v, nd: v == f"k_hybrid<{nd}, exact>", 1e-12, True)


# ---- 3. the three ways to run a step -----------------------------------------------------------
def test_three_ways_to_step_agree_bit_for_bit(gpu_device, monkeypatch):
    """jb_radiation_step (one C call), the task-driven Python path and JB_HANDOFF=step on one rank: the same
    struct, byte for byte."""
    from jaybenne_amd import _lib
    cid, bset = "G3U-imc", "S1"
    want = lc.oracle_ledgers(cid, bset, 1)[0]
    # the task-driven path
    a, _ = _driver(cid, bset, gpu_device)
    a.Step()
    _compare_ledger(a.md.ledger, want, 1e-12)
    la = _lib.EnergyLedger.from_dict(a.md.ledger)       # (the host sets the cycle of a ledger it closed itself)
    assert la.as_dict() == {k: v for k, v in a.md.ledger.items() if k not in ("e_start", "residual")}

    def c_call():
        b, _ = _driver(cid, bset, gpu_device)
        md = b.md
        md._sync_stream()
        e0 = _lib.EnergyLedger()
        _lib.check(md.lib.jb_ledger_close(md.pkg.ctx, md.handle, C.byref(md.sv), 0.0, 0.0, C.byref(e0)))
        next_id, cycle = C.c_uint64(md.next_id), C.c_uint32(md.cycle)
        _lib.check(md.lib.jb_radiation_step(md.pkg.ctx, md.handle, C.byref(md.sv), 0.0, b.dt, C.byref(next_id),
                                            C.byref(cycle), md.prefix.data_ptr()))
        lb = _lib.EnergyLedger()
        _lib.check(md.lib.jb_ledger_last(md.pkg.ctx, C.byref(lb)))
        assert e0.e_census == a.md.ledger["e_start"]
        return lb, b

    lb, b = c_call()
    # JB_HANDOFF=step on one rank
    handoff_before = os.environ.get("JB_HANDOFF")
    monkeypatch.setenv("JB_HANDOFF", "step")
    c, _ = _driver(cid, bset, gpu_device)
    assert c.md.handoff == "step"
    c.Step()
    assert c.md.handoff_path().startswith("c: jb_radiation_step_ranks")
    lc_ = _lib.EnergyLedger()
    _lib.check(c.md.lib.jb_ledger_last(c.md.pkg.ctx, C.byref(lc_)))
    if handoff_before is None:      # (further C calls run as the first one did)
        monkeypatch.delenv("JB_HANDOFF")
    else:
        monkeypatch.setenv("JB_HANDOFF", handoff_before)
    sl = a.mesh.interior()

    def inputs(drv):
        return drv.md.get_field("tally")[sl], drv.md.get_swarm()["id"]

    def agree(one, other):
        # Two of the ledger's INPUTS are not the same bits in every run of one problem: the tracking kernels
        # accumulate the tally field with atomics (tests/test_gpu_parity.py compares it to 1e-12 for that reason),
        # and RemoveMarkedParticles pairs holes with movers through an atomic cursor, so the slot ORDER of the census
        # swarm may differ (the existing tests compare swarms by creation id).  The ledger's sum of a given input is
        # reproducible (the sweep test above); here e_tally / e_census must be the same bits whenever the field /
        # the slot order is, and within 1e-12 otherwise.  Every other word of the struct must be identical.
        (n1, l1, (tally1, slots1)), (n2, l2, (tally2, slots2)) = one, other
        name = f"{n2} against {n1}"
        same = {"e_tally": np.array_equal(tally1, tally2), "e_census": np.array_equal(slots1, slots2)}
        print(f"{name}: inputs bit-equal: {same}")
        for k, _t in _lib.EnergyLedger._fields_:
            x, y = getattr(l1, k), getattr(l2, k)
            x, y = (list(x), list(y)) if hasattr(x, "__len__") else (x, y)
            if not same.get(k, True):
                assert abs(x - y) <= 1e-12 * abs(y), (name, k, x, y)
            else:
                assert x == y, (name, k, x, y)
        if all(same.values()):
            assert bytes(l1) == bytes(l2), name
        return sum(same.values())

    runs = [("task path", la, inputs(a)), ("C call", lb, inputs(b)), ("JB_HANDOFF=step", lc_, inputs(c))]
    exact = agree(runs[0], runs[1]) + agree(runs[0], runs[2]) + agree(runs[1], runs[2])
    # (the bit-equal branch must not go unused.  Whether an input repeats is up to the order in which the hardware
    # served the atomics -- in about half of the runs of these three neither does --, so the C call is made again,
    # every run held against all earlier ones, until one repeats.)
    for extra in range(64):
        if exact > 0:
            break
        lx, x = c_call()
        runs.append((f"C call {extra + 2}", lx, inputs(x)))
        exact += sum(agree(r, runs[-1]) for r in runs[:-1])
    assert exact > 0, "neither the tally field nor the census slot order repeated in any of the runs"


def test_a_cycle_after_release_scratch_gives_the_oracles_ledger(gpu_device):
    """jb_release_scratch between two ledger-on cycles: the ledger's own buffers stay, the scratch memory is taken
    again, and both cycles' ledgers are the oracle's"""
    from jaybenne_amd import _lib
    cid, bset = "G3U-imc", "S1"
    want = lc.oracle_ledgers(cid, bset, 2)
    drv, _ = _driver(cid, bset, gpu_device)
    md = drv.md
    drv.Step()
    _compare_ledger(md.ledger, want[0], 1e-12)
    md._sync_stream()
    _lib.check(md.lib.jb_release_scratch(md.pkg.ctx))
    drv.Step()
    _compare_ledger(md.ledger, want[1], 1e-12)


# ---- 4. several ranks --------------------------------------------------------------------------
RANKS = [("G3S-imc", "S3", 2, "blocks", "step"), ("G3S-ddmc", "S1", 4, "blocks", "step"),
         ("G3S-imc", "S3", 2, "blocks", "c"), ("G3S-ddmc", "S1", 2, "replicated", "c")]


def _rank_worker(rank, world, port, cid, bset, outdir, decomposition, handoff):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_HANDOFF=handoff, JB_EXACT_ARITH="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import mcblock
        from jaybenne_amd.comm import Comm
        case, ov, pattern, _ = lc.setup_of(cid, bset)
        drv = mcblock.McblockDriver(load_deck(case.deck, ov), rank=rank, nranks=world, comm=Comm(),
                                    device=torch.device("cuda", 0), capacity_factor=2.0, decomposition=decomposition,
                                    initial_state=hs.state_for(case.deck, ov, pattern), ledger=True)
        assert drv.decomposition == decomposition
        for _ in range(case.cycles):
            drv.Step()
        if handoff == "step":
            assert drv.md.handoff_path().startswith("c: jb_radiation_step_ranks"), drv.md.handoff_path()
        with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
            json.dump({"history": drv.md.ledger_history, "n_outgoing": drv.md.stats()["n_outgoing"],
                       "handoff_records": drv.md.handoff_records}, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("cid,bset,world,decomposition,handoff", RANKS,
                         ids=[f"{c}-{s}-{w}-{d}-{h}" for c, s, w, d, h in RANKS])
def test_ranks(gpu_device, cid, bset, world, decomposition, handoff, tmp_path):
    """The reduced ledger is the same on every rank, bit for bit, and the single-process oracle's to 1e-12; the
    hand-off really ran; nothing is counted twice."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, TESTS)
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, cid, bset, str(tmp_path), decomposition, handoff))
             for r in range(world)]             # (at most 4 rank processes + this one hold the GPU)
    _run_workers(procs)
    case = lc.case_of(cid)
    want = lc.oracle_ledgers(cid, bset, case.cycles)
    parts = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(world)]
    for p in parts[1:]:
        assert p["history"] == parts[0]["history"]          # (json round-trips a double's bits)
    if decomposition == "blocks":
        assert sum(p["n_outgoing"] for p in parts) > 0 and sum(p["handoff_records"] for p in parts) > 0
    for c in range(case.cycles):
        got = parts[0]["history"][c]
        _compare_ledger(got, want[c], 1e-12)
        assert sum(got["n_escaped"]) + got["n_absorbed"] + got["n_census"] == \
            sum(want[c]["n_escaped"]) + want[c]["n_absorbed"] + want[c]["n_census"]


# ---- 5. off means off --------------------------------------------------------------------------
def test_off_means_off(gpu_device):
    """The ledger only reads: swarm, fields and event count of a run without it equal a run with it; and without
    it there is no ledger to ask for."""
    from jaybenne_amd import _lib
    cid, bset = "G3U-imc", "S1"
    on, case = _driver(cid, bset, gpu_device)
    off, _ = _driver(cid, bset, gpu_device, ledger=False)
    assert on.md.ledger_enabled() and not off.md.ledger_enabled()
    for _ in range(case.cycles):
        on.Step()
        off.Step()
    assert off.md.ledger is None and off.md.ledger_history == [] and len(on.md.ledger_history) == case.cycles
    ga, gb = on.md.get_swarm(), off.md.get_swarm()
    assert on.md.n == off.md.n and on.md.events == off.md.events
    sa, sb = on.md.stats(), off.md.stats()
    for k in ("n_census", "n_absorbed", "n_escaped", "n_outgoing", "n_events"):      # (not the scheduling diagnostics)
        assert sa[k] == sb[k], k
    oa, ob = np.argsort(ga["id"]), np.argsort(gb["id"])
    for k in ga:
        assert np.array_equal(ga[k][oa], gb[k][ob]), k
    sl = on.mesh.interior()
    for k in ("tally", "edelta", "u", "fleck"):          # (atomic accumulation order differs from run to run)
        fa, fb = on.md.get_field(k)[sl], off.md.get_field(k)[sl]
        np.testing.assert_allclose(fa, fb, rtol=1e-12, atol=1e-12 * np.abs(fa).max(), err_msg=k)
    led = _lib.EnergyLedger()
    lib, ctx = off.md.lib, off.md.pkg.ctx
    assert lib.jb_ledger_last(ctx, C.byref(led)) == _lib.JB_ERR_INVALID and b"disabled" in lib.jb_last_error()
    assert lib.jb_ledger_close(ctx, off.md.handle, C.byref(off.md.sv), 0.0, 1.0, C.byref(led)) == _lib.JB_ERR_INVALID
    assert lib.jb_ledger_accumulate(ctx, off.md.handle, C.byref(off.md.sv), 0, 1, 0) == _lib.JB_ERR_INVALID
    assert b"disabled" in lib.jb_last_error()


def test_deck_key_and_environment_switch_it_on(gpu_device, monkeypatch):
    from jaybenne_amd import mcblock
    case, ov, pattern, cf = lc.setup_of("G1-imc", "RO")
    st = hs.state_for(case.deck, ov, pattern)
    drv = mcblock.McblockDriver(load_deck(case.deck, dict(ov, **{"jaybenne_amd/ledger": "true"})), device=gpu_device,
                                initial_state=st)
    assert drv.md.ledger_enabled()
    assert not mcblock.McblockDriver(load_deck(case.deck, ov), device=gpu_device, initial_state=st).md.ledger_enabled()
    monkeypatch.setenv("JB_LEDGER", "1")
    drv = mcblock.McblockDriver(load_deck(case.deck, ov), device=gpu_device, initial_state=st)
    assert drv.md.ledger_enabled()
    drv.Step()
    _compare_ledger(drv.md.ledger, lc.oracle_ledgers("G1-imc", "RO", 1)[0], 1e-12)


# ---- 6. under the checked library --------------------------------------------------------------
def child_case():
    import torch
    drv, case = _driver("G3S-hybrid", "S2", torch.device("cuda", 0))
    assert drv.md.invariants_enabled() and drv.md.ledger_enabled()
    for _ in range(case.cycles):
        drv.Step()
    rep = drv.md.invariant_report()
    rep["variant"] = _variant(drv)
    rep["history"] = drv.md.ledger_history
    return rep


@pytest.mark.timeout(600, method="thread")
def test_checked_library(gpu_device, checked_lib):
    e = dict(os.environ, JAYBENNE_AMD_LIB=CHECKED, JB_EXACT_ARITH="1")
    e.pop("JB_COOP_GATHER", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "checked"], capture_output=True, text=True, env=e,
                         timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    rep = json.loads(res.stdout.strip().splitlines()[-1])
    _clean(rep)
    assert rep["passes"]["hybrid"] > 0, rep
    want = lc.oracle_ledgers("G3S-hybrid", "S2", 1)
    assert len(rep["history"]) == 1
    _compare_ledger(rep["history"][0], want[0], 1e-12)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    print(json.dumps(child_case()))
