"""Exact deposition (include/jaybenne_amd.h: jb_set_deposition, JB_DEPOSIT_EXACT) on the GPU: energy_delta and the
census tally against tests/deposit_model.py bit for bit -- crafted swarms in three slot orders, with and without
truncation; every tracking family for one cycle, task by task, against the model over the GPU's own absorbed slots
and against the atomic mode; whole runs with emission and feedback on that do not depend on when the swarm was sorted
or on how many ranks hold it; the default mode untouched; the ledger.  Expected values come from the Python-integer
model and math.fsum, never from the library."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import comb_model as cm
import deposit_cases as dc
import deposit_model as dm
from helpers import load_deck

from test_gpu_comb import _by_id, _hash, _same, _upload
from test_gpu_hetero import _variant

pytestmark = pytest.mark.gpu

# one mesh on each side of kDepositLds = 1024 cells (jb_limits.hpp): 128 cells accumulate in LDS, 8 blocks of 8^3 in
# device memory
MESHES = {
    "1d-lds": ("stepdiff", {"parthenon/mesh/nx1": 128, "parthenon/meshblock/nx1": 64, "jaybenne/num_particles": 64}),
    "3d-global": ("inf", {"parthenon/mesh/nx1": 16, "parthenon/mesh/nx2": 16, "parthenon/mesh/nx3": 16,
                          "parthenon/meshblock/nx1": 8, "parthenon/meshblock/nx2": 8, "parthenon/meshblock/nx3": 8,
                          "jaybenne/num_particles": 64}),
}
N_SLOTS, N_HOT = 20000, 5000
ST_ESCAPED = 2


def _driver(name, device):
    from jaybenne_amd import mcblock
    deck, ov = MESHES[name]
    drv = mcblock.McblockDriver(load_deck(deck, ov), device=device)
    drv.md.deposition = "exact"
    assert drv.md.deposition == "exact"
    return drv


def _crafted(mesh, kmax, salt):
    """~20 000 slots in a hashed order: statuses ACTIVE / ABSORBED / ESCAPED at random, a quarter of the ABSORBED
    slots with bit 63 in the id (arrivals absorbed on their sender); weights a random 53-bit significand x 2^k,
    k in [0, kmax]; the hot cell holds 5 000 absorbed addends -- more than a wave, more than a tile -- and as many
    census photons; every third cell is empty."""
    nx = [int(v) for v in mesh.nx]
    ncell = nx[0] * nx[1] * nx[2]
    ncells = mesh.nblocks * ncell
    assert (ncells <= 1024) == (mesh.ndim == 1)
    i = np.arange(N_SLOTS)
    used = np.flatnonzero(np.arange(ncells) % 3 != 1)
    hot = int(used[len(used) // 2])
    cell_of = used[(_hash(i, salt + 1) % np.uint64(len(used))).astype(np.int64)]
    status = (_hash(i, salt + 2) % np.uint64(3)).astype(np.int32)        # 0 ACTIVE, 1 ABSORBED, 2 ESCAPED
    cell_of[:2 * N_HOT] = hot
    status[:N_HOT] = dm.ST_ABSORBED
    status[N_HOT:2 * N_HOT] = dm.ST_ACTIVE
    blk, c = cell_of // ncell, cell_of % ncell
    ijk = [c % nx[0], (c // nx[0]) % nx[1], c // (nx[0] * nx[1])]
    sw = {}
    for d, name in enumerate(("x", "y", "z")):
        sw[name] = (mesh.blk_xmin[blk, d] + (ijk[d] + 0.5) * mesh.blk_dx[blk, d]) if d < mesh.ndim else np.zeros(N_SLOTS)
    for q, name in enumerate(("vx", "vy", "vz", "t", "e")):
        sw[name] = np.full(N_SLOTS, 0.25 + q)
    sig = ((_hash(i, salt + 3) >> np.uint64(12)) | np.uint64(1 << 52)).astype(np.uint64)
    k = (_hash(i, salt + 4) % np.uint64(kmax + 1)).astype(np.int32)
    sw["w"] = np.ldexp(sig.astype(np.float64), k - 100)
    # (what must add nothing, in counted slots: rejected, not summed)
    sw["w"][2 * N_HOT:2 * N_HOT + 6] = [0.0, -1.5, np.inf, np.nan, -0.0, -np.inf]
    status[2 * N_HOT:2 * N_HOT + 3] = dm.ST_ABSORBED
    status[2 * N_HOT + 3:2 * N_HOT + 6] = dm.ST_ACTIVE
    ng = mesh.ng
    sw["ip"] = (ijk[0] + ng).astype(np.int32)
    sw["jp"] = (ijk[1] + (ng if mesh.ndim >= 2 else 0)).astype(np.int32)
    sw["kp"] = (ijk[2] + (ng if mesh.ndim >= 3 else 0)).astype(np.int32)
    sw["blk"] = blk.astype(np.int32)
    sw["status"] = status
    ids = (i + 1000).astype(np.uint64)
    marked = (status == dm.ST_ABSORBED) & (_hash(i, salt + 5) % np.uint64(4) == 0)
    ids[marked] |= np.uint64(dm.BIT63)
    sw["id"] = ids
    sw["rng"] = _hash(i, salt + 6)
    order = np.argsort(_hash(i, salt + 7), kind="stable")
    sw = {k_: np.ascontiguousarray(v[order]) for k_, v in sw.items()}
    per = np.bincount(cell_of, minlength=ncells)
    assert (per == 0).sum() >= ncells // 3 and per[hot] >= 2 * N_HOT
    assert int(marked.sum()) > 500 and int(((status == dm.ST_ABSORBED) & ~marked).sum()) > 5000
    return sw


def _orders(mesh, sw):
    """the swarm as crafted, in a random slot permutation, and in (block, cell) order"""
    n = len(sw["w"])
    perm = np.random.default_rng(11).permutation(n)
    by_cell = np.argsort(dm.cell_index(mesh, sw, n), kind="stable")
    return {"hashed": sw, "permuted": {k: np.ascontiguousarray(v[perm]) for k, v in sw.items()},
            "by cell": {k: np.ascontiguousarray(v[by_cell]) for k, v in sw.items()}}


def _volumes(mesh):
    return np.repeat([mesh.cell_volume(b) for b in range(mesh.nblocks)], mesh.ncell)


def _expected(mesh, sw, n, what, base):
    """(energy_delta, energy_tally, stats) of accumulate(what) + close on the first n slots, per interior cell."""
    E = dm.scale(sw["w"][:n])
    acc, n_add, n_trunc, n_rej = dm.deposit(mesh, sw, n, dm.counted(sw, n, what), E)
    assert not dm.top_bit(acc)
    D = dm.field(acc, E)
    edelta = np.where(np.array([a != 0 for a in acc]), base + D, base)
    act = sw["status"][:n] == dm.ST_ACTIVE
    Et = dm.scale(sw["w"][:n][act])
    acc_t, n_cen, n_trunc_t, n_rej_t = dm.deposit(mesh, sw, n, act, Et)
    tally = dm.field(acc_t, Et) / _volumes(mesh)
    return edelta, tally, dict(n_absorbed_addends=n_add, n_census_addends=n_cen, n_truncated=n_trunc + n_trunc_t,
                               n_rejected=n_rej + n_rej_t, scale_absorbed=E, scale_census=Et)


def _set_base(md, mesh, salt):
    """energy_delta before the deposits: something of either sign in every cell (the close adds to it, once)"""
    base = np.zeros(mesh.field_shape)
    flat = (_hash(np.arange(mesh.nblocks * mesh.ncell), salt).astype(np.float64) / 2.0 ** 64 - 0.5) * 2.0 ** 20
    base[mesh.interior()] = flat.reshape(base[mesh.interior()].shape)
    md.set_field("edelta", base)
    return flat


def _accumulate(md, first, last, what):
    md._sync_stream()
    return md.lib.jb_deposit_accumulate(md.pkg.ctx, md.handle, C.byref(md.sv), first, last, what)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _run_crafted(drv, sw, what_calls, device, salt=77):
    from jaybenne_amd import _lib
    md, mesh = drv.md, drv.mesh
    base = _set_base(md, mesh, salt)
    _upload(md, sw, device)
    for first, last, what in what_calls:
        assert _accumulate(md, first, last, what) == _lib.JB_COMPLETE, md.lib.jb_last_error()
    stats = md.deposit_close()
    return base, dm.interior_flat(mesh, md.get_field("edelta")), dm.interior_flat(mesh, md.get_field("tally")), stats


# ---- 1: crafted swarms, no transport ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_crafted_swarms_equal_the_model_in_any_order(gpu_device, name):
    from jaybenne_amd import _lib
    drv = _driver(name, gpu_device)
    md, mesh = drv.md, drv.mesh
    n = N_SLOTS
    both = _lib.JB_DEPOSIT_ABSORBED | _lib.JB_DEPOSIT_ARRIVALS
    orders = _orders(mesh, _crafted(mesh, 150, salt=5))
    calls = {"hashed": [(0, n, _lib.JB_DEPOSIT_ABSORBED), (0, n, _lib.JB_DEPOSIT_ARRIVALS)],   # two sweeps of the range
             "permuted": [(0, n, both)],                                                     # one, the id unread
             "by cell": [(0, 7001, both), (7001, n, both)]}                                  # two ranges, a run cut in two
    seen = []
    for key, sw in orders.items():
        base, edelta, tally, stats = _run_crafted(drv, sw, calls[key], gpu_device)
        want_d, want_t, want_s = _expected(mesh, sw, n, both, base)
        print(name, key, stats)
        assert stats == want_s and stats["n_truncated"] == 0 and stats["n_rejected"] == 6
        assert _bits_equal(edelta, want_d), key
        assert _bits_equal(tally, want_t), key
        assert (want_t == 0).sum() >= len(want_t) // 3 and np.array_equal(want_d == base, edelta == base)
        seen.append((edelta, tally))
    for e, t in seen[1:]:
        assert _bits_equal(e, seen[0][0]) and _bits_equal(t, seen[0][1])
    # the holes are told apart by bit 63: ABSORBED alone counts the ordinary ones, ARRIVALS alone the marked ones
    sw = orders["hashed"]
    for what in (_lib.JB_DEPOSIT_ABSORBED, _lib.JB_DEPOSIT_ARRIVALS):
        base, edelta, _, stats = _run_crafted(drv, sw, [(0, n, what)], gpu_device, salt=78 + what)
        want_d, _, want_s = _expected(mesh, sw, n, what, base)
        assert stats == want_s and _bits_equal(edelta, want_d), what
    # argument checks of the task form, and the mode cannot change with accumulators open
    assert _accumulate(md, 0, md.n + 1, both) == _lib.JB_ERR_INVALID and b"outside the swarm" in md.lib.jb_last_error()
    assert _accumulate(md, 0, 1, 0) == _lib.JB_ERR_INVALID and _accumulate(md, 0, 1, 4) == _lib.JB_ERR_INVALID
    assert _accumulate(md, 0, n, both) == _lib.JB_COMPLETE
    assert md.lib.jb_set_deposition(md.pkg.ctx, _lib.DEPOSIT_ATOMIC) == _lib.JB_ERR_INVALID
    assert b"open" in md.lib.jb_last_error() and md.deposition == "exact"
    md.deposit_close()
    md.deposition = "atomic"
    assert md.deposition == "atomic"


# ---- 2: truncation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_truncation_is_counted_and_equals_the_model(gpu_device, name):
    from jaybenne_amd import _lib
    drv = _driver(name, gpu_device)
    mesh = drv.mesh
    both = _lib.JB_DEPOSIT_ABSORBED | _lib.JB_DEPOSIT_ARRIVALS
    sw = _crafted(mesh, 200, salt=9)
    for key, s in _orders(mesh, sw).items():
        base, edelta, tally, stats = _run_crafted(drv, s, [(0, N_SLOTS, both)], gpu_device)
        want_d, want_t, want_s = _expected(mesh, s, N_SLOTS, both, base)
        print(name, key, stats)
        assert stats == want_s and stats["n_truncated"] > 0
        assert _bits_equal(edelta, want_d) and _bits_equal(tally, want_t), key


def test_a_heavier_later_range_raises_the_scale(gpu_device):
    """The scale is fixed by the first accumulate call; a later range with a heavier weight -- an arrival from a rank
    with hotter blocks -- raises it in front of its sweep: the accumulators move down, exactly while no set bit falls
    off (n_truncated == 0, the fields are the model's at any scale), counted where one does."""
    from jaybenne_amd import _lib
    drv = _driver("1d-lds", gpu_device)
    md, mesh = drv.md, drv.mesh
    n, half = 4000, 2000
    sw = {k: v[:n].copy() for k, v in _crafted(mesh, 20, salt=3).items()}
    heavy = int(np.flatnonzero(sw["status"][half:] == dm.ST_ABSORBED)[0]) + half
    for lift, truncates in ((40, False), (160, True)):
        base = _set_base(md, mesh, 5 + lift)
        _upload(md, sw, gpu_device)
        assert _accumulate(md, 0, half, 3) == _lib.JB_COMPLETE              # the scale is fixed here, over [0, n)
        s2 = {k: v.copy() for k, v in sw.items()}
        s2["w"][heavy] = float(sw["w"][np.isfinite(sw["w"])].max()) * 2.0 ** lift   # more than the headroom holds
        md.swarm["w"][heavy] = float(s2["w"][heavy])
        assert _accumulate(md, half, n, 3) == _lib.JB_COMPLETE
        stats = md.deposit_close()
        edelta = dm.interior_flat(mesh, md.get_field("edelta"))
        E0, E1 = dm.scale(sw["w"]), dm.scale(s2["w"])
        assert E1 == E0 + lift + 1 or E1 == E0 + lift
        assert stats["scale_absorbed"] == E1, (stats, E0, E1)
        # the model: the first range at the first scale, moved down; the second range at the raised scale
        sel = dm.counted(s2, n, 3)
        first, second = sel.copy(), sel.copy()
        first[half:], second[:half] = False, False
        acc0, a0, t0, r0 = dm.deposit(mesh, sw, n, first, E0)
        acc1, a1, t1, r1 = dm.deposit(mesh, s2, n, second, E1)
        moved = [dm.shift_right(a, E1 - E0) for a in acc0]
        acc = [(m[0] + b) & dm.MASK for m, b in zip(moved, acc1)]
        n_trunc = t0 + t1 + sum(m[1] for m in moved)
        print(lift, stats, n_trunc)
        assert (n_trunc > 0) == truncates
        assert (stats["n_absorbed_addends"], stats["n_rejected"]) == (a0 + a1, r0 + r1)
        act = s2["status"] == dm.ST_ACTIVE
        _, _, t_cen, _ = dm.deposit(mesh, s2, n, act, dm.scale(s2["w"][act]))
        assert stats["n_truncated"] == n_trunc + t_cen
        D = dm.field(acc, E1)
        assert _bits_equal(edelta, np.where(np.array([a != 0 for a in acc]), base + D, base))
        if not truncates:       # ... which is then the exact sum, whatever the scales were
            both_acc, _, t_all, _ = dm.deposit(mesh, s2, n, sel, E1)
            assert t_all == 0 and both_acc == acc
    md.deposition = "atomic"          # (nothing is left open)


def _records(mesh, sw, sel):
    """the hand-off records (13 words each, include/jaybenne_amd.h: JB_RECORD_WORDS) of the selected slots, as their
    sender packs them: bit 63 of the id word says "absorbed in a halo copy, deposit the weight"; one rank, so a
    block's global id is its index"""
    idx = np.flatnonzero(sel)
    rec = np.zeros((len(idx), 13), dtype=np.int64)
    for q, k in enumerate(("x", "y", "z", "vx", "vy", "vz", "t", "w", "e")):
        rec[:, q] = sw[k][idx].view(np.int64)
    rec[:, 9] = sw["id"][idx].view(np.int64)
    rec[:, 10] = (sw["jp"][idx].astype(np.int64) << 32) | sw["ip"][idx].astype(np.int64)
    rec[:, 11] = (sw["blk"][idx].astype(np.int64) << 32) | sw["kp"][idx].astype(np.int64)
    rec[:, 12] = sw["rng"][idx].view(np.int64)
    return rec


@pytest.mark.parametrize("name", list(MESHES))
def test_the_first_call_in_the_mode_may_be_an_unpack(gpu_device, name):
    """A rank whose swarm was empty so far, or a host that flips the switch and unpacks: the mesh's FIRST call in
    EXACT mode is jb_unpack_incoming.  The unpack kernel must get the decoy view even then -- energy_delta is the
    model's, every arrival's weight deposited once and not a second time by the kernel's own atomic."""
    import torch
    from jaybenne_amd import _lib, mcblock
    deck, ov = MESHES[name]
    drv = mcblock.McblockDriver(load_deck(deck, ov), device=gpu_device)          # (initialised in the default mode)
    md, mesh = drv.md, drv.mesh
    assert md.deposition == "atomic" and md.lib.jb_deposit_memory(md.handle) == 0
    md.deposition = "exact"
    assert md.lib.jb_deposit_memory(md.handle) == 0                               # (nothing taken by the switch alone)
    sw = _crafted(mesh, 150, salt=21)
    arrivals = dm.counted(sw, N_SLOTS, dm.ARRIVALS)          # bit 63: absorbed on their sender
    travellers = sw["status"] == dm.ST_ACTIVE               # ... and photons that go on
    rec = _records(mesh, sw, arrivals | travellers)
    base = _set_base(md, mesh, 31)
    n0 = md.n
    md.reserve(n0 + len(rec))
    rec_d = torch.from_numpy(rec).to(gpu_device)
    md._sync_stream()
    _lib.check(md.lib.jb_unpack_incoming(md.pkg.ctx, md.handle, C.byref(md.sv), rec_d.data_ptr(), len(rec)))
    assert md.n == n0 + len(rec) and md.lib.jb_deposit_memory(md.handle) >= 40 * mesh.nblocks * mesh.ncell
    g = md.get_swarm()
    holes = dm.counted(g, md.n, dm.ARRIVALS)
    assert int(holes.sum()) == int(arrivals.sum()) > 500 and int(dm.counted(g, md.n, dm.ABSORBED).sum()) == 0
    stats = md.deposit_close()
    want_d, want_t, want_s = _expected(mesh, g, md.n, dm.ARRIVALS, base)
    print(name, stats)
    assert stats == want_s and int(holes.sum()) - 3 <= stats["n_absorbed_addends"] <= int(holes.sum())
    assert _bits_equal(dm.interior_flat(mesh, md.get_field("edelta")), want_d)
    assert _bits_equal(dm.interior_flat(mesh, md.get_field("tally")), want_t)
    md.deposition = "atomic"


def test_a_replicated_mesh_turns_the_key_down(gpu_device):
    """A replicated mesh sums its fields over the ranks in floating point: the deck key is an error there, as the
    comb's and the boundary source's are, and so is the property."""
    from jaybenne_amd import mcblock
    pin = load_deck("stepdiff", dict(dc.ONE_D, **{"jaybenne_amd/deposition": "exact"}))
    with pytest.raises(ValueError, match="jaybenne_amd/deposition = exact"):
        mcblock.McblockDriver(pin, rank=0, nranks=2, comm=None, device=gpu_device, decomposition="replicated")


# ---- 3: every family, one cycle, task by task ---------------------------------------------------------
def _case_driver(name, device, arith, deposition):
    from jaybenne_amd import mcblock
    deck, ov, state, cf = dc.setup_of(name)
    drv = mcblock.McblockDriver(load_deck(deck, ov), device=device, capacity_factor=cf, initial_state=state)
    drv.pkg.set_arithmetic(arith)
    drv.md.deposition = deposition
    return drv


def _one_cycle(drv):
    """The cycle of jaybenne._radiation_step task by task, the swarm read after the transport call and before the
    compaction: (fields before transport, swarm after it, fields at the end, stats of the close or None)."""
    from jaybenne_amd import jaybenne as jb
    md, mesh = drv.md, drv.mesh
    use_ddmc = bool(drv.pkg.Param("use_ddmc"))
    md.cycle += 1
    jb.UpdateDerivedTransportFields(md, drv.dt)
    jb.SourcePhotons(md, jb.SourceType.emission, drv.time, drv.dt)
    md._sync_stream()
    md.lib.jb_zero_energy_tally(md.pkg.ctx, md.handle)
    before = dm.interior_flat(mesh, md.get_field("edelta"))
    (jb.TransportPhotons_DDMC if use_ddmc else jb.TransportPhotons)(md, drv.time, drv.dt, 0, md.n, fuse_census_tally=True)
    n = md.n
    g = md.get_swarm()
    variant = _variant(drv)
    jb.RemoveMarkedParticles(md)
    stats = md.deposit_close() if md.deposition == "exact" else None
    after = {k: dm.interior_flat(mesh, md.get_field(k)) for k in ("edelta", "tally")}
    return before, g, n, after, stats, variant


FAMILIES = [
    ("imc-1d", "exact", {}, lambda v: v.startswith("k_transport<1, ") and v.endswith("true, false>")),
    ("imc-1d", "lean", {}, lambda v: v.startswith("k_imc_cell<1, ")),
    ("imc-3d-smr", "exact", {}, lambda v: v.startswith("k_transport<3, ")),
    ("imc-3d-smr", "lean", {}, lambda v: v.startswith("k_imc_cell<3, ")),
    ("imc-3d", "exact", {}, lambda v: v.startswith("k_transport<3, ")),
    ("ddmc-1d", "exact", {"JB_DDMC_QUEUES": "1"}, lambda v: "cell codes, queues" in v),
    ("ddmc-1d", "exact", {"JB_DDMC_QUEUES": "0"}, lambda v: v.startswith("k_ddmc_all<1, ") and "queues" not in v),
    ("hybrid-2d", "exact", {}, lambda v: v == "k_hybrid<2, exact>"),
]


@pytest.mark.parametrize("name, arith, env, variant_ok", FAMILIES,
                         ids=[f"{n}-{a}" + "".join(f"-{k[3:].lower()}{v}" for k, v in e.items()) for n, a, e, _ in FAMILIES])
def test_every_family_deposits_what_it_absorbed(gpu_device, monkeypatch, name, arith, env, variant_ok):
    """Photons bit-identical to the atomic mode's; energy_delta = (value before transport) + the model over the GPU's
    own ST_ABSORBED slots, bit for bit, the tally likewise over its ACTIVE slots; and both within
    (m + 2) 2^-52 of the atomic fields per cell, m the cell's addend count -- the m - 1 roundings of a sum of m
    addends, relative to the largest partial sum the atomic adds can pass through, |before| + sum of the addends
    (the emission source leaves energy_delta negative, the deposits are positive)."""
    monkeypatch.delenv("JB_COOP_GATHER", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mesh = None
    out = {}
    for mode in ("atomic", "exact"):
        drv = _case_driver(name, gpu_device, arith, mode)
        out[mode] = _one_cycle(drv)
        mesh = drv.mesh
    before, g, n, after, stats, variant = out["exact"]
    before_a, g_a, n_a, after_a, _, variant_a = out["atomic"]
    assert variant_ok(variant) and variant_ok(variant_a), (variant, variant_a)
    # (the plan of the exact mode is made without the fused tally; k_hybrid's name does not say)
    if "k_hybrid" not in variant:
        assert (variant.split(",")[1].strip(" >"), variant_a.split(",")[1].strip(" >")) == ("false", "true"), (variant, variant_a)
    assert n == n_a and _same(g, g_a) and _bits_equal(before, before_a)
    absorbed = dm.counted(g, n, dm.ABSORBED)
    active = g["status"] == dm.ST_ACTIVE
    assert int(absorbed.sum()) >= 100 and int(dm.counted(g, n, dm.ARRIVALS).sum()) == 0
    E, Et = dm.scale(g["w"]), dm.scale(g["w"][active])
    acc, n_add, n_trunc, n_rej = dm.deposit(mesh, g, n, absorbed, E)
    acc_t, n_cen, n_trunc_t, n_rej_t = dm.deposit(mesh, g, n, active, Et)
    print(name, arith, variant, stats)
    assert stats == dict(n_absorbed_addends=n_add, n_census_addends=n_cen, n_truncated=0, n_rejected=0,
                         scale_absorbed=E, scale_census=Et)
    assert (n_trunc, n_rej, n_trunc_t, n_rej_t) == (0, 0, 0, 0) and n_add == int(absorbed.sum())
    D = dm.field(acc, E)
    want_d = np.where(D != 0, before + D, before)
    want_t = dm.field(acc_t, Et) / _volumes(mesh)
    assert _bits_equal(after["edelta"], want_d)
    assert _bits_equal(after["tally"], want_t)
    # against the atomic fields
    ncells = len(before)
    cells = dm.cell_index(mesh, g, n)
    m_d = np.bincount(cells[absorbed], minlength=ncells)
    m_t = np.bincount(cells[active], minlength=ncells)
    assert int((m_d >= 2).sum()) >= 10
    err_d = np.abs(after_a["edelta"] - after["edelta"])
    assert np.all(err_d <= (m_d + 2) * 2.0 ** -52 * (np.abs(before) + D)), float((err_d / (np.abs(before) + D + 1e-300)).max())
    err_t = np.abs(after_a["tally"] - after["tally"])
    assert np.all(err_t <= (m_t + 2) * 2.0 ** -52 * want_t), float((err_t / (want_t + 1e-300)).max())


def test_update_fluid_closes_what_is_open(gpu_device):
    """A host that only flips the switch: UpdateFluid with accumulators open closes them first, with the swarm of the
    last transport call as the compaction left it -- the fields of the explicit close, bit for bit."""
    from jaybenne_amd import jaybenne as jb
    outs = []
    for explicit in (True, False):
        drv = _case_driver("imc-1d", gpu_device, "exact", "exact")
        md, mesh = drv.md, drv.mesh
        md.cycle += 1
        jb.UpdateDerivedTransportFields(md, drv.dt)
        jb.SourcePhotons(md, jb.SourceType.emission, drv.time, drv.dt)
        jb.TransportPhotons(md, drv.time, drv.dt, 0, md.n, fuse_census_tally=True)
        jb.RemoveMarkedParticles(md)
        if explicit:
            md.deposit_close()
        jb.UpdateFluid(md)
        outs.append(({k: dm.interior_flat(mesh, md.get_field(k)) for k in ("edelta", "tally", "u")}, md.deposit_last()))
        launched = md.lib.jb_deposit_kernel_launches(md.pkg.ctx)
        assert launched > 0
        jb.UpdateFluid(md)          # nothing is open now: no kernel of the mode is launched, the counts stand
        assert md.lib.jb_deposit_kernel_launches(md.pkg.ctx) == launched
        assert md.deposit_last() == outs[-1][1]
    (fa, sa), (fb, sb) = outs
    assert sa == sb and sa["n_absorbed_addends"] >= 100 and sa["n_census_addends"] >= 100
    for k in fa:
        assert _bits_equal(fa[k], fb[k]), k


# ---- 4: whole runs ------------------------------------------------------------------------------------
# the RUN of tests/test_gpu_cell_order.py with what that test had to switch off switched on: emission, feedback and
# an absorption opacity, so that every deposit reaches the next cycle's opacities, emission counts and weights
def _run_overrides():
    from test_gpu_cell_order import RUN
    return dict(RUN, **dc.HOT, **{"jaybenne_amd/deposition": "exact"})


def _run(device, cycles, before=None, **ov):
    from jaybenne_amd import mcblock
    drv = mcblock.McblockDriver(load_deck("stepdiff", dict(_run_overrides(), **ov)), device=device, capacity_factor=2.0)
    drv.pkg.set_arithmetic("exact")
    assert drv.md.cell_order == "id" and drv.md.deposition == "exact"
    if before is not None:
        before(drv)
    for _ in range(cycles):
        drv.Step()
    return drv


FIELDS = ("u", "sie", "edelta", "tally")


def test_runs_with_feedback_do_not_depend_on_when_the_swarm_was_sorted(gpu_device):
    finals = []
    for interval in (0, 1):
        drv = _run(gpu_device, 3, **{"jaybenne/defrag_interval": interval})
        md = drv.md
        assert md.defrag_interval == interval and len(md.deposit_history) == 3
        print(interval, md.deposit_history)
        assert all(h["n_truncated"] == 0 and h["n_rejected"] == 0 and h["n_absorbed_addends"] >= 100
                   for h in md.deposit_history)
        g = md.get_swarm()
        assert len(np.unique(g["id"])) == md.n
        finals.append((_by_id(g), {k: md.get_field(k) for k in FIELDS}, md.deposit_history))
    (ga, fa, ha), (gb, fb, hb) = finals
    assert np.array_equal(ga["id"], gb["id"]) and _same(ga, gb)
    for k in FIELDS:
        assert _bits_equal(fa[k], fb[k]), k
    assert ha == hb
    # feedback did reach the material: the hot half cooled, the cold half warmed
    assert len(np.unique(fa["u"][drv.mesh.interior()])) > 2


# ---- 5: one rank against two ----------------------------------------------------------------------------
def _rank_worker(rank, world, port, outdir, handoff):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), JB_HANDOFF=handoff)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import mcblock
        from jaybenne_amd.comm import Comm
        from test_gpu_cell_order import _active_global
        drv = mcblock.McblockDriver(load_deck("stepdiff", _run_overrides()), rank=rank, nranks=world, comm=Comm(),
                                    device=torch.device("cuda", 0), capacity_factor=2.0)
        drv.pkg.set_arithmetic("exact")
        assert drv.md.cell_order == "id" and drv.md.deposition == "exact" and drv.md.handoff == handoff
        for _ in range(2):
            drv.Step()
        g = _active_global(drv.md, drv.md.get_swarm())
        hist = drv.md.deposit_history
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), resident=np.asarray(drv.md.resident_gids),
                 owner=np.asarray(drv.mesh.owner), gids=np.asarray(drv.md.gids),
                 truncated=np.array([h["n_truncated"] for h in hist]),
                 addends=np.array([h["n_absorbed_addends"] for h in hist]),
                 handed=np.array([drv.md.handoff_records]),
                 kernel_absorbed=np.array([drv.md.stats()["n_absorbed"]]),
                 **{"f_" + k: drv.md.get_field(k) for k in FIELDS}, **{k: g[k] for k in cm.SWARM_KEYS})
    finally:
        dist.destroy_process_group()


def _emit_as_a_rank_of(monkeypatch, blocks_per_rank):
    """The reference divides the emission count of a cell by the number of blocks in the CALLING rank's MeshData
    (sourcing.cpp:68-69; jaybenne.SourcePhotons passes the blocks the rank owns): two ranks with one block each emit
    twice the photons one rank with both blocks emits.  That is the source's, not the deposition's: the one-rank run
    the ranks are compared with makes its emission count calls with the ranks' block count, and is then the same
    problem."""
    from jaybenne_amd import _lib

    def before(drv):
        real = drv.md.lib.jb_source_photons_count

        def count(ctx, mesh, source_type, dt, blocks_in_call, *rest):
            if source_type == _lib.JB_SOURCE_EMISSION:
                blocks_in_call = blocks_per_rank
            return real(ctx, mesh, source_type, dt, blocks_in_call, *rest)

        monkeypatch.setattr(drv.md.lib, "jb_source_photons_count", count)
    return before


@pytest.mark.parametrize("handoff", ["c", "step"])
def test_two_ranks_equal_one(gpu_device, tmp_path, monkeypatch, handoff):
    import torch.multiprocessing as mp
    from test_gpu_cell_order import _active_global
    from test_gpu_multirank import _free_port, _run_workers
    sys.path.insert(0, os.path.dirname(__file__))
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path), handoff)) for r in range(2)])
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    assert all(len(p["gids"]) == 1 for p in parts)
    one = _run(gpu_device, 2, before=_emit_as_a_rank_of(monkeypatch, 1))
    hist = one.md.deposit_history
    g = _active_global(one.md, one.md.get_swarm())
    both = {k: np.concatenate([p[k] for p in parts]) for k in cm.SWARM_KEYS}
    assert len(np.unique(both["id"])) == len(both["id"]) == len(g["id"])
    a, b = _by_id(both), _by_id(g)
    assert np.array_equal(a["id"], b["id"])
    for k in cm.SWARM_KEYS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    for p in parts:
        assert np.all(p["truncated"] == 0) and len(p["truncated"]) == 2
        for k in FIELDS:
            assert _bits_equal(p["f_" + k], one.md.get_field(k)[p["gids"]]), k
    # every absorption was deposited once, by the owner of its cell: the ranks' addends add up to the one-rank run's.
    # And the arrivals sweep counted some of them: a rank's tracking kernels count the histories they end ABSORBED
    # in an owned block (an absorption in a halo copy ends OUTGOING_ABSORBED), so what the rank deposited beyond
    # that count arrived from the other rank
    for p in parts:
        arrivals = int(p["addends"].sum()) - int(p["kernel_absorbed"][0])
        print(handoff, "arrivals deposited:", arrivals, "handed over:", int(p["handed"][0]))
        assert int(p["handed"][0]) > 0 and arrivals > 0
    assert np.array_equal(parts[0]["addends"] + parts[1]["addends"], [h["n_absorbed_addends"] for h in hist])
    print(handoff, [p["addends"].tolist() for p in parts], [h["n_absorbed_addends"] for h in hist])


# ---- 6: off means off ---------------------------------------------------------------------------------
def test_the_default_mode_is_untouched(gpu_device):
    """ATOMIC (the default): the entry points of the exact mode are JB_ERR_INVALID, and a cycle is the oracle's, bit
    for bit in the exact arithmetic, through the kernel with the fused tally."""
    from jaybenne_amd import _lib, mcblock
    from helpers import make_oracle, run_oracle_cycles
    from oracle import orc
    over = {"jaybenne/num_particles": 2000}
    O, _, _ = make_oracle(load_deck("stepdiff", over), orc.MATH_PORTABLE)
    run_oracle_cycles(O, load_deck("stepdiff", over), 1)
    drv = mcblock.McblockDriver(load_deck("stepdiff", over), device=gpu_device)
    md = drv.md
    drv.pkg.set_arithmetic("exact")
    assert md.deposition == "atomic" and md.deposit_history == []
    st = _lib.DepositStats()
    assert md.lib.jb_deposit_last(md.pkg.ctx, C.byref(st)) == _lib.JB_ERR_INVALID
    assert md.lib.jb_deposit_close(md.pkg.ctx, md.handle, C.byref(md.sv)) == _lib.JB_ERR_INVALID
    assert _accumulate(md, 0, md.n, 3) == _lib.JB_ERR_INVALID and b"not exact" in md.lib.jb_last_error()
    drv.Step()
    assert _variant(drv).startswith("k_transport<1, true, ")           # (the fused tally is in the plan)
    g = md.get_swarm()
    assert md.n == O.n and md.events == O.events and md.deposit_history == []
    for k in ("ip", "rng", "status", "x", "vx", "t", "w"):
        assert np.array_equal(g[k], O.sw[k][:O.n]), k
    assert md.lib.jb_deposit_last(md.pkg.ctx, C.byref(st)) == _lib.JB_ERR_INVALID
    # the cycle (its UpdateFluid included) launched no kernel of the mode and took no memory for it
    assert md.lib.jb_deposit_kernel_launches(md.pkg.ctx) == 0 and md.lib.jb_deposit_memory(md.handle) == 0
    from jaybenne_amd import jaybenne as jb
    jb.UpdateFluid(md)
    jb.EvaluateRadiationEnergy(md)
    assert md.lib.jb_deposit_kernel_launches(md.pkg.ctx) == 0 and md.lib.jb_deposit_memory(md.handle) == 0
    # all tracked fields of the cycle are the oracle's to the tolerance of the atomic sums
    sl = drv.mesh.interior()
    for k in ("tally", "edelta"):
        np.testing.assert_allclose(md.get_field(k)[sl], O.fields[k][sl], rtol=1e-12)


# ---- 7: the ledger ------------------------------------------------------------------------------------
def test_the_ledger_closes_over_the_exact_fields(gpu_device):
    import ledger_cases as lc
    from test_gpu_ledger import _compare_ledger, _driver as ledger_driver
    cid, bset = "G3S-hot", "S1"
    drv, case = ledger_driver(cid, bset, gpu_device)
    drv.pkg.set_arithmetic("exact")
    drv.md.deposition = "exact"
    want = lc.oracle_ledgers(cid, bset, case.cycles)
    for c in range(case.cycles):
        drv.Step()
        led = drv.md.ledger_history[c]
        _compare_ledger(led, want[c], 1e-12)
        mesh = drv.mesh
        e_delta = math.fsum(dm.interior_flat(mesh, drv.md.get_field("edelta")))
        assert abs(led["e_delta"] - e_delta) <= 1e-12 * abs(e_delta), (led["e_delta"], e_delta)
        h = drv.md.deposit_history[c]
        assert h["n_truncated"] == 0 and h["n_absorbed_addends"] == led["n_absorbed"] and h["n_census_addends"] == led["n_census"]
