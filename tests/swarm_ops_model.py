"""The kernels that move whole photons from slot to slot, restated in numpy: compaction (jb_remove_marked_particles),
the defrag sort in its default order (jb_defrag_particles under JB_CELL_ORDER_ANY) and the inter-rank hand-off
(jb_pack_outgoing, jb_unpack_incoming, jb_exchange) -- and the crafted swarms they are held to, with the counters
that say which paths a crafted swarm exercises.  No library code computes anything here; status numbers,
JB_RECORD_WORDS and the record layout are read from / follow include/jaybenne_amd.h.  All comparisons are of bits.

A swarm is a dict of sixteen arrays (KEYS); a geometry (Geom) is one rank's view of a mesh: the resident blocks in
the order of the rank's list, the owner of every global block, the local index of every global block."""
import math
import os
import re

import numpy as np

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jaybenne_amd.h")
with open(_HEADER) as _f:
    _TEXT = _f.read()
_ST = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bJB_ST_([A-Z_]+) = (\d+)", _TEXT)}
ST_ACTIVE, ST_ABSORBED, ST_ESCAPED = _ST["ACTIVE"], _ST["ABSORBED"], _ST["ESCAPED"]
ST_OUTGOING, ST_OUTGOING_ABSORBED = _ST["OUTGOING"], _ST["OUTGOING_ABSORBED"]
RECORD_WORDS = int(re.search(r"#define JB_RECORD_WORDS (\d+)", _TEXT).group(1))
DEFRAG_SORT_NOW = int(re.search(r"\bJB_DEFRAG_SORT_NOW = (\d+)", _TEXT).group(1))
assert sorted(_ST.values()) == [0, 1, 2, 3, 4] and RECORD_WORDS == 13

LIVE = (ST_ACTIVE, ST_OUTGOING, ST_OUTGOING_ABSORBED)      # what RemoveMarkedParticles keeps
DEAD = (ST_ABSORBED, ST_ESCAPED)
F64 = ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e")
I32 = ("ip", "jp", "kp", "blk", "status")
U64 = ("id", "rng")
KEYS = F64 + I32 + U64
BIT63 = np.uint64(1 << 63)
WAVE = 64
INT_MAX = 2 ** 31 - 1


# ---- geometry ---------------------------------------------------------------------------------------
class Geom:
    """One rank's view of a mesh, from the arrays of the host's mesh object (data, not code): ``resident`` the
    global ids of the resident blocks in the rank's order (owned first), ``owner`` the rank of every global block."""

    def __init__(self, mesh, resident, owner=None, nowned=None):
        g = np.asarray(resident, dtype=np.int64)
        self.ndim, self.ng = int(mesh.ndim), int(mesh.ng)
        self.nx = [int(v) for v in mesh.nx]
        self.first = [self.ng if d < self.ndim else 0 for d in range(3)]          # is, js, ks
        self.dims = [self.nx[d] + 2 * self.first[d] for d in range(3)]            # ni, nj, nk
        self.ntot = self.dims[0] * self.dims[1] * self.dims[2]
        self.ncell = self.nx[0] * self.nx[1] * self.nx[2]
        self.gids = g
        self.nblocks, self.nblocks_total = len(g), int(mesh.nblocks)
        self.nowned = self.nblocks if nowned is None else int(nowned)
        self.xmin = np.asarray(mesh.blk_xmin, dtype=np.float64)[g]
        self.dx = np.asarray(mesh.blk_dx, dtype=np.float64)[g]
        self.owner = np.asarray(mesh.owner if owner is None else owner, dtype=np.int64)
        self.local_index = np.full(self.nblocks_total, -1, dtype=np.int64)
        self.local_index[g] = np.arange(self.nblocks)
        self.nkeys = self.nblocks * self.ntot


# ---- hashes -----------------------------------------------------------------------------------------
def _hash(i, salt):
    """a bijection of the 64-bit words (odd multipliers, xor-shifts)"""
    x = (np.asarray(i).astype(np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    return x


def _unit(i, salt):
    return ((_hash(i, salt) >> np.uint64(11)) % np.uint64(1 << 20)).astype(np.float64) / float(1 << 20)


def _mod(i, salt, m):
    return (_hash(i, salt) % np.uint64(m)).astype(np.int64)


def _odd_doubles(ids, salt):
    """Bit patterns no kernel under test may interpret: the raw hash (any double at all), and in three eighths of
    the slots -0.0, a denormal, a NaN with a payload (quiet or signalling, either sign)."""
    h = _hash(ids, salt)
    sel = _mod(ids, salt + 1, 8)
    frac = (h & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(1)
    sign = h & BIT63
    out = h.copy()
    out[sel == 0] = BIT63
    out[sel == 1] = (sign | frac)[sel == 1]
    out[sel == 2] = (sign | np.uint64(0x7FF0000000000000) | frac)[sel == 2]
    return out.view(np.float64)


# ---- the crafted swarm --------------------------------------------------------------------------------
EDGE_KINDS = 6      # of 32: one ghost layer below / above, past the ghosts below / above, far below / above
FAR = 1000003       # cells: "far out", and still an int after the division by dx


def crafted(geom, n, salt, status=None, keys=None, dest=None, edges=True, bad_blk=True, arrivals=False):
    """A deterministic swarm of n slots.

    Binding: ids are unique and below 2^63 (a bijective hash of the slot number, shifted); every other attribute of
    a slot is a different hash of its ID, so one photon's value under another's id, or x where y belongs, changes
    bytes.  vx vy vz t e w are odd bit patterns (_odd_doubles), rng is all ones in an eighth of the slots; ip jp kp
    are arbitrary 32-bit values, negative ones included.  Positions are finite.

    ``status``: per slot (default: half ACTIVE, the rest spread over the four other statuses, by id).
    ``keys``: per slot, for ACTIVE slots: local block * interior cells + interior cell (k, j, i order) the photon's
    position is placed in, at a hashed place inside the cell away from its faces (default: hashed).  With ``edges`` a
    share of 6/32 per active axis lies outside the block instead: one ghost layer out, past the ghost layers, and
    FAR cells out, on either side -- the sort key clamps those to the block's array.  With ``bad_blk`` 1/16 of the
    ACTIVE slots carry a blk outside [0, nblocks): -1, nblocks, 2^31 - 1 (the key behind all cells).
    Slots that are not ACTIVE: blk is -1, nblocks, 2^31 - 1 or a valid global id, by id; ``dest`` (per slot, global
    block ids) overrides that for the two OUTGOING kinds, whose blk the pack kernels look up the owner of.
    ``arrivals``: the OUTGOING_ABSORBED slots are absorbed arrivals in the making -- the receiver indexes a field
    with them, so they get interior ip jp kp and a weight that is a small integer times 2^-10."""
    i = np.arange(n, dtype=np.int64)
    ids = _hash(i, salt) >> np.uint64(1)
    assert len(np.unique(ids)) == n
    if status is None:
        h = _mod(ids, salt + 11, 8)
        status = np.where(h < 4, ST_ACTIVE, np.array([0, 0, 0, 0, ST_ABSORBED, ST_ESCAPED, ST_OUTGOING,
                                                      ST_OUTGOING_ABSORBED])[h])
    status = np.asarray(status, dtype=np.int32).copy()
    assert status.shape == (n,)
    active = status == ST_ACTIVE
    if keys is None:
        keys = _mod(ids, salt + 12, geom.nblocks * geom.ncell)
    keys = np.asarray(keys, dtype=np.int64)
    lb, c = keys // geom.ncell, keys % geom.ncell
    assert n == 0 or (keys.min() >= 0 and lb.max() < geom.nblocks)
    cell = [c % geom.nx[0], (c // geom.nx[0]) % geom.nx[1], c // (geom.nx[0] * geom.nx[1])]
    sw = {}
    for d, name in enumerate(("x", "y", "z")):
        anywhere = (_unit(ids, salt + 20 + d) - 0.5) * np.ldexp(1.0, _mod(ids, salt + 23 + d, 41) - 20)
        if d < geom.ndim:
            frac = 0.05 + 0.9 * _unit(ids, salt + 26 + d)
            where = cell[d].astype(np.float64)
            if edges:
                kind = _mod(ids, salt + 29 + d, 32)
                nxd, ng = geom.nx[d], geom.ng
                for q, v in enumerate((-1, nxd, -(ng + 1), nxd + ng, -FAR, nxd + FAR)):
                    where = np.where(kind == q, float(v), where)
            inside = geom.xmin[lb, d] + (where + frac) * geom.dx[lb, d]
            sw[name] = np.where(active, inside, anywhere)
        else:
            sw[name] = anywhere
        assert np.all(np.isfinite(sw[name]))
    for q, name in enumerate(("vx", "vy", "vz", "t", "w", "e")):
        sw[name] = _odd_doubles(ids, salt + 40 + 2 * q)
    for q, name in enumerate(("ip", "jp", "kp")):
        sw[name] = (_hash(ids, salt + 60 + q) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    # blk
    odd = np.array([-1, geom.nblocks, INT_MAX], dtype=np.int64)
    pick = _mod(ids, salt + 70, 6)
    other = np.where(pick < 3, odd[np.minimum(pick, 2)], _mod(ids, salt + 71, geom.nblocks_total))
    blk = np.where(active, lb, other)
    if bad_blk:
        bad = active & (_mod(ids, salt + 72, 16) == 0)
        blk = np.where(bad, odd[_mod(ids, salt + 73, 3)], blk)
    outgoing = (status == ST_OUTGOING) | (status == ST_OUTGOING_ABSORBED)
    if dest is not None:
        blk = np.where(outgoing, np.asarray(dest, dtype=np.int64), blk)
    sw["blk"] = blk.astype(np.int32)
    sw["status"] = status
    sw["id"] = ids
    rng = _hash(ids, salt + 80)
    rng[_mod(ids, salt + 81, 8) == 0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    sw["rng"] = rng
    if arrivals:
        assert dest is not None
        ab = status == ST_OUTGOING_ABSORBED
        for d, name in enumerate(("ip", "jp", "kp")):
            sw[name] = np.where(ab, geom.first[d] + _mod(ids, salt + 90 + d, geom.nx[d]), sw[name]).astype(np.int32)
        sw["w"] = np.where(ab, (1 + _mod(ids, salt + 93, 4096)) * 2.0 ** -10, sw["w"])
    return {k: np.ascontiguousarray(sw[k]) for k in KEYS}


def edelta_base(geom, salt):
    """energy_delta before an unpack, every resident cell (ghosts too): small integers times 2^-10 of either sign"""
    q = np.arange(geom.nblocks * geom.ntot)
    v = (_mod(q, salt, 4096) - 2048) * 2.0 ** -10
    return v.reshape(geom.nblocks, geom.dims[2], geom.dims[1], geom.dims[0])


# ---- whole records -------------------------------------------------------------------------------------
def take(sw, idx):
    return {k: np.ascontiguousarray(sw[k][idx]) for k in KEYS}


def copy(sw):
    return {k: sw[k].copy() for k in KEYS}


def differing(a, b):
    """the attributes whose bytes differ between two swarms of equal length (empty: the same bytes)"""
    return [k for k in KEYS if not np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8))]


def by_id(sw):
    """slots ordered by the id word (ids are unique, bit 63 included: one order, so equal multisets of whole records
    are equal arrays afterwards)"""
    return take(sw, np.argsort(sw["id"], kind="stable"))


def same_multiset(a, b):
    """[] when the two swarms hold the same whole records, each as often; else what differs"""
    if len(a["id"]) != len(b["id"]):
        return ["length"]
    return differing(by_id(a), by_id(b))


# ---- compaction ----------------------------------------------------------------------------------------
def live(status):
    """swarm_slot_live: ACTIVE, and the two kinds that wait for their hand-off"""
    status = np.asarray(status)
    return (status == ST_ACTIVE) | (status == ST_OUTGOING) | (status == ST_OUTGOING_ABSORBED)


def compact(sw, n):
    """RemoveMarkedParticles on slots 0..n-1: (survivors, expected swarm of `survivors` slots, holes, movers).
    Every live slot below `survivors` keeps its place and bytes; the holes below it (slots that are not live) take
    the live slots at or above it as whole records -- which mover fills which hole is not defined, so the expected
    swarm shows them in ascending order and compact_failures compares that part as a multiset."""
    alive = live(sw["status"][:n])
    survivors = int(alive.sum())
    slot = np.arange(n)
    holes = slot[(slot < survivors) & ~alive]
    movers = slot[(slot >= survivors) & alive]
    assert len(holes) == len(movers)
    want = take(sw, np.arange(survivors))
    for k in KEYS:
        want[k][holes] = sw[k][movers]
    return survivors, want, holes, movers


def compact_failures(sw, n, got):
    """`got`: the first `survivors` slots after the call.  [] or the list of what is wrong."""
    survivors, want, holes, _ = compact(sw, n)
    if len(got["id"]) != survivors:
        return ["length"]
    stay = np.ones(survivors, dtype=bool)
    stay[holes] = False
    bad = ["stayer " + k for k in differing(take(got, stay), take(want, stay))]
    return bad + ["moved " + k for k in same_multiset(take(got, holes), take(want, holes))]


# ---- the sort key -----------------------------------------------------------------------------------------
def raw_cell_index(geom, sw, n):
    """per axis, the index of the cell that holds the position in the block's array, NOT clamped (int64), for the
    block sw["blk"] clipped into the resident list"""
    blk = sw["blk"][:n].astype(np.int64)
    b = np.clip(blk, 0, geom.nblocks - 1)
    keyed = (sw["status"][:n] == ST_ACTIVE) & (blk == b)             # the slots whose position the kernel looks at
    out = []
    for d, name in enumerate(("x", "y", "z")):
        if d < geom.ndim:
            q = np.floor((sw[name][:n] - geom.xmin[b, d]) * (1.0 / geom.dx[b, d]))
            assert np.all(np.abs(q[keyed]) < 2.0 ** 31 - 8)         # (the kernel converts to int)
            q = np.where(keyed, q, 0.0)
            out.append(q.astype(np.int64) + geom.first[d])
        else:
            out.append(np.zeros(n, dtype=np.int64))
    return out


def sort_key(geom, sw, n):
    """(resident block, cell of the position clamped to the block's array, ghosts included) as one number;
    nkeys for anything that is not ACTIVE or whose blk is outside [0, nblocks)"""
    blk = sw["blk"][:n].astype(np.int64)
    i, j, k = (np.clip(q, 0, size - 1) for q, size in zip(raw_cell_index(geom, sw, n), geom.dims))
    key = blk * geom.ntot + (k * geom.dims[1] + j) * geom.dims[0] + i
    behind = (sw["status"][:n] != ST_ACTIVE) | (blk < 0) | (blk >= geom.nblocks)
    return np.where(behind, geom.nkeys, key)


def sorted_failures(geom, before, after, n):
    """[] when `after` is `before` sorted: keys non-decreasing (so the nkeys group comes last), and every key's
    group the same multiset of whole records -- all sixteen attributes, bytes."""
    if any(len(after[k]) != n or len(before[k]) != n for k in KEYS):
        return ["length"]
    k0, k1 = sort_key(geom, before, n), sort_key(geom, after, n)
    bad = []
    if np.any(np.diff(k1) < 0):
        bad.append("keys decrease")
    if n and k1[-1] != k1.max():
        bad.append("the last group is not the largest key")
    o0, o1 = np.lexsort((before["id"], k0)), np.lexsort((after["id"], k1))
    if not np.array_equal(k0[o0], k1[o1]):
        bad.append("group sizes")
    return bad + ["group " + k for k in differing(take(before, o0), take(after, o1))]


# ---- hand-off ----------------------------------------------------------------------------------------------
def records(sw, idx):
    """the 13-word records of slots idx, in that order:
    0..8 x y z vx vy vz t w e | 9 id, bit 63 set for OUTGOING_ABSORBED | 10 ip (low), jp (high) |
    11 kp (low), blk -- a global block id -- (high) | 12 rng"""
    idx = np.asarray(idx, dtype=np.int64)
    rec = np.zeros((len(idx), RECORD_WORDS), dtype=np.uint64)
    for q, k in enumerate(F64):
        rec[:, q] = sw[k][idx].view(np.uint64)
    absorbed = sw["status"][idx] == ST_OUTGOING_ABSORBED
    rec[:, 9] = sw["id"][idx] | np.where(absorbed, BIT63, np.uint64(0))
    lo = lambda v: v[idx].view(np.uint32).astype(np.uint64)      # noqa: E731  (the 32 bits, not the sign-extended value)
    rec[:, 10] = lo(sw["ip"]) | (lo(sw["jp"]) << np.uint64(32))
    rec[:, 11] = lo(sw["kp"]) | (lo(sw["blk"]) << np.uint64(32))
    rec[:, 12] = sw["rng"][idx]
    return rec


def record_set(rec):
    """records in the order of their id word (unique): equal sets are equal arrays"""
    rec = np.asarray(rec).view(np.uint64).reshape(-1, RECORD_WORDS)
    return rec[np.argsort(rec[:, 9], kind="stable")]


def pack(owner, sw, first, last, nranks):
    """jb_pack_outgoing on [first, last): (counts per rank, one record_set per rank, the swarm afterwards).  Packed
    slots become ABSORBED and nothing else changes; slots outside the range are untouched, outgoing or not."""
    st = sw["status"]
    slot = np.arange(len(st))
    out = (slot >= first) & (slot < last) & ((st == ST_OUTGOING) | (st == ST_OUTGOING_ABSORBED))
    idx = slot[out]
    rank = np.asarray(owner, dtype=np.int64)[sw["blk"][idx]]
    counts = np.bincount(rank, minlength=nranks).astype(np.int64)
    assert len(counts) == nranks
    segments = [record_set(records(sw, idx[rank == r])) for r in range(nranks)]
    after = copy(sw)
    after["status"][idx] = ST_ABSORBED
    return counts, segments, after


def unpack(geom, sw, n, rec, edelta):
    """jb_unpack_incoming onto a swarm of n slots: (the swarm afterwards, n + nrec slots: the first n as they were,
    the arrivals behind them at slots n .. n + nrec in record order; energy_delta afterwards).  blk is the local index of
    the record's global block id; an absorbed arrival (bit 63 of word 9) becomes an ABSORBED hole that keeps bit 63
    in its id and adds its weight to energy_delta at (blk, kp, jp, ip); the others become ACTIVE with bit 63 clear.

    The kernel adds with floating-point atomics in whatever order the lanes arrive.  The crafted absorbed arrivals
    carry weights that are small integers times 2^-10, and edelta_base values of the same kind: every partial sum
    in every order is an integer times 2^-10 below 2^53, so every order gives the same double -- this one."""
    rec = np.asarray(rec).view(np.uint64).reshape(-1, RECORD_WORDS)
    before, sw = sw, {k: np.ascontiguousarray(rec[:, q]).view(np.float64) for q, k in enumerate(F64)}
    absorbed = (rec[:, 9] >> np.uint64(63)) != 0
    sw["id"] = np.where(absorbed, rec[:, 9], rec[:, 9] & ~BIT63)
    low = lambda w: (w & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)      # noqa: E731
    sw["ip"], sw["jp"] = low(rec[:, 10]), low(rec[:, 10] >> np.uint64(32))
    sw["kp"] = low(rec[:, 11])
    gid = (rec[:, 11] >> np.uint64(32)).astype(np.int64)
    li = geom.local_index[gid]
    assert np.all(li >= 0), "a record for a block that is not resident"
    sw["blk"] = li.astype(np.int32)
    sw["status"] = np.where(absorbed, ST_ABSORBED, ST_ACTIVE).astype(np.int32)
    sw["rng"] = rec[:, 12].copy()
    out = np.array(edelta, dtype=np.float64, copy=True)
    a = np.flatnonzero(absorbed)
    w = sw["w"][a]
    assert np.all(w * 1024 == np.round(w * 1024)) and np.all(out * 1024 == np.round(out * 1024))
    np.add.at(out, (li[a], sw["kp"][a], sw["jp"][a], sw["ip"][a]), w)
    assert np.all(np.abs(out) < 2.0 ** 40)
    return {k: np.concatenate((before[k][:n], sw[k].astype(before[k].dtype, copy=False))) for k in KEYS}, out


def sorted_ok(geom, before, after, n):
    """sorted_failures as a yes or no"""
    return sorted_failures(geom, before, after, n) == []


# ---- which paths a swarm exercises -----------------------------------------------------------------------
def wave_census(key, first=0):
    """over the waves of 64 slots from `first`: (runs of equal keys that cross a wave boundary, full waves whose 64
    keys are all distinct)"""
    key = np.asarray(key)[first:]
    edge = np.arange(WAVE, len(key), WAVE)
    crossing = int((key[edge] == key[edge - 1]).sum())
    full = key[:len(key) // WAVE * WAVE].reshape(-1, WAVE)
    s = np.sort(full, axis=1)
    return crossing, int(np.all(np.diff(s, axis=1) != 0, axis=1).sum())


def run_starts(key):
    """{run length: set of lane offsets (slot % 64) at which a run of that length starts}"""
    key = np.asarray(key)
    start = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1])))
    length = np.diff(np.concatenate((start, [len(key)])))
    out = {}
    for s, m in zip(start.tolist(), length.tolist()):
        out.setdefault(m, set()).add(s % WAVE)
    return out


def clamp_census(geom, sw, n):
    """per active axis: (ACTIVE photons of a resident block whose cell index is clamped from below, from above)"""
    blk = sw["blk"][:n]
    ok = (sw["status"][:n] == ST_ACTIVE) & (blk >= 0) & (blk < geom.nblocks)
    raw = raw_cell_index(geom, sw, n)
    return [(int((ok & (raw[d] < 0)).sum()), int((ok & (raw[d] >= geom.dims[d])).sum())) for d in range(geom.ndim)]


def destination_census(owner, sw, first, last):
    """over the waves of 64 slots of [first, last): (waves that hold no outgoing photon, full waves whose 64 lanes
    go to 64 different ranks)"""
    st = sw["status"][first:last]
    out = (st == ST_OUTGOING) | (st == ST_OUTGOING_ABSORBED)
    rank = np.where(out, np.asarray(owner, dtype=np.int64)[np.where(out, sw["blk"][first:last], 0)], -1)
    m = len(st)
    pad = (-m) % WAVE
    none = int((~np.concatenate((out, np.zeros(pad, dtype=bool))).reshape(-1, WAVE).any(axis=1)).sum())
    full = rank[:m // WAVE * WAVE].reshape(-1, WAVE)
    s = np.sort(full, axis=1)
    distinct = np.all(np.diff(s, axis=1) != 0, axis=1) & (s[:, 0] >= 0)
    return none, int(distinct.sum())


# ---- the cases: meshes, sizes and layouts, shared by tests/test_swarm_ops_host.py and tests/test_gpu_swarm_ops.py -------
MESHES = {
    "1d": ("stepdiff", {"parthenon/mesh/nx1": 16, "parthenon/meshblock/nx1": 8, "jaybenne/num_particles": 64}),
    "3d": ("inf", {"parthenon/meshblock/nx1": 2, "parthenon/meshblock/nx2": 2, "parthenon/meshblock/nx3": 2,
                   "jaybenne/num_particles": 64}),
    "smr": ("stepdiff_smr", {"jaybenne/num_particles": 6000}),   # 2-D, two levels: block widths differ
}
# 1-D meshes whose histogram does not fit one stretch of 1024 tile sums: k_scan_sums carries a running offset from
# stretch to stretch.  Three blocks of 700 004 cells: 2 100 013 bins, 1026 tiles, two stretches -- the offset is
# handed on once.  Three blocks of 1 400 004 cells: 4 200 013 bins, 2051 tiles, three stretches -- the offset handed
# on the second time is the sum of BOTH stretches before it (after the first it is that stretch's total alone, so a
# carry that forgets what it was handed shows only from the third stretch on).
CARRY_MESHES = {
    "two stretches": ("stepdiff", {"parthenon/mesh/nx1": 2100000, "parthenon/meshblock/nx1": 700000,
                                   "jaybenne/num_particles": 64}),
    "three stretches": ("stepdiff", {"parthenon/mesh/nx1": 4200000, "parthenon/meshblock/nx1": 1400000,
                                     "jaybenne/num_particles": 64}),
}
CARRY_N = 4099
SCAN_TILE, SUMS_STRETCH = 2048, 1024       # kScanTile; entries k_scan_sums takes per trip
# 64 blocks of 4 cells, dealt to R ranks; the test holds rank 0's view
RANK_MESH = ("stepdiff", {"parthenon/mesh/nx1": 256, "parthenon/meshblock/nx1": 4, "jaybenne/num_particles": 64})
RANKS = (2, 8, 64)
SMALL_N = (1, 63, 64, 65, 255, 256, 257, 2049)
BLOCK = 256                                 # kBlock: threads per workgroup
MI355X_CUS = 256


def full_grid_n(multi_processor_count=MI355X_CUS):
    """one more than a full grid (8 workgroups per CU) and a ragged wave: every grid-stride loop takes a second trip"""
    return 8 * int(multi_processor_count) * BLOCK + 257


LAYOUTS = ("random", "all live", "none live", "one live at 0", "one live at n-1", "upper half live", "alternating waves")


def status_layout(layout, n, salt):
    """statuses of the compaction cases; the live slots cycle through the three live kinds, the dead through two"""
    i = np.arange(n)
    alive = {"random": _mod(i, salt, 2) == 1, "all live": np.ones(n, dtype=bool), "none live": np.zeros(n, dtype=bool),
             "one live at 0": i == 0, "one live at n-1": i == n - 1,
             "upper half live": i >= (n + 1) // 2,            # every live slot is a mover: as many as there can be
             "alternating waves": (i // WAVE) % 2 == 1}[layout]
    return np.where(alive, np.array(LIVE)[_mod(i, salt + 1, 3)], np.array(DEAD)[_mod(i, salt + 2, 2)]).astype(np.int32)


def host_view(case, rank=0, nranks=1):
    """(mesh, Geom) of one rank's view of a case's mesh, built on the host the way McblockDriver / MeshData build it:
    blocks dealt by Mesh.partition over block_costs, one ring of halo copies.  (The host objects supply arrays;
    nothing of the model is computed by them.)  tests/test_gpu_swarm_ops.py checks that the driver's view is this one."""
    from jaybenne_amd import mcblock
    from jaybenne_amd.deck import load_deck
    from jaybenne_amd.mesh import Mesh
    pin = load_deck(*case)
    mesh = Mesh.from_deck(pin)
    if nranks > 1:
        mesh.partition(nranks, cost=mcblock.block_costs(mesh, pin, mcblock.Initialize(pin)))
    owned = np.flatnonzero(np.asarray(mesh.owner) == rank) if nranks > 1 else np.arange(mesh.nblocks)
    halo = mesh.neighbours(owned, 1) if nranks > 1 else np.zeros(0, dtype=np.int64)
    return mesh, Geom(mesh, np.concatenate([owned, halo]), nowned=len(owned))


RUN_LENGTHS = (1, 2, 63, 64, 65, 200)      # 395 slots ...
SINGLES = 130                               # ... then 130 runs of one slot: two whole waves of distinct keys; 525 slots
#                                             in all, 13 mod 64: the pattern starts at every lane offset in turn


def run_layout(geom, n):
    """(status, keys) of a swarm made of runs of equal keys: the pattern RUN_LENGTHS, then SINGLES runs of length 1,
    over and over; consecutive runs take different cells (7 cells on, modulo the interior cells); every fifth run of
    the pattern is a run of slots that are not ACTIVE (the key behind all cells)."""
    ncells = geom.nblocks * geom.ncell
    assert math.gcd(7, ncells) == 1
    lengths, dead = [], []
    while sum(lengths) < n:
        for q, m in enumerate(RUN_LENGTHS):
            lengths.append(m)
            dead.append((len(lengths) % 5) == 0)
        lengths += [1] * SINGLES
        dead += [False] * SINGLES
    run = np.repeat(np.arange(len(lengths)), lengths)[:n]
    keys = (7 * run) % ncells
    status = np.where(np.array(dead)[run], np.array(DEAD + (ST_OUTGOING,))[run % 3], ST_ACTIVE).astype(np.int32)
    return status, keys


def sort_swarm(geom, group, n, salt):
    """the three groups of the sort cases: "hashed" -- hashed keys in a hashed slot order, every position inside its
    cell, every blk valid; "runs" -- run_layout; "edges" -- hashed, with the out-of-block positions and out-of-range
    blk values of crafted()"""
    if group == "runs":
        status, keys = run_layout(geom, n)
        return crafted(geom, n, salt, status=status, keys=keys, edges=False, bad_blk=False)
    return crafted(geom, n, salt, edges=group == "edges", bad_blk=group == "edges")


def carry_tiles(geom):
    """the scan tiles the carry case puts keys in: the first and the last of every stretch of 1024 tile sums"""
    tiles = (geom.nkeys + 1 + SCAN_TILE - 1) // SCAN_TILE
    assert tiles > SUMS_STRETCH + 1
    edge = sorted({t for s in range(0, tiles, SUMS_STRETCH) for t in (s, min(s + SUMS_STRETCH, tiles) - 1)})
    return tiles, edge


def carry_swarm(geom, n, salt):
    """photons whose keys fall in the first and the last scan tile of every stretch (tiles 0, 1023, 1024, ... and the
    last one), in the last cell's bin and, the slots that are not ACTIVE, in the bin behind all cells"""
    tiles, edge = carry_tiles(geom)
    targets = np.array([t * SCAN_TILE + off for t in edge for off in (3, 700, 701, SCAN_TILE - 1)
                        if t * SCAN_TILE + off < geom.nkeys] + [geom.nkeys - 1])
    # a target key -> the interior cell whose key it is (ghost keys: moved to the nearest interior cell of the block)
    b, cell = targets // geom.ntot, targets % geom.ntot
    interior = np.clip(cell - geom.ng, 0, geom.nx[0] - 1)
    keys = (b * geom.ncell + interior)[_mod(np.arange(n), salt + 5, len(targets))]
    status = np.where(_mod(np.arange(n), salt + 6, 8) == 0, ST_ESCAPED, ST_ACTIVE)
    return crafted(geom, n, salt, status=status, keys=keys, edges=True, bad_blk=True)


STRETCH = 130       # slots: holds a whole wave wherever the range starts


def pack_swarm(geom, n, salt, rank=0, to_self=True, arrivals=False):
    """A swarm for the pack cases on one rank's view: hashed statuses; every outgoing photon's blk is a global block
    id, hashed over the whole mesh (``to_self`` False: over the blocks of the other ranks only, as jb_exchange
    demands).  From slot 256 on (n permitting) STRETCH outgoing slots whose destinations cycle through the first
    block of every rank -- 64 different ranks in a wave when there are 64 --, then STRETCH slots of which none is
    outgoing."""
    i = np.arange(n)
    ids = _hash(i, salt) >> np.uint64(1)
    h = _mod(ids, salt + 11, 8)
    status = np.array([ST_ACTIVE, ST_ACTIVE, ST_ABSORBED, ST_ESCAPED, ST_OUTGOING, ST_OUTGOING, ST_OUTGOING_ABSORBED,
                       ST_OUTGOING_ABSORBED])[h]
    nranks = int(geom.owner.max()) + 1
    allowed = np.flatnonzero(geom.owner != rank) if not to_self else np.arange(geom.nblocks_total)
    dest = allowed[_mod(ids, salt + 13, len(allowed))]
    first_of = np.array([np.flatnonzero(geom.owner == r)[0] for r in range(nranks) if to_self or r != rank])
    a, b, c = min(n, 256), min(n, 256 + STRETCH), min(n, 256 + 2 * STRETCH)
    status[a:b] = np.where(i[a:b] % 3 == 0, ST_OUTGOING_ABSORBED, ST_OUTGOING)
    dest[a:b] = first_of[(i[a:b] - a) % len(first_of)]
    status[b:c] = np.array([ST_ACTIVE, ST_ABSORBED, ST_ESCAPED])[i[b:c] % 3]
    sw = crafted(geom, n, salt, status=status, dest=dest, arrivals=arrivals)
    return sw, (b, c)


def pack_ranges(n, quiet):
    """the [first, last) ranges of the pack cases: all, ragged at both ends, five slots inside a wave, empty, and
    one that holds no outgoing photon (inside the quiet stretch of pack_swarm)"""
    out = [(0, n)]
    if n >= 3:
        out.append((1, n - 1))
    if n >= 70:
        out.append((65, 70))
    out.append((n // 2, n // 2))
    if quiet[1] - quiet[0] >= 2:
        out.append((quiet[0] + 1, quiet[1] - 1))
    return out


SALT = {"compact": 101, "sort": 211, "carry": 307, "pack": 401, "base": 503, "resident": 601, "arrivals": 701,
        "exchange": 809}
