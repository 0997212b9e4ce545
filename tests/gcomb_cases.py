"""The crafted swarms of the global comb's tests (tests/test_gcomb_host.py counts the cases, tests/test_gpu_gcomb.py runs
them on the GPU).  A swarm is laid out cell by cell over the interior cells of a mesh in key order, so consecutive
specs are neighbours in the sorted swarm.

Crafted weights are integers times 2^-20 and the total weight of the valid cells is N 2^-4 exactly, so that every sum
is exact in any order, scale = N / W_tot = 16 exactly and nu = 16 W_k is known: a cell with an integer nu gets
K = nu whatever its draw, a cell with a fractional nu (multiples of 1/16) takes its draw."""
from collections import namedtuple

import numpy as np

UNIT = 2.0 ** -4                    # weight per photon of the target population
Q = 1 << 16                         # UNIT in units of 2^-20
R_BAND, S_MAX = 2.0, 5000           # the band and the split limit the crafted cases are written for
N_DEAD, N_BADBLK = 37, 5
SCAN_TILE = 2048

# m photons; nu16 = 16 nu (None: not a valid cell); kind: how the weights are dealt; tag: the case it stands for
Spec = namedtuple("Spec", "m nu16 kind tag")


def _hash(i, salt):
    x = (np.atleast_1d(i).astype(np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    return x if np.ndim(i) else x[0]


def _unit(i, salt):
    return ((_hash(i, salt) >> np.uint64(11)) % np.uint64(1 << 20)).astype(np.float64) / float(1 << 20)


TILE_PADS = (0, 22, 44)             # with TILE_CELLS cells of 2049 behind each: every lane offset 0 .. 63 is a start
TILE_CELLS = 22


def tile_specs(pad):
    """``pad`` photons in one cell, then TILE_CELLS cells of 2049 photons (2049 = 1 mod 64: each starts one lane
    further than the one before): thinned to 500, left alone, split to 4100 in turn.  The three pads of TILE_PADS
    together start a 2049-photon cell -- the size that crosses a scan tile -- at every lane offset."""
    out = [Spec(pad, 16 * pad, "hashed", "pad")] if pad else []
    for q in range(TILE_CELLS):
        out.append(Spec(2049, (16 * 500, 16 * 2049, 16 * 4100)[q % 3], "hashed", "tile-2049"))
    return out


def specs(max_cells, pad=None):
    """The cells, in key order.  Every case of the issue's list is here; the sweep of cell sizes over the lane offsets
    is as long as the mesh has cells for.  ``pad``: the swarm of tile_specs(pad) instead."""
    if pad is not None:
        return tile_specs(pad)
    fixed = [
        Spec(2049, 16 * 500, "hashed", "m2049-thin"), Spec(2049, 16 * 5000, "hashed", "m2049-split"),
        Spec(2049, 16 * 2049, "hashed", "m2049-alone"),
        Spec(1, 16 * 2, "hashed", "one-to-2"), Spec(1, 16 * 64, "hashed", "one-to-64"),
        Spec(1, 16 * 65, "hashed", "one-to-65"), Spec(1, 16 * 5000, "hashed", "one-to-5000"),
        Spec(1, 16 * 6000, "hashed", "S-binds"),
        Spec(2 * SCAN_TILE + 100, 16, "hashed", "three-tiles-to-1"),
        Spec(40, 16 * 10, "hashed", "thin-before-split"), Spec(5, 16 * 20, "hashed", "split-between"),
        Spec(40, 16 * 10, "hashed", "thin-after-split"),
        Spec(10, 16 * 30, "dominant", "zero-copies-in-split"),
        Spec(7, None, "floor", "floor-holds-1"),
        Spec(5, None, "zeros", "all-zero"), Spec(3, None, "negative", "negative"), Spec(4, None, "inf", "inf"),
        Spec(6, 16 * 2, "ghost", "ghost-cell"),
    ]
    sweep = []
    cycles = max(0, min(64, (max_cells - len(fixed) - 1) // 5))
    q = 0
    for c in range(cycles):
        for m in (1, 2, 63, 64, 65):
            mode = q % 4
            nu16 = (16 * max(1, m // 4), 16 * 3 * m, 16 * m, 48 * m + 6)[mode]    # thin, split, alone, split by a draw
            sweep.append(Spec(m, nu16, "hashed", f"sweep-{m}"))
            q += 1
    return sweep + fixed


def _deal(total, m, salt, allow_zero=False):
    """m integers that sum to ``total``: hashed cut points; every part >= 1 unless allow_zero."""
    if m == 1:
        return np.array([total], dtype=np.int64)
    room = total if allow_zero else total - m
    assert room >= 0
    cuts = np.sort((_hash(np.arange(m - 1), salt) % np.uint64(room + 1)).astype(np.int64))
    parts = np.diff(np.concatenate(([0], cuts, [room])))
    return parts if allow_zero else parts + 1


def _interior_cells(mesh, nblocks):
    nx = [int(v) for v in mesh.nx]
    ncell = nx[0] * nx[1] * nx[2]
    return nx, ncell, nblocks * ncell


def crafted(mesh, local_gids, salt, weights="crafted", pad=None):
    """(swarm dict in a hashed slot order, N, the specs with the key each landed on).  ``weights``: "crafted"
    (integers times 2^-20, nu known) or "hashed" (floating point over six decades: the same cells, nu unknown).
    ``pad``: the cells of tile_specs(pad) instead of those of specs()."""
    gids = np.asarray(local_gids)
    nx, ncell, ncells = _interior_cells(mesh, len(gids))
    sp = specs(ncells, pad)
    assert len(sp) + 1 <= ncells, "the mesh has too few cells for the fixed cases"
    # spread the specs over the interior cells in key order, leaving every seventh cell empty
    slots_for = [c for c in range(ncells) if c % 7 != 3][:len(sp) + 1]
    if len(slots_for) < len(sp) + 1:
        slots_for = list(range(len(sp) + 1))
    ng = mesh.ng
    nk, nj, ni = mesh.field_shape[1:]
    rows, placed = [], []
    nu16_sum = 0
    for q, s in enumerate(sp):
        c = slots_for[q]
        blk, cc = c // ncell, c % ncell
        ijk = [cc % nx[0], (cc // nx[0]) % nx[1], cc // (nx[0] * nx[1])]
        if s.kind == "ghost":
            ijk[0] = -1                                     # half a cell outside the block: clamped into the ghost cell
        if s.kind == "floor":
            wi = np.ones(s.m, dtype=np.int64)               # nu = 7 / 65536
            nu16 = None
        elif s.kind == "zeros":
            wi = np.zeros(s.m, dtype=np.int64)
        elif s.kind in ("negative", "inf"):
            wi = -(1 + np.arange(s.m, dtype=np.int64))
        elif s.kind == "dominant":
            wi = np.ones(s.m, dtype=np.int64)
            wi[s.m // 2] = s.nu16 * (Q // 16) - (s.m - 1)
        else:
            wi = _deal(s.nu16 * (Q // 16), s.m, salt + 1000 + q, allow_zero=s.nu16 * (Q // 16) < s.m)
        w = wi.astype(np.float64) * 2.0 ** -20
        if s.kind == "inf":
            w[1] = np.inf
        if s.nu16 is not None:
            nu16_sum += s.nu16
        ci = [ijk[d] + (ng if d < mesh.ndim else 0) for d in range(3)]
        key = blk * (nk * nj * ni) + (ci[2] * nj + ci[1]) * ni + ci[0]
        placed.append((s, int(key)))
        for j in range(s.m):
            rows.append((blk, ijk[0], ijk[1], ijk[2], w[j]))
    # the floor cell's weight counts: 7 x 2^-20; the filler cell brings the total to N UNIT exactly
    floor16 = sum(s.m for s in sp if s.kind == "floor")     # in units of 2^-20
    N = nu16_sum // 16 + 201
    fill_int = N * Q - nu16_sum * (Q // 16) - floor16
    m_fill = 150
    c = slots_for[len(sp)]
    blk, cc = c // ncell, c % ncell
    ijk = [cc % nx[0], (cc // nx[0]) % nx[1], cc // (nx[0] * nx[1])]
    wf = _deal(fill_int, m_fill, salt + 7).astype(np.float64) * 2.0 ** -20
    ci = [ijk[d] + (ng if d < mesh.ndim else 0) for d in range(3)]
    placed.append((Spec(m_fill, None, "filler", "filler"), int(blk * (nk * nj * ni) + (ci[2] * nj + ci[1]) * ni + ci[0])))
    for j in range(m_fill):
        rows.append((blk, ijk[0], ijk[1], ijk[2], wf[j]))
    n_act = len(rows)
    # slots that are not ACTIVE, and ACTIVE ones with a block index outside the view: carried along behind all cells
    for j in range(N_DEAD + N_BADBLK):
        rows.append((int(_hash(j, salt + 9) % np.uint64(len(gids))), 0, 0, 0, 0.25 + j))
    n = len(rows)
    arr = np.array(rows, dtype=np.float64)
    blk = arr[:, 0].astype(np.int64)
    i = np.arange(n)
    sw = {}
    g = gids[blk]
    for d, name in enumerate(("x", "y", "z")):
        if d < mesh.ndim:
            sw[name] = mesh.blk_xmin[g, d] + (arr[:, 1 + d] + 0.05 + 0.9 * _unit(i, salt + 31 + d)) * mesh.blk_dx[g, d]
        else:
            sw[name] = np.zeros(n)
    for q, name in enumerate(("vx", "vy", "vz", "t", "e")):
        sw[name] = _unit(i, salt + 50 + q) - 0.5
    w = arr[:, 4].copy()
    if weights == "hashed":
        ok = np.isfinite(w) & (w > 0.0)
        # (four decades from photon to photon, two from cell to cell: some cells hold much more than their share)
        code = ((blk * 64 + (arr[:, 1] + 1).astype(np.int64)) * 64 + arr[:, 2].astype(np.int64)) * 64 + arr[:, 3].astype(np.int64)
        w[ok] = 10.0 ** (-3.0 + 4.0 * _unit(i[ok], salt + 70) + 2.0 * _unit(code[ok], salt + 71))
    sw["w"] = w
    sw["ip"] = (arr[:, 1] + ng).astype(np.int32)
    sw["jp"] = (arr[:, 2] + (ng if mesh.ndim >= 2 else 0)).astype(np.int32)
    sw["kp"] = (arr[:, 3] + (ng if mesh.ndim >= 3 else 0)).astype(np.int32)
    status = np.zeros(n, dtype=np.int32)
    status[n_act:n_act + N_DEAD] = 1 + (np.arange(N_DEAD) % 2)          # ABSORBED / ESCAPED
    sw["status"] = status
    blk32 = blk.astype(np.int32)
    blk32[n_act + N_DEAD:] = np.array([-1, len(gids), len(gids) + 7, -5, 1 << 20], dtype=np.int32)[:N_BADBLK]
    sw["blk"] = blk32
    sw["id"] = (i + 1000).astype(np.uint64)
    sw["rng"] = _hash(i, salt + 99)
    order = np.argsort(_hash(i, salt + 123))
    return {k: np.ascontiguousarray(v[order]) for k, v in sw.items()}, int(N), placed
