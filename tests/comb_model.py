"""The census comb (include/jaybenne_amd.h: jb_comb_census_plan) restated in numpy, from its rule -- never from the
library.  Random numbers come from the CPU oracle's generator (oracle.orc.seed_state / stream_start).

For a cell with photons j = 1..m in slot order, W = sum w_j, D = W / K, C_j = w_1 + .. + w_j and xi in (0,1):
    u_0 = 0,   u_j = clamp(ceil(C_j / D - xi), 0, K) for j < m,   u_m = K,   k_j = u_j - u_(j-1)
copies of weight D each.  The first copy keeps id and stream state; further copies take consecutive new ids, in
output-slot order over the whole call, and the start of that id's stream."""
import numpy as np

RNG_DOMAIN_COMB = 2
ST_ACTIVE = 0
SWARM_KEYS = ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e", "ip", "jp", "kp", "blk", "status", "id", "rng")


def u52_to_double(k52: int) -> float:
    return (float(k52) + 0.5) * 2.0 ** -52


def xi_of(seed: int, epoch: int, gblock: int, cell: int) -> float:
    """The cell's uniform: one draw of the state seeded by (epoch << 44 | global block id << 24 | cell)."""
    from oracle import orc
    assert 0 <= epoch < (1 << 20) and 0 <= gblock < (1 << 20) and 0 <= cell < (1 << 24)
    return u52_to_double(orc.seed_state(seed, RNG_DOMAIN_COMB, (epoch << 44) | (gblock << 24) | cell) >> 12)


def comb_counts(w: np.ndarray, K: int, xi: float):
    """(k_j, D) of one combed cell; C by sequential summation in slot order."""
    C = np.cumsum(np.asarray(w, dtype=np.float64))
    delta = C[-1] / K
    u = np.clip(np.ceil(C / delta - xi), 0, K).astype(np.int64)
    u[-1] = K
    return np.diff(np.concatenate(([0], u))), delta


def comb_margin(w: np.ndarray, K: int, xi: float) -> float:
    """The smallest distance of some C_j / D - xi (j < m) from an integer: where it is tiny, the last bit of a running
    sum decides a count, and two ways of summing may differ."""
    C = np.cumsum(np.asarray(w, dtype=np.float64))
    if len(C) < 2:
        return 1.0
    r = C[:-1] / (C[-1] / K) - xi
    return float(np.abs(r - np.round(r)).min())


def cell_keys(mesh, local_gids, sw, n: int):
    """(key, cell) per slot as the sort forms them: key = local block * cells per block + cell, cell = index in the
    block's array (ghosts included) of the cell that holds the POSITION; slots that are not ACTIVE: key = nkeys."""
    nk, nj, ni = mesh.field_shape[1:]
    ntot = nk * nj * ni
    nkeys = len(local_gids) * ntot
    blk = sw["blk"][:n].astype(np.int64)
    g = np.asarray(local_gids)[np.clip(blk, 0, len(local_gids) - 1)]
    ng = mesh.ng
    idx = []
    for d, name, size in ((0, "x", ni), (1, "y", nj), (2, "z", nk)):
        if d < mesh.ndim:
            q = np.floor((sw[name][:n] - mesh.blk_xmin[g, d]) * (1.0 / mesh.blk_dx[g, d])).astype(np.int64) + ng
        else:
            q = np.zeros(n, dtype=np.int64)
        idx.append(np.clip(q, 0, size - 1))
    cell = (idx[2] * nj + idx[1]) * ni + idx[0]
    key = blk * ntot + cell
    dead = (sw["status"][:n] != ST_ACTIVE) | (blk < 0) | (blk >= len(local_gids))
    key[dead] = nkeys
    return key, cell, nkeys, ntot


def comb_swarm(mesh, local_gids, sw, n: int, T: int, K: int, seed: int, epoch: int, id_base: int, sort: bool = True):
    """The whole call on a swarm given as a dict of arrays (slots 0..n-1).  ``sort``: bring the slots into key order
    first (stable: the order within a cell is the input's).  Returns (new swarm dict, info) with info = n_after,
    n_new_ids, cells_combed, max_per_cell, counts (k_j per input slot, in the order combed), order (the slot
    permutation applied first), margins {key: comb_margin} of the combed cells."""
    from oracle import orc
    assert 1 <= K <= T
    key, cell, nkeys, ntot = cell_keys(mesh, local_gids, sw, n)
    order = np.argsort(key, kind="stable") if sort else np.arange(n)
    assert np.all(np.diff(key[order]) >= 0), "the swarm is not in (block, cell) order"
    key, cell = key[order], cell[order]
    w = sw["w"][:n][order]
    counts = np.ones(n, dtype=np.int64)
    new_w = w.copy()
    margins = {}
    bounds = np.flatnonzero(np.diff(np.concatenate(([-1], key, [nkeys + 1]))))
    most = 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        k = int(key[a])
        if k >= nkeys:
            continue
        most = max(most, b - a)
        W = float(np.cumsum(w[a:b])[-1])
        if b - a <= T or not (0.0 < W < np.inf):
            continue
        xi = xi_of(seed, epoch, int(local_gids[k // ntot]), k % ntot)
        counts[a:b], delta = comb_counts(w[a:b], K, xi)
        new_w[a:b] = delta
        margins[k] = comb_margin(w[a:b], K, xi)
    src = np.repeat(np.arange(n), counts)                       # source slot (of the sorted order) per output slot
    first = np.concatenate(([True], src[1:] != src[:-1])) if len(src) else np.zeros(0, dtype=bool)
    out = {name: sw[name][:n][order][src].copy() for name in SWARM_KEYS}
    out["w"] = new_w[src]
    extra = np.flatnonzero(~first)
    ids = np.uint64(id_base) + np.arange(len(extra), dtype=np.uint64)
    out["id"][extra] = ids
    out["rng"][extra] = np.array([orc.stream_start(seed, int(i)) for i in ids], dtype=np.uint64)
    info = dict(n_after=len(src), n_new_ids=len(extra), cells_combed=len(margins), max_per_cell=int(most),
                counts=counts, order=order, margins=margins, key=key)
    return out, info
