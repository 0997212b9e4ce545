"""The global census comb (include/jaybenne_amd.h: jb_comb_census_weigh / _plan_global / _apply) restated in numpy,
from its rule -- never from the library.  Keys, xi and the in-cell rule come from comb_model, the block and total
trees from source_alloc_model, the count draw xi' from the CPU oracle's generator in domain 9.

Per valid cell (m >= 1 ACTIVE photons, 0 < W < inf):  nu = W scale, f = floor(nu), K = f + ((nu - f) > xi'),
K = max(K, 1), K = min(K, S m, 2^32 - 1); combed iff m > r K or K > r m; a combed cell comes out as K copies of
weight W / K by comb_model's rule with u_m = K."""
import math

import numpy as np

import comb_model as cm
import source_alloc_model as sam

RNG_DOMAIN_COMB_COUNT = 9
SWARM_KEYS = cm.SWARM_KEYS


def xi_count_of(seed: int, epoch: int, gblock: int, cell: int) -> float:
    """xi' of the cell: keyed as comb_model.xi_of is, in domain 9."""
    from oracle import orc
    assert 0 <= epoch < (1 << 20) and 0 <= gblock < (1 << 20) and 0 <= cell < (1 << 24)
    return cm.u52_to_double(orc.seed_state(seed, RNG_DOMAIN_COMB_COUNT, (epoch << 44) | (gblock << 24) | cell) >> 12)


def _join(a, b):
    """(sum of the open segment, "a segment started in here") of a, then b"""
    return np.where(b[1] != 0, b[0], a[0] + b[0]), a[1] | b[1]


def _wave_scan(s, f):
    """Inclusive and exclusive segmented scan over the last axis (64 lanes) by shuffles: d = 1, 2, .. 32."""
    lane = np.arange(64)
    for d in (1, 2, 4, 8, 16, 32):
        us, uf = np.roll(s, d, axis=-1), np.roll(f, d, axis=-1)
        js, jf = _join((us, uf), (s, f))
        s, f = np.where(lane >= d, js, s), np.where(lane >= d, jf, f)
    es, ef = np.roll(s, 1, axis=-1), np.roll(f, 1, axis=-1)
    es, ef = np.where(lane == 0, 0.0, es), np.where(lane == 0, 0, ef)
    return (s, f), (es, ef)


def running_tree(key, w):
    """C_j of the default order over the WHOLE sorted swarm, by the fixed tree the header of the comb's kernels
    states: tiles of 2048 slots aligned to slot 0; in a tile 256 lanes of 8 consecutive slots each, a lane over its
    slots in slot order, a wave of 64 lanes by shuffles, the 4 waves in wave order; the tiles' carries by one
    workgroup in tile order; a carry is added to the slots that continue the segment before the tile.  Slots behind
    the swarm are empty segments of their own."""
    n = len(w)
    if n == 0:
        return np.zeros(0)
    nt = (n + 2047) // 2048
    assert nt <= 64, "the model scans the tiles' carries in one wave"
    kp = np.full(nt * 2048, -1, dtype=np.int64)
    kp[:n] = key
    wp = np.zeros(nt * 2048)
    wp[:n] = w
    head = np.ones(nt * 2048, dtype=bool)
    head[1:n] = kp[1:n] != kp[:n - 1]
    H, Wt = head.reshape(nt, 256, 8), wp.reshape(nt, 256, 8)
    v = np.zeros((nt, 256, 8))
    run = np.zeros((nt, 256))
    seen = np.zeros((nt, 256), dtype=bool)
    cont = np.zeros((nt, 256, 8), dtype=bool)
    for q in range(8):
        run = np.where(H[:, :, q], Wt[:, :, q], run + Wt[:, :, q])
        v[:, :, q] = run
        seen = seen | H[:, :, q]
        cont[:, :, q] = ~seen
    s, f = run.reshape(nt, 4, 64), seen.astype(np.int64).reshape(nt, 4, 64)
    (is_, if_), (es, ef) = _wave_scan(s, f)
    ws, wf = is_[:, :, 63], if_[:, :, 63]
    before = (np.zeros((nt, 4)), np.zeros((nt, 4), dtype=np.int64))
    total = (np.zeros(nt), np.zeros(nt, dtype=np.int64))
    for q in range(4):
        p = (ws[:, q], wf[:, q])
        js, jf = _join((before[0], before[1]), (p[0][:, None], p[1][:, None]))
        later = np.arange(4)[None, :] > q
        before = (np.where(later, js, before[0]), np.where(later, jf, before[1]))
        total = _join(total, p)
    opn = _join((before[0][:, :, None], before[1][:, :, None]), (es, ef))[0].reshape(nt, 256)
    C = np.where(cont, opn[:, :, None] + v, v).reshape(-1)
    # the tiles' (sum, flag), scanned exclusively by one wave (lanes behind the tiles: empty)
    ts, tf = np.zeros(64), np.zeros(64, dtype=np.int64)
    ts[:nt], tf[:nt] = total
    _, (xs, xf) = _wave_scan(ts, tf)
    carry = _join((np.zeros(64), np.zeros(64, dtype=np.int64)), _join((np.zeros(64), np.zeros(64, dtype=np.int64)), (xs, xf)))[0]
    for t in range(1, nt):
        a = t * 2048
        sel = np.flatnonzero(kp[a:a + 2048] == kp[a - 1]) + a
        C[sel] = carry[t] + C[sel]
    return C[:n]


def running_exact(w):
    """C_j under cell_order = id: 128-bit fixed-point sums on the scale of the cell's largest weight -- its mantissa
    at bits 42..94, smaller weights truncated below bit 0, negative weights zero --, converted as
    (double)hi 2^64 + (double)lo with every conversion and the sum rounded to nearest, then scaled by a power of two.
    A cell with a weight that is not finite: inf everywhere."""
    w = np.asarray(w, dtype=np.float64)
    if not np.all(np.isfinite(w)):
        return np.full(len(w), np.inf)
    pos = w[w > 0.0]
    if len(pos) == 0:
        return np.zeros(len(w))
    assert pos.min() >= 2.0 ** -1022, "the model leaves subnormal weights out"
    emax = math.frexp(float(pos.max()))[1]
    out = np.zeros(len(w))
    acc = 0
    for j, v in enumerate(w.tolist()):
        if v > 0.0:
            mant, ex = math.frexp(v)
            M = int(mant * 2.0 ** 53)
            sh = ex - emax + 42
            acc += (M << sh) if sh >= 0 else (M >> -sh)
        hi, lo = divmod(acc, 1 << 64)
        out[j] = math.ldexp(float(hi) * 18446744073709551616.0 + float(lo), emax - 95)
    return out


def target_of(W: float, m: int, scale: float, S: int, xi_count: float) -> int:
    nu = W * scale
    f = math.floor(nu) if math.isfinite(nu) else nu
    if math.isfinite(nu):
        K = float(f) + (1.0 if (nu - float(f)) > xi_count else 0.0)
    else:
        K = nu
    K = max(K, 1.0)
    K = min(K, float(S) * float(m), 4294967295.0)
    return int(K)


def is_combed(m: int, K: int, r: float) -> bool:
    return float(m) > r * float(K) or float(K) > r * float(m)


def counts_of(C: np.ndarray, K: int, xi: float):
    """(k_j, D) of one combed cell from its running weights: comb_model.comb_counts with C given."""
    delta = C[-1] / K
    u = np.clip(np.ceil(C / delta - xi), 0, K).astype(np.int64)
    u[-1] = K
    return np.diff(np.concatenate(([0], u))), delta


def margin_of(C: np.ndarray, W: float, m: int, K: int, nu: float, xi_count: float, xi: float, r: float, combed: bool):
    """The smallest distance of the cell from a decision: the draw threshold of the target, a band edge, an integer
    on the u_j."""
    d = [abs((nu - math.floor(nu)) - xi_count)] if math.isfinite(nu) else []
    # (a band edge met exactly is no floating-point decision: m, K and r are the same numbers on every side)
    d += [v for v in (abs(float(m) - r * K) / max(float(m), 1.0), abs(K - r * float(m)) / max(float(K), 1.0)) if v > 0.0]
    if combed and len(C) > 1:
        q = C[:-1] / (W / K) - xi
        d.append(float(np.abs(q - np.round(q)).min()))
    return min(d)


def weigh(mesh, local_gids, owned, sw, n: int, exact: bool, sort: bool = True):
    """Steps 1 and 2: (order, key, C, cells, e_block) with cells = {key: (a, b, W, valid)} over the occupied cells of
    the swarm in (block, cell) order and e_block one sum per resident block."""
    key, cell, nkeys, ntot = cm.cell_keys(mesh, local_gids, sw, n)
    order = np.argsort(key, kind="stable") if sort else np.arange(n)
    key = key[order]
    assert np.all(np.diff(key) >= 0), "the swarm is not in (block, cell) order"
    w = sw["w"][:n][order]
    C = np.zeros(n) if exact else running_tree(key, w)
    cells = {}
    Wcell = np.zeros(len(local_gids) * ntot)
    bounds = np.flatnonzero(np.diff(np.concatenate(([-1], key, [nkeys + 1]))))
    for a, b in zip(bounds[:-1], bounds[1:]):
        k = int(key[a])
        if k >= nkeys:
            continue
        if exact:
            C[a:b] = running_exact(w[a:b])
        W = float(C[b - 1])
        valid = 0.0 < W < math.inf
        cells[k] = (int(a), int(b), W, valid)
        if valid:
            Wcell[k] = W
    e_block = np.array([sam.block_sum(Wcell[q * ntot:(q + 1) * ntot]) if owned[q] else 0.0
                        for q in range(len(local_gids))])
    return order, key, C, cells, e_block, nkeys, ntot


def gcomb_swarm(mesh, local_gids, owned, sw, n: int, N: int, r: float, S: int, seed: int, epoch: int, id_base: int,
                exact: bool = False, sort: bool = True, w_total=None):
    """The whole call on a swarm given as a dict of arrays (slots 0..n-1).  ``w_total``: the total of all ranks'
    block sums where this swarm is one rank's; else this swarm's own.  Returns (new swarm dict, info)."""
    from oracle import orc
    order, key, C, cells, e_block, nkeys, ntot = weigh(mesh, local_gids, owned, sw, n, exact, sort)
    if w_total is None:
        by_gid = np.zeros(mesh.nblocks)
        by_gid[np.asarray(local_gids)] = e_block
        w_total = sam.total(by_gid)
    w = sw["w"][:n][order]
    counts = np.ones(n, dtype=np.int64)
    new_w = w.copy()
    info = dict(order=order, key=key, e_block=e_block, w_total=w_total, targets={}, combed={}, margins={}, nu={},
                cells_thinned=0, cells_split=0, max_target=0, cells=cells,
                max_per_cell=max([b - a for a, b, _, _ in cells.values()], default=0))
    go = w_total > 0.0 and math.isfinite(w_total)
    scale = float(N) / w_total if go else 0.0
    info["scale"] = scale
    for k, (a, b, W, valid) in cells.items():
        if not (go and valid):
            continue
        m = b - a
        g, c = int(local_gids[k // ntot]), k % ntot
        xc = xi_count_of(seed, epoch, g, c)
        K = target_of(W, m, scale, S, xc)
        combed = is_combed(m, K, r)
        xi = cm.xi_of(seed, epoch, g, c)
        info["targets"][k], info["nu"][k] = K, W * scale
        info["max_target"] = max(info["max_target"], K)
        info["margins"][k] = margin_of(C[a:b], W, m, K, W * scale, xc, xi, r, combed)
        if combed:
            counts[a:b], delta = counts_of(C[a:b], K, xi)
            new_w[a:b] = delta
            info["combed"][k] = K
            info["cells_thinned" if K < m else "cells_split"] += 1
    src = np.repeat(np.arange(n), counts)
    first = np.concatenate(([True], src[1:] != src[:-1])) if len(src) else np.zeros(0, dtype=bool)
    out = {name: sw[name][:n][order][src].copy() for name in SWARM_KEYS}
    out["w"] = new_w[src]
    extra = np.flatnonzero(~first)
    ids = np.uint64(id_base) + np.arange(len(extra), dtype=np.uint64)
    out["id"][extra] = ids
    out["rng"][extra] = np.array([orc.stream_start(seed, int(i)) for i in ids], dtype=np.uint64)
    info.update(n_after=len(src), n_new_ids=len(extra), counts=counts, src=src)
    return out, info
