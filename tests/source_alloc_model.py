"""Energy-proportional source allocation (include/jaybenne_amd.h: jb_set_source_allocation) restated in numpy and
Python floats, operation for operation and in the order the contract writes them: the reference of
tests/test_source_alloc_host.py (CPU) and tests/test_gpu_source_alloc.py.  numpy rounds every operation on its own
and fuses nothing, / is correctly rounded as the library's is, and no expression below mixes a product with a sum.
The rounding draw and the photons' draws come from the oracle's primitives (``orc.seed_state``, ``orc.stream_start``,
``orc.draw_stream``; the photons' direction and frequency from its portable math).
"""
from __future__ import annotations

import math

import numpy as np

THREADS = 256
RNG_DOMAIN_CELL = 1                     # jb_rng.hpp: kRngDomainCell
THERMAL, EMISSION = 0, 1
ST_ACTIVE = 0
INT32_MAX = 2 ** 31 - 1


def cell_stream_id(epoch, gblock, cell):
    return (int(epoch) << 44) | (int(gblock) << 24) | int(cell)


# ------------------------------------------------------------------------------------------------ 1. energy pass
def temperature(sie, cv):
    """eos_temperature of the ideal gas: sie / cv where that is positive, else 0."""
    with np.errstate(invalid="ignore"):
        t = sie / cv
        return np.where(t > 0.0, t, 0.0)


def erad_thermal(sie, cv, sb, c, dv):
    """((4 sb / c) (T^2 T^2)) dv -- k_source_count's expression and product order (sourcing.cpp:93)."""
    t = temperature(sie, cv)
    t2 = t * t
    return ((4.0 * sb / c) * (t2 * t2)) * dv


def erad_emission(rho, sie, fleck, cv, sb, kappa, dv, dt, ep_E=None):
    """((fleck j) dv) dt with the gray emissivity j = (rho kappa) ((4 sb) (T^2 T^2)) (sourcing.cpp:95-96) or, with
    ``ep_E`` (the EPBremss coefficient E in code units, include/jaybenne_amd.h), j = (E (rho rho)) sqrt(T)."""
    t = temperature(sie, cv)
    if ep_E is not None:
        j = (ep_E * (rho * rho)) * np.sqrt(t)
    else:
        t2 = t * t
        j = (rho * kappa) * ((4.0 * sb) * (t2 * t2))
    return ((fleck * j) * dv) * dt


def block_sum(a):
    """The block's sum in the kernel's order: thread t of 256 starts from +0.0 and adds the cells t, t + 256, ... in
    rising order; then s[t] += s[t + d] for t < d, d = 128, 64, ... 1; the sum is s[0]."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    s = np.zeros(THREADS)
    for row in range(0, a.size, THREADS):          # one cell per thread and row: thread t adds cell row + t
        chunk = a[row:row + THREADS]
        s[:chunk.size] = s[:chunk.size] + chunk
    d = THREADS // 2
    while d >= 1:
        s[:d] = s[:d] + s[d:2 * d]
        d //= 2
    return float(s[0])


# ------------------------------------------------------------------------------------------------ 2. total
def total(e_block_by_gid):
    """The sum over the global block ids in rising order, sequentially from +0.0."""
    e = 0.0
    for v in e_block_by_gid:
        e = e + float(v)
    return e


def gather(parts, nblocks_total):
    """What the ranks' integer all-reduce does: ``parts`` = one (gids, block sums) pair per rank, each block with one
    owner; the bit patterns are added as int64 into a zero-filled array."""
    bits = np.zeros(nblocks_total, dtype=np.int64)
    for gids, e in parts:
        mine = np.zeros(nblocks_total, dtype=np.int64)
        mine[np.asarray(gids)] = np.ascontiguousarray(e, dtype=np.float64).view(np.int64)
        bits = bits + mine
    return bits.view(np.float64)


def scale_of(n_target, e_total):
    """(double)N / E_tot, one division; 0 when there is nothing to source.  Raises what the library rejects."""
    if not math.isfinite(e_total) or e_total < 0.0:
        raise ValueError("E_tot is not finite")
    if e_total == 0.0:
        return 0.0
    s = float(n_target) / e_total
    if not math.isfinite(s):
        raise ValueError("N / E_tot is not finite")
    return s


def check_target(n_target, ncell):
    if n_target < 0 or n_target + ncell > INT32_MAX:
        raise ValueError("a block's count could pass 2^31 - 1")


# ------------------------------------------------------------------------------------------------ 3. count pass
def rounding_draws(seed, epoch, gid, ncell):
    """xi of every cell of block ``gid``: the one draw of the cell's rounding stream."""
    from oracle import orc
    out = np.empty(ncell)
    for cell in range(ncell):
        u, _ = orc.draw_stream(orc.seed_state(int(seed), RNG_DOMAIN_CELL, cell_stream_id(epoch, gid, cell)), 1)
        out[cell] = u[0]
    return out


def count_cells(erad, scale, xi):
    """(n, ew) per cell from erad, scale and the draws."""
    erad = np.asarray(erad, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        nu = erad * scale
        f = np.floor(nu)
        n = f + ((nu - f) > xi).astype(np.float64)
        ew = np.where(f >= 1.0, erad / n, np.where(n == 1.0, erad / nu, 0.0))
    return n, ew


def prefix_of(n):
    """(exclusive prefix int32 [ncell], the block's count) in (k, j, i) order."""
    cnt = np.rint(np.asarray(n).reshape(-1)).astype(np.int64)
    incl = np.cumsum(cnt)
    return (incl - cnt).astype(np.int32), int(incl[-1]) if cnt.size else 0


# ------------------------------------------------------------------------------------------------ 4. energy_delta
def energy_delta(n, ew, source_type, set_energy_delta=True):
    if source_type != EMISSION or not set_energy_delta:
        return np.zeros_like(np.asarray(ew, dtype=np.float64))
    return -(np.asarray(n) * np.asarray(ew))


# ------------------------------------------------------------------------------------------------ a whole call
class Call:
    """One source call on a whole mesh: per global block id ``erad``, ``n``, ``ew`` as [nx3, nx2, nx1] arrays,
    ``prefix`` [ncell], ``nper``, ``e_block``; ``e_total``, ``scale``."""


def source_call(mesh, rho, sie, fleck, par, source_type, dt, n_target, epoch, blocks=None):
    """``rho``, ``sie``, ``fleck``: [len(blocks), nk, nj, ni] with ghosts (fleck may be None for the thermal source);
    ``blocks``: the global ids of their rows (default: the whole mesh, which a call needs for E_tot -- a partial list
    gives that rank's block sums only and stops there); ``par``: dict(cv, sb, c, kappa, seed) and, for EPBremss, ep_E."""
    whole = blocks is None
    blocks = list(range(mesh.nblocks)) if whole else [int(b) for b in blocks]
    check_target(n_target, mesh.ncell)
    sl = mesh.interior()[1:]
    out = Call()
    out.blocks, out.erad, out.e_block = blocks, {}, {}
    for row, b in enumerate(blocks):
        dv = (mesh.blk_dx[b, 0] * mesh.blk_dx[b, 1]) * mesh.blk_dx[b, 2]
        if source_type == THERMAL:
            e = erad_thermal(sie[row][sl], par["cv"], par["sb"], par["c"], dv)
        else:
            e = erad_emission(rho[row][sl], sie[row][sl], fleck[row][sl], par["cv"], par["sb"], par["kappa"], dv, dt,
                              par.get("ep_E"))
        out.erad[b] = e
        out.e_block[b] = block_sum(e)
    if not whole:
        return out
    finish_call(out, mesh, [out.e_block[b] for b in range(mesh.nblocks)], par["seed"], n_target, epoch)
    return out


def finish_call(out, mesh, e_block_by_gid, seed, n_target, epoch):
    """Steps 2 and 3 for the blocks ``out`` holds, from the block sums of the WHOLE mesh."""
    out.e_total = total(e_block_by_gid)
    out.scale = scale_of(n_target, out.e_total)
    out.n, out.ew, out.prefix, out.nper = {}, {}, {}, {}
    for b in out.blocks:
        xi = rounding_draws(seed, epoch, b, mesh.ncell).reshape(out.erad[b].shape)
        out.n[b], out.ew[b] = count_cells(out.erad[b], out.scale, xi)
        out.prefix[b], out.nper[b] = prefix_of(out.n[b])
    return out


# ------------------------------------------------------------------------------------------------ 5. photons
def cell_of(prefix, p):
    """The cell the fill's bisection names for the block's photon number p: the last cell with prefix <= p."""
    return int(np.searchsorted(prefix, p, side="right")) - 1


def photons(mesh, call, par, source_type, t_start, dt, next_id, sie, blocks=None):
    """The photons the fill makes for ``call``: block b's take the ids ``next_id`` + (photons of the blocks < b) in
    cell order.  ``sie`` [nblocks, nk, nj, ni] of the whole mesh (the Planck draw's temperature).  ``blocks``: the
    global ids to make photons for (default all); ``blk`` holds global ids.  Draw order of sourcing.cpp:175-198:
    x, y, z; theta, phi; Planck (5); emission: time."""
    from oracle import orc
    orc.set_math_mode(orc.MATH_PORTABLE)
    excl, run = {}, 0
    for b in range(mesh.nblocks):
        excl[b] = run
        run += call.nper[b]
    blocks = list(range(mesh.nblocks)) if blocks is None else [int(b) for b in blocks]
    n = sum(call.nper[b] for b in blocks)
    sw = {k: np.zeros(n) for k in ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e")}
    sw.update({k: np.zeros(n, dtype=np.int32) for k in ("ip", "jp", "kp", "blk", "status")})
    sw["id"], sw["rng"] = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    first = [int(mesh.is_[d]) for d in range(3)]
    nx = [int(v) for v in mesh.nx]
    ndraw = 11 if source_type == EMISSION else 10
    q = 0
    for b in blocks:
        dx = [float(mesh.blk_dx[b, d]) for d in range(3)]
        x0 = [float(mesh.blk_xmin[b, d]) - first[d] * dx[d] for d in range(3)]
        ew = call.ew[b].reshape(-1)
        for p in range(call.nper[b]):
            cell = cell_of(call.prefix[b], p)
            k, r = divmod(cell, nx[0] * nx[1])
            j, i = divmod(r, nx[0])
            idx = [i + first[0], j + first[1], k + first[2]]
            pid = int(next_id) + excl[b] + p
            u, state = orc.draw_stream(orc.stream_start(int(par["seed"]), pid), ndraw)
            pos = [(x0[a] + (idx[a] + 0.5) * dx[a]) + dx[a] * (u[a] - 0.5) for a in range(3)]
            theta = orc.math_acos(np.array([2.0 * u[3] - 1.0]))
            sth, cth = orc.math_sincos(theta)
            sph, cph = orc.math_sincos2pi(np.array([u[4]]))
            c = par["c"]
            vel = [c * sth[0] * cph[0], c * sth[0] * sph[0], c * cth[0]]
            temp = float(temperature(sie[b][idx[2], idx[1], idx[0]], par["cv"]))
            e, used = orc.call_planck(par["sb"], temp, u[5:10])
            assert used == 5
            for name, val in (("x", pos[0]), ("y", pos[1]), ("z", pos[2]), ("vx", vel[0]), ("vy", vel[1]),
                              ("vz", vel[2]), ("t", t_start + u[10] * dt if source_type == EMISSION else 0.0),
                              ("w", ew[cell]), ("e", e)):
                sw[name][q] = val
            sw["ip"][q], sw["jp"][q], sw["kp"][q] = idx
            sw["blk"][q] = b
            sw["status"][q] = ST_ACTIVE
            sw["id"][q] = pid
            sw["rng"][q] = state
            q += 1
    return sw
