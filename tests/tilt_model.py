"""The source tilt (include/jaybenne_amd.h: jb_set_source_tilt) restated in numpy, operation for operation: the
reference of tests/test_tilt_host.py (CPU) and tests/test_gpu_tilt.py.  numpy rounds every operation on its own and
fuses nothing; sqrt and / are correctly rounded, as the library's are.
"""
from __future__ import annotations

import numpy as np

BC_PERIODIC = 0
U_MAX = 1.0 - 2.0 ** -52


# ------------------------------------------------------------------------------------------------ slopes
def e4(sie, cv):
    """E = (T T) (T T), T = eos_temperature(rho, sie) of the ideal gas: sie / cv where that is positive, else 0."""
    with np.errstate(invalid="ignore"):
        t = sie / cv
        t = np.where(t > 0.0, t, 0.0)
    t2 = t * t
    return t2 * t2


def on_boundary(mesh, b, f):
    d = f >> 1
    half = 0.5 * mesh.blk_dx[b, d]
    return bool(mesh.blk_xmax[b, d] > mesh.gmax[d] - half) if f & 1 else bool(mesh.blk_xmin[b, d] < mesh.gmin[d] + half)


def slope(e_c, e_m, e_p):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s_raw = (e_p - e_m) / (4.0 * e_c)
        s = np.minimum(np.maximum(s_raw, -1.0), 1.0)
    return np.where((e_c == 0.0) | ~np.isfinite(s_raw), 0.0, s)


def slopes(mesh, sie, cv, blocks=None):
    """[len(blocks), 3, nx3, nx2, nx1]: the slope of every interior cell along every axis (zeros on inactive axes).
    ``sie``: [len(blocks), nk, nj, ni] with the ghost layers the library reads; ``blocks``: the global ids of its rows
    (default: the whole mesh).  The ghost cells behind a non-periodic domain face are not looked at."""
    blocks = range(mesh.nblocks) if blocks is None else blocks
    nx, first = mesh.nx, mesh.is_
    out = np.zeros((len(blocks), 3, nx[2], nx[1], nx[0]))
    for n, b in enumerate(blocks):
        E = e4(sie[n], cv)

        def moved(d, by):
            s = [slice(first[a] + (by if a == d else 0), first[a] + nx[a] + (by if a == d else 0)) for a in range(3)]
            return E[s[2], s[1], s[0]]

        e_c = moved(0, 0)
        for d in range(mesh.ndim):
            e_m, e_p = moved(d, -1).copy(), moved(d, 1).copy()
            layer = [slice(None)] * 3
            if mesh.swarm_bc[2 * d] != BC_PERIODIC and on_boundary(mesh, int(b), 2 * d):
                layer[2 - d] = 0
                e_m[tuple(layer)] = e_c[tuple(layer)]
            if mesh.swarm_bc[2 * d + 1] != BC_PERIODIC and on_boundary(mesh, int(b), 2 * d + 1):
                layer[2 - d] = nx[d] - 1
                e_p[tuple(layer)] = e_c[tuple(layer)]
            out[n, d] = slope(e_c, e_m, e_p)
    return out


def nan_behind_walls(mesh, field, blocks=None):
    """A copy of ``field`` ([len(blocks), nk, nj, ni]) with NaN in every ghost layer that lies behind a non-periodic
    domain face: the cells whose content nobody defines."""
    blocks = range(mesh.nblocks) if blocks is None else blocks
    out = field.copy()
    for n, b in enumerate(blocks):
        for d in range(mesh.ndim):
            idx = [slice(None)] * 3
            if mesh.swarm_bc[2 * d] != BC_PERIODIC and on_boundary(mesh, int(b), 2 * d):
                idx[2 - d] = slice(0, mesh.is_[d])
                out[n][tuple(idx)] = np.nan
            if mesh.swarm_bc[2 * d + 1] != BC_PERIODIC and on_boundary(mesh, int(b), 2 * d + 1):
                idx[2 - d] = slice(mesh.is_[d] + mesh.nx[d], None)
                out[n][tuple(idx)] = np.nan
    return out


# ------------------------------------------------------------------------------------------------ sampling
def sample_u(s, xi):
    """u in [-1, 1 - 2^-52] with density (1 + s u) / 2 from the uniform draw xi."""
    s, xi = np.asarray(s, dtype=np.float64), np.asarray(xi, dtype=np.float64)
    a = 1.0 - s
    arg = a * a + (4.0 * s) * xi
    root = np.sqrt(np.where(arg > 0.0, arg, 0.0))
    u = ((4.0 * xi - 2.0) + s) / (1.0 + root)
    return np.maximum(np.minimum(u, U_MAX), -1.0)


def position(s, xi, xc, dx):
    return xc + (0.5 * dx) * sample_u(s, xi)


def position_untilted(xi, xc, dx):
    return xc + dx * (np.asarray(xi) - 0.5)        # sourcing.cpp:175-177


def cdf(u, s):
    return (u + 1.0) / 2.0 + s * (u * u - 1.0) / 4.0


# ------------------------------------------------------------------------------------------------ photons
def draws(seed, ids, n=3):
    """[len(ids), n]: the first n uniforms of the streams of the photons ``ids`` (the position draws x, y, z)."""
    from oracle import orc
    out = np.empty((len(ids), n))
    for q, pid in enumerate(ids):
        out[q], _ = orc.draw_stream(orc.stream_start(int(seed), int(pid)), n)
    return out


def photon_positions(mesh, seed, s_all, ids, gblk, row, kp, jp, ip):
    """(x, y, z) of the photons ``ids`` in the cells (gblk; kp, jp, ip) -- global block ids and block-local indices
    with ghosts, as the swarm carries them; ``row``: each photon's row of ``s_all`` (= ``slopes(...)``)."""
    xi = draws(seed, ids)
    idx = (np.asarray(ip), np.asarray(jp), np.asarray(kp))
    pos = []
    for d in range(3):
        dx = mesh.blk_dx[gblk, d]
        x0 = mesh.blk_xmin[gblk, d] - mesh.is_[d] * dx
        xc = x0 + (idx[d] + 0.5) * dx
        s = s_all[row, d, idx[2] - mesh.is_[2], idx[1] - mesh.is_[1], idx[0] - mesh.is_[0]]
        pos.append(position(s, xi[:, d], xc, dx))
    return pos
