"""The boundary source (include/jaybenne_amd.h: jb_source_boundary_count / _fill) restated in numpy: the reference of
tests/test_bsource_host.py (CPU) and tests/test_gpu_bsource.py.  The CPU oracle has no boundary source; this model
builds the photons from the oracle's own primitives -- ``orc.seed_state``, ``orc.stream_start``, ``orc.draw_stream``,
``orc.call_face_iso_dir``, ``orc.call_planck`` in the portable math mode -- writes them into an ``Oracle``'s ``sw``
arrays and advances ``n`` and ``next_id``; the oracle then transports them like any other photon.

Every floating-point expression is written in the order the header states (Python floats: IEEE doubles, no fused
multiply-add), so that the library's photons can be compared bit for bit.
"""
from __future__ import annotations

import ctypes as C
import math
import sys

import numpy as np

import ledger_cases as lc

FACES = ("ix1", "ox1", "ix2", "ox2", "ix3", "ox3")
K_EPS_IMC = 1.0e6 * (10.0 * sys.float_info.epsilon)     # reference transport_utils.hpp:24 (jb_physics.hpp: kEpsImc)
RNG_DOMAIN_BOUNDARY = 3                                 # jb_rng.hpp: kRngDomainBoundary (+ f)
BC_PERIODIC = 0
ST_ACTIVE = 0


def cell_stream_id(epoch, gblock, cell):
    return (int(epoch) << 44) | (int(gblock) << 24) | int(cell)


def on_boundary(mesh, b, f):
    d = f >> 1
    half = 0.5 * mesh.blk_dx[b, d]
    return bool(mesh.blk_xmax[b, d] > mesh.gmax[d] - half) if f & 1 else bool(mesh.blk_xmin[b, d] < mesh.gmin[d] + half)


def check_faces(mesh, temps):
    """The conditions jb_source_boundary_count answers with JB_ERR_INVALID."""
    for f, t in enumerate(temps):
        if not (t >= 0.0 and math.isfinite(t)):
            raise ValueError(f"face {f}: temperature {t}")
        if t > 0.0 and f >= 2 * mesh.ndim:
            raise ValueError(f"face {f}: inactive axis")
        if t > 0.0 and mesh.swarm_bc[f] == BC_PERIODIC:
            raise ValueError(f"face {f}: periodic")


def source_faces(mesh, temps, blocks=None):
    """[(block, face)] that source, blocks ascending, faces ascending."""
    blocks = range(mesh.nblocks) if blocks is None else blocks
    return [(b, f) for b in blocks for f in range(2 * mesh.ndim) if temps[f] > 0.0 and on_boundary(mesh, b, f)]


def face_cells_total(mesh, temps):
    return sum(mesh.ncell // int(mesh.nx[f >> 1]) for _, f in source_faces(mesh, temps))


def face_cells(mesh, f):
    """The zero-based interior (k, j, i) of the cells of face f of a block, in (k, j, i) order."""
    nx = [int(v) for v in mesh.nx] + [1] * (3 - len(mesh.nx))
    d = f >> 1
    rng = [range(nx[0]), range(nx[1]), range(nx[2])]
    rng[d] = [nx[d] - 1] if f & 1 else [0]
    return [(k, j, i) for k in rng[2] for j in rng[1] for i in rng[0]]


def cell_energy(mesh, sb, b, f, temp, dt):
    """E_c = ((sb T^4) A) dt, A the product of the two transverse widths of the block."""
    d = f >> 1
    area = float(mesh.blk_dx[b, (d + 1) % 3]) * float(mesh.blk_dx[b, (d + 2) % 3])
    t2 = temp * temp
    return ((sb * (t2 * t2)) * area) * dt


def count(mesh, sb, seed, temps, num_particles, dt, epoch, blocks=None):
    """Per block (dict b -> list) the source face cells in creation order -- face, then cell in (k, j, i) order --
    as (f, (k, j, i), snpc, weight); and e_face / n_face.  ``blocks``: the blocks of one rank (default: all)."""
    from oracle import orc
    check_faces(mesh, temps)
    total = face_cells_total(mesh, temps)
    if total < 1:
        raise ValueError("no source face cells")
    npc = float(num_particles) / float(total)
    if not npc >= 1.0:
        raise ValueError("npc < 1")
    nx = [int(v) for v in mesh.nx] + [1] * (3 - len(mesh.nx))
    out = {}
    e_face, n_face = [[] for _ in range(6)], [0] * 6
    for b, f in source_faces(mesh, temps, blocks):
        e_cell = cell_energy(mesh, sb, b, f, temps[f], dt)
        for (k, j, i) in face_cells(mesh, f):
            cell = (k * nx[1] + j) * nx[0] + i
            xi, _ = orc.draw_stream(orc.seed_state(seed, RNG_DOMAIN_BOUNDARY + f, cell_stream_id(epoch, b, cell)), 1)
            snpc = math.floor(npc)
            snpc += float((npc - snpc) > xi[0])
            out.setdefault(b, []).append((f, (k, j, i), int(snpc), e_cell / snpc))
            e_face[f].append(e_cell)
            n_face[f] += int(snpc)
    return out, dict(e_face=[math.fsum(v) for v in e_face], n_face=n_face)


def closed_form_energy(mesh, sb, temps, dt):
    """sb T^4 (area of the face) dt per face, from the domain's extents."""
    ext = [float(mesh.gmax[d] - mesh.gmin[d]) for d in range(3)]
    return [sb * temps[f] ** 4 * ext[((f >> 1) + 1) % 3] * ext[((f >> 1) + 2) % 3] * dt for f in range(6)]


def photons(mesh, sb, c, seed, temps, cells_b, b, id_base, t_start, dt, blk_index=None):
    """The photons of block b (``cells_b``: its list from ``count``), ids from ``id_base``: a dict of arrays."""
    from oracle import orc
    orc.set_math_mode(orc.MATH_PORTABLE)
    n = sum(s for _, _, s, _ in cells_b)
    sw = {k: np.zeros(n) for k in orc.SWARM_F64}
    sw.update({k: np.zeros(n, dtype=np.int32) for k in orc.SWARM_I32})
    sw["id"], sw["rng"] = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    first = [int(mesh.is_[d]) for d in range(3)]
    dx = [float(mesh.blk_dx[b, d]) for d in range(3)]
    x0 = [float(mesh.blk_xmin[b, d]) - first[d] * dx[d] for d in range(3)]
    q = 0
    for f, (k, j, i), snpc, weight in cells_b:
        d = f >> 1
        a1, a2 = (d + 1) % 3, (d + 2) % 3
        idx = [i + first[0], j + first[1], k + first[2]]
        xc = [x0[a] + (idx[a] + 0.5) * dx[a] for a in range(3)]
        for _ in range(snpc):
            pid = int(id_base) + q
            u, state = orc.draw_stream(orc.stream_start(seed, pid), 10)
            pos, vel = [0.0] * 3, [0.0] * 3
            pos[a1] = xc[a1] + dx[a1] * (u[0] - 0.5)
            pos[a2] = xc[a2] + dx[a2] * (u[1] - 0.5)
            if f & 1:
                pos[d] = (xc[d] + 0.5 * dx[d]) - K_EPS_IMC * dx[d]
            else:
                pos[d] = (xc[d] - 0.5 * dx[d]) + K_EPS_IMC * dx[d]
            v, used = orc.call_face_iso_dir(-c if f & 1 else c, u[2:4])
            assert used == 2
            vel[d], vel[a1], vel[a2] = v[0], v[1], v[2]
            e, used = orc.call_planck(sb, temps[f], u[4:9])
            assert used == 5
            for name, val in (("x", pos[0]), ("y", pos[1]), ("z", pos[2]), ("vx", vel[0]), ("vy", vel[1]),
                              ("vz", vel[2]), ("t", t_start + u[9] * dt), ("w", weight), ("e", e)):
                sw[name][q] = val
            sw["ip"][q], sw["jp"][q], sw["kp"][q] = idx
            sw["blk"][q] = b if blk_index is None else blk_index
            sw["status"][q] = ST_ACTIVE
            sw["id"][q] = pid
            sw["rng"][q] = state
            q += 1
    return sw


def append(O, sw):
    n = len(sw["id"])
    if O.n + n > O.cap:
        raise MemoryError("oracle swarm capacity exceeded")
    for k, v in sw.items():
        O.sw[k][O.n:O.n + n] = v
    O.n += n


def source(O, temps, num_particles, t_start, dt, epoch=None, id_base=None):
    """SourceBoundaryPhotons on an oracle that holds the whole mesh, with no emission source in front: block b's
    photons take consecutive ids in block order from ``O.next_id`` (or ``id_base[b]``).  Returns the record."""
    mesh, P = O.mesh, O.P
    epoch = O.cycle if epoch is None else epoch
    cells, rec = count(mesh, P.sb, P.seed, temps, num_particles, dt, epoch)
    run = 0
    for b in sorted(cells):
        nb = sum(s for _, _, s, _ in cells[b])
        base = O.next_id + run if id_base is None else id_base[b]
        append(O, photons(mesh, P.sb, P.c, P.seed, temps, cells[b], b, base, t_start, dt))
        run += nb
    if id_base is None:
        O.next_id += run
    return rec


def source_cycle(O, temps, num_particles, t_start, dt, blocks_in_call=None):
    """The two sources of one cycle on the oracle (``O.cycle`` already advanced, the derived fields updated):
    block b takes n_em[b] + n_bs[b] consecutive ids, the emission photons first; the boundary photons lie behind all
    emission photons in the swarm.  Returns the boundary source's record (None with every face off)."""
    from oracle import orc
    m = O.mesh
    O._enter()
    nper = np.zeros(m.nblocks, dtype=np.int32)
    prefix = np.zeros(m.nblocks * m.ncell, dtype=np.int32)
    if O.P.do_emission:
        M = O._mesh_c()
        orc.lib().orc_source_count(C.byref(M), C.byref(O.P), orc.SRC_EMISSION, dt,
                                   m.nblocks if blocks_in_call is None else blocks_in_call, O.cycle,
                                   nper.ctypes.data_as(orc._ip), prefix.ctypes.data_as(orc._ip))
    on = any(t > 0.0 for t in temps)
    cells, rec = count(m, O.P.sb, O.P.seed, temps, num_particles, dt, O.cycle) if on else ({}, None)
    n_bs = np.array([sum(s for _, _, s, _ in cells.get(b, [])) for b in range(m.nblocks)], dtype=np.int64)
    both = nper.astype(np.int64) + n_bs
    id_base = O.next_id + np.concatenate(([0], np.cumsum(both)[:-1]))
    tot = int(nper.sum())
    if O.n + tot + int(n_bs.sum()) > O.cap:
        raise MemoryError("oracle swarm capacity exceeded")
    if tot:
        excl = np.concatenate(([0], np.cumsum(nper)[:-1])).astype(np.int64)
        slot_base = np.ascontiguousarray(O.n + excl, dtype=np.int64)
        ids = np.ascontiguousarray(id_base, dtype=np.uint64)
        M, S = O._mesh_c(), O._swarm_c()
        orc.lib().orc_source_fill(C.byref(M), C.byref(O.P), C.byref(S), orc.SRC_EMISSION, t_start, dt,
                                  prefix.ctypes.data_as(orc._ip), slot_base.ctypes.data_as(C.POINTER(C.c_int64)),
                                  ids.ctypes.data_as(C.POINTER(C.c_uint64)))
        O.n += tot
    for b in sorted(cells):
        append(O, photons(m, O.P.sb, O.P.c, O.P.seed, temps, cells[b], b, int(id_base[b]) + int(nper[b]), t_start, dt))
    O.next_id += int(both.sum())
    return rec


def oracle_cycle(O, pin, t, temps, num_particles):
    """tests/ledger_cases.py: oracle_cycle with the boundary source behind the emission source.  The ledger's terms
    as a dict, plus ``e_sourced_face`` / ``n_sourced_face`` and, under ``swarm_after_transport``, a copy of the
    swarm between TransportPhotons and RemoveMarkedParticles."""
    dt = pin.GetReal("jaybenne", "dt")
    mesh = O.mesh
    e_start, _ = lc.census_energy(O)
    O.cycle += 1
    O.UpdateDerivedTransportFields(dt)
    n0 = O.n
    rec = source_cycle(O, temps, num_particles, t, dt, getattr(O, "emission_blocks_in_call", None))
    led = {"cycle": O.cycle, "t_start": t, "dt": dt, "e_start": e_start,
           "e_sourced": math.fsum(O.sw["w"][n0:O.n]), "n_sourced": O.n - n0,
           "e_sourced_face": rec["e_face"] if rec else [0.0] * 6, "n_sourced_face": rec["n_face"] if rec else [0] * 6}
    O.TransportPhotons(t, dt)
    n = O.n
    st, w = O.sw["status"][:n], O.sw["w"][:n]
    esc = st == lc.ST_ESCAPED
    face, outside = lc.classify(mesh, O.sw["x"][:n][esc], O.sw["y"][:n][esc], O.sw["z"][:n][esc])
    led["e_escaped"] = [math.fsum(w[esc][face == f]) for f in range(6)]
    led["n_escaped"] = [int((face == f).sum()) for f in range(6)]
    led["e_escaped_unclassified"] = math.fsum(w[esc][face == 6])
    led["n_escaped_unclassified"] = int((face == 6).sum())
    led["e_absorbed"] = math.fsum(w[st == lc.ST_ABSORBED])
    led["n_absorbed"] = int((st == lc.ST_ABSORBED).sum())
    led["swarm_after_transport"] = {k: v[:n].copy() for k, v in O.sw.items()}
    led["n_before_source"] = n0
    O.RemoveMarkedParticles()
    assert O.CheckCompletion(t + dt) == 0
    O.EvaluateRadiationEnergy()
    O.UpdateFluid()
    led["e_census"], led["n_census"] = lc.census_energy(O)
    vol = np.array([mesh.cell_volume(b) for b in range(mesh.nblocks)])[:, None, None, None]
    sl = mesh.interior()
    led["e_tally"] = math.fsum((O.fields["tally"] * vol)[sl].ravel())
    led["e_delta"] = math.fsum(O.fields["edelta"][sl].ravel())
    led["e_material"] = math.fsum((O.fields["u"] * vol)[sl].ravel())
    lhs = math.fsum([led["e_start"], led["e_sourced"]])
    led["residual"] = lc.residual(led) if lhs > 0.0 else 0.0
    if pin.GetOrAddBoolean("jaybenne", "do_feedback", True):
        mesh.fill_ghosts(O.fields["u"])
    O.fields["sie"][...] = O.fields["u"] / O.fields["rho"]
    return led
