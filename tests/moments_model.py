"""Radiation moments (include/jaybenne_amd.h: jb_evaluate_radiation_moments) restated in numpy: the twelve per-cell
fields of a swarm that lies in (block, cell) order on a swarm_ops_model.Geom, with the sort key of
swarm_ops_model.sort_key and every sum formed in the order the kernel header writes down -- and the crafted swarms
the kernels are held to.  No library code computes anything here.  All comparisons are of bits.

Order of summation (jaybenne_amd/csrc/jb_kernel_moments.hpp): a cell's photons are a run a_0 .. a_(L-1) of consecutive
slots.  The run is cut into chunks of CHUNK = 4096 slots from its head; in a chunk lane l (0 .. 63) starts from +0.0
and adds elements l, l + 64, l + 128, .. in rising order; the 64 lane sums are joined by
``for d in 32, 16, 8, 4, 2, 1: s[l] = s[l] + s[l + d] for l < d``; the run's sum is the first chunk's sum, then the
further chunks' sums added in chunk order."""
from fractions import Fraction

import numpy as np

import swarm_ops_model as som

MOMENTS, CHUNK, LANES = 12, 4096, 64
NAMES = ("n", "e", "w2", "fx", "fy", "fz", "qxx", "qxy", "qxz", "qyy", "qyz", "qzz")
SUMS = MOMENTS - 1                       # the rounded sums: components 1 .. 11
DIVIDED = tuple(q != 1 for q in range(SUMS))      # W2 (sum 1) is stored as the sum itself, the others over dv
MAX_SLOTS = 100000


# ---- the sums -----------------------------------------------------------------------------------------
def addends(sw, idx):
    """[len(idx), 11]: what each photon adds to the eleven sums; every product rounded on its own"""
    w, vx, vy, vz = (np.asarray(sw[k])[idx] for k in ("w", "vx", "vy", "vz"))
    px, py, pz = w * vx, w * vy, w * vz
    return np.stack([w, w * w, px, py, pz, px * vx, px * vy, px * vz, py * vy, py * vz, pz * vz], axis=1)


def chunk_sum(a):
    """the sum of one chunk: a is [m, 11], m <= CHUNK"""
    m = len(a)
    assert 0 < m <= CHUNK
    rows = -(-m // LANES)
    pad = np.zeros((rows * LANES, a.shape[1]))
    pad[:m] = a
    pad = pad.reshape(rows, LANES, -1)
    has = (np.arange(rows * LANES) < m).reshape(rows, LANES, 1)
    s = np.zeros((LANES, a.shape[1]))                      # +0.0
    for r in range(rows):
        s = np.where(has[r], s + pad[r], s)                # a lane without an element adds nothing
    d = LANES // 2
    while d:
        s[:d] = s[:d] + s[d:2 * d]
        d //= 2
    return s[0].copy()


def run_sum(a):
    """the sum of one run: the chunks' sums in chunk order"""
    total = chunk_sum(a[:CHUNK])
    for c0 in range(CHUNK, len(a), CHUNK):
        total = total + chunk_sum(a[c0:c0 + CHUNK])
    return total


def exact_sum(a):
    """(the exact rational sum of every column of a, the sum of the absolute values)"""
    cols = [[Fraction(float(v)) for v in a[:, q]] for q in range(a.shape[1])]
    return [sum(c, Fraction(0)) for c in cols], [sum((abs(v) for v in c), Fraction(0)) for c in cols]


# ---- the fields ---------------------------------------------------------------------------------------
def cell_of_key(geom, key):
    """(local block, (k, j, i) in the block's array, interior?) of sort keys below nkeys"""
    key = np.asarray(key, dtype=np.int64)
    b, q = key // geom.ntot, key % geom.ntot
    i, j, k = q % geom.dims[0], (q // geom.dims[0]) % geom.dims[1], q // (geom.dims[0] * geom.dims[1])
    inside = np.ones(key.shape, dtype=bool)
    for v, d in ((i, 0), (j, 1), (k, 2)):
        inside &= (v >= geom.first[d]) & (v < geom.first[d] + geom.nx[d])
    return b, (k, j, i), inside


def in_order(geom, sw, n):
    return bool(np.all(np.diff(som.sort_key(geom, sw, n)) >= 0))


def moments(geom, sw, n):
    """(fields [12, nblocks, nx3, nx2, nx1], report) of the first n slots of a swarm that is in key order: per
    interior cell of an owned block N, E, W2, F, Q over the ACTIVE photons whose sort key is the cell; zeros in
    empty cells and in halo copies (the blocks behind the first geom.nowned)."""
    out = np.zeros((MOMENTS, geom.nblocks, geom.nx[2], geom.nx[1], geom.nx[0]))
    key = som.sort_key(geom, sw, n)
    assert np.all(np.diff(key) >= 0), "the model takes the swarm in (block, cell) order"
    start = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1]))) if n else np.zeros(0, dtype=np.int64)
    end = np.concatenate((start[1:], [n]))
    rep = dict(n_counted=0, n_skipped=0, cells_nonempty=0, longest_run=0)
    for s, e in zip(start.tolist(), end.tolist()):
        if key[s] >= geom.nkeys:
            continue
        b, (k, j, i), inside = cell_of_key(geom, key[s])
        if not inside or b >= geom.nowned:
            continue
        dv = (geom.dx[b, 0] * geom.dx[b, 1]) * geom.dx[b, 2]
        total = run_sum(addends(sw, np.arange(s, e)))
        at = (int(b), int(k - geom.first[2]), int(j - geom.first[1]), int(i - geom.first[0]))
        out[(0,) + at] = float(e - s)
        for q in range(SUMS):
            out[(q + 1,) + at] = total[q] / dv if DIVIDED[q] else total[q]
        rep["n_counted"] += e - s
        rep["cells_nonempty"] += 1
        rep["longest_run"] = max(rep["longest_run"], e - s)
    rep["n_skipped"] = n - rep["n_counted"]
    return out, rep


def canonical(geom, sw, n):
    """the first n slots in the canonical order of JB_CELL_ORDER_BY_ID: by (sort key, id, input slot)"""
    return som.take(sw, np.lexsort((np.arange(n), sw["id"][:n], som.sort_key(geom, sw, n))))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def differing_components(a, b):
    return [NAMES[q] for q in range(MOMENTS) if not same_bits(a[q], b[q])]


def integrals(fields, dx):
    """The domain integrals a command-line host prints: n, e, w2, f[3], q[6] -- each component summed sequentially in
    (block, cell) order, E F Q times the block's dv first."""
    nb = fields.shape[1]
    dv = [(dx[b][0] * dx[b][1]) * dx[b][2] for b in range(nb)]
    out = []
    for q in range(MOMENTS):
        s = 0.0
        for b in range(nb):
            for v in fields[q, b].reshape(-1).tolist():
                s += v * dv[b] if q not in (0, 2) else v
        out.append(s)
    return out


# ---- the crafted swarms ---------------------------------------------------------------------------------
def mesh_cases():
    """{name: (deck, overrides)}: 1-D (4 blocks of 512), the 2-D and the 3-D SMR mesh of tests/axis_cases.py (two
    levels: block widths differ; cells per block 16 x 4 and 16 x 4 x 2: no two axes alike), and the view with halo
    copies comes from swarm_ops_model.RANK_MESH on two ranks"""
    import axis_cases as ax
    out = {"1d": ("stepdiff", {"parthenon/mesh/nx1": 2048, "parthenon/meshblock/nx1": 512, "jaybenne/num_particles": 64})}
    for name, geom in (("2d", "G2S"), ("3d", "G3S")):
        kinds = next(iter(ax.boundary_sets(geom).values()))
        out[name] = ("stepdiff_smr", dict(ax.geometry_overrides(geom, kinds), **{"jaybenne/num_particles": 64}))
    return out


SHORT = (1, 2, 63, 64, 65)                 # 195 slots, 3 mod 64: 64 rounds start every length at every lane offset
LONG = (4095, 4096, 4097, 2 * CHUNK + 1)
ONE_CELL = 3 * CHUNK + 5
EXTRAS = 97                                # slots per swarm that are not counted: other statuses, ACTIVE with a bad blk
SALT = 907


def run_plans():
    """[(name, mesh, [run lengths])]: every length of SHORT and LONG starting at every lane offset 0 .. 63, in swarms
    of at most MAX_SLOTS slots.  A swarm that does not start its pattern at offset 0 opens with a filler run (a cell
    of its own) that restores the offset.  4096 alone would keep its offset: a run of one slot goes before each."""
    plans = [("short", "1d", list(SHORT) * LANES), ("short", "3d", list(SHORT) * LANES)]
    meshes = ("2d", "3d", "1d")
    for q, L in enumerate(LONG):
        unit = [1, L] if L % LANES == 0 else [L]
        seq, piece, offset, part = unit * LANES, [], 0, 0
        room = MAX_SLOTS - EXTRAS
        for m in seq:
            if sum(piece) + m > room:
                plans.append((f"{L}.{part}", meshes[(q + part) % 3], piece))
                part += 1
                piece = [offset % LANES] if offset % LANES else []
            piece.append(m)
            offset += m
        plans.append((f"{L}.{part}", meshes[(q + part) % 3], piece))
    plans.append(("one cell", "2d", [ONE_CELL]))
    return plans


def _physical(sw, salt):
    """w positive over 60 binary orders; v components of either sign with hashed magnitudes"""
    ids = sw["id"]
    sw["w"] = np.ldexp(1.0 + som._unit(ids, salt + 1), (som._mod(ids, salt + 2, 61) - 30).astype(np.int32))
    for q, name in enumerate(("vx", "vy", "vz")):
        mag = np.ldexp(0.5 + som._unit(ids, salt + 10 + q), (som._mod(ids, salt + 20 + q, 9) - 4).astype(np.int32))
        sw[name] = np.where(som._mod(ids, salt + 30 + q, 2) == 0, mag, -mag)
    return sw


def shuffle(sw, salt):
    """the slots in a hashed order"""
    n = len(sw["id"])
    return som.take(sw, np.argsort(som._hash(np.arange(n), salt + 77), kind="stable"))


def run_swarm(geom, lengths, salt=SALT, extras=EXTRAS, first_cell=None):
    """A swarm whose ACTIVE photons of resident blocks form runs of the given lengths, one interior cell each, in
    rising cell order with empty cells between them (``first_cell``: the one cell of a single run), plus ``extras``
    slots that must not be counted -- the four other statuses and ACTIVE slots with a blk outside [0, nblocks) --,
    all in a hashed slot order.  Returns (swarm, the runs' cells as block * ncell + interior cell)."""
    nruns = len(lengths)
    cells_total = geom.nowned * geom.ncell
    stride = cells_total // max(nruns, 1)
    assert stride >= 2 or nruns == 1, (cells_total, nruns)
    cells = np.arange(nruns) * stride + (stride - 1 if first_cell is None else first_cell)
    keys = np.concatenate((np.repeat(cells, lengths), np.zeros(extras, dtype=np.int64)))
    n = len(keys)
    assert n <= MAX_SLOTS
    kinds = np.array([som.ST_ABSORBED, som.ST_ESCAPED, som.ST_OUTGOING, som.ST_OUTGOING_ABSORBED, som.ST_ACTIVE])
    status = np.concatenate((np.full(n - extras, som.ST_ACTIVE), kinds[np.arange(extras) % 5])).astype(np.int32)
    sw = som.crafted(geom, n, salt, status=status, keys=keys, edges=False, bad_blk=False)
    bad = np.flatnonzero(status[n - extras:] == som.ST_ACTIVE) + (n - extras)
    sw["blk"][bad] = np.array([-1, geom.nblocks, som.INT_MAX], dtype=np.int32)[np.arange(len(bad)) % 3]
    return shuffle(_physical(sw, salt), salt), cells


def hashed_swarm(geom, n, salt=SALT):
    """hashed cells over all resident blocks (halo copies too), positions outside the block in a share of the slots
    (clamped into ghost cells: not counted), hashed statuses and bad blks: swarm_ops_model.crafted as it comes"""
    return shuffle(_physical(som.crafted(geom, n, salt), salt), salt)
