"""The radiation spectrum (include/jaybenne_amd.h: jb_evaluate_radiation_spectrum) restated in numpy: per interior cell
the energy density of the census in ngroups + 2 frequency bins, on a swarm that lies in (block, cell) order on a
swarm_ops_model.Geom -- the sort key, the runs and the order of summation are moments_model's, applied to every bin on
its own -- and the crafted photon energies the kernels are held to.  No library code computes anything here.  All
comparisons are of bits.

The bin of a photon is the number of edges j with edges[j] <= e: ``(edges[None, :] <= e[:, None]).sum(1)``.  A photon's
addend to its own bin is w; for every other bin it is skipped, which equals adding +0.0 bit for bit (a lane sum that
starts from +0.0 is never -0.0): ``run_sums`` adds +0.0 through moments_model.run_sum, ``run_sums_skipping`` skips."""
import numpy as np

import moments_model as mm
import swarm_ops_model as som

MAX_GROUPS = 64
NGROUPS = (1, 2, 7, 33, 64)
WIDEST = np.array([4.9e-324, np.finfo(np.float64).max])       # ngroups = 1: bin 1 takes every positive finite e
SALT = 1301


# ---- the bins -----------------------------------------------------------------------------------------
def check_edges(edges):
    """what the library accepts: 2 .. 65 finite, strictly increasing doubles"""
    edges = np.asarray(edges, dtype=np.float64)
    return bool(edges.ndim == 1 and 2 <= edges.size <= MAX_GROUPS + 1 and np.all(np.isfinite(edges))
                and np.all(edges[1:] > edges[:-1]))


def bins(edges, e):
    edges, e = np.asarray(edges, dtype=np.float64), np.asarray(e, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (edges[None, :] <= e[:, None]).sum(1)


# ---- the sums -----------------------------------------------------------------------------------------
def addends(w, b, nb):
    """[L, nb]: w in the photon's own bin, +0.0 elsewhere"""
    return np.where(b[:, None] == np.arange(nb)[None, :], np.asarray(w)[:, None], 0.0)


def run_sums(w, b, nb):
    """the nb sums of one run, every other bin's photons added as +0.0: moments_model's order, bin by bin"""
    return mm.run_sum(addends(w, b, nb))


def chunk_sum_skipping(w, b, nb):
    """the sums of one chunk with the photons of other bins skipped: lane l walks elements l, l + 64, .. and adds
    only those of the bin"""
    m = len(w)
    assert 0 < m <= mm.CHUNK
    s = np.zeros((mm.LANES, nb))                             # +0.0
    for p in range(m):
        s[p % mm.LANES, b[p]] = s[p % mm.LANES, b[p]] + w[p]
    d = mm.LANES // 2
    while d:
        s[:d] = s[:d] + s[d:2 * d]
        d //= 2
    return s[0].copy()


def run_sums_skipping(w, b, nb):
    total = chunk_sum_skipping(w[:mm.CHUNK], b[:mm.CHUNK], nb)
    for c0 in range(mm.CHUNK, len(w), mm.CHUNK):
        total = total + chunk_sum_skipping(w[c0:c0 + mm.CHUNK], b[c0:c0 + mm.CHUNK], nb)
    return total


# ---- the fields ---------------------------------------------------------------------------------------
def spectrum(geom, sw, n, edges):
    """(out [ngroups + 2, nblocks, nx3, nx2, nx1], report) of the first n slots of a swarm that is in key order:
    per interior cell of an owned block (sum of w over the ACTIVE photons whose sort key is the cell and whose bin
    it is) / dv; zeros in empty cells and in halo copies.  The photons that count are moments_model.moments'."""
    assert check_edges(edges)
    nb = len(edges) + 1
    out = np.zeros((nb, geom.nblocks, geom.nx[2], geom.nx[1], geom.nx[0]))
    key = som.sort_key(geom, sw, n)
    assert np.all(np.diff(key) >= 0), "the model takes the swarm in (block, cell) order"
    start = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1]))) if n else np.zeros(0, dtype=np.int64)
    end = np.concatenate((start[1:], [n]))
    b_all = bins(edges, sw["e"][:n])
    rep = dict(n_counted=0, n_skipped=0, cells_nonempty=0, longest_run=0, n_below=0, n_above=0)
    for s, e in zip(start.tolist(), end.tolist()):
        if key[s] >= geom.nkeys:
            continue
        b, (k, j, i), inside = mm.cell_of_key(geom, key[s])
        if not inside or b >= geom.nowned:
            continue
        dv = (geom.dx[b, 0] * geom.dx[b, 1]) * geom.dx[b, 2]
        total = run_sums(sw["w"][s:e], b_all[s:e], nb)
        out[:, int(b), int(k - geom.first[2]), int(j - geom.first[1]), int(i - geom.first[0])] = total / dv
        rep["n_counted"] += e - s
        rep["cells_nonempty"] += 1
        rep["longest_run"] = max(rep["longest_run"], e - s)
        rep["n_below"] += int((b_all[s:e] == 0).sum())
        rep["n_above"] += int((b_all[s:e] == nb - 1).sum())
    rep["n_skipped"] = n - rep["n_counted"]
    return out, rep


def differing_bins(a, b):
    return [q for q in range(max(len(a), len(b))) if q >= len(a) or q >= len(b) or not mm.same_bits(a[q], b[q])]


def integrals(out, dx):
    """The domain integrals a command-line host prints: per bin the sum over cells of out dv, sequentially in
    (block, cell) order"""
    nblocks = out.shape[1]
    dv = [(dx[b][0] * dx[b][1]) * dx[b][2] for b in range(nblocks)]
    res = []
    for q in range(out.shape[0]):
        s = 0.0
        for b in range(nblocks):
            for v in out[q, b].reshape(-1).tolist():
                s += v * dv[b]
        res.append(s)
    return res


# ---- the crafted energies -------------------------------------------------------------------------------
def edges_for(ngroups, salt=SALT):
    """ngroups + 1 edges that are data, not a formula a kernel could invert: edge j is (1 + a hashed fraction) 2^(j -
    ngroups / 2) -- strictly increasing, no two widths alike"""
    j = np.arange(ngroups + 1)
    return np.ldexp(1.0 + som._unit(j, salt + ngroups), (j - ngroups // 2).astype(np.int32))


SPECIALS = np.array([0x0000000000000000, 0x8000000000000000,          # +0.0, -0.0
                     0x0000000000000003, 0x800000000000002A,          # denormals of either sign
                     0xBFF8000000000000,                              # -1.5
                     0x7FF0000000000000, 0xFFF0000000000000,          # +inf, -inf
                     0x7FF8000000C0FFEE, 0xFFF400000000BEEF],         # NaN with a payload: quiet, signalling
                    dtype=np.uint64).view(np.float64)
KINDS = 16          # by id: 0 on an edge, 1 one ulp below it, 2 one ulp above it, 3 a special value, 4 .. 15 in a hashed bin


def craft_e(sw, edges, salt=SALT):
    """the swarm with its photon energies replaced, every one a hash of the photon's id: on every edge, one ulp below
    and above it; +-0, denormals, a negative, +-inf, NaNs with payloads; and values inside every bin"""
    edges = np.asarray(edges, dtype=np.float64)
    ng, nb = len(edges) - 1, len(edges) + 1
    ids = sw["id"]
    kind = som._mod(ids, salt + 1, KINDS)
    j = som._mod(ids, salt + 2, ng + 1)
    u = 0.01 + 0.98 * som._unit(ids, salt + 3)
    q = som._mod(ids, salt + 4, nb)
    lo = edges[np.clip(q - 1, 0, ng)]
    hi = edges[np.clip(q, 0, ng)]
    inner = np.where(q == 0, edges[0] - (1.0 + abs(edges[0])) * u, np.where(q == nb - 1, edges[ng] + (1.0 + abs(edges[ng])) * u,
                                                                         lo + (hi - lo) * u))
    e = np.where(kind == 0, edges[j], inner)
    e = np.where(kind == 1, np.nextafter(edges[j], -np.inf), e)
    e = np.where(kind == 2, np.nextafter(edges[j], np.inf), e)
    e = np.where(kind == 3, SPECIALS[som._mod(ids, salt + 5, len(SPECIALS))], e)
    out = dict(sw)
    out["e"] = np.ascontiguousarray(e)
    return out


def run_swarm(geom, lengths, edges, salt=mm.SALT, **kw):
    """moments_model.run_swarm (physical w over 60 binary orders, runs of the given lengths, slots that do not
    count, hashed slot order) with the crafted energies"""
    sw, cells = mm.run_swarm(geom, lengths, salt=salt, **kw)
    return craft_e(sw, edges, salt), cells


def hashed_swarm(geom, n, edges, salt=mm.SALT):
    return craft_e(mm.hashed_swarm(geom, n, salt), edges, salt)


def plan_groups(plan):
    """ngroups of run plan number ``plan``: the five widths in turn"""
    return NGROUPS[plan % len(NGROUPS)]


# ---- the Planck law -----------------------------------------------------------------------------------
def planck_tail(a, terms=200):
    """15 / pi^4 times the integral of x^3 / (e^x - 1) from a to infinity, from the series sum over k >= 1 of
    e^(-k a) (a^3 / k + 3 a^2 / k^2 + 6 a / k^3 + 6 / k^4)"""
    import math
    s = math.fsum(math.exp(-k * a) * (a ** 3 / k + 3 * a * a / k ** 2 + 6 * a / k ** 3 + 6 / k ** 4) for k in range(1, terms + 1))
    return 15.0 / math.pi ** 4 * s


def planck_fractions(x_edges):
    """the share of a Planck law's energy in the bins of edges x = h nu / k T: below the first, between, above the last"""
    tails = [1.0] + [planck_tail(x) for x in x_edges] + [0.0]
    return [tails[q] - tails[q + 1] for q in range(len(tails) - 1)]
