"""CPU conditions on the axis-asymmetric cases of tests/axis_cases.py -- what keeps tests/test_gpu_axes.py from
passing vacuously.

* distinctness: widths, cells per block, blocks per axis, leaf counts, origins and extents differ from axis to axis;
* traffic: every non-periodic face of every (case, boundary set) is touched by at least 100 histories, and
  switching a periodic pair to reflecting changes at least 100 photons;
* regimes and class counts of the DDMC / hybrid cases;
* ``mcblock.ProblemGenerator``'s closed-form ghosts against the by-position exchange on every new geometry;
* ``Mesh.find_block`` and the neighbour-level table against the oracle's relocation just beyond every block face.
"""
import numpy as np
import pytest

import axis_cases as ax
import hetero_states as hs
from helpers import load_deck, run_oracle_cycles
from jaybenne_amd import mcblock
from jaybenne_amd.mesh import BC_OUTFLOW, BC_PERIODIC, BC_REFLECT, Mesh

TRAFFIC_FLOOR = 100


def _distinct(v, n):
    return len(set(float(x) for x in v[:n])) == n


@pytest.mark.parametrize("geom", list(ax.GEOMETRIES))
def test_every_per_axis_number_differs_between_the_axes(geom):
    for kinds in ax.boundary_sets(geom).values():
        m = ax.mesh_of(geom, kinds)
        nd = m.ndim
        assert nd == len(ax.GEOMETRIES[geom].nx)
        for b in range(m.nblocks):
            assert _distinct(m.blk_dx[b], nd), (b, m.blk_dx[b])
        assert _distinct(m.nx, nd), m.nx
        assert _distinct(m.nleaf, nd), m.nleaf
        assert _distinct(m.nroot, nd), m.nroot
        assert _distinct(m.gmin, nd), m.gmin
        assert _distinct(m.gmax - m.gmin, nd)
        for d in range(nd):
            assert m.gmin[d] != -m.gmax[d] and m.gmin[d] != 0.0, d
        # the two faces of an axis differ in kind where they are not periodic
        for d in range(nd):
            lo, hi = m.swarm_bc[2 * d], m.swarm_bc[2 * d + 1]
            assert (lo == BC_PERIODIC and hi == BC_PERIODIC) or (lo != hi and BC_PERIODIC not in (lo, hi))
            assert [m.mesh_bc[2 * d], m.mesh_bc[2 * d + 1]] == [BC_PERIODIC if k == BC_PERIODIC else BC_OUTFLOW
                                                                for k in (lo, hi)]
    # over the sets every face of an active axis sees every kind it can
    seen = [set() for _ in range(2 * nd)]
    for kinds in ax.boundary_sets(geom).values():
        for f in range(2 * nd):
            seen[f].add(kinds[f])
    want = {ax.R, ax.O} if nd == 1 else {ax.R, ax.O, ax.P}
    assert all(s == want for s in seen), seen


def test_the_refined_meshes_are_the_ones_described():
    m = ax.mesh_of("G3S")
    assert m.nblocks == 52 and int((m.blk_level == 0).sum()) == 20 and int((m.blk_level == 1).sum()) == 32
    fine = m.blk_level == 1
    assert np.any(m.blk_xmin[fine, 1] == m.gmin[1]) and np.any(m.blk_xmax[fine, 2] == m.gmax[2])
    assert ax.mesh_of("G3U").nblocks == 24 and list(ax.mesh_of("G3U").nroot) == [2, 3, 4]
    for geom in ("G2S", "G2O"):
        assert set(ax.mesh_of(geom).blk_level) == {0, 1}


# ------------------------------------------------------------------------------------------------ traffic
def _run(case, kinds, pattern):
    ov = ax.overrides(case, None, kinds)
    O, mesh, pkg = hs.oracle_on(case.deck, ov, pattern)
    run_oracle_cycles(O, load_deck(case.deck, ov), case.cycles)
    return O


def _face_traffic(case, kinds, pattern):
    """{face or pair: histories that touched it}.  A non-periodic face: the oracle once more with that one face
    switched between reflecting and outflow -- the difference in surviving photons; a periodic pair: switched to
    reflecting -- the photons that differ, counted in both directions."""
    nd = len(ax.GEOMETRIES[case.geom].nx)
    base = _run(case, kinds, pattern)
    out = {}
    for d in range(nd):
        if kinds[2 * d] == ax.P:
            k = list(kinds)
            k[2 * d], k[2 * d + 1] = ax.R, ax.R
            other = _run(case, tuple(k), pattern)
            out[f"x{d + 1} pair"] = int(round(max(hs.differing_photons(base, other) * base.n,
                                                  hs.differing_photons(other, base) * other.n)))
            continue
        for side in (0, 1):
            k = list(kinds)
            k[2 * d + side] = ax.O if kinds[2 * d + side] == ax.R else ax.R
            other = _run(case, tuple(k), pattern)
            out[ax.FACES[2 * d + side]] = abs(base.n - other.n)
    return out


PAIRS = ax.all_pairs()


@pytest.mark.parametrize("case,bset", PAIRS, ids=[f"{c.id}-{s}" for c, s in PAIRS])
def test_photons_pass_through_every_face(case, bset):
    counts = _face_traffic(case, ax.boundary_sets(case.geom)[bset], ax.DDMC_PALETTE.get((case.id, bset), case.pattern))
    worst = min(counts, key=counts.get)
    print(f"{case.id} {bset}: {counts}; smallest {counts[worst]} at {worst}")
    assert counts[worst] >= TRAFFIC_FLOOR, counts


# ------------------------------------------------------------------------------------------------ regimes
def _tau(pin):
    return pin.GetOrAddReal("jaybenne", "tau_ddmc", 5.0)


HYBRID = [(c, p) for c in ax.CASES if c.family == "hybrid" for p in ax.HYBRID_PATTERNS]


@pytest.mark.parametrize("case,pattern", HYBRID, ids=[f"{c.id}-{p}" for c, p in HYBRID])
def test_hybrid_cases_have_both_regimes_on_both_levels(case, pattern):
    ov = ax.overrides(case, "S1")
    pin = load_deck(case.deck, ov)
    O, mesh, pkg = hs.oracle_on(case.deck, ov, pattern)
    ddmc = hs.regime_map(mesh, pkg, O.fields["rho"], _tau(pin))[mesh.interior()]
    shares = []
    for lev in (0, 1):
        cells = ddmc[mesh.blk_level == lev]
        assert cells.size > 0
        shares.append(float(cells.mean()))
        assert 0.1 <= shares[-1] <= 0.9, (lev, shares)
    print(f"{case.id} {pattern}: DDMC share {shares[0]:.2f} / {shares[1]:.2f} on level 0 / 1")


DDMC = [c for c in ax.CASES if c.family == "ddmc"]


@pytest.mark.parametrize("case", DDMC, ids=[c.id for c in DDMC])
def test_all_ddmc_cases_stay_all_ddmc_and_their_classes_fit_the_brackets(case):
    counts = {}
    ncell = None
    for bset in ax.boundary_sets(case.geom):
        for pattern in ("smooth_dense", ax.DDMC_PALETTE[case.id, bset]):
            ov = ax.overrides(case, bset)
            pin = load_deck(case.deck, ov)
            O, mesh, pkg = hs.oracle_on(case.deck, ov, pattern)
            O.UpdateDerivedTransportFields(pin.GetReal("jaybenne", "dt"))
            assert hs.regime_map(mesh, pkg, O.fields["rho"], _tau(pin))[mesh.interior()].all()
            counts[pattern, bset] = hs.class_count(mesh, pkg, O)
            ncell = mesh.nblocks * mesh.ncell
    print(f"{case.id}: distinct step records {counts}")
    lo, hi = ax.DDMC_CLASS_BRACKET[case.id]
    for (pattern, bset), n in counts.items():
        if pattern == "smooth_dense":
            assert n > 256 or n == ncell <= 256, (bset, n)      # the 64-byte gathers (1-D: a record per cell)
        else:
            assert lo < n <= hi, (pattern, bset, n)


# ------------------------------------------------------------------------------------------------ initial state
GEOM_SETS = [(g, s) for g in ax.GEOMETRIES for s in ax.boundary_sets(g)]


@pytest.mark.parametrize("geom,bset", GEOM_SETS, ids=[f"{g}-{s}" for g, s in GEOM_SETS])
def test_closed_form_ghosts_equal_the_exchange_by_position(geom, bset):
    """The stepdiff state with its step off the block boundaries, x1 periodic in S2 and x2 / x3 outflow."""
    g = ax.GEOMETRIES[geom]
    pin = load_deck("stepdiff_smr" if g.refine else "stepdiff", ax.geometry_overrides(geom, ax.boundary_sets(geom)[bset]))
    mesh = Mesh.from_deck(pin)
    pkg = mcblock.Initialize(pin)
    a = mcblock.ProblemGenerator(mesh, pkg, analytic_ghosts=True)
    b = mcblock.ProblemGenerator(mesh, pkg, analytic_ghosts=False)
    for k in ("rho", "sie", "u"):
        assert np.array_equal(a[k], b[k]), (k, int(np.count_nonzero(a[k] != b[k])), a[k].size)
    if mesh.gmin[0] < 0.0:
        assert len(np.unique(a["sie"])) == 2        # the step is inside the domain
    # ... and a subset of the blocks (what a rank asks for) gets the same arrays
    some = np.arange(mesh.nblocks)[::3]
    sub = mcblock.ProblemGenerator(mesh, pkg, gids=some)
    for k in ("rho", "sie", "u"):
        assert np.array_equal(sub[k], a[k][some]), k


# ------------------------------------------------------------------------------------------------ host mirrors
@pytest.mark.parametrize("geom,bset", GEOM_SETS, ids=[f"{g}-{s}" for g, s in GEOM_SETS])
def test_relocation_beyond_every_block_face_agrees_with_the_host_tables(geom, bset):
    """One photon per block face, a quarter of a finest-level cell inside it and flying outwards for half such a
    cell (next to the block's lower corner in the other axes, so that a finer neighbour is met at its own
    level): the oracle's apply_swarm_bcs + find_block against the boundary kinds, ``Mesh.find_block`` and
    ``Mesh.blk_nbr_lev`` evaluated here."""
    from oracle import orc
    g = ax.GEOMETRIES[geom]
    kinds = ax.boundary_sets(geom)[bset]
    deck = "stepdiff_smr" if g.refine else "stepdiff"
    ov = dict(ax.geometry_overrides(geom, kinds), **{"jaybenne/num_particles": 64, hs.SCAT: 1.0e-6})
    pin = load_deck(deck, ov)
    O, m, pkg = hs.oracle_on(deck, ov, "smooth", capacity_factor=1.0)
    nd = m.ndim
    c = pkg.opacity.c
    dt = pin.GetReal("jaybenne", "dt")
    fine = (m.gmax - m.gmin) / np.asarray(m.nleaf, dtype=np.float64)
    n = 2 * nd * m.nblocks
    assert n <= O.cap
    want_blk, want_alive, want_pos, want_v, crossing = [], [], [], [], []
    q = 0
    for b in range(m.nblocks):
        for d in range(nd):
            for side in (0, 1):
                p = m.blk_xmin[b] + 0.25 * fine * (np.arange(3) < nd)
                p[nd:] = 0.5 * (m.gmin[nd:] + m.gmax[nd:])
                face = m.blk_xmin[b, d] if side == 0 else m.blk_xmax[b, d]
                sign = -1.0 if side == 0 else 1.0
                p[d] = face - sign * 0.25 * fine[d]
                for k, name in enumerate(("x", "y", "z")):
                    O.sw[name][q] = p[k]
                    O.sw["v" + name][q] = sign * c if k == d else 0.0
                O.sw["t"][q] = dt - 0.5 * fine[d] / c
                O.sw["blk"][q] = b
                O.sw["status"][q] = orc.ST_ACTIVE
                O.sw["id"][q] = q
                O.sw["rng"][q] = orc.stream_start(1, q)
                O.sw["w"][q] = O.sw["e"][q] = 1.0
                # the host's answer for a point a quarter of a finest-level cell beyond the face
                e = p.copy()
                e[d] = face + sign * 0.25 * fine[d]
                v = sign
                alive = True
                outside = e[d] < m.gmin[d] or e[d] > m.gmax[d]
                if outside:
                    kind = m.swarm_bc[2 * d + side]
                    wall = m.gmin[d] if side == 0 else m.gmax[d]
                    if kind == BC_REFLECT:
                        e[d] = wall - sign * 0.25 * fine[d]
                        v = -sign
                    elif kind == BC_PERIODIC:
                        e[d] = (m.gmax[d] if side == 0 else m.gmin[d]) + sign * 0.25 * fine[d]
                    else:
                        assert kind == BC_OUTFLOW
                        alive = False
                dest = int(m.find_block(e[None, :])[0]) if alive else -1
                if alive and not (outside and m.swarm_bc[2 * d + side] == BC_REFLECT):
                    # the neighbour-level table: the level of the block behind the face (its own at a wall)
                    assert m.blk_nbr_lev[b, 2 * d + side] == m.blk_level[dest], (b, d, side)
                else:
                    assert m.blk_nbr_lev[b, 2 * d + side] == m.blk_level[b], (b, d, side)
                want_blk.append(dest)
                want_alive.append(alive)
                want_pos.append(e[d])
                want_v.append(v * c)
                crossing.append((b, d, side))
                q += 1
    O.n = n
    O.TransportPhotons(0.0, dt)
    pos = np.stack([O.sw[k][:n] for k in ("x", "y", "z")], axis=1)
    vel = np.stack([O.sw["v" + k][:n] for k in ("x", "y", "z")], axis=1)
    kinds_seen = set()
    for q, (b, d, side) in enumerate(crossing):
        assert (O.sw["status"][q] == orc.ST_ACTIVE) == want_alive[q], crossing[q]
        if not want_alive[q]:
            assert O.sw["status"][q] == orc.ST_ESCAPED
            kinds_seen.add("escaped")
            continue
        assert O.sw["blk"][q] == want_blk[q], (crossing[q], int(O.sw["blk"][q]), want_blk[q])
        assert abs(pos[q, d] - want_pos[q]) <= 1e-3 * fine[d], (crossing[q], pos[q, d], want_pos[q])
        assert vel[q, d] == want_v[q], crossing[q]
        kinds_seen.add("reflected" if want_blk[q] == b and vel[q, d] * (1 if side else -1) < 0 else "moved")
        # ... and the block found holds the photon, in the cell the oracle says
        dest = want_blk[q]
        assert np.all(pos[q, :nd] >= m.blk_xmin[dest, :nd]) and np.all(pos[q, :nd] <= m.blk_xmax[dest, :nd])
        for k, name in enumerate(("ip", "jp", "kp")[:nd]):
            cell = int(np.floor((pos[q, k] - m.blk_xmin[dest, k]) / m.blk_dx[dest, k])) + m.is_[k]
            assert O.sw[name][q] == cell, (crossing[q], name)
    assert kinds_seen == {"escaped", "reflected", "moved"}
