"""CPU conditions on the heterogeneous states of tests/hetero_states.py -- what makes tests/test_gpu_hetero.py
meaningful -- and pins of the oracle where a constant material state could not pin it.

* discrimination: on every (deck, pattern) of the GPU file a one-cell shift of the pattern along any single axis
  changes at least 5 % of the photons (a condition on the inputs);
* regime mix of the hybrid cases; class counts of the all-DDMC cases;
* fleck and P1..P3 against a numpy statement of UpdateDerivedTransportFields that the oracle did not write;
* Mesh.fill_ghosts against a direct evaluation by position.
"""
import itertools

import numpy as np
import pytest

import hetero_states as hs
from helpers import load_deck, run_oracle_cycles

ALL = hs.all_deck_patterns()


def _tau(pin):
    return pin.GetOrAddReal("jaybenne", "tau_ddmc", 5.0)


@pytest.mark.parametrize("cid,deck,ov,pattern", ALL, ids=[c[0] for c in ALL])
def test_a_one_cell_shift_changes_the_photons(cid, deck, ov, pattern):
    pin = load_deck(deck, ov)
    O, mesh, _ = hs.oracle_on(deck, ov, pattern)
    run_oracle_cycles(O, pin, 1)
    for d in range(mesh.ndim):
        shift = [0, 0, 0]
        shift[d] = 1
        S, _, _ = hs.oracle_on(deck, ov, pattern, shift=shift)
        run_oracle_cycles(S, pin, 1)
        frac = hs.differing_photons(O, S)
        print(f"{cid}: shift along x{d + 1} changes {frac:.3f} of {O.n} photons")
        assert frac >= 0.05, (cid, d, frac)


def _face_pairs(mesh, ddmc):
    """Counts of neighbouring cell pairs of different regimes: {(where, axis, "imc|ddmc" / "ddmc|imc"): n}; the
    first cell of a pair is the lower one along the axis.  where: interior (both cells in one block), same
    (across a face between blocks of one level), level (... of different levels), periodic (across a periodic
    domain face)."""
    m = mesh
    out = {}

    def add(key, lower, upper):
        for order, hit in (("imc|ddmc", ~lower & upper), ("ddmc|imc", lower & ~upper)):
            out[key + (order,)] = out.get(key + (order,), 0) + int(np.count_nonzero(hit))

    inner = ddmc[m.interior()]
    for d in range(m.ndim):
        lo, up = [slice(None)] * 4, [slice(None)] * 4
        lo[3 - d], up[3 - d] = slice(0, -1), slice(1, None)
        add(("interior", d), inner[tuple(lo)], inner[tuple(up)])
    flat = ddmc.reshape(m.nblocks, -1)
    ni, nj = m.ntot_dim[0], m.ntot_dim[1]
    for b in range(m.nblocks):
        dst, gid, cell = m.ghost_sources(b)
        kk, r = np.divmod(dst, nj * ni)
        jj, ii = np.divmod(r, ni)
        idx = [ii, jj, kk]
        outside = [np.where(idx[d] < m.is_[d], -1, np.where(idx[d] >= m.is_[d] + m.nx[d], 1, 0)) if d < m.ndim
                   else np.zeros_like(ii) for d in range(3)]
        nout = sum(np.abs(o) for o in outside)
        for d in range(m.ndim):
            for side in (-1, 1):
                edge = m.is_[d] - 1 if side < 0 else m.is_[d] + m.nx[d]
                sel = (nout == 1) & (outside[d] == side) & (idx[d] == edge)     # first ghost layer, faces only
                own = [ii[sel], jj[sel], kk[sel]]
                own[d] = own[d] - side
                mine = ddmc[b, own[2], own[1], own[0]]
                at_domain = bool(m.blk_xmin[b, d] <= m.gmin[d]) if side < 0 else bool(m.blk_xmax[b, d] >= m.gmax[d])
                if at_domain and m.mesh_bc[2 * d + (side > 0)] != 0:
                    continue        # a wall: checked separately
                for q in range(gid.shape[1]):
                    theirs = flat[gid[sel, q], cell[sel, q]]
                    lev = m.blk_level[gid[sel, q]]
                    for where, pick in (("periodic", np.full(len(lev), at_domain)),
                                        ("same", (lev == m.blk_level[b]) & (not at_domain)),
                                        ("level", (lev != m.blk_level[b]) & (not at_domain))):
                        if side < 0:
                            add((where, d), theirs[pick], mine[pick])
                        else:
                            add((where, d), mine[pick], theirs[pick])
    return out


HYBRID = [(f"{name}-{pat}", deck, ov, pat) for name, deck, ov, _ in hs.HYBRID_MESHES for pat in hs.HYBRID_PATTERNS]


@pytest.mark.parametrize("cid,deck,ov,pattern", HYBRID, ids=[c[0] for c in HYBRID])
def test_hybrid_states_mix_the_regimes(cid, deck, ov, pattern):
    pin = load_deck(deck, ov)
    O, mesh, pkg = hs.oracle_on(deck, ov, pattern)
    ddmc = hs.regime_map(mesh, pkg, O.fields["rho"], _tau(pin))
    sl = mesh.interior()
    share = float(ddmc[sl].mean())
    assert 0.2 <= share <= 0.8, share
    per_block = ddmc[sl].reshape(mesh.nblocks, -1).mean(axis=1)
    assert np.mean((per_block > 0) & (per_block < 1)) >= 0.25
    pairs = _face_pairs(mesh, ddmc)
    for d in range(mesh.ndim):
        for order in ("imc|ddmc", "ddmc|imc"):      # (both orders along an axis = its lower and its upper faces)
            assert pairs[("interior", d, order)] > 0, (d, order)
    for where in ("same", "level", "periodic"):
        assert sum(n for (w, _, _), n in pairs.items() if w == where) > 0, (where, pairs)
    # the reflecting walls (x1): cells of both regimes lie on each of them
    for side in (0, 1):
        at_wall = mesh.blk_xmin[:, 0] <= mesh.gmin[0] if side == 0 else mesh.blk_xmax[:, 0] >= mesh.gmax[0]
        wall = ddmc[sl][at_wall][..., 0 if side == 0 else -1]
        assert wall.any() and not wall.all(), side
    if pattern == "threshold":
        # cells on the threshold itself, of both kinds, and the oracle's expression separates them
        lo, hi = hs.threshold_pair(float(mesh.blk_dx[0, :mesh.ndim].min()), pkg, _tau(pin))
        assert np.nextafter(lo, np.inf) == hi
        b0 = O.fields["rho"][0][tuple(sl[1:])]
        d0 = ddmc[0][tuple(sl[1:])]
        assert np.count_nonzero(b0 == lo) > 10 and np.count_nonzero(b0 == hi) > 10
        assert not d0[b0 == lo].any() and d0[b0 == hi].all()
    # photons cross the interface: at least 2 % end in a cell of the other regime, in each direction
    before = hs.swarm_cells(mesh, O.sw, O.n)
    n0 = O.n
    run_oracle_cycles(O, pin, 1)
    assert O.n == n0
    to_ddmc, to_imc = hs.regime_crossings(ddmc, before, hs.swarm_cells(mesh, O.sw, O.n))
    print(f"{cid}: DDMC share {share:.3f}; IMC -> DDMC {to_ddmc:.3f}, DDMC -> IMC {to_imc:.3f} of the photons")
    assert to_ddmc >= 0.02 and to_imc >= 0.02


def _classes(deck, ov, pattern):
    pin = load_deck(deck, ov)
    O, mesh, pkg = hs.oracle_on(deck, ov, pattern)
    O.UpdateDerivedTransportFields(pin.GetReal("jaybenne", "dt"))
    ddmc = hs.regime_map(mesh, pkg, O.fields["rho"], _tau(pin))
    assert ddmc[mesh.interior()].all()        # an all-DDMC mesh stays one
    return hs.class_count(mesh, pkg, O), mesh


@pytest.mark.parametrize("name,deck,ov,ndim", hs.DDMC_MESHES, ids=[m[0] for m in hs.DDMC_MESHES])
def test_class_counts_of_the_all_ddmc_states(name, deck, ov, ndim):
    """The three selection branches of launch_transport: more classes than the table of 256 holds (the 64-byte
    gathers), at most 256 (cell codes), at most 64 (codes and records both in LDS on a small mesh)."""
    n_smooth, mesh = _classes(deck, ov, "smooth_dense")
    assert mesh.ndim == ndim
    ncell = mesh.nblocks * mesh.ncell
    if ncell > 256:
        assert n_smooth > 256, n_smooth
    else:
        assert n_smooth == ncell     # (1-D deck: 100 cells, a record of its own in each)
    n_pal, _ = _classes(deck, ov, hs.DDMC_PALETTE[name])
    print(f"{name}: {n_smooth} classes on smooth_dense, {n_pal} on {hs.DDMC_PALETTE[name]}")
    lo, hi = hs.DDMC_CLASS_BRACKET[name]
    assert lo < n_pal <= hi, n_pal


def test_a_hashed_palette_overflows_the_class_table_in_3d():
    """Why the 3-D meshes do not run palette3: a record holds the cell's own density and its six neighbours', so
    three hashed values make up to 3^7 records per level."""
    for name, deck, ov, _ in hs.DDMC_MESHES[2:]:
        n, _ = _classes(deck, ov, "palette3")
        assert n > 256, (name, n)


def _derived_numpy(mesh, par, rho, sie, dt):
    """UpdateDerivedTransportFields (reference jaybenne.cpp:304-489) in numpy: fleck everywhere, P1..P3 on
    the interior plus the upper face layer of their axis; ghost cells of rho / sie read at block faces."""
    m = mesh
    cv, kap_a, kap_s, apm = par["cv"], par["kappa_a"], par["kappa_s"], par["apm"]
    temp = np.maximum(sie / cv, 0.0)
    ss = (rho / apm) * kap_s
    aa = rho * kap_a
    t2 = temp * temp
    emis = (rho * kap_a) * ((4.0 * par["sb"]) * (t2 * t2))
    with np.errstate(invalid="ignore", divide="ignore"):
        fleck = 1.0 / (1.0 + (4.0 * emis / (rho * cv * temp)) * dt)
    sig = ss + aa
    out = {"fleck": fleck}
    for d, name in enumerate(("P1", "P2", "P3")[:m.ndim]):
        ax = 3 - d
        # faces f = is .. ie + 1 along d, interior elsewhere; cell f - 1 is the lower one
        up = [slice(None)] + [slice(m.is_[dd], m.is_[dd] + m.nx[dd] + (1 if dd == d else 0)) for dd in (2, 1, 0)]
        lo = list(up)
        lo[ax] = slice(m.is_[d] - 1, m.is_[d] + m.nx[d])
        shape = [m.nblocks, 1, 1, 1]
        dx_l = np.broadcast_to(m.blk_dx[:, d].reshape(shape), sig[tuple(up)].shape).copy()
        dx_u = dx_l.copy()
        lev = m.blk_level.astype(np.float64)
        first, last = [slice(None)] * 4, [slice(None)] * 4
        first[ax], last[ax] = slice(0, 1), slice(-1, None)
        dx_l[tuple(first)] = (2.0 ** (lev - m.blk_nbr_lev[:, 2 * d]) * m.blk_dx[:, d]).reshape(shape)
        dx_u[tuple(last)] = (2.0 ** (lev - m.blk_nbr_lev[:, 2 * d + 1]) * m.blk_dx[:, d]).reshape(shape)
        tau_l = dx_l * sig[tuple(lo)]
        tau_u = dx_u * sig[tuple(up)]
        tau_l = np.where(tau_l > par["tau_ddmc"], tau_l, 2.0 * 0.7104)
        tau_u = np.where(tau_u > par["tau_ddmc"], tau_u, 2.0 * 0.7104)
        out[name] = (2.0 / (3.0 * (tau_l + tau_u)), tuple(up))
    return out


DERIVED = [("2d-smr", "stepdiff_smr_hybrid", {"jaybenne/num_particles": 1000}),
           ("3d-smr", "stepdiff_smr_hybrid", dict(hs.SMR3D, **{"jaybenne/num_particles": 1000, "jaybenne/tau_ddmc": 20.0})),
           ("3-level", "stepdiff_smr_hybrid", dict(hs.C5_LEVEL2, **{"jaybenne/num_particles": 1000}))]


@pytest.mark.parametrize("pattern", ["smooth", "islands", "hot_spots"])
@pytest.mark.parametrize("name,deck,ov", DERIVED, ids=[c[0] for c in DERIVED])
def test_derived_fields_equal_the_formulas_bit_for_bit(name, deck, ov, pattern):
    from helpers import oracle_params
    if pattern == "hot_spots":    # (the Fleck factor needs absorption and emission to differ from one)
        ov = dict(ov, **{"mcblock/opacity_model": "constant", "mcblock/opacity_constant_value": 40.0,
                         "mcblock/initial_temperature": 1.0e6, "jaybenne/do_emission": "true"})
    pin = load_deck(deck, ov)
    O, mesh, pkg = hs.oracle_on(deck, ov, pattern)
    par = oracle_params(pin, pkg)
    dt = pin.GetReal("jaybenne", "dt")
    O.UpdateDerivedTransportFields(dt)
    want = _derived_numpy(mesh, par, O.fields["rho"], O.fields["sie"], dt)
    sl = mesh.interior()
    assert np.array_equal(O.fields["fleck"][sl], want["fleck"][sl])
    if pattern == "hot_spots":
        f = O.fields["fleck"][sl]
        assert f.min() > 0.0 and f.max() < 1.0 and len(np.unique(f)) > 0.4 * f.size
    for nm in ("P1", "P2", "P3")[:mesh.ndim]:
        val, where = want[nm]
        assert np.array_equal(O.fields[nm][where], val), nm
        if pattern != "hot_spots":
            assert len(np.unique(val)) > 2


@pytest.mark.parametrize("name,deck,ov", DERIVED, ids=[c[0] for c in DERIVED])
def test_ghost_fill_across_levels_by_position(name, deck, ov):
    """Mesh.fill_ghosts on ``smooth`` against the closed form evaluated at the source cells found by position: a
    same-level or coarser source gives that cell's value, a finer one the pairwise mean of the 2^ndim fine cells
    under the ghost cell; periodic wrap in x2 / x3, the nearest interior cell at the x1 walls."""
    from jaybenne_amd import mcblock
    from jaybenne_amd.mesh import Mesh
    pin = load_deck(deck, ov)
    mesh = Mesh.from_deck(pin)
    pkg = mcblock.Initialize(pin)
    nd = mesh.ndim
    rho = hs.initial_state(mesh, pkg, "smooth")["rho"]

    def closed_form(p):
        """rho of the leaf cell that contains each point of p [n, 3], and that cell's level."""
        nb = mesh.find_block(p)
        c = []
        for d in range(3):     # the cell's centre as Mesh.cell_centers forms it
            dx = mesh.blk_dx[nb, d]
            q = np.clip(np.floor((p[:, d] - mesh.blk_xmin[nb, d]) / dx), 0, mesh.nx[d] - 1) if d < nd else 0.0
            x0 = mesh.blk_xmin[nb, d] - mesh.is_[d] * dx
            c.append(x0 + (q + mesh.is_[d] + 0.5) * dx)
        f = np.sin(7.0 * c[0] + 0.3)
        if nd >= 2:
            f = f * np.cos(11.0 * c[1] - 0.2 + 3.0 * c[0])
        if nd >= 3:
            f = f * np.cos(5.0 * c[2] + 1.1 + 2.0 * c[1])
        return pkg.initial_density * (1.0 + 0.5 * f), mesh.blk_level[nb]

    kinds = set()
    offs = list(itertools.product(*[(-0.25, 0.25) if d < nd else (0.0,) for d in range(3)]))
    for b in range(mesh.nblocks):
        X, Y, Z = hs.cell_positions(mesh, b)
        ghost = np.ones(X.shape, dtype=bool)
        ghost[tuple(mesh.interior()[1:])] = False
        base = np.stack([X[ghost], Y[ghost], Z[ghost]], axis=1)
        samples, finer = [], np.zeros(len(base), dtype=bool)
        for o in offs:
            p = base + np.asarray(o) * mesh.blk_dx[b]
            for d in range(nd):
                ext = mesh.gmax[d] - mesh.gmin[d]
                if mesh.mesh_bc[2 * d] == 0:
                    p[:, d] = np.where(p[:, d] < mesh.gmin[d], p[:, d] + ext, p[:, d])
                    p[:, d] = np.where(p[:, d] > mesh.gmax[d], p[:, d] - ext, p[:, d])
                else:
                    h = 0.25 * mesh.blk_dx[b, d]
                    p[:, d] = np.clip(p[:, d], mesh.gmin[d] + h, mesh.gmax[d] - h)
            v, lev = closed_form(p)
            samples.append(v)
            finer |= lev > mesh.blk_level[b]
            kinds |= {int(np.sign(l - mesh.blk_level[b])) for l in np.unique(lev)}
        assert all(np.array_equal(s[~finer], samples[0][~finer]) for s in samples)   # one source cell
        s = list(samples)
        while len(s) > 1:
            s = [s[q] + s[q + 1] for q in range(0, len(s), 2)]
        want = np.where(finer, s[0] / len(offs), samples[0])
        assert np.array_equal(rho[b][ghost], want), b
    assert kinds == {-1, 0, 1}
