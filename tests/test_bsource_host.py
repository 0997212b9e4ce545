"""The boundary source's semantics (include/jaybenne_amd.h: jb_source_boundary_count / _fill) on the CPU: the numpy
model of tests/bsource_model.py against closed forms, and the model's photons transported by the CPU oracle -- a vacuum
slab, black walls in equilibrium with the material, and a DDMC slab whose albedo admits or reflects them.  No GPU."""
import math

import numpy as np
import pytest

import axis_cases as ax
import bsource_model as bm
from helpers import load_deck, make_oracle

OUT = "outflow"
N_B = 2000


def _constants(pin):
    from jaybenne_amd import mcblock
    pkg = mcblock.Initialize(pin)
    return pkg.opacity.sb, pkg.opacity.c, pin.GetOrAddInteger("jaybenne", "seed", 123)


# ---- 1. the model against closed forms, over all six faces ---------------------------------------
@pytest.fixture(scope="module")
def open_box():
    """G3U of tests/axis_cases.py (2 x 3 x 4 blocks, every per-axis number different) with every face outflow."""
    kinds = (OUT,) * 6
    pin = load_deck("stepdiff", ax.geometry_overrides("G3U", kinds))
    return ax.mesh_of("G3U", kinds), pin


@pytest.mark.parametrize("face", range(6), ids=bm.FACES)
def test_model_against_closed_forms(open_box, face):
    mesh, pin = open_box
    sb, c, seed = _constants(pin)
    dt = pin.GetReal("jaybenne", "dt")
    temps = [0.0] * 6
    temps[face] = 1.0e6 * (1.0 + 0.1 * face)
    cells, rec = bm.count(mesh, sb, seed, temps, N_B, dt, epoch=1)
    want = bm.closed_form_energy(mesh, sb, temps, dt)
    for f in range(6):
        if f == face:
            assert abs(rec["e_face"][f] - want[f]) <= 1e-12 * want[f], (rec["e_face"][f], want[f])
        else:
            assert rec["e_face"][f] == 0.0 and rec["n_face"][f] == 0
    # stochastic rounding: floor or ceil of npc in every cell, N_b in total to within the rounding's scatter
    total = bm.face_cells_total(mesh, temps)
    npc = N_B / total
    counts = [s for b in cells for _, _, s, _ in cells[b]]
    assert len(counts) == total and set(counts) <= {math.floor(npc), math.floor(npc) + 1}
    assert abs(sum(counts) - N_B) <= 5.0 * math.sqrt(total * 0.25)      # (a Bernoulli sum: variance <= 1/4 per cell)
    d, upper = face >> 1, face & 1
    mus, e_sum = [], []
    base = 10 ** 6
    for b in sorted(cells):
        sw = bm.photons(mesh, sb, c, seed, temps, cells[b], b, base, 0.25, dt)
        base += len(sw["id"])
        pos = (sw["x"], sw["y"], sw["z"])[d]
        vel = np.stack([sw["vx"], sw["vy"], sw["vz"]])
        idx = (sw["ip"], sw["jp"], sw["kp"])[d] - mesh.is_[d]
        dx = mesh.blk_dx[b, d]
        lo = mesh.blk_xmin[b, d] + idx * dx
        hi = lo + dx
        assert np.all((pos > lo) & (pos < hi))                           # strictly inside its cell on axis d
        wall = mesh.gmax[d] if upper else mesh.gmin[d]
        assert np.all(np.abs(pos - wall) < 2.5 * bm.K_EPS_IMC * dx) and np.all(pos != wall)
        assert np.all(idx == (mesh.nx[d] - 1 if upper else 0))
        assert np.all(vel[d] < 0.0) if upper else np.all(vel[d] > 0.0)   # inward
        speed = np.sqrt((vel * vel).sum(axis=0))
        assert np.all(np.abs(speed - c) <= 1e-15 * c)
        for a in range(3):                                               # inside the cell on the other axes too
            if a != d:
                ia = (sw["ip"], sw["jp"], sw["kp"])[a] - mesh.is_[a]
                la = mesh.blk_xmin[b, a] + ia * mesh.blk_dx[b, a]
                pa = (sw["x"], sw["y"], sw["z"])[a]
                assert np.all((pa >= la) & (pa <= la + mesh.blk_dx[b, a]))
        assert np.all((sw["t"] > 0.25) & (sw["t"] < 0.25 + dt)) and np.all(sw["e"] > 0.0) and np.all(sw["w"] > 0.0)
        mus.append(np.abs(vel[d]) / c)
        e_sum.append(math.fsum(sw["w"]))
    mu = np.concatenate(mus)
    assert abs(mu.mean() - 2.0 / 3.0) <= 5.0 * math.sqrt((1.0 / 18.0) / len(mu)), mu.mean()   # the cosine law
    assert abs(math.fsum(e_sum) - want[face]) <= 1e-12 * want[face]      # the photons carry the face's energy


def test_model_refuses_what_the_library_refuses(open_box):
    mesh, pin = open_box
    sb, c, seed = _constants(pin)
    with pytest.raises(ValueError, match="npc"):
        bm.count(mesh, sb, seed, [1.0e6, 0, 0, 0, 0, 0], 50, 1e-11, 1)      # 96 cells on ix1
    with pytest.raises(ValueError, match="temperature"):
        bm.count(mesh, sb, seed, [-1.0, 0, 0, 0, 0, 0], N_B, 1e-11, 1)
    periodic = ax.mesh_of("G3U")                                            # S1: x3 periodic
    with pytest.raises(ValueError, match="periodic"):
        bm.count(periodic, sb, seed, [0, 0, 0, 0, 1.0e6, 0], N_B, 1e-11, 1)
    slab = ax.mesh_of("G1")
    with pytest.raises(ValueError, match="inactive"):
        bm.count(slab, sb, seed, [0, 0, 1.0e6, 0, 0, 0], N_B, 1e-11, 1)


# ---- 2. the model's photons on the oracle ----------------------------------------------------------
SLAB = {"parthenon/mesh/nx1": 8, "parthenon/meshblock/nx1": 8, "parthenon/swarm/ix1_bc": OUT,
        "parthenon/swarm/ox1_bc": OUT}
# opacities zero: the deck path accepts opacity_model = none with scattering_model = none
VACUUM = dict(SLAB, **{"mcblock/scattering_model": "none", "mcblock/initial_radiation": "none",
                       "jaybenne/num_particles": 1000})


def test_vacuum_slab():
    from oracle import orc
    pin = load_deck("stepdiff", VACUUM)
    O, mesh, _ = make_oracle(pin, orc.MATH_PORTABLE, threads=1)
    assert O.n == 0 and O.P.kappa_a == 0.0 and O.P.kappa_s == 0.0 and mesh.nblocks == 1 and list(mesh.nx) == [8, 1, 1]
    temps = [1.0e6, 0.0, 0.0, 0.0, 0.0, 0.0]
    dt, t = pin.GetReal("jaybenne", "dt"), 0.0
    sourced, escaped = [], []
    for _ in range(4):
        led = bm.oracle_cycle(O, pin, t, temps, N_B)
        t += dt
        assert led["n_absorbed"] == 0 and led["e_absorbed"] == 0.0
        assert led["e_escaped"][0] == 0.0 and led["n_escaped"][0] == 0
        sourced.append(led["e_sourced"])
        escaped.append(led["e_escaped"][1])
        lhs = math.fsum(sourced)
        assert abs(lhs - math.fsum(escaped) - led["e_census"]) <= 1e-12 * lhs
    assert escaped[-1] > 0.5 * sourced[-1]        # (c dt is the slab's length: the flow through ox1 has set in)


T_B = 1.0e6
EQUILIBRIUM = dict(SLAB, **{"mcblock/scattering_model": "none", "mcblock/initial_radiation": "thermal",
                            "mcblock/opacity_model": "constant", "mcblock/opacity_constant_value": 2.0,
                            "mcblock/initial_temperature": T_B, "jaybenne/num_particles": 4000,
                            "jaybenne/do_emission": "true", "jaybenne/do_feedback": "true",
                            "parthenon/job/problem_id": "equilibrium"})


def test_black_walls_in_equilibrium():
    """ix1 and ox1 at T_b, material and initial radiation at T_b, emission and feedback on: what leaves through a
    face is what the wall behind it sends in, and the census holds (4 sb / c) T_b^4 V -- over cycles 5..20, within 5
    standard errors taken from the cycle-to-cycle scatter.  Fixed seed, no cycle left out."""
    from oracle import orc
    pin = load_deck("stepdiff", EQUILIBRIUM)
    O, mesh, _ = make_oracle(pin, orc.MATH_PORTABLE, threads=1, capacity_factor=8.0)
    temps = [T_B, T_B, 0.0, 0.0, 0.0, 0.0]
    dt, t = pin.GetReal("jaybenne", "dt"), 0.0
    ratio, census = ([], []), []
    for cycle in range(1, 21):
        led = bm.oracle_cycle(O, pin, t, temps, N_B)
        t += dt
        assert led["residual"] <= 1e-12
        if cycle >= 5:
            for f in (0, 1):
                ratio[f].append(led["e_escaped"][f] / led["e_sourced_face"][f])
            census.append(led["e_census"])
    for f in (0, 1):
        r = np.array(ratio[f])
        se = r.std(ddof=1) / math.sqrt(len(r))
        print(f"{bm.FACES[f]}: escaped / sourced = {r.mean():.5f} +- {se:.5f}")
        assert abs(r.mean() - 1.0) <= 5.0 * se, (f, r.mean(), se)
    volume = float(np.prod(np.asarray(mesh.gmax) - np.asarray(mesh.gmin)))
    want = (4.0 * O.P.sb / O.P.c) * T_B ** 4 * volume
    e = np.array(census)
    se = e.std(ddof=1) / math.sqrt(len(e))
    print(f"census / equilibrium = {e.mean() / want:.5f} +- {se / want:.5f}")
    assert abs(e.mean() - want) <= 5.0 * se, (e.mean(), want, se)


def test_ddmc_slab_admits_and_reflects():
    """The stepdiff_ddmc material (every cell a DDMC cell) behind a source on ix1: the albedo condition of
    ptcl_ddmc_albedo admits a photon with probability P = 2 P_f (1 + 1.5 mu), P_f = (2 / 3) / (sigma dx + 2 lambda),
    on the first draw behind the source's ten -- evaluated here from the model's photons, not read off the oracle --
    and a rejected photon leaves through the face it came from."""
    from oracle import orc
    pin = load_deck("stepdiff_ddmc", {"parthenon/swarm/ix1_bc": OUT, "mcblock/initial_radiation": "none",
                                      "jaybenne/num_particles": 1000})
    O, mesh, pkg = make_oracle(pin, orc.MATH_PORTABLE, threads=1, capacity_factor=4.0)
    assert O.n == 0
    temps = [1.0e6, 0.0, 0.0, 0.0, 0.0, 0.0]
    dt = pin.GetReal("jaybenne", "dt")
    led = bm.oracle_cycle(O, pin, 0.0, temps, N_B)
    sw = led["swarm_after_transport"]
    n = led["n_sourced"]
    assert n == len(sw["id"]) and abs(n - N_B) <= 1
    # the source's own photons again, for their direction and the state of their stream behind the ten draws
    cells, _ = bm.count(mesh, O.P.sb, O.P.seed, temps, N_B, dt, epoch=1)
    born = bm.photons(mesh, O.P.sb, O.P.c, O.P.seed, temps, cells[0], 0, 0, 0.0, dt)
    assert np.array_equal(born["id"], sw["id"])
    sigma = pkg.initial_density * pkg.opacity.kappa + (pkg.initial_density / pkg.scattering.apm) * pkg.scattering.kappa_s
    dx = float(mesh.blk_dx[0, 0])
    assert dx * sigma > pin.GetOrAddReal("jaybenne", "tau_ddmc", 5.0)           # a DDMC cell
    p_f = (2.0 / 3.0) / (sigma * dx + 2.0 * 0.7104)
    p_admit = 2.0 * p_f * (1.0 + 1.5 * born["vx"] / O.P.c)
    xi = np.array([orc.draw_stream(int(s), 1)[0][0] for s in born["rng"]])
    rejected = xi > p_admit
    assert rejected.sum() >= 100 and (~rejected).sum() >= 100, (rejected.sum(), (~rejected).sum())
    assert np.all(sw["status"][rejected] == bm.lc.ST_ESCAPED) and np.all(sw["x"][rejected] < mesh.gmin[0])
    assert np.all(sw["t"][rejected] == born["t"][rejected])                      # ... at once
    assert led["n_escaped"][0] >= rejected.sum() and led["n_escaped_unclassified"] == 0
    assert led["residual"] <= 1e-12
