"""The cases that make the per-event temperature and the photon's own frequency count, and what the CPU oracle says
about them.

``k_transport<NDIM, DDMC, TALLY, GRAY = 0>`` evaluates the opacities at every event from the cell's rho and sie and the
photon's frequency.  Under the gray models the temperature and the frequency are dead, and the one test with EPBremss
(tests/test_gpu_parity.py::test_epbremss_opacity_bit_exact) runs decks whose material is a function of x1 alone, on
symmetric axes, one photon per lane.  The rows below are EPBremss on the geometries and boundary sets of
tests/axis_cases.py, on the ``smooth_hot_fine`` state of tests/hetero_states.py (rho AND sie different in every cell),
with emission and without feedback; each row carries the ``mass_scale`` and scattering value at which its histories
have several events, all three outcomes are common and -- with ``use_ddmc`` -- photons of both regimes share cells: the
DDMC criterion ``dx_push (sigma_a(nu) + sigma_s) > tau_ddmc`` is then decided by the photon's frequency.

tests/test_freq_host.py (CPU) holds those conditions on the oracle alone; tests/test_gpu_freq.py runs the kernel.
Both import the table and the functions below.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import axis_cases as ax
import hetero_states as hs
from helpers import load_deck, oracle_params

PATTERN = "smooth_hot_fine"
MASS = "mcblock/mass_scale"
SCAT, NP, TAU = ax.SCAT, ax.NP, ax.TAU
EPBREMSS = {"mcblock/opacity_model": "ep_bremss", "jaybenne/do_emission": "true", "jaybenne/do_feedback": "false"}

# (id, geometry, boundary set, deck, use_ddmc, photons, mass_scale, scattering value, tau_ddmc, cycles, grid caps of the
# lane-reuse runs).  The photon counts are within those of axis_cases.CASES (6 000 .. 30 000); the scales are those at
# which the conditions of tests/test_freq_host.py hold (its docstring has the measured table).  In 1-D nothing lies
# between "absorbed in one event" (mass_scale 3e-13) and "nothing on the DDMC side" (3e-14) but a narrow window, and
# tau_ddmc = 1 there keeps scattering alone (dx sigma_s <= 0.6) on the IMC side
Case = namedtuple("Case", "id geom bset deck ddmc photons mass_scale scat tau cycles grids")
CASES = [
    Case("F1-imc", "G1", "OR", "stepdiff", False, 8000, 5.0e-14, 1.0e15, None, 2, (1, 3)),
    Case("F1-hybrid", "G1", "RO", "stepdiff_ddmc", True, 20000, 8.0e-14, 3.0e14, 1.0, 2, (1,)),
    Case("F3U-imc", "G3U", "S2", "stepdiff", False, 6000, 3.0e-13, 1.0e14, None, 2, (1,)),
    Case("F3S-imc", "G3S", "S3", "stepdiff_smr", False, 20000, 1.0e-9, 1.0e12, None, 2, (1,)),
    Case("F2S-hybrid", "G2S", "S1", "stepdiff_smr_hybrid", True, 30000, 3.0e-13, 1.0e15, 10.0, 2, (1, 3)),
    Case("F3S-hybrid", "G3S", "S3", "stepdiff_smr_hybrid", True, 30000, 3.0e-13, 1.0e15, 10.0, 2, (1,)),
    Case("F2O-hybrid", "G2O", "S2", "stepdiff_smr_hybrid", True, 30000, 3.0e-13, 1.0e15, 10.0, 2, (1,)),
    Case("F3O-hybrid", "G3O", "S1", "stepdiff_ddmc", True, 20000, 3.0e-13, 1.0e14, 10.0, 2, (1,)),
]
BY_ID = {c.id: c for c in CASES}
DDMC_CASES = [c for c in CASES if c.ddmc]
CAPACITY_FACTOR = 4.0            # emission adds photons every cycle

# the gray control of test_freq_host: the same kernel family (JB_PER_EVENT_OPACITY=1 on the device; the oracle always
# evaluates its models per event), opacity_model = none
GRAY_CONTROL = ax.BY_ID["G2S-hybrid"]


def kinds_seen():
    """{axis: the boundary kinds it carries somewhere in the table}, and the same over the 3-D rows alone."""
    every, in_3d = {0: set(), 1: set(), 2: set()}, {0: set(), 1: set(), 2: set()}
    for c in CASES:
        nd = len(ax.GEOMETRIES[c.geom].nx)
        kinds = ax.boundary_sets(c.geom)[c.bset]
        for d in range(nd):
            every[d] |= {kinds[2 * d], kinds[2 * d + 1]}
            if nd == 3:
                in_3d[d] |= {kinds[2 * d], kinds[2 * d + 1]}
    return every, in_3d


def overrides(case, **more):
    ov = dict(ax.geometry_overrides(case.geom, ax.boundary_sets(case.geom)[case.bset]), **EPBREMSS)
    ov.update({NP: case.photons, MASS: case.mass_scale, SCAT: case.scat})
    if case.tau is not None:
        ov[TAU] = case.tau
    ov.update(more)
    return ov


def oracle_of(case, shift=(0, 0, 0), **more):
    """(pin, oracle, mesh, mcblock package) of a row, the state moved by ``shift`` cells."""
    ov = overrides(case, **more)
    O, mesh, pkg = hs.oracle_on(case.deck, ov, PATTERN, shift=shift, capacity_factor=CAPACITY_FACTOR)
    return load_deck(case.deck, ov), O, mesh, pkg


def model_params(pin, pkg):
    """What ``orc.model_eval`` takes: the oracle's own parameters of the deck."""
    return oracle_params(pin, pkg)


def at_transport(O, fn):
    """Call ``fn(O)`` on the swarm as every TransportPhotons call from now on finds it (the emission source has run by
    then) and keep what it returns, one entry per call."""
    kept = []
    inner = O.TransportPhotons

    def transport(t_start, dt, first=0, last=None):
        kept.append(fn(O))
        return inner(t_start, dt, first, last)

    O.TransportPhotons = transport
    return kept


def cell_inputs(O, mesh, par, n=None):
    """(rho, temp, dx_push, cell key) per photon of the swarm as it stands, as the history loop forms them (orc.c:
    eos_temperature = sie / cv where positive; dx_push the smallest of the block's three widths)."""
    n = O.n if n is None else n
    blk, kp, jp, ip = hs.swarm_cells(mesh, O.sw, n)
    rho = O.fields["rho"][blk, kp, jp, ip]
    t = O.fields["sie"][blk, kp, jp, ip] / par["cv"]
    temp = np.where(t > 0.0, t, 0.0)
    dx_push = mesh.blk_dx[blk].min(axis=1)
    key = ((blk * mesh.field_shape[1] + kp) * mesh.field_shape[2] + jp) * mesh.field_shape[3] + ip
    return rho, temp, dx_push, key


def is_ddmc(par, rho, temp, dx_push, e):
    """The oracle's own expression, ``dx_push * (ss + aa) > tau_ddmc`` (orc.c, the history loop), with its models."""
    from oracle import orc
    orc.set_math_mode(orc.MATH_PORTABLE)
    aa = orc.model_eval(par, 0, rho, temp, e)
    ss = orc.model_eval(par, 2, rho, temp, e)
    return dx_push * (ss + aa) > par["tau_ddmc"]


def regime_mix(O, mesh, par, n=None):
    """(share of the photons that start on the DDMC side, share of the occupied cells that hold photons of both
    regimes) for the swarm as it stands."""
    n = O.n if n is None else n
    rho, temp, dx_push, key = cell_inputs(O, mesh, par, n)
    d = is_ddmc(par, rho, temp, dx_push, O.sw["e"][:n].copy())
    cells, inv = np.unique(key, return_inverse=True)
    n_d = np.bincount(inv, weights=d.astype(np.float64), minlength=len(cells))
    n_all = np.bincount(inv, minlength=len(cells))
    mixed = (n_d > 0) & (n_d < n_all)
    return float(d.mean()), float(mixed.mean())


E_LOW, E_HIGH = 1.0, 1.0e30       # brackets every frequency the Planck sampler gives between numin and numax


def threshold_frequencies(par, rho, temp, dx_push):
    """Per cell (arrays of equal length): neighbouring doubles ``e_lo < e_hi`` with ``is_ddmc(e_lo)`` true and
    ``is_ddmc(e_hi)`` false, and ``found``: false where E_LOW is not DDMC or E_HIGH is (no threshold in frequency).
    Bisection on the doubles' bit patterns: every step keeps "lo is DDMC, hi is not" by the oracle's own expression, so
    the pair it ends on is the flip itself whatever the rounding does to monotonicity nearby."""
    n = len(rho)
    lo, hi = np.full(n, E_LOW), np.full(n, E_HIGH)
    found = is_ddmc(par, rho, temp, dx_push, lo) & ~is_ddmc(par, rho, temp, dx_push, hi)
    lo_i, hi_i = lo.view(np.int64).copy(), hi.view(np.int64).copy()      # (positive doubles order as their bits do)
    while np.any(hi_i - lo_i > 1):
        mid_i = lo_i + (hi_i - lo_i) // 2
        d = is_ddmc(par, rho, temp, dx_push, mid_i.view(np.float64).copy())
        lo_i = np.where(d, mid_i, lo_i)
        hi_i = np.where(d, hi_i, mid_i)
    e_lo, e_hi = lo_i.view(np.float64).copy(), hi_i.view(np.float64).copy()
    ok = is_ddmc(par, rho, temp, dx_push, e_lo) & ~is_ddmc(par, rho, temp, dx_push, e_hi) & (np.nextafter(e_lo, np.inf) == e_hi)
    assert np.all(ok[found])
    return e_lo, e_hi, found


def on_the_threshold(O, mesh, par, n=None):
    """The frequencies of test d: every 5th photon of the swarm (by creation id) gets ``e_lo`` or ``e_hi`` of the cell
    it starts in, by the next bit of the id.  Returns (e [n], on the DDMC side [n] bool, on the IMC side [n] bool)."""
    n = O.n if n is None else n
    rho, temp, dx_push, _ = cell_inputs(O, mesh, par, n)
    e_lo, e_hi, found = threshold_frequencies(par, rho, temp, dx_push)
    ids = O.sw["id"][:n].astype(np.int64)
    pick = (ids % 5 == 0) & found
    low = pick & ((ids // 5) % 2 == 0)
    high = pick & ~low
    e = O.sw["e"][:n].copy()
    e[low], e[high] = e_lo[low], e_hi[high]
    return e, low, high
