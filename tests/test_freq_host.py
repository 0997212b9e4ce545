"""CPU conditions on the rows of tests/freq_cases.py -- what keeps tests/test_gpu_freq.py from passing vacuously.
Everything here is the oracle's.  Every test prints what it measured; the values at the time of writing:

    row / set        a: sie moved one cell    b: the neigh-   d: DDMC side /    e: at the call / census / absorbed /
                     along x1 / x2 / x3       bour's e        cells of both     escaped / events per photon
    F1-imc / OR      1.000                    1.000           --                10 000 /  3 634 /  6 102 /   264 /  53
    F1-hybrid / RO   1.000                    1.000           0.24 / 0.94       24 997 /  2 335 / 22 264 /   398 /  18
    F3U-imc / S2     0.606 / 0.582 / 0.540    0.736           --                 6 249 /    911 /  4 678 /   660 /  14
    F3S-imc / S3     1.000 / 1.000 / 1.000    1.000           --                20 433 /  1 873 / 17 242 / 1 318 / 177
    F2S-hybrid / S1  0.076 / 0.087            0.117           0.66 / 0.64       32 131 /  3 966 / 27 501 /   664 /  39
    F3S-hybrid / S3  0.091 / 0.105 / 0.075    0.148           0.56 / 0.42       30 699 /  3 871 / 22 999 / 3 829 /  60
    F2O-hybrid / S2  0.102 / 0.117            0.234           0.46 / 0.54       31 271 /  3 478 / 27 308 /   485 /  46
    F3O-hybrid / S1  0.331 / 0.334 / 0.326    0.379           0.68 / 0.30       20 884 /  4 802 / 15 657 /   425 /  17
    gray G2S-hybrid  0.000 / 0.000            0.000   (c: 27 315 photons, opacity_model = none)
    f: a threshold pair for 1.000 of the photons of all five use_ddmc rows; with every 5th photon on one
       F2S-hybrid: 2 998 on e_lo, 2 998 on e_hi, census 3 235, absorbed 28 363, escaped 533;
       F3S-hybrid: 3 007 on e_lo, 3 006 on e_hi, census 3 107, absorbed 24 496, escaped 3 096
    (escaped is the real count on every row: each has an open face, the 1-D rows one)

* a: share of the surviving photons that differ after one cycle (emission off) when sie and u are the pattern moved by
  one cell along that axis while rho and the starting swarm stay: the temperature counts in tracking itself, not only
  through the sourced photons.  b: the same when every photon tracks with its neighbour's frequency, in an attribute
  other than ``e``.  Both at least 0.05, the project's discrimination bound.
* c: the control that states the gap.  The gray deck (opacity_model = none) on the same mesh and state gives exactly
  0.000 for both: no gray case can see the per-event temperature gather or a stale frequency.
* d: at the first transport call of a ``use_ddmc`` row the share of the photons with ``dx_push (sigma_a(e) + sigma_s) >
  tau_ddmc`` lies in [0.2, 0.8] and at least 25 % of the occupied cells hold photons of both regimes.
* e: census, absorbed and escaped of the first cycle are each at least 256 -- escaped too on the 1-D rows, whose one open
  face is reached by enough photons; no row is all-periodic -- and the photons at the call force the lane reuse of the
  row's grid caps.
* f: the threshold frequencies e_lo (DDMC) < e_hi (not), neighbouring doubles, exist for the starting cell of every
  photon of every ``use_ddmc`` row, and a cycle with every 5th photon placed on one (more than 256 on each side) keeps
  the floors of e on the two rows the GPU file runs that way.

These are conditions, not measurements: a row that falls under a bound gets other scales.
"""
import numpy as np
import pytest

import axis_cases as ax
import freq_cases as fc
import hetero_states as hs
import lane_reuse_cases as lr
from helpers import load_deck, run_oracle_cycles

BOUND = 0.05
NO_EMISSION = {"jaybenne/do_emission": "false"}
IDS = [c.id for c in fc.CASES]
DDMC_IDS = [c.id for c in fc.DDMC_CASES]
THRESHOLD_ROWS = ("F2S-hybrid", "F3S-hybrid")        # the rows of test_gpu_freq's threshold runs


def _ndim(case):
    return len(ax.GEOMETRIES[case.geom].nx)


def test_the_table_covers_what_it_says():
    every, in_3d = fc.kinds_seen()
    assert all(every[d] == {ax.R, ax.O, ax.P} for d in range(3)), every
    assert len(in_3d[1]) >= 2 and len(in_3d[2]) >= 2, in_3d
    have = {(c.geom, c.ddmc) for c in fc.CASES}
    assert {("G1", False), ("G1", True), ("G3U", False), ("G3S", False), ("G2S", True), ("G3S", True)} <= have
    assert ("G2O", True) in have or ("G3O", True) in have
    for c in fc.CASES:
        pin = load_deck(c.deck, fc.overrides(c))
        assert pin.GetString("mcblock", "opacity_model") == "ep_bremss"
        assert pin.GetOrAddBoolean("jaybenne", "use_ddmc", False) == c.ddmc
        assert pin.GetOrAddBoolean("jaybenne", "do_emission", True) and not pin.GetOrAddBoolean("jaybenne", "do_feedback", True)
        assert 6000 <= c.photons <= 30000


@pytest.mark.parametrize("geom", ["G1", "G2S", "G3S"])
def test_the_new_pattern_varies_both_factors_in_every_cell(geom):
    mesh = ax.mesh_of(geom)
    for b in (0, mesh.nblocks - 1):
        fr, fs = hs.rho_factor(mesh, None, fc.PATTERN, b)
        assert np.array_equal(fr, hs.rho_factor(mesh, None, "smooth", b)[0])
        sl = tuple(mesh.interior()[1:])
        assert len(np.unique(fs[sl])) == fs[sl].size and len(np.unique(fr[sl])) == fr[sl].size
        assert 0.5 <= fs.min() and fs.max() <= 1.5 and fs[sl].max() - fs[sl].min() > 0.5


# ------------------------------------------------------------------------------------------------ a, b, c
def _twins(deck, ov, pattern):
    """Two oracles from the same state with the same starting swarm."""
    A, mesh, pkg = hs.oracle_on(deck, ov, pattern, capacity_factor=fc.CAPACITY_FACTOR)
    B, _, _ = hs.oracle_on(deck, ov, pattern, capacity_factor=fc.CAPACITY_FACTOR)
    assert A.n == B.n and all(np.array_equal(A.sw[k][:A.n], B.sw[k][:B.n]) for k in A.sw)
    return load_deck(deck, ov), A, B, mesh, pkg


def _temperature_shift(deck, ov, pattern, d):
    """Share of the photons that differ when tracking reads the temperature of the pattern one cell along axis d."""
    pin, A, B, mesh, pkg = _twins(deck, ov, pattern)
    shift = [0, 0, 0]
    shift[d] = 1
    moved = hs.initial_state(mesh, pkg, pattern, shift=shift)
    assert not np.array_equal(moved["sie"], B.fields["sie"])
    B.fields["sie"][...] = moved["sie"]
    B.fields["u"][...] = B.fields["rho"] * moved["sie"]
    assert np.array_equal(A.fields["rho"], B.fields["rho"])
    run_oracle_cycles(A, pin, 1)
    run_oracle_cycles(B, pin, 1)
    return hs.differing_photons(A, B), A.n


def _neighbours_frequency(deck, ov, pattern):
    """Share of the photons that differ, in an attribute other than e, when each tracks with its neighbour's e."""
    pin, A, B, mesh, pkg = _twins(deck, ov, pattern)
    n = B.n
    B.sw["e"][:n] = np.roll(B.sw["e"][:n], 1)
    assert np.mean(A.sw["e"][:n] != B.sw["e"][:n]) > 0.99
    run_oracle_cycles(A, pin, 1)
    run_oracle_cycles(B, pin, 1)
    return hs.differing_photons(A, B, skip=("e",)), A.n


@pytest.mark.parametrize("cid", IDS)
def test_a_the_temperature_counts_in_tracking(cid):
    case = fc.BY_ID[cid]
    for d in range(_ndim(case)):
        frac, n = _temperature_shift(case.deck, fc.overrides(case, **NO_EMISSION), fc.PATTERN, d)
        print(f"{cid}: sie moved one cell along x{d + 1} changes {frac:.3f} of {n} photons")
        assert frac >= BOUND, (cid, d, frac)


@pytest.mark.parametrize("cid", IDS)
def test_b_the_frequency_counts(cid):
    case = fc.BY_ID[cid]
    frac, n = _neighbours_frequency(case.deck, fc.overrides(case, **NO_EMISSION), fc.PATTERN)
    print(f"{cid}: the neighbour's frequency changes {frac:.3f} of {n} photons")
    assert frac >= BOUND, (cid, frac)


def test_c_gray_opacities_see_neither():
    """The control: on the gray deck every per-event opacity is rho kappa_a and (rho / apm) kappa_s (the oracle evaluates
    its models at every event, as the device does under JB_PER_EVENT_OPACITY=1), so both give exactly nothing."""
    case = fc.GRAY_CONTROL
    ov = ax.overrides(case, "S1")
    pin = load_deck(case.deck, ov)
    assert pin.GetString("mcblock", "opacity_model") == "none" and not pin.GetOrAddBoolean("jaybenne", "do_emission", True)
    for d in range(2):
        frac, n = _temperature_shift(case.deck, ov, fc.PATTERN, d)
        print(f"gray {case.id}: sie moved one cell along x{d + 1} changes {frac:.3f} of {n} photons")
        assert frac == 0.0
    frac, n = _neighbours_frequency(case.deck, ov, fc.PATTERN)
    print(f"gray {case.id}: the neighbour's frequency changes {frac:.3f} of {n} photons")
    assert frac == 0.0 and n > 1000


# ------------------------------------------------------------------------------------------------ d, e
@pytest.mark.parametrize("cid", IDS)
def test_d_e_regimes_mix_through_frequency_and_every_outcome_is_common(cid):
    case = fc.BY_ID[cid]
    pin, O, mesh, pkg = fc.oracle_of(case)
    par = fc.model_params(pin, pkg)
    mix = fc.at_transport(O, lambda o: fc.regime_mix(o, mesh, par))
    log = lr.watch(O)
    run_oracle_cycles(O, pin, 1)
    out = lr.outcomes(log)
    print(f"{cid} {case.bset}: {out['live']} at the transport call, census {out['n_census']}, absorbed {out['n_absorbed']}, "
          f"escaped {out['n_escaped']}, {O.events / out['live']:.0f} events per photon")
    for k in ("n_census", "n_absorbed", "n_escaped"):
        assert out[k] >= lr.FLOOR, (k, out)
    for G in case.grids:
        assert out["live"] >= lr.reuse_floor(G) and O.cap >= out["live"], (G, out)
    assert O.events >= 10 * out["live"]                 # histories, not single events
    assert bool(par["use_ddmc"]) == case.ddmc
    if case.ddmc:
        share, mixed = mix[0]
        print(f"{cid}: {share:.2f} of the photons start on the DDMC side, {mixed:.2f} of the occupied cells hold both regimes")
        assert 0.2 <= share <= 0.8, share
        assert mixed >= 0.25, mixed
    if case.cycles == 2:                                # the second cycle of the GPU runs has photons to follow
        assert out["n_census"] >= lr.FLOOR


# ------------------------------------------------------------------------------------------------ f
@pytest.mark.parametrize("cid", DDMC_IDS)
def test_f_threshold_frequencies_exist(cid):
    case = fc.BY_ID[cid]
    pin, O, mesh, pkg = fc.oracle_of(case)
    par = fc.model_params(pin, pkg)
    rho, temp, dx_push, _ = fc.cell_inputs(O, mesh, par)
    e_lo, e_hi, found = fc.threshold_frequencies(par, rho, temp, dx_push)
    print(f"{cid}: threshold pair found for {found.mean():.3f} of {O.n} photons; e_lo from {e_lo.min():.3e} to {e_lo.max():.3e}")
    assert found.all()
    assert np.all(np.nextafter(e_lo, np.inf) == e_hi)
    assert fc.is_ddmc(par, rho, temp, dx_push, e_lo).all() and not fc.is_ddmc(par, rho, temp, dx_push, e_hi).any()
    if cid not in THRESHOLD_ROWS:
        return
    e, low, high = fc.on_the_threshold(O, mesh, par)
    O.sw["e"][:O.n] = e
    log = lr.watch(O)
    run_oracle_cycles(O, pin, 1)
    out = lr.outcomes(log)
    print(f"{cid}: {int(low.sum())} photons on e_lo, {int(high.sum())} on e_hi; census {out['n_census']}, absorbed "
          f"{out['n_absorbed']}, escaped {out['n_escaped']}")
    assert low.sum() > lr.FLOOR and high.sum() > lr.FLOOR
    for k in ("n_census", "n_absorbed", "n_escaped"):
        assert out[k] >= lr.FLOOR, (k, out)
