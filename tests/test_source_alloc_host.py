"""Energy-proportional source allocation (include/jaybenne_amd.h: jb_set_source_allocation) without a GPU: the deck
key and the environment default, the reference's own ``source_strategy = energy`` still rejected, and the properties
of tests/source_alloc_model.py that the GPU tests then hold the library to bit for bit -- the block sum's error
bound, E_tot independent of the partition, exact unbiasedness of the count, and the photon total."""
import math
import types
from fractions import Fraction

import numpy as np
import pytest

import axis_cases as ax
import hetero_states as hs
import source_alloc_model as sam
from helpers import load_deck
from jaybenne_amd import mcblock
from jaybenne_amd._lib import ALLOC_ENERGY, ALLOC_UNIFORM  # noqa: F401  (the mode's symbols: without it nothing here runs)

KEY = "jaybenne_amd/source_allocation"
U = 2.0 ** -53


# ---- the deck key and the environment ----------------------------------------------------------------------
@pytest.mark.parametrize("value,want", [(None, None), ("uniform", "uniform"), ("energy", "energy")])
def test_deck_key(value, want, monkeypatch):
    from jaybenne_amd import _lib, jaybenne as jb
    monkeypatch.delenv("JB_SOURCE_ALLOCATION", raising=False)
    pin = load_deck("stepdiff", {} if value is None else {KEY: value})
    assert mcblock.deck_source_allocation(pin) == want
    assert mcblock.source_allocation_of(pin) == (want or "uniform")
    if want:
        assert jb.source_allocation_code(want) == {"uniform": _lib.ALLOC_UNIFORM, "energy": _lib.ALLOC_ENERGY}[want]
    assert (_lib.ALLOC_UNIFORM, _lib.ALLOC_ENERGY) == (0, 1) and jb.SOURCE_ALLOCATIONS == ("uniform", "energy")


@pytest.mark.parametrize("value", ["Energy", "proportional", "1"])
def test_deck_key_bad_value(value):
    from jaybenne_amd import jaybenne as jb
    with pytest.raises(ValueError, match="jaybenne_amd/source_allocation"):
        mcblock.deck_source_allocation(load_deck("stepdiff", {KEY: value}))
    with pytest.raises(ValueError, match="source_allocation"):
        jb.source_allocation_code(value)


def test_environment_default(monkeypatch):
    """JB_SOURCE_ALLOCATION=energy (exactly that value, as jb_initialize compares it) is the default of a deck without
    the key; the key wins."""
    plain = load_deck("stepdiff")
    monkeypatch.setenv("JB_SOURCE_ALLOCATION", "energy")
    assert mcblock.deck_source_allocation(plain) is None and mcblock.source_allocation_of(plain) == "energy"
    assert mcblock.source_allocation_of(load_deck("stepdiff", {KEY: "uniform"})) == "uniform"
    for other in ("ENERGY", "1", "uniform", ""):
        monkeypatch.setenv("JB_SOURCE_ALLOCATION", other)
        assert mcblock.source_allocation_of(plain) == "uniform"
        assert mcblock.source_allocation_of(load_deck("stepdiff", {KEY: "energy"})) == "energy"


def test_reference_strategy_energy_is_still_rejected():
    """<jaybenne> source_strategy = energy is the reference's declared, unimplemented strategy (sourcing.cpp:38):
    SourcePhotons rejects it before it looks at anything else, whatever <jaybenne_amd> source_allocation says."""
    from jaybenne_amd import jaybenne as jb
    for extra in ({}, {KEY: "energy"}):
        pin = load_deck("stepdiff", dict({"jaybenne/source_strategy": "energy"}, **extra))
        assert pin.GetOrAddString("jaybenne", "source_strategy", "uniform") == "energy"
        assert mcblock.deck_source_allocation(pin) == extra.get(KEY)          # the two keys do not read each other
        md = types.SimpleNamespace(pkg=types.SimpleNamespace(Param=lambda k: {"source_strategy": jb.SourceStrategy.energy}[k]))
        with pytest.raises(NotImplementedError, match="Energy source strategy"):
            jb.SourcePhotons(md, jb.SourceType.thermal, 0.0, 0.0)


# ---- 1. the block sum ----------------------------------------------------------------------------------------
def _addends(kind, L, seed):
    r = np.random.default_rng(seed)
    if kind == "wide":                    # 40 decades, like the energies of a mesh with a hot and a cold half
        return r.random(L) * 10.0 ** r.integers(-20, 20, L)
    if kind == "signed":
        return (r.random(L) - 0.5) * 10.0 ** r.integers(-3, 3, L)
    return r.random(L)


@pytest.mark.parametrize("L", [1, 50, 255, 256, 257, 513, 4099, 32768])
@pytest.mark.parametrize("kind", ["flat", "wide", "signed"])
def test_block_sum_within_its_bound_of_fsum(L, kind):
    a = _addends(kind, L, 1000 + L)
    got, want = sam.block_sum(a), math.fsum(a)
    assert abs(got - want) <= (L + 1) * U * math.fsum(np.abs(a)), (got, want)


def test_block_sum_is_the_stated_order():
    """Restated with Python floats, thread by thread; and another order gives other bits on the same addends."""
    a = _addends("wide", 1300, 7)
    s = [0.0] * 256
    for t in range(256):
        for cell in range(t, len(a), 256):
            s[t] = s[t] + float(a[cell])
    d = 128
    while d >= 1:
        for t in range(d):
            s[t] = s[t] + s[t + d]
        d //= 2
    assert sam.block_sum(a) == s[0]
    seq = 0.0
    for v in a:
        seq += float(v)
    assert seq != s[0]
    assert sam.block_sum(np.zeros(10)) == 0.0 and math.copysign(1.0, sam.block_sum(np.zeros(10))) == 1.0
    assert sam.block_sum(np.array([])) == 0.0


# ---- 2. the total ----------------------------------------------------------------------------------------------
def _mesh_call(n_target=20000, source_type=sam.THERMAL, blocks=None):
    pin = load_deck("stepdiff_smr", ax.geometry_overrides("G2S", ax.BOUNDARY_SETS["S1"][:4] + (ax.P,) * 2))
    mesh = ax.mesh_of("G2S")
    mcb = mcblock.Initialize(pin)
    ic = hs.initial_state(mesh, mcb, "hot_spots")
    par = dict(cv=mcb.eos.cv, sb=mcb.opacity.sb, c=mcb.opacity.c, kappa=mcb.opacity.kappa or 5.0,     # (the deck has no absorption)
               seed=pin.GetOrAddInteger("jaybenne", "seed", 123))
    rows = slice(None) if blocks is None else np.asarray(blocks)
    fleck = np.full_like(ic["rho"], 0.75)
    call = sam.source_call(mesh, ic["rho"][rows], ic["sie"][rows], fleck[rows], par, source_type, 1.0e-11, n_target, 3,
                           blocks=blocks)
    return mesh, par, ic, call


def test_total_has_the_same_bits_for_every_partition():
    mesh, par, ic, whole = _mesh_call()
    assert mesh.nblocks >= 10 and len({mesh.cell_volume(b) for b in range(mesh.nblocks)}) == 2
    e = np.array([whole.e_block[b] for b in range(mesh.nblocks)])
    assert len(set(e.tolist())) == mesh.nblocks            # every block sums to something else
    want = sam.total(e)
    for nranks in (1, 2, 5):
        for owner in (np.arange(mesh.nblocks) % nranks, np.arange(mesh.nblocks) * nranks // mesh.nblocks,
                      np.random.default_rng(nranks).integers(0, nranks, mesh.nblocks)):
            parts = []
            for r in range(nranks):
                gids = np.nonzero(owner == r)[0]
                # each rank computes its own blocks' sums from its own rows
                _, _, _, mine = _mesh_call(blocks=gids) if len(gids) else (None, None, None, None)
                if len(gids):
                    parts.append((gids, [mine.e_block[int(g)] for g in gids]))
            got = sam.gather(parts, mesh.nblocks)
            assert np.array_equal(got.view(np.int64), e.view(np.int64))
            assert sam.total(got) == want
    # the order matters: on sums of like size (here two blocks hold the energy, the others 1e-20 of it) another order
    # gives other bits, so "the same bits" says something
    like = np.random.default_rng(3).random(mesh.nblocks) + 1.0
    assert any(sam.total(like[np.random.default_rng(s).permutation(mesh.nblocks)]) != sam.total(like) for s in range(20))
    assert (e > 1e-12 * e.max()).sum() == 2 and (e > 0.0).all()
    assert want == pytest.approx(math.fsum(e), rel=mesh.nblocks * U * 2)


# ---- 3. the count ----------------------------------------------------------------------------------------------
def _ulp_neighbourhood(x):
    return Fraction(float(np.nextafter(x, -np.inf))), Fraction(float(np.nextafter(x, np.inf)))


def p_up(frac):
    """P((nu - f) > xi) for the library's uniforms xi = (2 k + 1) 2^-53, k = 0 .. 2^52 - 1: the number of odd
    multiples of 2^-53 below frac, over 2^52."""
    m = Fraction(frac) * 2 ** 53             # xi < frac  <=>  2 k + 1 < m
    k_max = (math.ceil(m) - 1 - 1) // 2      # the largest k with 2 k + 1 <= ceil(m) - 1
    return Fraction(max(k_max + 1, 0), 2 ** 52)


def test_unbiasedness_is_exact():
    """Per cell, sum over the outcomes of P(n) n ew: with P(n = f + 1) = nu - f it is a convex combination of
    f ew_f and (f + 1) ew_(f+1), each of which is erad or a neighbouring double (f >= 1); for f = 0 it is
    nu (erad / nu), one rounding from erad.  And the uniforms' grid realises that probability exactly wherever
    nu >= 1 (nu - f is then a multiple of 2^-52)."""
    r = np.random.default_rng(5)
    erad = np.concatenate([r.random(400) * 10.0 ** r.integers(-12, 6, 400), [1.0, 3.0, 1e-300]])
    for scale in (1.0, 7.3e3, 1.9e-4, 2.0 ** 20):
        nu = erad * scale
        f = np.floor(nu)
        for q in range(len(erad)):
            e, v, fl = float(erad[q]), float(nu[q]), float(f[q])
            p1 = Fraction(v) - Fraction(fl)
            assert 0 <= p1 < 1 and Fraction(v - fl) == p1          # nu - f is exact in floating point
            n_lo, ew_lo = sam.count_cells(np.array([e]), scale, np.array([1.0]))        # xi above every fraction: n = f
            n_hi, ew_hi = sam.count_cells(np.array([e]), scale, np.array([-1.0]))       # below every fraction: n = f + 1
            assert n_lo[0] == fl and n_hi[0] == fl + 1.0
            if fl >= 1.0:
                lo, hi = _ulp_neighbourhood(e)
                for n, ew in ((n_lo[0], ew_lo[0]), (n_hi[0], ew_hi[0])):
                    assert lo <= Fraction(float(n * ew)) <= hi                 # as the library multiplies them
                    assert lo <= Fraction(float(n)) * Fraction(float(ew)) <= hi
                mean = (1 - p1) * Fraction(fl) * Fraction(float(ew_lo[0])) + p1 * Fraction(fl + 1.0) * Fraction(float(ew_hi[0]))
                assert lo <= mean <= hi
                assert p_up(v - fl) == p1                                      # the grid gives exactly nu - f
            else:
                assert ew_lo[0] == 0.0 and n_lo[0] == 0.0
                if v > 0.0:
                    assert ew_hi[0] == e / v
                    mean = Fraction(v) * Fraction(float(ew_hi[0]))
                    assert abs(mean - Fraction(e)) <= Fraction(U) * Fraction(e)
                    assert abs(p_up(v) - p1) <= Fraction(1, 2 ** 53)
    # nothing below the smallest uniform 2^-53 is ever rounded up; an exact integer never is either
    assert p_up(4e-18) == 0 and p_up(2.0 ** -53) == 0 and p_up(2.0 ** -52) == Fraction(1, 2 ** 52) and p_up(0.0) == 0


def test_counts_add_up_to_the_target():
    for n_target, st in ((20000, sam.THERMAL), (777, sam.EMISSION), (3, sam.THERMAL)):
        mesh, par, ic, call = _mesh_call(n_target, st)
        _counts_add_up(mesh, call, n_target)


def test_epbremss_emission_on_the_3d_two_level_row():
    """The emission source of tests/freq_cases.py's F3S-hybrid row (EPBremss, rho and sie different in every cell, dv
    different by level) under source_allocation = energy: the model's emissivity (E (rho rho)) sqrt(T) is the
    oracle's ``opac_emissivity`` bit for bit, erad = ((fleck j) dv) dt with the oracle's Fleck factor, and the counts
    add up as they do for the gray form."""
    import freq_cases as fc
    from oracle import orc
    case = fc.BY_ID["F3S-hybrid"]
    pin, O, mesh, mcb = fc.oracle_of(case, **{KEY: "energy"})
    assert mcblock.source_allocation_of(pin) == "energy" and mcb.opacity.model == mcblock.OPAC_EPBREMSS
    assert mesh.ndim == 3 and set(mesh.blk_level) == {0, 1}
    par_o = fc.model_params(pin, mcb)
    dt = pin.GetReal("jaybenne", "dt")
    O.UpdateDerivedTransportFields(dt)
    par = dict(cv=mcb.eos.cv, sb=mcb.opacity.sb, c=mcb.opacity.c, kappa=mcb.opacity.kappa, ep_E=par_o["ep_E"],
               seed=pin.GetOrAddInteger("jaybenne", "seed", 123))
    assert par["kappa"] == 0.0 and par["ep_E"] > 0.0
    call = sam.source_call(mesh, O.fields["rho"], O.fields["sie"], O.fields["fleck"], par, sam.EMISSION, dt, case.photons, 1)
    sl = mesh.interior()[1:]
    orc.set_math_mode(orc.MATH_PORTABLE)
    for b in range(mesh.nblocks):
        rho, fleck = O.fields["rho"][b][sl], O.fields["fleck"][b][sl]
        temp = sam.temperature(O.fields["sie"][b][sl], par["cv"])
        j = orc.model_eval(par_o, 1, rho, temp, np.ones_like(rho)).reshape(rho.shape)
        dv = (mesh.blk_dx[b, 0] * mesh.blk_dx[b, 1]) * mesh.blk_dx[b, 2]
        assert np.array_equal(call.erad[b], ((fleck * j) * dv) * dt), b
    f = O.fields["fleck"][mesh.interior()]
    assert len(np.unique(f)) > 0.4 * f.size and 0.0 < f.min() and f.max() <= 1.0
    n = _counts_add_up(mesh, call, case.photons)
    print(f"EPBremss emission on {case.id}: E_tot {call.e_total:.6e}, {int(n.sum())} photons for a target of {case.photons}, "
          f"{int((n == 0).sum())} cells without one, {int((n >= 2).sum())} with several")
    assert (n >= 2).any() and (n == 0).any()


def _counts_add_up(mesh, call, n_target):
    """The assertions on one whole call: sum nu = N, the counts, the carried energy, the prefix."""
    erad = np.concatenate([call.erad[b].reshape(-1) for b in range(mesh.nblocks)])
    n = np.concatenate([call.n[b].reshape(-1) for b in range(mesh.nblocks)])
    ew = np.concatenate([call.ew[b].reshape(-1) for b in range(mesh.nblocks)])
    nu = erad * call.scale
    sourcing = int((erad > 0.0).sum())
    assert sourcing == erad.size
    # sum nu = N to rounding: each nu carries one rounding of the product and scale one of the quotient, E_tot
    # the roundings of its two-stage sum
    assert abs(math.fsum(nu) - n_target) <= n_target * U * (mesh.ncell + mesh.nblocks + 4)
    assert abs(int(n.sum()) - n_target) <= sourcing
    assert np.all(np.abs(n - nu) < 1.0) and sum(call.nper.values()) == int(n.sum())
    # every cell with f >= 1 carries its energy exactly (to the neighbouring double)
    full = np.floor(nu) >= 1.0
    assert np.all(np.abs(n[full] * ew[full] - erad[full]) <= np.spacing(erad[full]))
    for b in range(mesh.nblocks):
        cnt = np.rint(call.n[b].reshape(-1)).astype(np.int64)
        assert np.array_equal(call.prefix[b], np.cumsum(cnt) - cnt) and call.nper[b] == cnt.sum()
        for p in (0, call.nper[b] // 2, call.nper[b] - 1):
            if call.nper[b]:
                cell = sam.cell_of(call.prefix[b], p)
                assert call.prefix[b][cell] <= p < call.prefix[b][cell] + cnt[cell]
    return n


def test_nothing_to_source_and_bad_totals():
    assert sam.scale_of(1000, 0.0) == 0.0
    n, ew = sam.count_cells(np.zeros(5), 0.0, np.full(5, 2.0 ** -53))
    assert not n.any() and not ew.any()
    for bad in (math.inf, math.nan, -1.0):
        with pytest.raises(ValueError):
            sam.scale_of(1000, bad)
    with pytest.raises(ValueError):
        sam.scale_of(10 ** 9, 5e-324)                    # N / E_tot overflows
    sam.check_target(2 ** 31 - 1 - 128, 128)
    with pytest.raises(ValueError):
        sam.check_target(2 ** 31 - 128, 128)
    # energy_delta: one product, zero for the thermal source and with set_energy_delta = 0
    n, ew = np.array([3.0, 0.0, 1.0]), np.array([0.5, 0.0, 2.0])
    assert np.array_equal(sam.energy_delta(n, ew, sam.EMISSION), [-1.5, 0.0, -2.0])
    assert not sam.energy_delta(n, ew, sam.THERMAL).any() and not sam.energy_delta(n, ew, sam.EMISSION, False).any()
