"""Radiation moments on the CPU (tests/moments_model.py: a numpy restatement of include/jaybenne_amd.h,
jb_evaluate_radiation_moments): the model's sums against exact rational sums, its independence of where a cell lies
in the swarm, counts that show the crafted swarms of tests/test_gpu_moments.py hold what they claim, and what the
quantities rest on in the CPU oracle's census -- the cell of the position is (ip, jp, kp), |v| = c, and the domain's
first and second angular moments are those of an isotropic field within their statistical error."""
import math
from fractions import Fraction

import numpy as np
import pytest

import moments_model as mm
import swarm_ops_model as som
from helpers import load_deck


@pytest.fixture(scope="module")
def geoms():
    return {name: som.host_view(case)[1] for name, case in mm.mesh_cases().items()}


# ---- the sums -----------------------------------------------------------------------------------------
def _addends(L, salt):
    ids = som._hash(np.arange(L), salt) >> np.uint64(1)
    sw = mm._physical({"id": ids}, salt)
    return mm.addends(sw, np.arange(L))


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 700, 4096, 4097, 2 * 4096 + 1])
def test_model_sums_lie_within_the_bound_of_any_summation_order(L):
    """|model - exact| <= (L + 1) 2^-53 sum |a| per component: (L - 1) 2^-53 sum |a| bounds any order of L - 1
    additions to first order, and the addends are themselves rounded products."""
    a = _addends(L, 31 + L)
    got = mm.run_sum(a)
    exact, mag = mm.exact_sum(a)
    for q in range(mm.SUMS):
        err = abs(Fraction(float(got[q])) - exact[q])
        assert err <= (L + 1) * Fraction(1, 2 ** 53) * mag[q], (L, q, float(err), float(mag[q]))


def test_summation_order_shows_in_the_bits():
    """the crafted addends are such that another order gives other bits: a plain left-to-right sum differs"""
    a = _addends(4097, 5)
    assert not mm.same_bits(mm.run_sum(a), np.add.accumulate(a, axis=0)[-1])
    assert not mm.same_bits(mm.run_sum(a), a.sum(axis=0))


def test_short_runs_equal_a_narrower_tree():
    """a run of L <= G slots summed by G lanes (joins d = G/2 .. 1) has the bits of the 64-lane tree, for every
    power of two G >= L: what lets the kernel take short runs with small groups"""
    for L in (1, 2, 3, 4, 7, 8, 31, 32, 33, 64):
        a = _addends(L, 77 + L)
        want = mm.chunk_sum(a)
        G = 1
        while G <= 64:
            if G >= L:
                s = np.zeros((G, mm.SUMS))
                s[:L] = s[:L] + a
                d = G // 2
                while d:
                    s[:d] = s[:d] + s[d:2 * d]
                    d //= 2
                assert mm.same_bits(s[0], want), (L, G)
            G *= 2


def test_a_cell_does_not_depend_on_what_lies_before_it(geoms):
    """prepending photons in earlier cells -- any number: the later cells start at other slots, other lane offsets,
    other chunk phases -- changes no bit of a later cell"""
    g = geoms["1d"]
    lengths = [65, 4097, 1, 2 * 4096 + 1, 64]
    sw, cells = mm.run_swarm(g, lengths, extras=0)
    sw = mm.canonical(g, sw, len(sw["id"]))
    base, _ = mm.moments(g, sw, len(sw["id"]))
    assert cells[0] >= 3
    for extra in (1, 63, 64, 1000, 4095):
        more, _ = mm.run_swarm(g, [extra], salt=mm.SALT + extra, extras=0, first_cell=1)
        both = {k: np.concatenate((more[k], sw[k])) for k in som.KEYS}
        both = mm.canonical(g, both, len(both["id"]))
        got, _ = mm.moments(g, both, len(both["id"]))
        flat_b, flat_g = base.reshape(mm.MOMENTS, -1), got.reshape(mm.MOMENTS, -1)
        assert mm.same_bits(flat_b[:, cells], flat_g[:, cells]), extra
        assert flat_g[0, 1] == extra and flat_b[0, 1] == 0


# ---- the crafted swarms hold what they claim ---------------------------------------------------------------
def test_run_plans_start_every_length_at_every_lane_offset(geoms):
    seen = {}
    for name, mesh, lengths in mm.run_plans():
        g = geoms[mesh]
        sw, cells = mm.run_swarm(g, lengths)
        n = len(sw["id"])
        assert n <= mm.MAX_SLOTS
        assert not mm.in_order(g, sw, n), name                            # given unsorted
        srt = mm.canonical(g, sw, n)
        key = som.sort_key(g, srt, n)
        counted = key < g.nkeys
        assert int((~counted).sum()) == mm.EXTRAS
        for L, offs in som.run_starts(key[counted]).items():
            seen.setdefault(L, set()).update(offs)
        fields, rep = mm.moments(g, srt, n)
        assert rep["n_counted"] == sum(lengths) and rep["n_skipped"] == mm.EXTRAS
        assert rep["cells_nonempty"] == len([m for m in lengths if m]) and rep["longest_run"] == max(lengths)
        flat = fields[0].reshape(-1)
        assert np.array_equal(flat[cells], np.asarray(lengths, dtype=np.float64))
        if len(lengths) > 1:
            assert np.all(flat[cells[1:] - 1] == 0)                       # empty cells between the runs
        # statuses are mixed, and some ACTIVE slots carry a bad blk
        st, blk = sw["status"], sw["blk"]
        assert set(st.tolist()) == {0, 1, 2, 3, 4}
        assert int(((st == som.ST_ACTIVE) & ((blk < 0) | (blk >= g.nblocks))).sum()) >= 10
    for L in mm.SHORT + mm.LONG:
        assert seen[L] == set(range(64)), (L, sorted(set(range(64)) - seen[L]))
    assert mm.ONE_CELL in seen


def test_crafted_values_span_what_they_claim(geoms):
    g = geoms["3d"]
    sw = mm.hashed_swarm(g, 6000)
    w = sw["w"]
    assert np.all(w > 0) and math.log2(w.max() / w.min()) > 59
    for k in ("vx", "vy", "vz"):
        assert (sw[k] > 0).sum() > 2000 and (sw[k] < 0).sum() > 2000
    # photons clamped into ghost cells, photons of bad blks: not counted
    srt = mm.canonical(g, sw, 6000)
    key = som.sort_key(g, srt, 6000)
    _, _, inside = mm.cell_of_key(g, key[key < g.nkeys])
    assert (~inside).sum() > 500
    _, rep = mm.moments(g, srt, 6000)
    assert rep["n_counted"] == int(inside.sum()) and rep["n_skipped"] == 6000 - rep["n_counted"]
    # the meshes: two levels (block widths differ), no two axes alike
    assert len({tuple(r) for r in g.dx.tolist()}) >= 2 and len(set(g.nx)) == 3
    g2 = geoms["2d"]
    assert len({tuple(r) for r in g2.dx.tolist()}) >= 2 and g2.nx[0] != g2.nx[1]


def test_halo_copies_get_zeros():
    _, g = som.host_view(som.RANK_MESH, 1, 2)
    assert g.nowned < g.nblocks
    sw = mm.canonical(g, mm.hashed_swarm(g, 3000), 3000)
    assert int(((sw["status"] == som.ST_ACTIVE) & (sw["blk"] >= g.nowned) & (sw["blk"] < g.nblocks)).sum()) > 10
    fields, rep = mm.moments(g, sw, 3000)
    assert not fields[:, g.nowned:].any() and fields[0, :g.nowned].sum() == rep["n_counted"] > 500


# ---- what the quantities rest on: the oracle's census ------------------------------------------------------------
@pytest.mark.parametrize("deck", ["inf", "stepdiff", "stepdiff_ddmc"])
def test_oracle_census_is_isotropic_within_its_error(deck):
    """Two cycles at 20000 photons.  Measured on the CPU oracle for these decks: no photon whose position's cell is
    not (ip, jp, kp); |v|^2 / c^2 within 7e-16 of 1; first moments at most 2.0 sigma, second moments at most 1.6."""
    from jaybenne_amd.constants import SPEED_OF_LIGHT as c
    from oracle import orc
    from oracle.harness import make_oracle, run_oracle_cycles
    pin = load_deck(deck, {"jaybenne/num_particles": 20000})
    O, mesh, _ = make_oracle(pin, orc.MATH_LIBM, threads=8, capacity_factor=4.0)
    run_oracle_cycles(O, pin, 2)
    n = O.n
    sw = {k: np.asarray(O.sw[k][:n]) for k in som.F64 + som.I32}
    g = som.Geom(mesh, np.arange(mesh.nblocks))
    act = sw["status"] == som.ST_ACTIVE
    assert act.sum() > 10000
    raw = som.raw_cell_index(g, sw, n)
    for d, name in enumerate(("ip", "jp", "kp")):
        assert int((act & (raw[d] != sw[name])).sum()) == 0, name
    print(deck, "moments", end=" ")
    assert domain_isotropy(sw, act, c, report=True)


def domain_isotropy(sw, act, c, report=False):
    """|v|^2 / c^2 within 1e-14 of 1; sum w v_d / (c sum w) within 6 sigma of 0 and sum w v_d^2 / (c^2 sum w) within 6
    sigma of 1/3, with sigma = sqrt(1 / (3 N_eff)) and sqrt(4 / (45 N_eff)): the variances of mu and mu^2 of an
    isotropic direction, over N_eff = (sum w)^2 / sum w^2 equal-weight photons"""
    w = sw["w"][act]
    v = [sw[k][act] for k in ("vx", "vy", "vz")]
    speed = (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) / (c * c)
    ok = bool(np.all(np.abs(speed - 1.0) <= 1e-14))
    W = math.fsum(w)
    neff = W * W / math.fsum(w * w)
    s1, s2 = math.sqrt(1.0 / (3.0 * neff)), math.sqrt(4.0 / (45.0 * neff))
    for d in range(3):
        m1 = math.fsum(w * v[d]) / (c * W)
        m2 = math.fsum(w * v[d] * v[d]) / (c * c * W)
        if report:
            print(f"axis {d}: first {m1 / s1:+.2f} sigma, second {(m2 - 1 / 3) / s2:+.2f} sigma", end="; ")
        ok = ok and abs(m1) <= 6.0 * s1 and abs(m2 - 1.0 / 3.0) <= 6.0 * s2
    if report:
        print(f"N_eff {neff:.0f}, max | |v|^2/c^2 - 1 | {float(np.abs(speed - 1).max()):.1e}")
    return ok
