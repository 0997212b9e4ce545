"""The census comb's rule on the CPU (tests/comb_model.py: a numpy restatement of include/jaybenne_amd.h,
jb_comb_census_plan): its properties, and the acceptance run -- the CPU oracle's stepdiff with four times the
photons, combed back to a quarter after every cycle, against the reference's own gate."""
import math

import numpy as np
import pytest

import comb_model as cm
from helpers import load_deck


def _weights(m, decades, salt):
    rng = np.random.default_rng(salt)
    return 10.0 ** (decades * rng.random(m))


@pytest.mark.parametrize("K", [1, 7, 100, 400])
@pytest.mark.parametrize("decades", [0.0, 3.0])
def test_counts_sum_to_K_and_stay_within_floor_ceil(K, decades):
    w = _weights(400, decades, 11 + K)
    for xi in (1e-12, 0.25, 0.5, 0.999999, cm.u52_to_double(0), cm.u52_to_double((1 << 52) - 1)):
        k, delta = cm.comb_counts(w, K, xi)
        assert k.sum() == K and k.min() >= 0
        assert delta == np.cumsum(w)[-1] / K
        # floor(w / D) <= k <= ceil(w / D); one part in 1e12 of slack for the rounding of the running sums
        r = w / delta
        assert np.all(k >= np.floor(r * (1 - 1e-12))) and np.all(k <= np.ceil(r * (1 + 1e-12)))
        assert math.isclose(k.sum() * delta, math.fsum(w), rel_tol=1e-13)


def test_one_photon_with_nearly_all_the_weight():
    w = np.full(50, 1.0)
    w[17] = 999.0 * 49.0        # 99.9 % of W
    k, _ = cm.comb_counts(w, 10, 0.3)
    assert k.sum() == 10 and k[17] >= 9


def test_unbiased_over_xi():
    """E[k_j] = w_j / D: over N equidistant xi the mean of k_j is within 1 / N of it (k_j, as a function of xi, is
    a step between floor and ceil with one jump)."""
    w = _weights(60, 3.0, 5)
    K, N = 13, 20000
    total = np.zeros(len(w))
    for q in range(N):
        k, delta = cm.comb_counts(w, K, (q + 0.5) / N)
        total += k
    assert np.all(np.abs(total / N - w / delta) <= 2.0 / N)


def test_xi_is_keyed_by_epoch_block_and_cell():
    seen = {cm.xi_of(123, e, g, c) for e in (1, 2) for g in (0, 5) for c in (0, 77)}
    assert len(seen) == 8 and all(0.0 < x < 1.0 for x in seen)
    assert cm.xi_of(123, 3, 4, 5) == cm.xi_of(123, 3, 4, 5) != cm.xi_of(124, 3, 4, 5)


def test_comb_swarm_ids_streams_and_untouched_cells():
    from jaybenne_amd.mesh import Mesh
    from oracle import orc
    pin = load_deck("stepdiff", {"parthenon/mesh/nx1": 16, "parthenon/meshblock/nx1": 8})
    mesh = Mesh.from_deck(pin)
    gids = np.arange(mesh.nblocks)
    per_cell = [0, 1, 6, 7, 30, 0, 0, 12] + [3] * 7 + [25]
    n = sum(per_cell)
    rng = np.random.default_rng(3)
    cellx = np.repeat(np.arange(16), per_cell)
    sw = {k: np.zeros(n) for k in ("x", "y", "z", "vx", "vy", "vz", "t", "w", "e")}
    sw.update({k: np.zeros(n, dtype=np.int32) for k in ("ip", "jp", "kp", "blk", "status")})
    sw["x"] = -0.5 + (cellx + rng.random(n) * 0.9 + 0.05) / 16.0
    sw["w"] = 10.0 ** (3.0 * rng.random(n))
    sw["vx"] = rng.random(n)
    sw["blk"] = (cellx // 8).astype(np.int32)
    sw["id"] = np.arange(n, dtype=np.uint64) + np.uint64(100)
    sw["rng"] = np.arange(n, dtype=np.uint64) * np.uint64(977)
    perm = rng.permutation(n)
    sw = {k: v[perm] for k, v in sw.items()}
    T, K, seed, base = 6, 4, 349857, 5000
    out, info = cm.comb_swarm(mesh, gids, sw, n, T, K, seed, 3, base)
    combed = [c for c, m in enumerate(per_cell) if m > T]
    assert info["cells_combed"] == len(combed) == 4 and info["max_per_cell"] == 30
    assert info["n_after"] == n - sum(per_cell[c] - K for c in combed)
    key, _, _, _ = cm.cell_keys(mesh, gids, out, info["n_after"])
    assert np.all(np.diff(key) >= 0)
    by_id = {int(i): q for q, i in enumerate(sw["id"])}
    new = out["id"] >= np.uint64(base)
    assert sorted(out["id"][new].tolist()) == list(range(base, base + info["n_new_ids"]))
    assert np.all(np.diff(out["id"][new].astype(np.int64)) == 1)          # in output-slot order
    for q in np.flatnonzero(new):
        assert int(out["rng"][q]) == orc.stream_start(seed, int(out["id"][q]))
        assert out["x"][q] == out["x"][q - 1] and out["vx"][q] == out["vx"][q - 1]     # a copy of the slot before
    ck_in, _, _, _ = cm.cell_keys(mesh, gids, sw, n)
    for k in np.unique(key):
        sel_out, sel_in = key == k, ck_in == k
        assert math.isclose(math.fsum(out["w"][sel_out]), math.fsum(sw["w"][sel_in]), rel_tol=1e-13)
        if sel_in.sum() <= T:
            assert sel_out.sum() == sel_in.sum()
            for q in np.flatnonzero(sel_out):
                src = by_id[int(out["id"][q])]
                assert all(out[name][q] == sw[name][src] for name in cm.SWARM_KEYS)
        else:
            assert sel_out.sum() == K and len(set(out["w"][sel_out])) == 1


def test_trigger_of_the_deck_keys():
    from jaybenne_amd.jaybenne import comb_trigger_of
    assert comb_trigger_of(781, 2.0) == 1562 and comb_trigger_of(25, 1.0) == 25 and comb_trigger_of(3, 1.5) == 5
    assert comb_trigger_of(0, 2.0) == 0
    with pytest.raises(ValueError):
        comb_trigger_of(10, 0.5)


def test_stepdiff_acceptance_with_the_comb():
    """The oracle runs stepdiff at nx1 = 128 with 4e5 photons (3125 per cell); the model combs after every cycle with
    K = 781, T = 1562.  The run must pass the reference's gate (mean_frac_error_weighted <= 0.05; an uncombed run
    of 1e5 photons gives 0.025 .. 0.035) and end with 128 x 781 = 99 968 photons, its energy kept."""
    from jaybenne_amd.analysis import analytic_errors
    from oracle import orc
    from oracle.harness import make_oracle
    K, T = 781, 1562
    pin = load_deck("stepdiff", {"parthenon/mesh/nx1": 128, "parthenon/meshblock/nx1": 64,
                                 "jaybenne/num_particles": 400000})
    O, mesh, _ = make_oracle(pin, orc.MATH_LIBM, threads=16)
    seed = pin.GetOrAddInteger("jaybenne", "seed", 123)
    dt = pin.GetReal("jaybenne", "dt")
    gids = np.arange(mesh.nblocks)
    e0 = math.fsum(O.sw["w"][:O.n])
    assert O.n == 400000
    t, first_new = 0.0, None
    for _ in range(10):
        O.RadiationStep(t, dt)
        O.fields["sie"][...] = O.fields["u"] / O.fields["rho"]
        t += dt
        out, info = cm.comb_swarm(mesh, gids, O.sw, O.n, T, K, seed, O.cycle, O.next_id)
        if first_new is None:
            first_new = info["n_new_ids"]
            assert info["cells_combed"] == 128
        for name in cm.SWARM_KEYS:
            O.sw[name][:info["n_after"]] = out[name]
        O.n = info["n_after"]
        O.next_id += info["n_new_ids"]
    print("split copies in the first comb:", first_new)
    assert O.n == 99968
    assert math.isclose(math.fsum(O.sw["w"][:O.n]), e0, rel_tol=1e-12)
    assert len(np.unique(O.sw["id"][:O.n])) == O.n
    O.EvaluateRadiationEnergy()          # the tally of the combed census
    err = analytic_errors(mesh, O.fields["tally"], t)
    print("combed stepdiff:", err)
    assert err["mean_frac_error_weighted"] <= 0.05
