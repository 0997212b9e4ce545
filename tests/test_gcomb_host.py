"""The global census comb's rule on the CPU (tests/gcomb_model.py: a numpy restatement of include/jaybenne_amd.h,
jb_comb_census_weigh / _plan_global): its properties, the crafted swarms of tests/test_gpu_gcomb.py counted case by
case, and the acceptance run on the CPU oracle's stepdiff."""
import math

import numpy as np
import pytest

import axis_cases as ax
import comb_model as cm
import gcomb_cases as gc
import gcomb_model as gm
from helpers import load_deck

SEED, EPOCH, ID_BASE = 349857, 5, 1 << 33


def _ulp(x):
    return math.ulp(x)


def _run(geom, weights, r=gc.R_BAND, S=gc.S_MAX, exact=False, salt=5, N=None, pad=None):
    mesh = ax.mesh_of(geom)
    gids = np.arange(mesh.nblocks)
    sw, n_target, placed = gc.crafted(mesh, gids, salt, weights, pad)
    n = len(sw["w"])
    N = n_target if N is None else N
    if exact:
        import cell_order_model as om
        sw = om.canonical_sort(mesh, gids, sw, n)
    out, info = gm.gcomb_swarm(mesh, gids, np.ones(mesh.nblocks), sw, n, N, r, S, SEED, EPOCH, ID_BASE, exact=exact)
    return mesh, gids, sw, n, N, placed, out, info


def _check_cells(mesh, gids, sw, n, N, r, S, out, info):
    """The per-cell properties of the rule on any swarm."""
    key_in = info["key"]
    w_in = sw["w"][:n][info["order"]]
    key_out, _, nkeys, _ = cm.cell_keys(mesh, gids, out, info["n_after"])
    assert np.all(np.diff(key_out) >= 0)
    src = info["src"]
    for k, (a, b, W, valid) in info["cells"].items():
        m = b - a
        sel = key_out == k
        if not valid or k not in info["combed"]:
            # inside the band, or invalid: byte for byte as it was
            assert int(sel.sum()) == m
            for name in cm.SWARM_KEYS:
                assert np.array_equal(out[name][sel].view(np.uint8), sw[name][:n][info["order"]][a:b].view(np.uint8)), (k, name)
            continue
        K = info["combed"][k]
        assert int(info["counts"][a:b].sum()) == K == int(sel.sum())
        assert 1 <= K <= S * m
        assert float(m) > r * K or float(K) > r * float(m)
        e_in, e_out = math.fsum(w_in[a:b]), math.fsum(out["w"][sel])
        assert abs(e_out - e_in) <= 2 * m * _ulp(W), (k, e_in, e_out)
        assert len(set(out["w"][sel].tolist())) == 1
    for k, K in info["targets"].items():
        a, b = info["cells"][k][:2]
        assert 1 <= K <= S * (b - a)
    assert info["n_after"] <= n + N
    dead = key_in >= nkeys
    assert np.array_equal(src[-int(dead.sum()):], np.flatnonzero(dead)) if dead.any() else True


@pytest.mark.parametrize("geom", ["G1", "G2S", "G3S"])
def test_the_crafted_swarm_holds_every_case(geom):
    mesh, gids, sw, n, N, placed, out, info = _run(geom, "crafted")
    assert n <= 100000 and info["n_after"] <= 100000
    assert info["scale"] == 16.0 and info["w_total"] == N * gc.UNIT          # every sum is exact
    _check_cells(mesh, gids, sw, n, N, gc.R_BAND, gc.S_MAX, out, info)
    by_tag = {}
    for s, k in placed:
        by_tag.setdefault(s.tag, []).append((s, k))
    T, C = info["targets"], info["combed"]
    # cells of 1, 2, 63, 64, 65 photons: on the two-level meshes each size starts at every lane offset of the sorted
    # swarm; the 1-D mesh has 64 cells, which hold nine rounds of the sweep beside the fixed cases: nine starts per
    # size there.  (Cells of 2049 at every offset: test_cells_of_2049_start_at_every_lane_offset.)
    for m in (1, 2, 63, 64, 65):
        cells = by_tag[f"sweep-{m}"]
        offs = {info["cells"][k][0] % 64 for _, k in cells}
        assert len(cells) == (9 if geom == "G1" else 64)
        assert len(offs) == (9 if geom == "G1" else 64), (m, len(offs))
        assert {k in C for _, k in cells} == {True, False}
    assert all(info["cells"][k][1] - info["cells"][k][0] == 2049 for t in ("m2049-thin", "m2049-split", "m2049-alone")
               for _, k in by_tag[t])
    (s, k), = by_tag["m2049-thin"]; assert C[k] == 500
    (s, k), = by_tag["m2049-split"]; assert C[k] == 5000
    (s, k), = by_tag["m2049-alone"]; assert T[k] == 2049 and k not in C
    # one photon into 2, 64, 65 and 5000 copies (2 is inside the band of r = 2 -- K = r m is not beyond it -- so that
    # cell is split under r = 1 only: test_r_one_and_s_one_are_sharp)
    for tag, K in (("one-to-64", 64), ("one-to-65", 65), ("one-to-5000", 5000)):
        (s, k), = by_tag[tag]
        assert C[k] == K and info["counts"][info["cells"][k][0]] == K
    (s, k), = by_tag["one-to-2"]; assert T[k] == 2 and k not in C
    (s, k), = by_tag["S-binds"]; assert info["nu"][k] == 6000.0 and C[k] == gc.S_MAX * 1
    # a cell over three scan tiles thinned to 1
    (s, k), = by_tag["three-tiles-to-1"]
    a, b = info["cells"][k][:2]
    assert C[k] == 1 and (b - 1) // gc.SCAN_TILE - a // gc.SCAN_TILE >= 2
    # thinned right in front of split, and the reverse: neighbours in the sorted swarm
    (_, k0), = by_tag["thin-before-split"]; (_, k1), = by_tag["split-between"]; (_, k2), = by_tag["thin-after-split"]
    assert info["cells"][k0][1] == info["cells"][k1][0] and info["cells"][k1][1] == info["cells"][k2][0]
    assert (C[k0], C[k1], C[k2]) == (10, 20, 10)
    # photons that come out 0 times inside a split cell
    (s, k), = by_tag["zero-copies-in-split"]
    a, b = info["cells"][k][:2]
    assert C[k] == 30 > b - a and int((info["counts"][a:b] == 0).sum()) >= 7
    # held at 1 by the floor
    (s, k), = by_tag["floor-holds-1"]; assert info["nu"][k] < 1e-3 and C[k] == 1
    # weights all 0, negative, inf: invalid, left alone; they add nothing to the block sums
    for tag in ("all-zero", "negative", "inf"):
        (s, k), = by_tag[tag]
        assert info["cells"][k][3] is False and k not in T
    # empty cells between occupied ones; a ghost cell; the slots behind all cells
    nk, nj, ni = mesh.field_shape[1:]
    occupied = set(info["cells"])
    assert any(k + 1 not in occupied and k + 2 in occupied for k in occupied)
    (s, k), = by_tag["ghost-cell"]
    assert (k % (nk * nj * ni)) % ni == mesh.ng - 1 and C[k] == 2
    nkeys = mesh.nblocks * nk * nj * ni
    assert int((info["key"] == nkeys).sum()) == gc.N_DEAD + gc.N_BADBLK
    assert info["cells_thinned"] >= 4 and info["cells_split"] >= 6 and info["max_target"] == 5000
    assert info["max_per_cell"] == 2 * gc.SCAN_TILE + 100
    # a draw decides some target: nu with a fraction, K above floor(nu) in some cells and at it in others
    frac = [(k, v) for k, v in info["nu"].items() if v != math.floor(v) and v > 1]
    ups = {T[k] - math.floor(v) for k, v in frac}
    assert ups == ({0, 1} if geom != "G1" else ups) and ups <= {0, 1}


@pytest.mark.parametrize("geom,weights,exact", [("G1", "crafted", False), ("G2S", "crafted", False), ("G1", "hashed", True)])
def test_cells_of_2049_start_at_every_lane_offset(geom, weights, exact):
    """The swarms of gcomb_cases.tile_specs: over the three pads a cell of 2049 photons -- one more than a scan tile --
    starts at each of the 64 lane offsets, and is thinned, split and left alone at offsets all over the wave."""
    offs, fate = set(), {}
    for pad in gc.TILE_PADS:
        S = gc.S_MAX if weights == "crafted" else 64
        mesh, gids, sw, n, N, placed, out, info = _run(geom, weights, S=S, exact=exact, pad=pad)
        assert n <= 100000 and info["n_after"] <= 100000
        _check_cells(mesh, gids, sw, n, N, gc.R_BAND, S, out, info)
        tiles = [k for s, k in placed if s.tag == "tile-2049"]
        assert len(tiles) == gc.TILE_CELLS
        for k in tiles:
            a, b = info["cells"][k][:2]
            assert b - a == 2049 and (b - 1) // gc.SCAN_TILE > a // gc.SCAN_TILE      # crosses a scan tile
            offs.add(a % 64)
            K = info["combed"].get(k)
            fate.setdefault("alone" if K is None else ("thin" if K < 2049 else "split"), set()).add(a % 64)
        if weights == "crafted":
            assert info["scale"] == 16.0
            assert sorted({info["targets"][k] for k in tiles}) == [500, 2049, 4100]
    assert offs == set(range(64))
    if weights == "crafted":
        assert all(len(fate[f]) >= 20 for f in ("thin", "alone", "split")), {f: len(v) for f, v in fate.items()}
    else:
        assert len(fate.get("thin", ())) + len(fate.get("split", ())) >= 20


def test_r_one_and_s_one_are_sharp():
    mesh, gids, sw, n, N, placed, out, info = _run("G2S", "crafted", r=1.0)
    _check_cells(mesh, gids, sw, n, N, 1.0, gc.S_MAX, out, info)
    for k, K in info["targets"].items():
        a, b = info["cells"][k][:2]
        assert (k in info["combed"]) == (K != b - a)            # r = 1 combs every cell whose target is not its count
    k2 = next(k for s, k in placed if s.tag == "one-to-2")
    assert info["combed"][k2] == 2
    mesh, gids, sw, n, N, placed, out, info = _run("G2S", "crafted", S=1)
    _check_cells(mesh, gids, sw, n, N, gc.R_BAND, 1, out, info)
    assert info["cells_split"] == 0 and info["n_new_ids"] >= 0 and info["n_after"] < n
    key_out = cm.cell_keys(mesh, gids, out, info["n_after"])[0]
    for k, (a, b, W, valid) in info["cells"].items():
        assert int((key_out == k).sum()) <= b - a                # S = 1 never grows any cell


@pytest.mark.parametrize("exact", [False, True], ids=["tree", "exact"])
def test_floating_point_weights_and_the_margin_cap(exact):
    """The hashed weights of the GPU test: the properties hold, and the share of cells within 1e-9 of a decision --
    what the GPU test may leave out under the default order -- is at most 1 %."""
    for geom in ("G1", "G2S", "G3S"):
        mesh, gids, sw, n, N, placed, out, info = _run(geom, "hashed", S=64, exact=exact)
        _check_cells(mesh, gids, sw, n, N, gc.R_BAND, 64, out, info)
        close = [k for k, v in info["margins"].items() if v < 1e-9]
        print(geom, "cells within 1e-9 of a decision:", len(close), "of", len(info["margins"]))
        assert len(close) <= 0.01 * len(info["margins"])
        assert info["cells_thinned"] > 0 and info["cells_split"] > 0


def test_running_weights_of_the_canonical_order_are_exact_and_the_tree_is_close():
    rng = np.random.default_rng(7)
    w = 10.0 ** (6.0 * rng.random(3000) - 3.0)
    C = gm.running_exact(w)
    for j in (0, 1, 17, 500, 2999):              # (the conversion rounds lo, then the sum: within an ulp of exact)
        assert abs(C[j] - math.fsum(w[:j + 1])) <= _ulp(C[j])
    key = np.sort(rng.integers(0, 9, 7000))
    w = 10.0 ** (6.0 * rng.random(7000) - 3.0)
    T = gm.running_tree(key, w)
    for k in range(9):
        sel = np.flatnonzero(key == k)
        ref = np.array([math.fsum(w[sel[0]:j + 1]) for j in sel[::97]])
        assert np.all(np.abs(T[sel[::97]] - ref) <= len(sel) * 2.0 ** -53 * ref)
    wi = np.round(w * 1024.0) * 2.0 ** -20
    T = gm.running_tree(key, wi)
    assert all(np.array_equal(T[key == k], np.cumsum(wi[key == k])) for k in range(9))


def test_count_draw_is_keyed_and_differs_from_the_selection_draw():
    seen = {gm.xi_count_of(123, e, g, c) for e in (1, 2) for g in (0, 5) for c in (0, 77)}
    assert len(seen) == 8 and all(0.0 < x < 1.0 for x in seen)
    assert gm.xi_count_of(123, 3, 4, 5) == gm.xi_count_of(123, 3, 4, 5) != gm.xi_count_of(124, 3, 4, 5)
    assert all(gm.xi_count_of(123, e, 2, c) != cm.xi_of(123, e, 2, c) for e in (1, 2) for c in (0, 77))


def test_unbiased_over_the_epochs():
    """Over 4096 epochs: E[K_k] = nu_k for the cells whose clamps do not bind, and the mean copy count of a photon is
    w_j Kbar_k / W_k, each within 5 sigma."""
    rng = np.random.default_rng(11)
    E = 4096
    cells = [(3, 2.37), (5, 7.5), (2, 12.25), (8, 3.9), (4, 1.6)]     # (m, nu): 1 < nu, far below S m
    S = 64
    for c, (m, nu) in enumerate(cells):
        w = 10.0 ** (2.0 * rng.random(m))
        C = np.cumsum(w)
        W = float(C[-1])
        scale = nu / W
        Ks = np.zeros(E)
        copies = np.zeros((E, m))
        for e in range(E):
            K = gm.target_of(W, m, scale, S, gm.xi_count_of(SEED, e, 3, c))
            Ks[e] = K
            copies[e] = gm.counts_of(C, K, cm.xi_of(SEED, e, 3, c))[0]     # r = 1: combed whenever K != m
        nu_f = W * scale
        p = nu_f - math.floor(nu_f)
        sigma = math.sqrt(p * (1 - p) / E)
        assert abs(Ks.mean() - nu_f) <= 5 * sigma, (m, nu, Ks.mean())
        want = w * Ks.mean() / W
        sd = copies.std(axis=0) / math.sqrt(E)
        assert np.all(np.abs(copies.mean(axis=0) - want) <= 5 * sd + 1e-12), (copies.mean(axis=0), want)


def test_census_total_keys_are_checked():
    from jaybenne_amd.jaybenne import check_census_total
    check_census_total(0, 2.0, 64)
    check_census_total(50000, 1.0, 1)
    for bad in ((-1, 2.0, 64), (1 << 31, 2.0, 64), (10, 0.5, 64), (10, float("inf"), 64), (10, float("nan"), 64), (10, 2.0, 0)):
        with pytest.raises(ValueError):
            check_census_total(*bad)
    with pytest.raises(ValueError) as err:
        check_census_total(10, 2.0, 64, per_cell_max=25)
    assert "census_total_target" in str(err.value) and "census_per_cell_max" in str(err.value)


def _n_eff(w):
    return math.fsum(w) ** 2 / math.fsum(w * w)


def test_stepdiff_acceptance_with_the_global_comb():
    """The oracle runs stepdiff at nx1 = 128 with 1e5 photons (uniform allocation) and the model combs after every
    cycle with N = 5e4, r = 1.  N_eff / n must rise at the first comb; every combed cell with nu >= 8 has its copy
    weight within [8/9, 8/7] of W_tot / N (|K - nu| < 1); the run passes the reference's gate (0.05)."""
    from jaybenne_amd.analysis import analytic_errors
    from oracle import orc
    from oracle.harness import make_oracle
    N, r, S = 50000, 1.0, 64
    pin = load_deck("stepdiff", {"parthenon/mesh/nx1": 128, "parthenon/meshblock/nx1": 64,
                                 "jaybenne/num_particles": 100000})
    O, mesh, _ = make_oracle(pin, orc.MATH_LIBM, threads=16)
    seed = pin.GetOrAddInteger("jaybenne", "seed", 123)
    dt = pin.GetReal("jaybenne", "dt")
    gids = np.arange(mesh.nblocks)
    e0 = math.fsum(O.sw["w"][:O.n])
    t, first = 0.0, None
    for _ in range(10):
        O.RadiationStep(t, dt)
        O.fields["sie"][...] = O.fields["u"] / O.fields["rho"]
        t += dt
        n = O.n
        before = _n_eff(O.sw["w"][:n]) / n
        out, info = gm.gcomb_swarm(mesh, gids, np.ones(mesh.nblocks), O.sw, n, N, r, S, seed, O.cycle, O.next_id)
        after = _n_eff(out["w"]) / info["n_after"]
        if first is None:
            first = (before, after)
            print("N_eff / n before and after the first comb:", before, after, "n:", n, "->", info["n_after"])
            assert after > before
            share = info["w_total"] / N
            key_out = cm.cell_keys(mesh, gids, out, info["n_after"])[0]
            checked = 0
            for k, K in info["combed"].items():
                if info["nu"][k] >= 8.0:
                    wk = out["w"][key_out == k][0]
                    assert 8.0 / 9.0 <= wk / share <= 8.0 / 7.0, (k, wk / share)
                    checked += 1
            assert checked > 0
        assert info["n_after"] <= n + N
        for name in cm.SWARM_KEYS:
            O.sw[name][:info["n_after"]] = out[name]
        O.n = info["n_after"]
        O.next_id += info["n_new_ids"]
    assert math.isclose(math.fsum(O.sw["w"][:O.n]), e0, rel_tol=1e-12)
    assert len(np.unique(O.sw["id"][:O.n])) == O.n
    occupied = len(np.unique(cm.cell_keys(mesh, gids, O.sw, O.n)[0]))
    # (every cell comes out with K_k > nu_k - 1 or stays within r of it, so n >= N / r - occupied is what the rule
    # gives; at r = 1, where every cell is combed to floor(nu) or floor(nu) + 1, the sum of the targets can fall a
    # few photons short of N itself, so the lower end of the deck runs' [N / r, r N + occupied] is not implied here)
    assert N / r - occupied <= O.n <= r * N + occupied
    O.EvaluateRadiationEnergy()
    err = analytic_errors(mesh, O.fields["tally"], t)
    print("globally combed stepdiff:", err)
    assert err["mean_frac_error_weighted"] <= 0.05
