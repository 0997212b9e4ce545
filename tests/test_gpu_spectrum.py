"""The radiation spectrum on the GPU (jb_evaluate_radiation_spectrum: k_spec_chunks, k_spec_cells) against
tests/spectrum_model.py bit for bit on crafted swarms -- tests/test_spectrum_host.py shows that the swarms hold the
cases --, against the moments kernels' E, the call's invariances, the Planck law of the census of ``inf``, the two
command-line hosts, and two ranks."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import moments_model as mm
import spectrum_model as sm
import swarm_ops_model as som
from helpers import DECK_DIR, ROOT, load_deck

from test_gpu_comb import _upload
from test_gpu_swarm_ops import _check, _download

pytestmark = pytest.mark.gpu

NP = "jaybenne/num_particles"
PLANS = mm.run_plans()
# JB_SPECTRUM_GROUP: every lanes-per-cell width k_spec_cells is compiled for, beside the host's own choice
GROUPS = ("1", "2", "4", "8", "16", "32", "64")


@pytest.fixture(scope="module")
def views(gpu_device):
    """(driver, Geom) per (mesh, rank, nranks), made once"""
    from jaybenne_amd import mcblock
    made = {}

    def get(case, rank=0, nranks=1):
        key = (repr(case), rank, nranks)
        if key not in made:
            drv = mcblock.McblockDriver(load_deck(*case), rank=rank, nranks=nranks, comm=None, device=gpu_device)
            md = drv.md
            assert md.cell_order == "any" and md.deposition == "atomic"
            made[key] = (drv, som.Geom(drv.mesh, md.resident_gids, md.field_owner, md.nowned))
        return made[key]

    yield get
    for drv, _ in made.values():
        drv.md.cell_order = "any"
        drv.md.close()
    made.clear()


def _out(md, ngroups, fill=float("nan")):
    import torch
    nx = md.mesh.nx
    return torch.full((ngroups + 2, md.nblocks, int(nx[2]), int(nx[1]), int(nx[0])), fill, dtype=torch.float64,
                      device=md.device)


def _spectrum(md, edges, group=None, report=True):
    """(out [NB, nblocks, nx3, nx2, nx1] on the host, report) of one call; the output array is filled with NaN
    first: every word must be written"""
    import torch
    from jaybenne_amd import _lib
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    ng = len(edges) - 1
    out = _out(md, ng)
    assert out.numel() == md.lib.jb_spectrum_words(md.handle, ng)
    rep = _lib.SpectrumReport()
    md._sync_stream()
    if group is None:
        os.environ.pop("JB_SPECTRUM_GROUP", None)
    else:
        os.environ["JB_SPECTRUM_GROUP"] = group
    try:
        st = md.lib.jb_evaluate_radiation_spectrum(md.pkg.ctx, md.handle, C.byref(md.sv), edges.ctypes.data, ng,
                                                   out.data_ptr(), C.byref(rep) if report else None)
    finally:
        os.environ.pop("JB_SPECTRUM_GROUP", None)
    _check(md, st)
    torch.cuda.synchronize(md.device)
    return out.cpu().numpy(), rep.as_dict()


def _against_the_model(md, g, sw, edges, what):
    """uploads sw, calls, and holds bins and report to the model on the swarm as the call left it"""
    n = len(sw["id"])
    _upload(md, sw, md.device)
    got, rep = _spectrum(md, edges)
    after = _download(md, n)
    assert som.sorted_failures(g, sw, after, n) == [], what          # the same photons, in key order
    want, want_rep = sm.spectrum(g, after, n, edges)
    assert sm.differing_bins(got, want) == [], what
    assert rep == dict(want_rep, sorted=0 if mm.in_order(g, sw, n) else 1), (what, rep, want_rep)
    return got, after


# ---- 1: crafted swarms, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("plan", range(len(PLANS)), ids=[f"{p[0]}-{p[1]}-{sm.plan_groups(q)}" for q, p in enumerate(PLANS)])
def test_runs_equal_the_model(gpu_device, views, plan):
    """runs of 1, 2, 63, 64, 65, 4095, 4096, 4097, 2 x 4096 + 1 slots at every lane offset and one cell of
    3 x 4096 + 5, given unsorted with other statuses and bad blks among them, energies on and beside every edge and
    the odd values, 1, 2, 7, 33, 64 groups in turn; then the sorted swarm again under every group width: the same
    bits, and the call does not sort"""
    name, mesh, lengths = PLANS[plan]
    edges = sm.edges_for(sm.plan_groups(plan))
    drv, g = views(mm.mesh_cases()[mesh])
    sw, _ = sm.run_swarm(g, lengths, edges)
    got, after = _against_the_model(drv.md, g, sw, edges, name)
    assert not np.isnan(got).any() and got.any(axis=(1, 2, 3, 4)).all()              # every bin holds something
    for group in GROUPS:
        again, rep = _spectrum(drv.md, edges, group)
        assert sm.differing_bins(again, got) == [] and rep["sorted"] == 0, (name, group)
    assert som.differing(_download(drv.md, len(sw["id"])), after) == []        # a sorted swarm is not moved


@pytest.mark.parametrize("mesh", ["1d", "2d", "3d"])
def test_hashed_swarm_equals_the_model(gpu_device, views, mesh):
    """hashed cells, photons clamped into ghost cells, hashed statuses and bad blks"""
    drv, g = views(mm.mesh_cases()[mesh])
    for n, ng in ((1, 64), (65, 33), (20011, 7)):
        edges = sm.edges_for(ng)
        got, _ = _against_the_model(drv.md, g, sm.hashed_swarm(g, n, edges, mm.SALT + n), edges, (mesh, n))
    for group in GROUPS:
        again, _ = _spectrum(drv.md, edges, group)
        assert sm.differing_bins(again, got) == [], (mesh, group)


# ---- 2: against the moments kernels ---------------------------------------------------------------------
def test_one_group_with_the_widest_edges_is_the_moments_e(gpu_device, views):
    """edges {4.9e-324, DBL_MAX}, every e positive and finite: bin 1 equals JB_MOM_E of
    jb_evaluate_radiation_moments on the same uploaded swarm bit for bit, under the host's own lanes-per-cell width
    and each of the seven forced ones"""
    from jaybenne_amd import _lib
    from test_gpu_moments import _moments
    drv, g = views(mm.mesh_cases()["2d"])
    md = drv.md
    sw, _ = mm.run_swarm(g, [65, 4097, 1, 2 * mm.CHUNK + 1, 64, 700, 2, 63])
    sw["e"] = np.ldexp(1.0 + som._unit(sw["id"], 3), (som._mod(sw["id"], 4, 2000) - 1000).astype(np.int32))
    sw["e"][::501] = 4.9e-324
    _upload(md, sw, gpu_device)
    fields, mrep = _moments(md)
    for group in (None,) + GROUPS:
        spec, rep = _spectrum(md, sm.WIDEST, group)
        assert mm.same_bits(spec[1], fields[_lib.MOMENT_NAMES.index("e")]), group
        assert not spec[0].any() and not spec[2].any()
        assert rep == dict(mrep, sorted=0, n_below=0, n_above=0)
    assert fields[0].max() == 2 * mm.CHUNK + 1


# ---- 3: invariances -----------------------------------------------------------------------------------------
def test_halo_copies_get_zeros(gpu_device, views):
    drv, g = views(som.RANK_MESH, 1, 2)
    assert g.nowned < g.nblocks
    edges = sm.edges_for(7)
    got, after = _against_the_model(drv.md, g, sm.hashed_swarm(g, 3000, edges), edges, "halo")
    assert not got[:, g.nowned:].any() and got[:, :g.nowned].any()
    assert int(((after["status"] == som.ST_ACTIVE) & (after["blk"] >= g.nowned) & (after["blk"] < g.nblocks)).sum()) > 10


def test_empty_swarm_and_one_photon_in_the_last_cell(gpu_device, views):
    drv, g = views(mm.mesh_cases()["3d"])
    md = drv.md
    edges = sm.edges_for(33)
    md.sv.n = 0
    got, rep = _spectrum(md, edges)
    assert not got.any() and not np.isnan(got).any()
    assert rep == dict(n_counted=0, n_skipped=0, cells_nonempty=0, longest_run=0, n_below=0, n_above=0, sorted=0)
    got, rep = _spectrum(md, edges, report=False)
    assert not got.any() and not np.isnan(got).any()
    sw, cells = sm.run_swarm(g, [1], edges, extras=0, first_cell=g.nblocks * g.ncell - 1)
    got, _ = _against_the_model(md, g, sw, edges, "one photon")
    b = int(sm.bins(edges, sw["e"])[0])
    assert got[b, -1, -1, -1, -1] > 0 and np.count_nonzero(got) == 1


def test_null_and_bad_arguments_are_refused_with_out_untouched(gpu_device, views):
    import torch
    from jaybenne_amd import _lib
    from test_spectrum_host import BAD_EDGES
    drv, g = views(mm.mesh_cases()["1d"])
    md = drv.md
    sw = sm.hashed_swarm(g, 3000, sm.edges_for(2))
    _upload(md, sw, gpu_device)
    md._sync_stream()
    rep = _lib.SpectrumReport()
    f = md.lib.jb_evaluate_radiation_spectrum
    good = np.ascontiguousarray(sm.edges_for(2))
    out = _out(md, 64, fill=-7.0)
    assert f(md.pkg.ctx, md.handle, C.byref(md.sv), good.ctypes.data, 2, None, C.byref(rep)) == _lib.JB_ERR_INVALID
    assert f(md.pkg.ctx, md.handle, C.byref(md.sv), None, 2, out.data_ptr(), C.byref(rep)) == _lib.JB_ERR_INVALID
    assert f(md.pkg.ctx, md.handle, None, good.ctypes.data, 2, out.data_ptr(), C.byref(rep)) == _lib.JB_ERR_INVALID
    assert f(md.pkg.ctx, None, C.byref(md.sv), good.ctypes.data, 2, out.data_ptr(), C.byref(rep)) == _lib.JB_ERR_INVALID
    assert f(None, md.handle, C.byref(md.sv), good.ctypes.data, 2, out.data_ptr(), None) == _lib.JB_ERR_INVALID
    host = np.full(out.numel(), -7.0)
    for name, edges, ng in BAD_EDGES:
        arr = np.ascontiguousarray(edges, dtype=np.float64)
        assert f(md.pkg.ctx, md.handle, C.byref(md.sv), arr.ctypes.data, ng, out.data_ptr(), C.byref(rep)) == _lib.JB_ERR_INVALID, name
        assert md.lib.jb_evaluate_radiation_spectrum_host(md.pkg.ctx, md.handle, C.byref(md.sv), arr.ctypes.data, ng,
                                                          host.ctypes.data, None) == _lib.JB_ERR_INVALID, name
    torch.cuda.synchronize(md.device)
    assert bool((out == -7.0).all()) and np.all(host == -7.0)
    assert som.differing(_download(md, 3000), sw) == []               # nothing was launched: not even the sort
    assert md.lib.jb_spectrum_words(md.handle, 2) == 4 * g.nblocks * g.ncell
    assert md.lib.jb_spectrum_words(md.handle, 0) == 0 and md.lib.jb_spectrum_words(md.handle, 65) == 0
    # the host-array form agrees with the device-array form
    want, want_rep = _spectrum(md, good)
    host = np.full(want.size, np.nan)
    _check(md, md.lib.jb_evaluate_radiation_spectrum_host(md.pkg.ctx, md.handle, C.byref(md.sv), good.ctypes.data, 2,
                                                          host.ctypes.data, C.byref(rep)))
    assert mm.same_bits(host.reshape(want.shape), want) and rep.as_dict() == dict(want_rep, sorted=0)


def _mixed(g, edges):
    return sm.run_swarm(g, [65, 4097, 1, 2 * mm.CHUNK + 1, 64, 700, 2, 63], edges, extras=mm.EXTRAS)


def test_by_id_any_permutation_gives_the_same_bits(gpu_device, views):
    drv, g = views(mm.mesh_cases()["2d"])
    md = drv.md
    edges = sm.edges_for(7)
    sw, _ = _mixed(g, edges)
    n = len(sw["id"])
    want, want_rep = sm.spectrum(g, mm.canonical(g, sw, n), n, edges)
    md.cell_order = "id"
    try:
        for salt in (1, 2, 3):
            _upload(md, mm.shuffle(sw, salt), gpu_device)
            got, rep = _spectrum(md, edges)
            assert sm.differing_bins(got, want) == [], salt
            assert rep == dict(want_rep, sorted=1)
            assert som.differing(_download(md, n), mm.canonical(g, sw, n)) == []
        got, rep = _spectrum(md, edges)                                    # in canonical order already
        assert sm.differing_bins(got, want) == [] and rep["sorted"] == 0
    finally:
        md.cell_order = "any"


def test_a_cell_does_not_depend_on_where_it_lies(gpu_device, views):
    """JB_CELL_ORDER_ANY: photons put into an earlier cell -- every later cell then starts at another slot -- change
    no bit of a later cell, and the call does not sort a swarm in key order"""
    drv, g = views(mm.mesh_cases()["1d"])
    md = drv.md
    edges = sm.edges_for(7)
    sw, cells = _mixed(g, edges)
    n = len(sw["id"])
    a = mm.canonical(g, sw, n)
    _upload(md, a, gpu_device)
    base, rep = _spectrum(md, edges)
    assert rep["sorted"] == 0 and som.differing(_download(md, n), a) == []
    for extra in (1, 63, 1000):
        more, _ = sm.run_swarm(g, [extra], edges, salt=mm.SALT + extra, extras=0, first_cell=1)
        both = mm.canonical(g, {k: np.concatenate((more[k], a[k])) for k in som.KEYS}, n + extra)
        _upload(md, both, gpu_device)
        got, rep = _spectrum(md, edges)
        flat_a, flat_g = base.reshape(len(base), -1), got.reshape(len(got), -1)
        assert rep["sorted"] == 0 and flat_g[:, 1].any() and not flat_a[:, 1].any()
        assert mm.same_bits(flat_a[:, cells], flat_g[:, cells]), extra


def test_everything_else_is_untouched(gpu_device, views):
    """energy_tally, energy_delta and the multiset of photons by id are bit-identical before and after"""
    import torch
    drv, g = views(mm.mesh_cases()["3d"])
    md = drv.md
    edges = sm.edges_for(7)
    sw = sm.hashed_swarm(g, 20011, edges, mm.SALT + 5)
    _upload(md, sw, gpu_device)
    marks = {}
    for q, name in enumerate(("tally", "edelta")):
        base = som.edelta_base(g, 11 + q)
        md.set_field(name, base, local=True)
        marks[name] = base
    _spectrum(md, edges)
    torch.cuda.synchronize(md.device)
    for name, base in marks.items():
        assert np.array_equal(md.fields[name].cpu().numpy().view(np.uint64), base.view(np.uint64)), name
    assert md.n == 20011 and som.same_multiset(_download(md, 20011), sw) == []


def test_the_scratch_changes_hands(gpu_device, views):
    """sort, comb, moments and spectrum on one context: a comb plan lies in the scratch memory until it is applied, and
    a spectrum evaluation in between takes the memory -- the apply then finds no plan; then the sort, a comb plan and
    apply and the moments against their models (tests/test_gpu_moments.py), the spectrum against its own with 1 and 64
    groups (its partials and edges lie where the moments' partials lay), and the moments once more"""
    from jaybenne_amd import _lib
    from test_gpu_comb import _apply, _plan
    from test_gpu_moments import TILE_COMB, TILE_MESHES, _sort_comb_moments, _tile_swarm
    from test_gpu_moments import _against_the_model as _moments_against_the_model
    name, n = "8 cells", 40009
    drv, g = views(TILE_MESHES[name])
    md = drv.md
    T, K = TILE_COMB[name]
    _upload(md, _tile_swarm(drv.mesh, n), gpu_device)
    st, plan = _plan(md, T, K)
    assert st == _lib.JB_COMPLETE and plan.n_after < n, md.lib.jb_last_error()
    _spectrum(md, sm.edges_for(2))
    st, _ = _apply(md)
    assert st == _lib.JB_ERR_INVALID and b"no plan for this swarm" in md.lib.jb_last_error()
    assert md.n == n
    _sort_comb_moments(drv, g, name, 2049, "any", gpu_device)
    for ng in (64, 1):
        edges = sm.edges_for(ng)
        sw = sm.craft_e(_tile_swarm(drv.mesh, n), edges)
        _, after = _against_the_model(md, g, mm.shuffle(sw, 5), edges, (name, ng))
        _moments_against_the_model(md, g, mm.shuffle(after, 9), (name, ng))


# ---- 4: physics ---------------------------------------------------------------------------------------------
X_EDGES = (0.5, 1, 2, 3, 4, 6, 8, 12)


def test_the_census_of_inf_is_planckian(gpu_device):
    """``inf`` (gray, do_feedback = false: T stays at its initial value), 20000 photons, three cycles; edges at
    x sb T for x = 0.5, 1, 2, 3, 4, 6, 8, 12, with the sb the package was initialised with.  The share of the domain's
    census energy in every bin is 15 / pi^4 times the integral of x^3 / (e^x - 1) over the bin (from the series)
    within 5 sqrt(p (1 - p) / N_eff), N_eff = (sum w)^2 / sum w^2 from the moments call; and in every cell the bins
    sum to the moments' E within (2 L + NB) 2^-53 relative, L the cell's count."""
    from jaybenne_amd import jaybenne as jb, mcblock
    drv = mcblock.McblockDriver(load_deck("inf", {NP: 20000}), device=gpu_device, capacity_factor=4.0)
    md = drv.md
    try:
        assert not drv.pkg.Param("do_feedback")
        for _ in range(3):
            drv.Step()
        sbT = drv.pkg.Param("stefan_boltzmann") * drv.mcb.initial_temperature
        edges = [x * sbT for x in X_EDGES]
        spec_t, rep = jb.EvaluateRadiationSpectrum(md, edges)
        assert spec_t is md.spectrum and rep == md.spectrum_report
        spec = spec_t.cpu().numpy()
        fields, mrep = jb.EvaluateRadiationMoments(md)
        m = fields.cpu().numpy()
        nb = len(edges) + 1
        assert spec.shape == (nb,) + m.shape[1:] and {k: rep[k] for k in mrep if k != "sorted"} == {k: mrep[k] for k in mrep if k != "sorted"}
        assert rep["n_counted"] > 20000
        dx = np.asarray(drv.mesh.blk_dx)[md.resident_gids]
        integ = sm.integrals(spec, dx)
        mint = mm.integrals(m, dx)
        neff = mint[1] ** 2 / mint[2]
        total = math.fsum(integ)
        assert abs(total - mint[1]) <= 1e-12 * mint[1]
        want = sm.planck_fractions(X_EDGES)
        print(f"N_eff {neff:.0f}; photons {rep['n_counted']}; below {rep['n_below']} above {rep['n_above']}")
        worst = 0.0
        for q in range(nb):
            p, got = want[q], integ[q] / total
            sigma = math.sqrt(p * (1.0 - p) / neff)
            print(f"bin {q}: share {got:.6f}, Planck {p:.6f}, {(got - p) / sigma:+.2f} sigma")
            worst = max(worst, abs(got - p) / sigma)
        assert worst <= 5.0, worst
        # cell by cell: the bins add up to E
        L, E = m[0], m[1]
        total_c = np.zeros_like(E)
        for q in range(nb):
            total_c = total_c + spec[q]
        bound = (2.0 * L + nb) * 2.0 ** -53 * E
        print("largest |sum of bins - E| / bound:", float(np.max(np.abs(total_c - E)[L > 0] / bound[L > 0])))
        assert np.all(np.abs(total_c - E) <= bound) and (L > 0).sum() == rep["cells_nonempty"]
    finally:
        md.close()


# ---- 5: the command-line hosts, two ranks ---------------------------------------------------------------------
EDGE_TEXT = "2.8e-5,5.7e-5, 1.1e-4,1.7e-4,2.3e-4,3.4e-4,4.5e-4,6.8e-4"


def test_both_hosts_write_the_same_lines(gpu_device, tmp_path):
    """``--spectrum FILE`` on one short inf run, in the canonical cell order and with exact deposition so that the run
    is a function of the deck alone: the files agree line for line; the deck key alone writes spectrum.jsonl, and
    spectrum_edges alone does nothing"""
    exe = os.path.join(ROOT, "examples", "mcblock_amd")
    assert os.path.exists(exe), "examples/mcblock_amd has not been built (__graft_entry__.build())"
    ov = {NP: 4000, "parthenon/time/tlim": 2.5e-12, "jaybenne_amd/cell_order": "id", "jaybenne_amd/deposition": "exact",
          "jaybenne_amd/spectrum_edges": EDGE_TEXT}
    args = ["-i", os.path.join(DECK_DIR, "inf.in")] + [f"{k}={v}" for k, v in ov.items()]
    env = dict(os.environ, JB_EXACT_ARITH="1")
    runs = {"py": [sys.executable, "-m", "jaybenne_amd"], "cc": [exe]}
    for name, cmd in runs.items():
        res = subprocess.run(cmd + args + ["--spectrum", str(tmp_path / f"{name}.jsonl")], capture_output=True, text=True,
                             env=env, timeout=240, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    py, cc = (open(tmp_path / f"{name}.jsonl").read().splitlines() for name in runs)
    assert len(py) == 3 and py == cc, (py, cc)
    edges = [float(v) for v in EDGE_TEXT.split(",")]
    for q, line in enumerate(py):
        rec = json.loads(line)
        assert rec["cycle"] == q + 1 and rec["n_counted"] > 4000 and rec["sorted"] == 1 and rec["ngroups"] == 7
        assert rec["edges"] == edges and len(rec["e"]) == 9 and all(v > 0 for v in rec["e"])
        assert 0 < rec["n_below"] < rec["n_above"] + rec["n_below"] < rec["n_counted"]
    # off by default, on by the deck key; the edges alone do nothing
    res = subprocess.run(runs["cc"] + args + ["jaybenne_amd/spectrum=true"], capture_output=True, text=True, env=env,
                         timeout=240, cwd=str(tmp_path))
    assert res.returncode == 0 and open(tmp_path / "spectrum.jsonl").read().splitlines() == cc
    os.remove(tmp_path / "spectrum.jsonl")
    res = subprocess.run(runs["cc"] + args, capture_output=True, text=True, env=env, timeout=240, cwd=str(tmp_path))
    assert res.returncode == 0 and not os.path.exists(tmp_path / "spectrum.jsonl")


def test_both_hosts_refuse_the_same_edge_text(gpu_device, tmp_path):
    """a hex float -- a number to strtod, not to float(): both hosts stop with exit code 2 and the same words, and write
    no line (the grammar and the other refusals: tests/test_spectrum_host.py)"""
    exe = os.path.join(ROOT, "examples", "mcblock_amd")
    assert os.path.exists(exe), "examples/mcblock_amd has not been built (__graft_entry__.build())"
    runs = {"py": [sys.executable, "-m", "jaybenne_amd"], "cc": [exe]}
    for text, words in (("0x1p-3,1", "spectrum_edges: '0x1p-3' is not a decimal number"),):
        for name, cmd in runs.items():
            out = tmp_path / f"{name}.jsonl"
            res = subprocess.run(cmd + ["-i", os.path.join(DECK_DIR, "inf.in"), f"{NP}=400", "parthenon/time/tlim=1e-12",
                                        f"jaybenne_amd/spectrum_edges={text}", "--spectrum", str(out)],
                                 capture_output=True, text=True, timeout=240, cwd=ROOT)
            assert res.returncode == 2 and res.stderr.strip().endswith(words), (name, text, res.returncode, res.stderr[-500:])
            assert not os.path.exists(out) or open(out).read() == ""


RUN = {"parthenon/mesh/nx1": 16, "parthenon/meshblock/nx1": 8, NP: 20000, "jaybenne/do_emission": "false",
       "jaybenne/do_feedback": "false", "jaybenne_amd/cell_order": "id"}
RUN_X = (1, 2, 3, 4, 6, 8)


def _run_edges(drv):
    # (stepdiff's census is not at one temperature: the edges only have to spread its photons over the bins)
    return [x * drv.pkg.Param("stefan_boltzmann") for x in RUN_X]


def _rank_worker(rank, world, port, outdir, decomposition):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jaybenne_amd import jaybenne as jb, mcblock
        from jaybenne_amd.comm import Comm
        drv = mcblock.McblockDriver(load_deck("stepdiff", RUN), rank=rank, nranks=world, comm=Comm(),
                                    device=torch.device("cuda", 0), capacity_factor=2.0, decomposition=decomposition)
        drv.pkg.set_arithmetic("exact")
        for _ in range(2):
            drv.Step()
        spec, rep = jb.EvaluateRadiationSpectrum(drv.md, _run_edges(drv))
        np.savez(os.path.join(outdir, f"{decomposition}{rank}.npz"), resident=np.asarray(drv.md.resident_gids),
                 owner=np.asarray(drv.mesh.owner), nowned=drv.md.nowned, spec=spec.cpu().numpy(),
                 counted=rep["n_counted"], below=rep["n_below"], above=rep["n_above"])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("decomposition", ["blocks", "replicated"])
def test_two_ranks_equal_one(gpu_device, tmp_path, decomposition):
    """stepdiff in two blocks, canonical cell order (the mesh of tests/test_gpu_moments.py).  Block partition: each
    rank's owned cells have the one-rank run's bits (and its halo copy zeros).  Replicated mesh: the ranks' sums agree
    with it to 1e-12 of a bin's largest entry, the counts exactly."""
    import torch.multiprocessing as mp
    from jaybenne_amd import jaybenne as jb, mcblock
    from test_gpu_multirank import _free_port, _run_workers
    ctx = mp.get_context("spawn")
    port = _free_port()
    _run_workers([ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path), decomposition)) for r in range(2)])
    parts = [np.load(tmp_path / f"{decomposition}{r}.npz") for r in range(2)]
    drv = mcblock.McblockDriver(load_deck("stepdiff", RUN), device=gpu_device)
    try:
        drv.pkg.set_arithmetic("exact")
        for _ in range(2):
            drv.Step()
        spec, rep = jb.EvaluateRadiationSpectrum(drv.md, _run_edges(drv))
        one = spec.cpu().numpy()
    finally:
        drv.md.close()
    assert one.shape[:2] == (len(RUN_X) + 1, 2) and rep["n_counted"] > 10000 and one.any(axis=(1, 2, 3, 4)).all()
    if decomposition == "blocks":
        for k in ("counted", "below", "above"):
            assert sum(int(p[k]) for p in parts) == rep["n_" + k], k
        for r, p in enumerate(parts):
            nowned, resident = int(p["nowned"]), p["resident"]
            assert nowned == 1 and len(resident) == 2 and p["owner"][resident[0]] == r
            assert sm.differing_bins(p["spec"][:, :1], one[:, resident[:1]]) == [], r
            assert not p["spec"][:, 1:].any()
    else:
        for p in parts:
            for k in ("counted", "below", "above"):
                assert int(p[k]) == rep["n_" + k], k
            for q in range(len(one)):
                assert np.abs(p["spec"][q] - one[q]).max() <= 1e-12 * np.abs(one[q]).max(), q
        assert sm.differing_bins(parts[0]["spec"], parts[1]["spec"]) == []
