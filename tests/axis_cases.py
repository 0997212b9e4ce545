"""Meshes whose per-axis numbers all differ, under boundary kinds that differ from face to face, and the list of
cases that run on them.

On every mesh of tests/test_gpu_parity.py::CASES and tests/hetero_states.py the second and third axes are
interchangeable (dy == dz, nj == nk, nleaf[1] == nleaf[2]), every domain is symmetric about 0 (gmin == -gmax), x2 and
x3 are periodic in (nearly) every tracking run and the two faces of an axis never differ in kind: a kernel that
swaps hy with hz, nj with nk, nleaf[1] with nleaf[2], bc[2] with bc[4] or bc[2 d] with bc[2 d + 1], or whose sign
only holds for gmin < 0 < gmax, computes the same bits there.  Here cell widths, cells per block, blocks per axis,
leaf counts, origins and extents take a different value on every active axis, no origin is 0 or minus the upper
bound, and three boundary sets rotate reflecting / outflow / periodic over the faces.

The material is ``hetero_states.State`` (the plain ``ProblemGenerator`` state is a function of x1 alone).
tests/test_axis_host.py (CPU) checks that the inputs are asymmetric and send photons through every face;
tests/test_gpu_axes.py runs the kernels on them.  Both import the tables below.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import hetero_states as hs
from helpers import load_deck
from jaybenne_amd.mesh import Mesh

R, O, P = "jaybenne_reflecting", "outflow", "periodic"
FACES = ("ix1", "ox1", "ix2", "ox2", "ix3", "ox3")
# over the three sets every face sees every kind, and the two faces of an axis differ where they are not periodic
BOUNDARY_SETS = {"S1": (R, O, O, R, P, P), "S2": (P, P, R, O, O, R), "S3": (O, R, P, P, R, O)}
BOUNDARY_SETS_1D = {"RO": (R, O), "OR": (O, R)}

Geometry = namedtuple("Geometry", "nx bx extents refine exact")

GEOMETRIES = {
    # 3-D, one level, 2 x 3 x 4 blocks; widths 1/16, 1/8, 1/32
    "G3U": Geometry((16, 12, 8), (8, 4, 2), ((-0.25, 0.75), (0.5, 2.0), (-1.0, -0.75)), None, True),
    # 3-D, two levels, 2 x 3 x 4 base blocks, 20 coarse + 32 fine; base widths 1/32, 1/16, 1/64; the fine blocks
    # touch the ix2 and ox3 boundaries; x3 is the thin axis so that DDMC photons reach its faces
    "G3S": Geometry((32, 12, 8), (16, 4, 2), ((-0.25, 0.75), (0.5, 1.25), (-3.0, -2.875)),
                    ((0.0, 0.5), (0.5, 0.75), (-2.9375, -2.875)), True),
    # 2-D, two levels; base widths 1/64, 1/32
    "G2S": Geometry((64, 8), (16, 4), ((-0.25, 0.75), (0.5, 0.75)), ((0.0, 0.5), (0.5, 0.625)), True),
    # as G3U with widths 1/24, 1/10, 3/80: the general-geometry kernels
    "G3O": Geometry((24, 12, 8), (12, 4, 2), ((-0.25, 0.75), (0.5, 1.7), (-1.0, -0.7)), None, False),
    # widths 1/16, 1/8, 1/32 as G3U, but x1 starts at -7/32 = -3.5 widths: every number is exact, the faces are
    # not whole numbers of widths, so exact geometry must be off (the hot / cold step at x1 = 0 is inside a cell)
    "G3X": Geometry((16, 12, 8), (8, 4, 2), ((-0.21875, 0.78125), (0.5, 2.0), (-1.0, -0.75)), None, False),
    # 2-D, two levels, widths 1/120 and 1/100 (4 x 3 base blocks of 30 x 10)
    "G2O": Geometry((120, 30), (30, 10), ((-0.25, 0.75), (0.5, 0.8)), ((0.0, 0.5), (0.5, 0.65)), False),
    # 1-D, 4 blocks of 16, width 1/64, the whole domain right of 0
    "G1": Geometry((64,), (16,), ((0.25, 1.25),), None, True),
}


def boundary_sets(geom):
    """{name: six swarm boundary kinds} of a geometry: inactive axes stay periodic."""
    nd = len(GEOMETRIES[geom].nx)
    if nd == 1:
        return {k: v + (P,) * 4 for k, v in BOUNDARY_SETS_1D.items()}
    return {k: v[:2 * nd] + (P,) * (6 - 2 * nd) for k, v in BOUNDARY_SETS.items()}


def deck_overrides(nx, bx, extents, kinds, refine=None):
    """Deck overrides of a mesh: cells, cells per block, (min, max) per active axis, the six swarm boundary kinds
    (the mesh boundary is periodic where the swarm's is, outflow otherwise; periodic comes in pairs) and the
    level-1 region of the SMR decks."""
    out = {}
    for d in range(3):
        out[f"parthenon/mesh/nx{d + 1}"] = nx[d] if d < len(nx) else 1
        out[f"parthenon/meshblock/nx{d + 1}"] = bx[d] if d < len(bx) else 1
    for d, (lo, hi) in enumerate(extents):
        out[f"parthenon/mesh/x{d + 1}min"], out[f"parthenon/mesh/x{d + 1}max"] = lo, hi
    assert len(kinds) == 6
    for d in range(3):
        assert (kinds[2 * d] == P) == (kinds[2 * d + 1] == P), kinds
    for face, kind in zip(FACES, kinds):
        out[f"parthenon/swarm/{face}_bc"] = kind
        out[f"parthenon/mesh/{face}_bc"] = P if kind == P else O
    if refine is not None:
        out["parthenon/static_refinement1/level"] = 1
        for d, (lo, hi) in enumerate(refine):
            out[f"parthenon/static_refinement1/x{d + 1}min"] = lo
            out[f"parthenon/static_refinement1/x{d + 1}max"] = hi
    return out


def geometry_overrides(geom, kinds):
    g = GEOMETRIES[geom]
    return deck_overrides(g.nx, g.bx, g.extents, kinds, g.refine)


def mesh_of(geom, kinds=None):
    g = GEOMETRIES[geom]
    kinds = kinds or next(iter(boundary_sets(geom).values()))
    return Mesh.from_deck(load_deck("stepdiff_smr" if g.refine else "stepdiff", geometry_overrides(geom, kinds)))


def _whole_widths(mesh):
    """(every width a power of two, every block origin a whole number of widths): jb_mesh_create's condition
    for the exact-geometry kernels."""
    dx, x0 = mesh.blk_dx[:, :mesh.ndim], mesh.blk_xmin[:, :mesh.ndim]
    return bool(np.all(np.frexp(dx)[0] == 0.5)), bool(np.all(x0 / dx == np.rint(x0 / dx)))


# a later edit of the table must not silently move a case to another kernel family
for _name, _g in GEOMETRIES.items():
    _pow2, _whole = _whole_widths(mesh_of(_name))
    assert (_pow2 and _whole) == _g.exact, (_name, _pow2, _whole)
assert _whole_widths(mesh_of("G3X")) == (True, False)       # exact numbers, faces off the lattice of widths
assert _whole_widths(mesh_of("G3O"))[0] is False and _whole_widths(mesh_of("G2O"))[0] is False

SCAT = hs.SCAT
NP = "jaybenne/num_particles"
TAU = "jaybenne/tau_ddmc"

# (id, geometry, deck, overrides beside the geometry, pattern, cycles, family); the opacities and photon counts are
# those at which every non-periodic face is touched by at least 100 histories (tests/test_axis_host.py)
Case = namedtuple("Case", "id geom deck extra pattern cycles family")
CASES = [
    Case("G1-imc", "G1", "stepdiff", {NP: 8000, SCAT: 150.0}, "smooth", 2, "imc"),
    Case("G2S-imc", "G2S", "stepdiff_smr", {NP: 6000, SCAT: 100.0}, "smooth", 1, "imc"),
    Case("G3U-imc", "G3U", "stepdiff", {NP: 6000, SCAT: 20.0}, "smooth", 2, "imc"),
    Case("G3S-imc", "G3S", "stepdiff_smr", {NP: 20000, SCAT: 50.0}, "smooth", 1, "imc"),
    Case("G3O-imc", "G3O", "stepdiff", {NP: 6000, SCAT: 20.0}, "smooth", 2, "imc"),
    Case("G3X-imc", "G3X", "stepdiff", {NP: 6000, SCAT: 20.0}, "smooth", 2, "imc"),
    Case("G1-ddmc", "G1", "stepdiff_ddmc", {NP: 20000}, "palette3", 2, "ddmc"),
    Case("G2S-ddmc", "G2S", "stepdiff_smr_ddmc", {NP: 30000}, "palette2", 2, "ddmc"),
    Case("G3S-ddmc", "G3S", "stepdiff_smr_ddmc", {NP: 30000}, "stripes3", 2, "ddmc"),
    Case("G2S-hybrid", "G2S", "stepdiff_smr_hybrid", {NP: 30000, TAU: 10.0}, "islands", 1, "hybrid"),
    Case("G3S-hybrid", "G3S", "stepdiff_smr_hybrid", {NP: 30000, TAU: 10.0}, "islands", 1, "hybrid"),
    Case("G2O-hybrid", "G2O", "stepdiff_smr_hybrid", {NP: 30000}, "islands", 1, "hybrid"),
]
BY_ID = {c.id: c for c in CASES}
# the G3S case with absorption, for the kernels' !NOABS form
HOT_CASE = Case("G3S-hot", "G3S", "stepdiff_smr", dict(hs.ABSORBING, **{NP: 20000, SCAT: 50.0}), "hot_spots", 1, "imc")

# the palette each all-DDMC mesh runs the cell codes on and the bracket (lo, hi] its class count falls into, as
# hetero_states.DDMC_PALETTE / DDMC_CLASS_BRACKET.  The boundary kinds are part of the mesh: under S2 (x1 periodic)
# stripes3 has 270 distinct step records on G3S, more than the class table of 256 holds, stripes2 has 84
DDMC_PALETTE = {("G1-ddmc", "RO"): "palette3", ("G1-ddmc", "OR"): "palette3",
                ("G2S-ddmc", "S1"): "palette2", ("G2S-ddmc", "S2"): "palette2", ("G2S-ddmc", "S3"): "palette2",
                ("G3S-ddmc", "S1"): "stripes3", ("G3S-ddmc", "S2"): "stripes2", ("G3S-ddmc", "S3"): "stripes3"}
DDMC_CLASS_BRACKET = {"G1-ddmc": (0, 64), "G2S-ddmc": (64, 256), "G3S-ddmc": (64, 256)}
HYBRID_PATTERNS = hs.HYBRID_PATTERNS


def overrides(case, bset, kinds=None):
    """Deck overrides of a case under the boundary set named ``bset`` (or the six ``kinds`` given)."""
    kinds = kinds or boundary_sets(case.geom)[bset]
    return dict(geometry_overrides(case.geom, kinds), **case.extra)


def all_pairs():
    """Every (case, name of a boundary set)."""
    return [(c, s) for c in CASES for s in boundary_sets(c.geom)]
