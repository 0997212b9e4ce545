// jb_select.hpp -- which tracking kernel a transport call runs: a pure function of a few scalars of the
// call, the mesh and the context.  launch_transport (jb_api.hip) fills the inputs, launches what the
// plan says and reports variant_name(plan) through jb_last_transport_variant; tests/select_test.cpp
// walks the thresholds on the host.  Plain C++17: no HIP include.
#pragma once

#include <cstddef>
#include <cstdio>

#include "jb_limits.hpp"

namespace jb {

struct TransportInputs {
  // the call and the mesh
  int ndim = 1;
  bool ddmc = false;            // the entry point: jb_transport_photons_ddmc
  bool tally = false;           // fuse_census_tally
  bool gray = false;            // DevMesh::lam_abs != nullptr
  bool has_ddmc_cell = false;   // DevMesh::ddmc_cell != nullptr
  bool has_ddmc_code = false;   // DevMesh::ddmc_code != nullptr
  int nblocks = 1;              // resident blocks
  long long ntot = 0;           // cells per block, ghosts included
  long long last = 0;           // end of the particle range
  // host copies of DevMesh::not_all_ddmc[0..1], read back for a gray DDMC call on <= kLdsBlocks blocks and
  // looked at by no other: some cell takes IMC steps; the number of distinct step records
  bool not_all_ddmc = false;
  int nclass = 0;
  bool noabs = false;           // kappa_a == 0
  // the mesh geometry (jb_mesh)
  bool exact_geom = false, cell_ok = false, uniform_geom = false;
  bool equal_h = false;         // the active cell widths of block 0 are equal
  // the library: false in a build without k_imc_cell's unit-cell form (-DJB_IMC_PARENT_COORDS)
  bool unit_cell_form = true;
  // the context
  bool lean_arith = true, no_imc_cell = false;
  int coop_gather = -1;         // JB_COOP_GATHER
  bool ddmc_queues = true, ddmc_lds_codes = true;
  int max_classes = kMaxClasses;
};

enum class Family { k_transport, k_imc_cell, k_ddmc_all, k_ddmc_q, k_hybrid };

// The family's template arguments as runtime values; an argument the family does not have keeps its default.
// k_ddmc_all and k_ddmc_q are followed by k_hybrid<NDIM, TALLY, NOABS, 0, 0> on the photons they hand over;
// k_hybrid stands for its three launches (hybrid_phase below).
struct TransportPlan {
  Family family = Family::k_transport;
  int ndim = 1;
  bool ddmc = false, tally = false;
  int gray = 0;                    // k_transport GRAY: 0 frequency-dependent, 1 gray, 2 gray without absorption
  bool exact = false, lean = false;   // k_transport
  bool noabs = false;              // k_imc_cell, k_hybrid
  bool uniform = false;            // k_imc_cell
  // k_imc_cell: position and direction in units of the half cell width (UNITCELL); every active width equal (EQUALH)
  bool unit_cell = false, equal_h = false;
  int gather = 0;                  // k_ddmc_all
  bool lcodes = false;             // k_ddmc_q
  int mode = 0;                    // k_hybrid: 0 exact arithmetic, 1 lean, 2 lean on exact geometry, 3 lean, cell-local
  size_t dyn_lds = 0;              // dynamic LDS bytes (k_ddmc_all, k_ddmc_q)
  bool occ_cap3 = false;           // at most 3 workgroups per CU whatever the occupancy query says
};

inline TransportPlan select_transport(const TransportInputs &in) {
  TransportPlan p;
  p.ndim = in.ndim;
  p.ddmc = in.ddmc;
  p.tally = in.tally;
  // Gray opacities: UpdateDerivedTransportFields has packed the cell records and left a flag on
  // the device saying whether every cell takes DDMC steps.  Every cell: k_ddmc_all; a mix of IMC
  // and DDMC cells: k_hybrid.  Both keep the per-block tables in LDS, so meshes with more resident
  // blocks than fit there stay with the general kernel below.
  if (in.ddmc && in.gray && in.has_ddmc_cell && in.nblocks <= kLdsBlocks) {
    p.noabs = in.noabs;
    if (in.not_all_ddmc) {
      // A mix of IMC and DDMC cells, three launches: k_hybrid<.., PHASE 1> follows the photons in
      // IMC cells (its service phase also takes the albedo step of a photon that enters a DDMC
      // cell) and parks those that settle in DDMC cells; <.., PHASE 2> follows these and parks the
      // ones that leak back into IMC cells; <.., PHASE 0>, which runs both event loops, finishes
      // that remainder -- the photons that keep changing regime at the interface (alternating
      // phases 1 and 2 until nothing is left costs one launch per change of regime of the most
      // persistent photon: measured ~80 rounds of ~0.5 ms on BASELINE configs[4]).
      p.family = Family::k_hybrid;
      p.mode = !in.lean_arith ? 0 : (in.exact_geom && in.cell_ok && !in.no_imc_cell) ? 3 : in.exact_geom ? 2 : 1;
      return p;
    }
    const unsigned long long ncell_all = (unsigned long long)in.nblocks * (unsigned long long)in.ntot;
    // The quad-cooperative gather (jb_kernel_ddmc.hpp) addresses the step records with 32-bit byte
    // offsets; it pays once the records no longer sit in the CU's vector L1 (measured, ms per
    // 1e8 histories: 128^3 cells 31.5 -> 27.9, 64^3 7.2 -> 6.9, 32^3 equal, 128 cells in 1-D
    // 11.6 -> 13.1: there every lookup hits L1 and the detour through LDS only adds latency).
    const unsigned long long rec_bytes = 64ull * ncell_all;
    // (record numbers are 32-bit: fewer than 2^32 resident cells; 64-bit addresses when the records
    // span 4 GiB or more -- JB_COOP_GATHER=2 forces that form on any table, for the parity tests)
    const bool coop = rec_bytes < (64ull << 32) &&
                      (in.coop_gather >= 0 ? in.coop_gather >= 1 : rec_bytes >= (1ull << 20));
    const bool wide = coop && (rec_bytes >= (1ull << 32) || in.coop_gather == 2);
    // ... and a mesh of at most kLdsRecCells cells (the reference's 1-D decks) keeps its records in
    // LDS: 12.3 -> 10.3 ms per 1e8 histories on BASELINE configs[2] as shipped
    const bool in_lds = !coop && in.coop_gather < 0 && (long long)ncell_all <= (long long)kLdsRecCells;
    // ... and everything between with at most kMaxClasses DISTINCT step records (k_ddmc_pack counts them
    // every cycle: the gray decks have a handful) gathers a 4-byte cell code per step, the records in LDS
    // (JB_COOP_GATHER=4 also on the smallest meshes; 0 / 1 / 2 keep the 64-byte forms, for tests and A/B)
    const bool codes_ok = in.has_ddmc_code && in.nclass >= 1 && in.nclass <= in.max_classes;
    // ... and, with the codes, the wave's photons staged through queues in LDS (k_ddmc_q, jb_kernel_ddmc_q.hpp:
    // the event loop at full width, the service phase in whole batches) -- any mesh size, up to kQBlocks
    // resident blocks and 2^32 slots; JB_DDMC_QUEUES=0 keeps k_ddmc_all
    const bool queues = codes_ok && in.ddmc_queues && in.coop_gather < 0 && in.nblocks <= kQBlocks &&
                        in.last <= (1ll << 32);
    const bool codes = queues || (codes_ok && (in.coop_gather == 4 || (in.coop_gather < 0 && !in_lds)));
    p.family = queues ? Family::k_ddmc_q : Family::k_ddmc_all;
    p.gather = codes ? 4 : (coop ? (wide ? 3 : 1) : (in_lds ? 2 : 0));
    // ... the codes themselves in LDS on a mesh of at most kLdsCodeCells cells (JB_DDMC_LDS_CODES=0: not)
    // (and at most 64 classes: tally 8 KB + classes 4 KB + codes 4 KB + 37.7 KB static stay under the 64 KB a
    // workgroup may have; with up to kMaxClasses = 256 records, 16 KB, the codes would not fit beside them)
    p.lcodes = queues && in.ddmc_lds_codes && (long long)ncell_all <= (long long)kLdsCodeCells && in.nclass <= 64;
    // (dynamic shared memory: the tally of a mesh with <= kLdsTally cells, resident blocks' ghosts included,
    // then the distinct step records or the records of a small mesh, then the codes)
    p.dyn_lds = (size_t)((in.tally && (long long)ncell_all <= (long long)kLdsTally ? sizeof(double) * ((ncell_all + 1) / 2 * 2) : 0) +
                         (codes ? 64 * (unsigned long long)in.nclass : (in_lds ? 64 * ncell_all : 0)) +
                         (p.lcodes ? sizeof(unsigned) * ((ncell_all + 1) / 2 * 2) : 0));
    // (four 16-byte loads per lane on a table that does not sit in L1 -- only a table of >= 4 GiB, or
    // JB_COOP_GATHER=0, gets here -- saturate the vector L1's look-ups: a fourth wave per SIMD then
    // costs time, 38.2 against 31.5 ms per 1e8 histories on the 160 MB table)
    p.occ_cap3 = p.gather == 0 && rec_bytes >= (1ull << 20);
    return p;
  }
  const bool gray_imc = in.gray && !in.ddmc;
  // lean arithmetic: the step in cell-local coordinates (jb_kernel_imc.hpp).  It does not care what the
  // cell widths are: only its conversions to and from the swarm's coordinates round, by an ulp of the position.
  if (gray_imc && in.lean_arith && !in.no_imc_cell && in.cell_ok) {
    p.family = Family::k_imc_cell;
    p.noabs = in.noabs;
    p.uniform = in.uniform_geom;
    // ... in units of the half cell width where that is one wave-uniform power of two per axis (every stepdiff
    // deck: the scaling is exact, the results are the unscaled form's bit for bit, jb_kernel_imc.hpp); other
    // uniform widths (1/24), blocks of several sizes keep the form above.  The name below does not say which.
    p.unit_cell = in.unit_cell_form && in.uniform_geom && in.exact_geom;
    p.equal_h = p.unit_cell && in.equal_h;
    return p;
  }
  // gray opacity with kappa = 0 (opacity_model = none): sigma_a = rho * 0 in every cell
  p.gray = !in.gray ? 0 : (in.noabs ? 2 : 1);
  // (EXACT and LEAN are variants of the gray IMC kernels)
  p.exact = gray_imc && in.exact_geom;
  p.lean = gray_imc && in.lean_arith;
  return p;
}

// The NOABS, MODE arguments of the plan's k_hybrid launch of one PHASE.  PHASE 2, the DDMC loop alone, has neither
// an absorption branch of its own nor IMC arithmetic: it exists as <.., true, 0, 2> only.  (The launch behind
// k_ddmc_all / k_ddmc_q is PHASE 0 of a plan whose mode is 0.)
struct HybridPhase {
  bool noabs;
  int mode;
};
inline HybridPhase hybrid_phase(const TransportPlan &p, int phase) {
  return phase == 2 ? HybridPhase{true, 0} : HybridPhase{p.noabs, p.mode};
}

// What jb_last_transport_variant reports.  k_transport: NDIM, TALLY, GRAY, EXACT geometry, LEAN arithmetic (the
// DDMC flag is the entry point that was called); k_imc_cell: NDIM, TALLY, NOABS and the arithmetic; the all-DDMC
// kernels: NDIM, TALLY and how the step records are gathered; k_hybrid: NDIM and the IMC phase's MODE.
inline void variant_name(const TransportPlan &p, char *buf, size_t n) {
  const auto b = [](bool v) { return v ? "true" : "false"; };
  switch (p.family) {
  case Family::k_transport:
    snprintf(buf, n, "k_transport<%d, %s, %d, %s, %s>", p.ndim, b(p.tally), p.gray, b(p.exact), b(p.lean));
    break;
  case Family::k_imc_cell:
    snprintf(buf, n, "k_imc_cell<%d, %s, %s, lean>", p.ndim, b(p.tally), b(p.noabs));
    break;
  case Family::k_ddmc_all: {
    static const char *const gathers[5] = {"", ", quad gather", ", records in LDS", ", quad gather", ", cell codes"};
    snprintf(buf, n, "k_ddmc_all<%d, %s%s>", p.ndim, b(p.tally), gathers[p.gather]);
    break;
  }
  case Family::k_ddmc_q:
    snprintf(buf, n, "k_ddmc_all<%d, %s, cell codes, queues%s>", p.ndim, b(p.tally), p.lcodes ? ", codes in LDS" : "");
    break;
  case Family::k_hybrid: {
    static const char *const modes[4] = {"exact", "lean", "lean, exact geometry", "lean, cell-local"};
    snprintf(buf, n, "k_hybrid<%d, %s>", p.ndim, modes[p.mode]);
    break;
  }
  }
}

}  // namespace jb
