// jaybenne_amd.hpp -- C++ host-side mirror of the reference's package / task interface
// (reference src/jaybenne/jaybenne.hpp:48-78) over the C ABI of jaybenne_amd.h.
//
// The reference is a C++ package driven by a C++ host application (src/mcblock).  This header
// is what such a host includes: the task functions keep the reference's names, argument order
// and TaskStatus results; PARTHENON_REQUIRE / PARTHENON_FAIL conditions surface as
// jaybenne_amd::Error.  It needs nothing but the C ABI (no HIP headers, no Parthenon): the host
// owns every device buffer and hands raw device pointers over, exactly as Parthenon's packs do
// for the reference.  examples/mcblock_amd.cpp is a complete host application written on it;
// jaybenne_amd/jaybenne.py is the same mirror in Python (and adds the multi-rank hand-off).
//
// RadiationStep comes in two overloads: RadiationStep(md, t_start, dt) is the task list of
// jaybenne.cpp:104-138 for a mesh held by one rank, where one transport launch resolves every block
// crossing in flight; RadiationStep(md, t_start, dt, transport, rank, nranks) runs it on every rank of a
// block-partitioned mesh, the iterate-sublist (transport, hand-off, completion test) inside one library
// call (jb_radiation_step_ranks) over the host's jb_exchange_transport (MPI, RCCL, ...).  Halo refresh
// and replicated meshes stay with the host (examples/handoff_mpi.cpp, jaybenne_amd/jaybenne.py).
#ifndef JAYBENNE_AMD_HPP_
#define JAYBENNE_AMD_HPP_

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <functional>
#include <limits>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "jaybenne_amd.h"

namespace jaybenne_amd {

using Real = double;

// parthenon::TaskStatus as the reference's tasks return it (jaybenne.cpp:34,55-56)
enum class TaskStatus { complete, incomplete, iterate };
enum class SourceType { thermal, emission };     // jaybenne.hpp:56
enum class SourceStrategy { uniform, energy };   // jaybenne.hpp:55

struct Error : std::runtime_error {
  jb_status status;
  Error(jb_status st, const std::string &what) : std::runtime_error(what), status(st) {}
};

// the checked library (libjaybenne_amd_checked.so): a step that violated a transport invariant
struct InvariantError : Error {
  using Error::Error;
};

inline TaskStatus Check(jb_status st) {
  if (st == JB_ERR_INVARIANT) throw InvariantError(st, jb_last_error());
  if (st < 0) throw Error(st, jb_last_error());
  return st == JB_ITERATE ? TaskStatus::iterate
                          : (st == JB_INCOMPLETE ? TaskStatus::incomplete : TaskStatus::complete);
}

// The StateDescriptor role (jaybenne.cpp:158-266): owns the package context; parameters by name.
class StateDescriptor {
 public:
  StateDescriptor(const jb_params &p, const jb_opacity &opacity, const jb_scattering &scattering,
                  const jb_eos &eos, int device = 0)
      : params_(p) {
    Check(jb_initialize(&p, &eos, &opacity, &scattering, device, &ctx_));
  }
  ~StateDescriptor() { jb_finalize(ctx_); }
  StateDescriptor(const StateDescriptor &) = delete;
  StateDescriptor &operator=(const StateDescriptor &) = delete;

  jb_context *ctx() const { return ctx_; }
  const jb_params &params() const { return params_; }
  int seed() const { return jb_param_seed(ctx_); }  // Param<int>("seed"), jaybenne.cpp:187-190
  // arithmetic of the gray IMC tracking step: JB_ARITH_LEAN (default) or JB_ARITH_EXACT
  void SetArithmetic(int mode) { Check(jb_set_arithmetic(ctx_, mode)); }
  void SetCellOrder(int mode) { Check(jb_set_cell_order(ctx_, mode)); }
  int Arithmetic() const { return jb_get_arithmetic(ctx_); }

 private:
  jb_context *ctx_ = nullptr;
  jb_params params_;
};

// jaybenne::Initialize(pin, opacity, scattering, eos) -- jaybenne.hpp:50-52
inline std::shared_ptr<StateDescriptor> Initialize(const jb_params &p, const jb_opacity &opacity,
                                                   const jb_scattering &scattering,
                                                   const jb_eos &eos, int device = 0) {
  return std::make_shared<StateDescriptor>(p, opacity, scattering, eos, device);
}

// The energy ledger of one radiation cycle (jaybenne_amd.h: jb_energy_ledger), summed over the ranks, with the
// census energy the cycle started from and the residual of
//   e_start + e_sourced = e_census + e_absorbed + sum_f e_escaped[f] + e_escaped_unclassified
// relative to its left-hand side.  LedgerResidual is a fixed sequence of IEEE operations, the one
// jaybenne_amd/_lib.py: ledger_residual performs: both hosts print the same bits.
struct EnergyLedger : jb_energy_ledger {
  double e_start = 0.0, residual = 0.0;
};
// one combed cycle (MeshData::comb_history; the keys of the Python host's md.comb_history)
// one cycle of the boundary source (MeshData::boundary_source_history; the keys of the Python host's
// md.boundary_source_history): energy and photons sourced through each domain face
struct BoundarySourceCycle {
  int64_t cycle;
  double e_face[6];
  int64_t n_face[6];
};
struct CombRecord {
  int64_t cycle, n_before, n_after, n_new_ids;
  uint64_t id_base;
  int64_t cells_combed, max_per_cell;
  double e_before, e_after;
  // a cycle of the global comb (CombCensusGlobal; the Python host's mode = "global") fills these too
  bool global = false;
  int64_t cells_thinned = 0, cells_split = 0, max_target = 0;
  double w_total = 0.0, scale = 0.0;
};
inline double LedgerResidual(const jb_energy_ledger &l, double e_start) {
  const double lhs = e_start + l.e_sourced;
  double r = lhs - l.e_census;
  r -= l.e_absorbed;
  for (int f = 0; f < 6; ++f) r -= l.e_escaped[f];
  r -= l.e_escaped_unclassified;
  return lhs > 0.0 ? (r < 0.0 ? -r : r) / lhs : 0.0;
}

// The MeshData<Real> + swarm role: what one rank's tasks operate on.  The host fills `view`
// (host arrays of per-block DEVICE pointers) and `swarm` (device arrays it allocated);
// `reserve(n)` is the host's pool growth (Swarm::AddEmptyParticles, sourcing.cpp:123-131): it
// must leave swarm.capacity >= n with the first swarm.n particles preserved.
class MeshData {
 public:
  MeshData(std::shared_ptr<StateDescriptor> pkg, const jb_mesh_view &view, int32_t *prefix_dev,
           std::function<void(jb_swarm_view &, int64_t)> reserve)
      : pkg_(std::move(pkg)), nblocks_(view.nblocks), nblocks_total_(view.nblocks_total),
        gid_(view.gid, view.gid + view.nblocks), prefix_dev_(prefix_dev), reserve_(std::move(reserve)) {
    Check(jb_mesh_create(pkg_->ctx(), &view, &mesh_));
  }
  ~MeshData() { jb_mesh_destroy(mesh_); }
  MeshData(const MeshData &) = delete;
  MeshData &operator=(const MeshData &) = delete;

  StateDescriptor &pkg() const { return *pkg_; }
  jb_context *ctx() const { return pkg_->ctx(); }
  jb_mesh *mesh() const { return mesh_; }
  int nblocks() const { return nblocks_; }
  int nblocks_total() const { return nblocks_total_; }
  const std::vector<int32_t> &gid() const { return gid_; }   // global id of each resident block
  int32_t *prefix_dev() const { return prefix_dev_; }
  void Reserve(int64_t n) {
    if (n > swarm.capacity) reserve_(swarm, n);
    if (n > swarm.capacity) throw Error(JB_ERR_CAPACITY, "swarm pool could not be grown");
  }

  // jb_rank_comm::reserve of the multi-rank RadiationStep: the host's pool growth, 0 = success
  static int ReserveTrampoline(void *host, jb_swarm_view *swarm, int64_t n) {
    try {
      static_cast<MeshData *>(host)->reserve_(*swarm, n);
    } catch (...) {
      return 1;
    }
    return swarm->capacity >= n ? 0 : 1;
  }

  jb_swarm_view swarm{};   // n, capacity and the device arrays
  uint64_t next_id = 0;    // first unused random-stream id
  uint64_t cycle = 0;      // RadiationStep counter (keys the per-cell rounding streams: SourceEpoch); 0 = initialisation
  int64_t events = 0;      // tracking events so far
  // DefragParticles: -1 (default) when the library's policy asks for it (jb_defrag_policy: a cycle
  // that costs 10 % more per event than the best one since the last sort); k > 0 after every k-th
  // RadiationStep; 0 never, as the reference (slot order then stays what the task list makes it)
  int defrag_interval = -1;
  int defrags = 0;
  int steps_since_defrag = 0;
  jb_step_report last_step{};   // what the last multi-rank RadiationStep did on this rank
  // energy ledger (EnableLedger, or JB_LEDGER=1 in the environment): the last cycle's and every cycle's
  EnergyLedger ledger{};
  std::vector<EnergyLedger> ledger_history;
  bool ledger_started = false;  // ledger_e0 holds the census energy the next cycle starts from
  double ledger_e0 = 0.0;
  // census comb (CombCensus; jaybenne_amd.h: jb_comb_census_plan): a cell that ends a cycle with more than
  // comb_trigger photons comes out with comb_target; 0 = off (the reference: no population control)
  int64_t comb_target = 0, comb_trigger = 0;
  std::vector<CombRecord> comb_history;   // one record per cycle whose comb changed the swarm
  // global census comb (CombCensusGlobal; jaybenne_amd.h: jb_comb_census_weigh): the whole mesh is held near
  // census_total_target photons of equal weight; 0 = off.  Not together with comb_target.
  int64_t census_total_target = 0, census_split_max = 64;
  double census_total_band = 2.0;
  // boundary source (SetBoundarySource; jaybenne_amd.h: jb_source_boundary_count): N_b photons per cycle over all
  // source faces of the WHOLE mesh, and the number of source face cells of the whole mesh (SetBoundarySource sets it
  // for a rank that holds the whole mesh; a host with several ranks stores the sum of jb_boundary_face_cells)
  int64_t bsource_num_particles = 0, bsource_face_cells_total = 0;
  std::vector<BoundarySourceCycle> boundary_source_history;   // one record per cycle, this rank's part
  // counted by SourcePhotons(emission), filled by SourceBoundaryPhotons
  struct {
    bool valid = false;
    uint64_t cycle = 0;
    std::vector<int32_t> nper;
    std::vector<uint64_t> id_base;
    jb_boundary_source_plan plan{};
  } bsource_pending;

 private:
  std::shared_ptr<StateDescriptor> pkg_;
  jb_mesh *mesh_ = nullptr;
  int nblocks_, nblocks_total_;
  std::vector<int32_t> gid_;
  int32_t *prefix_dev_;
  std::function<void(jb_swarm_view &, int64_t)> reserve_;
};

// T = ceil(trigger K) of the deck keys <jaybenne_amd> census_per_cell_max = K and census_comb_trigger (every
// host forms it this way)
inline int64_t CombTrigger(int64_t target, double trigger) {
  if (target < 0) throw std::invalid_argument("census_per_cell_max must be >= 0");
  if (!(trigger >= 1.0)) throw std::invalid_argument("census_comb_trigger must be >= 1");
  return (int64_t)std::ceil(trigger * (double)target);
}

// ---- host-side arithmetic of SourcePhotons shared by every host (this header's single-rank tasks,
// examples/handoff_mpi.cpp across MPI ranks, adapters/parthenon/jaybenne_amd_tasks.cpp) ----------
// Random-stream ids are GLOBAL creation indices -- block-major over the global block ids, then the
// order within the block -- so that results do not depend on the block -> rank partition.
//   nper_local[b]   new photons of resident block b of this rank (jb_source_photons_count)
//   gid[b]          its global block id
//   all_counts[g]   new photons of every global block g (the sum of the ranks' contributions;
//                   one rank: its own counts scattered by gid)
// Result: slot_base[b] (first swarm slot of block b's new photons, appended after the n_now live
// ones), id_base[b] (stream id of its first new photon), total_local, and the first unused id
// after this source call (identical on every rank).
struct SourcePlan {
  std::vector<int64_t> slot_base;
  std::vector<uint64_t> id_base;
  int64_t total_local = 0;
  uint64_t next_id = 0;
  // PlanSourceWithBoundary: the same for the boundary photons of the call (empty otherwise)
  std::vector<int64_t> slot_base_boundary;
  std::vector<uint64_t> id_base_boundary;
};
inline SourcePlan PlanSource(const std::vector<int32_t> &nper_local, const std::vector<int32_t> &gid,
                             const std::vector<long long> &all_counts, uint64_t next_id,
                             int64_t n_now) {
  SourcePlan pl;
  const size_t nb = nper_local.size();
  std::vector<uint64_t> excl(all_counts.size());
  uint64_t run = 0;
  for (size_t g = 0; g < all_counts.size(); ++g) { excl[g] = run; run += (uint64_t)all_counts[g]; }
  pl.slot_base.resize(nb);
  pl.id_base.resize(nb);
  for (size_t b = 0; b < nb; ++b) {
    pl.slot_base[b] = n_now + pl.total_local;
    pl.id_base[b] = next_id + excl[(size_t)gid[b]];
    pl.total_local += nper_local[b];
  }
  pl.next_id = next_id + run;
  return pl;
}
// ... and with the boundary source on (jaybenne_amd.h: jb_source_boundary_count): block b takes
// nper_emission[b] + nper_boundary[b] CONSECUTIVE ids, the emission photons first; all_counts[g] is the sum of
// both for global block g.  In the swarm the boundary photons lie behind all emission photons of the call.
// total_local counts both.
inline SourcePlan PlanSourceWithBoundary(const std::vector<int32_t> &nper_emission, const std::vector<int32_t> &nper_boundary,
                                         const std::vector<int32_t> &gid, const std::vector<long long> &all_counts,
                                         uint64_t next_id, int64_t n_now) {
  SourcePlan pl = PlanSource(nper_emission, gid, all_counts, next_id, n_now);
  const size_t nb = nper_emission.size();
  pl.slot_base_boundary.resize(nb);
  pl.id_base_boundary.resize(nb);
  int64_t run = 0;
  for (size_t b = 0; b < nb; ++b) {
    pl.slot_base_boundary[b] = n_now + pl.total_local + run;
    pl.id_base_boundary[b] = pl.id_base[b] + (uint64_t)nper_emission[b];
    run += nper_boundary[b];
  }
  pl.total_local += run;
  return pl;
}
// The key of the per-cell rounding streams (`epoch` of jb_source_photons_count) as a function of
// the cycle (0 = initialisation, k = the k-th RadiationStep) and the source type, so that every rank
// of every host -- whatever the number of blocks it calls the source for -- uses the same one: 0 for
// the initial thermal source, k for the emission source of cycle k -- the order in which a run makes
// its source calls (jaybenne.cpp:104-105, 570-578); a thermal source inside a cycle, which no task
// list of the reference makes, gets a key of its own.  (jb_source_photons_count accepts epochs below
// 2^20: half a million cycles.)
inline uint32_t SourceEpoch(uint64_t cycle, SourceType st) {
  if (st == SourceType::emission) return (uint32_t)cycle;
  return cycle == 0 ? 0u : (uint32_t)((1u << 19) | cycle);
}

// ---- block -> rank partition (several ranks; jaybenne_amd/mesh.py Mesh.partition is the same algorithm,
// operation for operation, so that a C++ host and the Python host deal the same blocks to the same rank) --
// Contiguous runs of the Z-ordered block list.  cost[b] = the tracking work of block b for one cycle
// (photons sourced there x events per history: BlockCost below); the runs are the split with the
// SMALLEST LARGEST load, found exactly by dynamic programming over the prefix sums (a cycle lasts as
// long as its slowest rank); then a boundary that separates the children of one parent (group[b] equal
// for consecutive blocks) moves to the nearer end of that family if the largest load stays within
// 1 + sibling_slack of the optimum.  The reference inherits Parthenon's balancer with unit cost per
// block (jaybenne.cpp:92-95): pass cost = all ones for that.
// Returns bounds[0 .. nranks]: rank r owns blocks bounds[r] .. bounds[r + 1] - 1.
inline std::vector<int32_t> PartitionBlocks(const std::vector<double> &cost, int nranks,
                                            const std::vector<int64_t> &group, double sibling_slack = 0.10) {
  const int nb = (int)cost.size();
  if (nranks < 1 || nranks > nb) throw Error(JB_ERR_INVALID, "cannot spread the blocks over that many ranks");
  std::vector<double> S((size_t)nb + 1, 0.0);
  for (int b = 0; b < nb; ++b) {
    if (!(cost[b] > 0.0) || !std::isfinite(cost[b])) throw Error(JB_ERR_INVALID, "block costs must be positive and finite");
    S[(size_t)b + 1] = S[(size_t)b] + cost[b];
  }
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<std::vector<double>> best((size_t)nranks, std::vector<double>((size_t)nb + 1, inf));
  std::vector<std::vector<int32_t>> cut((size_t)nranks, std::vector<int32_t>((size_t)nb + 1, 0));
  for (int i = 1; i <= nb; ++i) best[0][(size_t)i] = S[(size_t)i];
  for (int r = 1; r < nranks; ++r)
    for (int i = r + 1; i <= nb; ++i) {
      double bv = inf;
      int32_t bj = r;
      for (int j = r; j < i; ++j) {
        const double a = best[(size_t)r - 1][(size_t)j], c = S[(size_t)i] - S[(size_t)j];
        const double v = a > c ? a : c;
        if (v < bv) { bv = v; bj = j; }                    // (the first of equal minima)
      }
      best[(size_t)r][(size_t)i] = bv;
      cut[(size_t)r][(size_t)i] = bj;
    }
  std::vector<int32_t> bounds((size_t)nranks + 1, 0);
  bounds[(size_t)nranks] = nb;
  for (int r = nranks - 1; r >= 1; --r) bounds[(size_t)r] = cut[(size_t)r][(size_t)bounds[(size_t)r + 1]];
  const double optimum = best[(size_t)nranks - 1][(size_t)nb];
  auto largest = [&](const std::vector<int32_t> &bd) {
    double m = 0.0;
    for (int r = 0; r < nranks; ++r) {
      const double l = S[(size_t)bd[(size_t)r + 1]] - S[(size_t)bd[(size_t)r]];
      m = l > m ? l : m;
    }
    return m;
  };
  for (int r = 1; r < nranks; ++r) {
    const int q = bounds[(size_t)r];
    if (group[(size_t)q - 1] != group[(size_t)q]) continue;   // not inside a family
    int lo = q, hi = q;
    while (lo > 0 && group[(size_t)lo - 1] == group[(size_t)q]) --lo;
    while (hi < nb && group[(size_t)hi] == group[(size_t)q]) ++hi;
    bool have = false;
    double bl = 0.0;
    int bd_dist = 0, bc = q;
    for (int cand : {lo, hi}) {
      if (!(bounds[(size_t)r - 1] < cand && cand < bounds[(size_t)r + 1])) continue;
      std::vector<int32_t> bd = bounds;
      bd[(size_t)r] = cand;
      const double l = largest(bd);
      const int dist = cand > q ? cand - q : q - cand;
      // (order of the Python host's tuples: load, distance, position)
      if (!have || l < bl || (l == bl && (dist < bd_dist || (dist == bd_dist && cand < bc)))) {
        have = true; bl = l; bd_dist = dist; bc = cand;
      }
    }
    if (have && bl <= (1.0 + sibling_slack) * optimum) bounds[(size_t)r] = bc;
  }
  return bounds;
}

// group[] of PartitionBlocks from the Z-ordered leaf list: level[b] and the logical location lloc[3 b + d]
// at that level (Mesh.sibling_groups of the Python host)
inline std::vector<int64_t> SiblingGroups(int ndim, const std::vector<int32_t> &level, const std::vector<int32_t> &lloc) {
  std::vector<int64_t> group(level.size());
  int64_t g = -1;
  bool have_prev = false;
  int32_t pl = 0, pp[3] = {0, 0, 0};
  for (size_t b = 0; b < level.size(); ++b) {
    bool same = false;
    int32_t par[3] = {0, 0, 0};
    if (level[b] > 0) {
      for (int d = 0; d < 3; ++d) par[d] = d < ndim ? lloc[3 * b + d] >> 1 : 0;
      same = have_prev && pl == level[b] && pp[0] == par[0] && pp[1] == par[1] && pp[2] == par[2];
    }
    if (!same) ++g;
    group[b] = g;
    have_prev = level[b] > 0;
    pl = level[b];
    for (int d = 0; d < 3; ++d) pp[d] = par[d];
  }
  return group;
}

// The tracking work of a block for one cycle, in events per photon it starts with (mcblock.block_costs of
// the Python host, the same expressions): c dt (sigma_s + sigma_a + sum_d 1 / (2 dx_d)) in a block that
// takes IMC steps; c dt (sigma_a + sum_d 2 P / dx_d), P = 1 / (3 (sigma_a + sigma_s) dx_d), in one that takes
// DDMC steps (dx_min (sigma_a + sigma_s) > tau_ddmc, transport_ddmc.cpp:135).  With the `uniform` source
// strategy every block starts with the same number of photons (sourcing.cpp:68-69), so this IS the cost.
inline double BlockCost(int ndim, const double dx[3], double c_dt, double sig_a, double sig_s, bool use_ddmc,
                        double tau_ddmc) {
  double dmin = dx[0];
  for (int d = 1; d < ndim; ++d) dmin = dx[d] < dmin ? dx[d] : dmin;
  double per_history;
  if (use_ddmc && dmin * (sig_a + sig_s) > tau_ddmc) {
    double leak = 0.0;
    for (int d = 0; d < ndim; ++d) leak += 2.0 * (2.0 / (3.0 * 2.0 * (sig_a + sig_s) * dx[d])) / dx[d];
    per_history = c_dt * (sig_a + leak);
  } else {
    double cross = 0.0;
    for (int d = 0; d < ndim; ++d) cross += 0.5 / dx[d];
    per_history = c_dt * (sig_s + sig_a + cross);
  }
  return per_history > 1.0 ? per_history : 1.0;
}

// Replicated mesh, split particles (jb_source_photons_fill_range; jaybenne_amd/jaybenne.py rank_share): of
// the nper[b] new photons of block b, rank `rank` of `nranks` sources count[b] starting at first[b].
inline void RankShare(const std::vector<int32_t> &nper, int rank, int nranks, std::vector<int32_t> *first,
                      std::vector<int32_t> *count) {
  first->resize(nper.size());
  count->resize(nper.size());
  for (size_t b = 0; b < nper.size(); ++b) {
    const int64_t n = nper[b];
    const int64_t f = (n * rank) / nranks;
    (*first)[b] = (int32_t)f;
    (*count)[b] = (int32_t)((n * (rank + 1)) / nranks - f);
  }
}

// ---- halo copies (several ranks; shared by examples/handoff_mpi.cpp, the Parthenon adapter and,
// restated in numpy, the Python host: jaybenne_amd/mesh.py Mesh.neighbours, halo.py) -------------
// A rank keeps read-only copies of the other ranks' blocks that TOUCH one of its own (face, edge or
// corner, through periodic boundaries too).  A photon that wanders across the rank boundary keeps
// being tracked in flight and is handed to the owner of the block it ends in ONCE, when its history
// is over: two transport iterations per cycle instead of one per rank-boundary crossing of the most
// persistent photon (reference jaybenne.cpp:113-131 iterates ~80 times on BASELINE configs[1]).
//   Mesh description (what jb_mesh_view holds for ALL blocks of the mesh, by global id):
//   leaf_map over the finest-level leaf grid nleaf[3], block corners, mesh boundary kinds
//   (periodic[2 d + side]), owner[g].
// Result: resident_gids = this rank's blocks (ascending global id) followed by its halo copies
// (ascending), owned[] for jb_mesh_view::owned, local_index[g] (-1: not resident).
struct HaloPlan {
  std::vector<int32_t> resident_gids, owned, local_index;
  int nowned = 0;
};
struct MeshTopology {
  int ndim = 1;
  double gmin[3] = {0, 0, 0}, gmax[3] = {1, 1, 1};
  int nleaf[3] = {1, 1, 1};
  bool periodic[6] = {false, false, false, false, false, false};
  const int32_t *leaf_map = nullptr;   // [nleaf[2]][nleaf[1]][nleaf[0]] -> global block id
  int nblocks_total = 0;
  const double *blk_xmin = nullptr, *blk_xmax = nullptr;   // [nblocks_total][3]
  const int32_t *owner = nullptr;                           // [nblocks_total]
  const int32_t *level = nullptr;                           // [nblocks_total] (FaceNeighbourLevels only)
};
// jb_mesh_view::blk_nbr_lev of block g: the level of the block behind each face (2 axis + upper), the
// block's own level at a mesh boundary that is not periodic and on an inactive axis
// (jaybenne.cpp:341-351) -- what a host that keeps a HALO COPY of g has to supply for it
inline void FaceNeighbourLevels(const MeshTopology &T, int g, int32_t out[6]) {
  for (int f = 0; f < 6; ++f) out[f] = T.level[g];
  long long l0[3] = {0, 0, 0}, cnt[3] = {1, 1, 1};
  for (int d = 0; d < T.ndim; ++d) {
    const double fine = (T.gmax[d] - T.gmin[d]) / (double)T.nleaf[d];
    l0[d] = (long long)std::llround((T.blk_xmin[3 * g + d] - T.gmin[d]) / fine);
    cnt[d] = (long long)std::llround((T.blk_xmax[3 * g + d] - T.blk_xmin[3 * g + d]) / fine);
  }
  for (int d = 0; d < T.ndim; ++d)
    for (int up = 0; up < 2; ++up) {
      long long l[3] = {l0[0], l0[1], l0[2]};   // (any leaf behind the face: 2:1 balance, one level there)
      l[d] = up ? l0[d] + cnt[d] : l0[d] - 1;
      if (l[d] < 0) { if (!T.periodic[2 * d]) continue; l[d] += T.nleaf[d]; }
      else if (l[d] >= T.nleaf[d]) { if (!T.periodic[2 * d + 1]) continue; l[d] -= T.nleaf[d]; }
      out[2 * d + up] = T.level[T.leaf_map[(l[2] * T.nleaf[1] + l[1]) * T.nleaf[0] + l[0]]];
    }
}
// leaf blocks that touch block b: the blocks under the one-leaf-wide shell of leaves around it
inline void TouchingBlocks(const MeshTopology &T, int b, std::vector<int32_t> *out) {
  long long lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};   // the shell's leaf range per axis, inclusive
  for (int d = 0; d < 3; ++d) {
    if (d >= T.ndim) continue;
    const double fine = (T.gmax[d] - T.gmin[d]) / (double)T.nleaf[d];
    lo[d] = (long long)std::llround((T.blk_xmin[3 * b + d] - T.gmin[d]) / fine) - 1;
    hi[d] = (long long)std::llround((T.blk_xmax[3 * b + d] - T.gmin[d]) / fine);
  }
  for (long long k = lo[2]; k <= hi[2]; ++k)
    for (long long j = lo[1]; j <= hi[1]; ++j)
      for (long long i = lo[0]; i <= hi[0]; ++i) {
        long long l[3] = {i, j, k};
        bool inside = true;
        for (int d = 0; d < T.ndim; ++d) {
          if (l[d] < 0) { if (T.periodic[2 * d]) l[d] += T.nleaf[d]; else inside = false; }
          else if (l[d] >= T.nleaf[d]) { if (T.periodic[2 * d + 1]) l[d] -= T.nleaf[d]; else inside = false; }
        }
        if (!inside) continue;
        const int32_t g = T.leaf_map[(l[2] * T.nleaf[1] + l[1]) * T.nleaf[0] + l[0]];
        if (g != b) out->push_back(g);
      }
}
inline HaloPlan PlanHalo(const MeshTopology &T, int rank, int rings = 1) {
  HaloPlan pl;
  std::vector<char> have((size_t)T.nblocks_total, 0), is_halo((size_t)T.nblocks_total, 0);
  std::vector<int32_t> frontier;
  for (int g = 0; g < T.nblocks_total; ++g)
    if (T.owner[g] == rank) { have[g] = 1; frontier.push_back(g); pl.resident_gids.push_back(g); }
  pl.nowned = (int)pl.resident_gids.size();
  for (int ring = 0; ring < rings; ++ring) {
    std::vector<int32_t> touched, next;
    for (int32_t b : frontier) TouchingBlocks(T, b, &touched);
    for (int32_t g : touched)
      if (!have[g]) { have[g] = 1; is_halo[g] = 1; next.push_back(g); }
    frontier.swap(next);
  }
  for (int g = 0; g < T.nblocks_total; ++g)
    if (is_halo[g]) pl.resident_gids.push_back(g);
  pl.owned.assign(pl.resident_gids.size(), 0);
  for (int q = 0; q < pl.nowned; ++q) pl.owned[q] = 1;
  pl.local_index.assign((size_t)T.nblocks_total, -1);
  for (size_t q = 0; q < pl.resident_gids.size(); ++q) pl.local_index[(size_t)pl.resident_gids[q]] = (int32_t)q;
  return pl;
}
// The refresh of the halo copies' interior cells after the owner changed a field (UpdateFluid:
// internal_energy; mcblock_driver.cpp:58-74 runs Parthenon's boundary exchange there): every rank
// can work out, without talking to anybody, which of its blocks the others keep copies of.
//   serve_*      (local block, cell) of the cells this rank sends, grouped by destination rank in
//                rank order -- jb_gather_cells packs them; send_counts[r] cells go to rank r
//   dst_*, src_* arguments of jb_fill_cells with one sample per destination: interior cell c of halo
//                copy lb takes element src_cell of the receive buffer (src_blk = -1), which holds
//                recv_counts[r] values from rank r, in rank order
// Cells are the interior cells of a block in (k, j, i) order, as flat indices into [nk][nj][ni].
struct HaloRefreshPlan {
  std::vector<int32_t> serve_blk, serve_cell, dst_blk, dst_cell, src_blk, src_cell;
  std::vector<int64_t> send_counts, recv_counts;
};
inline HaloRefreshPlan PlanHaloRefresh(const MeshTopology &T, int rank, int nranks, const int nx[3], int ng,
                                       int rings = 1) {
  HaloRefreshPlan pl;
  pl.send_counts.assign((size_t)nranks, 0);
  pl.recv_counts.assign((size_t)nranks, 0);
  const int is = ng, js = T.ndim >= 2 ? ng : 0, ks = T.ndim >= 3 ? ng : 0;
  const int ni = nx[0] + 2 * is, nj = nx[1] + 2 * js;
  std::vector<int32_t> interior;
  for (int k = 0; k < nx[2]; ++k)
    for (int j = 0; j < nx[1]; ++j)
      for (int i = 0; i < nx[0]; ++i) interior.push_back(((k + ks) * nj + (j + js)) * ni + (i + is));
  const HaloPlan mine = PlanHalo(T, rank, rings);
  for (int r = 0; r < nranks; ++r) {
    if (r == rank) continue;
    const HaloPlan theirs = PlanHalo(T, r, rings);
    for (size_t q = (size_t)theirs.nowned; q < theirs.resident_gids.size(); ++q) {
      const int32_t g = theirs.resident_gids[q];
      if (T.owner[g] != rank) continue;          // rank r keeps a copy of MY block g
      for (int32_t c : interior) { pl.serve_blk.push_back(mine.local_index[(size_t)g]); pl.serve_cell.push_back(c); }
      pl.send_counts[(size_t)r] += (int64_t)interior.size();
    }
  }
  int64_t off = 0;
  for (int r = 0; r < nranks; ++r) {
    if (r == rank) continue;
    for (size_t q = (size_t)mine.nowned; q < mine.resident_gids.size(); ++q) {
      const int32_t g = mine.resident_gids[q];
      if (T.owner[g] != r) continue;             // my copy of rank r's block g
      for (int32_t c : interior) {
        pl.dst_blk.push_back((int32_t)q); pl.dst_cell.push_back(c);
        pl.src_blk.push_back(-1); pl.src_cell.push_back((int32_t)off++);
      }
      pl.recv_counts[(size_t)r] += (int64_t)interior.size();
    }
  }
  return pl;
}

// ---- tasks (jaybenne.hpp:59-76) ----------------------------------------------------------------
inline TaskStatus UpdateDerivedTransportFields(MeshData *md, const Real dt) {
  return Check(jb_update_derived_transport_fields(md->ctx(), md->mesh(), dt));
}

// ---- boundary source: Planckian inflow through chosen domain faces (jaybenne_amd.h) -----------------
inline bool BoundarySourceOn(MeshData *md) { return jb_boundary_source_enabled(md->ctx()) == 1; }
// A black wall of temperature `temperature` behind domain face `face` (0..5 = ix1 .. ox3); 0 = off.  For a rank that
// holds the whole mesh (the number of source face cells is taken from its view).
inline void SetBoundarySource(MeshData *md, int face, const Real temperature) {
  Check(jb_set_boundary_source(md->ctx(), face, temperature));
  md->bsource_face_cells_total = jb_boundary_face_cells(md->ctx(), md->mesh());
  Check(jb_set_boundary_source_count(md->ctx(), md->bsource_num_particles, md->bsource_face_cells_total));
}
// jb_source_boundary_count into md->bsource_pending (the library's own prefix workspace)
inline void CountBoundaryPhotons(MeshData *md, const Real dt) {
  auto &bp = md->bsource_pending;
  bp.nper.assign((size_t)md->nblocks(), 0);
  bp.plan = jb_boundary_source_plan{};
  bp.plan.nper_block = bp.nper.data();
  Check(jb_source_boundary_count(md->ctx(), md->mesh(), dt, md->bsource_face_cells_total, md->bsource_num_particles,
                                 SourceEpoch(md->cycle, SourceType::emission), &bp.plan, nullptr));
  bp.cycle = md->cycle;
  bp.valid = true;
}

// SourcePhotons<T, ST>(md, t_start, dt): per_block = the MeshBlockData instantiation used at
// initialisation (one call per block, sourcing.cpp:68-69).  The emission source with the boundary source on also
// counts the boundary photons: block b's take the ids behind its emission photons (PlanSourceWithBoundary), and
// SourceBoundaryPhotons fills them.
inline TaskStatus SourcePhotons(MeshData *md, SourceType st, const Real t_start, const Real dt,
                                bool per_block = false) {
  const jb_params &p = md->pkg().params();
  if (p.source_strategy == JB_STRATEGY_ENERGY)  // sourcing.cpp:38
    throw Error(JB_ERR_INVALID, "Energy source strategy not implemented!");
  if (st == SourceType::emission && !p.do_emission) return TaskStatus::complete;
  const int type = st == SourceType::thermal ? JB_SOURCE_THERMAL : JB_SOURCE_EMISSION;
  const int nb = md->nblocks();
  std::vector<int32_t> nper(nb, 0);
  Check(jb_source_photons_count(md->ctx(), md->mesh(), type, dt, per_block ? 1 : nb,
                                SourceEpoch(md->cycle, st), nper.data(), md->prefix_dev()));
  const bool with_boundary = st == SourceType::emission && BoundarySourceOn(md);
  if (with_boundary) CountBoundaryPhotons(md, dt);
  // (this rank holds the whole mesh: global id = local index, global counts = local counts)
  std::vector<int32_t> gid(nb);
  std::vector<long long> all(nb);
  for (int b = 0; b < nb; ++b) { gid[b] = b; all[b] = nper[b] + (with_boundary ? md->bsource_pending.nper[b] : 0); }
  const SourcePlan pl = with_boundary
      ? PlanSourceWithBoundary(nper, md->bsource_pending.nper, gid, all, md->next_id, md->swarm.n)
      : PlanSource(nper, gid, all, md->next_id, md->swarm.n);
  md->Reserve(md->swarm.n + pl.total_local);
  Check(jb_source_photons_fill(md->ctx(), md->mesh(), &md->swarm, type, t_start, dt, nper.data(),
                               md->prefix_dev(), pl.slot_base.data(), pl.id_base.data()));
  for (int b = 0; b < nb; ++b) md->swarm.n += nper[b];
  md->next_id = pl.next_id;
  if (with_boundary) md->bsource_pending.id_base = pl.id_base_boundary;
  return TaskStatus::complete;
}

// The boundary source of one cycle, right behind SourcePhotons(emission): every source face cell emits
// sb T_f^4 A dt (jaybenne_amd.h).  Appends the cycle's record to md->boundary_source_history.  Every face off:
// nothing, and no kernel.
inline TaskStatus SourceBoundaryPhotons(MeshData *md, const Real t_start, const Real dt) {
  if (!BoundarySourceOn(md)) return TaskStatus::complete;
  auto &bp = md->bsource_pending;
  const int nb = md->nblocks();
  if (!bp.valid || bp.cycle != md->cycle) {   // (no emission source in front: the boundary photons alone)
    CountBoundaryPhotons(md, dt);
    std::vector<int32_t> gid(nb);
    std::vector<long long> all(nb);
    for (int b = 0; b < nb; ++b) { gid[b] = b; all[b] = bp.nper[b]; }
    const SourcePlan pl = PlanSource(bp.nper, gid, all, md->next_id, md->swarm.n);
    bp.id_base = pl.id_base;
    md->next_id = pl.next_id;
  }
  std::vector<int64_t> slot(nb);
  int64_t tot = 0;
  for (int b = 0; b < nb; ++b) { slot[b] = md->swarm.n + tot; tot += bp.nper[b]; }
  md->Reserve(md->swarm.n + tot);
  Check(jb_source_boundary_fill(md->ctx(), md->mesh(), &md->swarm, t_start, dt, bp.nper.data(), nullptr, slot.data(),
                                bp.id_base.data()));
  md->swarm.n += tot;
  BoundarySourceCycle rec{};
  rec.cycle = (int64_t)md->cycle;
  for (int f = 0; f < 6; ++f) { rec.e_face[f] = bp.plan.e_face[f]; rec.n_face[f] = bp.plan.n_face[f]; }
  md->boundary_source_history.push_back(rec);
  bp.valid = false;
  return TaskStatus::complete;
}

inline TaskStatus TransportPhotons(MeshData *md, const Real t_start, const Real dt,
                                   bool fuse_census_tally = false) {
  return Check(jb_transport_photons(md->ctx(), md->mesh(), &md->swarm, t_start, dt, 0,
                                    md->swarm.n, fuse_census_tally ? 1 : 0));
}
inline TaskStatus TransportPhotons_DDMC(MeshData *md, const Real t_start, const Real dt,
                                        bool fuse_census_tally = false) {
  return Check(jb_transport_photons_ddmc(md->ctx(), md->mesh(), &md->swarm, t_start, dt, 0,
                                         md->swarm.n, fuse_census_tally ? 1 : 0));
}
inline TaskStatus SampleDDMCBlockFace(MeshData *md) {
  return Check(jb_sample_ddmc_block_face(md->ctx(), md->mesh(), &md->swarm, 0, md->swarm.n));
}
inline TaskStatus CheckCompletion(MeshData *md, const Real t_end) {
  int64_t unfinished = 0;
  return Check(jb_check_completion(md->ctx(), &md->swarm, t_end, &unfinished));
}
inline TaskStatus EvaluateRadiationEnergy(MeshData *md) {
  return Check(jb_evaluate_radiation_energy(md->ctx(), md->mesh(), &md->swarm));
}
inline TaskStatus UpdateFluid(MeshData *md) { return Check(jb_update_fluid(md->ctx(), md->mesh())); }
// jaybenne::DefragParticles -- jaybenne.cpp:499-509 (scheduled by no task list of the reference):
// the swarm sorted by block and cell, in place (jaybenne_amd.h: jb_defrag_particles)
inline TaskStatus DefragParticles(MeshData *md) {
  return Check(jb_defrag_particles(md->ctx(), md->mesh(), &md->swarm));
}
// the order of the photons within a cell behind a sort: JB_CELL_ORDER_ANY (default) or JB_CELL_ORDER_BY_ID, the
// canonical order by creation id (jaybenne_amd.h: jb_set_cell_order) -- DefragParticles, the library's schedule
// and the comb's plan then sort by (block, cell, id)
inline void SetCellOrder(MeshData *md, int mode) { Check(jb_set_cell_order(md->ctx(), mode)); }
inline int GetCellOrder(MeshData *md) { return jb_get_cell_order(md->ctx()); }
// the mode of the deck key <jaybenne_amd> cell_order = any | id
inline int CellOrderOf(const std::string &value) {
  if (value == "any") return JB_CELL_ORDER_ANY;
  if (value == "id") return JB_CELL_ORDER_BY_ID;
  throw std::invalid_argument("jaybenne_amd/cell_order = '" + value + "': one of any, id");
}
// exact deposition: JB_DEPOSIT_ATOMIC (default) or JB_DEPOSIT_EXACT -- energy_delta and the census tally as one
// rounding of the exact sum of their addends (jaybenne_amd.h: jb_set_deposition); DepositClose before UpdateFluid
inline void SetDeposition(MeshData *md, int mode) { Check(jb_set_deposition(md->ctx(), mode)); }
inline int GetDeposition(MeshData *md) { return jb_get_deposition(md->ctx()); }
inline jb_deposit_stats DepositClose(MeshData *md) {
  jb_deposit_stats s{};
  Check(jb_deposit_close(md->ctx(), md->mesh(), &md->swarm));
  Check(jb_deposit_last(md->ctx(), &s));
  return s;
}
// the mode of the deck key <jaybenne_amd> deposition = atomic | exact
inline int DepositionOf(const std::string &value) {
  if (value == "atomic") return JB_DEPOSIT_ATOMIC;
  if (value == "exact") return JB_DEPOSIT_EXACT;
  throw std::invalid_argument("jaybenne_amd/deposition = '" + value + "': one of atomic, exact");
}
// source tilt: JB_TILT_NONE (default) or JB_TILT_LINEAR -- SourcePhotons places a new photon in its cell along the
// gradient of T^4 taken from the neighbouring cells (jaybenne_amd.h: jb_set_source_tilt); ids and draws are the same
inline void SetSourceTilt(MeshData *md, int mode) { Check(jb_set_source_tilt(md->ctx(), mode)); }
inline int GetSourceTilt(MeshData *md) { return jb_get_source_tilt(md->ctx()); }
// the mode of the deck key <jaybenne_amd> source_tilt = none | linear
inline int SourceTiltOf(const std::string &value) {
  if (value == "none") return JB_TILT_NONE;
  if (value == "linear") return JB_TILT_LINEAR;
  throw std::invalid_argument("jaybenne_amd/source_tilt = '" + value + "': one of none, linear");
}
// source allocation: JB_ALLOC_UNIFORM (default: every cell the same number of new photons, sourcing.cpp:68-69) or
// JB_ALLOC_ENERGY -- a cell's number follows the energy it sources, num_particles over the whole mesh per call, so
// the new photons carry nearly equal weights (jaybenne_amd.h: jb_set_source_allocation).  This MeshData holds the
// whole mesh, so SourcePhotons and RadiationStep need nothing else: jb_source_photons_count runs the energy pass, the
// total and the count pass in a row.
inline void SetSourceAllocation(MeshData *md, int mode) { Check(jb_set_source_allocation(md->ctx(), mode)); }
inline int GetSourceAllocation(MeshData *md) { return jb_get_source_allocation(md->ctx()); }
// the mode of the deck key <jaybenne_amd> source_allocation = uniform | energy
inline int SourceAllocationOf(const std::string &value) {
  if (value == "uniform") return JB_ALLOC_UNIFORM;
  if (value == "energy") return JB_ALLOC_ENERGY;
  throw std::invalid_argument("jaybenne_amd/source_allocation = '" + value + "': one of uniform, energy");
}
inline Real EstimateTimestepMesh(MeshData *md) { return jb_estimate_timestep(md->ctx()); }

// jaybenne::InitializeRadiation(mbd, is_thermal) -- jaybenne.cpp:570-578
inline void InitializeRadiation(MeshData *md, bool is_thermal) {
  if (is_thermal) SourcePhotons(md, SourceType::thermal, 0.0, 0.0, /*per_block=*/true);
  EvaluateRadiationEnergy(md);
}

// A trace range for the lifetime of the object (jb_range_push / jb_range_pop: ROCTx, a no-op without the marker
// library) -- the reference's Kokkos::Profiling::pushRegion / popRegion, jaybenne.cpp:87,115,127,145
struct TraceRange {
  explicit TraceRange(const char *name) { jb_range_push(name); }
  ~TraceRange() { jb_range_pop(); }
  TraceRange(const TraceRange &) = delete;
  TraceRange &operator=(const TraceRange &) = delete;
};

// (not in the reference's task list: DefragParticles at the end of a cycle, on the library's schedule or every
// k-th cycle)
inline void DefragAfterStep(MeshData *md, int64_t events) {
  if (md->defrag_interval < 0) {
    int32_t sorted = 0;
    Check(jb_defrag_policy(md->ctx(), md->mesh(), &md->swarm, events, JB_DEFRAG_DECIDE_AND_SORT, &sorted));
    md->defrags += sorted;
  } else if (md->defrag_interval > 0 && ++md->steps_since_defrag >= md->defrag_interval) {
    DefragParticles(md);
    md->steps_since_defrag = 0;
    ++md->defrags;
  }
}

// Census population control at the end of a cycle, single process (not in the reference's task list): every cell
// with more than md->comb_trigger ACTIVE photons comes out with exactly md->comb_target of equal weight, its
// energy kept (jaybenne_amd.h: jb_comb_census_plan / _apply).  New creation ids come from md->next_id.  Returns
// true when the plan sorted the swarm.
inline bool CombCensus(MeshData *md) {
  if (md->comb_target <= 0) return false;
  jb_comb_plan plan{};
  Check(jb_comb_census_plan(md->ctx(), md->mesh(), &md->swarm, md->comb_trigger, md->comb_target, (uint32_t)md->cycle,
                            &plan));
  if (plan.cells_combed > 0) {
    jb_comb_report rep{};
    Check(jb_comb_census_apply(md->ctx(), md->mesh(), &md->swarm, md->next_id, &rep));
    md->comb_history.push_back(CombRecord{(int64_t)md->cycle, plan.n_before, rep.n_after, rep.n_new_ids, md->next_id,
                                          plan.cells_combed, plan.max_per_cell, plan.e_before, rep.e_after});
    md->next_id += (uint64_t)rep.n_new_ids;
  }
  return plan.sorted != 0;
}
// The ranges of the deck keys <jaybenne_amd> census_total_target, census_total_band and census_split_max (every host
// checks them this way), and that the global comb is not asked for together with the per-cell comb.
inline void CheckCensusTotal(int64_t target, double band, int64_t split_max, int64_t per_cell_max = 0) {
  if (target < 0 || target >= ((int64_t)1 << 31)) throw std::invalid_argument("census_total_target must be in [0, 2^31)");
  if (!(band >= 1.0) || !std::isfinite(band)) throw std::invalid_argument("census_total_band must be a finite number >= 1");
  if (split_max < 1) throw std::invalid_argument("census_split_max must be >= 1");
  if (target > 0 && per_cell_max > 0)
    throw std::invalid_argument("census_total_target and census_per_cell_max: one comb at a time -- the global comb "
                                "deals the cells their shares itself");
}
// Census population control for the whole mesh at the end of a cycle, single process (not in the reference's task
// list): the swarm is held near md->census_total_target photons of equal weight -- the target is dealt to the cells
// in proportion to the census energy they hold; a cell off its share by more than the factor census_total_band is
// thinned or split to it (at most to census_split_max times its count) and keeps its energy (jaybenne_amd.h:
// jb_comb_census_weigh / _plan_global / _apply).  The mesh is wholly resident and owned here: the block sums are
// ordered by global block id and added by jb_source_energy_total, as every host adds them.  Returns true when the
// weigh sorted the swarm.
inline bool CombCensusGlobal(MeshData *md) {
  const int64_t N = md->census_total_target;
  if (N <= 0) return false;
  CheckCensusTotal(N, md->census_total_band, md->census_split_max, md->comb_target);
  if (md->nblocks() != md->nblocks_total())
    throw std::invalid_argument("CombCensusGlobal: this host adds the block sums of one process; the mesh must be wholly resident");
  const int64_t n = md->swarm.n, S = md->census_split_max;
  const int64_t n_room = n + N < S * n ? n + N : S * n;   // (n_after <= n + N: every combed cell had a photon)
  md->Reserve(n_room);
  jb_comb_global_plan plan{};
  std::vector<double> e_local((size_t)md->nblocks()), e_gid((size_t)md->nblocks_total(), 0.0);
  Check(jb_comb_census_weigh(md->ctx(), md->mesh(), &md->swarm, n_room, e_local.data(), &plan));
  for (int b = 0; b < md->nblocks(); ++b) e_gid[(size_t)md->gid()[(size_t)b]] = e_local[(size_t)b];
  const double w_total = jb_source_energy_total(e_gid.data(), md->nblocks_total());
  if (w_total > 0.0 && std::isfinite(w_total))
    Check(jb_comb_census_plan_global(md->ctx(), md->mesh(), &md->swarm, w_total, N, md->census_total_band, S,
                                     (uint32_t)md->cycle, &plan));
  if (plan.cells_thinned + plan.cells_split > 0) {
    jb_comb_report rep{};
    Check(jb_comb_census_apply(md->ctx(), md->mesh(), &md->swarm, md->next_id, &rep));
    CombRecord r{(int64_t)md->cycle, plan.n_before, rep.n_after, rep.n_new_ids, md->next_id,
                 plan.cells_thinned + plan.cells_split, plan.max_per_cell, plan.e_before, rep.e_after};
    r.global = true;
    r.cells_thinned = plan.cells_thinned;
    r.cells_split = plan.cells_split;
    r.max_target = plan.max_target;
    r.w_total = w_total;
    r.scale = (double)N / w_total;
    md->comb_history.push_back(r);
    md->next_id += (uint64_t)rep.n_new_ids;
  }
  return plan.sorted != 0;
}
// One line of JSON per combed cycle (the keys of the Python host's md.comb_history, %.17g: both hosts print the same
// bits); the global comb's keys only for its records.
inline std::string CombJson(const CombRecord &r) {
  char buf[1024];
  int len = std::snprintf(buf, sizeof buf,
                          "{\"cycle\": %lld, \"n_before\": %lld, \"n_after\": %lld, \"n_new_ids\": %lld, \"id_base\": %llu, "
                          "\"cells_combed\": %lld, \"max_per_cell\": %lld, \"e_before\": %.17g, \"e_after\": %.17g",
                          (long long)r.cycle, (long long)r.n_before, (long long)r.n_after, (long long)r.n_new_ids,
                          (unsigned long long)r.id_base, (long long)r.cells_combed, (long long)r.max_per_cell, r.e_before,
                          r.e_after);
  if (r.global)
    len += std::snprintf(buf + len, sizeof buf - (size_t)len,
                         ", \"mode\": \"global\", \"cells_thinned\": %lld, \"cells_split\": %lld, \"max_target\": %lld, "
                         "\"w_total\": %.17g, \"scale\": %.17g",
                         (long long)r.cells_thinned, (long long)r.cells_split, (long long)r.max_target, r.w_total, r.scale);
  return std::string(buf) + "}";
}
// the end of a cycle: the comb where it is on, then DefragParticles' schedule.  A cycle whose comb sorted the
// swarm counts as a sort: the k-th-cycle counter starts over; the library's schedule has started over inside
// the plan and is still called (it reads the cycle's kernel times and, one cycle behind a sort, never sorts).
inline void CombAfterStep(MeshData *md, int64_t events) {
  const bool sorted = md->census_total_target > 0 ? CombCensusGlobal(md) : CombCensus(md);
  if (sorted && md->defrag_interval >= 0) {
    md->steps_since_defrag = 0;
    return;
  }
  DefragAfterStep(md, events);
}

// ---- radiation moments (jaybenne_amd.h: jb_evaluate_radiation_moments): only when a host asks -------------
// Per-cell count, energy density, sum of squared weights, flux and second-moment tensor of the census as a host
// array [JB_MOMENTS][nblocks][ncell] (interior cells in (k, j, i) order; zeros in halo copies).  Sorts the swarm
// by (block, cell) when it is not in that order.
inline std::vector<double> EvaluateRadiationMoments(MeshData *md, jb_moments_report *report = nullptr) {
  std::vector<double> out((size_t)jb_moments_words(md->mesh()));
  Check(jb_evaluate_radiation_moments_host(md->ctx(), md->mesh(), &md->swarm, out.data(), report));
  return out;
}
// The domain integrals a command-line host prints per cycle: n, e = sum E dv, w2, f = sum F dv, q = sum Q dv, each
// summed sequentially in (component, block, cell) order -- every host forms them this way, so that two hosts print
// the same digits for the same run -- and eddington[d] = q_dd / (c^2 e).  blk_dx: [nblocks][3], as jb_mesh_view's.
struct MomentsIntegrals {
  double n = 0.0, e = 0.0, w2 = 0.0, f[3] = {0.0, 0.0, 0.0}, q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double eddington[3] = {0.0, 0.0, 0.0};
};
inline MomentsIntegrals IntegrateMoments(const std::vector<double> &m, int nblocks, int64_t ncell, const double *blk_dx,
                                         double c) {
  double s[JB_MOMENTS];
  for (int comp = 0; comp < JB_MOMENTS; ++comp) {
    const bool per_volume = comp != JB_MOM_N && comp != JB_MOM_W2;
    double acc = 0.0;
    for (int b = 0; b < nblocks; ++b) {
      const double dv = (blk_dx[3 * b] * blk_dx[3 * b + 1]) * blk_dx[3 * b + 2];
      const double *v = m.data() + ((size_t)comp * (size_t)nblocks + (size_t)b) * (size_t)ncell;
      for (int64_t q = 0; q < ncell; ++q) {
        const double t = per_volume ? v[q] * dv : v[q];   // (its own statement: rounded before it is added)
        acc += t;
      }
    }
    s[comp] = acc;
  }
  MomentsIntegrals I;
  I.n = s[JB_MOM_N];
  I.e = s[JB_MOM_E];
  I.w2 = s[JB_MOM_W2];
  for (int d = 0; d < 3; ++d) I.f[d] = s[JB_MOM_FX + d];
  for (int d = 0; d < 6; ++d) I.q[d] = s[JB_MOM_QXX + d];
  const double c2e = (c * c) * I.e;
  const int diag[3] = {0, 3, 5};
  for (int d = 0; d < 3; ++d) I.eddington[d] = c2e > 0.0 ? I.q[diag[d]] / c2e : 0.0;
  return I;
}
// one cycle's line of `--moments FILE` (the keys and digits of `python -m jaybenne_amd --moments`)
inline std::string MomentsJson(uint64_t cycle, double time, const jb_moments_report &r, const MomentsIntegrals &I) {
  char buf[2048];
  const int n = std::snprintf(
      buf, sizeof buf,
      "{\"cycle\": %lld, \"time\": %.17g, \"n_counted\": %lld, \"n_skipped\": %lld, \"cells_nonempty\": %lld, "
      "\"longest_run\": %lld, \"sorted\": %d, \"n\": %.17g, \"e\": %.17g, \"w2\": %.17g, \"f\": [%.17g, %.17g, %.17g], "
      "\"q\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g], \"eddington\": [%.17g, %.17g, %.17g]}",
      (long long)cycle, time, (long long)r.n_counted, (long long)r.n_skipped, (long long)r.cells_nonempty,
      (long long)r.longest_run, (int)r.sorted, I.n, I.e, I.w2, I.f[0], I.f[1], I.f[2], I.q[0], I.q[1], I.q[2], I.q[3],
      I.q[4], I.q[5], I.eddington[0], I.eddington[1], I.eddington[2]);
  return std::string(buf, n > 0 ? (size_t)n : 0);
}

// ---- radiation spectrum (jaybenne_amd.h: jb_evaluate_radiation_spectrum): only when a host asks ------------
// Per-cell energy density of the census in the ngroups + 2 bins of edges.size() - 1 frequency groups as a host array
// [ngroups + 2][nblocks][ncell] (interior cells in (k, j, i) order; zeros in halo copies).  Sorts the swarm by
// (block, cell) when it is not in that order.
inline std::vector<double> EvaluateRadiationSpectrum(MeshData *md, const std::vector<double> &edges,
                                                     jb_spectrum_report *report = nullptr) {
  const int ngroups = (int)edges.size() - 1;
  std::vector<double> out((size_t)jb_spectrum_words(md->mesh(), ngroups));
  Check(jb_evaluate_radiation_spectrum_host(md->ctx(), md->mesh(), &md->swarm, edges.data(), ngroups, out.data(), report));
  return out;
}
// `spectrum_edges = e0, e1, ..` of a deck or a command line: a comma-separated list of decimal numbers; blanks
// around a number and empty items are ignored.  A number is  [+-] digits [. digits] | [+-] . digits,  then
// optionally  e|E [+-] digits  -- one grammar in every host (`python -m jaybenne_amd` holds its list to the same
// before float()), so that no text is a number to one host and an error to another: no hex floats, no inf or nan,
// no digit separators.  The value is strtod's, correctly rounded.  Anything else throws, naming the item.
inline bool IsDecimalNumber(const std::string &t) {
  size_t q = 0;
  auto digits = [&] {
    const size_t q0 = q;
    while (q < t.size() && t[q] >= '0' && t[q] <= '9') ++q;
    return q - q0;
  };
  if (q < t.size() && (t[q] == '+' || t[q] == '-')) ++q;
  size_t mant = digits();
  if (q < t.size() && t[q] == '.') {
    ++q;
    mant += digits();
  }
  if (mant == 0) return false;
  if (q < t.size() && (t[q] == 'e' || t[q] == 'E')) {
    ++q;
    if (q < t.size() && (t[q] == '+' || t[q] == '-')) ++q;
    if (digits() == 0) return false;
  }
  return q == t.size();
}
inline std::vector<double> ParseSpectrumEdges(const std::string &text) {
  std::vector<double> edges;
  size_t at = 0;
  while (at <= text.size()) {
    const size_t comma = std::min(text.find(',', at), text.size());
    std::string item = text.substr(at, comma - at);
    const size_t first = item.find_first_not_of(" \t");
    if (first != std::string::npos) {
      item = item.substr(first, item.find_last_not_of(" \t") - first + 1);
      if (!IsDecimalNumber(item)) throw std::runtime_error("spectrum_edges: '" + item + "' is not a decimal number");
      edges.push_back(std::strtod(item.c_str(), nullptr));
    }
    at = comma + 1;
  }
  if (edges.size() < 2 || edges.size() > JB_SPECTRUM_MAX_GROUPS + 1)
    throw std::runtime_error("spectrum_edges: 2 .. 65 comma-separated edges are needed");
  return edges;
}
// The domain integrals a command-line host prints per cycle: sum over cells of out[bin] dv for every bin, summed
// sequentially in (block, cell) order, as IntegrateMoments does.
inline std::vector<double> IntegrateSpectrum(const std::vector<double> &s, int nbins, int nblocks, int64_t ncell,
                                             const double *blk_dx) {
  std::vector<double> integ((size_t)nbins, 0.0);
  for (int bin = 0; bin < nbins; ++bin) {
    double acc = 0.0;
    for (int b = 0; b < nblocks; ++b) {
      const double dv = (blk_dx[3 * b] * blk_dx[3 * b + 1]) * blk_dx[3 * b + 2];
      const double *v = s.data() + ((size_t)bin * (size_t)nblocks + (size_t)b) * (size_t)ncell;
      for (int64_t q = 0; q < ncell; ++q) {
        const double t = v[q] * dv;   // (its own statement: rounded before it is added)
        acc += t;
      }
    }
    integ[(size_t)bin] = acc;
  }
  return integ;
}
// one cycle's line of `--spectrum FILE` (the keys and digits of `python -m jaybenne_amd --spectrum`)
inline std::string SpectrumJson(uint64_t cycle, double time, const jb_spectrum_report &r, const std::vector<double> &edges,
                                const std::vector<double> &integ) {
  char buf[512];
  auto list = [&buf](const std::vector<double> &v) {
    std::string s = "[";
    for (size_t q = 0; q < v.size(); ++q) {
      std::snprintf(buf, sizeof buf, "%s%.17g", q ? ", " : "", v[q]);
      s += buf;
    }
    return s + "]";
  };
  std::snprintf(buf, sizeof buf,
                "{\"cycle\": %lld, \"time\": %.17g, \"n_counted\": %lld, \"n_skipped\": %lld, \"cells_nonempty\": %lld, "
                "\"longest_run\": %lld, \"n_below\": %lld, \"n_above\": %lld, \"sorted\": %d, \"ngroups\": %d, ",
                (long long)cycle, time, (long long)r.n_counted, (long long)r.n_skipped, (long long)r.cells_nonempty,
                (long long)r.longest_run, (long long)r.n_below, (long long)r.n_above, (int)r.sorted, (int)edges.size() - 1);
  const std::string head = buf;
  return head + "\"edges\": " + list(edges) + ", \"e\": " + list(integ) + "}";
}

// ---- energy ledger (jaybenne_amd.h: jb_ledger_*): off by default ----------------------------------
inline bool LedgerEnabled(MeshData *md) { return jb_ledger_enabled(md->ctx()) == 1; }
inline void EnableLedger(MeshData *md, bool on = true) {
  Check(jb_ledger_enable(md->ctx(), on ? 1 : 0));
  md->ledger = EnergyLedger{};
  md->ledger_history.clear();
  md->ledger_started = false;
}
// before the first cycle with the ledger on: the census energy it starts from (a close of its own; collective
// when nranks > 1)
inline void LedgerBegin(MeshData *md, const Real t_start, const jb_exchange_transport *tr = nullptr, int rank = 0,
                        int nranks = 1) {
  if (md->ledger_started) return;
  jb_energy_ledger led{};
  Check(jb_ledger_close(md->ctx(), md->mesh(), &md->swarm, t_start, 0.0, &led));
  Check(jb_ledger_reduce(md->ctx(), tr, rank, nranks, 0, &led));
  md->ledger_e0 = led.e_census;
  md->ledger_started = true;
}
inline void LedgerRecord(MeshData *md, const jb_energy_ledger &led) {
  EnergyLedger l{};
  static_cast<jb_energy_ledger &>(l) = led;
  l.e_start = md->ledger_e0;
  l.residual = LedgerResidual(led, md->ledger_e0);
  md->ledger_e0 = led.e_census;
  md->ledger = l;
  md->ledger_history.push_back(l);
}
// one cycle's ledger as a JSON line (the keys of `python -m jaybenne_amd --ledger`; %.17g restores the bits)
inline std::string LedgerJson(const EnergyLedger &l) {
  char buf[2048];
  int n = std::snprintf(buf, sizeof buf, "{\"cycle\": %lld, \"t_start\": %.17g, \"dt\": %.17g, \"e_start\": %.17g, "
                        "\"e_sourced\": %.17g, \"n_sourced\": %lld, \"e_escaped\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g], "
                        "\"n_escaped\": [%lld, %lld, %lld, %lld, %lld, %lld], \"e_escaped_unclassified\": %.17g, "
                        "\"n_escaped_unclassified\": %lld, \"e_absorbed\": %.17g, \"n_absorbed\": %lld, \"e_census\": %.17g, "
                        "\"n_census\": %lld, \"e_tally\": %.17g, \"e_delta\": %.17g, \"e_material\": %.17g, \"residual\": %.17g}",
                        (long long)l.cycle, l.t_start, l.dt, l.e_start, l.e_sourced, (long long)l.n_sourced, l.e_escaped[0],
                        l.e_escaped[1], l.e_escaped[2], l.e_escaped[3], l.e_escaped[4], l.e_escaped[5],
                        (long long)l.n_escaped[0], (long long)l.n_escaped[1], (long long)l.n_escaped[2],
                        (long long)l.n_escaped[3], (long long)l.n_escaped[4], (long long)l.n_escaped[5],
                        l.e_escaped_unclassified, (long long)l.n_escaped_unclassified, l.e_absorbed, (long long)l.n_absorbed,
                        l.e_census, (long long)l.n_census, l.e_tally, l.e_delta, l.e_material, l.residual);
  return std::string(buf, n > 0 ? (size_t)n : 0);
}

// ... with the boundary source's per-face terms of the same cycle appended (`--ledger` lines gain them only when a
// face is on)
inline std::string LedgerJson(const EnergyLedger &l, const BoundarySourceCycle &b) {
  std::string s = LedgerJson(l);
  char buf[512];
  const int n = std::snprintf(buf, sizeof buf, ", \"e_sourced_face\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g], "
                              "\"n_sourced_face\": [%lld, %lld, %lld, %lld, %lld, %lld]}",
                              b.e_face[0], b.e_face[1], b.e_face[2], b.e_face[3], b.e_face[4], b.e_face[5],
                              (long long)b.n_face[0], (long long)b.n_face[1], (long long)b.n_face[2],
                              (long long)b.n_face[3], (long long)b.n_face[4], (long long)b.n_face[5]);
  if (!s.empty() && s.back() == '}') s.pop_back();
  return s + std::string(buf, n > 0 ? (size_t)n : 0);
}

// jaybenne::RadiationStep(pmesh, t_start, dt) for one rank -- jaybenne.cpp:68-151
inline TaskStatus RadiationStep(MeshData *md, const Real t_start, const Real dt) {
  TraceRange timestep("Jaybenne::Timestep");
  const jb_params &p = md->pkg().params();
  const bool ledger = LedgerEnabled(md);
  if (ledger) LedgerBegin(md, t_start);
  md->cycle += 1;
  UpdateDerivedTransportFields(md, dt);
  const int64_t n_before = md->swarm.n;
  SourcePhotons(md, SourceType::emission, t_start, dt);
  SourceBoundaryPhotons(md, t_start, dt);
  if (ledger && md->swarm.n > n_before)
    Check(jb_ledger_accumulate(md->ctx(), md->mesh(), &md->swarm, n_before, md->swarm.n, JB_LEDGER_SOURCED));
  Check(jb_zero_energy_tally(md->ctx(), md->mesh()));
  jb_transport_stats before{}, after{};
  Check(jb_get_transport_stats(md->ctx(), &before, 0));
  {
    TraceRange loop("Jaybenne::TransportLoop");   // (one pass: every block crossing is resolved in flight)
    if (p.use_ddmc) TransportPhotons_DDMC(md, t_start, dt, /*fuse_census_tally=*/true);
    else TransportPhotons(md, t_start, dt, /*fuse_census_tally=*/true);
    // (what this launch absorbed and let escape, before the compaction closes those slots)
    if (ledger) Check(jb_ledger_accumulate(md->ctx(), md->mesh(), &md->swarm, 0, md->swarm.n, JB_LEDGER_TRANSPORTED));
  }
  Check(jb_get_transport_stats(md->ctx(), &after, 0));
  if (after.n_outgoing != before.n_outgoing)
    throw Error(JB_ERR_INVALID, "particles left for another rank in a single-rank step");
  if (after.n_absorbed != before.n_absorbed || after.n_escaped != before.n_escaped)
    Check(jb_remove_marked_particles(md->ctx(), &md->swarm));
  md->events += after.n_events - before.n_events;
  if (CheckCompletion(md, t_start + dt) != TaskStatus::complete) return TaskStatus::iterate;
  // (exact deposition: energy_delta and the tally, each rounded once, before UpdateFluid reads them)
  if (GetDeposition(md) == JB_DEPOSIT_EXACT) DepositClose(md);
  UpdateFluid(md);
  if (ledger) {
    jb_energy_ledger led{};
    Check(jb_ledger_close(md->ctx(), md->mesh(), &md->swarm, t_start, dt, &led));
    led.cycle = (int64_t)md->cycle;
    LedgerRecord(md, led);
  }
  CombAfterStep(md, after.n_events - before.n_events);
  return TaskStatus::complete;
}

// jaybenne::RadiationStep(pmesh, t_start, dt) on every rank of a block-partitioned mesh -- jaybenne.cpp:68-151
// with the iterate-sublist of :113-131 inside ONE library call, jb_radiation_step_ranks (collective: every rank
// calls it in the same cycle; see its contract in jaybenne_amd.h).  tr: the two collectives of the hand-off
// (may be NULL with nranks == 1); the swarm grows through MeshData's reserve.  JB_ITERATE (max_transport_iterations
// passes did not finish the sublist) comes back as TaskStatus::iterate on every rank; errors throw on every rank.
// The refresh of the halo copies after UpdateFluid stays with the host.  DefragParticles: as the single-rank
// overload, each rank on its own (a host whose ranks should sort together reduces JB_DEFRAG_DECIDE itself).
inline TaskStatus RadiationStep(MeshData *md, const Real t_start, const Real dt, const jb_exchange_transport *tr,
                                int rank, int nranks) {
  jb_rank_comm comm{};
  comm.rank = rank;
  comm.nranks = nranks;
  comm.transport = tr;
  comm.host = md;
  comm.reserve = &MeshData::ReserveTrampoline;
  const bool ledger = LedgerEnabled(md);   // (on on every rank or on none: the step reduces it with one more all-gather)
  if (ledger) LedgerBegin(md, t_start, tr, rank, nranks);
  const bool boundary = BoundarySourceOn(md);   // (the same faces, N_b and global face-cell count on every rank)
  if (boundary) Check(jb_set_boundary_source_count(md->ctx(), md->bsource_num_particles, md->bsource_face_cells_total));
  uint32_t cycle = (uint32_t)md->cycle;
  jb_step_report rep{};
  const jb_status st = jb_radiation_step_ranks(md->ctx(), md->mesh(), &md->swarm, t_start, dt, &md->next_id, &cycle,
                                               md->prefix_dev(), &comm, &rep);
  md->cycle = cycle;
  md->last_step = rep;
  if (Check(st) != TaskStatus::complete) return TaskStatus::iterate;
  md->events += rep.events;
  if (boundary) {   // (sourced inside the call, behind the emission source; this rank's part)
    jb_boundary_source_record last{};
    Check(jb_boundary_source_last(md->ctx(), &last));
    BoundarySourceCycle rec{};
    rec.cycle = (int64_t)md->cycle;
    for (int f = 0; f < 6; ++f) { rec.e_face[f] = last.e_face[f]; rec.n_face[f] = last.n_face[f]; }
    md->boundary_source_history.push_back(rec);
  }
  if (ledger) {   // (closed and reduced over the ranks inside the call)
    jb_energy_ledger led{};
    Check(jb_ledger_last(md->ctx(), &led));
    LedgerRecord(md, led);
  }
  DefragAfterStep(md, rep.events);
  return TaskStatus::complete;
}

// ---- transport invariants: the checked library's counts (include/jaybenne_amd.h) ----------------------
inline bool InvariantsEnabled() { return jb_invariants_enabled() == 1; }
// throws Error(JB_ERR_UNSUPPORTED) under the release library
inline jb_invariant_report InvariantReport(MeshData *md, bool reset = false) {
  jb_invariant_report r{};
  Check(jb_invariant_report_get(md->ctx(), &r, reset ? 1 : 0));
  return r;
}

}  // namespace jaybenne_amd

#endif  // JAYBENNE_AMD_HPP_
