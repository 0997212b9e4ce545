/* jaybenne_amd.h -- C ABI of the MI355X-native Implicit Monte Carlo history loop.
 *
 * This is the drop-in boundary for the hot path of lanl/jaybenne: one entry point per task the
 * reference package exposes to its host application (reference src/jaybenne/jaybenne.hpp:48-78),
 * over plain pointers and sizes.  The host framework owns every field and particle array (as
 * Parthenon does for the reference); the library borrows DEVICE pointers per call and owns only
 * its parameters, small lookup tables and scratch.  Nothing here throws; every function returns
 * a jb_status and jb_last_error() describes the most recent failure on the calling thread.
 *
 * Threading: calls on one jb_context are not re-entrant (the reference's tasks keep
 * function-local static pack descriptors, transport.cpp:44-52, and require one partition per
 * rank, jaybenne.cpp:92-95).  Work is enqueued on the context's HIP stream (jb_set_stream);
 * functions that return counts to the host synchronise that stream, the others do not.
 *
 * Index conventions (Parthenon's): a block's cell arrays are [nk][nj][ni]
 * with i fastest, ni = nx[0] + 2 ng etc. in active dimensions and a single index in inactive
 * ones; interior cells are ng .. ng+nx-1.  Face field F_d shares the cell layout: face i is
 * the lower-x_d face of cell i (reference transport_ddmc.cpp:150-159), so ng >= 1 is required.
 */
#ifndef JAYBENNE_AMD_H_
#define JAYBENNE_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* TaskStatus of the reference tasks (jaybenne.cpp:34,55-56; transport.cpp:211-215) + errors */
typedef enum jb_status {
  JB_COMPLETE = 0,
  JB_ITERATE = 1,
  JB_INCOMPLETE = 2,
  JB_ERR_INVALID = -1,   /* PARTHENON_REQUIRE / PARTHENON_FAIL conditions of the reference */
  JB_ERR_HIP = -2,
  JB_ERR_CAPACITY = -3,
  JB_ERR_UNSUPPORTED = -4,
  JB_ERR_INVARIANT = -5  /* checked library: a transport invariant was violated (jb_invariant_report) */
} jb_status;

enum { JB_BC_PERIODIC = 0, JB_BC_REFLECT = 1, JB_BC_OUTFLOW = 2 }; /* <parthenon/swarm> i/ox?_bc */
enum { JB_SOURCE_THERMAL = 0, JB_SOURCE_EMISSION = 1 };  /* SourceType, jaybenne.hpp:56 */
enum { JB_STRATEGY_UNIFORM = 0, JB_STRATEGY_ENERGY = 1 }; /* SourceStrategy, jaybenne.hpp:55 */
enum { JB_EOS_IDEAL_GAS = 0 };
enum { JB_OPAC_GRAY = 0, JB_OPAC_EPBREMSS = 1 };
enum { JB_SCAT_GRAY = 0, JB_SCAT_THOMSON = 1 };
/* particle status written by the transport tasks */
enum {
  JB_ST_ACTIVE = 0,   /* resident on this device (in flight before, at census after transport) */
  JB_ST_ABSORBED = 1, /* MarkParticleForRemoval after an absorption (transport.cpp:157-163) */
  JB_ST_ESCAPED = 2,  /* left through an outflow swarm boundary */
  JB_ST_OUTGOING = 3, /* to be handed to the rank that owns block `blk` (a GLOBAL id): the
                         particle left the resident blocks, or reached census in a halo copy */
  JB_ST_OUTGOING_ABSORBED = 4 /* absorbed inside a halo copy: the owner deposits its weight */
};

/* <jaybenne> input block, keys and defaults of reference jaybenne.cpp:163-223 */
typedef struct jb_params {
  int64_t num_particles; /* required */
  double dt;             /* default DBL_MAX */
  double min_swarm_occupancy;
  double numin, numax;   /* parsed, unused */
  double tau_ddmc;       /* default 5.0 */
  int32_t unique_rank_seeds;
  int32_t seed;          /* default 123 */
  int32_t max_transport_iterations; /* default 10000 */
  int32_t use_ddmc;
  int32_t source_strategy;
  int32_t do_emission;
  int32_t do_feedback;
  int32_t rank;          /* Globals::my_rank, used with unique_rank_seeds */
} jb_params;

/* the host's EOS / opacity / scattering objects (reference jaybenne.hpp:50-52,
 * jaybenne_config.hpp.in:19-26; mcblock.cpp:78-145), as tagged POD evaluated device-side */
typedef struct jb_eos {
  int32_t model, pad;
  double gm1, cv;        /* IdealGas(gm1, cv): T = sie / cv */
} jb_eos;
typedef struct jb_opacity {
  int32_t model, pad;
  double kappa;          /* Gray: sigma_a = rho kappa, j = sigma_a 4 sb T^4 */
  double c, sb;          /* GetRuntimePhysicalConstants(): speed of light, Stefan-Boltzmann,
                            in code units */
  /* NonCGSUnits<...>(opac, time, mass, length, temperature): code -> CGS conversion factors
   * (mcblock.cpp:84-91); read by JB_OPAC_EPBREMSS only (Gray takes kappa in code units):
   * electron-proton bremsstrahlung of fully ionised hydrogen, n_e = n_i = rho / m_p,
   *   alpha_nu = 4 e^6 / (3 m_e h c) sqrt(2 pi / (3 k m_e)) T^-1/2 n_e n_i nu^-3 (1 - e^(-h nu / k T))
   *   j        = sqrt(2 pi k T / (3 m_e)) 2^5 pi e^6 / (3 h m_e c^3) n_e n_i
   * (Rybicki & Lightman 5.18a, 5.15a, Gaunt factor 1) -- singularity-opac is not vendored in the
   * reference tree, so its constants could not be compared: parity unpinned for this model. */
  double time_scale, mass_scale, length_scale, temperature_scale;
} jb_opacity;
typedef struct jb_scattering {
  int32_t model, pad;
  double kappa_s, apm;   /* GrayS: sigma_s = (rho / apm) kappa_s; apm also read by ThomsonS */
  /* JB_SCAT_THOMSON: sigma_s = n_e sigma_T with n_e = rho / apm (apm in code mass units, as
   * mcblock.cpp:124 passes it), i.e. GrayS with kappa_s = sigma_T / length_scale^2 */
  double time_scale, mass_scale, length_scale, temperature_scale;
} jb_scattering;

/* The slice of the mesh this rank owns (the MeshData / SparsePack role).  All pointers in this
 * struct are HOST pointers; rho..P3 are host arrays of per-block DEVICE pointers. */
typedef struct jb_mesh_view {
  int32_t ndim, ng;
  int32_t nblocks;        /* blocks resident on this rank: the ones it owns + halo copies */
  int32_t nblocks_total;  /* Mesh::nbtotal */
  int32_t nx[3];          /* interior cells per block */
  int32_t nleaf[3];       /* extent of leaf_map (blocks of the finest level) */
  int32_t bc[6];          /* swarm boundary per face: ix1, ox1, ix2, ox2, ix3, ox3 */
  int32_t rank, pad;
  double gmin[3], gmax[3];
  const int32_t *leaf_map;     /* [nleaf2][nleaf1][nleaf0] -> global block id */
  const int32_t *owner;        /* [nblocks_total] rank that owns each global block */
  const int32_t *local_index;  /* [nblocks_total] index in this rank's resident list, or -1 */
  const int32_t *gid;          /* [nblocks] global id of each resident block */
  const int32_t *owned;        /* [nblocks] 1 = owned by this rank, 0 = halo copy: a read-only
                                  mirror of a neighbour rank's block (fields filled by the host)
                                  that lets particles be tracked across the rank boundary; may be
                                  NULL = every resident block is owned */
  const double *blk_xmin;      /* [nblocks][3] */
  const double *blk_xmax;      /* [nblocks][3] */
  const double *blk_dx;        /* [nblocks][3] (inactive dimensions: full extent) */
  const int32_t *blk_level;    /* [nblocks] */
  const int32_t *blk_nbr_lev;  /* [nblocks][6] neighbour level per face; own level at a
                                  physical boundary (jaybenne.cpp:341-351) */
  /* HOST_DENSITY, HOST_SPECIFIC_INTERNAL_ENERGY, HOST_UPDATE_ENERGY (jaybenne_config.hpp.in:28-30) */
  double *const *rho, *const *sie, *const *u;
  /* field.jaybenne.* (jaybenne_variables.hpp:35-40) */
  double *const *fleck, *const *tally, *const *edelta, *const *src_ew, *const *src_num;
  double *const *P1, *const *P2, *const *P3; /* ddmc_face_prob F1/F2/F3; may be NULL w/o DDMC */
} jb_mesh_view;

/* The photons swarm (jaybenne.cpp:236-245): structure of arrays, DEVICE pointers, particles
 * 0..n-1 valid.  rng is the state of each particle's own random stream (csrc/jb_rng.hpp); id is
 * the particle's creation index, which seeded that stream. */
typedef struct jb_swarm_view {
  int64_t n, capacity;
  double *x, *y, *z;      /* swarm_position::x,y,z */
  double *vx, *vy, *vz;   /* particle.photons.v[3] */
  double *t, *w, *e;      /* time, weight, energy */
  int32_t *ip, *jp, *kp;  /* particle.photons.ijk[3] */
  int32_t *blk;           /* local block index (global id when status == JB_ST_OUTGOING) */
  int32_t *status;
  uint64_t *id;           /* creation index, below 2^63.  Of a slot that is NOT live -- the JB_ST_ABSORBED hole
                             jb_unpack_incoming makes of an arrival that was absorbed on the sending rank -- the
                             id carries bit 63: "deposited on behalf of another rank" (read by the energy
                             ledger's sweep); holes vanish at the next jb_remove_marked_particles */
  uint64_t *rng;
} jb_swarm_view;

typedef struct jb_transport_stats {
  int64_t n_census, n_absorbed, n_escaped, n_outgoing;
  int64_t n_events;  /* passes through the while loop of transport.cpp:98-171 */
  int64_t n_wave_passes;    /* diagnostics: 64-lane passes through the kernel's event loop ... */
  int64_t n_wave_services;  /* ... and through its service phase, summed over waves */
} jb_transport_stats;

typedef struct jb_context jb_context;
typedef struct jb_mesh jb_mesh;

const char *jb_last_error(void);
const char *jb_version(void);

/* jaybenne::Initialize(pin, opacity, scattering, eos) -- jaybenne.hpp:50-52, jaybenne.cpp:158-266 */
jb_status jb_initialize(const jb_params *params, const jb_eos *eos, const jb_opacity *opacity,
                        const jb_scattering *scattering, int device, jb_context **ctx);
jb_status jb_finalize(jb_context *ctx);
jb_status jb_set_stream(jb_context *ctx, void *hip_stream);
jb_status jb_synchronize(jb_context *ctx);
/* Param<int>("seed"): seed + rank when unique_rank_seeds (jaybenne.cpp:187-190).  The random
 * streams are keyed with the UNADJUSTED seed, as the reference's pool is (quirk 1). */
int32_t jb_param_seed(const jb_context *ctx);

/* uploads the lookup tables of a mesh view; the view's host arrays may be freed afterwards */
jb_status jb_mesh_create(jb_context *ctx, const jb_mesh_view *view, jb_mesh **mesh);
jb_status jb_mesh_destroy(jb_mesh *mesh);

/* UpdateDerivedTransportFields(md, dt) -- jaybenne.hpp:66, jaybenne.cpp:285-492 */
jb_status jb_update_derived_transport_fields(jb_context *ctx, jb_mesh *mesh, double dt);

/* SourcePhotons<T,ST>(md, t_start, dt) -- jaybenne.hpp:63-64, sourcing.cpp:25-208, split at the
 * host round-trip of sourcing.cpp:120-131:
 *   _count  "SourcePhotons1": per-cell number / energy weight, per-block totals (to the host)
 *           and per-cell exclusive prefix (device int32 [nblocks][ncells]); blocks_in_call is
 *           the `nblocks` of sourcing.cpp:68-69 (1 on the MeshBlockData path);
 *   _fill   "SourcePhotons2": attributes of the nper_block[b] new particles of each block;
 *           block b writes slots slot_base[b].. and stream ids id_base[b]..  (host arrays
 *           [nblocks]; the slot assignment is Parthenon's AddEmptyParticles step).
 * Returns JB_COMPLETE without doing anything for emission when do_emission is false
 * (sourcing.cpp:41-43); JB_ERR_INVALID for the `energy` strategy (sourcing.cpp:38) and for
 * epoch >= 2^20 (the per-cell rounding streams are keyed by 20 bits of it). */
jb_status jb_source_photons_count(jb_context *ctx, jb_mesh *mesh, int source_type, double dt,
                                  int blocks_in_call, uint32_t epoch, int32_t *nper_block_host,
                                  int32_t *prefix_dev);
jb_status jb_source_photons_fill(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                 int source_type, double t_start, double dt,
                                 const int32_t *nper_block_host, const int32_t *prefix_dev,
                                 const int64_t *slot_base_host, const uint64_t *id_base_host);
/* ... and the same for a SHARE of every block's new particles: of the photons _count found for block b
 * (numbered 0.. in cell order, the order the stream ids follow) this call creates nper_block[b] of
 * them starting at number first_in_block[b]; id_base[b] stays the id of the block's photon 0.  This is
 * what a rank of a replicated-mesh run calls (every rank holds every block and sources its share of
 * each: SURVEY 8e "replicated mesh, split particles"; the reference has no such mode -- its blocks
 * are partitioned, jaybenne.cpp:92-95): histories are then dealt to ranks by stream id, whatever the
 * blocks cost.  set_energy_delta = 0 makes the emission source leave energy_delta at zero instead of
 * minus the emitted energy (sourcing.cpp:165-166,196): all ranks but one, so that the sum of the
 * ranks' energy_delta carries the emission once.  first_in_block_host = NULL: all of them, from 0. */
jb_status jb_source_photons_fill_range(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                       int source_type, double t_start, double dt,
                                       const int32_t *nper_block_host, const int32_t *prefix_dev,
                                       const int64_t *slot_base_host, const uint64_t *id_base_host,
                                       const int32_t *first_in_block_host, int set_energy_delta);

/* ---- boundary source: Planckian inflow through chosen domain faces (the reference has none: its sources are
 * inside the volume, sourcing.cpp).  Off by default; with every face off no kernel of it is launched and every
 * call above and below takes the branches it took and gives the bits it gave.  DESIGN.md 4.8.
 *
 * Which faces.  A boundary source is a temperature T_f > 0 on a domain face f; faces are numbered 0..5 = ix1, ox1,
 *   ix2, ox2, ix3, ox3.  T_f = 0: the face is off.  Only faces of active axes (f < 2 ndim) whose swarm boundary is
 *   not periodic may be set; both are checked where the mesh is known, by jb_source_boundary_count.
 * Which cells, how much energy.  A SOURCE FACE CELL is an interior cell of an owned block whose face f lies on the
 *   domain boundary.  Per cycle each emits E_c = sb T_f^4 A_c dt -- with a c / 4 = sb the one-sided flux of a black
 *   wall --, A_c the area of the cell's face from the block's own widths (on an inactive axis the width is the
 *   full extent, as blk_dx holds it), sb = jb_opacity.sb; evaluated as ((sb (T^2 T^2)) A) dt.
 * How many photons.  num_particles = N_b are asked for over all source faces of the WHOLE mesh; npc = N_b /
 *   face_cells_total, the host passing the global number of source face cells (jb_boundary_face_cells, summed over
 *   the ranks), so that nothing depends on the decomposition.  npc < 1: JB_ERR_INVALID.  A cell gets
 *   snpc = floor(npc) + (npc - floor(npc) > xi) photons, xi the first draw of rng_seed_state(seed, domain 3 + f,
 *   cell_stream_id(epoch, global block, cell)) -- cell and epoch as in the emission source --, each of weight
 *   E_c / snpc: the energy sourced through a face is sb T_f^4 (face area) dt to rounding, every cycle.
 * A photon's attributes come from its own stream, rng_stream_start(seed, id); with d = f / 2 the face's axis, ten
 *   draws: (1) the position on axis (d + 1) % 3 as xc + dx (xi - 0.5), (2) on axis (d + 2) % 3 the same way
 *   (inactive axes included, as the volume source does), (3, 4) sample_face_iso_dir(+c on a lower face, -c on an
 *   upper one): the principal component on axis d, the other two on (d + 1) % 3 and (d + 2) % 3 -- the cyclic
 *   assignment of ptcl_ddmc_albedo, transport_utils.hpp:280-397 --, (5-9) sample_planck_energy(sb, T_f),
 *   (10) t = t_start + xi dt.  The coordinate on axis d is face + eps_imc dx_d on a lower face, face - eps_imc dx_d
 *   on an upper one (face = xc -+ dx_d / 2 of the face cell): where the reference leaves a photon that has just
 *   crossed that face (transport_utils.hpp:151-159), so an IMC cell tracks it and a DDMC cell's albedo admits or
 *   reflects it.  ip / jp / kp the face cell, blk the block, status JB_ST_ACTIVE.
 * Ids and slots.  Within a cycle block b has n_em[b] emission and n_bs[b] boundary photons and takes
 *   n_em[b] + n_bs[b] consecutive ids from the per-block plan of the hosts (jaybenne_amd.hpp: PlanSource /
 *   PlanSourceWithBoundary), the emission photons first, the boundary photons behind them ordered by face, then by
 *   cell in (k, j, i) order, then by copy.  The boundary photons occupy the slots behind all emission photons of
 *   the call.  Ids therefore do not depend on the partition.
 *
 *   jb_set_boundary_source / _get_: T_f of one face.  JB_ERR_INVALID: face outside 0..5, negative or non-finite T.
 *   jb_set_boundary_source_count: N_b and the global number of source face cells for the STEP calls
 *     (jb_radiation_step, jb_radiation_step_ranks: they run the boundary source behind the emission source when a
 *     face is on; the same values on every rank).
 *   jb_boundary_face_cells: the source face cells of this rank's owned blocks under the faces now set.
 *   jb_boundary_prefix_words: int32 words of the prefix workspace of the two calls below for this mesh; prefix_dev
 *     = NULL in both: a workspace of the library's own (one per context, as the step calls use it).
 *   _count: per source face cell snpc; per resident block the number of new photons (plan_out->nper_block, host
 *     [nblocks], the caller's) and the exclusive prefix over the block's (face, cell) entries (device); e_face /
 *     n_face: energy and photons per face for this rank, summed in a fixed order without floating-point atomics
 *     (the same call gives the same bits).  One synchronisation.  Every face off: zeros, no kernel.
 *   _fill: the attributes of the new photons; block b writes slots slot_base[b].. and ids id_base[b]..
 *   jb_boundary_source_last: e_face / n_face of the last _count on this context (this rank's; the hosts reduce
 *     them over the ranks) and the number of boundary-source kernels launched since jb_initialize. */
typedef struct jb_boundary_source_plan {
  int32_t *nper_block;   /* host [nblocks], provided by the caller */
  double e_face[6];
  int64_t n_face[6];
} jb_boundary_source_plan;
typedef struct jb_boundary_source_record {
  double e_face[6];
  int64_t n_face[6];
  int64_t kernel_launches;
} jb_boundary_source_record;
jb_status jb_set_boundary_source(jb_context *ctx, int face, double temperature);
jb_status jb_get_boundary_source(const jb_context *ctx, int face, double *temperature);
int jb_boundary_source_enabled(const jb_context *ctx);
jb_status jb_set_boundary_source_count(jb_context *ctx, int64_t num_particles, int64_t face_cells_total);
int64_t jb_boundary_face_cells(const jb_context *ctx, const jb_mesh *mesh);
int64_t jb_boundary_prefix_words(const jb_mesh *mesh);
jb_status jb_source_boundary_count(jb_context *ctx, jb_mesh *mesh, double dt, int64_t face_cells_total,
                                   int64_t num_particles, uint32_t epoch, jb_boundary_source_plan *plan_out,
                                   int32_t *prefix_dev);
jb_status jb_source_boundary_fill(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, double t_start,
                                  double dt, const int32_t *nper_block_host, const int32_t *prefix_dev,
                                  const int64_t *slot_base_host, const uint64_t *id_base_host);
jb_status jb_boundary_source_last(const jb_context *ctx, jb_boundary_source_record *out);

/* TransportPhotons / TransportPhotons_DDMC(md, t_start, dt) -- jaybenne.hpp:59-60,
 * transport.cpp:28-181, transport_ddmc.cpp:28-237.  Particles [first,last) with status ACTIVE
 * are followed until census, absorption, escape, or until they enter a block that is not
 * resident on this rank (status OUTGOING).  Crossing into a resident block -- owned or a halo
 * copy -- does not end the launch: the swarm
 * boundary conditions (boundaries.hpp:46-82, periodic, outflow), the destination-block lookup
 * and SampleDDMCBlockFace are applied to the particle in flight.  With fuse_census_tally != 0
 * a particle reaching census in an OWNED block adds weight / cell volume to energy_tally
 * (EvaluateRadiationEnergy fused; the caller zeroes the tally first with jb_zero_energy_tally).
 * A particle that reaches census or is absorbed in a HALO copy is marked OUTGOING /
 * OUTGOING_ABSORBED: its owner tallies it after the hand-off.
 * The calls return when the kernel is launched (jb_synchronize / jb_get_transport_stats wait
 * for it), with one exception: jb_transport_photons_ddmc with gray opacities reads one flag back
 * first (does every cell take DDMC steps?) and, on a mesh that mixes IMC and DDMC cells, runs
 * three launches with the size of a work list read back before the second and the third. */
jb_status jb_transport_photons(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                               double t_start, double dt, int64_t first, int64_t last,
                               int fuse_census_tally);
jb_status jb_transport_photons_ddmc(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                    double t_start, double dt, int64_t first, int64_t last,
                                    int fuse_census_tally);
/* Arithmetic of the tracking step of the gray IMC kernels (the headline path).
 *   JB_ARITH_EXACT: every operation is the one the CPU oracle's portable flavour performs --
 *     correctly rounded quotients, the reference's unfused position update -- and the particles
 *     come out bit-identical to it.
 *   JB_ARITH_LEAN (default): while a lane follows a photon it carries the unit direction v / c and
 *     the distance left to census c (t_end - t) instead of v and t, and the position RELATIVE TO
 *     THE CENTRE OF ITS CELL instead of x, with the cell as one byte offset into the per-cell arrays
 *     (k_imc_cell; any cell widths: only the conversion from and to the
 *     swarm's coordinates, when a photon is loaded and written back, depends on them -- exact where
 *     they are powers of two, jb_mesh_exact_geometry, an ulp of the position elsewhere; the
 *     per-cell arrays of the resident blocks must lie within 4 GiB); distance to a face as
 *     (h - sgn(omega) p) / |omega| with a once-refined reciprocal of the direction component (within
 *     2^-48, ~20 ulp, of the correctly rounded quotient; in 3-D the three reciprocals come from one,
 *     of the product of the components, to the same accuracy), position update as one fused
 *     multiply-add per axis, logarithm without its compensated sum (<= 3 ulp), square root of
 *     1 - mu^2 with one residual correction (<= 2 ulp) -- every operation within 4e-15 (relative) of
 *     the exact variant's, the cell-local position carrying ~8 bits MORE than the absolute one the
 *     exact variant (and the reference) round at every event.  Both faces of an axis are tested for
 *     the nudge of transport_utils.hpp:151-159, as in the reference.  (More than 4 GiB of per-cell
 *     arrays, or JB_NO_IMC_CELL=1: the x-space form of round 3, which tests only the face ahead.)
 *     ~40 % fewer instructions per event than the exact variant.
 *     In one line: 1e-9 PER CYCLE; measured growth about one decade per cycle, 1e-4 of the domain and
 *     <= 1e-3 of the histories re-sequenced after ten cycles (the same as the CPU path's libm vs portable
 *     arithmetic); the tally within 6 sigma per cell at any length.  bench.py measures these in every
 *     default run (accuracy.lean_vs_exact_after_10_cycles).
 *     Stated tolerance (tests/test_gpu_lean.py, tests/test_gpu_accuracy.py):
 *       - after ONE full cycle every floating-point attribute of every photon is within 1e-9 of the
 *         exact variant's and of the oracle's (positions relative to the domain size, velocities to
 *         c, times to dt), after TWO within 1e-8; integer attributes and stream states equal;
 *       - beyond that the two roundings of a history separate like nearby trajectories of any
 *         chaotic system -- measured: largest position difference over 1e5 photons 5e-12 of the
 *         domain after one cycle, 1.3e-9 after two, then about a decade per cycle, 1e-4 after ten
 *         (the oracle's own libm / portable flavours, <= 1 ulp apart in log and sincos, separate
 *         at the same rate; what the lean variant differs by from the exact one is mostly the exact
 *         variant's own rounding of x to the absolute grid) -- and a photon changes its sequence of
 *         events only where a difference flips a comparison: 20 of 1e5 photons in ten cycles;
 *       - at any length: the energy tally within 6 sigma of each cell's Monte Carlo noise of the
 *         libm-arithmetic CPU path on the same streams (measured 3e-13 sigma on BASELINE
 *         configs[0], 0.016 sigma per x-plane on configs[1]'s geometry) and the reference's error
 *         metric against the analytic profile not worse than that path's + 0.01.
 * The IMC steps of a hybrid (IMC / DDMC) deck follow the same switch -- on a mesh without the
 * exact geometry (jb_mesh_exact_geometry) testing BOTH faces per axis, as the reference does: there
 * a photon that leaked from a coarse DDMC cell into a finer block can be left, unresampled and
 * with zero velocity, on a face of the fine cells (sample_ddmc_bface.cpp's fuzzy test, tolerance
 * 2e-16 dx, missing it) -- ; DDMC steps and the per-event-opacity kernels have the exact arithmetic
 * only.  JB_EXACT_ARITH=1
 * in the environment makes exact the default of jb_initialize. */
enum { JB_ARITH_EXACT = 0, JB_ARITH_LEAN = 1 };
jb_status jb_set_arithmetic(jb_context *ctx, int mode);
int jb_get_arithmetic(const jb_context *ctx);
/* the kernel the last transport call on this mesh launched: "k_transport<3, true, 2, true, true>" =
 * <NDIM, TALLY (census tally fused), GRAY (0 per-event opacities, 1 gray, 2 gray without
 * absorption), EXACT (exact cell-face arithmetic, 32-bit cell offsets), LEAN (lean arithmetic)>;
 * "k_ddmc_all<3, true>" = <NDIM, TALLY> on a mesh whose every cell takes DDMC steps (", quad gather"
 * appended when its cell records, more than 1 MiB of them, are fetched quad-cooperatively,
 * ", records in LDS" when the mesh has at most 256 cells and the kernel keeps them in LDS,
 * ", cell codes" when the mesh has at most 256 DISTINCT step records: jb_mesh_ddmc_classes -- and
 * ", cell codes, queues" when, with at most 64 resident blocks, the wave's photons are also staged
 * through queues in LDS: k_ddmc_q, the default on such meshes; ", codes in LDS" behind that when the
 * mesh has at most 1024 cells and 64 distinct records and the codes sit in LDS too);
 * "k_hybrid<2, lean, exact geometry>" on a mesh that mixes IMC and DDMC cells (three launches: IMC
 * phase, DDMC phase, remainder); "" before the first launch.  The pointer is valid until the next
 * transport call on this mesh or until the mesh is destroyed.  jb_mesh_exact_geometry: 1 if every
 * resident block has power-of-two cell widths and a lower corner that is a whole number of them
 * (and the per-cell arrays of the resident blocks span less than 4 GiB).
 * jb_last_transport_grid: the largest number of workgroups any persistent tracking launch of the
 * last transport call on this mesh used (a call makes up to three launches), 0 before the first.
 * JB_TRANSPORT_MAX_BLOCKS=k in the environment at jb_initialize caps it at k (a test aid: the
 * results do not depend on the grid; unset or <= 0: no cap).
 * jb_last_transport_unit_cell: what the variant string does not say of a "k_imc_cell<..., lean>"
 * launch -- 0: position and direction in real units; 1: in units of the half cell width (every
 * resident block has the same power-of-two cell widths: the same results bit for bit); 2: the
 * same with all active widths equal.  0 for every other kernel and before the first launch. */
const char *jb_last_transport_variant(const jb_mesh *mesh);
int jb_last_transport_grid(const jb_mesh *mesh);
int jb_last_transport_unit_cell(const jb_mesh *mesh);
int jb_mesh_exact_geometry(const jb_mesh *mesh);
/* All-DDMC meshes: the number of DISTINCT step records UpdateDerivedTransportFields found among the
 * resident cells this cycle, as the last jb_transport_photons_ddmc call read it back (0 before the
 * first; gray decks: one per level x face-neighbour pattern).  Up to 256 of them the tracking kernel
 * keeps the records in LDS and gathers a 4-byte cell code per step (variant "..., cell codes");
 * beyond (e.g. a material whose Fleck factor differs from cell to cell) it gathers the 64-byte step
 * record of the cell.  Same results either way. */
int jb_mesh_ddmc_classes(const jb_mesh *mesh);
/* counters accumulated by the transport tasks since the last reset (synchronises) */
jb_status jb_get_transport_stats(jb_context *ctx, jb_transport_stats *stats, int reset);

/* SampleDDMCBlockFace(md) -- jaybenne.hpp:61, sample_ddmc_bface.cpp:81-427; for particles
 * that arrived from another rank */
jb_status jb_sample_ddmc_block_face(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                    int64_t first, int64_t last);

/* CheckCompletion(md, t_end) -- jaybenne.hpp:62, transport.cpp:187-216: JB_ITERATE if any
 * ACTIVE particle has t < t_end, else JB_COMPLETE; the count goes to *unfinished */
jb_status jb_check_completion(jb_context *ctx, const jb_swarm_view *swarm, double t_end,
                              int64_t *unfinished);

/* EvaluateRadiationEnergy<T>(md) -- jaybenne.hpp:67-68, jaybenne.cpp:514-564 */
jb_status jb_zero_energy_tally(jb_context *ctx, jb_mesh *mesh);
jb_status jb_evaluate_radiation_energy(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm);

/* UpdateFluid(md) -- jaybenne.hpp:69, jaybenne.cpp:583-615 */
jb_status jb_update_fluid(jb_context *ctx, jb_mesh *mesh);

/* PhotonReflectBC<BFACE>(swarm) -- boundaries.hpp:24-84; face = 0..5 (ix1, ox1, ix2, ...) */
jb_status jb_photon_reflect_bc(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, int face);

/* Swarm::RemoveMarkedParticles (transport.cpp:176-178) / DefragParticles (jaybenne.cpp:499-509):
 * keeps the ACTIVE particles and the ones still waiting for their hand-off (OUTGOING, not packed yet --
 * jb_pack_outgoing / jb_exchange turn those slots into holes), closes the holes, updates swarm->n */
jb_status jb_remove_marked_particles(jb_context *ctx, jb_swarm_view *swarm);
/* jaybenne::DefragParticles (reference jaybenne.cpp:499-509: Swarm::Defrag; scheduled by no task
 * list of the reference).  The swarm is compact after jb_remove_marked_particles; this call restores
 * its ORDER: the first swarm->n particles are sorted, in place, by (resident block, cell of their
 * position) -- the order photons are sourced in, which keeps the cell data a wave gathers in the L2
 * of its XCD and which diffusion loosens from cycle to cycle (all-DDMC 3-D, 1e8 photons: 26.5 ms per
 * cycle at cycle 2, 39.9 at cycle 16).  Nothing a particle carries changes; particles of one cell
 * come out in arbitrary order (JB_CELL_ORDER_ANY, the default; jb_set_cell_order below).  Works through 128 bytes
 * of library scratch memory per particle.  Asynchronous on the context's stream. */
jb_status jb_defrag_particles(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm);
/* The order of the photons WITHIN a cell behind a sort.  JB_CELL_ORDER_ANY (the default): whatever order the waves
 * of the sort's move reached the cell's counter in -- it differs from run to run.  JB_CELL_ORDER_BY_ID, the
 * canonical order: jb_defrag_particles sorts the first swarm->n slots by the triple (sort key, id, input slot) --
 * the sort key is (resident block, cell) as above, one past the last cell for every slot that is not an ACTIVE
 * photon in a resident block; the id is compared as a full unsigned 64-bit word (bit 63 of a hole's id takes part).
 * Live ids are unique, so the output does not depend on the input's slot order; the input slot only breaks ties
 * among dead slots.  Nothing a photon carries changes, and a swarm already in this order is not moved at all: one
 * pass over (key, id) decides that and finds the largest id and key, which set the number of radix passes (8-bit
 * digits of the id, then of the key: 4 + 3 for 1e8 photons in 128^3 cells; ids with bit 63 set force all 8 of the
 * id).  In this mode the call synchronises the stream ONCE, for that 16-byte read-back.  Same limits (2^32 - 1
 * photons, 2^32 - 2 cells); scratch: 20 1/8 bytes per photon on top of the 128 (two 8-byte (word, slot) arrays,
 * the 4-byte destinations, the digit counts); if it cannot be allocated the swarm is left as it was and JB_ERR_HIP
 * is returned, as in the default mode.  No atomics on photons' data, no floating point: the same photons give the
 * same slots, bit for bit, whatever order they came in.  jb_defrag_policy sorts this way too when the mode is on
 * (and times the sort as S as before: a dearer sort is scheduled less often); so does jb_comb_census_plan.
 * With the mode off no kernel of the canonical sort is launched and every call does what it did.
 * JB_CELL_ORDER=id in the environment makes BY_ID the default of jb_initialize.  jb_set_cell_order: JB_ERR_INVALID
 * for any other mode (the mode stays); changing the mode discards a plan of jb_comb_census_plan not yet applied. */
enum { JB_CELL_ORDER_ANY = 0, JB_CELL_ORDER_BY_ID = 1 };
jb_status jb_set_cell_order(jb_context *ctx, int mode);
int jb_get_cell_order(const jb_context *ctx);
/* The default schedule of DefragParticles ("defrag_interval = -1", what RadiationStep of the hosts
 * calls at the end of a cycle, after it has read the cycle's event count): the library times the
 * tracking kernels of every jb_transport_photons* call and every sort with HIP events on the
 * context's stream.  It keeps the lowest time per event seen since the last sort and adds up what
 * the cycles since have cost above it (the loss L); the swarm is sorted (*sorted = 1) when one more
 * cycle in the present order would cost more than a cycle has cost on average since the last sort,
 * the sort included -- e(p + 1) >= (S + L) / p with p cycles behind the sort, S the cost of a sort
 * (measured; 15 ms per 1e8 photons until one has been) and e(p + 1) this cycle's loss extrapolated
 * linearly: the period with the lowest cost per cycle for a loss that keeps growing -- and the current
 * cycle is at least 1.5 % slower than the best one, at least 2 cycles after the last sort and with
 * at least 2^20 photons in the swarm.  A sort after which the next cycle is not at least 1 % faster
 * was not what the kernels needed: the minimum distance between sorts doubles (2, 4, .. 256 cycles)
 * until one pays
 * again.  The sort's scratch records (128 bytes per photon) are allocated when the cycles first slow down
 * by 0.5 % (at least a cycle before a sort can be decided, so that the allocation -- ~30 ms per GB -- does
 * not land in the sorting cycle; a run whose swarm keeps its order never allocates them);
 * jb_release_scratch returns them.
 * Slot order only affects speed, never results -- but under this schedule WHEN the swarm is sorted
 * depends on measured times, so the order of the slots (not what any photon carries: compare photons by
 * their creation id) differs from run to run; defrag_interval = 0 in the hosts keeps the order of the
 * reference (never sorted, reproducible slot for slot), k > 0 sorts after every k-th cycle.
 * The caller must have synchronised the stream since the cycle's last transport call.
 * mode: JB_DEFRAG_DECIDE_AND_SORT for a host that holds the whole swarm.  Several ranks sort
 * TOGETHER (a cycle is as long as its slowest rank: a sort on one rank per cycle, in turn, would be
 * paid every cycle): every rank calls with JB_DEFRAG_DECIDE (*sorted = 1: this rank would sort),
 * the host reduces that over the ranks (max) and, if any rank asked, every rank calls again with
 * JB_DEFRAG_SORT_NOW. */
enum { JB_DEFRAG_DECIDE_AND_SORT = 0, JB_DEFRAG_DECIDE = 1, JB_DEFRAG_SORT_NOW = 2 };
jb_status jb_defrag_policy(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                           int64_t events_this_cycle, int32_t mode, int32_t *sorted);
/* Gives the library's scratch memory back (synchronises the stream first).  The scratch buffer
 * grows on demand and is otherwise kept for the life of the context: 128 bytes per photon after a
 * DefragParticles (sized exactly), a few bytes per photon for the hole / hand-off lists.  If it cannot
 * be allocated, jb_defrag_particles returns JB_ERR_HIP and leaves the swarm as it was; jb_defrag_policy
 * then skips the sort with a message on stderr and stops asking. */
jb_status jb_release_scratch(jb_context *ctx);

/* Census population control: an energy-conserving comb per cell (the reference has none: nothing there ever
 * reduces the number of photons, and a deck with do_emission adds num_particles per cycle).  Called between two
 * cycles.  A cell that holds more than trigger_T ACTIVE photons comes out with exactly target_K,
 * 1 <= target_K <= trigger_T; every other cell, and every slot that is not ACTIVE, is left bit for bit as it was.
 * For a combed cell with photons j = 1..m in the slot order the sort left them, W = sum w_j, D = W / K,
 * C_j = w_1 + .. + w_j and xi one uniform in (0,1) per cell and epoch:
 *     u_0 = 0,   u_j = clamp(ceil(C_j / D - xi), 0, K) for j < m,   u_m = K,
 * and photon j comes out as k_j = u_j - u_(j-1) copies of weight D.  sum k_j = K; k_j is floor(w_j / D) or
 * ceil(w_j / D); the expectation of k_j D over xi is w_j; the cell's energy is conserved to rounding.
 * A copy carries everything its original carries (position, direction, time, e, indices, block, status).  The
 * first copy also keeps id and stream state; every further copy takes the next unused creation id -- handed out in
 * output-slot order over the call, from id_base -- and starts that id's stream (what the source gives a new
 * photon, so the streams stay disjoint).
 *     xi = uniform of the state  seed_state(seed, domain 2, epoch << 44 | global block id << 24 | cell),
 * cell = the cell's index in the block's array (ghost cells included, < 2^24), epoch < 2^20 the cycle number:
 * the draw does not depend on how the blocks are dealt to ranks.
 * A cell whose weight is not positive and finite is left alone.  Weights are taken to be non-negative.
 *
 * jb_comb_census_plan sorts the swarm by (block, cell) -- jb_defrag_particles; slots that are not ACTIVE end up
 * behind all cells; a swarm that is in that order already is not moved, so the same sorted swarm gives the same
 * bits --, forms the running weights with a segmented scan, decides k_j for every slot and reads
 * back the plan; it synchronises the stream.  Nothing a photon carries has changed yet.  When no cell exceeds
 * trigger_T, n_after == n_before and cells_combed == 0: the host skips jb_comb_census_apply.  For the schedule of
 * jb_defrag_policy a plan that sorted counts as a sort (the policy starts over from the sorted order; the sort's cost per
 * photon it keeps is that of the last sort it timed itself).
 * jb_comb_census_apply moves survivors and copies into a compact swarm that is still in (block, cell) order,
 * sets swarm->n (n_after <= n_before: the call never needs capacity) and reports the census energy behind it,
 * summed in a fixed order; it synchronises too.  The plan lives in the library's scratch memory: no other call
 * that uses this context may come between the two.
 * Which photons of a cell survive depends on the order the sort left them in.  JB_CELL_ORDER_ANY (the default): that
 * order is arbitrary within a cell -- counts, energies per cell and the distribution do not differ from run to run,
 * the surviving ids can.  JB_CELL_ORDER_BY_ID (jb_set_cell_order): the plan asks "in canonical order already?" and
 * otherwise runs the canonical sort (sorted reports which), so the photons of a cell are combed in the order of
 * their creation ids: the survivors, the weights and the id every further copy takes are then a function of the
 * photons alone, not of their slots -- the same from run to run, whenever the swarm was last sorted and however
 * the blocks are dealt to ranks.  To that end the running weights C_j are formed exactly in this mode -- 128-bit
 * fixed-point sums on the scale of the cell's largest weight (weights below 2^-95 of it are truncated, negative ones
 * count as zero), each rounded once -- because a floating-point sum tree aligned to the swarm's slots would round
 * the same cell differently at another offset.  In the output of jb_comb_census_apply the survivors (first copies) are again in
 * canonical order; a further copy sits right behind its original with an id above every old one, so the next
 * canonical sort moves it behind the cell's older photons -- the same way in every run.
 * JB_ERR_INVALID: target_K < 1, target_K > trigger_T, trigger_T >= 2^32, epoch >= 2^20, the limits of
 * jb_defrag_particles (2^32 - 1 photons, 2^32 - 2 cells), apply without a plan for this swarm.  Scratch: what the
 * sort takes plus 16 bytes per photon; if it cannot be allocated, JB_ERR_HIP and the swarm is as it was. */
typedef struct jb_comb_plan {
  int64_t n_before;      /* swarm->n */
  int64_t n_after;       /* ... behind jb_comb_census_apply */
  int64_t n_new_ids;     /* creation ids apply hands out: id_base .. id_base + n_new_ids - 1 */
  int64_t cells_combed;
  int64_t max_per_cell;  /* most ACTIVE photons in one cell, before the comb */
  double e_before;       /* weight of the ACTIVE photons, summed in a fixed order */
  int64_t sorted;        /* 1: the plan sorted the swarm; 0: it was in (block, cell) order -- under
                          * JB_CELL_ORDER_BY_ID: in canonical order -- already */
} jb_comb_plan;
typedef struct jb_comb_report {
  int64_t n_after;
  int64_t n_new_ids;
  double e_after;        /* weight of the ACTIVE photons behind the comb, summed in the same order */
} jb_comb_report;
jb_status jb_comb_census_plan(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, int64_t trigger_T,
                              int64_t target_K, uint32_t epoch, jb_comb_plan *out);
jb_status jb_comb_census_apply(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, uint64_t id_base,
                               jb_comb_report *out);

/* Census population control for the whole mesh: a GLOBAL comb (jaybenne_amd/csrc/jb_kernel_gcomb.hpp).  The per-cell
 * comb above bounds a cell, not the swarm, and never splits.  This one holds the swarm near target_N photons of
 * equal weight: target_N is dealt to the cells in proportion to the census energy they hold; cells above their share
 * are thinned, cells below it are split, each cell's energy is conserved.  Off unless a host calls it.
 * The rule.  Every operation is individually rounded; no product is fused with a sum.
 *   1. jb_comb_census_weigh brings the swarm into (block, cell) order exactly as jb_comb_census_plan does -- the
 *      "in order already?" test, the canonical sort under JB_CELL_ORDER_BY_ID, the restart of jb_defrag_policy's
 *      schedule when the sort moved anything -- and forms the running weights C_j with the same segmented scan
 *      (floating point by default, exact 128-bit sums rounded once under JB_CELL_ORDER_BY_ID).
 *   2. For cell key k (ghost cells of the block's array included) m_k is its number of ACTIVE photons and
 *      W_k = C[end - 1].  The cell is VALID iff m_k >= 1 and 0 < W_k < inf; an invalid cell is never touched and
 *      contributes +0.0.  e_block[b] = the sum of W_k over all cells of resident block b in cell-index order with the
 *      tree of jb_source_energy_sums (thread t adds cells t, t + 256, ... from +0.0, then s[t] += s[t + d],
 *      d = 128 ... 1); 0 for a halo copy.  No floating-point atomics.
 *   3. The host gathers the block sums by global block id (as bit patterns through an integer all-reduce), adds them
 *      with jb_source_energy_total to W_tot and passes it as w_total.  If w_total is not > 0 or not finite, nothing
 *      is combed (n_after == n_before).  Otherwise scale = (double)target_N / w_total, one division.
 *   4. nu = W_k scale, f = floor(nu), K_k = f + ((nu - f) > xi'_k), xi'_k the first uniform of
 *      seed_state(seed, domain 9, epoch << 44 | global block id << 24 | cell) -- keyed as xi of the per-cell comb is,
 *      in a domain of its own.  Then K_k = max(K_k, 1) (no roulette: every occupied cell keeps its energy), then
 *      K_k = min(K_k, split_max m_k, 2^32 - 1), compared in double.
 *   5. The cell is COMBED iff (double)m_k > band K_k or K_k > band (double)m_k.  Every other cell, and every slot
 *      that is not ACTIVE, comes out bit for bit as it was.
 *   6. A combed cell comes out as exactly K_k copies of weight W_k / K_k by the rule above with K = K_k and the
 *      same xi (domain 2); u_m = K_k; C_(j-1) is the neighbouring slot's stored value.  The first copy keeps id and
 *      stream state; a further copy takes id_base + offset, offsets in output-slot order, and that id's stream start.
 * K_k depends on W_k and xi'_k alone, not on the selection, and K_k >= 1: the comb is unbiased and each cell's energy
 * is conserved to rounding.  Under JB_CELL_ORDER_BY_ID every input of the rule is a function of the photons alone, so
 * survivors, weights and new ids do not depend on how the blocks are dealt to ranks.  With band > 1 the population is
 * bounded by band target_N + occupied cells, not by target_N.  Copies of a split photon start at one point and
 * separate only through their streams.
 * jb_comb_census_weigh: n_room is the most slots jb_comb_census_apply may fill, swarm->n <= n_room <=
 * swarm->capacity (else JB_ERR_INVALID); ALL scratch is taken here, before the sort (what the comb takes, 4 bytes per
 * photon, and 128 bytes per slot of n_room when n_room > n).  e_block_host: one double per resident block.
 * report: n_before, e_before and sorted are set, n_after = n_before, the rest 0.
 * jb_comb_census_plan_global must follow a weigh on the same swarm and scratch generation with no other call on this
 * context in between (else JB_ERR_INVALID); it reads back the plan.  n_after > n_room: JB_ERR_CAPACITY, nothing a
 * photon carries has changed.  JB_ERR_INVALID: target_N < 1 or >= 2^31, band < 1 or not finite, split_max < 1,
 * epoch >= 2^20.  jb_comb_census_apply serves both kinds of plan (sets swarm->n = n_after, which may exceed n_before
 * here).  jb_radiation_step_ranks and the Parthenon adapter do not drive the global comb; a replicated mesh is not
 * covered (the photons of a cell must lie on one rank). */
typedef struct jb_comb_global_plan {
  int64_t n_before;       /* swarm->n */
  int64_t n_after;        /* ... behind jb_comb_census_apply */
  int64_t n_new_ids;      /* creation ids apply hands out: id_base .. id_base + n_new_ids - 1 */
  int64_t cells_thinned;  /* combed cells with K_k < m_k */
  int64_t cells_split;    /* combed cells with K_k > m_k */
  int64_t max_per_cell;   /* most ACTIVE photons in one cell, before the comb */
  int64_t max_target;     /* largest K_k of a valid cell, combed or not */
  int64_t sorted;         /* 1: the weigh sorted the swarm */
  double e_before;        /* weight of the ACTIVE photons, summed in the order jb_comb_plan.e_before is */
} jb_comb_global_plan;
jb_status jb_comb_census_weigh(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, int64_t n_room,
                               double *e_block_host, jb_comb_global_plan *report);
/* Kernels of jb_kernel_gcomb.hpp launched on this context so far: 0 as long as no host has called the global comb. */
int64_t jb_gcomb_kernel_launches(const jb_context *ctx);
jb_status jb_comb_census_plan_global(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, double w_total,
                                     int64_t target_N, double band, int64_t split_max, uint32_t epoch,
                                     jb_comb_global_plan *plan);

/* ---- radiation moments: per-cell count, energy density, flux and second-moment tensor of the census
 * (jaybenne_amd/csrc/jb_kernel_moments.hpp).  The reference has none: energy_tally is the zeroth angular moment
 * alone, and its tests copy the swarm to the host for anything else.  Called between two cycles.
 * For every interior cell of every OWNED resident block, JB_MOMENTS = 12 doubles over the ACTIVE photons whose
 * sort key is that cell -- the key jb_defrag_particles orders by: the cell of the photon's POSITION clamped to the
 * block's array (not ip, jp, kp).  With v = c Omega the photon's velocity, p_d = w v_d and dv = (dx0 dx1) dx2 of
 * the block, as the energy tally forms it:
 *     JB_MOM_N              the number of photons, as a double
 *     JB_MOM_E              (sum of w) / dv                 the energy density (energy_tally, summed otherwise)
 *     JB_MOM_W2             sum of w w                      N_eff = (E dv)^2 / W2 equal-weight photons stand behind E
 *     JB_MOM_FX, FY, FZ     (sum of p_d) / dv               the energy flux
 *     JB_MOM_QXX .. QZZ     (sum of p_i v_j) / dv, i <= j   Q / c^2 is the pressure tensor, Q_ij / (c^2 E) Eddington's
 * Every product is rounded on its own, the division is one rounding of the sum, and all three velocity components
 * take part whatever ndim is.  Cells of halo copies and empty cells get twelve zeros: every word of out_dev is
 * written.  Not counted (report->n_skipped): slots that are not ACTIVE, ACTIVE slots whose blk is outside
 * [0, nblocks), photons of halo copies, and photons whose clamped position lies in a ghost cell.
 * out_dev: a caller-owned device array [JB_MOMENTS][nblocks][ncell] (jb_moments_words doubles), interior cells in
 * (k, j, i) order, blocks in the mesh's resident order.
 * Order of summation -- what makes the result a function of the cell's photons in their slot order and of nothing
 * else (not of the cell's offset in the swarm, the launch geometry or the run): the cell's photons are a run of L
 * consecutive slots a_0 .. a_(L-1) of the sorted swarm.  The run is cut into chunks of 4096 slots counted from
 * its head; in a chunk "lane" l = 0 .. 63 starts from +0.0 and adds the elements l, l + 64, l + 128, .. in rising
 * order; the 64 lane sums are joined by  for d in 32, 16, 8, 4, 2, 1: s[l] = s[l] + s[l + d] for l < d;  the run's
 * sum is the first chunk's sum with the further chunks' sums added in chunk order.  No floating-point atomics.
 * The call asks "in (block, cell) order already?" as jb_comb_census_plan does and sorts with jb_defrag_particles
 * if not (report->sorted; for jb_defrag_policy that counts as a sort, exactly as a comb plan that sorted does).
 * JB_CELL_ORDER_ANY: the order within a cell is then whatever the sort left, and a swarm already in key order is
 * not moved -- the same sorted swarm gives the same bits.  JB_CELL_ORDER_BY_ID: the question is "in canonical
 * order?", the sort the canonical one, and the result a function of the photons alone, whatever slots they came in
 * and however the blocks are dealt to ranks.
 * Stream synchronisations: ONE in either mode (the read-back of the order test: 4 bytes, or the 16 of the
 * canonical sort's test), none for n = 0; ONE more when report is not NULL.  Otherwise asynchronous on the
 * context's stream.  Scratch: what the sort takes, plus 176 bytes per 4096 photons; a comb plan not yet applied
 * is discarded.  Limits: those of jb_defrag_particles (2^32 - 1 photons, 2^32 - 2 cells).
 * Left as they were: energy_tally, energy_delta, open deposit accumulators, and everything a photon carries -- the
 * slots aside, which the sort permutes.
 * Limitation: in DDMC cells the census direction is the resampled isotropic one (reference
 * transport_utils.hpp:265-276), so there Q is the isotropic tensor and F carries no diffusive flux.
 * JB_ERR_INVALID: a null ctx, mesh, swarm or out_dev, or the sort's limits; JB_ERR_HIP with the swarm as it was
 * when the scratch cannot be allocated.  n = 0 is valid and writes zeros.
 * Opens the trace range "Jaybenne::EvaluateRadiationMoments". */
enum { JB_MOM_N = 0, JB_MOM_E, JB_MOM_W2, JB_MOM_FX, JB_MOM_FY, JB_MOM_FZ,
       JB_MOM_QXX, JB_MOM_QXY, JB_MOM_QXZ, JB_MOM_QYY, JB_MOM_QYZ, JB_MOM_QZZ, JB_MOMENTS };
typedef struct jb_moments_report {
  int64_t n_counted, n_skipped;      /* slots of [0, n) summed / not summed */
  int64_t cells_nonempty, longest_run;
  int32_t sorted, pad;               /* 1: the call had to sort */
} jb_moments_report;
int64_t jb_moments_words(const jb_mesh *mesh);      /* JB_MOMENTS * nblocks * ncell */
jb_status jb_evaluate_radiation_moments(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                        double *out_dev, jb_moments_report *report /* or NULL */);
/* The same into a HOST array of jb_moments_words doubles, for a host that allocates no device memory of its own:
 * through a device array the context keeps (jb_release_scratch returns it); synchronises the stream at the end. */
jb_status jb_evaluate_radiation_moments_host(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                             double *out_host, jb_moments_report *report /* or NULL */);

/* ---- radiation spectrum: per-cell energy density of the census in frequency groups
 * (jaybenne_amd/csrc/jb_kernel_spectrum.hpp).  Every photon carries its energy e -- both sources draw it from a
 * Planck law, and under EPBremss it is the frequency the absorption opacity is evaluated at --, and energy_tally,
 * the moments and the ledger all integrate over it.  A sibling of jb_evaluate_radiation_moments, called between
 * two cycles, with that call's rules wherever nothing else is said here.
 * edges_host[0 .. ngroups]: ngroups + 1 finite, strictly increasing doubles on the host (read before the call returns),
 * 1 <= ngroups <= JB_SPECTRUM_MAX_GROUPS.  There are NB = ngroups + 2 bins, and
 *     THE BIN OF A PHOTON IS THE NUMBER OF EDGES j WITH edges[j] <= e.
 * Bin 0 is below the first edge -- and takes an e that is NaN, negative, zero or -inf: every comparison is false --,
 * bins g = 1 .. ngroups are the groups [edges[g - 1], edges[g]), bin ngroups + 1 is at or above the last edge, +inf
 * included.  The rule is applied literally, by comparisons, with no logarithm or reciprocal bin width: edges are
 * data, and a photon that sits on an edge lands in the same bin in every implementation.
 * out_dev: a caller-owned device array [NB][nblocks][ncell] (jb_spectrum_words doubles), interior cells in (k, j, i)
 * order, blocks in the mesh's resident order:
 *     out[bin][block][cell] = (sum of w over the cell's ACTIVE photons in that bin) / dv,   dv = (dx0 dx1) dx2,
 * the division one rounding.  Which photons count (the sort key's cell) and which are skipped is the moments'
 * rule; cells of halo copies and empty cells get zeros: every word of out_dev is written.
 * Order of summation: for each bin the moments' order over the positions of the cell's run -- the run is cut into
 * chunks of 4096 slots counted from its head; in a chunk "lane" l = 0 .. 63 starts from +0.0 and adds the elements
 * l, l + 64, l + 128, .. in rising order; the 64 lane sums are joined by  for d in 32, 16, 8, 4, 2, 1: s[l] = s[l] +
 * s[l + d] for l < d;  the run's sum is the first chunk's sum with the further chunks' sums added in chunk order.
 * A photon's addend to its own bin is w; for every other bin the photon is skipped -- a lane sum that starts from
 * +0.0 is never -0.0, so skipping equals adding +0.0, bit for bit.  No floating-point atomics.  Consequences:
 * with edges = {4.9e-324, DBL_MAX} and every e positive and finite, bin 1 is JB_MOM_E of
 * jb_evaluate_radiation_moments on the same swarm bit for bit; the result does not depend on the launch geometry,
 * on the lanes per cell or on where the cell lies in the swarm; under JB_CELL_ORDER_BY_ID it does not depend on the
 * slot order or on the number of ranks the blocks are dealt to (a cell's photons on one rank: a block partition; the
 * sum of several ranks' arrays on a replicated mesh is another order of summation).
 * As jb_evaluate_radiation_moments: the question "in order already?" and the sort under either cell order
 * (report->sorted; a sort for jb_defrag_policy); ONE stream synchronisation, none for n = 0, ONE more when report
 * is not NULL (the edges travel as a kernel argument: no copy to wait for); a comb plan not yet applied is discarded;
 * energy_tally, energy_delta, open deposit accumulators and everything a photon carries are left as they were,
 * the slots aside, which the sort permutes; the sort's limits.  Scratch: what the sort takes, plus 16 NB bytes per
 * 4096 photons.
 * report: n_counted .. sorted as jb_moments_report's; n_below, n_above: the counted photons in bin 0 and in bin
 * ngroups + 1.
 * JB_ERR_INVALID: a null ctx, mesh, swarm, edges_host or out_dev, the sort's limits, ngroups outside
 * [1, JB_SPECTRUM_MAX_GROUPS], an edge that is not finite or not above the one before it -- then nothing is
 * launched and nothing written; JB_ERR_HIP with the swarm as it was when the scratch cannot be allocated.  n = 0
 * is valid and writes zeros.  Opens the trace range "Jaybenne::EvaluateRadiationSpectrum". */
#define JB_SPECTRUM_MAX_GROUPS 64
typedef struct jb_spectrum_report {
  int64_t n_counted, n_skipped;      /* slots of [0, n) summed / not summed */
  int64_t cells_nonempty, longest_run;
  int64_t n_below, n_above;          /* counted photons in bin 0 / bin ngroups + 1 */
  int32_t sorted, pad;               /* 1: the call had to sort */
} jb_spectrum_report;
int64_t jb_spectrum_words(const jb_mesh *mesh, int ngroups);   /* (ngroups + 2) * nblocks * ncell; 0: bad ngroups */
jb_status jb_evaluate_radiation_spectrum(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                         const double *edges_host, int ngroups, double *out_dev,
                                         jb_spectrum_report *report /* or NULL */);
/* The same into a HOST array of jb_spectrum_words doubles, through a device array the context keeps
 * (jb_release_scratch returns it); synchronises the stream at the end. */
jb_status jb_evaluate_radiation_spectrum_host(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                              const double *edges_host, int ngroups, double *out_host,
                                              jb_spectrum_report *report /* or NULL */);

/* MeshSend / MeshReceive (jaybenne.cpp:36-61) for the inter-rank part: OUTGOING particles are
 * among [first,last) are copied into fixed-size records (JB_RECORD_WORDS x 8 bytes), ordered by
 * destination rank, and their slots are re-marked JB_ST_ABSORBED-like holes (status
 * JB_ST_ESCAPED is kept for escapes; packed particles become JB_ST_ABSORBED so that a later
 * pack does not send them twice).  counts_host[r] = records for rank r.  Unpack appends records
 * to the swarm as ACTIVE particles of this rank's blocks. */
#define JB_RECORD_WORDS 13
jb_status jb_pack_outgoing(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                           int64_t first, int64_t last, int nranks, int64_t *records_dev,
                           int64_t record_capacity, int64_t *counts_host);
jb_status jb_unpack_incoming(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm,
                             const int64_t *records_dev, int64_t nrecords);

/* MeshResetCommunication -> MeshSend -> MeshReceive (jaybenne.cpp:26-61) in ONE call, the records never
 * leaving the device: the OUTGOING particles among [first,last) are counted per destination rank on the
 * device; the transport gathers every rank's counts into the rank x rank matrix straight from that buffer;
 * the matrix is read back once (the only host read-back of the call: nranks (nranks + 3) words -- it carries this
 * rank's receive sizes and *moved_anywhere, the answer to the completion question of jaybenne.cpp:130-131);
 * if anything moved anywhere the records are packed into send_dev, exchanged into recv_dev and appended to
 * the swarm, everything on the context's stream (the call returns when the unpack kernel is launched).
 * *nsent / *nreceived: records this rank handed over / took in.
 * JB_ERR_CAPACITY (nothing has been packed or changed yet; *nsent / *nreceived hold what THIS rank
 * needs; jb_last_error names the rank that lacks room): some rank's buffer or swarm is too small.  Every
 * rank's room travels with its counts in the all-gather, so EVERY rank returns this status in the same
 * call -- none is left waiting in the payload exchange -- and every rank calls again: after growing what
 * was too small, or closing its swarm's holes with jb_remove_marked_particles, with [first,last) =
 * [0, swarm->n) (what still has to go is found by its status).
 *
 * A jb_exchange_transport is the two collectives of the exchange on DEVICE buffers, enqueued on the given
 * HIP stream (0 = success): all_gather_u64 -- count words of every rank, in rank order; all_to_all_v --
 * send_counts[r] records of `words` 8-byte words at send_offsets[r] (in records) to rank r, recv_counts[r]
 * from rank r to recv_offsets[r].  jb_transport_rccl makes the production one from an RCCL communicator
 * (ncclComm_t, one rank per GPU): ncclAllGather and one grouped ncclSend / ncclRecv per peer -- xGMI is a
 * full point-to-point mesh, every rank pair moves its records over its own link.  RCCL is loaded with
 * dlopen when the first transport is made; the library does not link against it.  A host with another
 * fabric fills the struct with its own functions (examples/handoff_mpi.cpp: MPI with host staging). */
typedef struct jb_exchange_transport {
  void *handle;
  int (*all_gather_u64)(void *handle, const uint64_t *in_dev, uint64_t *out_dev, int count, void *hip_stream);
  int (*all_to_all_v)(void *handle, const int64_t *send_dev, const int64_t *send_counts,
                      const int64_t *send_offsets, int64_t *recv_dev, const int64_t *recv_counts,
                      const int64_t *recv_offsets, int words, void *hip_stream);
} jb_exchange_transport;
jb_status jb_transport_rccl(void *nccl_comm, int rank, int nranks, jb_exchange_transport *out);
jb_status jb_transport_release(jb_exchange_transport *transport);
jb_status jb_exchange(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, int64_t first, int64_t last,
                      int rank, int nranks, const jb_exchange_transport *transport,
                      int64_t *send_dev, int64_t send_capacity, int64_t *recv_dev, int64_t recv_capacity,
                      int64_t *nsent, int64_t *nreceived, int64_t *moved_anywhere);

/* Ghost-zone / halo refresh of one host field -- the role of Parthenon's boundary exchange on
 * the host's FillGhost fields (mcblock.cpp:66-70: density, internal_energy; driven from
 * McblockDriver::HostUpdateTasks, mcblock_driver.cpp:58-74, after UpdateFluid changed
 * internal_energy).  `field` names a member of jb_mesh_view (enum jb_field).
 *   jb_gather_cells: out_dev[i] = field[blk_dev[i]][cell_dev[i]] -- packs the cells another rank
 *     asked for (cell = flat index into the block's [nk][nj][ni] array, ghosts included).
 *   jb_fill_cells: field[dst_blk_dev[i]][dst_cell_dev[i]] = mean of nsamples (a power of two)
 *     source values, summed pairwise (exact when the samples are equal); source s of destination
 *     i is field[src_blk_dev[i*nsamples+s]][src_cell_dev[i*nsamples+s]], or, when that src_blk is
 *     -1, remote_dev[src_cell_dev[i*nsamples+s]] (values received from other ranks).
 * Sources must not be destinations of the same call. */
typedef enum jb_field {
  JB_FIELD_RHO = 0, JB_FIELD_SIE = 1, JB_FIELD_U = 2, JB_FIELD_FLECK = 3, JB_FIELD_TALLY = 4,
  JB_FIELD_EDELTA = 5
} jb_field;
jb_status jb_gather_cells(jb_context *ctx, jb_mesh *mesh, int field, int64_t n,
                          const int32_t *blk_dev, const int32_t *cell_dev, double *out_dev);
jb_status jb_fill_cells(jb_context *ctx, jb_mesh *mesh, int field, int64_t n, int nsamples,
                        const int32_t *dst_blk_dev, const int32_t *dst_cell_dev,
                        const int32_t *src_blk_dev, const int32_t *src_cell_dev,
                        const double *remote_dev);

/* EstimateTimestepMesh(md) -- jaybenne.hpp:75, jaybenne.cpp:271-275 */
double jb_estimate_timestep(const jb_context *ctx);

/* RadiationStep(pmesh, t_start, dt) for a mesh held by ONE rank -- jaybenne.hpp:72,
 * jaybenne.cpp:68-151: derived fields, emission source, transport to completion, census tally,
 * fluid update.  next_id: first unused stream id (updated); cycle: the number of radiation cycles
 * taken so far (0 after initialisation; incremented at ENTRY) -- the emission source of cycle k keys
 * its per-cell rounding streams with epoch k, as every host does (jaybenne_amd.hpp: SourceEpoch).
 * (Changed in round 4: the counter used to be a source-call counter incremented AFTER the source; a
 * caller that still passes 1 for the first cycle gets epoch 2 and different -- equally valid -- rounding
 * streams than the other hosts.  JB_ERR_INVALID for *cycle >= 2^19 - 1: beyond that the keys of the
 * emission and the in-cycle thermal source, (1 << 19) | cycle, would meet.)
 * With a boundary source face on (jb_set_boundary_source) the boundary source runs behind the emission source, with
 * the N_b and face-cell count of jb_set_boundary_source_count and the library's own prefix workspace; the ledger's
 * sourced sweep covers both. */
jb_status jb_radiation_step(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, double t_start,
                            double dt, uint64_t *next_id, uint32_t *cycle, int32_t *prefix_dev);

/* RadiationStep(pmesh, t_start, dt) for a BLOCK-PARTITIONED mesh, on every rank -- jaybenne.cpp:68-151 with
 * its iterate-sublist (:113-131) inside the call: derived fields; the emission source (blocks_in_call = the
 * blocks this rank OWNS, sourcing.cpp:68-69; stream ids and slots by PlanSource of jaybenne_amd.hpp over every
 * rank's counts; *next_id advances by the GLOBAL total); the census tally zeroed; then, at most
 * max_transport_iterations times, transport of [first, n) with the fused census tally -> jb_exchange over
 * comm->transport -> stop when nothing moved anywhere -> SampleDDMCBlockFace on the arrivals (DDMC); the
 * marked particles removed; UpdateFluid.  The photons are those of the same task list driven by hand
 * (jaybenne_amd/jaybenne.py) bit for bit.  DefragParticles (jb_defrag_policy) and the refresh of the halo
 * copies after UpdateFluid stay with the host, as for jb_radiation_step.
 *
 * Collective contract: every rank of comm calls with the same cycle, t_start, dt and *next_id, and every
 * rank returns the same status from the same call:
 *   - the first collective is an all-gather of [status word | this rank's new photons per GLOBAL block],
 *     made on every step (emission or not); before it the call checks its arguments, allocates all it
 *     needs (the count matrix of jb_exchange, the record buffers, the gather buffer), counts the emission
 *     and calls reserve for its new photons.  A rank that fails there puts its verdict in the status
 *     word: every rank then returns that error (the lowest failing rank's), none is left in a collective;
 *   - JB_ERR_CAPACITY of jb_exchange comes out on every rank in the same call: each grows the record
 *     buffers the library owns (released by jb_release_scratch), closes its swarm's holes and calls
 *     reserve if the swarm is still short, and all call again over [0, n) -- at most 4 calls per
 *     transport iteration, then JB_ERR_CAPACITY on every rank (report->capacity_rounds counts them);
 *   - JB_ITERATE when max_transport_iterations passes did not empty the sublist (moved_anywhere is global:
 *     on every rank alike); neither tally nor fluid is then updated.
 * The library's other failures (a HIP error in a kernel, a failing collective) are local, as in the
 * task calls themselves.
 * Boundary source (a face on, on every rank alike): its count and the reserve for its photons happen before the
 * first collective, like the emission's; the all-gather keeps its shape and the per-block word carries
 * n_em + n_bs; the fill follows the emission fill (PlanSourceWithBoundary of jaybenne_amd.hpp).
 * Checked first, with JB_ERR_INVALID and no collective: null pointers, rank outside [0, nranks) or not the
 * mesh view's rank, nranks below the owners of the view, transport missing when nranks > 1, and a view
 * with ONE owner under nranks > 1 -- a replicated mesh (every rank holds every block: jb_mesh_view cannot
 * tell it from a single-rank mesh) is not driven by this call.  nranks == 1 with transport == NULL:
 * exactly jb_radiation_step.  report may be NULL. */
typedef struct jb_rank_comm {
  int32_t rank, nranks;                     /* rank must equal the mesh view's rank */
  const jb_exchange_transport *transport;   /* its two collectives; may be NULL when nranks == 1 */
  void *host;                               /* handed back to reserve */
  /* optional: room for >= n_slots particles (grow the device arrays, carry 0..n-1 over, update swarm's
   * pointers and capacity); 0 = success.  NULL: the swarm must already have the room. */
  int (*reserve)(void *host, jb_swarm_view *swarm, int64_t n_slots);
} jb_rank_comm;
typedef struct jb_step_report {
  int32_t transport_iterations, capacity_rounds;
  int64_t sent, received, events;           /* this rank, this step */
} jb_step_report;
jb_status jb_radiation_step_ranks(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, double t_start,
                                  double dt, uint64_t *next_id, uint32_t *cycle, int32_t *prefix_dev,
                                  const jb_rank_comm *comm, jb_step_report *report);

/* ---- energy ledger -- how much energy went where in one radiation cycle, summed on the device (the
 * reference has no such task: its hosts see counts only, and an escaped photon's weight vanishes when
 * RemoveMarkedParticles closes its slot).  Off by default; with it off none of its kernels is launched and
 * every call above behaves exactly as without it.  All terms are per cycle, for the blocks this rank owns.
 * With E0 the e_census of the cycle before (of the initial swarm for the first: a jb_ledger_close before the
 * first step returns it), summed over all ranks,
 *     E0 + e_sourced = e_census + e_absorbed + sum_f e_escaped[f] + e_escaped_unclassified
 * to rounding; the hosts print the residual relative to the left-hand side.
 * The sums use no floating-point atomics (csrc/jb_kernel_ledger.hpp: registers -> LDS -> one line of partial
 * sums per workgroup -> one workgroup that adds them in a fixed order): the same call on the same swarm gives
 * the same bits.  Everything is enqueued on the context's stream; only jb_ledger_close synchronises (one
 * copy of 184 bytes). */
typedef struct jb_energy_ledger {
  /* sum of w and number of the photons the emission source created this cycle (the slots SourcePhotons filled) */
  double e_sourced; int64_t n_sourced;
  /* ... of the photons that ended JB_ST_ESCAPED this cycle, by face (ix1, ox1, ix2, ox2, ix3, ox3): the first
   * active axis d, in the order x1, x2, x3, on which the position left in the slot lies strictly outside --
   * x_d < gmin[d]: face 2 d, x_d > gmax[d]: face 2 d + 1 -- the test on which the swarm boundaries let a
   * photon go (boundaries.hpp:46-82 + Parthenon's outflow) */
  double e_escaped[6]; int64_t n_escaped[6];
  /* ... of the escaped photons for which that rule finds no outflow face.  Expected 0; never dropped. */
  double e_escaped_unclassified; int64_t n_escaped_unclassified;
  /* ... of the photons that ended JB_ST_ABSORBED or JB_ST_OUTGOING_ABSORBED in a transport call of this
   * cycle, counted on the rank whose kernel absorbed them, before the hand-off turns packed slots into
   * absorbed-looking holes (jb_pack_outgoing) */
  double e_absorbed; int64_t n_absorbed;
  /* ... of the JB_ST_ACTIVE photons when the cycle closes */
  double e_census; int64_t n_census;
  /* sum of energy_tally x cell volume over the interior cells of the owned blocks: agrees with e_census */
  double e_tally;
  /* sum of energy_delta over the same cells, raw.  energy_delta is an energy per cell, not a density
   * (transport.cpp:159-161), and a reference quirk applies: the emission source OVERWRITES it with minus the
   * emitted energy (sourcing.cpp:165-166,196) and without emission nothing ever resets it (SURVEY App. C
   * quirk 5) -- with emission it is this cycle's absorbed minus emitted energy, without it the absorbed
   * energy of all cycles so far */
  double e_delta;
  /* sum of HOST_UPDATE_ENERGY x cell volume over the same cells, after UpdateFluid */
  double e_material;
  double t_start, dt;
  /* the cycle: *cycle of the step calls; jb_ledger_close called by a host returns 0 here and the host, which
   * knows its cycle, sets it */
  int64_t cycle;
} jb_energy_ledger;
enum { JB_LEDGER_SOURCED = 0, JB_LEDGER_TRANSPORTED = 1 };
/* on != 0: allocates the ledger's buffers (once: 64 + 32 x 8 x CUs words, and 27 words per possible rank for
 * jb_ledger_reduce) and zeroes the running sums.
 * JB_LEDGER=1 in the environment makes on the default of jb_initialize, like JB_EXACT_ARITH.  Ranks that
 * step together (jb_radiation_step_ranks) must all have it on or all off. */
jb_status jb_ledger_enable(jb_context *ctx, int on);
int jb_ledger_enabled(const jb_context *ctx);
/* The task form, for a host that drives the tasks itself; adds to the running sums of the cycle.
 *   JB_LEDGER_SOURCED: [first, last) = the slots jb_source_photons_fill has just filled (swarm->n updated).
 *   JB_LEDGER_TRANSPORTED: [first, last) = the range a transport call has just followed; before any pack or
 *     exchange, and with no slot in it that an earlier call in this cycle has counted.  The holes arrivals
 *     absorbed on another rank become are told apart and skipped BY BIT 63 OF THEIR id, which
 *     jb_unpack_incoming leaves there (see jb_swarm_view::id): a host that unpacks records with code of its
 *     own must set that bit in such a hole's id too, or the absorption is counted on both ranks.
 * Every escaped or absorbed photon is then counted exactly once, also when the swarm's holes are closed
 * between two transport iterations.  JB_ERR_INVALID while the ledger is disabled. */
jb_status jb_ledger_accumulate(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, int64_t first,
                               int64_t last, int what);
/* After UpdateFluid: sums the census ([0, swarm->n)) and the fields, reads the cycle's ledger back (the one
 * synchronisation), zeroes the running sums.  out may be NULL (jb_ledger_last has it). */
jb_status jb_ledger_close(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, double t_start,
                          double dt, jb_energy_ledger *out);
/* The ranks' ledgers through the transport's all_gather_u64 (doubles bit-cast), added in rank order: every
 * rank ends with the same bits.  replicated != 0 (every rank holds every block and the all-reduced fields):
 * swarm terms summed, field terms (e_tally, e_delta, e_material) taken once.  Collective.  nranks == 1:
 * nothing to do (transport may be NULL).  The gather buffer is taken by jb_ledger_enable, so that nothing can
 * fail on one rank alone before the collective.  Inside jb_radiation_step_ranks a rank whose close failed still
 * makes the all-gather, with its status in front of its ledger, and every rank returns that failure. */
jb_status jb_ledger_reduce(jb_context *ctx, const jb_exchange_transport *transport, int rank, int nranks,
                           int replicated, jb_energy_ledger *inout);
/* The ledger of the last completed jb_radiation_step / jb_radiation_step_ranks (reduced over the ranks:
 * one more all-gather on every rank, inside the call) or jb_ledger_close.  With the ledger enabled the step
 * calls do all of the above inside: the sourced sweep after the fill, a transported sweep after every transport
 * launch over exactly the range it followed, before jb_exchange, the close after UpdateFluid.
 * JB_ERR_INVALID while the ledger is disabled or before the first close. */
jb_status jb_ledger_last(const jb_context *ctx, jb_energy_ledger *out);

/* ---- exact deposition: energy_delta and the census tally as ONE rounding of the exact sum of their addends --
 * the same bits whatever the order of the photons, the launch geometry, the time of the last sort or the number
 * of ranks (jaybenne_amd/csrc/jb_kernel_deposit.hpp, jb_deposit_fixed.hpp).  The reference has
 * no such task.  JB_DEPOSIT_ATOMIC (the default): every tracking kernel adds an absorbed weight to energy_delta,
 * and the fused tally a census weight to energy_tally, with a floating-point atomic; the last bit of a cell then
 * depends on the order the adds arrive in, and with emission and feedback on it reaches the next cycle's
 * opacities, emission counts and weights.  JB_DEPOSIT_EXACT:
 *   - Per interior cell of every resident block the library keeps a 256-bit unsigned fixed-point accumulator
 *     (four 64-bit words).  An addend w (finite, > 0) is converted at the cycle's scale exponent E: its 53-bit
 *     significand is placed so that a weight of exponent E has its top bit at bit 222 -- 33 bits of headroom
 *     above (2^32 addends of the largest weight, or heavier arrivals), and every addend of exponent >= E - 170
 *     exact.  An addend with non-zero bits below is truncated, never rounded, and counted in n_truncated
 *     (a function of (w, E) alone: the result stays independent of the order); w <= 0 or not finite adds nothing
 *     and is counted in n_rejected, as is a slot whose block or cell indices lie outside a resident block.
 *   - The adds are integer adds with carry (returning atomics: every wrap of a word is seen by exactly one).
 *   - E is fixed for the cycle by the first accumulate call after a close: the largest exponent of w over slots
 *     [0, swarm->n).  A later accumulate call of the cycle whose range [first, last) holds a heavier weight --
 *     arrivals from a rank with hotter blocks can lie further above this rank's own weights than the headroom
 *     reaches -- RAISES E to that weight's exponent in front of its sweep: every accumulator moves down by the
 *     difference, and an accumulator that loses non-zero bits there is counted in n_truncated.  E is rank-local;
 *     while n_truncated == 0 the sum is exact and does not depend on E, which is the condition the cross-rank
 *     identity is stated under.
 *   - After its launch every transport entry point sweeps exactly the range it followed and adds w of every
 *     JB_ST_ABSORBED slot whose id has bit 63 clear to the cell (blk, kp, jp, ip) left in the slot; wherever
 *     arrivals are unpacked (jb_unpack_incoming, jb_exchange) the arrivals are swept for JB_ST_ABSORBED slots WITH
 *     bit 63.  Every deposit is counted once, by the rank that owns the cell.
 *   - The tracking kernels and the unpack kernel are the ones of JB_DEPOSIT_ATOMIC, unchanged: they are handed a
 *     mesh view whose energy_delta table points at a library-owned decoy field that nothing reads, so the real
 *     fields never see an atomic.  fuse_census_tally is ignored (the plan is made without the tally); the tally is
 *     the close's.
 *   - jb_deposit_close, in this order: a set top bit in any accumulator of the absorbed sums (overflow) is
 *     JB_ERR_INVALID before any field is written; energy_delta[q] = energy_delta[q] + D for every cell that received something, D the
 *     accumulator as a double with one round-to-nearest-even; the accumulators zeroed; a new scale over the ACTIVE
 *     slots; [0, swarm->n) swept for ACTIVE photons in owned blocks; energy_tally[q] = T / dv (dv = dx1 dx2 dx3 of
 *     the block, cells without census photons 0); the accumulators zeroed again.  Two synchronisations.  A set top
 *     bit after the census sweep is JB_ERR_INVALID too, before energy_tally is written but AFTER energy_delta has its
 *     deposits.  Either error zeroes the accumulators: the sums of the stage that overflowed are lost with it.
 *   - With accumulators open, jb_update_fluid and jb_ledger_close close them first (jb_update_fluid, which has no
 *     swarm argument, with the swarm of the last accumulate, its n as jb_remove_marked_particles last left it): a
 *     host that only flips the switch gets the right fields.  That view of the swarm is kept per mesh, with the
 *     pointers of the last accumulate: a host that reallocates its swarm arrays between the last transport or
 *     unpack call of a cycle and jb_update_fluid must call jb_deposit_close itself, with the new view.  jb_evaluate_radiation_energy computes the tally by
 *     the exact path.  Changing the mode with accumulators open is JB_ERR_INVALID.
 * Memory: 32 bytes of accumulator + 8 of decoy field per cell of the resident blocks, taken at the first use in
 * EXACT mode: 40 B per cell, about 0.7 GB on a mesh of 256^3 cells.  JB_DEPOSITION=exact in the environment makes
 * EXACT the default of jb_initialize, like JB_CELL_ORDER.  A replicated mesh sums its fields over the ranks in
 * floating point: exact deposition is not for it. */
enum { JB_DEPOSIT_ATOMIC = 0, JB_DEPOSIT_EXACT = 1 };
enum { JB_DEPOSIT_ABSORBED = 1, JB_DEPOSIT_ARRIVALS = 2 };
typedef struct jb_deposit_stats {
  int64_t n_absorbed_addends;  /* addends of the absorbed and arrivals sweeps of the cycle the last close ended */
  int64_t n_census_addends;    /* ... of its census sweep */
  int64_t n_truncated;         /* addends of either with non-zero bits below the accumulator's bit 0 */
  int64_t n_rejected;          /* slots of either that added nothing: w <= 0, not finite, or outside the mesh */
  int32_t scale_absorbed;      /* E of the energy_delta stage (the biased exponent field of a double: 1 .. 2046) */
  int32_t scale_census;        /* E of the tally stage */
} jb_deposit_stats;
jb_status jb_set_deposition(jb_context *ctx, int mode);
int jb_get_deposition(const jb_context *ctx);
/* The task form of the sweeps, for a host that unpacks with code of its own, and the tests: what = a sum of
 * JB_DEPOSIT_ABSORBED (slots of [first, last) that are JB_ST_ABSORBED with bit 63 of the id clear) and
 * JB_DEPOSIT_ARRIVALS (... with bit 63 set).  The contract of jb_ledger_accumulate: no slot twice, before any
 * pack.  JB_ERR_INVALID in ATOMIC mode. */
jb_status jb_deposit_accumulate(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, int64_t first,
                                int64_t last, int what);
jb_status jb_deposit_close(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm);
/* The counts of the last close (synchronises the context's stream).  JB_ERR_INVALID in ATOMIC mode or before the
 * first close. */
jb_status jb_deposit_last(jb_context *ctx, jb_deposit_stats *out);
/* What the mode has cost so far (diagnostics; no synchronisation): the device memory taken for this mesh's
 * accumulators, decoy field and second view -- 0 until the mesh's first call in EXACT mode --, and the number of
 * kernels of jb_kernel_deposit.hpp this context has launched -- it stands still in ATOMIC mode, and across a
 * jb_update_fluid or jb_ledger_close that finds nothing open. */
int64_t jb_deposit_memory(const jb_mesh *mesh);
int64_t jb_deposit_kernel_launches(const jb_context *ctx);

/* ---- source tilt -- where in its cell a new photon starts (jaybenne_amd/csrc/jb_kernel_tilt.hpp).  The reference
 * places every new photon uniformly in its cell (sourcing.cpp:175-177): a cell is isothermal, and in a cell that is
 * optically thick to absorption the energy absorbed at its hot face is re-emitted, on average, at its centre --
 * half a cell downstream every cycle.  Under JB_TILT_LINEAR the emission probability of SourcePhotons, thermal and
 * emission, varies linearly within a cell along every active axis, following the gradient of T^4 (Fleck and
 * Cummings' source tilt).  The boundary source, whose photons start on a face, is not tilted.  The contract:
 *   - Slopes.  jb_source_photons_count, behind its count kernel and only in this mode, computes for every interior
 *     cell of every owned resident block and every active axis d one slope s_d in [-1, 1]:
 *       E = (T T) (T T), T = the temperature of (rho, sie) exactly as the count forms it;
 *       E_c the cell's, E_m / E_p its lower / upper neighbour's along d -- read from the block's own ghost layer
 *       where the neighbour lies in another block (the host keeps those ghosts current, as for the DDMC face
 *       probabilities; across a level change this is what the host's ghost fill put there, at the block's own
 *       spacing).  A neighbour beyond a domain face whose swarm boundary is not periodic counts as E_c, and that
 *       ghost cell is not read;
 *       s_raw = (E_p - E_m) / (4 E_c);  s = min(max(s_raw, -1), 1);  s = 0 if E_c is zero or s_raw is not finite.
 *     Every operation is rounded on its own.  Inactive axes have s = 0.
 *   - Sampling.  With xi the draw the photon takes for that axis (draw order and count are those of JB_TILT_NONE,
 *     so everything drawn behind the positions keeps its bits):
 *       a = 1 - s;  D = sqrt(a a + (4 s) xi);  u = ((4 xi - 2) + s) / (1 + D);
 *       u = max(min(u, 1 - 2^-52), -1);  x = xc + (0.5 dx) u
 *     -- two products, one sum and one correctly rounded square root for D (a radicand that rounding took to 0 or
 *     below has D = 0), one correctly rounded quotient, no fused operation.  This inverts the density (1 + s u) / 2
 *     on [-1, 1] without cancellation for small s; for s = 0 it returns 2 xi - 1 exactly and x has the bits of
 *     xc + dx (xi - 0.5).  The position is a function of (s, xi, xc, dx) alone.
 *   - jb_source_photons_fill / _fill_range in this mode read the slopes of the mesh's last count call; without one
 *     in this mode they return JB_ERR_INVALID.  Ids and draws do not depend on the mode: a replicated mesh and
 *     several ranks source the photons of one rank.  jb_radiation_step and jb_radiation_step_ranks source through
 *     these calls and take the mode from the context.
 *   - The slopes live in a library-owned array of 8 ndim bytes per interior cell of the resident blocks, taken at
 *     the mesh's first count call in this mode and freed with the mesh.
 * With JB_TILT_NONE (the default) no kernel of jb_kernel_tilt.hpp is launched and every call gives the bits it
 * gave.  JB_SOURCE_TILT=linear in the environment makes LINEAR the default of jb_initialize, like JB_DEPOSITION. */
enum { JB_TILT_NONE = 0, JB_TILT_LINEAR = 1 };
jb_status jb_set_source_tilt(jb_context *ctx, int mode);
int jb_get_source_tilt(const jb_context *ctx);
/* The slopes of the mesh's last count call of resident block local_block, copied to out_host as [3][ncell]
 * doubles, cells in (k, j, i) order, zeros for inactive axes (synchronises the context's stream).
 * JB_ERR_INVALID if that call was not made under JB_TILT_LINEAR (or none was made), or for a halo copy. */
jb_status jb_source_tilt_slopes(jb_context *ctx, const jb_mesh *mesh, int local_block, double *out_host);

/* ---- source allocation -- how many of a source call's photons a cell gets (jaybenne_amd/csrc/jb_kernel_salloc.hpp).
 * The reference's `uniform` strategy gives every cell the same number whatever it sources (sourcing.cpp:68-69,
 * 99-103): a cold cell's photons carry almost no energy, yet each costs a full history.  Its `energy` strategy is
 * declared and rejected (sourcing.cpp:38), and <jaybenne> source_strategy = energy STAYS rejected by every call
 * here.  Under JB_ALLOC_ENERGY (an extension: <jaybenne_amd> source_allocation = energy) a cell's photon number is
 * proportional to the energy it sources, so the new photons carry nearly equal weights.  A source call, thermal or
 * emission, with N = params.num_particles -- the target for the WHOLE mesh and the whole call; blocks_in_call and
 * the npc of sourcing.cpp:68-69 play no part -- then does:
 *   1. Energy pass (jb_source_energy_sums).  For every interior cell of every owned resident block, erad with the
 *      very expressions and product order of the uniform count -- thermal ((4 sb / c) (T^2 T^2)) dv, emission
 *      ((fleck j) dv) dt -- stored in the src_ew field, which stages it between the two kernels so that both see
 *      the same bits.  Per block e_block[b]: thread t of 256 starts from +0.0 and adds cells t, t + 256, ... of the
 *      (k, j, i) order in rising order; then s[t] += s[t + d] for t < d, d = 128, 64, ... 1; e_block = s[0].  No
 *      floating-point atomics.  A halo copy gives 0.
 *   2. Total (jb_source_energy_total).  E_tot = the sum of e_block over the GLOBAL block ids in rising order,
 *      sequentially from +0.0: the same bits on every rank and for every partition.  scale = (double)N / E_tot,
 *      one division on the host.  A non-finite (or negative) E_tot, or a scale that is not finite, is
 *      JB_ERR_INVALID; E_tot == 0 sources nothing and completes (every count 0, every weight 0).
 *   3. Count pass (jb_source_photons_count_energy).  Per cell nu = erad scale; f = floor(nu);
 *      n = f + (double)((nu - f) > xi), xi the ONE draw of the cell's rounding stream -- the stream, epoch and
 *      draw of the uniform count; src_num = n; src_ew = erad / n when f >= 1 (the cell's energy is sourced
 *      exactly), erad / nu when f = 0 and n = 1 (unbiased roulette, about E_tot / N), 0 when n = 0.  Then the
 *      block's exclusive prefix and count as the uniform count forms them.  An N for which a block's count could
 *      pass 2^31 - 1 (N + cells per block) is JB_ERR_INVALID before any launch.
 *   4. energy_delta.  The emission source's fill sets energy_delta = -(n src_ew), one product, by a kernel of its
 *      own (the uniform path's serial loop over a cell's photons would run up to N times in one thread);
 *      set_energy_delta = 0 keeps its meaning.
 *   5. Fill.  jb_source_photons_fill / _fill_range are as they were: they read prefix, src_ew and the ids; the
 *      tilt's slopes are still written behind the count; the boundary source keeps its own N_b.
 * jb_source_photons_count in this mode runs 1-3 in a row when the mesh view is wholly resident and owned (one rank,
 * or a rank of a replicated mesh) -- the path jb_radiation_step takes; otherwise JB_ERR_INVALID, naming the calls
 * below, between which the host gathers every rank's block sums (each block has one owner: jaybenne_amd/jaybenne.py
 * sends them as bit patterns through an integer sum).  jb_radiation_step_ranks is outside this mode: under
 * JB_ALLOC_ENERGY it returns JB_ERR_UNSUPPORTED on every rank before its first collective (the mode is a property
 * of the call that all ranks share); examples/handoff_mpi and the Parthenon adapter do not set it.
 * With JB_ALLOC_UNIFORM (the default) no kernel of jb_kernel_salloc.hpp is launched and every call gives the bits it
 * gave.  JB_SOURCE_ALLOCATION=energy in the environment makes ENERGY the default of jb_initialize, like
 * JB_SOURCE_TILT. */
enum { JB_ALLOC_UNIFORM = 0, JB_ALLOC_ENERGY = 1 };
jb_status jb_set_source_allocation(jb_context *ctx, int mode);
int jb_get_source_allocation(const jb_context *ctx);
/* Step 1: e_block_host[b] for the mesh view's resident blocks b (0 for a halo copy; all 0 and no launch for the
 * emission source without do_emission).  Synchronises the context's stream.  JB_ERR_INVALID outside ENERGY mode. */
jb_status jb_source_energy_sums(jb_context *ctx, jb_mesh *mesh, int source_type, double dt, double *e_block_host);
/* Step 2: the sum of e_block_by_gid[0 .. nblocks_total) in rising order from +0.0 -- host code, so that every host
 * adds alike. */
double jb_source_energy_total(const double *e_block_by_gid, int nblocks_total);
/* Step 3, for the energies the mesh's last jb_source_energy_sums call of this source_type staged (JB_ERR_INVALID
 * without one since the mesh's last count); nper_block_host / prefix_dev as jb_source_photons_count. */
jb_status jb_source_photons_count_energy(jb_context *ctx, jb_mesh *mesh, int source_type, double dt, uint32_t epoch,
                                         double e_total, int32_t *nper_block_host, int32_t *prefix_dev);

/* ---- transport invariants (checked library) -- the reference's PARTHENON_DEBUG_REQUIREs of the
 * tracking loop and of SampleDDMCBlockFace, evaluated on every pass (jaybenne_amd/csrc/jb_invariants.hpp).
 * `make -C jaybenne_amd/csrc checked` builds libjaybenne_amd_checked.so from the same sources with
 * -DJB_INVARIANTS; a host selects it instead of libjaybenne_amd.so (Python: JAYBENNE_AMD_LIB).  The
 * release library exports the same symbols: jb_invariants_enabled() = 0 there and the other two return
 * JB_ERR_UNSUPPORTED.
 * Status policy of the checked library: tasks accumulate, steps report.  A task keeps its usual status
 * and only counts; jb_radiation_step returns JB_ERR_INVARIANT when the violation count rose during the
 * call, and jb_last_error() then quotes the reference's message for the first violation to claim the
 * record.  jb_exchange carries each rank's violations since its last exchange in its row of the call's
 * first all-gather: when any rank has one, EVERY rank returns JB_ERR_INVARIANT from that call, before the
 * payload exchange, and jb_radiation_step_ranks returns it too -- no rank is left in a collective.  The
 * counts are per process and device, shared by its contexts.  A violating photon is never used as an index
 * (k_ddmc_q, whose queues have no path that drops a photon, counts it and goes on): it leaves the tracking
 * loop untallied.
 * POSITION / INDEX at the top of every event pass and EVENT_OFF_BLOCK at the block exits of k_transport,
 * k_imc_cell, k_ddmc_all, k_ddmc_q and k_hybrid (cell-local kernels in their own coordinates); FACE_SAMPLE
 * in k_block_face; DDMC_CLASS; SWARM after SourcePhotons' fill, after an unpack of arrivals, on entry to
 * every transport task (indices not checked where arrivals may carry their sender's) and in
 * jb_verify_swarm. */
enum {
  JB_INV_POSITION = 0,        /* inside its block at the top of a tracking pass (transport.cpp:100-105) */
  JB_INV_INDEX = 1,           /* cell indices in the block's interior (transport.cpp:106-111) */
  JB_INV_EVENT_OFF_BLOCK = 2, /* no absorption / scattering on the step that leaves the block (:152) */
  JB_INV_FACE_SAMPLE = 3,     /* inside its block after block-face resampling (sample_ddmc_bface.cpp:229) */
  JB_INV_DDMC_CLASS = 4,      /* class record == the cell's own DDMC step record (after k_ddmc_pack) */
  JB_INV_SWARM = 5,           /* sweep over the live photons (jb_verify_swarm and the task entries) */
  JB_INV_NKINDS = 6
};
enum {  /* kernel families whose checks count lane-passes */
  JB_INV_FAM_TRANSPORT = 0,   /* k_transport (x-space tracking: IMC, DDMC, packed hybrid) */
  JB_INV_FAM_IMC_CELL = 1,    /* k_imc_cell */
  JB_INV_FAM_DDMC_ALL = 2,    /* k_ddmc_all */
  JB_INV_FAM_DDMC_Q = 3,      /* k_ddmc_q */
  JB_INV_FAM_HYBRID = 4,      /* k_hybrid */
  JB_INV_FAM_BLOCK_FACE = 5,  /* k_block_face */
  JB_INV_FAM_DDMC_CLASS = 6,  /* the DDMC_CLASS sweep (cells) */
  JB_INV_FAM_SWARM = 7,       /* the SWARM sweep (photon slots) */
  JB_INV_NFAMILIES = 8
};
typedef struct jb_invariant_report {
  int64_t evaluated[JB_INV_NKINDS];   /* checks made per kind (POSITION / INDEX: one per lane-pass) */
  int64_t violated[JB_INV_NKINDS];    /* ... and failed */
  int64_t passes[JB_INV_NFAMILIES];   /* lane-passes (photons or cells) checked per kernel family */
  /* the first violation since the last reset (valid when has_first) */
  int32_t has_first, first_kind, first_family, first_block;
  int64_t first_slot, first_id;       /* swarm slot (-1: a cell) and creation index (-1: unknown) */
  int32_t first_ip, first_jp, first_kp, first_axis;  /* first_axis: 0..2, the axis that failed */
  double first_x, first_y, first_z;
} jb_invariant_report;
int jb_invariants_enabled(void);
/* The counts since the last reset (synchronises the context's stream); reset != 0 zeroes them after. */
jb_status jb_invariant_report_get(jb_context *ctx, jb_invariant_report *report, int reset);
/* The SWARM sweep, now, over slots [0, swarm->n) of a swarm whose cycle is [t_start, t_end] (live
 * photons: t <= t_end).  *report (may be NULL) receives the counts of this sweep alone; they are added
 * to the running counts too.  JB_COMPLETE when the swarm is clean, JB_ERR_INVARIANT when it is not. */
jb_status jb_verify_swarm(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, double t_start,
                          double t_end, jb_invariant_report *report);

/* ---- trace ranges -- the reference's Kokkos::Profiling::pushRegion("Jaybenne::Timestep") ...
 * popRegion() and "Jaybenne::TransportLoop" (jaybenne.cpp:87,115,127,145).  Every task entry point
 * above opens a ROCTx range named after its reference task ("Jaybenne::TransportPhotons_DDMC", ...)
 * for its own duration and jb_radiation_step opens the reference's two; a host that drives the
 * tasks itself brackets its cycle and its iterate-sublist with these (jaybenne_amd/jaybenne.py,
 * include/jaybenne_amd.hpp do).  `rocprofv3 --marker-trace --kernel-trace` shows them beside the
 * kernels.  The marker library (librocprofiler-sdk-roctx / libroctx64) is dlopen()ed on first use:
 * no link dependency; absent, or with JB_NO_ROCTX=1, the calls do nothing and return -1
 * (jb_ranges_enabled() = 0).  push returns the nesting level as roctxRangePushA does. */
int jb_range_push(const char *name);
int jb_range_pop(void);
int jb_ranges_enabled(void);

/* ---- debug entry points (parity tests drive the device functions directly) ---------------- */
jb_status jb_debug_philox(jb_context *ctx, const uint32_t ctr[4], const uint32_t key[2],
                          uint32_t out[4]);
jb_status jb_debug_rocrand_philox(jb_context *ctx, uint64_t seed, uint64_t subsequence,
                                  uint32_t out[8]);
jb_status jb_debug_seed_state(jb_context *ctx, uint32_t seed, uint32_t domain, uint64_t id,
                              uint64_t *state);
/* first state of the random stream of the particle with creation index id (csrc/jb_rng.hpp) */
jb_status jb_debug_stream_start(jb_context *ctx, uint32_t seed, uint64_t id, uint64_t *state);
jb_status jb_debug_draw_stream(jb_context *ctx, uint64_t state, int n, double *out_host,
                               uint64_t *final_state);
/* which: 0 log, 1 sin, 2 cos, 3 acos, 4 sqrt, 5 reciprocal, 6 lean sqrt, 7 lean x[i] / x[i+1],
 * 8 lean x[i] / c, 9 sin(2 pi x), 10 cos(2 pi x), 11 1 - exp(-x), 12 x[i] / x[i+1] as the lean
 * arithmetic forms it (numerator times once-refined reciprocal), 13 lean log, 14 lean sqrt, 15 lean log
 * on its 1024-row table (the cell-local IMC kernel's), 16 / 17 sin / cos(2 pi x) with the grid point rounded by
 * adding the magic constant 2^44 + 2^43 to x (the scatter's form for generator uniforms; equal to 9 / 10 unless 256 x is
 * an integer plus one half) */
jb_status jb_debug_math(jb_context *ctx, int which, const double *x_host, int n, double *out_host);
/* the opacity / scattering models as the kernels evaluate them: out[0..3] = EPBremss A, B, E
 * (sigma_a = A rho^2 T^-1/2 (1 - e^(-B nu / T)) nu^-3, j = E rho^2 T^1/2, code units) and the
 * effective GrayS kappa_s; and one evaluation: which 0 absorption(rho, T, nu), 1 emissivity(rho,
 * T), 2 scattering(rho, T, nu) for n triples x_host[3 i .. 3 i + 2] */
jb_status jb_debug_model_coefficients(jb_context *ctx, double out[4]);
jb_status jb_debug_model_eval(jb_context *ctx, int which, const double *x_host, int n,
                              double *out_host);
/* step functions on a tape of uniforms.  st: jb_debug_step record (see below); which:
 * 0 ptcl_transport_step, 1 ptcl_ddmc_step, 2 ptcl_ddmc_albedo */
typedef struct jb_debug_step {
  double t_start, dt, ff, aa, ss, vv, dx_push;
  int32_t multi_d, three_d;
  double xl, yl, zl, xu, yu, zu, Px_l, Py_l, Pz_l, Px_u, Py_u, Pz_u;
  double t, x, y, z, vx, vy, vz;
  int32_t ip, jp, kp, is_absorbed, is_scattered, is_rejected;
} jb_debug_step;
jb_status jb_debug_step_call(jb_context *ctx, int which, jb_debug_step *st, const double *tape,
                             int ntape, int *ndraws);
/* which: 0 scatter(vv), 1 sample_face_iso_dir(vv), 2 sample_Planck_energy(sb=a0, temp=a1),
 * 3 SampleFace2D(i_l=i0, dx=a0, P_l=a1, P_u=a2; i=i1, x=a3),
 * 4 SampleFace3D(i1_l=i0, i2_l=i1, dx1=a0, dx2=a1, P=a2..a5; i=(i2,i3), x=(a6,a7)),
 * 5 scatter_dir (the unit direction the lean tracking kernels scatter into; on a tape the azimuth keeps the
 *   conversion form of jb_debug_math 9 / 10) */
jb_status jb_debug_sample_call(jb_context *ctx, int which, const double *a, const int32_t *i,
                               const double *tape, int ntape, double out[4], int32_t iout[2],
                               int *ndraws);

#ifdef __cplusplus
}
#endif
#endif /* JAYBENNE_AMD_H_ */
