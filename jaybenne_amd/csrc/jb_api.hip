// jb_api.hip -- host side of the C ABI declared in include/jaybenne_amd.h.
//
// Mirrors the task functions of the reference package (src/jaybenne/jaybenne.hpp:48-78) over
// raw device pointers.  No torch types, no exceptions across the boundary.
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_kernel.h>

#include <dlfcn.h>

#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/jaybenne_amd.h"
#include "../../include/jaybenne_amd.hpp"   // PlanSource: the stream-id arithmetic every host shares
#include "jb_kernels.hpp"
#include "jb_kernel_hybrid.hpp"
#include "jb_kernel_ddmc_q.hpp"
#include "jb_kernel_imc.hpp"
#include "jb_kernel_ledger.hpp"
#include "jb_kernel_comb.hpp"
#include "jb_kernel_gcomb.hpp"
#include "jb_kernel_order.hpp"
#include "jb_kernel_bsource.hpp"
#include "jb_kernel_deposit.hpp"
#include "jb_kernel_tilt.hpp"
#include "jb_kernel_salloc.hpp"
#include "jb_kernel_moments.hpp"
#include "jb_kernel_spectrum.hpp"
#include "jb_select.hpp"

using namespace jb;

// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static jb_status fail(jb_status st, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return st;
}

#define JB_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(JB_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                                 \
  } while (0)

// A device buffer of the context's own that only grows; growing it does not keep its contents.
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
};
static hipError_t dev_free(DevBuf &b) {
  const hipError_t e = b.p ? hipFree(b.p) : hipSuccess;
  b = DevBuf{};
  return e;
}
// what: the message's subject ("<what> failed"); a failure leaves the buffer empty and no sticky error behind
static jb_status dev_grow(DevBuf &b, size_t bytes, const char *what) {
  if (bytes <= b.bytes) return JB_COMPLETE;
  (void)dev_free(b);
  if (hipMalloc(&b.p, bytes) != hipSuccess) {
    b = DevBuf{};
    (void)hipGetLastError();
    return fail(JB_ERR_HIP, "%s failed", what);
  }
  b.bytes = bytes;
  return JB_COMPLETE;
}

struct jb_context {
  int device = 0;
  hipStream_t stream = nullptr;
  jb_params params{};
  jb_eos eos{};
  jb_opacity opac{};
  jb_scattering scat{};
  DevParams dp{};
  int num_cu = 256;
  unsigned long long *counters_d = nullptr;   // CNT_N + 2 cursors + per-rank counters
  unsigned long long *counters_h = nullptr;   // pinned
  DevBuf xch;                                 // jb_exchange: the gathered count matrix + pack offsets (u64)
  long long *scratch_d = nullptr;             // holes / movers / small tables
  bool scratch_alloc_failed = false;          // set by ensure_scratch when hipMalloc itself said no
  std::vector<unsigned long long> xch_matrix;  // jb_exchange: the rank x rank record counts (host copy)
  std::vector<long long> xch_tab;             // ... this rank's send / receive counts and offsets
  unsigned long long xch_room[4] = {0, 0, 0, 0}; // ... and its room: send buffer, receive buffer, free swarm slots (records)
                                              // | (checked build) this rank's invariant violations since its last exchange
  long long inv_reported = 0;                 // (checked build) the violation count the last jb_exchange reported
  size_t scratch_words = 0;
  unsigned long long scratch_gen = 0;         // counts the (re)allocations and releases of scratch_d
  // jb_comb_census_plan -> jb_comb_census_apply: the plan lies in scratch_d
  struct {
    bool valid = false;
    const jb_mesh *mesh = nullptr;
    const double *x = nullptr;                // the swarm it was made for
    long long n = 0, n_after = 0, n_new = 0;
    unsigned T = 0, K = 0;
    int ends_shift = 0;                       // the cells' ends are the histogram array from this entry on
    unsigned long long gen = 0;
    // a plan of the global comb (jb_comb_census_plan_global): apply runs k_gcomb_pack with the weigh's n_room
    bool global = false;
    long long n_room = 0;
  } comb;
  // jb_comb_census_weigh -> jb_comb_census_plan_global: order, ends and running weights lie in scratch_d
  struct {
    bool valid = false;
    const jb_mesh *mesh = nullptr;
    const double *x = nullptr;
    long long n = 0, n_room = 0;
    int ends_shift = 0;
    int64_t sorted = 0;
    double e_before = 0.0;
    unsigned long long gen = 0;
  } weigh;
  long long gcomb_launches = 0;               // kernels of jb_kernel_gcomb.hpp launched so far (jb_gcomb_kernel_launches)
  DevBuf gcomb_eblock;                        // jb_comb_census_weigh: the block sums (one double per resident block)
  // jb_radiation_step_ranks: the hand-off record buffers (JB_RECORD_WORDS words per record) and the buffer of
  // the step's first all-gather ([status | counts per global block] of this rank, then every rank's)
  DevBuf step_send, step_recv, step_gather;
  long long min_records = 0;  // JB_HANDOFF_MIN_RECORDS at jb_initialize: first size of those record buffers (tests)
  // jb_evaluate_radiation_moments_host: the device array the fields pass through
  DevBuf moments;
  // jb_evaluate_radiation_spectrum_host: the device array the bins pass through
  DevBuf spectrum;
  // arithmetic of the gray IMC tracking step: lean (default) or exact (JB_EXACT_ARITH=1 in the
  // environment at jb_initialize, or jb_set_arithmetic)
  bool lean_arith = true;
  // order of the photons within a cell behind a sort (JB_CELL_ORDER=id at jb_initialize, or jb_set_cell_order)
  int cell_order = JB_CELL_ORDER_ANY;
  int blocks_per_cu_env = 0;  // JB_TRANSPORT_BLOCKS_PER_CU at jb_initialize (tuning aid), 0 = occupancy query
  int max_blocks_env = 0;     // JB_TRANSPORT_MAX_BLOCKS at jb_initialize (tests: many photons per lane), <= 0 = no cap
  int grid_max = 0;           // largest grid launch_persistent used since transport_impl last cleared it
  bool no_ddmc_all = false;   // JB_NO_DDMC_ALL=1 at jb_initialize (tests: k_hybrid on all-DDMC meshes)
  int ddmc_lds_codes = 1;          // JB_DDMC_LDS_CODES=0: k_ddmc_q gathers the cell codes from device memory on any mesh (tests, A/B)
  int ddmc_queues = 1;             // JB_DDMC_QUEUES=0: k_ddmc_all instead of k_ddmc_q where both apply (tests, A/B)
  int max_classes = kMaxClasses;   // JB_DDMC_MAX_CLASSES: fewer (tests of the fall-back to the 64-byte gather)
  int coop_gather = -1;       // JB_COOP_GATHER=0 / 1 / 2: k_ddmc_all's quad-cooperative gather off / on / on with 64-bit addresses, whatever the table size
  bool no_imc_cell = false;   // JB_NO_IMC_CELL=1 at jb_initialize (tests, A/B): the lean step in x-space (k_transport<.., LEAN>) instead of k_imc_cell
  // jb_defrag_policy: HIP events around every transport call of the running cycle, and what the
  // policy remembers from cycle to cycle
  std::vector<hipEvent_t> tev;       // pairs (start, stop)
  int tev_used = 0;                  // events of tev recorded since the last policy call
  bool tev_overflow = false;
  double rate_ref = 0.0;             // lowest ms per event seen since the last sort (0: none yet)
  double rate_before_sort = 0.0;     // ... the rate of the cycle that triggered the last sort
  double excess_ms = 0.0;            // time spent above rate_ref since the last sort
  double last_rate = 0.0;            // ms per event of the cycle the policy looked at last
  double sort_ms_per_photon = 1.5e-7;  // cost of a sort: 15 ms per 1e8 photons until one has been timed
  hipEvent_t sort_ev[2] = {nullptr, nullptr};
  bool sort_timed = false;           // sort_ev brackets a sort whose time has not been read yet
  long long sort_n = 0;
  int cycles_since_sort = 0;
  int min_interval = 2;              // cycles between two sorts (doubles when a sort bought nothing)
  int policy_sorts = 0;
  bool sort_scratch_tried = false;   // the sort's scratch records have been asked for (first policy call)
  // energy ledger (jb_ledger_*; JB_LEDGER=1 at jb_initialize): off by default
  bool ledger_on = false;
  unsigned long long *ledger_d = nullptr;    // [kLedgerHead words: the running ledger | the workgroups' partial sums]
  int ledger_parts = 0;                      // workgroups the partials have room for
  DevBuf ledger_gather;                      // jb_ledger_reduce: this rank's ledger, then every rank's (u64)
  jb_energy_ledger ledger_last{};
  bool ledger_has_last = false;
  // boundary source (jb_set_boundary_source; jb_kernel_bsource.hpp): off (every temperature 0) by default
  double bs_temp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  long long bs_num_particles = 0, bs_face_cells_total = 0;   // what the step calls ask for (jb_set_boundary_source_count)
  DevBuf bs_prefix;                    // the step calls' prefix workspace (a host that drives the tasks brings its own)
  DevBuf bs_out;                       // [nblocks] counts, [nblocks][6] photons and energy of the last count call
  jb_boundary_source_record bs_last{};
  // exact deposition (jb_set_deposition; JB_DEPOSITION=exact at jb_initialize; jb_kernel_deposit.hpp): off by default
  int deposition = JB_DEPOSIT_ATOMIC;
  std::vector<jb_mesh *> dep_open_meshes;   // meshes of this context whose accumulators are open (a scale taken, no close yet)
  long long dep_launches = 0;          // kernels of jb_kernel_deposit.hpp launched so far (jb_deposit_kernel_launches)
  jb_deposit_stats dep_last{};
  bool dep_has_last = false;
  // source tilt (jb_set_source_tilt; JB_SOURCE_TILT=linear at jb_initialize; jb_kernel_tilt.hpp): off by default
  int source_tilt = JB_TILT_NONE;
  // source allocation (jb_set_source_allocation; JB_SOURCE_ALLOCATION=energy at jb_initialize; jb_kernel_salloc.hpp):
  // uniform by default
  int source_allocation = JB_ALLOC_UNIFORM;
};
constexpr int kLedgerHead = 64;   // words in front of the partial sums (LW_N of them used)
constexpr int kLedgerWords = (int)(sizeof(jb_energy_ledger) / 8);
constexpr int kLedgerGatherRow = kLedgerWords + 1;   // jb_ledger_reduce: [status | ledger] per rank
static_assert(sizeof(jb_energy_ledger) == 26 * 8 && offsetof(jb_energy_ledger, e_material) == 8 * LW_E_MATERIAL &&
              offsetof(jb_energy_ledger, n_escaped) == 8 * LW_N_ESCAPED && offsetof(jb_energy_ledger, e_census) == 8 * LW_E_CENSUS,
              "the running ledger on the device is the head of jb_energy_ledger, word for word");
constexpr int kTransportEventPairs = 64;
constexpr int kRankEnd = 1024;                               // CNT_N.. | 16..17 cursors | 32..1023 per-rank counts
constexpr int kCounterWords = kRankEnd + kQueues * kQueueStride;  // | 1024.. the queue heads, one line each (CNT_QUEUE)
static_assert(CNT_QUEUE == kRankEnd, "the queue heads follow the per-rank counts");
constexpr int kCursorBase = 16;
constexpr int kRankBase = 32;

struct jb_mesh {
  jb_context *ctx = nullptr;
  DevMesh dm{};
  std::vector<void *> owned;  // device allocations
  int nranks_seen = 1;
  // every resident block: power-of-two cell widths, lower corner a whole number of them (the
  // cell-face arithmetic is then exact; k_transport<..., EXACT>)
  bool exact_geom = false;
  // the mean-free-path arrays of all resident blocks lie within 4 GiB (32-bit byte offsets): what
  // the cell-local IMC kernel needs of a mesh, whatever its cell widths
  bool offsets32 = false;
  // the cell-local kernels (k_imc_cell, k_hybrid MODE 3) step the photon's byte offset with 24-bit
  // multiply-adds of the BYTE strides 8 ni and 8 ni nj: both have to stay below 2^23
  bool cell_ok = false;
  char last_variant[64] = "";  // variant_name of the last transport call's plan (jb_last_transport_variant)
  int last_grid = 0;           // ... and the largest grid of its persistent launches (jb_last_transport_grid)
  const DevMesh *dm_dev = nullptr;  // copy of dm in device memory (k_hybrid reads the view through it)
  const int *nbr_dq = nullptr;      // k_imc_cell: change of the cell's byte offset per (block, face) crossing
  bool uniform_geom = false;        // every resident block has the cell widths of block 0 (k_imc_cell<.., UNIFORM>)
  bool equal_h = false;             // the active cell widths of block 0 are equal (k_imc_cell<.., UNITCELL, EQUALH>)
  int last_unit_cell = 0;           // the last transport call's plan: 0 no unit-cell form, 1 UNITCELL, 2 with EQUALH
  // "some cell takes IMC steps" (DevMesh::not_all_ddmc) as the host last read it: -1 = not since
  // UpdateDerivedTransportFields rewrote it (the first DDMC transport call of a cycle reads it back,
  // one synchronisation; the further transport iterations of a multi-rank cycle reuse the answer)
  int not_all_ddmc_host = -1;
  int nclass_host = 0;   // ... and the number of distinct step records (DevMesh::ddmc_code), read with it
  // host copies of the view for jb_radiation_step_ranks: global id of each resident block, blocks owned
  // here, and whether every block of the view has the same owner (a single-rank or replicated view)
  std::vector<int32_t> gid_host;
  int nowned = 0;
  bool one_owner = true;
  // [nblocks][6]: 1 = face f of this owned block lies on the domain boundary (the boundary source's face cells)
  std::vector<uint8_t> bface_host;
  // exact deposition, taken at the first use in that mode (deposit_ensure): the accumulators ([nblocks * ncell][4]
  // words), their control words, and the view the tracking kernels get -- dm with the energy_delta table pointing
  // at a decoy field nothing reads -- by value and in device memory
  unsigned long long *dep_acc = nullptr, *dep_ctl = nullptr;
  DevMesh dm_x{};
  const DevMesh *dm_x_dev = nullptr;
  bool dep_ready = false, dep_open = false;
  size_t dep_bytes = 0;                // device memory taken for the above (jb_deposit_memory)
  jb_swarm_view dep_swarm{};           // the swarm of this mesh's last accumulate: what jb_update_fluid closes with
  // source tilt: the slopes of the last count call ([nblocks][ndim][ncell], taken at the first count call in the
  // mode; among `owned`, so freed with the mesh), whether that call wrote them, and a host copy of the owned flags
  double *tilt_d = nullptr;
  bool tilt_valid = false;
  std::vector<uint8_t> owned_host;
  // source allocation: the mesh's last count call was made under JB_ALLOC_ENERGY (the fill then sets energy_delta
  // by k_salloc_edelta), and the last jb_source_energy_sums call's source type (-1: none since the last count)
  bool salloc_last = false;
  int salloc_sums_type = -1;
};
// open / closed: the context knows the meshes whose accumulators are open (jb_set_deposition turns a change of mode
// down while there is one, jb_remove_marked_particles keeps their swarm's n, jb_finalize lets go of them)
static void deposit_mark_open(jb_context *ctx, jb_mesh *m) {
  if (m->dep_open) return;
  m->dep_open = true;
  ctx->dep_open_meshes.push_back(m);
}
static void deposit_mark_closed(jb_context *ctx, jb_mesh *m) {
  if (!m->dep_open) return;
  m->dep_open = false;
  for (size_t q = 0; q < ctx->dep_open_meshes.size(); ++q)
    if (ctx->dep_open_meshes[q] == m) {
      ctx->dep_open_meshes.erase(ctx->dep_open_meshes.begin() + (long)q);
      break;
    }
}
// the mesh view a tracking kernel (or k_unpack_incoming) is launched with
static const DevMesh &track_dm(const jb_mesh *m) {
  return m->ctx->deposition == JB_DEPOSIT_EXACT && m->dep_ready ? m->dm_x : m->dm;
}
static const DevMesh *track_dm_dev(const jb_mesh *m) {
  return m->ctx->deposition == JB_DEPOSIT_EXACT && m->dep_ready ? m->dm_x_dev : m->dm_dev;
}
static jb_status deposit_ensure(jb_context *ctx, jb_mesh *mesh);
static jb_status deposit_sweep(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, long long first,
                               long long last, int what);
static jb_status deposit_close(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm);

__global__ void k_rcp_refined(double b, double *out) { *out = m_rcp_refined(b); }

// ------------------------------------------------------------------------------------------------
// Trace ranges.  The reference brackets the cycle and its transport loop with
// Kokkos::Profiling::pushRegion("Jaybenne::Timestep" / "Jaybenne::TransportLoop") (jaybenne.cpp:87,115,
// 127,145), which Kokkos Tools hand to whatever profiler is attached.  Here every task entry point of
// the C ABI opens a ROCTx range of its reference name ("Jaybenne::<task>"), jb_radiation_step opens the
// reference's two, and a host that drives the tasks itself opens them through jb_range_push / _pop;
// `rocprofv3 --marker-trace` shows them beside the kernels.  The marker library is dlopen()ed on first
// use -- no link dependency -- and everything is a no-op when it is absent or JB_NO_ROCTX=1.
struct RoctxApi {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
};
static const RoctxApi &roctx_api() {
  static const RoctxApi api = [] {
    RoctxApi a;
    const char *off = getenv("JB_NO_ROCTX");
    if (off && off[0] == '1') return a;
    // (rocprofv3 listens to the SDK's marker library; the roctracer one is what older tools attach to)
    for (const char *name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      void *lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (!lib) continue;
      a.push = (int (*)(const char *))dlsym(lib, "roctxRangePushA");
      a.pop = (int (*)())dlsym(lib, "roctxRangePop");
      if (a.push && a.pop) break;
      a = RoctxApi();
    }
    return a;
  }();
  return api;
}
struct TraceRange {
  bool open;
  explicit TraceRange(const char *name) : open(roctx_api().push != nullptr) { if (open) (void)roctx_api().push(name); }
  ~TraceRange() { if (open) (void)roctx_api().pop(); }
  TraceRange(const TraceRange &) = delete;
  TraceRange &operator=(const TraceRange &) = delete;
};
#define JB_RANGE(name) TraceRange jb_trace_range_(name)

extern "C" int jb_range_push(const char *name) {
  if (!name || !roctx_api().push) return -1;
  return roctx_api().push(name);
}
extern "C" int jb_range_pop(void) { return roctx_api().pop ? roctx_api().pop() : -1; }
extern "C" int jb_ranges_enabled(void) { return roctx_api().push != nullptr ? 1 : 0; }

extern "C" const char *jb_last_error(void) { return g_err; }
extern "C" const char *jb_version(void) { return "jaybenne_amd 0.1 (gfx950)"; }

static int grid_for(const jb_context *ctx, long long n, int per_cu = 8) {
  long long blocks = (n + kBlock - 1) / kBlock;
  const long long cap = (long long)ctx->num_cu * per_cu;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// ------------------------------------------------------------------------------------------------
// Transport invariants (jb_invariants.hpp).  The checked library (-DJB_INVARIANTS, `make checked`) counts
// into one buffer per process and device, allocated by the first jb_initialize on that device; the
// release library has none of this and answers the three entry points below with "not built".
#ifdef JB_INVARIANTS
constexpr int kInvDevices = 64;
static unsigned long long *g_inv_d[kInvDevices] = {};

static jb_status inv_setup(int device) {
  if (device < 0 || device >= kInvDevices) return fail(JB_ERR_UNSUPPORTED, "checked library: device %d", device);
  if (g_inv_d[device]) return JB_COMPLETE;
  unsigned long long *p = nullptr;
  JB_HIP(hipMalloc(&p, inv::kBufferWords * sizeof(unsigned long long)));
  JB_HIP(hipMemset(p, 0, inv::kBufferWords * sizeof(unsigned long long)));
  JB_HIP(hipMemcpyToSymbol(HIP_SYMBOL(inv::jb_inv_buf), &p, sizeof p));
  g_inv_d[device] = p;
  return JB_COMPLETE;
}

// the counts as a report (stripes summed; POSITION / INDEX are evaluated once per lane-pass of a tracking
// family, so their evaluated counts are those families' pass counts)
static jb_status inv_read(jb_context *ctx, jb_invariant_report *r) {
  std::vector<unsigned long long> h(inv::kBufferWords);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  JB_HIP(hipMemcpy(h.data(), g_inv_d[ctx->device], h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  memset(r, 0, sizeof *r);
  auto sum = [&](int base, int index) {
    unsigned long long s = 0;
    for (int q = 0; q < inv::kStripes; ++q) s += h[base + index * inv::kCountWords + q * inv::kStripeWords];
    return (int64_t)s;
  };
  for (int k = 0; k < JB_INV_NKINDS; ++k) {
    r->evaluated[k] = sum(inv::kEvalBase, k);
    r->violated[k] = sum(inv::kViolBase, k);
  }
  for (int f = 0; f < JB_INV_NFAMILIES; ++f) r->passes[f] = sum(inv::kPassBase, f);
  for (int f = JB_INV_FAM_TRANSPORT; f <= JB_INV_FAM_HYBRID; ++f) {
    r->evaluated[JB_INV_POSITION] += r->passes[f];
    r->evaluated[JB_INV_INDEX] += r->passes[f];
  }
  const unsigned long long *rec = h.data() + inv::kRecord;
  r->has_first = h[inv::kClaim] != 0ull;
  if (r->has_first) {
    r->first_kind = (int32_t)rec[inv::R_KIND];
    r->first_family = (int32_t)rec[inv::R_FAMILY];
    r->first_block = (int32_t)(long long)rec[inv::R_BLOCK];
    r->first_slot = (int64_t)rec[inv::R_SLOT];
    r->first_id = (int64_t)rec[inv::R_ID];
    r->first_ip = (int32_t)(long long)rec[inv::R_IP];
    r->first_jp = (int32_t)(long long)rec[inv::R_JP];
    r->first_kp = (int32_t)(long long)rec[inv::R_KP];
    memcpy(&r->first_x, &rec[inv::R_X], sizeof(double));
    memcpy(&r->first_y, &rec[inv::R_Y], sizeof(double));
    memcpy(&r->first_z, &rec[inv::R_Z], sizeof(double));
    r->first_axis = (int32_t)rec[inv::R_AXIS];
  }
  return JB_COMPLETE;
}

static int64_t inv_total(const jb_invariant_report &r) {
  int64_t v = 0;
  for (int k = 0; k < JB_INV_NKINDS; ++k) v += r.violated[k];
  return v;
}

static jb_status inv_violations(jb_context *ctx, int64_t *out) {
  jb_invariant_report r;
  const jb_status st = inv_read(ctx, &r);
  *out = st == JB_COMPLETE ? inv_total(r) : 0;
  return st;
}

// JB_ERR_INVARIANT with the reference's message for the first violation
static jb_status inv_fail(jb_context *ctx, int64_t n_new, const char *who) {
  jb_invariant_report r;
  if (inv_read(ctx, &r) != JB_COMPLETE || !r.has_first)
    return fail(JB_ERR_INVARIANT, "%s: %lld transport invariant violation(s)", who, (long long)n_new);
  static const char *const kPosition[3] = {"Particle initially outside block X1 domain!",
                                           "Particle initially outside block X2 domain!",
                                           "Particle initially outside block x3 domain!"};
  static const char *const kIndex[3] = {"Particle initially outside X1 logical bnds!",
                                        "Particle initially outside X2 logical bnds!",
                                        "Particle initially outside X3 logical bnds!"};
  const int axis = r.first_axis >= 0 && r.first_axis < 3 ? r.first_axis : 0;
  const char *msg = "transport invariant violated";
  switch (r.first_kind) {
  case JB_INV_POSITION: msg = kPosition[axis]; break;
  case JB_INV_INDEX: msg = kIndex[axis]; break;
  case JB_INV_EVENT_OFF_BLOCK: msg = "Absorption/scattering event off block!"; break;
  case JB_INV_FACE_SAMPLE: msg = "Particle sampled outside of meshblock!"; break;
  case JB_INV_DDMC_CLASS: msg = "DDMC class record differs from the cell's own step record"; break;
  case JB_INV_SWARM: msg = "swarm invariant violated (block, indices, position, status, w, e or t)"; break;
  }
  return fail(JB_ERR_INVARIANT, "%s: %s (%lld violation(s); first: family %d, block %d, slot %lld, id %lld, "
              "ijk %d %d %d, x %.17g %.17g %.17g)", who, msg, (long long)n_new, r.first_family, r.first_block,
              (long long)r.first_slot, (long long)r.first_id, r.first_ip, r.first_jp, r.first_kp, r.first_x,
              r.first_y, r.first_z);
}

// the SWARM sweep over slots [first, last), on the context's stream
static jb_status inv_sweep(jb_context *ctx, const DevMesh &M, const DevSwarm &S, long long first, long long last,
                           double t_end, bool check_index) {
  if (last <= first) return JB_COMPLETE;
  hipLaunchKernelGGL(k_inv_swarm, dim3(grid_for(ctx, last - first)), dim3(kBlock), 0, ctx->stream, M, S, first,
                     last, t_end, check_index ? 1 : 0);
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}
#endif

extern "C" int jb_invariants_enabled(void) {
#ifdef JB_INVARIANTS
  return 1;
#else
  return 0;
#endif
}

extern "C" jb_status jb_invariant_report_get(jb_context *ctx, jb_invariant_report *report, int reset) {
#ifdef JB_INVARIANTS
  if (!ctx || !report) return fail(JB_ERR_INVALID, "jb_invariant_report_get: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  const jb_status st = inv_read(ctx, report);
  if (st != JB_COMPLETE) return st;
  if (reset) {   // (on the context's stream: the check kernels run there)
    JB_HIP(hipMemsetAsync(g_inv_d[ctx->device], 0, inv::kBufferWords * sizeof(unsigned long long), ctx->stream));
    JB_HIP(hipStreamSynchronize(ctx->stream));
    ctx->inv_reported = 0;
  }
  return JB_COMPLETE;
#else
  (void)ctx; (void)report; (void)reset;
  return fail(JB_ERR_UNSUPPORTED, "jb_invariant_report_get: this is the release library; the transport invariants "
              "are checked by libjaybenne_amd_checked.so (make -C jaybenne_amd/csrc checked)");
#endif
}

// (slack: small tables grow with the run and are re-requested often; the sort's particle records --
// 128 bytes per photon -- are sized exactly: 25 % on top of 12.8 GB is memory a run near the card's
// capacity may not have)
static jb_status ensure_scratch(jb_context *ctx, size_t words, bool slack = true) {
  if (words <= ctx->scratch_words) return JB_COMPLETE;
  if (ctx->scratch_d) JB_HIP(hipFree(ctx->scratch_d));
  ctx->scratch_d = nullptr;
  ctx->scratch_words = 0;
  ++ctx->scratch_gen;
  const size_t want = slack ? words + words / 4 + 1024 : words + 16;
  const hipError_t e = hipMalloc(&ctx->scratch_d, want * sizeof(long long));
  if (e != hipSuccess) {   // (told apart from every other failure: DefragParticles may go without its scratch)
    ctx->scratch_d = nullptr;
    ctx->scratch_alloc_failed = true;
    (void)hipGetLastError();
    return fail(JB_ERR_HIP, "hipMalloc of %zu bytes of scratch memory failed: %s", want * sizeof(long long),
                hipGetErrorString(e));
  }
  ctx->scratch_words = want;
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
extern "C" jb_status jb_initialize(const jb_params *params, const jb_eos *eos,
                                   const jb_opacity *opacity, const jb_scattering *scattering,
                                   int device, jb_context **out) {
  if (!params || !eos || !opacity || !scattering || !out)
    return fail(JB_ERR_INVALID, "jb_initialize: null argument");
  // PARTHENON_REQUIRE / PARTHENON_FAIL conditions of jaybenne.cpp:167-171,205-216
  if (!(params->min_swarm_occupancy >= 0.0 && params->min_swarm_occupancy < 1.0))
    return fail(JB_ERR_INVALID,
                "Minimum allowable swarm occupancy must be >= 0 and less than 1");
  if (params->source_strategy != JB_STRATEGY_UNIFORM && params->source_strategy != JB_STRATEGY_ENERGY)
    return fail(JB_ERR_INVALID, "Only uniform or energy source strategies supported!");
  if (params->num_particles < 0) return fail(JB_ERR_INVALID, "num_particles must be >= 0");
  if (eos->model != JB_EOS_IDEAL_GAS)
    return fail(JB_ERR_UNSUPPORTED, "only the IdealGas EOS is built");
  if (opacity->model != JB_OPAC_GRAY && opacity->model != JB_OPAC_EPBREMSS)
    return fail(JB_ERR_UNSUPPORTED, "unknown absorption opacity model (Gray, EPBremss)");
  if (scattering->model != JB_SCAT_GRAY && scattering->model != JB_SCAT_THOMSON)
    return fail(JB_ERR_UNSUPPORTED, "unknown scattering model (GrayS, ThomsonS)");
  if (opacity->model == JB_OPAC_EPBREMSS &&
      !(opacity->time_scale > 0.0 && opacity->mass_scale > 0.0 && opacity->length_scale > 0.0 &&
        opacity->temperature_scale > 0.0))
    return fail(JB_ERR_INVALID, "EPBremss needs positive time / mass / length / temperature scales");
  if (scattering->model == JB_SCAT_THOMSON && !(scattering->length_scale > 0.0))
    return fail(JB_ERR_INVALID, "ThomsonS needs a positive length scale");
  JB_HIP(hipSetDevice(device));
  jb_context *ctx = new (std::nothrow) jb_context();
  if (!ctx) return fail(JB_ERR_HIP, "out of host memory");
  ctx->device = device;
  ctx->params = *params;
  ctx->eos = *eos;
  ctx->opac = *opacity;
  ctx->scat = *scattering;
  {
    const char *ex = getenv("JB_EXACT_ARITH");
    ctx->lean_arith = !(ex && ex[0] == '1');
  }
  if (const char *e = getenv("JB_CELL_ORDER")) ctx->cell_order = strcmp(e, "id") == 0 ? JB_CELL_ORDER_BY_ID : JB_CELL_ORDER_ANY;
  if (const char *e = getenv("JB_DEPOSITION")) ctx->deposition = strcmp(e, "exact") == 0 ? JB_DEPOSIT_EXACT : JB_DEPOSIT_ATOMIC;
  if (const char *e = getenv("JB_SOURCE_TILT")) ctx->source_tilt = strcmp(e, "linear") == 0 ? JB_TILT_LINEAR : JB_TILT_NONE;
  if (const char *e = getenv("JB_SOURCE_ALLOCATION"))
    ctx->source_allocation = strcmp(e, "energy") == 0 ? JB_ALLOC_ENERGY : JB_ALLOC_UNIFORM;
  if (const char *e = getenv("JB_TRANSPORT_BLOCKS_PER_CU")) ctx->blocks_per_cu_env = atoi(e);
  if (const char *e = getenv("JB_TRANSPORT_MAX_BLOCKS")) ctx->max_blocks_env = atoi(e);
  if (const char *e = getenv("JB_NO_DDMC_ALL")) ctx->no_ddmc_all = e[0] == '1';
  if (const char *e = getenv("JB_NO_IMC_CELL")) ctx->no_imc_cell = e[0] == '1';
  if (const char *e = getenv("JB_COOP_GATHER")) ctx->coop_gather = e[0] == '1' ? 1 : (e[0] == '2' ? 2 : (e[0] == '4' ? 4 : 0));  // (tests, A/B runs)
  if (const char *e = getenv("JB_DDMC_QUEUES")) ctx->ddmc_queues = e[0] != '0';
  if (const char *e = getenv("JB_DDMC_LDS_CODES")) ctx->ddmc_lds_codes = e[0] != '0';
  if (const char *e = getenv("JB_HANDOFF_MIN_RECORDS")) ctx->min_records = atoll(e) > 0 ? atoll(e) : 0;
  if (const char *e = getenv("JB_DDMC_MAX_CLASSES")) {   // (tests: the fall-back when a mesh has more distinct step records)
    const int v = atoi(e);
    ctx->max_classes = v < 0 ? 0 : (v > kMaxClasses ? kMaxClasses : v);
  }
  const char *ledger_env = getenv("JB_LEDGER");
  ctx->dp.key0 = (uint32_t)params->seed;  // RngPool rng_pool(seed): unadjusted (quirk 1)
  ctx->dp.use_ddmc = params->use_ddmc;
  ctx->dp.do_feedback = params->do_feedback;
  ctx->dp.tau_ddmc = params->tau_ddmc;
  ctx->dp.c = opacity->c;
  ctx->dp.sb = opacity->sb;
  ctx->dp.cv = eos->cv;
  ctx->dp.kappa_a = opacity->kappa;
  ctx->dp.kappa_s = scattering->kappa_s;
  ctx->dp.apm = scattering->apm;
  ctx->dp.opac_model = opacity->model;
  ctx->dp.lean = ctx->lean_arith ? 1 : 0;
  ctx->dp.hyb_imc_budget = JB_HYBRID_IMC_BUDGET;    // (tuning aids: environment overrides)
  ctx->dp.hyb_park_budget = JB_HYBRID_PARK_BUDGET;
  if (const char *e = getenv("JB_HYBRID_IMC_BUDGET")) ctx->dp.hyb_imc_budget = atoi(e) > 0 ? atoi(e) : JB_HYBRID_IMC_BUDGET;
  if (const char *e = getenv("JB_HYBRID_PARK_BUDGET")) ctx->dp.hyb_park_budget = atoi(e) > 0 ? atoi(e) : JB_HYBRID_PARK_BUDGET;
  ctx->dp.ep_A = ctx->dp.ep_B = ctx->dp.ep_E = 0.0;
  {
    // CGS constants (CODATA 2018): electron charge (esu), electron / proton mass, Planck,
    // Boltzmann, speed of light, Thomson cross-section
    const double qe = 4.803204712570263e-10, me = 9.1093837015e-28, mp = 1.67262192369e-24,
                 hp = 6.62607015e-27, kb = 1.380649e-16, cl = 2.99792458e10,
                 sigma_t = 6.6524587321e-25, pi = 3.14159265358979323846;
    if (opacity->model == JB_OPAC_EPBREMSS) {
      const double tau = opacity->time_scale, mu = opacity->mass_scale, lam = opacity->length_scale,
                   th = opacity->temperature_scale;
      const double e6 = (qe * qe) * (qe * qe) * (qe * qe);
      const double k_abs = (4.0 * e6) / (3.0 * me * hp * cl) * std::sqrt((2.0 * pi) / (3.0 * kb * me));
      const double k_em = std::sqrt((2.0 * pi * kb) / (3.0 * me)) *
                          ((32.0 * pi * e6) / (3.0 * hp * me * (cl * cl * cl)));
      const double n_per_rho = (mu / (lam * lam * lam)) / mp;  // n_e = n_i per unit code density
      const double n2 = n_per_rho * n_per_rho, tau3 = tau * tau * tau;
      ctx->dp.ep_A = lam * k_abs * n2 / std::sqrt(th) * tau3;
      ctx->dp.ep_B = hp / (kb * th * tau);
      ctx->dp.ep_E = k_em * std::sqrt(th) * n2 * (tau3 * lam / mu);
      ctx->dp.kappa_a = 0.0;
    }
    if (scattering->model == JB_SCAT_THOMSON)
      ctx->dp.kappa_s = sigma_t / (scattering->length_scale * scattering->length_scale);
  }
  // (a failure below must not leak the context: jb_finalize releases whatever exists)
  auto init_device_state = [&]() -> jb_status {
    hipDeviceProp_t prop;
    JB_HIP(hipGetDeviceProperties(&prop, device));
    ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    JB_HIP(hipMalloc(&ctx->counters_d, kCounterWords * sizeof(unsigned long long)));
    JB_HIP(hipMemset(ctx->counters_d, 0, kCounterWords * sizeof(unsigned long long)));
    JB_HIP(hipHostMalloc(&ctx->counters_h, kCounterWords * sizeof(unsigned long long)));
    // the refined reciprocal of c that the step functions divide with (jb_math.hpp, m_div_r): one
    // device evaluation, so that it is the v_rcp_f64-seeded value the kernels would compute
    hipLaunchKernelGGL(k_rcp_refined, dim3(1), dim3(1), 0, 0, ctx->dp.c, (double *)ctx->counters_d);
    JB_HIP(hipMemcpy(&ctx->dp.rc, ctx->counters_d, sizeof(double), hipMemcpyDeviceToHost));
    JB_HIP(hipMemset(ctx->counters_d, 0, sizeof(double)));
#ifdef JB_INVARIANTS
    const jb_status ist = inv_setup(device);
    if (ist != JB_COMPLETE) return ist;
#endif
    return JB_COMPLETE;
  };
  const jb_status st = init_device_state();
  if (st != JB_COMPLETE) {
    jb_finalize(ctx);
    return st;
  }
  if (ledger_env && ledger_env[0] == '1') {
    const jb_status lst = jb_ledger_enable(ctx, 1);
    if (lst != JB_COMPLETE) {
      jb_finalize(ctx);
      return lst;
    }
  }
  *out = ctx;
  return JB_COMPLETE;
}

extern "C" jb_status jb_finalize(jb_context *ctx) {
  if (!ctx) return JB_COMPLETE;
  (void)hipSetDevice(ctx->device);
  // (a mesh destroyed after its context must not look for it: its open accumulators are let go of here)
  for (jb_mesh *m : ctx->dep_open_meshes) m->dep_open = false;
  ctx->dep_open_meshes.clear();
  if (ctx->counters_d) (void)hipFree(ctx->counters_d);
  if (ctx->counters_h) (void)hipHostFree(ctx->counters_h);
  if (ctx->scratch_d) (void)hipFree(ctx->scratch_d);
  if (ctx->ledger_d) (void)hipFree(ctx->ledger_d);
  for (DevBuf *b : {&ctx->xch, &ctx->step_send, &ctx->step_recv, &ctx->step_gather, &ctx->moments, &ctx->ledger_gather,
                    &ctx->bs_prefix, &ctx->bs_out, &ctx->gcomb_eblock})
    (void)dev_free(*b);
  for (hipEvent_t e : ctx->tev) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->sort_ev) if (e) (void)hipEventDestroy(e);
  delete ctx;
  return JB_COMPLETE;
}

extern "C" jb_status jb_set_stream(jb_context *ctx, void *hip_stream) {
  if (!ctx) return fail(JB_ERR_INVALID, "null context");
  ctx->stream = (hipStream_t)hip_stream;
  return JB_COMPLETE;
}

extern "C" jb_status jb_synchronize(jb_context *ctx) {
  if (!ctx) return fail(JB_ERR_INVALID, "null context");
  JB_HIP(hipSetDevice(ctx->device));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  return JB_COMPLETE;
}

extern "C" int32_t jb_param_seed(const jb_context *ctx) {
  return ctx->params.unique_rank_seeds ? ctx->params.seed + ctx->params.rank : ctx->params.seed;
}

extern "C" double jb_estimate_timestep(const jb_context *ctx) { return ctx->params.dt; }

// ------------------------------------------------------------------------------------------------
template <class T>
static jb_status upload(jb_mesh *m, const T *host, size_t count, const T **dev) {
  void *p = nullptr;
  if (count == 0) count = 1;
  JB_HIP(hipMalloc(&p, count * sizeof(T)));
  m->owned.push_back(p);
  if (host) JB_HIP(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
  *dev = (const T *)p;
  return JB_COMPLETE;
}

extern "C" jb_status jb_mesh_create(jb_context *ctx, const jb_mesh_view *v, jb_mesh **out) {
  if (!ctx || !v || !out) return fail(JB_ERR_INVALID, "jb_mesh_create: null argument");
  if (v->ndim < 1 || v->ndim > 3) return fail(JB_ERR_INVALID, "ndim must be 1, 2 or 3");
  if (v->ng < 1) return fail(JB_ERR_INVALID, "ng >= 1 required (face fields share the cell layout)");
  if (v->nblocks < 1 || v->nblocks_total < v->nblocks)
    return fail(JB_ERR_INVALID, "bad block counts");
  for (int d = 0; d < 3; ++d) {
    if (v->nx[d] < 1 || v->nleaf[d] < 1) return fail(JB_ERR_INVALID, "bad nx / nleaf");
    if (d >= v->ndim && v->nx[d] != 1) return fail(JB_ERR_INVALID, "inactive dimension with nx != 1");
    if (!(v->gmax[d] > v->gmin[d])) return fail(JB_ERR_INVALID, "empty domain");
  }
  if (!v->leaf_map || !v->owner || !v->local_index || !v->gid || !v->blk_xmin || !v->blk_xmax ||
      !v->blk_dx || !v->blk_level || !v->blk_nbr_lev)
    return fail(JB_ERR_INVALID, "jb_mesh_create: missing table");
  if (!v->rho || !v->sie || !v->u || !v->fleck || !v->tally || !v->edelta || !v->src_ew ||
      !v->src_num)
    return fail(JB_ERR_INVALID, "jb_mesh_create: missing field pointer table");
  if (ctx->params.use_ddmc && (!v->P1 || (v->ndim > 1 && !v->P2) || (v->ndim > 2 && !v->P3)))
    return fail(JB_ERR_INVALID, "use_ddmc requires the ddmc_face_prob arrays");
  // every table index the kernels will form is checked here, once
  const long long nleaf = (long long)v->nleaf[0] * v->nleaf[1] * v->nleaf[2];
  for (long long q = 0; q < nleaf; ++q)
    if (v->leaf_map[q] < 0 || v->leaf_map[q] >= v->nblocks_total)
      return fail(JB_ERR_INVALID, "leaf_map entry out of range");
  for (int g = 0; g < v->nblocks_total; ++g) {
    const int li = v->local_index[g];
    if (li >= v->nblocks || li < -1 || (li >= 0 && v->gid[li] != g))
      return fail(JB_ERR_INVALID, "local_index / gid inconsistent for block %d", g);
    if (v->owner[g] == v->rank) {
      if (li < 0) return fail(JB_ERR_INVALID, "owned block %d is not resident", g);
      if (v->owned && !v->owned[li]) return fail(JB_ERR_INVALID, "block %d owned but flagged as halo", g);
    } else if (li >= 0 && (!v->owned || v->owned[li])) {
      return fail(JB_ERR_INVALID, "resident block %d of another rank must be flagged as a halo copy", g);
    }
    if (v->owner[g] < 0) return fail(JB_ERR_INVALID, "negative owner rank");
  }
  JB_HIP(hipSetDevice(ctx->device));
  jb_mesh *m = new (std::nothrow) jb_mesh();
  if (!m) return fail(JB_ERR_HIP, "out of host memory");
  m->ctx = ctx;
  DevMesh &D = m->dm;
  D.ndim = v->ndim; D.ng = v->ng; D.nblocks = v->nblocks; D.nblocks_total = v->nblocks_total;
  D.rank = v->rank;
  for (int d = 0; d < 3; ++d) { D.nx[d] = v->nx[d]; D.nleaf[d] = v->nleaf[d]; D.gmin[d] = v->gmin[d]; D.gmax[d] = v->gmax[d]; }
  for (int f = 0; f < 6; ++f) {
    if (v->bc[f] < 0 || v->bc[f] > 2) { delete m; return fail(JB_ERR_INVALID, "unknown swarm boundary"); }
    D.bc[f] = v->bc[f];
  }
  D.is = v->ng; D.js = v->ndim >= 2 ? v->ng : 0; D.ks = v->ndim >= 3 ? v->ng : 0;
  D.ni = v->nx[0] + 2 * D.is; D.nj = v->nx[1] + 2 * D.js; D.nk = v->nx[2] + 2 * D.ks;
  D.ie = D.is + v->nx[0] - 1; D.je = D.js + v->nx[1] - 1; D.ke = D.ks + v->nx[2] - 1;
  D.ncell = v->nx[0] * v->nx[1] * v->nx[2];
  D.ntot = (long long)D.ni * D.nj * D.nk;
  D.inv_ntot = 1.0 / (double)D.ntot;
  D.inv_nij = 1.0 / ((double)D.ni * (double)D.nj);
  D.inv_ni = 1.0 / (double)D.ni;
  if (D.ntot * 8 >= (1ll << 31)) { delete m; return fail(JB_ERR_INVALID, "block too large: cell indices are 32-bit"); }
  if (D.ni >= (1 << 23) || (long long)D.nj * D.nk >= (1ll << 23)) {
    delete m;
    return fail(JB_ERR_INVALID, "block too large: ni and nj * nk must stay below 2^23 (24-bit cell index arithmetic)");
  }
  if (v->nblocks_total >= (1 << 20)) {  // cell_stream_id packs the global block id in 20 bits
    delete m;
    return fail(JB_ERR_INVALID, "more than 2^20 blocks: the per-cell source streams would alias");
  }
  if (D.ncell >= (1 << 24)) {           // ... and the cell in 24
    delete m;
    return fail(JB_ERR_INVALID, "more than 2^24 cells per block: the per-cell source streams would alias");
  }
  {
    const char *off = getenv("JB_NO_EXACT_GEOM");  // tests: run the general kernels on an exact mesh
    bool exact = !(off && off[0] == '1');
    for (int b = 0; exact && b < v->nblocks; ++b)
      for (int d = 0; exact && d < v->ndim; ++d) {
        const double dx = v->blk_dx[3 * b + d], x0 = v->blk_xmin[3 * b + d];
        int e;
        const double q = x0 / dx;  // exact when dx is a power of two
        exact = dx > 0.0 && std::frexp(dx, &e) == 0.5 && q == std::nearbyint(q) &&
                std::fabs(q) < 1099511627776.0;  // 2^40: (q + i + 0.5) dx is exact
      }
    D.exact = exact ? 1 : 0;
    // (the EXACT tracking kernels also address the mean-free-path arrays of all resident blocks
    // with 32-bit byte offsets: 16 bytes per cell)
    m->offsets32 = 16ull * (unsigned long long)D.ntot * (unsigned long long)v->nblocks < (1ull << 32);
    m->exact_geom = exact && m->offsets32;
    m->cell_ok = m->offsets32 && 8ll * D.ni < (1ll << 23) && (v->ndim < 3 || 8ll * D.ni * D.nj < (1ll << 23));
    m->uniform_geom = true;
    for (int b = 1; b < v->nblocks; ++b)
      for (int d = 0; d < 3; ++d) m->uniform_geom = m->uniform_geom && v->blk_dx[3 * b + d] == v->blk_dx[d];
    m->equal_h = v->nblocks > 0;
    for (int d = 1; d < v->ndim; ++d) m->equal_h = m->equal_h && v->blk_dx[d] == v->blk_dx[0];
  }
  int maxrank = 0;
  for (int g = 0; g < v->nblocks_total; ++g) maxrank = v->owner[g] > maxrank ? v->owner[g] : maxrank;
  m->nranks_seen = maxrank + 1;
  m->gid_host.assign(v->gid, v->gid + v->nblocks);
  for (int b = 0; b < v->nblocks; ++b) m->nowned += (!v->owned || v->owned[b]) ? 1 : 0;
  m->owned_host.assign((size_t)v->nblocks, 1);
  for (int b = 0; v->owned && b < v->nblocks; ++b) m->owned_host[(size_t)b] = v->owned[b] ? 1 : 0;
  for (int g = 1; g < v->nblocks_total; ++g) m->one_owner = m->one_owner && v->owner[g] == v->owner[0];
  m->bface_host.assign(6 * (size_t)v->nblocks, 0);
  for (int b = 0; b < v->nblocks; ++b)
    for (int f = 0; f < 2 * v->ndim && (!v->owned || v->owned[b]); ++f) {   // (bsource_on_boundary, on the host)
      const int d = f >> 1;
      const double half = 0.5 * v->blk_dx[3 * b + d];
      m->bface_host[6 * (size_t)b + f] =
          (f & 1) ? v->blk_xmax[3 * b + d] > v->gmax[d] - half : v->blk_xmin[3 * b + d] < v->gmin[d] + half;
    }
  jb_status st;
#define UP(field, count)                                                         \
  if ((st = upload(m, v->field, (size_t)(count), &D.field)) != JB_COMPLETE) {     \
    jb_mesh_destroy(m);                                                          \
    return st;                                                                   \
  }
  UP(leaf_map, nleaf);
  UP(owner, v->nblocks_total);
  UP(local_index, v->nblocks_total);
  UP(gid, v->nblocks);
  {
    std::vector<int32_t> ow(v->nblocks, 1);
    if (v->owned) ow.assign(v->owned, v->owned + v->nblocks);
    if ((st = upload(m, ow.data(), ow.size(), &D.owned)) != JB_COMPLETE) {
      jb_mesh_destroy(m);
      return st;
    }
  }
  UP(blk_xmin, 3 * v->nblocks);
  UP(blk_xmax, 3 * v->nblocks);
  UP(blk_dx, 3 * v->nblocks);
  {
    std::vector<double> inv(3 * (size_t)v->nblocks);
    for (size_t q = 0; q < inv.size(); ++q) inv[q] = 1.0 / v->blk_dx[q];
    if ((st = upload(m, inv.data(), inv.size(), &D.blk_inv_dx)) != JB_COMPLETE) {
      jb_mesh_destroy(m);
      return st;
    }
    for (int d = 0; d < 3; ++d)
      D.inv_leaf_len[d] = 1.0 / ((v->gmax[d] - v->gmin[d]) / (double)v->nleaf[d]);
  }
  UP(blk_level, v->nblocks);
  UP(blk_nbr_lev, 6 * v->nblocks);
#undef UP
#define UPF(field)                                                                           \
  if (v->field) {                                                                            \
    for (int b = 0; b < v->nblocks; ++b)                                                     \
      if (!v->field[b]) { jb_mesh_destroy(m); return fail(JB_ERR_INVALID, "null block pointer in " #field); } \
    const double *const *tmp = nullptr;                                                      \
    if ((st = upload(m, (const double *const *)v->field, (size_t)v->nblocks, &tmp)) != JB_COMPLETE) { \
      jb_mesh_destroy(m);                                                                    \
      return st;                                                                             \
    }                                                                                        \
    D.field = (double *const *)tmp;                                                          \
  } else {                                                                                   \
    D.field = nullptr;                                                                       \
  }
  UPF(rho) UPF(sie) UPF(u) UPF(fleck) UPF(tally) UPF(edelta) UPF(src_ew) UPF(src_num)
  UPF(P1) UPF(P2) UPF(P3)
#undef UPF
  // face-crossing table of the tracking kernels (DevMesh::nbr_ent / nbr_x0)
  {
    std::vector<int32_t> ent(6 * (size_t)v->nblocks, -1);
    std::vector<double> x0(6 * (size_t)v->nblocks, 0.0);
    // k_imc_cell: a photon that has stepped through face f of block b sits in b's ghost cell behind
    // that face; dq moves the byte offset of that cell (16 ntot bytes per block, 8 per cell) to the
    // cell it is in after the crossing -- the first / last interior cell along the axis of the
    // destination block, or, at a reflecting wall, the interior cell it came from
    std::vector<int32_t> dq(6 * (size_t)v->nblocks, 0);
    const long long stride8[3] = {8, 8ll * D.ni, 8ll * D.ni * D.nj};
    const int first[3] = {D.is, D.js, D.ks};
    for (int b = 0; b < v->nblocks; ++b) {
      long long l0[3] = {0, 0, 0}, cnt[3] = {1, 1, 1};
      bool ok = true;
      for (int d = 0; d < v->ndim; ++d) {
        const double leaf = (v->gmax[d] - v->gmin[d]) / (double)v->nleaf[d];
        const double q0 = (v->blk_xmin[3 * b + d] - v->gmin[d]) / leaf;
        const double qc = (v->blk_xmax[3 * b + d] - v->blk_xmin[3 * b + d]) / leaf;
        l0[d] = (long long)std::llround(q0);
        cnt[d] = (long long)std::llround(qc);
        ok = ok && std::fabs(q0 - (double)l0[d]) < 1e-6 && std::fabs(qc - (double)cnt[d]) < 1e-6 &&
             cnt[d] >= 1 && l0[d] >= 0 && l0[d] + cnt[d] <= v->nleaf[d];
      }
      if (!ok) continue;  // (a block that is not a union of leaves: general relocation only)
      for (int d = 0; d < v->ndim; ++d)
        for (int up = 0; up < 2; ++up) {
          const int f = 2 * d + up;
          long long l[3] = {l0[0], l0[1], l0[2]};
          l[d] = up ? l0[d] + cnt[d] : l0[d] - 1;
          int kind = 0;
          if (l[d] < 0 || l[d] >= v->nleaf[d]) {  // the face lies on the domain boundary
            const int bc = v->bc[f];
            if (bc == JB_BC_REFLECT) {
              ent[6 * (size_t)b + f] = (2 << 28) | b;
              x0[6 * (size_t)b + f] = v->blk_xmin[3 * b + d] - (double)first[d] * v->blk_dx[3 * b + d];
              dq[6 * (size_t)b + f] = (int32_t)(up ? -stride8[d] : stride8[d]);
              continue;
            }
            if (bc != JB_BC_PERIODIC) continue;  // outflow: the particle escapes
            kind = 1;
            l[d] = up ? 0 : v->nleaf[d] - 1;
          }
          const int g = v->leaf_map[(l[2] * v->nleaf[1] + l[1]) * v->nleaf[0] + l[0]];
          const int li = v->local_index[g];
          if (li < 0) continue;  // destination not resident: hand-off
          bool same = true;  // same size, aligned across the face
          for (int e = 0; e < 3; ++e) {
            same = same && v->blk_dx[3 * li + e] == v->blk_dx[3 * b + e];
            if (e != d && e < v->ndim) same = same && v->blk_xmin[3 * li + e] == v->blk_xmin[3 * b + e];
          }
          if (!same || li >= (1 << 28)) continue;
          ent[6 * (size_t)b + f] = (kind << 28) | li;
          x0[6 * (size_t)b + f] = v->blk_xmin[3 * li + d] - (double)first[d] * v->blk_dx[3 * li + d];
          if (m->offsets32)  // (offsets below 4 GiB: the difference fits 32 bits, as a wrapping sum)
            dq[6 * (size_t)b + f] = (int32_t)(uint32_t)(16ll * D.ntot * ((long long)li - b) +
                                                        (up ? -stride8[d] : stride8[d]) * v->nx[d]);
        }
    }
    if ((st = upload(m, dq.data(), dq.size(), &m->nbr_dq)) != JB_COMPLETE) { jb_mesh_destroy(m); return st; }
    if ((st = upload(m, ent.data(), ent.size(), &D.nbr_ent)) != JB_COMPLETE) { jb_mesh_destroy(m); return st; }
    if ((st = upload(m, x0.data(), x0.size(), &D.nbr_x0)) != JB_COMPLETE) { jb_mesh_destroy(m); return st; }
  }
  {
    // [0] = 1 until UpdateDerivedTransportFields has looked at the cells; [1] = distinct step records (cell classes)
    const int init[2] = {1, 0};
    const int *flag = nullptr;
    if ((st = upload(m, init, 2, &flag)) != JB_COMPLETE) { jb_mesh_destroy(m); return st; }
    D.not_all_ddmc = (int *)flag;
  }
  D.ddmc_code = nullptr;
  D.ddmc_class = nullptr;
  D.ddmc_class_slot = nullptr;
  D.ddmc_base = nullptr;
  D.ddmc_step = nullptr;
  D.lam_hyb = nullptr;
  // gray (frequency-independent) opacities: library-owned per-cell mean-free-path arrays
  D.lam_base = nullptr;
  D.lam_abs = nullptr;
  D.lam_sc = nullptr;
  D.ddmc_cell = nullptr;
  // JB_PER_EVENT_OPACITY=1 keeps the general path -- EOS and opacities evaluated per event from
  // rho, sie and the photon energy, as the reference does (transport.cpp:122-127) -- also for gray
  // models; it is what a frequency-dependent opacity would run, and the tests exercise it
  const char *general = getenv("JB_PER_EVENT_OPACITY");
  const bool per_event = general && general[0] == '1';
  if (!per_event && ctx->opac.model == JB_OPAC_GRAY) {  // (ThomsonS has the GrayS form)
    const size_t per = (size_t)D.ntot;
    double *base = nullptr;
    hipError_t e = hipMalloc(&base, sizeof(double) * per * 2 * (size_t)v->nblocks);
    if (e != hipSuccess) { jb_mesh_destroy(m); return fail(JB_ERR_HIP, "hipMalloc of the mean-free-path arrays failed: %s", hipGetErrorString(e)); }
    m->owned.push_back(base);
    std::vector<const double *> pa(v->nblocks), ps(v->nblocks);
    for (int b = 0; b < v->nblocks; ++b) {
      pa[b] = base + (size_t)(2 * b) * per;
      ps[b] = base + (size_t)(2 * b + 1) * per;
    }
    D.lam_base = base;
    const double *const *tmp = nullptr;
    if ((st = upload(m, (const double *const *)pa.data(), (size_t)v->nblocks, &tmp)) != JB_COMPLETE) { jb_mesh_destroy(m); return st; }
    D.lam_abs = (double *const *)tmp;
    if ((st = upload(m, (const double *const *)ps.data(), (size_t)v->nblocks, &tmp)) != JB_COMPLETE) { jb_mesh_destroy(m); return st; }
    D.lam_sc = (double *const *)tmp;
    D.ddmc_cell = nullptr;
    if (ctx->params.use_ddmc) {
      double *pack = nullptr;
      e = hipMalloc(&pack, sizeof(double) * per * 8 * (size_t)v->nblocks);
      if (e != hipSuccess) { jb_mesh_destroy(m); return fail(JB_ERR_HIP, "hipMalloc of the DDMC cell records failed: %s", hipGetErrorString(e)); }
      m->owned.push_back(pack);
      std::vector<const double *> pp(v->nblocks);
      for (int b = 0; b < v->nblocks; ++b) pp[b] = pack + (size_t)b * per * 8;
      if ((st = upload(m, (const double *const *)pp.data(), (size_t)v->nblocks, &tmp)) != JB_COMPLETE) { jb_mesh_destroy(m); return st; }
      D.ddmc_cell = (double *const *)tmp;
      D.ddmc_base = pack;
      double *step_rec = nullptr;
      e = hipMalloc(&step_rec, sizeof(double) * per * 8 * (size_t)v->nblocks);
      if (e != hipSuccess) { jb_mesh_destroy(m); return fail(JB_ERR_HIP, "hipMalloc of the DDMC step records failed: %s", hipGetErrorString(e)); }
      m->owned.push_back(step_rec);
      // (on the context's stream, like k_lam_ghost_codes below: a null-stream memset is not ordered against a
      // kernel on a non-blocking stream the host handed in with jb_set_stream, and would wipe the ghost codes)
      (void)hipMemsetAsync(step_rec, 0, sizeof(double) * per * 8 * (size_t)v->nblocks, ctx->stream);
      D.ddmc_step = step_rec;
      // cell codes + the table of distinct step records (k_ddmc_all<.., GATHER 4>); a code holds a record
      // number in 29 bits
      if ((unsigned long long)per * (unsigned long long)v->nblocks < (1ull << 29)) {
        unsigned *code = nullptr;
        e = hipMalloc(&code, sizeof(unsigned) * per * (size_t)v->nblocks);
        if (e != hipSuccess) { jb_mesh_destroy(m); return fail(JB_ERR_HIP, "hipMalloc of the DDMC cell codes failed: %s", hipGetErrorString(e)); }
        m->owned.push_back(code);
        // (ghost cells that k_lam_ghost_codes leaves alone -- there are none -- would read "class 0")
        (void)hipMemsetAsync(code, 0, sizeof(unsigned) * per * (size_t)v->nblocks, ctx->stream);
        double *cls = nullptr;
        e = hipMalloc(&cls, sizeof(double) * 8 * kMaxClasses + sizeof(int) * 2 * kClassSlots);
        if (e != hipSuccess) { jb_mesh_destroy(m); return fail(JB_ERR_HIP, "hipMalloc of the DDMC class table failed: %s", hipGetErrorString(e)); }
        m->owned.push_back(cls);
        D.ddmc_code = code;
        D.ddmc_class = cls;
        D.ddmc_class_slot = (int *)(cls + 8 * kMaxClasses);
      }
      double *hyb = nullptr;
      e = hipMalloc(&hyb, sizeof(double) * per * (size_t)v->nblocks);
      if (e != hipSuccess) { jb_mesh_destroy(m); return fail(JB_ERR_HIP, "hipMalloc of the hybrid mean-free-path array failed: %s", hipGetErrorString(e)); }
      m->owned.push_back(hyb);
      (void)hipMemsetAsync(hyb, 0, sizeof(double) * per * (size_t)v->nblocks, ctx->stream);
      D.lam_hyb = hyb;
    }
    // ghost cells of the scattering mean free path: which face of the block lies between them and
    // the interior (k_imc_cell reads "the photon has left its block" off the value it gathers);
    // UpdateDerivedTransportFields only ever writes interior cells
    hipLaunchKernelGGL(k_lam_ghost_codes, dim3(grid_for(ctx, (long long)v->nblocks * D.ntot)), dim3(kBlock), 0,
                       ctx->stream, D, m->nbr_dq);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
      jb_mesh_destroy(m);
      return fail(JB_ERR_HIP, "writing the ghost-cell codes of the mean-free-path arrays failed");
    }
  }
  {
    const DevMesh *copy = nullptr;
    if ((st = upload(m, &D, 1, &copy)) != JB_COMPLETE) { jb_mesh_destroy(m); return st; }
    m->dm_dev = copy;
  }
  *out = m;
  return JB_COMPLETE;
}

extern "C" jb_status jb_mesh_destroy(jb_mesh *m) {
  if (!m) return JB_COMPLETE;
  if (m->dep_open) deposit_mark_closed(m->ctx, m);   // (dep_open: the context is alive, jb_finalize clears it)
  for (void *p : m->owned) (void)hipFree(p);
  delete m;
  return JB_COMPLETE;
}

static DevSwarm dev_swarm(const jb_swarm_view *s) {
  DevSwarm S;
  S.x = s->x; S.y = s->y; S.z = s->z; S.vx = s->vx; S.vy = s->vy; S.vz = s->vz;
  S.t = s->t; S.w = s->w; S.e = s->e;
  S.ip = s->ip; S.jp = s->jp; S.kp = s->kp; S.blk = s->blk; S.status = s->status;
  S.id = (uint64_t *)s->id; S.rng = (uint64_t *)s->rng;
  return S;
}

static jb_status check_swarm(const jb_swarm_view *s, const char *who) {
  if (!s) return fail(JB_ERR_INVALID, "%s: null swarm", who);
  if (s->n < 0 || s->n > s->capacity) return fail(JB_ERR_INVALID, "%s: swarm n outside [0, capacity]", who);
  if (s->capacity > 0 && (!s->x || !s->y || !s->z || !s->vx || !s->vy || !s->vz || !s->t || !s->w ||
                          !s->e || !s->ip || !s->jp || !s->kp || !s->blk || !s->status || !s->id ||
                          !s->rng))
    return fail(JB_ERR_INVALID, "%s: null swarm array", who);
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
extern "C" jb_status jb_update_derived_transport_fields(jb_context *ctx, jb_mesh *mesh, double dt) {
  JB_RANGE("Jaybenne::UpdateDerivedTransportFields");
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  const DevMesh &M = mesh->dm;
  const long long cells = (long long)M.nblocks * M.ncell;
  hipLaunchKernelGGL(k_fleck, dim3(grid_for(ctx, 64ll * M.nblocks * M.nx[1] * M.nx[2])), dim3(kBlock), 0,
                     ctx->stream, M, ctx->dp, dt);
  if (ctx->params.use_ddmc) {
    const int g = grid_for(ctx, cells * 2);
    hipLaunchKernelGGL(k_face_prob<0>, dim3(g), dim3(kBlock), 0, ctx->stream, M, ctx->dp);
    if (M.ndim > 1) hipLaunchKernelGGL(k_face_prob<1>, dim3(g), dim3(kBlock), 0, ctx->stream, M, ctx->dp);
    if (M.ndim > 2) hipLaunchKernelGGL(k_face_prob<2>, dim3(g), dim3(kBlock), 0, ctx->stream, M, ctx->dp);
    if (M.ddmc_cell) {
      // JB_NO_DDMC_ALL=1 keeps the general kernel also on all-DDMC meshes (tests, A/B)
      JB_HIP(hipMemsetAsync(M.not_all_ddmc, ctx->no_ddmc_all ? 1 : 0, sizeof(int), ctx->stream));
      JB_HIP(hipMemsetAsync(M.not_all_ddmc + 1, 0, sizeof(int), ctx->stream));   // the distinct step records are numbered afresh
      if (M.ddmc_class_slot) JB_HIP(hipMemsetAsync(M.ddmc_class_slot, 0, sizeof(int) * 2 * kClassSlots, ctx->stream));
      mesh->not_all_ddmc_host = -1;
      const int gp = grid_for(ctx, cells);
      const int mc = ctx->max_classes;
      if (M.ndim == 1) hipLaunchKernelGGL(k_ddmc_pack<1>, dim3(gp), dim3(kBlock), 0, ctx->stream, M, ctx->dp, mc);
      else if (M.ndim == 2) hipLaunchKernelGGL(k_ddmc_pack<2>, dim3(gp), dim3(kBlock), 0, ctx->stream, M, ctx->dp, mc);
      else hipLaunchKernelGGL(k_ddmc_pack<3>, dim3(gp), dim3(kBlock), 0, ctx->stream, M, ctx->dp, mc);
#ifdef JB_INVARIANTS
      if (M.ddmc_code && M.ddmc_class)   // (checked build) DDMC_CLASS
        hipLaunchKernelGGL(k_inv_ddmc_class, dim3(gp), dim3(kBlock), 0, ctx->stream, M, mc);
#endif
    }
  }
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

static jb_status source_count_finish(jb_context *ctx, jb_mesh *mesh, int *nper_d, int32_t *nper_block_host);

extern "C" jb_status jb_source_photons_count(jb_context *ctx, jb_mesh *mesh, int source_type,
                                             double dt, int blocks_in_call, uint32_t epoch,
                                             int32_t *nper_block_host, int32_t *prefix_dev) {
  JB_RANGE("Jaybenne::SourcePhotons1");
  if (!ctx || !mesh || !nper_block_host || !prefix_dev) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  if (ctx->params.source_strategy == JB_STRATEGY_ENERGY)
    return fail(JB_ERR_INVALID, "Energy source strategy not implemented!");  // sourcing.cpp:38
  if (epoch >= (1u << 20))  // cell_stream_id keeps the source-call counter in 20 bits
    return fail(JB_ERR_INVALID, "more than 2^20 source calls: the per-cell rounding streams would repeat");
  const DevMesh &M = mesh->dm;
  if (source_type == JB_SOURCE_EMISSION && !ctx->params.do_emission) {  // sourcing.cpp:41-43
    for (int b = 0; b < M.nblocks; ++b) nper_block_host[b] = 0;
    return JB_COMPLETE;
  }
  if (ctx->source_allocation == JB_ALLOC_ENERGY) {
    // (source allocation: energy pass, total, count pass in a row -- only where this rank sees every block's sum)
    if (M.nblocks != M.nblocks_total || mesh->nowned != M.nblocks_total)
      return fail(JB_ERR_INVALID, "jb_source_photons_count: source allocation is energy and the mesh is not wholly "
                  "resident and owned (%d of %d blocks owned here): call jb_source_energy_sums, add the block sums of "
                  "all ranks by jb_source_energy_total, then jb_source_photons_count_energy", mesh->nowned,
                  M.nblocks_total);
    std::vector<double> e_local((size_t)M.nblocks), e_gid((size_t)M.nblocks_total, 0.0);
    jb_status st = jb_source_energy_sums(ctx, mesh, source_type, dt, e_local.data());
    if (st != JB_COMPLETE) return st;
    for (int b = 0; b < M.nblocks; ++b) e_gid[(size_t)mesh->gid_host[(size_t)b]] = e_local[(size_t)b];
    return jb_source_photons_count_energy(ctx, mesh, source_type, dt, epoch,
                                          jb_source_energy_total(e_gid.data(), M.nblocks_total), nper_block_host,
                                          prefix_dev);
  }
  mesh->salloc_last = false;
  mesh->salloc_sums_type = -1;
  if (blocks_in_call < 1) return fail(JB_ERR_INVALID, "blocks_in_call must be >= 1");
  jb_status st = ensure_scratch(ctx, (size_t)M.nblocks);
  if (st != JB_COMPLETE) return st;
  // sourcing.cpp:68-69
  const double npc = (double)ctx->params.num_particles / (double)M.ncell /
                     (double)(blocks_in_call * M.nblocks_total);
  int *nper_d = (int *)ctx->scratch_d;
  hipLaunchKernelGGL(k_source_count, dim3(M.nblocks), dim3(kBlock), 0, ctx->stream, M, ctx->dp,
                     source_type, dt, npc, epoch, nper_d, prefix_dev);
  JB_HIP(hipGetLastError());
  return source_count_finish(ctx, mesh, nper_d, nper_block_host);
}

// what follows the count kernel, whichever allocation it counted by: the tilt's slopes, the counts to the host
static jb_status source_count_finish(jb_context *ctx, jb_mesh *mesh, int *nper_d, int32_t *nper_block_host) {
  const DevMesh &M = mesh->dm;
  // (source tilt: the slopes of T^4 this call's photons are placed by, from the state the count read)
  mesh->tilt_valid = false;
  if (ctx->source_tilt == JB_TILT_LINEAR) {
    if (M.ng < 1) return fail(JB_ERR_INVALID, "source tilt: the blocks have no ghost layer to read the neighbours from");
    if (!mesh->tilt_d) {
      double *p = nullptr;
      JB_HIP(hipMalloc(&p, sizeof(double) * (size_t)M.nblocks * (size_t)M.ndim * (size_t)M.ncell));
      mesh->owned.push_back(p);
      mesh->tilt_d = p;
    }
    const dim3 g(grid_for(ctx, (long long)M.nblocks * M.ncell));
    if (M.ndim == 1) hipLaunchKernelGGL(k_source_tilt<1>, g, dim3(kBlock), 0, ctx->stream, M, ctx->dp, mesh->tilt_d);
    else if (M.ndim == 2) hipLaunchKernelGGL(k_source_tilt<2>, g, dim3(kBlock), 0, ctx->stream, M, ctx->dp, mesh->tilt_d);
    else hipLaunchKernelGGL(k_source_tilt<3>, g, dim3(kBlock), 0, ctx->stream, M, ctx->dp, mesh->tilt_d);
    JB_HIP(hipGetLastError());
    mesh->tilt_valid = true;
  }
  JB_HIP(hipMemcpyAsync(nper_block_host, nper_d, sizeof(int) * M.nblocks, hipMemcpyDeviceToHost,
                        ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  return JB_COMPLETE;
}

extern "C" jb_status jb_source_photons_fill(jb_context *ctx, jb_mesh *mesh,
                                            const jb_swarm_view *swarm, int source_type,
                                            double t_start, double dt,
                                            const int32_t *nper_block_host,
                                            const int32_t *prefix_dev,
                                            const int64_t *slot_base_host,
                                            const uint64_t *id_base_host) {
  return jb_source_photons_fill_range(ctx, mesh, swarm, source_type, t_start, dt, nper_block_host, prefix_dev,
                                      slot_base_host, id_base_host, nullptr, 1);
}

extern "C" jb_status jb_source_photons_fill_range(jb_context *ctx, jb_mesh *mesh,
                                                  const jb_swarm_view *swarm, int source_type,
                                                  double t_start, double dt,
                                                  const int32_t *nper_block_host,
                                                  const int32_t *prefix_dev,
                                                  const int64_t *slot_base_host,
                                                  const uint64_t *id_base_host,
                                                  const int32_t *first_in_block_host,
                                                  int set_energy_delta) {
  JB_RANGE("Jaybenne::SourcePhotons2");
  if (!ctx || !mesh || !nper_block_host || !prefix_dev || !slot_base_host || !id_base_host)
    return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_source_photons_fill");
  if (st != JB_COMPLETE) return st;
  const DevMesh &M = mesh->dm;
  if (source_type == JB_SOURCE_EMISSION && !ctx->params.do_emission) return JB_COMPLETE;
  st = ensure_scratch(ctx, (size_t)M.nblocks * 5 + 8);
  if (st != JB_COMPLETE) return st;
  const bool tilted = ctx->source_tilt == JB_TILT_LINEAR;
  if (tilted && !mesh->tilt_valid)
    return fail(JB_ERR_INVALID, "jb_source_photons_fill: source tilt is linear, but the mesh's last count call was not "
                                "made in that mode");
  const int32_t *nper = nper_block_host;
  std::vector<long long> tab(4 * (size_t)M.nblocks);
  long long total = 0;
  for (int b = 0; b < M.nblocks; ++b) {
    tab[b] = total;                                   // blk_first
    tab[M.nblocks + b] = slot_base_host[b];           // slot_base
    tab[2 * M.nblocks + b] = (long long)id_base_host[b];
    tab[3 * M.nblocks + b] = first_in_block_host ? (long long)first_in_block_host[b] : 0ll;
    if (first_in_block_host && first_in_block_host[b] < 0)
      return fail(JB_ERR_INVALID, "negative first photon number for block %d", b);
    if (nper[b] < 0) return fail(JB_ERR_INVALID, "negative particle count for block %d", b);
    if (nper[b] > 0 && (slot_base_host[b] < 0 || slot_base_host[b] + nper[b] > swarm->capacity))
      return fail(JB_ERR_CAPACITY, "swarm capacity %lld too small for block %d (slots %lld..%lld)",
                  (long long)swarm->capacity, b, (long long)slot_base_host[b],
                  (long long)slot_base_host[b] + nper[b]);
    total += nper[b];
  }
  long long *tab_d = ctx->scratch_d + M.nblocks;  // after the int counts (nblocks ints fit in nblocks words)
  JB_HIP(hipMemcpyAsync(tab_d, tab.data(), sizeof(long long) * tab.size(), hipMemcpyHostToDevice,
                        ctx->stream));
  // (set_energy_delta = 0: energy_delta := 0 instead of minus the emitted energy -- every rank of a
  // replicated-mesh run but one, so that the sum over ranks carries the emission once)
  if (!mesh->salloc_last)
    hipLaunchKernelGGL(k_source_edelta, dim3(grid_for(ctx, (long long)M.nblocks * M.ncell)),
                       dim3(kBlock), 0, ctx->stream, M, set_energy_delta ? source_type : 0);
  else   // (source allocation: one product per cell; k_source_edelta's loop runs once per photon of the cell)
    hipLaunchKernelGGL(k_salloc_edelta, dim3(grid_for(ctx, (long long)M.nblocks * M.ncell)),
                       dim3(kBlock), 0, ctx->stream, M, set_energy_delta ? source_type : 0);
  if (total > 0 && !tilted)
    hipLaunchKernelGGL(k_source_fill, dim3(grid_for(ctx, total)), dim3(kBlock), 0, ctx->stream, M,
                       ctx->dp, dev_swarm(swarm), source_type, t_start, dt, (const int *)prefix_dev,
                       (const long long *)tab_d, (const long long *)(tab_d + M.nblocks),
                       (const unsigned long long *)(tab_d + 2 * M.nblocks),
                       first_in_block_host ? (const long long *)(tab_d + 3 * M.nblocks) : (const long long *)nullptr,
                       total);
  if (total > 0 && tilted)   // (source tilt: the same photons, placed by the slopes of the count call)
    hipLaunchKernelGGL(k_source_fill_tilt, dim3(grid_for(ctx, total)), dim3(kBlock), 0, ctx->stream, M,
                       ctx->dp, dev_swarm(swarm), source_type, t_start, dt, (const int *)prefix_dev,
                       (const long long *)tab_d, (const long long *)(tab_d + M.nblocks),
                       (const unsigned long long *)(tab_d + 2 * M.nblocks),
                       first_in_block_host ? (const long long *)(tab_d + 3 * M.nblocks) : (const long long *)nullptr,
                       total, (const double *)mesh->tilt_d);
  JB_HIP(hipGetLastError());
#ifdef JB_INVARIANTS
  {  // (checked build) SWARM over the slots just filled
    long long lo = swarm->capacity, hi = 0;
    for (int b = 0; b < M.nblocks; ++b)
      if (nper[b] > 0) {
        lo = slot_base_host[b] < lo ? slot_base_host[b] : lo;
        hi = slot_base_host[b] + nper[b] > hi ? slot_base_host[b] + nper[b] : hi;
      }
    st = inv_sweep(ctx, M, dev_swarm(swarm), lo, hi, t_start + dt, true);
    if (st != JB_COMPLETE) return st;
  }
#endif
  JB_HIP(hipStreamSynchronize(ctx->stream));  // tab lives on this stack frame
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
// The source tilt (jb_kernel_tilt.hpp): the slopes are written by jb_source_photons_count, read by the fill.
extern "C" jb_status jb_set_source_tilt(jb_context *ctx, int mode) {
  if (!ctx || (mode != JB_TILT_NONE && mode != JB_TILT_LINEAR))
    return fail(JB_ERR_INVALID, "jb_set_source_tilt: mode = %d is neither JB_TILT_NONE nor JB_TILT_LINEAR", mode);
  ctx->source_tilt = mode;
  return JB_COMPLETE;
}
extern "C" int jb_get_source_tilt(const jb_context *ctx) {
  return ctx && ctx->source_tilt == JB_TILT_LINEAR ? JB_TILT_LINEAR : JB_TILT_NONE;
}

extern "C" jb_status jb_source_tilt_slopes(jb_context *ctx, const jb_mesh *mesh, int local_block, double *out_host) {
  if (!ctx || !mesh || !out_host) return fail(JB_ERR_INVALID, "jb_source_tilt_slopes: null argument");
  const DevMesh &M = mesh->dm;
  if (local_block < 0 || local_block >= M.nblocks)
    return fail(JB_ERR_INVALID, "jb_source_tilt_slopes: block %d outside 0..%d", local_block, M.nblocks - 1);
  if (!mesh->tilt_valid || !mesh->tilt_d)
    return fail(JB_ERR_INVALID, "jb_source_tilt_slopes: the mesh's last count call was not made under JB_TILT_LINEAR");
  if (!mesh->owned_host[(size_t)local_block])
    return fail(JB_ERR_INVALID, "jb_source_tilt_slopes: block %d is a halo copy: its owner has the slopes", local_block);
  JB_HIP(hipSetDevice(ctx->device));
  const size_t n = (size_t)M.ndim * (size_t)M.ncell;
  for (size_t q = n; q < 3 * (size_t)M.ncell; ++q) out_host[q] = 0.0;
  JB_HIP(hipMemcpyAsync(out_host, mesh->tilt_d + (size_t)local_block * n, sizeof(double) * n, hipMemcpyDeviceToHost,
                        ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
// The source allocation (jb_kernel_salloc.hpp): under JB_ALLOC_ENERGY a cell's photon number follows its energy.
extern "C" jb_status jb_set_source_allocation(jb_context *ctx, int mode) {
  if (!ctx || (mode != JB_ALLOC_UNIFORM && mode != JB_ALLOC_ENERGY))
    return fail(JB_ERR_INVALID, "jb_set_source_allocation: mode = %d is neither JB_ALLOC_UNIFORM nor JB_ALLOC_ENERGY", mode);
  ctx->source_allocation = mode;
  return JB_COMPLETE;
}
extern "C" int jb_get_source_allocation(const jb_context *ctx) {
  return ctx && ctx->source_allocation == JB_ALLOC_ENERGY ? JB_ALLOC_ENERGY : JB_ALLOC_UNIFORM;
}

// a cell's nu is at most N (1 + a few ulp), so a block's count stays below N + its cells: that must fit an int32
static jb_status salloc_check_target(const jb_context *ctx, const DevMesh &M) {
  const long long n_target = (long long)ctx->params.num_particles;
  if (n_target < 0 || n_target + (long long)M.ncell > 2147483647ll)
    return fail(JB_ERR_INVALID, "source allocation energy: num_particles = %lld plus the %d cells of a block passes "
                "2^31 - 1, the most a block's count can hold", n_target, M.ncell);
  return JB_COMPLETE;
}

extern "C" double jb_source_energy_total(const double *e_block_by_gid, int nblocks_total) {
  double e = 0.0;
  for (int g = 0; e_block_by_gid && g < nblocks_total; ++g) e += e_block_by_gid[g];
  return e;
}

extern "C" jb_status jb_source_energy_sums(jb_context *ctx, jb_mesh *mesh, int source_type, double dt,
                                           double *e_block_host) {
  JB_RANGE("Jaybenne::SourceEnergySums");
  if (!ctx || !mesh || !e_block_host) return fail(JB_ERR_INVALID, "jb_source_energy_sums: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  if (ctx->params.source_strategy == JB_STRATEGY_ENERGY)
    return fail(JB_ERR_INVALID, "Energy source strategy not implemented!");  // sourcing.cpp:38
  if (ctx->source_allocation != JB_ALLOC_ENERGY)
    return fail(JB_ERR_INVALID, "jb_source_energy_sums: source allocation is not energy (jb_set_source_allocation)");
  if (source_type != JB_SOURCE_THERMAL && source_type != JB_SOURCE_EMISSION)
    return fail(JB_ERR_INVALID, "jb_source_energy_sums: source_type = %d", source_type);
  const DevMesh &M = mesh->dm;
  mesh->salloc_sums_type = -1;
  if (source_type == JB_SOURCE_EMISSION && !ctx->params.do_emission) {  // sourcing.cpp:41-43
    for (int b = 0; b < M.nblocks; ++b) e_block_host[b] = 0.0;
    return JB_COMPLETE;
  }
  jb_status st = salloc_check_target(ctx, M);
  if (st != JB_COMPLETE) return st;
  st = ensure_scratch(ctx, (size_t)M.nblocks);
  if (st != JB_COMPLETE) return st;
  double *e_d = (double *)ctx->scratch_d;
  hipLaunchKernelGGL(k_salloc_energy, dim3(M.nblocks), dim3(kBlock), 0, ctx->stream, M, ctx->dp, source_type, dt, e_d);
  JB_HIP(hipGetLastError());
  JB_HIP(hipMemcpyAsync(e_block_host, e_d, sizeof(double) * M.nblocks, hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  mesh->salloc_sums_type = source_type;
  return JB_COMPLETE;
}

extern "C" jb_status jb_source_photons_count_energy(jb_context *ctx, jb_mesh *mesh, int source_type, double dt,
                                                    uint32_t epoch, double e_total, int32_t *nper_block_host,
                                                    int32_t *prefix_dev) {
  JB_RANGE("Jaybenne::SourcePhotons1");
  (void)dt;   // (the energies are those jb_source_energy_sums staged)
  if (!ctx || !mesh || !nper_block_host || !prefix_dev)
    return fail(JB_ERR_INVALID, "jb_source_photons_count_energy: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  if (ctx->params.source_strategy == JB_STRATEGY_ENERGY)
    return fail(JB_ERR_INVALID, "Energy source strategy not implemented!");  // sourcing.cpp:38
  if (ctx->source_allocation != JB_ALLOC_ENERGY)
    return fail(JB_ERR_INVALID, "jb_source_photons_count_energy: source allocation is not energy "
                "(jb_set_source_allocation)");
  if (epoch >= (1u << 20))  // cell_stream_id keeps the source-call counter in 20 bits
    return fail(JB_ERR_INVALID, "more than 2^20 source calls: the per-cell rounding streams would repeat");
  const DevMesh &M = mesh->dm;
  if (source_type == JB_SOURCE_EMISSION && !ctx->params.do_emission) {  // sourcing.cpp:41-43
    for (int b = 0; b < M.nblocks; ++b) nper_block_host[b] = 0;
    return JB_COMPLETE;
  }
  if (mesh->salloc_sums_type != source_type)
    return fail(JB_ERR_INVALID, "jb_source_photons_count_energy: no jb_source_energy_sums call of source type %d "
                "on this mesh since its last count", source_type);
  mesh->salloc_sums_type = -1;   // (the count overwrites the staged energies with the weights)
  const long long n_target = (long long)ctx->params.num_particles;
  jb_status st = salloc_check_target(ctx, M);
  if (st != JB_COMPLETE) return st;
  if (!std::isfinite(e_total) || e_total < 0.0)
    return fail(JB_ERR_INVALID, "source allocation energy: the total energy to source is %g", e_total);
  // E_tot = 0: nothing to source -- scale = 0 gives every cell nu = 0, no photon and weight 0
  const double scale = e_total > 0.0 ? (double)n_target / e_total : 0.0;
  if (!std::isfinite(scale))
    return fail(JB_ERR_INVALID, "source allocation energy: num_particles / E_tot = %lld / %g is not finite", n_target,
                e_total);
  st = ensure_scratch(ctx, (size_t)M.nblocks);
  if (st != JB_COMPLETE) return st;
  int *nper_d = (int *)ctx->scratch_d;
  hipLaunchKernelGGL(k_salloc_count, dim3(M.nblocks), dim3(kBlock), 0, ctx->stream, M, ctx->dp, scale, epoch, nper_d,
                     prefix_dev);
  JB_HIP(hipGetLastError());
  mesh->salloc_last = true;
  return source_count_finish(ctx, mesh, nper_d, nper_block_host);
}

// ------------------------------------------------------------------------------------------------
// The boundary source (jb_kernel_bsource.hpp): Planckian inflow through the domain faces that carry a temperature.
static bool bsource_on(const jb_context *ctx) {
  for (int f = 0; f < 6; ++f)
    if (ctx->bs_temp[f] > 0.0) return true;
  return false;
}

extern "C" jb_status jb_set_boundary_source(jb_context *ctx, int face, double temperature) {
  if (!ctx) return fail(JB_ERR_INVALID, "jb_set_boundary_source: null context");
  if (face < 0 || face > 5) return fail(JB_ERR_INVALID, "jb_set_boundary_source: face %d outside 0..5", face);
  if (!(temperature >= 0.0) || !std::isfinite(temperature))
    return fail(JB_ERR_INVALID, "jb_set_boundary_source: the temperature of face %d must be finite and >= 0", face);
  ctx->bs_temp[face] = temperature;
  return JB_COMPLETE;
}

extern "C" jb_status jb_get_boundary_source(const jb_context *ctx, int face, double *temperature) {
  if (!ctx || !temperature) return fail(JB_ERR_INVALID, "jb_get_boundary_source: null argument");
  if (face < 0 || face > 5) return fail(JB_ERR_INVALID, "jb_get_boundary_source: face %d outside 0..5", face);
  *temperature = ctx->bs_temp[face];
  return JB_COMPLETE;
}

extern "C" int jb_boundary_source_enabled(const jb_context *ctx) { return ctx && bsource_on(ctx) ? 1 : 0; }

extern "C" jb_status jb_set_boundary_source_count(jb_context *ctx, int64_t num_particles, int64_t face_cells_total) {
  if (!ctx) return fail(JB_ERR_INVALID, "jb_set_boundary_source_count: null context");
  if (num_particles < 0 || face_cells_total < 0)
    return fail(JB_ERR_INVALID, "jb_set_boundary_source_count: negative count");
  ctx->bs_num_particles = num_particles;
  ctx->bs_face_cells_total = face_cells_total;
  return JB_COMPLETE;
}

extern "C" int64_t jb_boundary_prefix_words(const jb_mesh *mesh) {
  if (!mesh) return 0;
  const DevMesh &M = mesh->dm;
  return (int64_t)M.nblocks * (bsource_layout(M.nx, M.ncell).off[6] + 1);
}

extern "C" int64_t jb_boundary_face_cells(const jb_context *ctx, const jb_mesh *mesh) {
  if (!ctx || !mesh) return 0;
  const DevMesh &M = mesh->dm;
  int64_t cells = 0;
  for (int b = 0; b < M.nblocks; ++b)
    for (int f = 0; f < 6; ++f)
      if (ctx->bs_temp[f] > 0.0 && mesh->bface_host[6 * (size_t)b + f]) cells += M.ncell / M.nx[f >> 1];
  return cells;
}

extern "C" jb_status jb_boundary_source_last(const jb_context *ctx, jb_boundary_source_record *out) {
  if (!ctx || !out) return fail(JB_ERR_INVALID, "jb_boundary_source_last: null argument");
  *out = ctx->bs_last;
  return JB_COMPLETE;
}

// the (block, face) results of the count kernel: [nblocks] int | pad to 8 | [nblocks][6] long long | [nblocks][6] double
static size_t bsource_out_counts(size_t nblocks) { return (nblocks * sizeof(int) + 7) / 8 * 8; }

extern "C" jb_status jb_source_boundary_count(jb_context *ctx, jb_mesh *mesh, double dt, int64_t face_cells_total,
                                              int64_t num_particles, uint32_t epoch,
                                              jb_boundary_source_plan *plan_out, int32_t *prefix_dev) {
  JB_RANGE("Jaybenne::SourceBoundaryPhotons1");
  if (!ctx || !mesh || !plan_out || !plan_out->nper_block)
    return fail(JB_ERR_INVALID, "jb_source_boundary_count: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  const DevMesh &M = mesh->dm;
  for (int b = 0; b < M.nblocks; ++b) plan_out->nper_block[b] = 0;
  for (int f = 0; f < 6; ++f) { plan_out->e_face[f] = 0.0; plan_out->n_face[f] = 0; }
  for (int f = 0; f < 6; ++f) { ctx->bs_last.e_face[f] = 0.0; ctx->bs_last.n_face[f] = 0; }
  if (!bsource_on(ctx)) return JB_COMPLETE;   // every face off: no kernel
  for (int f = 0; f < 6; ++f) {
    if (!(ctx->bs_temp[f] > 0.0)) continue;
    if (f >= 2 * M.ndim)
      return fail(JB_ERR_INVALID, "boundary source on face %d: axis %d is not active on a %d-D mesh", f, f >> 1, M.ndim);
    if (M.bc[f] == BC_PERIODIC)
      return fail(JB_ERR_INVALID, "boundary source on face %d: its swarm boundary is periodic", f);
  }
  if (!prefix_dev) {   // the library's own workspace
    const jb_status pst = dev_grow(ctx->bs_prefix, (size_t)jb_boundary_prefix_words(mesh) * sizeof(int),
                                   "hipMalloc of the boundary source's prefix workspace");
    if (pst != JB_COMPLETE) return pst;
    prefix_dev = (int32_t *)ctx->bs_prefix.p;
  }
  if (epoch >= (1u << 20))  // cell_stream_id keeps the source-call counter in 20 bits
    return fail(JB_ERR_INVALID, "more than 2^20 source calls: the per-cell rounding streams would repeat");
  if (face_cells_total < 1) return fail(JB_ERR_INVALID, "boundary source: no source face cells (face_cells_total < 1)");
  const double npc = (double)num_particles / (double)face_cells_total;
  if (!(npc >= 1.0))
    return fail(JB_ERR_INVALID, "boundary source: %lld photons for %lld source face cells -- fewer than one per cell",
                (long long)num_particles, (long long)face_cells_total);
  if (!(npc < 2.0e9)) return fail(JB_ERR_INVALID, "boundary source: more than 2e9 photons per source face cell");
  const size_t nb = (size_t)M.nblocks;
  const jb_status ost = dev_grow(ctx->bs_out, bsource_out_counts(nb) + nb * 6 * 16, "hipMalloc of the boundary source's counts");
  if (ost != JB_COMPLETE) return ost;
  int *nper_d = (int *)ctx->bs_out.p;
  long long *n_bf_d = (long long *)((char *)ctx->bs_out.p + bsource_out_counts(nb));
  double *e_bf_d = (double *)(n_bf_d + 6 * nb);
  BsFaces F;
  for (int f = 0; f < 6; ++f) F.temp[f] = ctx->bs_temp[f];
  const BsLayout L = bsource_layout(M.nx, M.ncell);
  hipLaunchKernelGGL(k_bsource_count, dim3(M.nblocks), dim3(kBlock), 0, ctx->stream, M, ctx->dp, F, L, dt, npc, epoch,
                     nper_d, (int *)prefix_dev, n_bf_d, e_bf_d);
  JB_HIP(hipGetLastError());
  ctx->bs_last.kernel_launches += 1;
  std::vector<char> host(bsource_out_counts(nb) + nb * 6 * 16);
  JB_HIP(hipMemcpyAsync(host.data(), ctx->bs_out.p, host.size(), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  const int *nper_h = (const int *)host.data();
  const long long *n_bf = (const long long *)(host.data() + bsource_out_counts(nb));
  const double *e_bf = (const double *)(n_bf + 6 * nb);
  for (size_t b = 0; b < nb; ++b) {   // (blocks in resident order: a fixed order of additions)
    plan_out->nper_block[b] = nper_h[b];
    for (int f = 0; f < 6; ++f) {
      plan_out->e_face[f] += e_bf[6 * b + f];
      plan_out->n_face[f] += n_bf[6 * b + f];
    }
  }
  for (int f = 0; f < 6; ++f) { ctx->bs_last.e_face[f] = plan_out->e_face[f]; ctx->bs_last.n_face[f] = plan_out->n_face[f]; }
  return JB_COMPLETE;
}

extern "C" jb_status jb_source_boundary_fill(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                             double t_start, double dt, const int32_t *nper_block_host,
                                             const int32_t *prefix_dev, const int64_t *slot_base_host,
                                             const uint64_t *id_base_host) {
  JB_RANGE("Jaybenne::SourceBoundaryPhotons2");
  if (!ctx || !mesh || !nper_block_host || !slot_base_host || !id_base_host)
    return fail(JB_ERR_INVALID, "jb_source_boundary_fill: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_source_boundary_fill");
  if (st != JB_COMPLETE) return st;
  if (!bsource_on(ctx)) return JB_COMPLETE;
  if (!prefix_dev) prefix_dev = (int32_t *)ctx->bs_prefix.p;   // the library's own workspace, as the count call filled it
  if (!prefix_dev) return fail(JB_ERR_INVALID, "jb_source_boundary_fill: no count call has filled the prefix workspace");
  const DevMesh &M = mesh->dm;
  st = ensure_scratch(ctx, (size_t)M.nblocks * 3 + 8);
  if (st != JB_COMPLETE) return st;
  const int32_t *nper = nper_block_host;
  std::vector<long long> tab(3 * (size_t)M.nblocks);
  long long total = 0;
  for (int b = 0; b < M.nblocks; ++b) {
    tab[b] = total;                                   // blk_first
    tab[M.nblocks + b] = slot_base_host[b];           // slot_base
    tab[2 * M.nblocks + b] = (long long)id_base_host[b];
    if (nper[b] < 0) return fail(JB_ERR_INVALID, "negative particle count for block %d", b);
    if (nper[b] > 0 && (slot_base_host[b] < 0 || slot_base_host[b] + nper[b] > swarm->capacity))
      return fail(JB_ERR_CAPACITY, "swarm capacity %lld too small for block %d (slots %lld..%lld)",
                  (long long)swarm->capacity, b, (long long)slot_base_host[b],
                  (long long)slot_base_host[b] + nper[b]);
    total += nper[b];
  }
  if (total == 0) return JB_COMPLETE;
  long long *tab_d = ctx->scratch_d;
  JB_HIP(hipMemcpyAsync(tab_d, tab.data(), sizeof(long long) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
  BsFaces F;
  for (int f = 0; f < 6; ++f) F.temp[f] = ctx->bs_temp[f];
  const BsLayout L = bsource_layout(M.nx, M.ncell);
  hipLaunchKernelGGL(k_bsource_fill, dim3(grid_for(ctx, total)), dim3(kBlock), 0, ctx->stream, M, ctx->dp,
                     dev_swarm(swarm), F, L, t_start, dt, (const int *)prefix_dev, (const long long *)tab_d,
                     (const long long *)(tab_d + M.nblocks), (const unsigned long long *)(tab_d + 2 * M.nblocks), total);
  JB_HIP(hipGetLastError());
  ctx->bs_last.kernel_launches += 1;
#ifdef JB_INVARIANTS
  {  // (checked build) SWARM over the slots just filled
    long long lo = swarm->capacity, hi = 0;
    for (int b = 0; b < M.nblocks; ++b)
      if (nper[b] > 0) {
        lo = slot_base_host[b] < lo ? slot_base_host[b] : lo;
        hi = slot_base_host[b] + nper[b] > hi ? slot_base_host[b] + nper[b] : hi;
      }
    st = inv_sweep(ctx, M, dev_swarm(swarm), lo, hi, t_start + dt, true);
    if (st != JB_COMPLETE) return st;
  }
#endif
  JB_HIP(hipStreamSynchronize(ctx->stream));  // tab lives on this stack frame
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
// Transport.  WHICH tracking kernel a call runs is decided in one place, select_transport (jb_select.hpp);
// what follows turns its plan into launches.

// A runtime value as a template argument: f(std::integral_constant) for the one of the listed values that v has.
template <int... Vs, class F>
static void with_int(int v, F &&f) {
  (void)((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}
template <class F>
static void with_bool(bool v, F &&f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}
template <auto Kernel>
using kernel_c = std::integral_constant<decltype(Kernel), Kernel>;

// The tracking kernels are persistent (waves draw particles from queues until they are empty), so the grid
// is exactly what the chip holds at once: more workgroups would only start when the queues
// are already drained.  JB_TRANSPORT_BLOCKS_PER_CU overrides the occupancy query (tuning aid);
// JB_TRANSPORT_MAX_BLOCKS caps the grid behind every policy (tests: a few workgroups follow the whole swarm, so
// every lane is refilled many times; placement only affects speed, never results).
enum class Occupancy {
  cached,           // one query per kernel instantiation and process (the kernels without dynamic LDS)
  per_launch,       // the dynamic LDS -- tally and record table of a small mesh -- changes with the mesh: ask per launch
  per_launch_cap3,  // ... and take at most 3 (TransportPlan::occ_cap3)
  one_per_queue,    // no query: kQueues workgroups (the handful of photons k_ddmc_all hands over)
};
template <auto Kernel, class... Args>
static void launch_persistent(jb_context *ctx, long long n, size_t dyn_lds, Occupancy policy, const Args &...args) {
  int g = kQueues;
  if (policy != Occupancy::one_per_queue) {
    static int cached = 0;
    int occ = policy == Occupancy::cached ? cached : 0;
    if (occ < 1) {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, Kernel, kBlock, dyn_lds) != hipSuccess || occ < 1) occ = 3;
      if (policy == Occupancy::cached) cached = occ;
    }
    if (policy == Occupancy::per_launch_cap3 && occ > 3) occ = 3;
    g = grid_for(ctx, n, ctx->blocks_per_cu_env > 0 ? ctx->blocks_per_cu_env : occ);
  }
  if (ctx->max_blocks_env > 0 && g > ctx->max_blocks_env) g = ctx->max_blocks_env;
  if (g > ctx->grid_max) ctx->grid_max = g;
  hipLaunchKernelGGL(Kernel, dim3(g), dim3(kBlock), dyn_lds, ctx->stream, args...);
}

// The dispatch functions below list the instantiations that exist, no others: every further one is a kernel
// to compile.

// k_transport<NDIM, DDMC, TALLY, GRAY, EXACT, LEAN>: EXACT and LEAN are variants of the gray IMC kernels
template <int NDIM>
static void launch_k_transport(jb_context *ctx, const jb_mesh *mesh, const TransportPlan &p, const DevSwarm &S,
                               double t_start, double dt, long long first, long long last) {
  with_bool(p.tally, [&](auto tc) {
    with_int<0, 1, 2>(p.gray, [&](auto gc) {
      constexpr bool T = decltype(tc)::value;
      constexpr int G = decltype(gc)::value;
      const auto go = [&](auto dc, auto xc, auto lc) {
        launch_persistent<k_transport<NDIM, decltype(dc)::value, T, G, decltype(xc)::value, decltype(lc)::value>>(
            ctx, last - first, 0, Occupancy::cached, track_dm(mesh), ctx->dp, S, t_start, dt, first, last,
            ctx->counters_d, (const int *)nullptr);
      };
      if constexpr (G != 0) {
        if (!p.ddmc) {
          with_bool(p.exact, [&](auto xc) { with_bool(p.lean, [&](auto lc) { go(std::false_type{}, xc, lc); }); });
          return;
        }
      }
      with_bool(p.ddmc, [&](auto dc) { go(dc, std::false_type{}, std::false_type{}); });
    });
  });
}

// k_imc_cell<NDIM, TALLY, NOABS, UNIFORM>, or k_imc_cell_unit<NDIM, TALLY, NOABS, EQUALH> where the plan says unit_cell
// (in 1-D there is one active width: always EQUALH)
template <int NDIM>
static void launch_k_imc_cell(jb_context *ctx, const jb_mesh *mesh, const TransportPlan &p, const DevSwarm &S,
                              double t_start, double dt, long long first, long long last) {
  with_bool(p.tally, [&](auto tc) {
    with_bool(p.noabs, [&](auto nc) {
      constexpr bool T = decltype(tc)::value, NA = decltype(nc)::value;
      const auto go = [&](auto kc) {
        launch_persistent<decltype(kc)::value>(ctx, last - first, 0, Occupancy::cached, track_dm_dev(mesh), ctx->dp, S,
                                               t_start, dt, first, last, ctx->counters_d, mesh->nbr_dq);
      };
      if (!p.uniform) return go(kernel_c<k_imc_cell<NDIM, T, NA, false>>{});
      if constexpr (kUnitCellForm) {
        if (p.unit_cell && (p.equal_h || NDIM == 1)) return go(kernel_c<k_imc_cell_unit<NDIM, T, NA, true>>{});
        if constexpr (NDIM > 1) {
          if (p.unit_cell) return go(kernel_c<k_imc_cell_unit<NDIM, T, NA, false>>{});
        }
      }
      go(kernel_c<k_imc_cell<NDIM, T, NA, true>>{});
    });
  });
}

// the heads of the launch's particle queues (jb_scaffold.hpp: QueueCursor) back to zero, in stream order in front of
// every persistent tracking launch
static void clear_queue_heads(jb_context *ctx) {
  (void)hipMemsetAsync(ctx->counters_d + CNT_QUEUE, 0, kQueues * kQueueStride * sizeof(unsigned long long), ctx->stream);
}

// k_hybrid<NDIM, TALLY, NOABS, MODE, PHASE> on entries [f, l) of list_in (nullptr: slots of the swarm), with the
// queue heads cleared in front of it; PHASE 2 exists as <.., true, 0, 2> only (hybrid_phase)
template <int NDIM>
static void launch_k_hybrid(jb_context *ctx, const jb_mesh *mesh, const TransportPlan &p, int phase, Occupancy policy,
                            const DevSwarm &S, double t_start, double dt, long long f, long long l,
                            const unsigned *list_in, unsigned *list_out, unsigned long long *count_out,
                            const unsigned long long *count_in) {
  clear_queue_heads(ctx);
  const HybridPhase h = hybrid_phase(p, phase);
  with_bool(p.tally, [&](auto tc) {
    with_bool(h.noabs, [&](auto nc) {
      with_int<0, 1, 2, 3>(h.mode, [&](auto mc) {
        constexpr bool T = decltype(tc)::value, NA = decltype(nc)::value;
        constexpr int MD = decltype(mc)::value;
        const auto go = [&](auto kc) {
          launch_persistent<decltype(kc)::value>(ctx, l - f, 0, policy, track_dm_dev(mesh), ctx->dp, S, t_start, dt, f, l,
                                                 ctx->counters_d, list_in, list_out, count_out, count_in);
        };
        if constexpr (NA && MD == 0) {
          if (phase == 2) return go(kernel_c<k_hybrid<NDIM, T, true, 0, 2>>{});
        }
        if (phase == 1) go(kernel_c<k_hybrid<NDIM, T, NA, MD, 1>>{});
        else go(kernel_c<k_hybrid<NDIM, T, NA, MD, 0>>{});
      });
    });
  });
}

// Every cell takes DDMC steps: k_ddmc_all<NDIM, TALLY, GATHER> or k_ddmc_q<NDIM, TALLY, LCODES>.
// A particle that sits at a face of its cell when it is loaded or relocated (one in ~1e8) needs
// the albedo step: the kernel lists it, and k_hybrid<.., both loops>, launched behind it on
// that list (its length read on the device: no synchronisation), tracks it to the end.
template <int NDIM>
static jb_status launch_all_ddmc(jb_context *ctx, const jb_mesh *mesh, const TransportPlan &p, const DevSwarm &S,
                                 double t_start, double dt, long long first, long long last) {
  const jb_status st = ensure_scratch(ctx, (size_t)(last - first) / 2 + 16);
  if (st != JB_COMPLETE) return st;
  unsigned *handed = (unsigned *)ctx->scratch_d;
  unsigned long long *n_handed = ctx->counters_d + kCursorBase;
  (void)hipMemsetAsync(n_handed, 0, sizeof(unsigned long long), ctx->stream);
  with_bool(p.tally, [&](auto tc) {
    constexpr bool T = decltype(tc)::value;
    const auto go = [&](auto kc) {
      launch_persistent<decltype(kc)::value>(ctx, last - first, p.dyn_lds,
                                             p.occ_cap3 ? Occupancy::per_launch_cap3 : Occupancy::per_launch,
                                             track_dm_dev(mesh), ctx->dp, S, t_start, dt, first, last, ctx->counters_d,
                                             (const int *)mesh->dm.not_all_ddmc, handed, n_handed);
    };
    if (p.family == Family::k_ddmc_q)
      with_bool(p.lcodes, [&](auto lc) { go(kernel_c<k_ddmc_q<NDIM, T, decltype(lc)::value>>{}); });
    else
      with_int<0, 1, 2, 3, 4>(p.gather, [&](auto gc) { go(kernel_c<k_ddmc_all<NDIM, T, decltype(gc)::value>>{}); });
  });
  launch_k_hybrid<NDIM>(ctx, mesh, p, 0, Occupancy::one_per_queue, S, t_start, dt, 0ll, last - first, handed,
                        nullptr, nullptr, n_handed);
  return JB_COMPLETE;
}

// A mix of IMC and DDMC cells: the three launches of k_hybrid (select_transport says why three).  The lists of
// parked photons (slot numbers, 4 bytes each) live in the context's scratch buffer.
template <int NDIM>
static jb_status launch_mixed(jb_context *ctx, const jb_mesh *mesh, const TransportPlan &p, const DevSwarm &S,
                              double t_start, double dt, long long first, long long last) {
  const long long nrange = last - first;
  const jb_status st = ensure_scratch(ctx, (size_t)nrange + 16);  // 2 lists x 4 bytes x n
  if (st != JB_COMPLETE) return st;
  unsigned *list_d = (unsigned *)ctx->scratch_d;          // parked by phase 1, read by phase 2
  unsigned *list_i = list_d + nrange;                     // parked by phase 2, read by phase 0
  unsigned long long *cnt = ctx->counters_d + kCursorBase;  // [0] |list_d|, [1] |list_i|
  volatile unsigned long long *cnt_h = ctx->counters_h + kCursorBase;
  const auto launch = [&](int phase, long long f, long long l, const unsigned *lin, unsigned *lout,
                          unsigned long long *cout) {
    launch_k_hybrid<NDIM>(ctx, mesh, p, phase, Occupancy::cached, S, t_start, dt, f, l, lin, lout, cout, nullptr);
  };
  (void)hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned long long), ctx->stream);
  launch(1, first, last, nullptr, list_d, cnt);
  (void)hipMemcpyAsync((void *)cnt_h, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  const long long n_d = (long long)cnt_h[0];
  if (n_d == 0) return JB_COMPLETE;
  launch(2, 0, n_d, list_d, list_i, cnt + 1);
  (void)hipMemcpyAsync((void *)(cnt_h + 1), cnt + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  const long long n_i = (long long)cnt_h[1];
  if (n_i == 0) return JB_COMPLETE;
  launch(0, 0, n_i, list_i, nullptr, nullptr);
  return JB_COMPLETE;
}

template <int NDIM>
static jb_status launch_transport(jb_context *ctx, jb_mesh *mesh, const DevSwarm &S, double t_start, double dt,
                                  long long first, long long last, bool tally, bool ddmc) {
  const DevMesh &M = mesh->dm;
  const bool gray = M.lam_abs != nullptr;
  clear_queue_heads(ctx);
  // (the one input the device holds: whether every cell takes DDMC steps, and the number of distinct step
  // records, as UpdateDerivedTransportFields left them)
  if (ddmc && gray && M.ddmc_cell && M.nblocks <= kLdsBlocks && mesh->not_all_ddmc_host < 0) {
    int *flag_h = (int *)(ctx->counters_h + kCounterWords - 1);
    flag_h[0] = 1; flag_h[1] = 0;
    (void)hipMemcpyAsync(flag_h, M.not_all_ddmc, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    JB_HIP(hipStreamSynchronize(ctx->stream));
    mesh->not_all_ddmc_host = flag_h[0] != 0 ? 1 : 0;
    mesh->nclass_host = flag_h[1];
  }
  TransportInputs in;
  in.ndim = NDIM;
  in.ddmc = ddmc;
  in.tally = tally;
  in.gray = gray;
  in.has_ddmc_cell = M.ddmc_cell != nullptr;
  in.has_ddmc_code = M.ddmc_code != nullptr;
  in.nblocks = M.nblocks;
  in.ntot = M.ntot;
  in.last = last;
  in.not_all_ddmc = mesh->not_all_ddmc_host != 0;
  in.nclass = mesh->nclass_host;
  in.noabs = ctx->dp.kappa_a == 0.0;
  in.exact_geom = mesh->exact_geom;
  in.cell_ok = mesh->cell_ok;
  in.uniform_geom = mesh->uniform_geom;
  in.equal_h = mesh->equal_h;
  in.unit_cell_form = kUnitCellForm;
  in.lean_arith = ctx->lean_arith;
  in.no_imc_cell = ctx->no_imc_cell;
  in.coop_gather = ctx->coop_gather;
  in.ddmc_queues = ctx->ddmc_queues != 0;
  in.ddmc_lds_codes = ctx->ddmc_lds_codes != 0;
  in.max_classes = ctx->max_classes;
  const TransportPlan plan = select_transport(in);
  variant_name(plan, mesh->last_variant, sizeof mesh->last_variant);
  mesh->last_unit_cell = plan.unit_cell ? (plan.equal_h ? 2 : 1) : 0;
  switch (plan.family) {
  case Family::k_transport: launch_k_transport<NDIM>(ctx, mesh, plan, S, t_start, dt, first, last); break;
  case Family::k_imc_cell: launch_k_imc_cell<NDIM>(ctx, mesh, plan, S, t_start, dt, first, last); break;
  case Family::k_ddmc_all:
  case Family::k_ddmc_q: return launch_all_ddmc<NDIM>(ctx, mesh, plan, S, t_start, dt, first, last);
  case Family::k_hybrid: return launch_mixed<NDIM>(ctx, mesh, plan, S, t_start, dt, first, last);
  }
  return JB_COMPLETE;
}

static jb_status transport_impl(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                double t_start, double dt, int64_t first, int64_t last, int tally,
                                bool ddmc) {
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_transport_photons");
  if (st != JB_COMPLETE) return st;
  if (first < 0 || last > swarm->n || first > last)
    return fail(JB_ERR_INVALID, "particle range [%lld,%lld) outside the swarm (n = %lld)",
                (long long)first, (long long)last, (long long)swarm->n);
  const DevMesh &M = mesh->dm;
  if (ddmc && (!M.P1 || (M.ndim > 1 && !M.P2) || (M.ndim > 2 && !M.P3)))
    return fail(JB_ERR_INVALID, "DDMC transport needs the ddmc_face_prob arrays");
  // (exact deposition: the tracking kernels deposit into the decoy field, the plan is made without the tally; the
  // decoy view exists from the first call in this mode on, whatever its range)
  const bool exact_dep = ctx->deposition == JB_DEPOSIT_EXACT;
  if (exact_dep && (st = deposit_ensure(ctx, mesh)) != JB_COMPLETE) return st;
  if (first == last) return JB_COMPLETE;
  const DevSwarm S = dev_swarm(swarm);
  const bool tl = tally != 0 && !exact_dep;
#ifdef JB_INVARIANTS
  st = inv_sweep(ctx, M, S, first, last, t_start + dt, false);   // (checked build) SWARM on entry (k_inv_swarm)
  if (st != JB_COMPLETE) return st;
#endif
  // (jb_defrag_policy: the time of the tracking kernels of this cycle, per event)
  hipEvent_t ev_stop = nullptr;
  if (ctx->tev_used + 2 <= 2 * kTransportEventPairs) {
    while ((int)ctx->tev.size() < ctx->tev_used + 2) {
      hipEvent_t e = nullptr;
      JB_HIP(hipEventCreate(&e));
      ctx->tev.push_back(e);
    }
    JB_HIP(hipEventRecord(ctx->tev[ctx->tev_used], ctx->stream));
    ev_stop = ctx->tev[ctx->tev_used + 1];
    ctx->tev_used += 2;
  } else {
    ctx->tev_overflow = true;
  }
  ctx->grid_max = 0;
  with_int<1, 2, 3>(M.ndim, [&](auto nd) {
    st = launch_transport<decltype(nd)::value>(ctx, mesh, S, t_start, dt, first, last, tl, ddmc);
  });
  mesh->last_grid = ctx->grid_max;
  if (ev_stop) (void)hipEventRecord(ev_stop, ctx->stream);
  if (st != JB_COMPLETE) return st;
  JB_HIP(hipGetLastError());
  // (exact deposition: exactly the range this call followed, before any pack turns packed slots into holes)
  if (exact_dep) return deposit_sweep(ctx, mesh, swarm, first, last, DEP_ABSORBED);
  return JB_COMPLETE;
}

extern "C" jb_status jb_transport_photons(jb_context *ctx, jb_mesh *mesh,
                                          const jb_swarm_view *swarm, double t_start, double dt,
                                          int64_t first, int64_t last, int fuse_census_tally) {
  JB_RANGE("Jaybenne::TransportPhotons");
  return transport_impl(ctx, mesh, swarm, t_start, dt, first, last, fuse_census_tally, false);
}
extern "C" jb_status jb_transport_photons_ddmc(jb_context *ctx, jb_mesh *mesh,
                                               const jb_swarm_view *swarm, double t_start, double dt,
                                               int64_t first, int64_t last, int fuse_census_tally) {
  JB_RANGE("Jaybenne::TransportPhotons_DDMC");
  return transport_impl(ctx, mesh, swarm, t_start, dt, first, last, fuse_census_tally, true);
}

extern "C" jb_status jb_verify_swarm(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, double t_start,
                                     double t_end, jb_invariant_report *report) {
#ifdef JB_INVARIANTS
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "jb_verify_swarm: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_verify_swarm");
  if (st != JB_COMPLETE) return st;
  if (!(t_start <= t_end)) return fail(JB_ERR_INVALID, "jb_verify_swarm: t_start > t_end");
  jb_invariant_report before, after;
  if ((st = inv_read(ctx, &before)) != JB_COMPLETE) return st;
  if ((st = inv_sweep(ctx, mesh->dm, dev_swarm(swarm), 0, swarm->n, t_end, true)) != JB_COMPLETE) return st;
  if ((st = inv_read(ctx, &after)) != JB_COMPLETE) return st;
  jb_invariant_report d = after;   // this sweep's counts; its first violation if the claim was free before it
  for (int k = 0; k < JB_INV_NKINDS; ++k) {
    d.evaluated[k] -= before.evaluated[k];
    d.violated[k] -= before.violated[k];
  }
  for (int f = 0; f < JB_INV_NFAMILIES; ++f) d.passes[f] -= before.passes[f];
  if (before.has_first) d.has_first = 0;
  if (report) *report = d;
  const int64_t n_new = inv_total(d);
  return n_new > 0 ? inv_fail(ctx, n_new, "jb_verify_swarm") : JB_COMPLETE;
#else
  (void)ctx; (void)mesh; (void)swarm; (void)t_start; (void)t_end; (void)report;
  return fail(JB_ERR_UNSUPPORTED, "jb_verify_swarm: this is the release library; the transport invariants are "
              "checked by libjaybenne_amd_checked.so (make -C jaybenne_amd/csrc checked)");
#endif
}

extern "C" const char *jb_last_transport_variant(const jb_mesh *mesh) {
  return mesh ? mesh->last_variant : "";
}
extern "C" int jb_last_transport_grid(const jb_mesh *mesh) { return mesh ? mesh->last_grid : 0; }
extern "C" int jb_last_transport_unit_cell(const jb_mesh *mesh) { return mesh ? mesh->last_unit_cell : 0; }
extern "C" int jb_mesh_exact_geometry(const jb_mesh *mesh) { return mesh && mesh->exact_geom; }
extern "C" int jb_mesh_ddmc_classes(const jb_mesh *mesh) { return mesh ? mesh->nclass_host : 0; }
extern "C" jb_status jb_set_arithmetic(jb_context *ctx, int mode) {
  if (!ctx || (mode != JB_ARITH_EXACT && mode != JB_ARITH_LEAN)) return fail(JB_ERR_INVALID, "bad argument");
  ctx->lean_arith = mode == JB_ARITH_LEAN;
  ctx->dp.lean = ctx->lean_arith ? 1 : 0;
  return JB_COMPLETE;
}
extern "C" int jb_get_arithmetic(const jb_context *ctx) {
  return ctx && ctx->lean_arith ? JB_ARITH_LEAN : JB_ARITH_EXACT;
}
extern "C" jb_status jb_set_cell_order(jb_context *ctx, int mode) {
  if (!ctx || (mode != JB_CELL_ORDER_ANY && mode != JB_CELL_ORDER_BY_ID))
    return fail(JB_ERR_INVALID, "jb_set_cell_order: mode = %d is neither JB_CELL_ORDER_ANY nor JB_CELL_ORDER_BY_ID", mode);
  if (mode != ctx->cell_order) ctx->comb.valid = ctx->weigh.valid = false;   // (the comb's arrays lie behind the sort's: a plan made before is none now)
  ctx->cell_order = mode;
  return JB_COMPLETE;
}
extern "C" int jb_get_cell_order(const jb_context *ctx) {
  return ctx && ctx->cell_order == JB_CELL_ORDER_BY_ID ? JB_CELL_ORDER_BY_ID : JB_CELL_ORDER_ANY;
}

extern "C" jb_status jb_set_deposition(jb_context *ctx, int mode) {
  if (!ctx || (mode != JB_DEPOSIT_ATOMIC && mode != JB_DEPOSIT_EXACT))
    return fail(JB_ERR_INVALID, "jb_set_deposition: mode = %d is neither JB_DEPOSIT_ATOMIC nor JB_DEPOSIT_EXACT", mode);
  if (mode != ctx->deposition && !ctx->dep_open_meshes.empty())
    return fail(JB_ERR_INVALID, "jb_set_deposition: accumulators are open (jb_deposit_close first)");
  if (mode != ctx->deposition) ctx->dep_has_last = false;
  ctx->deposition = mode;
  return JB_COMPLETE;
}
extern "C" int jb_get_deposition(const jb_context *ctx) {
  return ctx && ctx->deposition == JB_DEPOSIT_EXACT ? JB_DEPOSIT_EXACT : JB_DEPOSIT_ATOMIC;
}

static jb_status fetch_counters(jb_context *ctx) {
  JB_HIP(hipMemcpyAsync(ctx->counters_h, ctx->counters_d, sizeof(unsigned long long) * kRankBase,
                        hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  return JB_COMPLETE;
}

extern "C" jb_status jb_get_transport_stats(jb_context *ctx, jb_transport_stats *stats, int reset) {
  if (!ctx || !stats) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = fetch_counters(ctx);
  if (st != JB_COMPLETE) return st;
  stats->n_census = (int64_t)ctx->counters_h[CNT_CENSUS];
  stats->n_absorbed = (int64_t)ctx->counters_h[CNT_ABSORBED];
  stats->n_escaped = (int64_t)ctx->counters_h[CNT_ESCAPED];
  stats->n_outgoing = (int64_t)ctx->counters_h[CNT_OUTGOING];
  stats->n_events = (int64_t)ctx->counters_h[CNT_EVENTS];
  stats->n_wave_passes = (int64_t)ctx->counters_h[CNT_PASSES];
  stats->n_wave_services = (int64_t)ctx->counters_h[CNT_SERVICE];
#ifdef JB_TIMING  // (diagnostic build: wave-cycles / 1024 per sub-phase of k_ddmc_all's service phase)
  fprintf(stderr, "JB_TIMING phases reloc %llu claim %llu done %llu take %llu real %llu | episodes %llu passes %llu services %llu\n",
          ctx->counters_h[24], ctx->counters_h[25], ctx->counters_h[26], ctx->counters_h[27],
          ctx->counters_h[28], ctx->counters_h[29], ctx->counters_h[30], ctx->counters_h[31]);
#ifdef JB_TIMING_LOOP
  fprintf(stderr, "JB_TIMING_LOOP top %llu code wait %llu step %llu retire+tail %llu\n", ctx->counters_h[20],
          ctx->counters_h[21], ctx->counters_h[22], ctx->counters_h[23]);
#endif
#endif
#ifdef JB_HYB_STATS  // (diagnostic build of k_hybrid: see jb_kernel_hybrid.hpp)
  {
    unsigned long long h[48];
    (void)hipMemcpy(h, ctx->counters_d + 64, sizeof h, hipMemcpyDeviceToHost);
    const char *nm[9] = {"idle", "imc", "virt", "real", "done", "reloc", "emerge", "new", "park"};
    for (int ph = 0; ph < 3; ++ph) {
      fprintf(stderr, "JB_HYB_STATS phase %d: services %llu imc passes %llu (lanes %llu) ddmc passes %llu | lanes at service:", ph,
              h[16 * ph + 12], h[16 * ph + 9], h[16 * ph + 11], h[16 * ph + 10]);
      for (int k = 0; k < 9; ++k) fprintf(stderr, " %s %llu", nm[k], h[16 * ph + k]);
      fprintf(stderr, "\n");
    }
  }
#endif
  if (reset) JB_HIP(hipMemsetAsync(ctx->counters_d, 0, sizeof(unsigned long long) * CNT_N, ctx->stream));
  return JB_COMPLETE;
}

extern "C" jb_status jb_sample_ddmc_block_face(jb_context *ctx, jb_mesh *mesh,
                                               const jb_swarm_view *swarm, int64_t first,
                                               int64_t last) {
  JB_RANGE("Jaybenne::SampleDDMCBlockFace");
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_sample_ddmc_block_face");
  if (st != JB_COMPLETE) return st;
  const DevMesh &M = mesh->dm;
  if (!(M.ndim > 1)) return JB_COMPLETE;  // sample_ddmc_bface.cpp:90
  if (first < 0 || last > swarm->n || first > last) return fail(JB_ERR_INVALID, "bad particle range");
  if (!M.P1 || !M.P2 || (M.ndim > 2 && !M.P3)) return fail(JB_ERR_INVALID, "needs ddmc_face_prob");
  if (first == last) return JB_COMPLETE;
  const int g = grid_for(ctx, last - first);
  if (M.ndim == 2)
    hipLaunchKernelGGL(k_block_face<2>, dim3(g), dim3(kBlock), 0, ctx->stream, M, ctx->dp, dev_swarm(swarm), first, last);
  else
    hipLaunchKernelGGL(k_block_face<3>, dim3(g), dim3(kBlock), 0, ctx->stream, M, ctx->dp, dev_swarm(swarm), first, last);
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

extern "C" jb_status jb_check_completion(jb_context *ctx, const jb_swarm_view *swarm, double t_end,
                                         int64_t *unfinished) {
  JB_RANGE("Jaybenne::CheckCompletion");
  if (!ctx || !unfinished) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_check_completion");
  if (st != JB_COMPLETE) return st;
  JB_HIP(hipMemsetAsync(&ctx->counters_d[CNT_UNFINISHED], 0, sizeof(unsigned long long), ctx->stream));
  if (swarm->n > 0)
    hipLaunchKernelGGL(k_check_completion, dim3(grid_for(ctx, swarm->n)), dim3(kBlock), 0, ctx->stream,
                       dev_swarm(swarm), (long long)swarm->n, t_end, ctx->counters_d);
  JB_HIP(hipGetLastError());
  st = fetch_counters(ctx);
  if (st != JB_COMPLETE) return st;
  *unfinished = (int64_t)ctx->counters_h[CNT_UNFINISHED];
  return *unfinished > 0 ? JB_ITERATE : JB_COMPLETE;
}

extern "C" jb_status jb_zero_energy_tally(jb_context *ctx, jb_mesh *mesh) {
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  const DevMesh &M = mesh->dm;
  hipLaunchKernelGGL(k_zero_tally, dim3(grid_for(ctx, (long long)M.nblocks * M.ncell)), dim3(kBlock), 0,
                     ctx->stream, M);
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

extern "C" jb_status jb_evaluate_radiation_energy(jb_context *ctx, jb_mesh *mesh,
                                                  const jb_swarm_view *swarm) {
  JB_RANGE("Jaybenne::EvaluateRadiationEnergy");
  jb_status st = jb_zero_energy_tally(ctx, mesh);
  if (st != JB_COMPLETE) return st;
  st = check_swarm(swarm, "jb_evaluate_radiation_energy");
  if (st != JB_COMPLETE) return st;
  // (exact deposition: the tally by the exact path -- the close, which also lands what is open of energy_delta)
  if (ctx->deposition == JB_DEPOSIT_EXACT) return deposit_close(ctx, mesh, swarm);
  if (swarm->n > 0)
    hipLaunchKernelGGL(k_tally, dim3(grid_for(ctx, swarm->n)), dim3(kBlock), 0, ctx->stream, mesh->dm,
                       dev_swarm(swarm), (long long)swarm->n);
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

extern "C" jb_status jb_update_fluid(jb_context *ctx, jb_mesh *mesh) {
  JB_RANGE("Jaybenne::UpdateFluid");
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  // (exact deposition: with accumulators open the close comes first, so that energy_delta is final)
  if (mesh->dep_open) {
    const jb_status st = deposit_close(ctx, mesh, &mesh->dep_swarm);
    if (st != JB_COMPLETE) return st;
  }
  if (!ctx->params.do_feedback) return JB_COMPLETE;  // jaybenne.cpp:590
  const DevMesh &M = mesh->dm;
  hipLaunchKernelGGL(k_update_fluid, dim3(grid_for(ctx, (long long)M.nblocks * M.ncell)), dim3(kBlock), 0,
                     ctx->stream, M);
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

extern "C" jb_status jb_photon_reflect_bc(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                          int face) {
  JB_RANGE("Jaybenne::PhotonReflectBC");
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  if (face < 0 || face > 5) return fail(JB_ERR_INVALID, "face must be 0..5");
  jb_status st = check_swarm(swarm, "jb_photon_reflect_bc");
  if (st != JB_COMPLETE) return st;
  if (swarm->n > 0)
    hipLaunchKernelGGL(k_reflect_bc, dim3(grid_for(ctx, swarm->n)), dim3(kBlock), 0, ctx->stream, mesh->dm,
                       dev_swarm(swarm), (long long)swarm->n, face);
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

extern "C" jb_status jb_remove_marked_particles(jb_context *ctx, jb_swarm_view *swarm) {
  JB_RANGE("Jaybenne::RemoveMarkedParticles");
  if (!ctx) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_remove_marked_particles");
  if (st != JB_COMPLETE) return st;
  const long long n = swarm->n;
  if (n == 0) return JB_COMPLETE;
  const DevSwarm S = dev_swarm(swarm);
  unsigned long long *cur = ctx->counters_d + kCursorBase;
  JB_HIP(hipMemsetAsync(cur, 0, 4 * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_count_active, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, S, n, cur + 2);
  JB_HIP(hipGetLastError());
  st = fetch_counters(ctx);
  if (st != JB_COMPLETE) return st;
  const long long survivors = (long long)ctx->counters_h[kCursorBase + 2];
  const long long removed = n - survivors;
  if (removed > 0 && survivors > 0) {
    const long long maxlist = removed < survivors ? removed : survivors;
    st = ensure_scratch(ctx, (size_t)(2 * maxlist));
    if (st != JB_COMPLETE) return st;
    long long *holes = ctx->scratch_d, *movers = ctx->scratch_d + maxlist;
    hipLaunchKernelGGL(k_list_holes_movers, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, S, n,
                       survivors, holes, movers, cur);
    JB_HIP(hipGetLastError());
    st = fetch_counters(ctx);
    if (st != JB_COMPLETE) return st;
    const long long nh = (long long)ctx->counters_h[kCursorBase], nm = (long long)ctx->counters_h[kCursorBase + 1];
    if (nh != nm) return fail(JB_ERR_INVALID, "compaction lists disagree (%lld holes, %lld movers)", nh, nm);
    if (nh > 0)
      hipLaunchKernelGGL(k_fill_holes, dim3(grid_for(ctx, nh)), dim3(kBlock), 0, ctx->stream, S, holes,
                         movers, nh);
    JB_HIP(hipGetLastError());
  }
  swarm->n = survivors;
  for (jb_mesh *m : ctx->dep_open_meshes)   // (what jb_update_fluid closes with)
    if (m->dep_swarm.x == swarm->x) m->dep_swarm.n = survivors;
  return JB_COMPLETE;
}

// The scratch of the sort, the comb and the moments: jb_scratch_layout.hpp says where the arrays lie, and these
// turn a layout into pointers.
template <class T>
static T *scratch_at(const jb_context *ctx, const Span &a) { return (T *)((char *)ctx->scratch_d + a.off); }
struct SortScratch {
  unsigned long long *rec;
  unsigned *hist, *sums, *key;   // hist: the histogram, then the cells' starts (its scan) or ends (behind a move)
};
static SortScratch sort_scratch(const jb_context *ctx, const SortLayout &L) {
  return {scratch_at<unsigned long long>(ctx, L.rec), scratch_at<unsigned>(ctx, L.hist), scratch_at<unsigned>(ctx, L.sums),
          scratch_at<unsigned>(ctx, L.key)};
}
static bool order_by_id(const jb_context *ctx) { return ctx->cell_order == JB_CELL_ORDER_BY_ID; }
// the limits of the 32-bit keys and slot indices, in the words of the entry point `who`
static jb_status check_cell_keys(const CellKeys &k, const char *who) {
  if (k.over == KEYS_PARTICLES) return fail(JB_ERR_INVALID, "%s: more than 2^32 - 1 particles", who);
  if (k.over == KEYS_CELLS) return fail(JB_ERR_INVALID, "%s: more than 2^32 - 2 cells", who);
  return JB_COMPLETE;
}
// in-place exclusive scan of the n words of `data`; sums: a word per tile of kScanTile
static void scan_u32(jb_context *ctx, unsigned *data, long long n, unsigned *sums) {
  const int tiles = (int)((n + kScanTile - 1) / kScanTile);
  hipLaunchKernelGGL(k_scan_tiles, dim3(tiles), dim3(kBlock), 0, ctx->stream, data, n, sums);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, ctx->stream, sums, tiles);
  hipLaunchKernelGGL(k_scan_add, dim3(tiles), dim3(kBlock), 0, ctx->stream, data, n, (const unsigned *)sums);
}
// the keys of the first n slots and their histogram (scan_u32 makes the cells' starts of it)
static jb_status count_cells(jb_context *ctx, const DevMesh &M, const DevSwarm &S, long long n, const CellKeys &k,
                             const SortScratch &p) {
  JB_HIP(hipMemsetAsync(p.hist, 0, sizeof(unsigned) * (size_t)k.nbins, ctx->stream));
  hipLaunchKernelGGL(k_sort_count, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, M, S, n, k.nkeys, p.key, p.hist);
  return JB_COMPLETE;
}
// the schedule of jb_defrag_policy starts over from a sorted swarm
static void defrag_schedule_restart(jb_context *ctx) {
  ctx->rate_ref = 0.0;
  ctx->rate_before_sort = 0.0;
  ctx->excess_ms = 0.0;
  ctx->cycles_since_sort = 0;
}

// The canonical sort (jb_kernel_order.hpp): the first n slots by (sort key, id, input slot).  key: n words of
// scratch for the sort keys (written here).  *moved = 0: the swarm was in that order already and nothing was
// touched.  Synchronises the stream once, for the read-back of k_order_check.
static jb_status order_sort(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, unsigned nkeys,
                            const SortLayout &sort, int *moved) {
  *moved = 0;
  const long long n = swarm->n;
  const DevMesh &M = mesh->dm;
  const OrderLayout &L = sort.order;
  unsigned long long *base = (unsigned long long *)ctx->scratch_d;
  unsigned long long *rec = scratch_at<unsigned long long>(ctx, sort.rec);
  unsigned *key = scratch_at<unsigned>(ctx, sort.key);
  unsigned long long *pairs[2] = {base + L.pairs[0], base + L.pairs[1]};
  unsigned *dest = (unsigned *)(base + L.dest), *cnt = (unsigned *)(base + L.cnt), *csum = (unsigned *)(base + L.csum);
  OrderFlags *flags_d = (OrderFlags *)(base + L.flags);
  const DevSwarm S = dev_swarm(swarm);
  const int gn = grid_for(ctx, n);
  OrderFlags flags{};
  JB_HIP(hipMemsetAsync(flags_d, 0, sizeof(OrderFlags), ctx->stream));
  hipLaunchKernelGGL(k_comb_keys, dim3(gn), dim3(kBlock), 0, ctx->stream, M, S, n, nkeys, key);
  hipLaunchKernelGGL(k_order_check, dim3(gn), dim3(kBlock), 0, ctx->stream, (const unsigned *)key, (const uint64_t *)S.id, n, flags_d);
  JB_HIP(hipGetLastError());
  JB_HIP(hipMemcpyAsync(&flags, flags_d, sizeof(OrderFlags), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  const OrderPlan plan = plan_order(n, flags.max_id, flags.max_key);
  if (!flags.unsorted || plan.npasses == 0) return JB_COMPLETE;
  const int tiles = (int)L.tiles;
  hipLaunchKernelGGL(k_order_init, dim3(gn), dim3(kBlock), 0, ctx->stream, (const unsigned *)key, (const uint64_t *)S.id, n,
                     plan.pass[0].word, pairs[0]);
  for (int q = 0; q < plan.npasses; ++q) {
    const OrderPass &ps = plan.pass[q];
    const unsigned long long *in = pairs[q & 1];
    hipLaunchKernelGGL(k_order_count, dim3(tiles), dim3(kBlock), 0, ctx->stream, in, n, ps.shift, cnt, L.tiles);
    scan_u32(ctx, cnt, L.ncnt, csum);
    hipLaunchKernelGGL(k_order_scatter, dim3(tiles), dim3(kBlock), 0, ctx->stream, in, n, ps.shift, (const unsigned *)cnt,
                       L.tiles, ps.next, (const unsigned *)key, (const uint64_t *)S.id, pairs[(q + 1) & 1], dest);
  }
  hipLaunchKernelGGL(k_order_pack, dim3(gn), dim3(kBlock), 0, ctx->stream, S, n, (const unsigned *)dest, rec);
  hipLaunchKernelGGL(k_sort_unpack, dim3(gn), dim3(kBlock), 0, ctx->stream, S, n, (const unsigned long long *)rec);
  JB_HIP(hipGetLastError());
  *moved = 1;
  return JB_COMPLETE;
}

extern "C" jb_status jb_defrag_particles(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm) {
  JB_RANGE("Jaybenne::DefragParticles");
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_defrag_particles");
  if (st != JB_COMPLETE) return st;
  const long long n = swarm->n;
  if (n == 0) return JB_COMPLETE;
  const DevMesh &M = mesh->dm;
  const CellKeys k = cell_keys(M.nblocks, M.ntot, n);
  if ((st = check_cell_keys(k, "jb_defrag_particles")) != JB_COMPLETE) return st;
  const SortLayout L = sort_layout(n, k.nbins, order_by_id(ctx));
  st = ensure_scratch(ctx, L.words, /*slack=*/false);
  if (st != JB_COMPLETE) return st;
  if (L.by_id) {
    int moved = 0;
    return order_sort(ctx, mesh, swarm, k.nkeys, L, &moved);
  }
  const SortScratch p = sort_scratch(ctx, L);
  const DevSwarm S = dev_swarm(swarm);
  if ((st = count_cells(ctx, M, S, n, k, p)) != JB_COMPLETE) return st;
  scan_u32(ctx, p.hist, k.nbins, p.sums);
  hipLaunchKernelGGL(k_sort_pack, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, S, n, (const unsigned *)p.key,
                     p.hist, p.rec);
  hipLaunchKernelGGL(k_sort_unpack, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, S, n,
                     (const unsigned long long *)p.rec);
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
// Census comb (jb_kernel_comb.hpp).  Its scratch lies behind the sort's (jb_scratch_layout.hpp: comb_layout).
struct CombScratch : SortScratch {
  unsigned *kcnt, *extra, *ssum, *tflag;
  double *C, *tsum, *epart;
  unsigned long long *cpart;
  U128 *C128, *tsum128;   // (canonical order: in the records' memory)
};
static CombScratch comb_scratch(const jb_context *ctx, const CombLayout &L) {
  CombScratch c{sort_scratch(ctx, L.sort)};
  c.kcnt = scratch_at<unsigned>(ctx, L.kcnt);
  c.extra = scratch_at<unsigned>(ctx, L.extra);
  c.ssum = scratch_at<unsigned>(ctx, L.ssum);
  c.tflag = scratch_at<unsigned>(ctx, L.tflag);
  c.C = scratch_at<double>(ctx, L.C);
  c.tsum = scratch_at<double>(ctx, L.tsum);
  c.epart = scratch_at<double>(ctx, L.epart);
  c.cpart = scratch_at<unsigned long long>(ctx, L.cpart);
  c.C128 = scratch_at<U128>(ctx, L.C128);
  c.tsum128 = scratch_at<U128>(ctx, L.tsum128);
  return c;
}
static int comb_parts(long long n) {
  const long long b = (n + kBlock - 1) / kBlock;
  return (int)(b < 1 ? 1 : (b > kCombParts ? kCombParts : b));
}
// the weight of the ACTIVE slots of [0, n): per-workgroup sums on the device, added here in workgroup order
static jb_status comb_energy(jb_context *ctx, const DevSwarm &S, long long n, double *epart_d, double *out) {
  *out = 0.0;
  if (n <= 0) return JB_COMPLETE;
  const int g = comb_parts(n);
  std::vector<double> part((size_t)g);
  hipLaunchKernelGGL(k_comb_energy, dim3(g), dim3(kBlock), 0, ctx->stream, S, n, epart_d);
  JB_HIP(hipGetLastError());
  JB_HIP(hipMemcpyAsync(part.data(), epart_d, sizeof(double) * (size_t)g, hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  double e = 0.0;
  for (int q = 0; q < g; ++q) e += part[(size_t)q];
  *out = e;
  return JB_COMPLETE;
}

// Steps shared by jb_comb_census_plan and jb_comb_census_weigh: the swarm into (block, cell) order, the cells' ends
// (*ends_out) and the running weights c.C.  *unsorted_out: the swarm was not in order (it has been sorted).
static jb_status comb_order_and_weigh(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, const CellKeys &k,
                                      const CombLayout &L, const CombScratch &c, unsigned *unsorted_out,
                                      const unsigned **ends_out, int64_t *sorted) {
  const DevMesh &M = mesh->dm;
  const DevSwarm S = dev_swarm(swarm);
  const long long n = swarm->n;
  const unsigned nkeys = k.nkeys;
  const bool by_id = L.sort.by_id;
  const int gn = grid_for(ctx, n), nt = L.ntiles;
  jb_status st;
  // In key order already (behind a DefragParticles, or a comb, that nothing has moved since)?  Then the sort's
  // move is left out -- and the order within a cell, which the move leaves to its atomics, stays the caller's:
  // the same sorted swarm then gives the same bits.
  // Under JB_CELL_ORDER_BY_ID the test is "in canonical order already?", the sort is the canonical one (which makes
  // that test itself), and the cells' ends come from the histogram and its scan either way.
  unsigned unsorted = 0u;
  if (by_id) {
    int moved = 0;
    st = order_sort(ctx, mesh, swarm, nkeys, L.sort, &moved);
    if (st != JB_COMPLETE) return st;
    unsorted = moved ? 1u : 0u;
  } else {
    unsigned *flag_d = (unsigned *)c.cpart;
    JB_HIP(hipMemsetAsync(flag_d, 0, sizeof(unsigned), ctx->stream));
    hipLaunchKernelGGL(k_comb_keys, dim3(gn), dim3(kBlock), 0, ctx->stream, M, S, n, nkeys, c.key);
    hipLaunchKernelGGL(k_comb_unsorted, dim3(gn), dim3(kBlock), 0, ctx->stream, (const unsigned *)c.key, n, flag_d);
    JB_HIP(hipGetLastError());
    JB_HIP(hipMemcpyAsync(&unsorted, flag_d, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    JB_HIP(hipStreamSynchronize(ctx->stream));
  }
  const unsigned *ends = c.hist;   // (behind the move of jb_defrag_particles: the cells' ends)
  if (unsorted) {
    if (!by_id) {
      st = jb_defrag_particles(ctx, mesh, swarm);
      if (st != JB_COMPLETE) return st;
    }
    // (as behind defrag_now; this sort is not the one whose time the policy weighs against the kernels' loss)
    defrag_schedule_restart(ctx);
    *sorted = 1;
    if (!by_id) hipLaunchKernelGGL(k_comb_keys, dim3(gn), dim3(kBlock), 0, ctx->stream, M, S, n, nkeys, c.key);
  }
  if (by_id || !unsorted) {   // the histogram and its scan alone: the cells' starts, the ends one entry on
    if ((st = count_cells(ctx, M, S, n, k, c)) != JB_COMPLETE) return st;
    scan_u32(ctx, c.hist, k.nbins, c.sums);
    ends = c.hist + 1;
  }
  if (by_id) {
    // exact running weights (jb_kernel_comb.hpp): 128-bit sums in the records' memory, which nothing uses before
    // the move (CombLayout::fits_records); the cells' scales where k_comb_decide's counts go later
    U128 *C128 = c.C128, *tsum128 = c.tsum128;
    unsigned *cexp = c.kcnt;
    JB_HIP(hipMemsetAsync(cexp, 0, sizeof(unsigned) * (size_t)(n + 1), ctx->stream));
    hipLaunchKernelGGL(k_comb_cell_exp, dim3(gn), dim3(kBlock), 0, ctx->stream, (const unsigned *)c.key,
                       (const double *)S.w, ends, n, cexp);
    hipLaunchKernelGGL(k_comb_xseg_tiles, dim3(nt), dim3(kBlock), 0, ctx->stream, (const unsigned *)c.key,
                       (const double *)S.w, ends, (const unsigned *)cexp, n, C128, tsum128, c.tflag);
    hipLaunchKernelGGL(k_comb_xseg_sums, dim3(1), dim3(1024), 0, ctx->stream, tsum128, (const unsigned *)c.tflag, nt);
    hipLaunchKernelGGL(k_comb_xseg_add, dim3(nt), dim3(kBlock), 0, ctx->stream, (const unsigned *)c.key, ends,
                       (const unsigned *)cexp, n, (const U128 *)C128, (const U128 *)tsum128, c.C);
  } else {
    hipLaunchKernelGGL(k_comb_seg_tiles, dim3(nt), dim3(kBlock), 0, ctx->stream, (const unsigned *)c.key,
                       (const double *)S.w, n, c.C, c.tsum, c.tflag);
    hipLaunchKernelGGL(k_comb_seg_sums, dim3(1), dim3(1024), 0, ctx->stream, c.tsum, (const unsigned *)c.tflag, nt);
    hipLaunchKernelGGL(k_comb_seg_add, dim3(nt), dim3(kBlock), 0, ctx->stream, (const unsigned *)c.key, n, c.C,
                       (const double *)c.tsum);
  }
  *unsorted_out = unsorted;
  *ends_out = ends;
  return JB_COMPLETE;
}

extern "C" jb_status jb_comb_census_plan(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, int64_t trigger_T,
                                         int64_t target_K, uint32_t epoch, jb_comb_plan *out) {
  JB_RANGE("Jaybenne::CombCensus");
  if (!ctx || !mesh || !out) return fail(JB_ERR_INVALID, "jb_comb_census_plan: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  ctx->comb.valid = ctx->weigh.valid = false;
  jb_status st = check_swarm(swarm, "jb_comb_census_plan");
  if (st != JB_COMPLETE) return st;
  if (target_K < 1 || target_K > trigger_T)
    return fail(JB_ERR_INVALID, "jb_comb_census_plan: target_K = %lld outside [1, trigger_T = %lld]", (long long)target_K,
                (long long)trigger_T);
  if (trigger_T >= (1ll << 32)) return fail(JB_ERR_INVALID, "jb_comb_census_plan: trigger_T beyond 2^32 - 1");
  if (epoch >= (1u << 20)) return fail(JB_ERR_INVALID, "jb_comb_census_plan: epoch %u beyond 2^20 - 1", epoch);
  memset(out, 0, sizeof *out);
  const long long n = swarm->n;
  out->n_before = out->n_after = n;
  if (n == 0) return JB_COMPLETE;
  const DevMesh &M = mesh->dm;
  const CellKeys k = cell_keys(M.nblocks, M.ntot, n);
  if ((st = check_cell_keys(k, "jb_comb_census_plan")) != JB_COMPLETE) return st;
  const unsigned nkeys = k.nkeys;
  const bool by_id = order_by_id(ctx);
  const CombLayout L = comb_layout(n, k.nbins, by_id);
  // (all of the scratch first: the sort then finds room, and a failed allocation leaves the swarm as it was)
  st = ensure_scratch(ctx, L.words, /*slack=*/false);
  if (st != JB_COMPLETE) return st;
  const CombScratch c = comb_scratch(ctx, L);
  const DevSwarm S = dev_swarm(swarm);
  const unsigned T = (unsigned)trigger_T, K = (unsigned)target_K;
  const int gc = comb_parts((long long)nkeys);
  unsigned unsorted = 0u;
  const unsigned *ends = nullptr;
  if ((st = comb_order_and_weigh(ctx, mesh, swarm, k, L, c, &unsorted, &ends, &out->sorted)) != JB_COMPLETE) return st;
  hipLaunchKernelGGL(k_comb_decide, dim3(grid_for(ctx, n + 1)), dim3(kBlock), 0, ctx->stream, M, n, nkeys,
                     (const unsigned *)c.key, ends, (const double *)c.C, T, K, ctx->dp.key0, epoch,
                     c.kcnt, c.extra);
  hipLaunchKernelGGL(k_comb_cells, dim3(gc), dim3(kBlock), 0, ctx->stream, nkeys, ends, (const double *)c.C, T, c.cpart);
  for (unsigned *data : {c.kcnt, c.extra}) scan_u32(ctx, data, n + 1, c.ssum);
  JB_HIP(hipGetLastError());
  unsigned totals[2] = {0u, 0u};
  std::vector<unsigned long long> cpart((size_t)(2 * gc));
  JB_HIP(hipMemcpyAsync(&totals[0], c.kcnt + n, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipMemcpyAsync(&totals[1], c.extra + n, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipMemcpyAsync(cpart.data(), c.cpart, sizeof(unsigned long long) * cpart.size(), hipMemcpyDeviceToHost, ctx->stream));
  st = comb_energy(ctx, S, n, c.epart, &out->e_before);   // (synchronises)
  if (st != JB_COMPLETE) return st;
  out->n_after = (long long)totals[0];
  out->n_new_ids = (long long)totals[1];
  for (int q = 0; q < gc; ++q) {
    out->cells_combed += (int64_t)cpart[(size_t)(2 * q)];
    if ((int64_t)cpart[(size_t)(2 * q + 1)] > out->max_per_cell) out->max_per_cell = (int64_t)cpart[(size_t)(2 * q + 1)];
  }
  if (out->n_after > n)   // (K <= T rules it out unless a running weight falls: the move must not go past the records)
    return fail(JB_ERR_INVALID, "jb_comb_census_plan: the comb would grow the swarm (%lld -> %lld): negative weights?",
                n, (long long)out->n_after);
  ctx->comb.valid = true;
  ctx->comb.mesh = mesh;
  ctx->comb.x = swarm->x;
  ctx->comb.n = n;
  ctx->comb.n_after = out->n_after;
  ctx->comb.n_new = out->n_new_ids;
  ctx->comb.T = T;
  ctx->comb.K = K;
  ctx->comb.global = false;
  ctx->comb.gen = ctx->scratch_gen;
  ctx->comb.ends_shift = unsorted && !by_id ? 0 : 1;
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
// The global comb (jb_kernel_gcomb.hpp).  Its scratch lies behind the comb's (jb_scratch_layout.hpp: gcomb_layout).
static_assert(sizeof(jb_comb_global_plan) == 72, "nine 8-byte members");
static_assert(kGcombStats * kGcombParts <= 2 * kCombParts, "the report's partials lie in the comb's cpart");
static int gcomb_parts(long long ncells) {
  const long long b = (ncells + kBlock - 1) / kBlock;
  return (int)(b < 1 ? 1 : (b > kGcombParts ? kGcombParts : b));
}

extern "C" jb_status jb_comb_census_weigh(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, int64_t n_room,
                                          double *e_block_host, jb_comb_global_plan *report) {
  JB_RANGE("Jaybenne::CombCensusGlobal");
  if (!ctx || !mesh || !e_block_host || !report) return fail(JB_ERR_INVALID, "jb_comb_census_weigh: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  ctx->comb.valid = ctx->weigh.valid = false;
  jb_status st = check_swarm(swarm, "jb_comb_census_weigh");
  if (st != JB_COMPLETE) return st;
  const long long n = swarm->n;
  if (n_room < n || n_room > swarm->capacity)
    return fail(JB_ERR_INVALID, "jb_comb_census_weigh: n_room = %lld outside [n = %lld, capacity = %lld]", (long long)n_room,
                n, (long long)swarm->capacity);
  memset(report, 0, sizeof *report);
  report->n_before = report->n_after = n;
  const DevMesh &M = mesh->dm;
  for (int b = 0; b < M.nblocks; ++b) e_block_host[b] = 0.0;
  const CellKeys k = cell_keys(M.nblocks, M.ntot, n_room);
  if ((st = check_cell_keys(k, "jb_comb_census_weigh")) != JB_COMPLETE) return st;
  const bool by_id = order_by_id(ctx);
  const GcombLayout G = gcomb_layout(n, n_room, k.nbins, by_id);
  // (all of the scratch first: the sort then finds room, and a failed allocation leaves the swarm as it was)
  if ((st = ensure_scratch(ctx, G.words, /*slack=*/false)) != JB_COMPLETE) return st;
  if ((st = dev_grow(ctx->gcomb_eblock, sizeof(double) * (size_t)M.nblocks, "hipMalloc of the comb's block sums")) != JB_COMPLETE)
    return st;
  unsigned unsorted = 0u;
  if (n > 0) {
    const CombScratch c = comb_scratch(ctx, G.comb);
    const unsigned *ends = nullptr;
    if ((st = comb_order_and_weigh(ctx, mesh, swarm, k, G.comb, c, &unsorted, &ends, &report->sorted)) != JB_COMPLETE) return st;
    ++ctx->gcomb_launches;
    hipLaunchKernelGGL(k_gcomb_block_sums, dim3(M.nblocks), dim3(kBlock), 0, ctx->stream, M, ends, (const double *)c.C,
                       (double *)ctx->gcomb_eblock.p);
    JB_HIP(hipGetLastError());
    JB_HIP(hipMemcpyAsync(e_block_host, ctx->gcomb_eblock.p, sizeof(double) * (size_t)M.nblocks, hipMemcpyDeviceToHost,
                          ctx->stream));
    st = comb_energy(ctx, dev_swarm(swarm), n, c.epart, &report->e_before);   // (synchronises)
    if (st != JB_COMPLETE) return st;
  }
  ctx->weigh.valid = true;
  ctx->weigh.mesh = mesh;
  ctx->weigh.x = swarm->x;
  ctx->weigh.n = n;
  ctx->weigh.n_room = n_room;
  ctx->weigh.ends_shift = unsorted && !by_id ? 0 : 1;
  ctx->weigh.sorted = report->sorted;
  ctx->weigh.e_before = report->e_before;
  ctx->weigh.gen = ctx->scratch_gen;
  return JB_COMPLETE;
}

extern "C" int64_t jb_gcomb_kernel_launches(const jb_context *ctx) { return ctx ? (int64_t)ctx->gcomb_launches : 0; }

extern "C" jb_status jb_comb_census_plan_global(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, double w_total,
                                                int64_t target_N, double band, int64_t split_max, uint32_t epoch,
                                                jb_comb_global_plan *out) {
  JB_RANGE("Jaybenne::CombCensusGlobal");
  if (!ctx || !mesh || !out) return fail(JB_ERR_INVALID, "jb_comb_census_plan_global: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  ctx->comb.valid = false;
  const bool weighed = ctx->weigh.valid;
  ctx->weigh.valid = false;
  jb_status st = check_swarm(swarm, "jb_comb_census_plan_global");
  if (st != JB_COMPLETE) return st;
  if (target_N < 1 || target_N >= (1ll << 31))
    return fail(JB_ERR_INVALID, "jb_comb_census_plan_global: target_N = %lld outside [1, 2^31)", (long long)target_N);
  if (!(band >= 1.0) || !(band < __builtin_huge_val()))
    return fail(JB_ERR_INVALID, "jb_comb_census_plan_global: band = %g is not a finite number >= 1", band);
  if (split_max < 1) return fail(JB_ERR_INVALID, "jb_comb_census_plan_global: split_max = %lld < 1", (long long)split_max);
  if (epoch >= (1u << 20)) return fail(JB_ERR_INVALID, "jb_comb_census_plan_global: epoch %u beyond 2^20 - 1", epoch);
  if (!weighed || ctx->weigh.mesh != mesh || ctx->weigh.x != swarm->x || ctx->weigh.n != swarm->n ||
      ctx->weigh.gen != ctx->scratch_gen || (swarm->n > 0 && !ctx->scratch_d))
    return fail(JB_ERR_INVALID, "jb_comb_census_plan_global: this swarm has not been weighed (jb_comb_census_weigh comes first)");
  const long long n = swarm->n, n_room = ctx->weigh.n_room;
  if (n + (long long)target_N >= (1ll << 32))   // (n_after <= n + target_N: the scans' totals are 32-bit words)
    return fail(JB_ERR_INVALID, "jb_comb_census_plan_global: n + target_N beyond 2^32 - 1");
  memset(out, 0, sizeof *out);
  out->n_before = out->n_after = n;
  out->sorted = ctx->weigh.sorted;
  out->e_before = ctx->weigh.e_before;
  if (n == 0 || !(w_total > 0.0) || !(w_total < __builtin_huge_val())) return JB_COMPLETE;   // nothing is combed
  const DevMesh &M = mesh->dm;
  const CellKeys k = cell_keys(M.nblocks, M.ntot, n_room);
  const unsigned nkeys = k.nkeys;
  const GcombLayout G = gcomb_layout(n, n_room, k.nbins, order_by_id(ctx));
  const CombScratch c = comb_scratch(ctx, G.comb);
  unsigned *ktgt = scratch_at<unsigned>(ctx, G.ktgt);
  const unsigned *ends = c.hist + ctx->weigh.ends_shift;
  const double scale = (double)target_N / w_total;
  const int gc = gcomb_parts((long long)nkeys);
  ctx->gcomb_launches += 2;
  hipLaunchKernelGGL(k_gcomb_targets, dim3(gc), dim3(kBlock), 0, ctx->stream, M, nkeys, ends, (const double *)c.C, scale,
                     band, (double)split_max, ctx->dp.key0, epoch, ktgt, c.cpart);
  hipLaunchKernelGGL(k_gcomb_decide, dim3(grid_for(ctx, n + 1)), dim3(kBlock), 0, ctx->stream, M, n, nkeys,
                     (const unsigned *)c.key, ends, (const double *)c.C, (const unsigned *)ktgt, ctx->dp.key0, epoch,
                     c.kcnt, c.extra);
  for (unsigned *data : {c.kcnt, c.extra}) scan_u32(ctx, data, n + 1, c.ssum);
  JB_HIP(hipGetLastError());
  unsigned totals[2] = {0u, 0u};
  std::vector<unsigned long long> part((size_t)(kGcombStats * gc));
  JB_HIP(hipMemcpyAsync(&totals[0], c.kcnt + n, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipMemcpyAsync(&totals[1], c.extra + n, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipMemcpyAsync(part.data(), c.cpart, sizeof(unsigned long long) * part.size(), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  out->n_after = (long long)totals[0];
  out->n_new_ids = (long long)totals[1];
  unsigned long long in = 0ull, outn = 0ull;
  for (int q = 0; q < gc; ++q) {   // (the workgroups' partials in workgroup order)
    const unsigned long long *p = &part[(size_t)(kGcombStats * q)];
    out->cells_thinned += (int64_t)p[GS_THINNED];
    out->cells_split += (int64_t)p[GS_SPLIT];
    if ((int64_t)p[GS_MOST] > out->max_per_cell) out->max_per_cell = (int64_t)p[GS_MOST];
    if ((int64_t)p[GS_TARGET] > out->max_target) out->max_target = (int64_t)p[GS_TARGET];
    in += p[GS_IN];
    outn += p[GS_OUT];
  }
  // n_after in 64 bits from the targets: the k_j of a combed cell sum to its K_k.  The scans' totals are 32-bit words
  // and wrap where a caller's w_total is not the total (n_after <= n + target_N holds for the true one only).
  const unsigned long long n_after64 = (unsigned long long)n - in + outn;
  if (n_after64 > (unsigned long long)n_room) out->n_after = (int64_t)n_after64;
  if (out->n_after > n_room)   // (no record has been written)
    return fail(JB_ERR_CAPACITY, "jb_comb_census_plan_global: the comb needs %lld slots, n_room = %lld", (long long)out->n_after,
                n_room);
  ctx->comb.valid = true;
  ctx->comb.mesh = mesh;
  ctx->comb.x = swarm->x;
  ctx->comb.n = n;
  ctx->comb.n_after = out->n_after;
  ctx->comb.n_new = out->n_new_ids;
  ctx->comb.T = ctx->comb.K = 0u;
  ctx->comb.global = true;
  ctx->comb.n_room = n_room;
  ctx->comb.gen = ctx->scratch_gen;
  ctx->comb.ends_shift = ctx->weigh.ends_shift;
  return JB_COMPLETE;
}

// jb_comb_census_apply for a plan of the global comb
static jb_status gcomb_apply(jb_context *ctx, jb_swarm_view *swarm, const CellKeys &k, uint64_t id_base, jb_comb_report *out) {
  const long long n = ctx->comb.n, n_after = ctx->comb.n_after, n_room = ctx->comb.n_room;
  if (n_after > swarm->capacity || n_after > n_room)
    return fail(JB_ERR_CAPACITY, "jb_comb_census_apply: %lld slots needed, %lld there", n_after, (long long)swarm->capacity);
  const GcombLayout G = gcomb_layout(n, n_room, k.nbins, order_by_id(ctx));
  const CombScratch c = comb_scratch(ctx, G.comb);
  unsigned long long *rec = scratch_at<unsigned long long>(ctx, G.records());
  const DevSwarm S = dev_swarm(swarm);
  if (n_after > 0) {
    ++ctx->gcomb_launches;
    hipLaunchKernelGGL(k_gcomb_pack, dim3(grid_for(ctx, n_after)), dim3(kBlock), 0, ctx->stream, S, n, n_after, k.nkeys,
                       (const unsigned *)c.key, (const unsigned *)c.hist + ctx->comb.ends_shift, (const double *)c.C,
                       (const unsigned *)scratch_at<unsigned>(ctx, G.ktgt), (const unsigned *)c.kcnt,
                       (const unsigned *)c.extra, ctx->dp.key0, (unsigned long long)id_base, rec);
    hipLaunchKernelGGL(k_sort_unpack, dim3(grid_for(ctx, n_after)), dim3(kBlock), 0, ctx->stream, S, n_after,
                       (const unsigned long long *)rec);
  }
  JB_HIP(hipGetLastError());
  swarm->n = n_after;
  out->n_after = n_after;
  out->n_new_ids = ctx->comb.n_new;
  return comb_energy(ctx, S, n_after, c.epart, &out->e_after);
}

extern "C" jb_status jb_comb_census_apply(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, uint64_t id_base,
                                          jb_comb_report *out) {
  JB_RANGE("Jaybenne::CombCensus");
  if (!ctx || !mesh || !out) return fail(JB_ERR_INVALID, "jb_comb_census_apply: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_comb_census_apply");
  if (st != JB_COMPLETE) return st;
  if (!ctx->comb.valid || ctx->comb.mesh != mesh || ctx->comb.x != swarm->x || ctx->comb.n != swarm->n ||
      ctx->comb.gen != ctx->scratch_gen || !ctx->scratch_d)
    return fail(JB_ERR_INVALID, "jb_comb_census_apply: no plan for this swarm (jb_comb_census_plan comes first)");
  ctx->comb.valid = false;
  const long long n = ctx->comb.n, n_after = ctx->comb.n_after;
  const DevMesh &M = mesh->dm;
  const CellKeys k = cell_keys(M.nblocks, M.ntot, n);   // (within the limits: the plan was made)
  const unsigned nkeys = k.nkeys;
  if (ctx->comb.global) return gcomb_apply(ctx, swarm, k, id_base, out);
  const CombScratch c = comb_scratch(ctx, comb_layout(n, k.nbins, order_by_id(ctx)));
  const DevSwarm S = dev_swarm(swarm);
  hipLaunchKernelGGL(k_comb_pack, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, S, n, nkeys,
                     (const unsigned *)c.key, (const unsigned *)c.hist + ctx->comb.ends_shift, (const double *)c.C,
                     (const unsigned *)c.kcnt,
                     (const unsigned *)c.extra, ctx->comb.T, ctx->comb.K, ctx->dp.key0, (unsigned long long)id_base, c.rec);
  if (n_after > 0)
    hipLaunchKernelGGL(k_sort_unpack, dim3(grid_for(ctx, n_after)), dim3(kBlock), 0, ctx->stream, S, n_after,
                       (const unsigned long long *)c.rec);
  JB_HIP(hipGetLastError());
  swarm->n = n_after;
  out->n_after = n_after;
  out->n_new_ids = ctx->comb.n_new;
  return comb_energy(ctx, S, n_after, c.epart, &out->e_after);
}

// ------------------------------------------------------------------------------------------------
// Radiation moments (jb_kernel_moments.hpp).  Their scratch lies behind the sort's (jb_scratch_layout.hpp: mom_layout).
static_assert(kMoments == JB_MOMENTS && sizeof(jb_moments_report) == 40, "jb_limits.hpp restates the header");
struct MomScratch : SortScratch {
  double *part;
  unsigned long long *stats;
  unsigned *flag;
};
static MomScratch mom_scratch(const jb_context *ctx, const MomLayout &L) {
  return {sort_scratch(ctx, L.sort), scratch_at<double>(ctx, L.part), scratch_at<unsigned long long>(ctx, L.stats),
          scratch_at<unsigned>(ctx, L.flag)};
}
// The first part of a moments or a spectrum call: the swarm into (block, cell) order and the cells' bounds into
// p.hist.  In order already?  As jb_comb_census_plan asks: key order under JB_CELL_ORDER_ANY, the canonical order --
// whose sort makes that test itself -- under JB_CELL_ORDER_BY_ID; if not, the sort (*unsorted = 1; for
// jb_defrag_policy that is a sort, as a comb plan that sorted is).  Synchronises the stream once, not at all for
// n = 0.  flag: a word of scratch.
static jb_status cells_in_order(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, const CellKeys &k,
                                const SortLayout &sort, const SortScratch &p, unsigned *flag, unsigned *unsorted_out) {
  const long long n = swarm->n;
  const DevMesh &M = mesh->dm;
  const DevSwarm S = dev_swarm(swarm);
  const bool by_id = sort.by_id;
  jb_status st;
  unsigned unsorted = 0u;
  if (n > 0 && by_id) {
    int moved = 0;
    st = order_sort(ctx, mesh, swarm, k.nkeys, sort, &moved);
    if (st != JB_COMPLETE) return st;
    unsorted = moved ? 1u : 0u;
  } else if (n > 0) {
    // (one pass makes the keys and the histogram the cells' bounds come from; a swarm in order needs no second)
    JB_HIP(hipMemsetAsync(flag, 0, sizeof(unsigned), ctx->stream));
    if ((st = count_cells(ctx, M, S, n, k, p)) != JB_COMPLETE) return st;
    hipLaunchKernelGGL(k_comb_unsorted, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, (const unsigned *)p.key, n, flag);
    JB_HIP(hipGetLastError());
    JB_HIP(hipMemcpyAsync(&unsorted, flag, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    JB_HIP(hipStreamSynchronize(ctx->stream));
    if (unsorted) {
      st = jb_defrag_particles(ctx, mesh, swarm);
      if (st != JB_COMPLETE) return st;
    }
  }
  if (unsorted) defrag_schedule_restart(ctx);
  // the cells' bounds: the histogram of the keys of the swarm as it lies now, and its scan (what a move left in
  // the histogram's place are the cells' ends, not their starts)
  const bool counted = n > 0 && !by_id && !unsorted;   // the histogram of the order test stands
  if (n > 0) {
    if (!counted && (st = count_cells(ctx, M, S, n, k, p)) != JB_COMPLETE) return st;
    scan_u32(ctx, p.hist, k.nbins, p.sums);
  } else {   // (every cell is empty)
    JB_HIP(hipMemsetAsync(p.hist, 0, sizeof(unsigned) * (size_t)k.nbins, ctx->stream));
  }
  *unsorted_out = unsorted;
  return JB_COMPLETE;
}

// lanes per cell of k_mom_cells: the power of two that holds about twice the mean run and two more
static int mom_group(long long n, long long cells, const char *aid = "JB_MOMENTS_GROUP") {
  if (const char *e = getenv(aid)) {
    const int g = atoi(e);
    if (g >= 1 && g <= 64 && (g & (g - 1)) == 0) return g;
  }
  const double target = 2.0 * (double)n / (double)(cells > 0 ? cells : 1) + 2.0;
  int g = 1;
  while (g < 64 && (double)g < target) g *= 2;
  return g;
}

extern "C" int64_t jb_moments_words(const jb_mesh *mesh) {
  return mesh ? (int64_t)JB_MOMENTS * (int64_t)mesh->dm.nblocks * (int64_t)mesh->dm.ncell : 0;
}

extern "C" jb_status jb_evaluate_radiation_moments(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                                   double *out_dev, jb_moments_report *report) {
  JB_RANGE("Jaybenne::EvaluateRadiationMoments");
  if (!ctx || !mesh || !out_dev) return fail(JB_ERR_INVALID, "jb_evaluate_radiation_moments: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_evaluate_radiation_moments");
  if (st != JB_COMPLETE) return st;
  const long long n = swarm->n;
  const DevMesh &M = mesh->dm;
  const CellKeys k = cell_keys(M.nblocks, M.ntot, n);
  if ((st = check_cell_keys(k, "jb_evaluate_radiation_moments")) != JB_COMPLETE) return st;
  const unsigned nkeys = k.nkeys;
  const long long cells = (long long)M.nblocks * M.ncell;
  if (report) memset(report, 0, sizeof *report);
  const bool by_id = order_by_id(ctx);
  const MomLayout L = mom_layout(n, k.nbins, by_id);
  // (all of the scratch first: the sort then finds room, and a failed allocation leaves the swarm as it was)
  st = ensure_scratch(ctx, L.words, /*slack=*/false);
  if (st != JB_COMPLETE) return st;
  ctx->comb.valid = ctx->weigh.valid = false;   // (a comb plan not yet applied lived in this memory)
  const MomScratch m = mom_scratch(ctx, L);
  const DevSwarm S = dev_swarm(swarm);
  unsigned unsorted = 0u;
  if ((st = cells_in_order(ctx, mesh, swarm, k, L.sort, m, m.flag, &unsorted)) != JB_COMPLETE) return st;
  JB_HIP(hipMemsetAsync(m.stats, 0, sizeof(unsigned long long) * MS_N, ctx->stream));
  const int G = mom_group(n, cells);
  // (one workgroup per 256 slots, not a grid capped to the chip: chunk heads lie 64 waves apart in a long run, and
  // a strided walk would hand all of them to the same few waves; the hardware deals workgroups out as others end)
  if (n > 0)
    hipLaunchKernelGGL(k_mom_chunks, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, M, S, n, nkeys, (const unsigned *)m.key,
                       (const unsigned *)m.hist, (unsigned)G, m.part, out_dev);
  const int gc = grid_for(ctx, cells);
  with_int<1, 2, 4, 8, 16, 32, 64>(G, [&](auto g) {
    hipLaunchKernelGGL(k_mom_cells<decltype(g)::value>, dim3(gc), dim3(kBlock), 0, ctx->stream, M, S,
                       (const unsigned *)m.hist, (const double *)m.part, out_dev, m.stats);
  });
  JB_HIP(hipGetLastError());
  if (report) {
    unsigned long long stats[MS_N] = {};
    JB_HIP(hipMemcpyAsync(stats, m.stats, sizeof stats, hipMemcpyDeviceToHost, ctx->stream));
    JB_HIP(hipStreamSynchronize(ctx->stream));
    report->n_counted = (int64_t)stats[MS_COUNTED];
    report->n_skipped = (int64_t)n - report->n_counted;
    report->cells_nonempty = (int64_t)stats[MS_NONEMPTY];
    report->longest_run = (int64_t)stats[MS_LONGEST];
    report->sorted = unsorted ? 1 : 0;
  }
  return JB_COMPLETE;
}

extern "C" jb_status jb_evaluate_radiation_moments_host(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                                        double *out_host, jb_moments_report *report) {
  if (!ctx || !mesh || !out_host) return fail(JB_ERR_INVALID, "jb_evaluate_radiation_moments_host: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  const size_t words = (size_t)jb_moments_words(mesh);
  jb_status st = dev_grow(ctx->moments, words * sizeof(double), "hipMalloc of the moments array");
  if (st != JB_COMPLETE) return st;
  st = jb_evaluate_radiation_moments(ctx, mesh, swarm, (double *)ctx->moments.p, report);
  if (st != JB_COMPLETE) return st;
  JB_HIP(hipMemcpyAsync(out_host, ctx->moments.p, words * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
// Radiation spectrum (jb_kernel_spectrum.hpp).  Its scratch lies behind the sort's (jb_scratch_layout.hpp:
// spectrum_layout); the call is the moments' up to the kernels.
static_assert(kSpecMaxGroups == JB_SPECTRUM_MAX_GROUPS && sizeof(jb_spectrum_report) == 56,
              "jb_limits.hpp restates the header");
struct SpecScratch : SortScratch {
  double *part;
  unsigned long long *stats;
  unsigned *flag;
};
static SpecScratch spec_scratch(const jb_context *ctx, const SpecLayout &L) {
  return {sort_scratch(ctx, L.sort), scratch_at<double>(ctx, L.part), scratch_at<unsigned long long>(ctx, L.stats),
          scratch_at<unsigned>(ctx, L.flag)};
}
// ngroups + 1 finite, strictly increasing edges
static jb_status check_edges(const double *edges, int ngroups, const char *who) {
  if (ngroups < 1 || ngroups > JB_SPECTRUM_MAX_GROUPS)
    return fail(JB_ERR_INVALID, "%s: ngroups = %d is not in [1, %d]", who, ngroups, JB_SPECTRUM_MAX_GROUPS);
  if (!edges) return fail(JB_ERR_INVALID, "%s: null argument", who);
  for (int j = 0; j <= ngroups; ++j) {
    if (!std::isfinite(edges[j])) return fail(JB_ERR_INVALID, "%s: edge %d is not finite", who, j);
    if (j > 0 && !(edges[j - 1] < edges[j])) return fail(JB_ERR_INVALID, "%s: edge %d is not above edge %d", who, j, j - 1);
  }
  return JB_COMPLETE;
}

extern "C" int64_t jb_spectrum_words(const jb_mesh *mesh, int ngroups) {
  if (!mesh || ngroups < 1 || ngroups > JB_SPECTRUM_MAX_GROUPS) return 0;
  return (int64_t)(ngroups + 2) * (int64_t)mesh->dm.nblocks * (int64_t)mesh->dm.ncell;
}

extern "C" jb_status jb_evaluate_radiation_spectrum(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                                    const double *edges_host, int ngroups, double *out_dev,
                                                    jb_spectrum_report *report) {
  JB_RANGE("Jaybenne::EvaluateRadiationSpectrum");
  if (!ctx || !mesh || !out_dev) return fail(JB_ERR_INVALID, "jb_evaluate_radiation_spectrum: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_evaluate_radiation_spectrum");
  if (st != JB_COMPLETE) return st;
  if ((st = check_edges(edges_host, ngroups, "jb_evaluate_radiation_spectrum")) != JB_COMPLETE) return st;
  const long long n = swarm->n;
  const DevMesh &M = mesh->dm;
  const CellKeys k = cell_keys(M.nblocks, M.ntot, n);
  if ((st = check_cell_keys(k, "jb_evaluate_radiation_spectrum")) != JB_COMPLETE) return st;
  const long long cells = (long long)M.nblocks * M.ncell;
  if (report) memset(report, 0, sizeof *report);
  const SpecLayout L = spectrum_layout(n, k.nbins, order_by_id(ctx), ngroups);
  // (all of the scratch first: the sort then finds room, and a failed allocation leaves the swarm as it was)
  st = ensure_scratch(ctx, L.words, /*slack=*/false);
  if (st != JB_COMPLETE) return st;
  ctx->comb.valid = ctx->weigh.valid = false;   // (a comb plan not yet applied lived in this memory)
  const SpecScratch m = spec_scratch(ctx, L);
  const DevSwarm S = dev_swarm(swarm);
  SpecEdges edges{};   // (a kernel argument by value: no copy to the device, nothing to wait for)
  memcpy(edges.v, edges_host, sizeof(double) * (size_t)(ngroups + 1));
  unsigned unsorted = 0u;
  if ((st = cells_in_order(ctx, mesh, swarm, k, L.sort, m, m.flag, &unsorted)) != JB_COMPLETE) return st;
  JB_HIP(hipMemsetAsync(m.stats, 0, sizeof(unsigned long long) * SS_N, ctx->stream));
  const int G = mom_group(n, cells, "JB_SPECTRUM_GROUP");
  const size_t lds = sizeof(double) * (64 * (size_t)(ngroups + 2) + (size_t)(ngroups + 1));
  // (one workgroup -- one wave -- per 64 slots, not a grid capped to the chip: as k_mom_chunks)
  if (n > 0)
    hipLaunchKernelGGL(k_spec_chunks, dim3((unsigned)((n + kSpecBlock - 1) / kSpecBlock)), dim3(kSpecBlock), lds,
                       ctx->stream, M, S, n, k.nkeys, (const unsigned *)m.key, (const unsigned *)m.hist, (unsigned)G, edges,
                       ngroups, m.part, out_dev, m.stats);
  const long long waves = (cells + 63) / 64, cap = (long long)ctx->num_cu * 32;
  const unsigned gc = (unsigned)(waves < 1 ? 1 : waves < cap ? waves : cap);
  with_int<1, 2, 4, 8, 16, 32, 64>(G, [&](auto g) {
    hipLaunchKernelGGL(k_spec_cells<decltype(g)::value>, dim3(gc), dim3(kSpecBlock), lds, ctx->stream, M, S,
                       (const unsigned *)m.hist, (const double *)m.part, edges, ngroups, out_dev, m.stats);
  });
  JB_HIP(hipGetLastError());
  if (report) {
    unsigned long long stats[SS_N] = {};
    JB_HIP(hipMemcpyAsync(stats, m.stats, sizeof stats, hipMemcpyDeviceToHost, ctx->stream));
    JB_HIP(hipStreamSynchronize(ctx->stream));
    report->n_counted = (int64_t)stats[SS_COUNTED];
    report->n_skipped = (int64_t)n - report->n_counted;
    report->cells_nonempty = (int64_t)stats[SS_NONEMPTY];
    report->longest_run = (int64_t)stats[SS_LONGEST];
    report->n_below = (int64_t)stats[SS_BELOW];
    report->n_above = (int64_t)stats[SS_ABOVE];
    report->sorted = unsorted ? 1 : 0;
  }
  return JB_COMPLETE;
}

extern "C" jb_status jb_evaluate_radiation_spectrum_host(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                                         const double *edges_host, int ngroups, double *out_host,
                                                         jb_spectrum_report *report) {
  if (!ctx || !mesh || !out_host) return fail(JB_ERR_INVALID, "jb_evaluate_radiation_spectrum_host: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_edges(edges_host, ngroups, "jb_evaluate_radiation_spectrum_host");
  if (st != JB_COMPLETE) return st;
  const size_t words = (size_t)jb_spectrum_words(mesh, ngroups);
  st = dev_grow(ctx->spectrum, words * sizeof(double), "hipMalloc of the spectrum array");
  if (st != JB_COMPLETE) return st;
  st = jb_evaluate_radiation_spectrum(ctx, mesh, swarm, edges_host, ngroups, (double *)ctx->spectrum.p, report);
  if (st != JB_COMPLETE) return st;
  JB_HIP(hipMemcpyAsync(out_host, ctx->spectrum.p, words * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  return JB_COMPLETE;
}

// the sort of jb_defrag_policy, timed, and the policy's state behind it
static jb_status defrag_now(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, double rate, int32_t *sorted) {
  if (!ctx->sort_ev[0]) {
    JB_HIP(hipEventCreate(&ctx->sort_ev[0]));
    JB_HIP(hipEventCreate(&ctx->sort_ev[1]));
  }
  (void)hipEventRecord(ctx->sort_ev[0], ctx->stream);
  ctx->scratch_alloc_failed = false;
  jb_status st = jb_defrag_particles(ctx, mesh, swarm);
  // (only "no room for the sort's scratch records" lets the run go on unsorted: any other failure -- a
  // launch or a kernel of the sort itself -- may have left the swarm partly permuted and is the caller's)
  if (st == JB_ERR_HIP && ctx->scratch_alloc_failed) {
    fprintf(stderr, "jaybenne_amd: DefragParticles skipped (%s)\n", g_err);
    (void)hipGetLastError();
    ctx->min_interval = 256;
    ctx->cycles_since_sort = 0;
    ctx->excess_ms = 0.0;
    return JB_COMPLETE;
  }
  if (st != JB_COMPLETE) return st;
  (void)hipEventRecord(ctx->sort_ev[1], ctx->stream);
  ctx->sort_timed = true;
  ctx->sort_n = swarm->n;
  defrag_schedule_restart(ctx);
  ctx->rate_before_sort = rate;
  ++ctx->policy_sorts;
  *sorted = 1;
  return JB_COMPLETE;
}

extern "C" jb_status jb_release_scratch(jb_context *ctx) {
  if (!ctx) return fail(JB_ERR_INVALID, "null context");
  JB_HIP(hipSetDevice(ctx->device));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->scratch_d) JB_HIP(hipFree(ctx->scratch_d));
  ctx->scratch_d = nullptr;
  ctx->scratch_words = 0;
  ++ctx->scratch_gen;
  for (DevBuf *b : {&ctx->step_send, &ctx->step_recv, &ctx->step_gather, &ctx->moments, &ctx->spectrum}) JB_HIP(dev_free(*b));
  return JB_COMPLETE;
}

// jb_defrag_policy: the sort's scratch is taken now -- or there is no room, and the policy backs off
static void policy_take_scratch(jb_context *ctx, const jb_mesh *mesh, const jb_swarm_view *swarm) {
  ctx->sort_scratch_tried = true;
  const CellKeys k = cell_keys(mesh->dm.nblocks, mesh->dm.ntot, swarm->n);
  if (k.over) return;   // (the sort itself will say so)
  if (ensure_scratch(ctx, sort_layout(swarm->n, k.nbins, order_by_id(ctx)).words, /*slack=*/false) != JB_COMPLETE) {
    fprintf(stderr, "jaybenne_amd: no room for the scratch records of DefragParticles (%s): the swarm stays unsorted\n", g_err);
    (void)hipGetLastError();
    ctx->min_interval = 256;
  }
}

extern "C" jb_status jb_defrag_policy(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                       int64_t events_this_cycle, int32_t mode, int32_t *sorted) {
  if (!ctx || !mesh || !sorted) return fail(JB_ERR_INVALID, "null argument");
  if (mode < JB_DEFRAG_DECIDE_AND_SORT || mode > JB_DEFRAG_SORT_NOW) return fail(JB_ERR_INVALID, "unknown mode");
  *sorted = 0;
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_defrag_policy");
  if (st != JB_COMPLETE) return st;
  // (SORT_NOW: the ranks have agreed, and the cycle's times were taken by the DECIDE call)
  if (mode == JB_DEFRAG_SORT_NOW) return defrag_now(ctx, mesh, swarm, ctx->last_rate, sorted);
  // time of this cycle's tracking kernels (the caller has synchronised: it knows the event count)
  double ms = 0.0;
  bool ok = !ctx->tev_overflow && ctx->tev_used > 0;
  for (int q = 0; ok && q + 1 < ctx->tev_used; q += 2) {
    float t = 0.0f;
    if (hipEventElapsedTime(&t, ctx->tev[q], ctx->tev[q + 1]) != hipSuccess) ok = false;
    ms += (double)t;
  }
  (void)hipGetLastError();  // (an event that has not completed: not an error of the library's)
  ctx->tev_used = 0;
  ctx->tev_overflow = false;
  if (ctx->sort_timed) {  // what the last sort cost (it was queued behind the previous cycle)
    float t = 0.0f;
    if (hipEventElapsedTime(&t, ctx->sort_ev[0], ctx->sort_ev[1]) == hipSuccess && ctx->sort_n > 0)
      ctx->sort_ms_per_photon = (double)t / (double)ctx->sort_n;
    (void)hipGetLastError();
    ctx->sort_timed = false;
  }
  if (!ok || events_this_cycle <= 0 || swarm->n < (1ll << 20)) return JB_COMPLETE;
  const double rate = ms / (double)events_this_cycle;
  ++ctx->cycles_since_sort;
  if (ctx->cycles_since_sort == 1 && ctx->rate_before_sort > 0.0) {
    // the first cycle behind a sort: did it pay?  If the rate came down by less than 1 % (timing
    // noise between cycles is ~0.3 %), what made the kernels slower was not the order of the swarm
    // -- wait twice as long before the next one
    if (rate > 0.99 * ctx->rate_before_sort) ctx->min_interval = ctx->min_interval < 256 ? 2 * ctx->min_interval : 256;
    else ctx->min_interval = 2;
    ctx->rate_before_sort = 0.0;
  }
  // The sort's scratch records (128 bytes per photon; a fresh allocation costs ~30 ms per GB, which must not
  // land in the cycle that first sorts: 400 ms on BASELINE configs[2]) are asked for as soon as the cycles
  // START to slow down (0.5 %: at least one cycle before the 1.5 % a sort needs) -- a run whose swarm keeps
  // its order never allocates them (12.8 GB at 1e8 photons); one that has no room learns so here.
  // Where memory is plentiful (the records would take less than a quarter of what is free: 12.8 GB of an
  // MI355X's 288) they are taken at the FIRST cycle the policy sees -- a host's warm-up -- so that no later
  // cycle of the run pays for the allocation at all.  And a cycle that meets the sort's own condition without
  // them (a slow-down from under 0.5 % to over 1.5 % within one cycle) takes the allocation, not the sort:
  // the sort follows a cycle later (below).
  bool scratch_now = !ctx->sort_scratch_tried && ctx->rate_ref > 0.0 && rate > 1.005 * ctx->rate_ref;
  if (!ctx->sort_scratch_tried && !scratch_now && ctx->rate_ref == 0.0) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
        (double)free_b > 4.0 * 8.0 * (double)kSortRecWords * (double)swarm->n)
      scratch_now = true;
    (void)hipGetLastError();
  }
  bool allocated_this_cycle = false;
  if (scratch_now) {
    allocated_this_cycle = true;
    policy_take_scratch(ctx, mesh, swarm);
  }
  if (ctx->rate_ref == 0.0 || rate < ctx->rate_ref) ctx->rate_ref = rate;
  const double excess_now = (rate - ctx->rate_ref) * (double)events_this_cycle;
  ctx->excess_ms += excess_now;
  // Sort when one more cycle in this order would cost more than a cycle has cost on average since
  // the last sort, the sort included: with p cycles behind the sort, loss L so far and a sort that
  // costs S, that is  e(p + 1) >= (S + L) / p  -- for a loss per cycle that keeps growing, the period
  // with the lowest (S + L) / p.  e(p + 1) is extrapolated from this cycle's loss, e(p) p / (p - 1)
  // (linear growth from zero in the first cycle).  Only on a slow-down that is no timing noise (1.5 %).
  ctx->last_rate = rate;
  const double sort_ms = ctx->sort_ms_per_photon * (double)swarm->n;
  const int p = ctx->cycles_since_sort;
  const double excess_next = p > 1 ? excess_now * (double)p / (double)(p - 1) : excess_now;
  if (p >= ctx->min_interval && rate > 1.015 * ctx->rate_ref &&
      excess_next * (double)p >= sort_ms + ctx->excess_ms) {
    if (!ctx->sort_scratch_tried) {   // (never asked for: this cycle takes the allocation, the next one the sort)
      policy_take_scratch(ctx, mesh, swarm);
      return JB_COMPLETE;
    }
    if (allocated_this_cycle && mode != JB_DEFRAG_SORT_NOW) return JB_COMPLETE;
    if (mode == JB_DEFRAG_DECIDE) {
      *sorted = 1;  // (this rank would sort: the host asks the others, then calls again with SORT_NOW)
      return JB_COMPLETE;
    }
    return defrag_now(ctx, mesh, swarm, rate, sorted);
  }
  return JB_COMPLETE;
}

extern "C" jb_status jb_pack_outgoing(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm,
                                      int64_t first, int64_t last, int nranks, int64_t *records_dev,
                                      int64_t record_capacity, int64_t *counts_host) {
  JB_RANGE("Jaybenne::MeshSend");
  if (!ctx || !mesh || !counts_host) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_pack_outgoing");
  if (st != JB_COMPLETE) return st;
  if (first < 0 || last > swarm->n || first > last) return fail(JB_ERR_INVALID, "bad particle range");
  if (nranks < mesh->nranks_seen || nranks > kRankEnd - kRankBase)
    return fail(JB_ERR_INVALID, "nranks = %d does not cover the owners in the mesh view", nranks);
  unsigned long long *per_rank = ctx->counters_d + kRankBase;
  JB_HIP(hipMemsetAsync(per_rank, 0, sizeof(unsigned long long) * nranks, ctx->stream));
  const DevSwarm S = dev_swarm(swarm);
  if (last > first)
    hipLaunchKernelGGL(k_count_outgoing, dim3(grid_for(ctx, last - first)), dim3(kBlock), 0, ctx->stream,
                       mesh->dm, S, (long long)first, (long long)last, per_rank);
  JB_HIP(hipGetLastError());
  JB_HIP(hipMemcpyAsync(ctx->counters_h + kRankBase, per_rank, sizeof(unsigned long long) * nranks,
                        hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  long long total = 0;
  std::vector<long long> firsts(nranks);
  for (int r = 0; r < nranks; ++r) {
    counts_host[r] = (int64_t)ctx->counters_h[kRankBase + r];
    firsts[r] = total;
    total += counts_host[r];
  }
  if (total == 0) return JB_COMPLETE;
  if (!records_dev || total > record_capacity)
    return fail(JB_ERR_CAPACITY, "hand-off buffer holds %lld records, %lld needed",
                (long long)record_capacity, total);
  st = ensure_scratch(ctx, (size_t)nranks);
  if (st != JB_COMPLETE) return st;
  JB_HIP(hipMemcpyAsync(ctx->scratch_d, firsts.data(), sizeof(long long) * nranks, hipMemcpyHostToDevice,
                        ctx->stream));
  JB_HIP(hipMemsetAsync(per_rank, 0, sizeof(unsigned long long) * nranks, ctx->stream));
  hipLaunchKernelGGL(k_pack_outgoing, dim3(grid_for(ctx, last - first)), dim3(kBlock), 0, ctx->stream,
                     mesh->dm, S, (long long)first, (long long)last, (const long long *)ctx->scratch_d,
                     per_rank, (long long *)records_dev);
  JB_HIP(hipGetLastError());
  JB_HIP(hipStreamSynchronize(ctx->stream));  // firsts lives on this stack frame
  return JB_COMPLETE;
}

extern "C" jb_status jb_unpack_incoming(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm,
                                        const int64_t *records_dev, int64_t nrecords) {
  JB_RANGE("Jaybenne::MeshReceive");
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_unpack_incoming");
  if (st != JB_COMPLETE) return st;
  if (nrecords < 0) return fail(JB_ERR_INVALID, "negative record count");
  if (nrecords == 0) return JB_COMPLETE;
  if (!records_dev) return fail(JB_ERR_INVALID, "null record buffer");
  if (swarm->n + nrecords > swarm->capacity)
    return fail(JB_ERR_CAPACITY, "swarm capacity %lld too small for %lld arrivals",
                (long long)swarm->capacity, (long long)nrecords);
  // (exact deposition: the decoy view must exist BEFORE the launch, also when this is the mesh's first call in the mode)
  if (ctx->deposition == JB_DEPOSIT_EXACT && (st = deposit_ensure(ctx, mesh)) != JB_COMPLETE) return st;
  hipLaunchKernelGGL(k_unpack_incoming, dim3(grid_for(ctx, nrecords)), dim3(kBlock), 0, ctx->stream,
                     track_dm(mesh), dev_swarm(swarm), (long long)swarm->n, (const long long *)records_dev,
                     (long long)nrecords);
  JB_HIP(hipGetLastError());
#ifdef JB_INVARIANTS
  {  // (checked build) SWARM over the arrivals (their indices are their sender's: see k_inv_swarm)
    const jb_status ist = inv_sweep(ctx, mesh->dm, dev_swarm(swarm), swarm->n, swarm->n + nrecords, DBL_MAX, false);
    if (ist != JB_COMPLETE) return ist;
  }
#endif
  swarm->n += nrecords;
  // (exact deposition: the arrivals absorbed in a halo copy on their sender, deposited here by the owner)
  if (ctx->deposition == JB_DEPOSIT_EXACT)
    return deposit_sweep(ctx, mesh, swarm, swarm->n - nrecords, swarm->n, DEP_ARRIVALS);
  return JB_COMPLETE;
}

// the rank x rank count matrix of jb_exchange (+ its pack offsets), in a buffer of the context's own
static jb_status ensure_count_matrix(jb_context *ctx, int nranks) {
  const size_t R = nranks > 64 ? (size_t)nranks : 64;
  return dev_grow(ctx->xch, R * (R + 8) * sizeof(unsigned long long), "jb_exchange: hipMalloc of the count matrix");
}

// ------------------------------------------------------------------------------------------------
// jb_exchange: MeshResetCommunication -> MeshSend -> MeshReceive (jaybenne.cpp:26-61) as ONE call on the
// context's stream, the records never leaving the device.  What moves the bytes is a jb_exchange_transport
// (two collectives on device buffers): jb_transport_rccl below is the production one.
extern "C" jb_status jb_exchange(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, int64_t first,
                                 int64_t last, int rank, int nranks, const jb_exchange_transport *tr,
                                 int64_t *send_dev, int64_t send_capacity, int64_t *recv_dev,
                                 int64_t recv_capacity, int64_t *nsent, int64_t *nreceived,
                                 int64_t *moved_anywhere) {
  JB_RANGE("Jaybenne::MeshSendReceive");
  if (!ctx || !mesh || !tr || !tr->all_gather_u64 || !tr->all_to_all_v || !nsent || !nreceived || !moved_anywhere)
    return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  jb_status st = check_swarm(swarm, "jb_exchange");
  if (st != JB_COMPLETE) return st;
  if (first < 0 || last > swarm->n || first > last) return fail(JB_ERR_INVALID, "bad particle range");
  if (rank < 0 || rank >= nranks) return fail(JB_ERR_INVALID, "rank outside [0, nranks)");
#ifdef JB_INVARIANTS
  constexpr int kRoomWords = 4;   // (checked build) + this rank's invariant violations since its last exchange
#else
  constexpr int kRoomWords = 3;
#endif
  if (nranks < mesh->nranks_seen || nranks + kRoomWords > kRankEnd - kRankBase)
    return fail(JB_ERR_INVALID, "nranks = %d does not cover the owners in the mesh view", nranks);
  *nsent = 0; *nreceived = 0; *moved_anywhere = 0;
  // (exact deposition: the decoy view k_unpack_incoming gets must exist before its launch, also when the exchange is
  // this mesh's first call in the mode -- a rank whose swarm was empty so far; taken here, in front of the collectives)
  if (ctx->deposition == JB_DEPOSIT_EXACT && (st = deposit_ensure(ctx, mesh)) != JB_COMPLETE) return st;
  const int row = nranks + kRoomWords;   // what a rank contributes to the all-gather: counts | send, receive, swarm room
  // 1. records per destination rank, counted on the device ...
  unsigned long long *per_rank = ctx->counters_d + kRankBase;
  JB_HIP(hipMemsetAsync(per_rank, 0, sizeof(unsigned long long) * nranks, ctx->stream));
  const DevSwarm S = dev_swarm(swarm);
  if (last > first)
    hipLaunchKernelGGL(k_count_outgoing, dim3(grid_for(ctx, last - first)), dim3(kBlock), 0, ctx->stream,
                       mesh->dm, S, (long long)first, (long long)last, per_rank);
  JB_HIP(hipGetLastError());
  // ... followed, in the same buffer, by what this rank has room for: the capacity decision below must
  // come out the same on EVERY rank (a rank that returned early would leave the others hanging in the
  // payload exchange), so every rank gets to see every rank's room
  ctx->xch_room[0] = (unsigned long long)(send_dev ? send_capacity : 0);
  ctx->xch_room[1] = (unsigned long long)(recv_dev ? recv_capacity : 0);
  ctx->xch_room[2] = (unsigned long long)(swarm->capacity - swarm->n);
#ifdef JB_INVARIANTS
  {  // the violations since this rank's last exchange travel in its row: every rank sees every rank's
    int64_t tot = 0;
    JB_HIP(hipStreamSynchronize(ctx->stream));   // (the record counts above are not read back: only the kernels' end)
    if (inv_violations(ctx, &tot) != JB_COMPLETE) tot = ctx->inv_reported + 1;   // (unreadable: reported as one)
    ctx->xch_room[3] = (unsigned long long)(tot - ctx->inv_reported);
    ctx->inv_reported = tot;
  }
#endif
  JB_HIP(hipMemcpyAsync(per_rank + nranks, ctx->xch_room, kRoomWords * sizeof(unsigned long long), hipMemcpyHostToDevice,
                        ctx->stream));
  // 2. ... gathered from every rank straight from that buffer (no read-back in front of the collective):
  // the rank x rank matrix carries this rank's receive sizes AND the answer to "did anything move
  // anywhere" (the completion test of jaybenne.cpp:130-131 needs no collective of its own) ...
  // (the count matrix lives in a buffer of its own, taken on the FIRST call of a context -- before any rank has
  // entered a collective of the run's hot loop; a rank that cannot get its few KB fails there, and says so
  // in the gathered row of every later call: a rank-local failure must not leave the others in a collective)
  st = ensure_count_matrix(ctx, nranks);
  if (st != JB_COMPLETE) return st;
  unsigned long long *matrix_d = (unsigned long long *)ctx->xch.p;
  if (tr->all_gather_u64(tr->handle, (const uint64_t *)per_rank, (uint64_t *)matrix_d, row, (void *)ctx->stream) != 0)
    return fail(JB_ERR_HIP, "jb_exchange: the transport's all-gather of the record counts failed");
  // 3. ... and read back ONCE per call: nranks (nranks + 3) words
  ctx->xch_matrix.resize((size_t)nranks * (size_t)row);
  JB_HIP(hipMemcpyAsync(ctx->xch_matrix.data(), matrix_d, sizeof(unsigned long long) * ctx->xch_matrix.size(),
                        hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  auto cnt = [&](int from, int to) { return (long long)ctx->xch_matrix[(size_t)from * row + to]; };
  long long total = 0, mine_out = 0, mine_in = 0;
  ctx->xch_tab.assign(4 * (size_t)nranks, 0);   // send counts | send offsets | recv counts | recv offsets (records)
  long long *sc = ctx->xch_tab.data(), *so = sc + nranks, *rc = so + nranks, *ro = rc + nranks;
  for (int s_ = 0; s_ < nranks; ++s_)
    for (int r = 0; r < nranks; ++r) total += cnt(s_, r);
  for (int r = 0; r < nranks; ++r) {
    sc[r] = cnt(rank, r);
    rc[r] = cnt(r, rank);
    so[r] = mine_out; ro[r] = mine_in;
    mine_out += sc[r]; mine_in += rc[r];
  }
  *moved_anywhere = total;
  *nsent = mine_out; *nreceived = mine_in;
#ifdef JB_INVARIANTS
  {  // (checked build) the same verdict on every rank, before anything else is exchanged: JB_ERR_INVARIANT when any
     // rank has had a violation since its last exchange (steps report: jb_radiation_step_ranks returns it too)
    unsigned long long v = 0;
    for (int q = 0; q < nranks; ++q) v += ctx->xch_matrix[(size_t)q * row + nranks + 3];
    if (v != 0) return inv_fail(ctx, (int64_t)v, "jb_exchange");
  }
#endif
  // (every rank looks at every rank's diagonal: the same verdict everywhere)
  for (int q = 0; q < nranks; ++q)
    if (cnt(q, q) != 0) return fail(JB_ERR_INVALID, "jb_exchange: rank %d hands particles to itself", q);
  if (total == 0) return JB_COMPLETE;
  // the same verdict on every rank: does EVERY rank have room for what it sends and takes in?
  for (int q = 0; q < nranks; ++q) {
    long long out_q = 0, in_q = 0;
    for (int r = 0; r < nranks; ++r) { out_q += cnt(q, r); in_q += cnt(r, q); }
    const long long send_room = (long long)ctx->xch_matrix[(size_t)q * row + nranks];
    const long long recv_room = (long long)ctx->xch_matrix[(size_t)q * row + nranks + 1];
    const long long swarm_room = (long long)ctx->xch_matrix[(size_t)q * row + nranks + 2];
    if (out_q > send_room)
      return fail(JB_ERR_CAPACITY, "jb_exchange: rank %d's send buffer holds %lld records, %lld needed", q, send_room, out_q);
    if (in_q > recv_room)
      return fail(JB_ERR_CAPACITY, "jb_exchange: rank %d's receive buffer holds %lld records, %lld needed", q, recv_room, in_q);
    if (in_q > swarm_room)
      return fail(JB_ERR_CAPACITY, "jb_exchange: rank %d's swarm has room for %lld arrivals, %lld needed", q, swarm_room, in_q);
  }
  // 4. pack (the packed slots become holes), 5. the payload, 6. unpack behind it on the same stream
  if (mine_out > 0) {
    long long *firsts_d = (long long *)(matrix_d + (size_t)nranks * row);
    JB_HIP(hipMemcpyAsync(firsts_d, so, sizeof(long long) * nranks, hipMemcpyHostToDevice, ctx->stream));
    JB_HIP(hipMemsetAsync(per_rank, 0, sizeof(unsigned long long) * nranks, ctx->stream));
    hipLaunchKernelGGL(k_pack_outgoing, dim3(grid_for(ctx, last - first)), dim3(kBlock), 0, ctx->stream,
                       mesh->dm, S, (long long)first, (long long)last, (const long long *)firsts_d,
                       per_rank, (long long *)send_dev);
    JB_HIP(hipGetLastError());
  }
  if (tr->all_to_all_v(tr->handle, send_dev, (const int64_t *)sc, (const int64_t *)so, recv_dev,
                       (const int64_t *)rc, (const int64_t *)ro, kRecWords, (void *)ctx->stream) != 0)
    return fail(JB_ERR_HIP, "jb_exchange: the transport's record exchange failed");
  if (mine_in > 0) {
    hipLaunchKernelGGL(k_unpack_incoming, dim3(grid_for(ctx, mine_in)), dim3(kBlock), 0, ctx->stream,
                       track_dm(mesh), dev_swarm(swarm), (long long)swarm->n, (const long long *)recv_dev,
                       (long long)mine_in);
    JB_HIP(hipGetLastError());
#ifdef JB_INVARIANTS
    // (checked build) SWARM over the arrivals (their indices are their sender's: see k_inv_swarm)
    if (inv_sweep(ctx, mesh->dm, dev_swarm(swarm), swarm->n, swarm->n + mine_in, DBL_MAX, false) != JB_COMPLETE)
      return JB_ERR_HIP;
#endif
    swarm->n += mine_in;
    if (ctx->deposition == JB_DEPOSIT_EXACT)
      return deposit_sweep(ctx, mesh, swarm, swarm->n - mine_in, swarm->n, DEP_ARRIVALS);
  }
  return JB_COMPLETE;
}

// ---- the RCCL transport: all-gather + grouped send / recv on the caller's communicator.  RCCL is
// loaded when the first transport is made (dlopen: the library itself does not link against it, so a
// host without RCCL -- or with its own copy already in the process, as PyTorch has -- loads fine).
namespace {
struct RcclApi {
  void *lib = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;
constexpr int kNcclInt64 = 4, kNcclUint64 = 5;   // ncclDataType_t (rccl.h)
struct RcclHandle { void *comm; int rank, nranks; };

bool load_rccl() {
  if (g_rccl.lib) return true;
  for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    g_rccl.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (g_rccl.lib) break;
  }
  if (!g_rccl.lib) return false;
  g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(g_rccl.lib, "ncclAllGather");
  g_rccl.Send = (decltype(g_rccl.Send))dlsym(g_rccl.lib, "ncclSend");
  g_rccl.Recv = (decltype(g_rccl.Recv))dlsym(g_rccl.lib, "ncclRecv");
  g_rccl.GroupStart = (decltype(g_rccl.GroupStart))dlsym(g_rccl.lib, "ncclGroupStart");
  g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))dlsym(g_rccl.lib, "ncclGroupEnd");
  g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(g_rccl.lib, "ncclGetErrorString");
  return g_rccl.AllGather && g_rccl.Send && g_rccl.Recv && g_rccl.GroupStart && g_rccl.GroupEnd;
}

int rccl_all_gather(void *h, const uint64_t *in_dev, uint64_t *out_dev, int count, void *stream) {
  const RcclHandle *H = (const RcclHandle *)h;
  return g_rccl.AllGather(in_dev, out_dev, (size_t)count, kNcclUint64, H->comm, (hipStream_t)stream);
}
// every rank pair uses its own xGMI link: one grouped send / recv per peer, no ring through the node
int rccl_all_to_all_v(void *h, const int64_t *send_dev, const int64_t *sc, const int64_t *so, int64_t *recv_dev,
                      const int64_t *rc, const int64_t *ro, int words, void *stream) {
  const RcclHandle *H = (const RcclHandle *)h;
  int err = g_rccl.GroupStart();
  for (int r = 0; r < H->nranks && err == 0; ++r) {
    if (sc[r] > 0) err = g_rccl.Send(send_dev + so[r] * words, (size_t)(sc[r] * words), kNcclInt64, r, H->comm, (hipStream_t)stream);
    if (err == 0 && rc[r] > 0)
      err = g_rccl.Recv(recv_dev + ro[r] * words, (size_t)(rc[r] * words), kNcclInt64, r, H->comm, (hipStream_t)stream);
  }
  const int end = g_rccl.GroupEnd();
  return err != 0 ? err : end;
}
}  // namespace

extern "C" jb_status jb_transport_rccl(void *nccl_comm, int rank, int nranks, jb_exchange_transport *out) {
  if (!nccl_comm || !out) return fail(JB_ERR_INVALID, "null argument");
  if (rank < 0 || rank >= nranks) return fail(JB_ERR_INVALID, "rank outside [0, nranks)");
  if (!load_rccl()) return fail(JB_ERR_INVALID, "jb_transport_rccl: librccl.so could not be loaded (%s)", dlerror());
  RcclHandle *H = new (std::nothrow) RcclHandle{nccl_comm, rank, nranks};
  if (!H) return fail(JB_ERR_INVALID, "out of memory");
  out->handle = H;
  out->all_gather_u64 = rccl_all_gather;
  out->all_to_all_v = rccl_all_to_all_v;
  return JB_COMPLETE;
}

extern "C" jb_status jb_transport_release(jb_exchange_transport *tr) {
  if (tr && tr->all_gather_u64 == rccl_all_gather) delete (RcclHandle *)tr->handle;
  if (tr) { tr->handle = nullptr; tr->all_gather_u64 = nullptr; tr->all_to_all_v = nullptr; }
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
static double *const *field_table(const DevMesh &M, int field) {
  switch (field) {
    case JB_FIELD_RHO: return M.rho;
    case JB_FIELD_SIE: return M.sie;
    case JB_FIELD_U: return M.u;
    case JB_FIELD_FLECK: return M.fleck;
    case JB_FIELD_TALLY: return M.tally;
    case JB_FIELD_EDELTA: return M.edelta;
    default: return nullptr;
  }
}

extern "C" jb_status jb_gather_cells(jb_context *ctx, jb_mesh *mesh, int field, int64_t n,
                                     const int32_t *blk_dev, const int32_t *cell_dev,
                                     double *out_dev) {
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  double *const *F = field_table(mesh->dm, field);
  if (!F) return fail(JB_ERR_INVALID, "jb_gather_cells: unknown field %d", field);
  if (n < 0) return fail(JB_ERR_INVALID, "negative cell count");
  if (n == 0) return JB_COMPLETE;
  if (!blk_dev || !cell_dev || !out_dev) return fail(JB_ERR_INVALID, "null argument");
  hipLaunchKernelGGL(k_gather_cells, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, F,
                     (long long)n, blk_dev, cell_dev, out_dev);
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

extern "C" jb_status jb_fill_cells(jb_context *ctx, jb_mesh *mesh, int field, int64_t n,
                                   int nsamples, const int32_t *dst_blk_dev,
                                   const int32_t *dst_cell_dev, const int32_t *src_blk_dev,
                                   const int32_t *src_cell_dev, const double *remote_dev) {
  if (!ctx || !mesh) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  double *const *F = field_table(mesh->dm, field);
  if (!F) return fail(JB_ERR_INVALID, "jb_fill_cells: unknown field %d", field);
  if (n < 0) return fail(JB_ERR_INVALID, "negative cell count");
  if (n == 0) return JB_COMPLETE;
  if (!dst_blk_dev || !dst_cell_dev || !src_blk_dev || !src_cell_dev)
    return fail(JB_ERR_INVALID, "null argument");
#define JB_FILL(NS)                                                                              \
  hipLaunchKernelGGL(k_fill_cells<NS>, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, F,   \
                     (long long)n, dst_blk_dev, dst_cell_dev, src_blk_dev, src_cell_dev, remote_dev)
  switch (nsamples) {
    case 1: JB_FILL(1); break;
    case 2: JB_FILL(2); break;
    case 4: JB_FILL(4); break;
    case 8: JB_FILL(8); break;
    default: return fail(JB_ERR_INVALID, "jb_fill_cells: nsamples must be 1, 2, 4 or 8");
  }
#undef JB_FILL
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
// Energy ledger (jb_kernel_ledger.hpp): sweeps that write per-workgroup partial sums, one workgroup that adds
// them in a fixed order into the running ledger on the device, one read-back when the cycle closes.
// the buffer of jb_ledger_reduce: a row [status | ledger] of this rank's, then one of every rank's
static jb_status ledger_gather_room(jb_context *ctx, int nranks) {
  return dev_grow(ctx->ledger_gather, (size_t)kLedgerGatherRow * (size_t)(nranks + 1) * sizeof(unsigned long long),
                  "hipMalloc of the ledger's gather buffer");
}

extern "C" jb_status jb_ledger_enable(jb_context *ctx, int on) {
  if (!ctx) return fail(JB_ERR_INVALID, "jb_ledger_enable: null argument");
  JB_HIP(hipSetDevice(ctx->device));
  if (on && !ctx->ledger_d) {
    const int parts = ctx->num_cu * 8;
    JB_HIP(hipMalloc(&ctx->ledger_d, ((size_t)kLedgerHead + (size_t)parts * kLedgerStride) * sizeof(unsigned long long)));
    ctx->ledger_parts = parts;
  }
  // (taken here, for any number of ranks the step call accepts: jb_ledger_reduce then has nothing left that
  // can fail on one rank alone before its collective)
  if (on && !ctx->ledger_gather.p) {
    const jb_status st = ledger_gather_room(ctx, kRankEnd);
    if (st != JB_COMPLETE) return st;
  }
  if (on) JB_HIP(hipMemsetAsync(ctx->ledger_d, 0, kLedgerHead * sizeof(unsigned long long), ctx->stream));
  ctx->ledger_on = on != 0;
  ctx->ledger_has_last = false;
  return JB_COMPLETE;
}

extern "C" int jb_ledger_enabled(const jb_context *ctx) { return ctx && ctx->ledger_on ? 1 : 0; }

// one sweep over [first, last) and the sum of its partials, on the context's stream
static jb_status ledger_sweep(jb_context *ctx, const DevMesh &M, const DevSwarm &S, long long first, long long last,
                              int what) {
  if (last <= first) return JB_COMPLETE;
  // (a grid from the CU count, as grid_for; a workgroup takes kLedgerUnroll x kBlock slots per trip)
  const long long tile = (long long)kLedgerUnroll * kBlock;
  long long blocks = (last - first + tile - 1) / tile;
  if (blocks > ctx->ledger_parts) blocks = ctx->ledger_parts;
  unsigned long long *parts = ctx->ledger_d + kLedgerHead;
  const dim3 grid((unsigned)blocks), block(kBlock);
  switch (what) {
  case LEDGER_SOURCED: hipLaunchKernelGGL(k_ledger_sweep<LEDGER_SOURCED>, grid, block, 0, ctx->stream, M, S, first, last, parts); break;
  case LEDGER_TRANSPORTED: hipLaunchKernelGGL(k_ledger_sweep<LEDGER_TRANSPORTED>, grid, block, 0, ctx->stream, M, S, first, last, parts); break;
  default: hipLaunchKernelGGL(k_ledger_sweep<LEDGER_CENSUS>, grid, block, 0, ctx->stream, M, S, first, last, parts); break;
  }
  hipLaunchKernelGGL(k_ledger_final, dim3(1), block, 0, ctx->stream, (const unsigned long long *)parts, (int)blocks, what,
                     ctx->ledger_d);
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

extern "C" jb_status jb_ledger_accumulate(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, int64_t first,
                                          int64_t last, int what) {
  if (!ctx || !mesh || !swarm) return fail(JB_ERR_INVALID, "jb_ledger_accumulate: null argument");
  if (!ctx->ledger_on) return fail(JB_ERR_INVALID, "jb_ledger_accumulate: the energy ledger is disabled (jb_ledger_enable)");
  if (what != JB_LEDGER_SOURCED && what != JB_LEDGER_TRANSPORTED)
    return fail(JB_ERR_INVALID, "jb_ledger_accumulate: what = %d is neither JB_LEDGER_SOURCED nor JB_LEDGER_TRANSPORTED", what);
  JB_HIP(hipSetDevice(ctx->device));
  const jb_status st = check_swarm(swarm, "jb_ledger_accumulate");
  if (st != JB_COMPLETE) return st;
  if (first < 0 || last > swarm->n || first > last)
    return fail(JB_ERR_INVALID, "jb_ledger_accumulate: particle range [%lld,%lld) outside the swarm (n = %lld)",
                (long long)first, (long long)last, (long long)swarm->n);
  return ledger_sweep(ctx, mesh->dm, dev_swarm(swarm), first, last,
                      what == JB_LEDGER_SOURCED ? LEDGER_SOURCED : LEDGER_TRANSPORTED);
}

static jb_status ledger_close(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, double t_start, double dt,
                              long long cycle, jb_energy_ledger *out) {
  const DevMesh &M = mesh->dm;
  // (exact deposition: e_delta and e_tally read final fields)
  if (mesh->dep_open) {
    const jb_status dst = deposit_close(ctx, mesh, swarm);
    if (dst != JB_COMPLETE) return dst;
  }
  jb_status st = ledger_sweep(ctx, M, dev_swarm(swarm), 0, swarm->n, LEDGER_CENSUS);
  if (st != JB_COMPLETE) return st;
  {
    unsigned long long *parts = ctx->ledger_d + kLedgerHead;
    int blocks = grid_for(ctx, (long long)M.nblocks * M.ncell);
    if (blocks > ctx->ledger_parts) blocks = ctx->ledger_parts;
    hipLaunchKernelGGL(k_ledger_fields, dim3(blocks), dim3(kBlock), 0, ctx->stream, M, parts);
    hipLaunchKernelGGL(k_ledger_final, dim3(1), dim3(kBlock), 0, ctx->stream, (const unsigned long long *)parts, blocks,
                       -1, ctx->ledger_d);
    JB_HIP(hipGetLastError());
  }
  jb_energy_ledger led;
  memset(&led, 0, sizeof led);
  JB_HIP(hipMemcpyAsync(&led, ctx->ledger_d, LW_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipMemsetAsync(ctx->ledger_d, 0, kLedgerHead * sizeof(unsigned long long), ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  led.t_start = t_start;
  led.dt = dt;
  led.cycle = cycle;
  ctx->ledger_last = led;
  ctx->ledger_has_last = true;
  if (out) *out = led;
  return JB_COMPLETE;
}

extern "C" jb_status jb_ledger_close(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, double t_start,
                                     double dt, jb_energy_ledger *out) {
  if (!ctx || !mesh || !swarm) return fail(JB_ERR_INVALID, "jb_ledger_close: null argument");
  if (!ctx->ledger_on) return fail(JB_ERR_INVALID, "jb_ledger_close: the energy ledger is disabled (jb_ledger_enable)");
  JB_HIP(hipSetDevice(ctx->device));
  const jb_status st = check_swarm(swarm, "jb_ledger_close");
  if (st != JB_COMPLETE) return st;
  return ledger_close(ctx, mesh, swarm, t_start, dt, 0, out);   // (cycle: the host's to set)
}

// The reduction with this rank's verdict on what led to it in front of its ledger: a rank whose close failed
// still makes the collective, and every rank returns that failure (the lowest failing rank's) from the same call.
static jb_status ledger_reduce(jb_context *ctx, const jb_exchange_transport *tr, int rank, int nranks, int replicated,
                               jb_energy_ledger *inout, jb_status local) {
  if (!ctx || !inout) return fail(JB_ERR_INVALID, "jb_ledger_reduce: null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks)
    return fail(JB_ERR_INVALID, "jb_ledger_reduce: rank %d outside [0, nranks = %d)", rank, nranks);
  if (nranks > 1 && (!tr || !tr->all_gather_u64))
    return fail(JB_ERR_INVALID, "jb_ledger_reduce: %d ranks need a transport with all_gather_u64", nranks);
  if (nranks == 1) return local;
  JB_HIP(hipSetDevice(ctx->device));
  const jb_status gst = ledger_gather_room(ctx, nranks);
  if (gst != JB_COMPLETE) return gst;
  unsigned long long *in_d = (unsigned long long *)ctx->ledger_gather.p, *all_d = in_d + kLedgerGatherRow;
  std::vector<unsigned long long> mine((size_t)kLedgerGatherRow, 0), rows((size_t)kLedgerGatherRow * (size_t)nranks, 0);
  mine[0] = local == JB_COMPLETE ? 0ull : (unsigned long long)(-(long long)local);
  memcpy(&mine[1], inout, sizeof *inout);
  JB_HIP(hipMemcpyAsync(in_d, mine.data(), mine.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
  if (tr->all_gather_u64(tr->handle, (const uint64_t *)in_d, (uint64_t *)all_d, kLedgerGatherRow, (void *)ctx->stream) != 0)
    return fail(JB_ERR_HIP, "jb_ledger_reduce: the transport's all-gather failed");
  JB_HIP(hipMemcpyAsync(rows.data(), all_d, rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<jb_energy_ledger> all((size_t)nranks);
  for (int q = 0; q < nranks; ++q) {
    const unsigned long long w = rows[(size_t)q * kLedgerGatherRow];
    if (w != 0) {
      if (q == rank) return local;            // (jb_last_error: this rank's own reason)
      return fail((jb_status)(-(long long)w), "jb_ledger_reduce: rank %d failed to close its ledger (status %d)", q,
                  -(int)(long long)w);
    }
    memcpy(&all[(size_t)q], &rows[(size_t)q * kLedgerGatherRow + 1], sizeof(jb_energy_ledger));
  }
  // in rank order, from rank 0's: the same bits on every rank (cycle, t_start, dt are the same on all)
  jb_energy_ledger sum = all[0];
  for (int q = 1; q < nranks; ++q) {
    const jb_energy_ledger &r = all[(size_t)q];
    sum.e_sourced += r.e_sourced; sum.n_sourced += r.n_sourced;
    for (int f = 0; f < 6; ++f) { sum.e_escaped[f] += r.e_escaped[f]; sum.n_escaped[f] += r.n_escaped[f]; }
    sum.e_escaped_unclassified += r.e_escaped_unclassified; sum.n_escaped_unclassified += r.n_escaped_unclassified;
    sum.e_absorbed += r.e_absorbed; sum.n_absorbed += r.n_absorbed;
    sum.e_census += r.e_census; sum.n_census += r.n_census;
    if (!replicated) {   // (replicated mesh: every rank holds the all-reduced fields; rank 0's stand for all)
      sum.e_tally += r.e_tally; sum.e_delta += r.e_delta; sum.e_material += r.e_material;
    }
  }
  *inout = sum;
  if (ctx->ledger_on) {
    ctx->ledger_last = sum;
    ctx->ledger_has_last = true;
  }
  return JB_COMPLETE;
}

extern "C" jb_status jb_ledger_reduce(jb_context *ctx, const jb_exchange_transport *tr, int rank, int nranks,
                                      int replicated, jb_energy_ledger *inout) {
  return ledger_reduce(ctx, tr, rank, nranks, replicated, inout, JB_COMPLETE);
}

extern "C" jb_status jb_ledger_last(const jb_context *ctx, jb_energy_ledger *out) {
  if (!ctx || !out) return fail(JB_ERR_INVALID, "jb_ledger_last: null argument");
  if (!ctx->ledger_on) return fail(JB_ERR_INVALID, "jb_ledger_last: the energy ledger is disabled (jb_ledger_enable)");
  if (!ctx->ledger_has_last) return fail(JB_ERR_INVALID, "jb_ledger_last: no cycle has been closed yet");
  *out = ctx->ledger_last;
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
// Exact deposition (include/jaybenne_amd.h: jb_set_deposition; jb_kernel_deposit.hpp).

// (every launch of a kernel of jb_kernel_deposit.hpp is counted: jb_deposit_kernel_launches)
#define JB_DEP_LAUNCH(ctx, ...)          \
  do {                                   \
    hipLaunchKernelGGL(__VA_ARGS__);     \
    ++(ctx)->dep_launches;               \
  } while (0)

// the accumulators, their control words, the decoy energy_delta field and the view that names it: once per mesh
static jb_status deposit_ensure(jb_context *ctx, jb_mesh *mesh) {
  if (mesh->dep_ready) return JB_COMPLETE;
  const DevMesh &M = mesh->dm;
  const size_t cells = (size_t)M.nblocks * (size_t)M.ncell, per = (size_t)M.ntot;
  unsigned long long *acc = nullptr;
  double *decoy = nullptr;
  JB_HIP(hipMalloc(&acc, (cells * kDepWords + DC_N) * sizeof(unsigned long long)));
  mesh->owned.push_back(acc);
  JB_HIP(hipMalloc(&decoy, sizeof(double) * per * (size_t)M.nblocks));
  mesh->owned.push_back(decoy);
  JB_HIP(hipMemsetAsync(acc, 0, (cells * kDepWords + DC_N) * sizeof(unsigned long long), ctx->stream));
  JB_HIP(hipMemsetAsync(decoy, 0, sizeof(double) * per * (size_t)M.nblocks, ctx->stream));
  std::vector<const double *> tab((size_t)M.nblocks);
  for (int b = 0; b < M.nblocks; ++b) tab[(size_t)b] = decoy + (size_t)b * per;
  const double *const *tab_d = nullptr;
  jb_status st = upload(mesh, (const double *const *)tab.data(), (size_t)M.nblocks, &tab_d);
  if (st != JB_COMPLETE) return st;
  mesh->dm_x = mesh->dm;
  mesh->dm_x.edelta = (double *const *)tab_d;
  const DevMesh *copy = nullptr;
  if ((st = upload(mesh, &mesh->dm_x, 1, &copy)) != JB_COMPLETE) return st;
  mesh->dm_x_dev = copy;
  mesh->dep_acc = acc;
  mesh->dep_ctl = acc + cells * kDepWords;
  mesh->dep_ready = true;
  mesh->dep_bytes = (cells * kDepWords + DC_N) * sizeof(unsigned long long) + sizeof(double) * per * (size_t)M.nblocks +
                    sizeof(double *) * (size_t)M.nblocks + sizeof(DevMesh);
  return JB_COMPLETE;
}

static int deposit_grid(const jb_context *ctx, long long n) {
  const long long tile = (long long)kLedgerUnroll * kBlock;
  long long blocks = (n + tile - 1) / tile;
  const long long cap = (long long)ctx->num_cu * 8;
  return (int)(blocks > cap ? cap : (blocks < 1 ? 1 : blocks));
}

template <int WHAT>
static void launch_deposit_sweep(jb_context *ctx, const jb_mesh *mesh, const DevSwarm &S, long long first,
                                 long long last) {
  const DevMesh &M = mesh->dm;
  const dim3 grid((unsigned)deposit_grid(ctx, last - first)), block(kBlock);
  if ((long long)M.nblocks * M.ncell <= (long long)kDepositLds)
    JB_DEP_LAUNCH(ctx, (k_deposit_sweep<WHAT, true>), grid, block, 0, ctx->stream, M, S, first, last, mesh->dep_acc,
                       mesh->dep_ctl);
  else
    JB_DEP_LAUNCH(ctx, (k_deposit_sweep<WHAT, false>), grid, block, 0, ctx->stream, M, S, first, last, mesh->dep_acc,
                       mesh->dep_ctl);
}

// One sweep of [first, last) into the mesh's accumulators; the first one after a close takes the cycle's scale
// over [0, swarm->n) in front of it.
static jb_status deposit_sweep(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, long long first,
                               long long last, int what) {
  jb_status st = deposit_ensure(ctx, mesh);
  if (st != JB_COMPLETE) return st;
  const DevSwarm S = dev_swarm(swarm);
  mesh->dep_swarm = *swarm;
  if (!mesh->dep_open) {
    JB_HIP(hipMemsetAsync(mesh->dep_ctl, 0, DC_N * sizeof(unsigned long long), ctx->stream));
    if (swarm->n > 0)
      JB_DEP_LAUNCH(ctx, k_deposit_scale<false>, dim3(deposit_grid(ctx, swarm->n)), dim3(kBlock), 0, ctx->stream, S,
                         0ll, (long long)swarm->n, mesh->dep_ctl, (int)DC_SCALE);
    deposit_mark_open(ctx, mesh);
  } else if (last > first) {
    // (a later sweep of the cycle: a heavier weight in its range raises the scale, jb_kernel_deposit.hpp)
    const DevMesh &M = mesh->dm;
    const long long cells = (long long)M.nblocks * M.ncell;
    JB_DEP_LAUNCH(ctx, k_deposit_scale<false>, dim3(deposit_grid(ctx, last - first)), dim3(kBlock), 0, ctx->stream, S,
                       first, last, mesh->dep_ctl, (int)DC_SCALE_NEW);
    JB_DEP_LAUNCH(ctx, k_deposit_rescale, dim3(grid_for(ctx, cells)), dim3(kBlock), 0, ctx->stream, cells, mesh->dep_acc,
                       mesh->dep_ctl);
    JB_DEP_LAUNCH(ctx, k_deposit_commit, dim3(1), dim3(1), 0, ctx->stream, mesh->dep_ctl);
  }
  if (last > first) {
    switch (what) {
    case DEP_ABSORBED: launch_deposit_sweep<DEP_ABSORBED>(ctx, mesh, S, first, last); break;
    case DEP_ARRIVALS: launch_deposit_sweep<DEP_ARRIVALS>(ctx, mesh, S, first, last); break;
    default: launch_deposit_sweep<DEP_BOTH>(ctx, mesh, S, first, last); break;
    }
  }
  JB_HIP(hipGetLastError());
  return JB_COMPLETE;
}

// the control words on the host (one synchronisation); a set top bit is the overflow of an accumulator
static jb_status deposit_read_ctl(jb_context *ctx, jb_mesh *mesh, unsigned long long (&ctl)[DC_N], const char *stage) {
  JB_HIP(hipMemcpyAsync(ctl, mesh->dep_ctl, sizeof ctl, hipMemcpyDeviceToHost, ctx->stream));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  if (ctl[DC_TOP_BIT] != 0) {
    // (nothing of THIS stage has been written to a field -- an overflow of the census stage comes after energy_delta
    // has its deposits --; the accumulators start over: the stage's sums are lost with the error)
    const size_t cells = (size_t)mesh->dm.nblocks * (size_t)mesh->dm.ncell;
    (void)hipMemsetAsync(mesh->dep_acc, 0, (cells * kDepWords + DC_N) * sizeof(unsigned long long), ctx->stream);
    deposit_mark_closed(ctx, mesh);
    return fail(JB_ERR_INVALID, "jb_deposit_close: an accumulator of the %s stage overflowed (%llu adds reached the top bit)",
                stage, ctl[DC_TOP_BIT]);
  }
  return JB_COMPLETE;
}

static jb_status deposit_close(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm) {
  jb_status st = deposit_ensure(ctx, mesh);
  if (st != JB_COMPLETE) return st;
  const DevMesh &M = mesh->dm;
  const DevSwarm S = dev_swarm(swarm);
  const dim3 cgrid((unsigned)grid_for(ctx, (long long)M.nblocks * M.ncell)), block(kBlock);
  unsigned long long ctl[DC_N] = {};
  jb_deposit_stats stats{};
  // 1. what the cycle absorbed, into energy_delta
  if (mesh->dep_open) {
    if ((st = deposit_read_ctl(ctx, mesh, ctl, "energy_delta")) != JB_COMPLETE) return st;
    const int E = ctl[DC_SCALE] != 0 ? (int)ctl[DC_SCALE] : 1;
    stats.n_absorbed_addends = (int64_t)ctl[DC_N_ABSORBED];
    stats.n_truncated = (int64_t)ctl[DC_N_TRUNCATED];
    stats.n_rejected = (int64_t)ctl[DC_N_REJECTED];
    stats.scale_absorbed = E;
    if (ctl[DC_N_ABSORBED] != 0)
      JB_DEP_LAUNCH(ctx, k_deposit_final<0>, cgrid, block, 0, ctx->stream, M, mesh->dep_acc, E);
    deposit_mark_closed(ctx, mesh);
  }
  // 2. the census, through the same accumulators (zero again), into energy_tally
  JB_HIP(hipMemsetAsync(mesh->dep_ctl, 0, DC_N * sizeof(unsigned long long), ctx->stream));
  if (swarm->n > 0) {
    JB_DEP_LAUNCH(ctx, k_deposit_scale<true>, dim3(deposit_grid(ctx, swarm->n)), block, 0, ctx->stream, S, 0ll,
                       (long long)swarm->n, mesh->dep_ctl, (int)DC_SCALE);
    launch_deposit_sweep<DEP_CENSUS>(ctx, mesh, S, 0, swarm->n);
  }
  JB_HIP(hipGetLastError());
  if ((st = deposit_read_ctl(ctx, mesh, ctl, "energy_tally")) != JB_COMPLETE) return st;
  const int Et = ctl[DC_SCALE] != 0 ? (int)ctl[DC_SCALE] : 1;
  JB_DEP_LAUNCH(ctx, k_deposit_final<1>, cgrid, block, 0, ctx->stream, M, mesh->dep_acc, Et);
  JB_HIP(hipGetLastError());
  stats.n_census_addends = (int64_t)ctl[DC_N_CENSUS];
  stats.n_truncated += (int64_t)ctl[DC_N_TRUNCATED];
  stats.n_rejected += (int64_t)ctl[DC_N_REJECTED];
  stats.scale_census = Et;
  ctx->dep_last = stats;
  ctx->dep_has_last = true;
  return JB_COMPLETE;
}

extern "C" jb_status jb_deposit_accumulate(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm, int64_t first,
                                           int64_t last, int what) {
  if (!ctx || !mesh || !swarm) return fail(JB_ERR_INVALID, "jb_deposit_accumulate: null argument");
  if (ctx->deposition != JB_DEPOSIT_EXACT)
    return fail(JB_ERR_INVALID, "jb_deposit_accumulate: deposition is not exact (jb_set_deposition)");
  if (what < JB_DEPOSIT_ABSORBED || what > (JB_DEPOSIT_ABSORBED | JB_DEPOSIT_ARRIVALS))
    return fail(JB_ERR_INVALID, "jb_deposit_accumulate: what = %d is no sum of JB_DEPOSIT_ABSORBED and JB_DEPOSIT_ARRIVALS", what);
  JB_HIP(hipSetDevice(ctx->device));
  const jb_status st = check_swarm(swarm, "jb_deposit_accumulate");
  if (st != JB_COMPLETE) return st;
  if (first < 0 || last > swarm->n || first > last)
    return fail(JB_ERR_INVALID, "jb_deposit_accumulate: particle range [%lld,%lld) outside the swarm (n = %lld)",
                (long long)first, (long long)last, (long long)swarm->n);
  static_assert(JB_DEPOSIT_ABSORBED == DEP_ABSORBED && JB_DEPOSIT_ARRIVALS == DEP_ARRIVALS && DEP_BOTH == 3, "");
  return deposit_sweep(ctx, mesh, swarm, first, last, what);
}

extern "C" jb_status jb_deposit_close(jb_context *ctx, jb_mesh *mesh, const jb_swarm_view *swarm) {
  if (!ctx || !mesh || !swarm) return fail(JB_ERR_INVALID, "jb_deposit_close: null argument");
  if (ctx->deposition != JB_DEPOSIT_EXACT)
    return fail(JB_ERR_INVALID, "jb_deposit_close: deposition is not exact (jb_set_deposition)");
  JB_HIP(hipSetDevice(ctx->device));
  const jb_status st = check_swarm(swarm, "jb_deposit_close");
  if (st != JB_COMPLETE) return st;
  return deposit_close(ctx, mesh, swarm);
}

extern "C" int64_t jb_deposit_memory(const jb_mesh *mesh) { return mesh ? (int64_t)mesh->dep_bytes : 0; }
extern "C" int64_t jb_deposit_kernel_launches(const jb_context *ctx) { return ctx ? (int64_t)ctx->dep_launches : 0; }

extern "C" jb_status jb_deposit_last(jb_context *ctx, jb_deposit_stats *out) {
  if (!ctx || !out) return fail(JB_ERR_INVALID, "jb_deposit_last: null argument");
  if (ctx->deposition != JB_DEPOSIT_EXACT)
    return fail(JB_ERR_INVALID, "jb_deposit_last: deposition is not exact (jb_set_deposition)");
  if (!ctx->dep_has_last) return fail(JB_ERR_INVALID, "jb_deposit_last: no close yet");
  JB_HIP(hipSetDevice(ctx->device));
  JB_HIP(hipStreamSynchronize(ctx->stream));
  *out = ctx->dep_last;
  return JB_COMPLETE;
}

// ------------------------------------------------------------------------------------------------
// RadiationStep for a mesh held entirely by this rank: the task list of jaybenne.cpp:104-138 with
// the iterate-sublist collapsed to one launch (every block crossing is resolved in flight).
static jb_status radiation_step(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm, double t_start, double dt,
                                uint64_t *next_id, uint32_t *cycle, int32_t *prefix_dev) {
  if (!ctx || !mesh || !swarm || !next_id || !cycle) return fail(JB_ERR_INVALID, "null argument");
  const DevMesh &M = mesh->dm;
  if (M.nblocks != M.nblocks_total || mesh->nranks_seen != 1)
    return fail(JB_ERR_INVALID, "jb_radiation_step needs the whole mesh on one rank");
  if (*cycle >= (1u << 19) - 1u)   // (SourceEpoch: emission keys k and in-cycle thermal keys (1 << 19) | k must not meet)
    return fail(JB_ERR_INVALID, "jb_radiation_step: cycle counter %u at the limit of the source epochs (2^19 - 1)", *cycle);
  *cycle += 1;   // (keys the per-cell rounding streams of this cycle's emission source: SourceEpoch)
  JB_RANGE("Jaybenne::Timestep");               // jaybenne.cpp:87 ... :145
  jb_status st = jb_update_derived_transport_fields(ctx, mesh, dt);
  if (st != JB_COMPLETE) return st;
  const bool bs_on = bsource_on(ctx);
  if (ctx->params.do_emission || bs_on) {
    // Per block b: n_em[b] emission photons, then n_bs[b] boundary photons, take consecutive stream ids; in the
    // swarm the boundary photons lie behind all emission photons of the call.  Both counts come first.
    const int64_t n_before = swarm->n;
    std::vector<int32_t> nper(M.nblocks, 0), nper_bs(M.nblocks, 0);
    if (ctx->params.do_emission) {
      if (!prefix_dev) return fail(JB_ERR_INVALID, "emission source needs the prefix workspace");
      st = jb_source_photons_count(ctx, mesh, JB_SOURCE_EMISSION, dt, M.nblocks, *cycle, nper.data(),
                                   prefix_dev);
      if (st != JB_COMPLETE) return st;
    }
    if (bs_on) {
      jb_boundary_source_plan bp{};
      bp.nper_block = nper_bs.data();
      st = jb_source_boundary_count(ctx, mesh, dt, ctx->bs_face_cells_total, ctx->bs_num_particles, *cycle, &bp,
                                    nullptr);
      if (st != JB_COMPLETE) return st;
    }
    std::vector<int64_t> slot(M.nblocks), slot_bs(M.nblocks);
    std::vector<uint64_t> ids(M.nblocks), ids_bs(M.nblocks);
    int64_t tot = 0, tot_bs = 0;
    for (int b = 0; b < M.nblocks; ++b) {
      slot[b] = swarm->n + tot;
      ids[b] = *next_id + (uint64_t)(tot + tot_bs);
      ids_bs[b] = ids[b] + (uint64_t)nper[b];
      tot += nper[b];
      tot_bs += nper_bs[b];
    }
    for (int64_t b = 0, run = 0; b < M.nblocks; ++b) { slot_bs[b] = swarm->n + tot + run; run += nper_bs[b]; }
    if (swarm->n + tot + tot_bs > swarm->capacity)
      return fail(JB_ERR_CAPACITY, "swarm capacity %lld too small for %lld new particles",
                  (long long)swarm->capacity, (long long)(tot + tot_bs));
    if (ctx->params.do_emission) {
      st = jb_source_photons_fill(ctx, mesh, swarm, JB_SOURCE_EMISSION, t_start, dt, nper.data(),
                                  prefix_dev, slot.data(), ids.data());
      if (st != JB_COMPLETE) return st;
    }
    if (bs_on) {
      st = jb_source_boundary_fill(ctx, mesh, swarm, t_start, dt, nper_bs.data(), (int32_t *)ctx->bs_prefix.p, slot_bs.data(),
                                   ids_bs.data());
      if (st != JB_COMPLETE) return st;
    }
    swarm->n += tot + tot_bs;
    *next_id += (uint64_t)(tot + tot_bs);
    if (ctx->ledger_on && (st = ledger_sweep(ctx, M, dev_swarm(swarm), n_before, swarm->n, LEDGER_SOURCED)) != JB_COMPLETE)
      return st;
  }
  st = jb_zero_energy_tally(ctx, mesh);
  if (st != JB_COMPLETE) return st;
  jb_transport_stats before;
  st = jb_get_transport_stats(ctx, &before, 0);
  if (st != JB_COMPLETE) return st;
  {
    JB_RANGE("Jaybenne::TransportLoop");        // jaybenne.cpp:115 ... :127 (one pass: every crossing is resolved in flight)
    st = transport_impl(ctx, mesh, swarm, t_start, dt, 0, swarm->n, 1, ctx->params.use_ddmc != 0);
  }
  if (st != JB_COMPLETE) return st;
  // (energy ledger: what this launch absorbed and let escape, before the compaction closes those slots)
  if (ctx->ledger_on && (st = ledger_sweep(ctx, M, dev_swarm(swarm), 0, swarm->n, LEDGER_TRANSPORTED)) != JB_COMPLETE)
    return st;
  jb_transport_stats after;
  st = jb_get_transport_stats(ctx, &after, 0);
  if (st != JB_COMPLETE) return st;
  if (after.n_outgoing != before.n_outgoing)
    return fail(JB_ERR_INVALID, "particles left for another rank in a single-rank step");
  if (after.n_absorbed != before.n_absorbed || after.n_escaped != before.n_escaped) {
    st = jb_remove_marked_particles(ctx, swarm);
    if (st != JB_COMPLETE) return st;
  }
  if (ctx->deposition == JB_DEPOSIT_EXACT && (st = deposit_close(ctx, mesh, swarm)) != JB_COMPLETE) return st;
  st = jb_update_fluid(ctx, mesh);
  if (st != JB_COMPLETE || !ctx->ledger_on) return st;
  return ledger_close(ctx, mesh, swarm, t_start, dt, (long long)*cycle, nullptr);
}

extern "C" jb_status jb_radiation_step(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm,
                                       double t_start, double dt, uint64_t *next_id, uint32_t *cycle,
                                       int32_t *prefix_dev) {
#ifdef JB_INVARIANTS
  // (checked build) tasks accumulate, steps report: JB_ERR_INVARIANT when the count rose during the step
  if (!ctx) return fail(JB_ERR_INVALID, "null argument");
  JB_HIP(hipSetDevice(ctx->device));
  int64_t v0 = 0, v1 = 0;
  jb_status st = inv_violations(ctx, &v0);
  if (st != JB_COMPLETE) return st;
  st = radiation_step(ctx, mesh, swarm, t_start, dt, next_id, cycle, prefix_dev);
  const jb_status ist = inv_violations(ctx, &v1);
  if (ist != JB_COMPLETE) return ist;
  if (v1 > v0) return inv_fail(ctx, v1 - v0, "jb_radiation_step");
  return st;
#else
  return radiation_step(ctx, mesh, swarm, t_start, dt, next_id, cycle, prefix_dev);
#endif
}

// ------------------------------------------------------------------------------------------------
// RadiationStep across ranks: the task list of jaybenne.cpp:104-138 with the iterate-sublist of :113-131
// (transport -> MeshSend / MeshReceive -> SampleDDMCBlockFace -> global completion test) inside the call,
// step for step what jaybenne_amd/jaybenne.py drives through the task entry points.

// a hand-off record buffer of the library's own, grown to at least `records` (its contents are not kept)
static long long records_cap(const DevBuf &b) { return (long long)(b.bytes / (kRecWords * sizeof(long long))); }
static jb_status ensure_records(DevBuf &b, long long records) {
  char what[96];
  snprintf(what, sizeof what, "hipMalloc of a hand-off buffer of %lld records", records);
  return dev_grow(b, (size_t)records * kRecWords * sizeof(long long), what);
}

// room for n_slots particles: the host's reserve, if it gave one
static jb_status step_reserve(const jb_rank_comm *comm, jb_swarm_view *swarm, int64_t n_slots) {
  if (n_slots <= swarm->capacity) return JB_COMPLETE;
  if (comm->reserve && comm->reserve(comm->host, swarm, n_slots) == 0 && swarm->capacity >= n_slots)
    return check_swarm(swarm, "jb_radiation_step_ranks (after reserve)");
  return fail(JB_ERR_CAPACITY, "swarm capacity %lld too small for %lld particles%s", (long long)swarm->capacity,
              (long long)n_slots, comm->reserve ? " (reserve did not make the room)" : "");
}

extern "C" jb_status jb_radiation_step_ranks(jb_context *ctx, jb_mesh *mesh, jb_swarm_view *swarm,
                                             double t_start, double dt, uint64_t *next_id, uint32_t *cycle,
                                             int32_t *prefix_dev, const jb_rank_comm *comm,
                                             jb_step_report *report) {
  // what is the same on every rank (or makes a collective impossible): checked before any of them
  if (!comm) return fail(JB_ERR_INVALID, "jb_radiation_step_ranks: null comm");
  const int rank = comm->rank, nranks = comm->nranks;
  if (nranks < 1 || rank < 0 || rank >= nranks)
    return fail(JB_ERR_INVALID, "jb_radiation_step_ranks: rank %d outside [0, nranks = %d)", rank, nranks);
  const jb_exchange_transport *tr = comm->transport;
  if (nranks > 1 && (!tr || !tr->all_gather_u64 || !tr->all_to_all_v))
    return fail(JB_ERR_INVALID, "jb_radiation_step_ranks: %d ranks need a transport with both collectives", nranks);
  if (!ctx || !mesh || !swarm || !next_id || !cycle)
    return fail(JB_ERR_INVALID, "jb_radiation_step_ranks: null argument");
  if (ctx->source_allocation == JB_ALLOC_ENERGY)   // (the mode is a property of the call that all ranks share)
    return fail(JB_ERR_UNSUPPORTED, "jb_radiation_step_ranks: source allocation energy is not driven by this call "
                "(the hosts source through jb_source_energy_sums / jb_source_photons_count_energy)");
  const DevMesh &M = mesh->dm;
  if (nranks > 1 && mesh->one_owner)
    return fail(JB_ERR_INVALID, "jb_radiation_step_ranks: every block of the mesh view has the same owner -- a "
                "replicated (or single-rank) mesh, which this call does not drive across %d ranks", nranks);
  if (nranks < mesh->nranks_seen || nranks + 3 > kRankEnd - kRankBase)
    return fail(JB_ERR_INVALID, "jb_radiation_step_ranks: nranks = %d does not cover the owners in the mesh view", nranks);
  JB_HIP(hipSetDevice(ctx->device));
  const bool multi = nranks > 1;
  const bool ddmc = ctx->params.use_ddmc != 0;
  jb_step_report rep{};
  auto done = [&](jb_status st) {
    if (report) *report = rep;
    return st;
  };
  JB_RANGE("Jaybenne::Timestep");               // jaybenne.cpp:87 ... :145
  const uint32_t epoch = *cycle + 1;             // (*cycle advances once every rank got this far)
  const size_t row = 1 + (size_t)M.nblocks_total;   // what a rank puts into the first all-gather
  std::vector<int32_t> nper(M.nblocks, 0), nper_bs(M.nblocks, 0);
  const bool bs_on = bsource_on(ctx);   // (the same faces on every rank, like the ledger)
  // this rank's part up to the first collective: a failure goes into the gathered status word
  auto local_part = [&]() -> jb_status {
    // the gather buffer first (without it this rank could not say anything: the one failure it cannot
    // share), then the rest of what the step allocates
    const size_t words = row * (size_t)(nranks + 1);
    jb_status st = JB_COMPLETE;
    if (multi && (st = dev_grow(ctx->step_gather, words * sizeof(unsigned long long),
                                "jb_radiation_step_ranks: hipMalloc of the gather buffer")) != JB_COMPLETE)
      return st;
    if ((st = check_swarm(swarm, "jb_radiation_step_ranks")) != JB_COMPLETE) return st;
    if (M.rank != rank)
      return fail(JB_ERR_INVALID, "jb_radiation_step_ranks: comm rank %d is not the mesh view's rank %d", rank, M.rank);
    if (*cycle >= (1u << 19) - 1u)   // (SourceEpoch, as jb_radiation_step)
      return fail(JB_ERR_INVALID, "jb_radiation_step_ranks: cycle counter %u at the limit of the source epochs (2^19 - 1)", *cycle);
    if (ctx->params.do_emission && !prefix_dev)
      return fail(JB_ERR_INVALID, "emission source needs the prefix workspace");
    if (multi) {
      if ((st = ensure_count_matrix(ctx, nranks)) != JB_COMPLETE) return st;
      if (!ctx->step_send.p || !ctx->step_recv.p) {
        // (JB_HANDOFF_MIN_RECORDS: a small first size, so that the tests walk through the capacity protocol)
        const long long start = ctx->min_records > 0 ? ctx->min_records : (swarm->n / 16 > 4096 ? swarm->n / 16 : 4096);
        if ((st = ensure_records(ctx->step_send, start)) != JB_COMPLETE) return st;
        if ((st = ensure_records(ctx->step_recv, start)) != JB_COMPLETE) return st;
      }
    }
    if ((st = jb_update_derived_transport_fields(ctx, mesh, dt)) != JB_COMPLETE) return st;
    if (ctx->params.do_emission) {
      // SourcePhotons (md.nowned blocks in the call, sourcing.cpp:68-69); halo copies source nothing
      st = jb_source_photons_count(ctx, mesh, JB_SOURCE_EMISSION, dt, mesh->nowned, epoch, nper.data(), prefix_dev);
      if (st != JB_COMPLETE) return st;
      int64_t tot = 0;
      for (int b = 0; b < M.nblocks; ++b) tot += nper[b];
      if ((st = step_reserve(comm, swarm, swarm->n + tot)) != JB_COMPLETE) return st;
    }
    if (bs_on) {   // the boundary source's count and its room, like the emission's: before the collective
      jb_boundary_source_plan bp{};
      bp.nper_block = nper_bs.data();
      st = jb_source_boundary_count(ctx, mesh, dt, ctx->bs_face_cells_total, ctx->bs_num_particles, epoch, &bp,
                                    nullptr);
      if (st != JB_COMPLETE) return st;
      int64_t tot = 0;
      for (int b = 0; b < M.nblocks; ++b) tot += (int64_t)nper[b] + nper_bs[b];
      if ((st = step_reserve(comm, swarm, swarm->n + tot)) != JB_COMPLETE) return st;
    }
    return JB_COMPLETE;
  };
  const jb_status local = local_part();
  if (multi && !ctx->step_gather.p) return done(local);
  // the first collective: [status | new photons per global block] of every rank
  std::vector<unsigned long long> mine(row, 0), all(row * (size_t)nranks, 0);
  if (local != JB_COMPLETE) {
    mine[0] = (unsigned long long)(-(long long)local);
  } else {
    for (int b = 0; b < M.nblocks; ++b)   // (emission + boundary photons of the block: they take consecutive ids)
      mine[1 + (size_t)mesh->gid_host[b]] = (unsigned long long)nper[b] + (unsigned long long)nper_bs[b];
  }
  if (multi) {
    unsigned long long *in_d = (unsigned long long *)ctx->step_gather.p, *all_d = in_d + row;
    JB_HIP(hipMemcpyAsync(in_d, mine.data(), row * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    if (tr->all_gather_u64(tr->handle, (const uint64_t *)in_d, (uint64_t *)all_d, (int)row, (void *)ctx->stream) != 0)
      return done(fail(JB_ERR_HIP, "jb_radiation_step_ranks: the transport's all-gather of the source counts failed"));
    JB_HIP(hipMemcpyAsync(all.data(), all_d, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    JB_HIP(hipStreamSynchronize(ctx->stream));
  } else {
    all = mine;
  }
  for (int q = 0; q < nranks; ++q) {
    const unsigned long long w = all[(size_t)q * row];
    if (w == 0) continue;
    if (q == rank) return done(local);          // (jb_last_error: this rank's own reason)
    return done(fail((jb_status)(-(long long)w), "jb_radiation_step_ranks: rank %d failed before the step's first "
                     "collective (status %d)", q, -(int)(long long)w));
  }
  *cycle = epoch;   // (keys the per-cell rounding streams of this cycle's emission source: SourceEpoch)
  jb_status st = JB_COMPLETE;
  if (ctx->params.do_emission || bs_on) {
    std::vector<long long> all_counts((size_t)M.nblocks_total, 0);
    for (int q = 0; q < nranks; ++q)
      for (size_t g = 0; g < (size_t)M.nblocks_total; ++g) all_counts[g] += (long long)all[(size_t)q * row + 1 + g];
    jaybenne_amd::SourcePlan pl = jaybenne_amd::PlanSource(nper, mesh->gid_host, all_counts, *next_id, swarm->n);
    if (bs_on) pl = jaybenne_amd::PlanSourceWithBoundary(nper, nper_bs, mesh->gid_host, all_counts, *next_id, swarm->n);
    if (ctx->params.do_emission) {
      st = jb_source_photons_fill(ctx, mesh, swarm, JB_SOURCE_EMISSION, t_start, dt, nper.data(), prefix_dev,
                                  pl.slot_base.data(), pl.id_base.data());
      if (st != JB_COMPLETE) return done(st);
    }
    if (bs_on) {
      st = jb_source_boundary_fill(ctx, mesh, swarm, t_start, dt, nper_bs.data(), (int32_t *)ctx->bs_prefix.p,
                                   pl.slot_base_boundary.data(), pl.id_base_boundary.data());
      if (st != JB_COMPLETE) return done(st);
    }
    swarm->n += pl.total_local;
    *next_id = pl.next_id;
    if (ctx->ledger_on &&
        (st = ledger_sweep(ctx, M, dev_swarm(swarm), swarm->n - pl.total_local, swarm->n, LEDGER_SOURCED)) != JB_COMPLETE)
      return done(st);
  }
  if ((st = jb_zero_energy_tally(ctx, mesh)) != JB_COMPLETE) return done(st);
  jb_transport_stats before;
  if ((st = jb_get_transport_stats(ctx, &before, 0)) != JB_COMPLETE) return done(st);
  bool finished = false;
  {
    JB_RANGE("Jaybenne::TransportLoop");        // jaybenne.cpp:115 ... :127
    constexpr int kExchangeCalls = 4;           // jb_exchange calls per transport iteration (capacity protocol)
    int64_t first = 0;
    for (int it = 0; it < ctx->params.max_transport_iterations; ++it) {
      const int64_t last = swarm->n;
      st = (ddmc ? jb_transport_photons_ddmc : jb_transport_photons)(ctx, mesh, swarm, t_start, dt, first, last, 1);
      if (st != JB_COMPLETE) return done(st);
      // (energy ledger: exactly the range this launch followed, before the hand-off turns packed slots into holes)
      if (ctx->ledger_on && (st = ledger_sweep(ctx, M, dev_swarm(swarm), first, last, LEDGER_TRANSPORTED)) != JB_COMPLETE)
        return done(st);
      ++rep.transport_iterations;
      if (!multi) { finished = true; break; }   // (every block crossing was resolved in flight)
      int64_t nsent = 0, nrecv = 0, moved = 0, xf = first, xl = last;
      for (int call = 1;; ++call) {
        st = jb_exchange(ctx, mesh, swarm, xf, xl, rank, nranks, tr, (int64_t *)ctx->step_send.p, records_cap(ctx->step_send),
                         (int64_t *)ctx->step_recv.p, records_cap(ctx->step_recv), &nsent, &nrecv, &moved);
        if (st != JB_ERR_CAPACITY || call == kExchangeCalls) break;
        // The verdict is the same on every rank: each makes the room IT lacks and all call again.  A failure
        // to grow leaves the room short, and the next verdict -- again the same everywhere -- says so.
        ++rep.capacity_rounds;
        if (nsent > records_cap(ctx->step_send)) (void)ensure_records(ctx->step_send, nsent * 3 / 2 + 16);
        if (nrecv > records_cap(ctx->step_recv)) (void)ensure_records(ctx->step_recv, nrecv * 3 / 2 + 16);
        if (swarm->n + nrecv > swarm->capacity) {
          // close the holes earlier departures left; what still has to go is found by its status
          if ((st = jb_remove_marked_particles(ctx, swarm)) != JB_COMPLETE) return done(st);
          (void)step_reserve(comm, swarm, swarm->n + nrecv);
          xf = 0;
          xl = swarm->n;
        }
      }
      if (st != JB_COMPLETE) return done(st);
      rep.sent += nsent;
      rep.received += nrecv;
      if (moved == 0) { finished = true; break; }   // CheckCompletion with its global sync (jaybenne.cpp:130-131)
      first = swarm->n - nrecv;                     // the arrivals, appended at the end of the swarm
      if (ddmc && nrecv > 0 && (st = jb_sample_ddmc_block_face(ctx, mesh, swarm, first, swarm->n)) != JB_COMPLETE)
        return done(st);
    }
  }
  if (!finished) return done(JB_ITERATE);
  jb_transport_stats after;
  if ((st = jb_get_transport_stats(ctx, &after, 0)) != JB_COMPLETE) return done(st);
  rep.events = after.n_events - before.n_events;
  if (!multi && after.n_outgoing != before.n_outgoing)
    return done(fail(JB_ERR_INVALID, "particles left for another rank in a single-rank step"));
  if (after.n_absorbed != before.n_absorbed || after.n_escaped != before.n_escaped ||
      after.n_outgoing != before.n_outgoing) {
    if ((st = jb_remove_marked_particles(ctx, swarm)) != JB_COMPLETE) return done(st);
  }
  // (exact deposition: the close is local to the rank, no collective)
  if (ctx->deposition == JB_DEPOSIT_EXACT && (st = deposit_close(ctx, mesh, swarm)) != JB_COMPLETE) return done(st);
  st = jb_update_fluid(ctx, mesh);
  if (st != JB_COMPLETE || !ctx->ledger_on) return done(st);
  // the close, and one more all-gather made on every rank (the ledger is on on all of them or on none)
  // (a rank whose close fails still makes it, with its verdict in front: every rank returns that failure)
  jb_energy_ledger led;
  memset(&led, 0, sizeof led);
  st = ledger_close(ctx, mesh, swarm, t_start, dt, (long long)*cycle, &led);
  return done(ledger_reduce(ctx, tr, rank, nranks, 0, &led, st));
}

// ------------------------------------------------------------------------------------------------
// debug entry points
__global__ void k_dbg_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                             uint32_t k1, uint32_t *out) {
  const PhiloxBlock b = philox4x32_10(c0, c1, c2, c3, k0, k1);
  out[0] = b.w0; out[1] = b.w1; out[2] = b.w2; out[3] = b.w3;
}
__global__ void k_dbg_rocrand(unsigned long long seed, unsigned long long subseq, uint32_t *out) {
  rocrand_state_philox4x32_10 st;
  rocrand_init(seed, subseq, 0ull, &st);
  const uint4 a = rocrand4(&st);
  const uint4 b = rocrand4(&st);
  out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
  out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
}
__global__ void k_dbg_draw(unsigned long long state, int n, double *out, unsigned long long *fin) {
  LcgRng rng(state);
  for (int i = 0; i < n; ++i) out[i] = rng.drand();
  *fin = rng.s;
}
__global__ void k_dbg_seed(uint32_t seed, uint32_t domain, unsigned long long id,
                           unsigned long long *out) {
  *out = rng_seed_state(seed, domain, id);
}
__global__ void k_dbg_stream_start(uint32_t seed, unsigned long long id, unsigned long long *out) {
  *out = rng_stream_start(seed, id);
}
__global__ void k_dbg_math(int which, const double *x, int n, double *out) {
  load_math_tables<true, true, true, true, true>();
  // (cases 18 / 19 carry a shift k in the bits above the low eight: 18 | k << 8)
  const int shift = which >> 8;
  which &= 0xff;
  const double p2 = __longlong_as_double((long long)(1023 + shift) << 52);  // 2^k
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double s, c;
    switch (which) {
    case 0: out[i] = m_log(x[i]); break;
    case 1: m_sincos(x[i], s, c); out[i] = s; break;
    case 2: m_sincos(x[i], s, c); out[i] = c; break;
    case 3: out[i] = m_acos(x[i]); break;
    case 4: out[i] = sqrt(x[i]); break;
    case 5: out[i] = 1.0 / x[i]; break;
    case 6: out[i] = m_sqrt(x[i]); break;
    case 7: out[i] = m_div(x[i], x[(i + 1) % n]); break;
    case 8: out[i] = m_div_r(x[i], 2.99792458e10, m_rcp_refined(2.99792458e10)); break;
    case 9: m_sincos2pi(x[i], s, c); out[i] = s; break;
    case 10: m_sincos2pi(x[i], s, c); out[i] = c; break;
    case 11: out[i] = m_one_minus_exp_neg(x[i]); break;
    case 12: out[i] = x[i] * m_rcp_once(x[(i + 1) % n]); break;   // lean quotient
    case 13: out[i] = m_log_lean(x[i]); break;
    case 15: out[i] = m_log_lean<false, true>(x[i]); break;
    case 16: m_sincos2pi<false, true>(x[i], s, c); out[i] = s; break;   // grid point by the magic constant
    case 17: m_sincos2pi<false, true>(x[i], s, c); out[i] = c; break;
    // what k_imc_cell<.., UNITCELL> asks of the hardware's seeds: the lean reciprocal of x 2^k times 2^k and the
    // lean square root of x 4^k over 2^k are those of x (k = 0), bit for bit
    case 18: out[i] = m_rcp_once(x[i] * p2) * p2; break;
    case 19: out[i] = m_sqrt_lean((x[i] * p2) * p2) / p2; break;
    default: out[i] = m_sqrt_lean(x[i]); break;
    }
  }
}
__global__ void k_dbg_model(DevParams P, int which, const double *x, int n, double *out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double rho = x[3 * i], temp = x[3 * i + 1], nu = x[3 * i + 2];
    out[i] = which == 0 ? opac_absorption(P, rho, temp, nu)
             : which == 1 ? opac_emissivity(P, rho, temp) : opac_scattering(P, rho, temp, nu);
  }
}
__global__ void k_dbg_step(int which, jb_debug_step *d, const double *tape, int ntape, int *ndraws) {
  load_math_tables();
  TapeRng rng(tape, ntape);
  Step s;
  s.t_start = d->t_start; s.dt = d->dt; s.ff = d->ff; s.aa = d->aa; s.ss = d->ss; s.vv = d->vv; s.rvv = m_rcp_refined(d->vv);
  s.dx_push = d->dx_push;
  s.ffaa = s.ff * s.aa;
  s.sig = s.aa + s.ss;
  s.xl = d->xl; s.yl = d->yl; s.zl = d->zl; s.xu = d->xu; s.yu = d->yu; s.zu = d->zu;
  s.Px_l = d->Px_l; s.Py_l = d->Py_l; s.Pz_l = d->Pz_l; s.Px_u = d->Px_u; s.Py_u = d->Py_u; s.Pz_u = d->Pz_u;
  s.t = d->t; s.x = d->x; s.y = d->y; s.z = d->z; s.vx = d->vx; s.vy = d->vy; s.vz = d->vz;
  s.ip = d->ip; s.jp = d->jp; s.kp = d->kp;
  s.is_absorbed = d->is_absorbed != 0; s.is_scattered = d->is_scattered != 0;
  s.is_rejected = d->is_rejected != 0;
  const int nd = d->three_d ? 3 : (d->multi_d ? 2 : 1);
#define DISPATCH(fn)                                   \
  if (nd == 1) fn<1>(s, rng);                          \
  else if (nd == 2) fn<2>(s, rng);                     \
  else fn<3>(s, rng);
  if (which == 0) { DISPATCH(ptcl_transport_step) }
  else if (which == 1) { DISPATCH(ptcl_ddmc_step) }
  else { DISPATCH(ptcl_ddmc_albedo) }
#undef DISPATCH
  d->t = s.t; d->x = s.x; d->y = s.y; d->z = s.z; d->vx = s.vx; d->vy = s.vy; d->vz = s.vz;
  d->ip = s.ip; d->jp = s.jp; d->kp = s.kp;
  d->is_absorbed = s.is_absorbed; d->is_scattered = s.is_scattered; d->is_rejected = s.is_rejected;
  *ndraws = (int)rng.ctr;
}
__global__ void k_dbg_sample(int which, const double *a, const int *iv, const double *tape, int ntape,
                             double *out, int *iout, int *ndraws) {
  load_math_tables();
  TapeRng rng(tape, ntape);
  if (which == 0) {
    scatter(rng, a[0], out[0], out[1], out[2]);
  } else if (which == 1) {
    sample_face_iso_dir(a[0], rng, out[0], out[1], out[2]);
  } else if (which == 2) {
    out[0] = sample_planck_energy(rng, a[0], a[1]);
  } else if (which == 5) {   // the tracking kernels' scatter in direction space, on the tape generator
    scatter_dir(rng, out[0], out[1], out[2]);
  } else if (which == 3) {
    int i = iv[1];
    double x = a[3];
    sample_face_2d(iv[0], a[0], a[1], a[2], rng, i, x);
    iout[0] = i; out[0] = x;
  } else {
    int i1 = iv[2], i2 = iv[3];
    double x1 = a[6], x2 = a[7];
    sample_face_3d(iv[0], iv[1], a[0], a[1], a[2], a[3], a[4], a[5], rng, i1, i2, x1, x2);
    iout[0] = i1; iout[1] = i2; out[0] = x1; out[1] = x2;
  }
  *ndraws = (int)rng.ctr;
}

// small helper: run a debug kernel with device copies of host buffers
struct DbgBuf {
  void *d = nullptr;
  size_t bytes = 0;
  ~DbgBuf() { if (d) (void)hipFree(d); }
  hipError_t put(const void *h, size_t n) {
    bytes = n ? n : 8;
    hipError_t e = hipMalloc(&d, bytes);
    if (e != hipSuccess) return e;
    if (h && n) e = hipMemcpy(d, h, n, hipMemcpyHostToDevice);
    return e;
  }
  hipError_t get(void *h, size_t n) { return hipMemcpy(h, d, n, hipMemcpyDeviceToHost); }
};

extern "C" jb_status jb_debug_philox(jb_context *ctx, const uint32_t ctr[4], const uint32_t key[2],
                                     uint32_t out[4]) {
  if (!ctx) return fail(JB_ERR_INVALID, "null context");
  JB_HIP(hipSetDevice(ctx->device));
  DbgBuf o;
  JB_HIP(o.put(nullptr, 16));
  hipLaunchKernelGGL(k_dbg_philox, dim3(1), dim3(1), 0, ctx->stream, ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], (uint32_t *)o.d);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  JB_HIP(o.get(out, 16));
  return JB_COMPLETE;
}
extern "C" jb_status jb_debug_rocrand_philox(jb_context *ctx, uint64_t seed, uint64_t subsequence,
                                             uint32_t out[8]) {
  if (!ctx) return fail(JB_ERR_INVALID, "null context");
  JB_HIP(hipSetDevice(ctx->device));
  DbgBuf o;
  JB_HIP(o.put(nullptr, 32));
  hipLaunchKernelGGL(k_dbg_rocrand, dim3(1), dim3(1), 0, ctx->stream, (unsigned long long)seed,
                     (unsigned long long)subsequence, (uint32_t *)o.d);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  JB_HIP(o.get(out, 32));
  return JB_COMPLETE;
}
extern "C" jb_status jb_debug_seed_state(jb_context *ctx, uint32_t seed, uint32_t domain,
                                         uint64_t id, uint64_t *state) {
  if (!ctx || !state) return fail(JB_ERR_INVALID, "bad argument");
  JB_HIP(hipSetDevice(ctx->device));
  DbgBuf o;
  JB_HIP(o.put(nullptr, 8));
  hipLaunchKernelGGL(k_dbg_seed, dim3(1), dim3(1), 0, ctx->stream, seed, domain, (unsigned long long)id, (unsigned long long *)o.d);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  JB_HIP(o.get(state, 8));
  return JB_COMPLETE;
}
extern "C" jb_status jb_debug_stream_start(jb_context *ctx, uint32_t seed, uint64_t id,
                                           uint64_t *state) {
  if (!ctx || !state) return fail(JB_ERR_INVALID, "bad argument");
  JB_HIP(hipSetDevice(ctx->device));
  DbgBuf o;
  JB_HIP(o.put(nullptr, 8));
  hipLaunchKernelGGL(k_dbg_stream_start, dim3(1), dim3(1), 0, ctx->stream, seed, (unsigned long long)id, (unsigned long long *)o.d);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  JB_HIP(o.get(state, 8));
  return JB_COMPLETE;
}
extern "C" jb_status jb_debug_draw_stream(jb_context *ctx, uint64_t state, int n, double *out_host,
                                          uint64_t *final_state) {
  if (!ctx || n < 0 || !final_state) return fail(JB_ERR_INVALID, "bad argument");
  JB_HIP(hipSetDevice(ctx->device));
  DbgBuf o, f;
  JB_HIP(o.put(nullptr, sizeof(double) * n));
  JB_HIP(f.put(nullptr, 8));
  hipLaunchKernelGGL(k_dbg_draw, dim3(1), dim3(1), 0, ctx->stream, (unsigned long long)state, n, (double *)o.d, (unsigned long long *)f.d);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  JB_HIP(o.get(out_host, sizeof(double) * n));
  JB_HIP(f.get(final_state, 8));
  return JB_COMPLETE;
}
extern "C" jb_status jb_debug_model_coefficients(jb_context *ctx, double out[4]) {
  if (!ctx || !out) return fail(JB_ERR_INVALID, "bad argument");
  out[0] = ctx->dp.ep_A; out[1] = ctx->dp.ep_B; out[2] = ctx->dp.ep_E; out[3] = ctx->dp.kappa_s;
  return JB_COMPLETE;
}
extern "C" jb_status jb_debug_model_eval(jb_context *ctx, int which, const double *x_host, int n,
                                         double *out_host) {
  if (!ctx || n < 0 || which < 0 || which > 2) return fail(JB_ERR_INVALID, "bad argument");
  JB_HIP(hipSetDevice(ctx->device));
  DbgBuf x, o;
  JB_HIP(x.put(x_host, sizeof(double) * 3 * n));
  JB_HIP(o.put(nullptr, sizeof(double) * n));
  hipLaunchKernelGGL(k_dbg_model, dim3(64), dim3(256), 0, ctx->stream, ctx->dp, which, (const double *)x.d, n, (double *)o.d);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  JB_HIP(o.get(out_host, sizeof(double) * n));
  return JB_COMPLETE;
}
extern "C" jb_status jb_debug_math(jb_context *ctx, int which, const double *x_host, int n,
                                   double *out_host) {
  if (!ctx || n < 0) return fail(JB_ERR_INVALID, "bad argument");
  JB_HIP(hipSetDevice(ctx->device));
  DbgBuf x, o;
  JB_HIP(x.put(x_host, sizeof(double) * n));
  JB_HIP(o.put(nullptr, sizeof(double) * n));
  hipLaunchKernelGGL(k_dbg_math, dim3(64), dim3(256), 0, ctx->stream, which, (const double *)x.d, n, (double *)o.d);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  JB_HIP(o.get(out_host, sizeof(double) * n));
  return JB_COMPLETE;
}
extern "C" jb_status jb_debug_step_call(jb_context *ctx, int which, jb_debug_step *st,
                                        const double *tape, int ntape, int *ndraws) {
  if (!ctx || !st || !tape || ntape < 1 || !ndraws) return fail(JB_ERR_INVALID, "bad argument");
  JB_HIP(hipSetDevice(ctx->device));
  DbgBuf s, t, n;
  JB_HIP(s.put(st, sizeof(*st)));
  JB_HIP(t.put(tape, sizeof(double) * ntape));
  JB_HIP(n.put(nullptr, sizeof(int)));
  hipLaunchKernelGGL(k_dbg_step, dim3(1), dim3(1), 0, ctx->stream, which, (jb_debug_step *)s.d, (const double *)t.d, ntape, (int *)n.d);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  JB_HIP(s.get(st, sizeof(*st)));
  JB_HIP(n.get(ndraws, sizeof(int)));
  return JB_COMPLETE;
}
extern "C" jb_status jb_debug_sample_call(jb_context *ctx, int which, const double *a,
                                          const int32_t *i, const double *tape, int ntape,
                                          double out[4], int32_t iout[2], int *ndraws) {
  if (!ctx || !a || !i || !tape || ntape < 1 || !ndraws) return fail(JB_ERR_INVALID, "bad argument");
  JB_HIP(hipSetDevice(ctx->device));
  DbgBuf da, di, t, o, io, n;
  JB_HIP(da.put(a, sizeof(double) * 8));
  JB_HIP(di.put(i, sizeof(int) * 4));
  JB_HIP(t.put(tape, sizeof(double) * ntape));
  JB_HIP(o.put(nullptr, sizeof(double) * 4));
  JB_HIP(io.put(nullptr, sizeof(int) * 2));
  JB_HIP(n.put(nullptr, sizeof(int)));
  JB_HIP(hipMemset(o.d, 0, sizeof(double) * 4));
  JB_HIP(hipMemset(io.d, 0, sizeof(int) * 2));
  hipLaunchKernelGGL(k_dbg_sample, dim3(1), dim3(1), 0, ctx->stream, which, (const double *)da.d,
                     (const int *)di.d, (const double *)t.d, ntape, (double *)o.d, (int *)io.d, (int *)n.d);
  JB_HIP(hipStreamSynchronize(ctx->stream));
  JB_HIP(o.get(out, sizeof(double) * 4));
  JB_HIP(io.get(iout, sizeof(int) * 2));
  JB_HIP(n.get(ndraws, sizeof(int)));
  return JB_COMPLETE;
}
