// jb_invariants.hpp -- the transport invariants of the reference's debug build, for the checked library.
//
// The reference states them as PARTHENON_DEBUG_REQUIRE (checked in a debug build only):
//   POSITION         transport.cpp:100-105, transport_ddmc.cpp:102-107: at the top of every pass of the
//                    tracking loop the photon is inside its block, x_min <= x <= x_max per axis
//   INDEX            transport.cpp:106-111, transport_ddmc.cpp:108-113: ... and its cell indices are
//                    inside the block's interior range
//   EVENT_OFF_BLOCK  transport.cpp:152, transport_ddmc.cpp:204: no absorption or scattering on the step
//                    that takes the photon off its block
//   FACE_SAMPLE      sample_ddmc_bface.cpp:229-234, 415-420: after block-face resampling the photon is
//                    inside its (new) block.  The reference joins the two bounds of an axis with ||,
//                    which makes the condition always true; it is checked here as intended, with &&.
// and this library adds
//   DDMC_CLASS       after k_ddmc_pack: the class record of every interior cell whose code is a class
//                    number (below max_classes) is bit-equal to the cell's own step record
//   SWARM            a sweep over the photons of a swarm (after SourcePhotons' fill, on entry to each
//                    transport task, and jb_verify_swarm): a defined status; for a resident photon block
//                    in range, indices in the interior (not on entry to transport: an arrival carries
//                    its sender's indices, which tracking recomputes), position inside the block,
//                    w and e finite and >= 0, t <= t_end.
//
// Call sites: POSITION / INDEX at the top of every event pass of k_transport, k_imc_cell, k_ddmc_all, k_ddmc_q
// and both loops of k_hybrid (the cell-local kernels in their own coordinates: the condition is stated at
// each), EVENT_OFF_BLOCK at their block exits, FACE_SAMPLE in k_block_face, k_inv_ddmc_class and k_inv_swarm
// (jb_kernels.hpp).  The "first" violation is the one whose lane won the claim, not the lowest slot.
//
// Every check is a predicate on plain values (host and device: tests/invariants_test.cpp compiles them
// with a host compiler).  The kernels call them through the JB_INV_* macros of jb_kernels.hpp, which
// expand to nothing unless JB_INVARIANTS is defined (make checked: libjaybenne_amd_checked.so), so the
// release library's kernels are the same instructions as without this file.
//
// In the checked build the kernels count into one buffer per process and device (jb_inv_buf,
// allocated by the first jb_initialize): per kind evaluated and violated, per kernel family the lane-
// passes checked.  Counts are aggregated per wave (ballot, popcount, one atomic from one lane) and
// spread over kStripes cache lines by workgroup.  The first violation is claimed with an atomicCAS on
// one word; the claiming lane writes the record with ordinary vector stores.  A violating photon is
// never used as an index: it leaves the tracking loop untallied (its slot keeps the state it had when
// the launch loaded it) and is counted.  No kernel stops on a violation: the host reads the counts.
#pragma once

#include <stdint.h>

#include <cmath>

#include "../../include/jaybenne_amd.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define JB_INV_HD __host__ __device__
#else
#define JB_INV_HD
#endif

namespace jb {
namespace inv {

constexpr int kKinds = JB_INV_NKINDS;
constexpr int kFamilies = JB_INV_NFAMILIES;
constexpr int kStripes = 16;       // workgroup % kStripes picks the cache line of a count
constexpr int kStripeWords = 16;   // 128 bytes per stripe
constexpr int kCountWords = kStripes * kStripeWords;
// the buffer, in 64-bit words: per kind [evaluated][violated], per family [passes], each kCountWords;
// then the claim word of the first violation (in a line of its own) and the record
constexpr int kEvalBase = 0;
constexpr int kViolBase = kKinds * kCountWords;
constexpr int kPassBase = 2 * kKinds * kCountWords;
constexpr int kClaim = kPassBase + kFamilies * kCountWords;
constexpr int kRecord = kClaim + 16;
enum { R_KIND = 0, R_FAMILY, R_BLOCK, R_SLOT, R_ID, R_IP, R_JP, R_KP, R_X, R_Y, R_Z, R_AXIS, kRecordWords };
constexpr int kBufferWords = kRecord + kRecordWords;

// ---- the predicates ------------------------------------------------------------------------------
// (NaN fails every one of them: comparisons with it are false)

// POSITION: lo[d] <= x[d] <= hi[d] on the active axes.  (An inactive axis of a 1-D or 2-D mesh: the
// photon keeps the coordinate it was sourced with and the library keeps no block extent there.)
JB_INV_HD inline bool position_ok(int ndim, const double x[3], const double lo[3], const double hi[3]) {
  bool ok = true;
  for (int d = 0; d < 3; ++d)
    if (d < ndim) ok = ok && x[d] >= lo[d] && x[d] <= hi[d];
  return ok;
}

// the first active axis on which position_ok fails (0 when none does)
JB_INV_HD inline int first_axis_out(int ndim, const double x[3], const double lo[3], const double hi[3]) {
  for (int d = 0; d < 3; ++d)
    if (d < ndim && !(x[d] >= lo[d] && x[d] <= hi[d])) return d;
  return 0;
}

// INDEX: first[d] <= idx[d] <= last[d] on every axis (an inactive axis has first = last)
JB_INV_HD inline bool index_ok(const int idx[3], const int first[3], const int last[3]) {
  return idx[0] >= first[0] && idx[0] <= last[0] && idx[1] >= first[1] && idx[1] <= last[1] &&
         idx[2] >= first[2] && idx[2] <= last[2];
}

// EVENT_OFF_BLOCK, asked on the step that takes the photon off its block
JB_INV_HD inline bool event_off_block_ok(bool is_absorbed, bool is_scattered) {
  return !(is_absorbed || is_scattered);
}

// block number in [0, nblocks)
JB_INV_HD inline bool block_ok(long long b, long long nblocks) { return b >= 0 && b < nblocks; }

// a status the transport tasks define (JB_ST_*)
JB_INV_HD inline bool status_ok(int status) {
  return status >= JB_ST_ACTIVE && status <= JB_ST_OUTGOING_ABSORBED;
}

// SWARM's scalar attributes: w and e finite and >= 0, t <= t_end
JB_INV_HD inline bool attributes_ok(double w, double e, double t, double t_end) {
  return std::isfinite(w) && w >= 0.0 && std::isfinite(e) && e >= 0.0 && t <= t_end;
}

// DDMC_CLASS: the two 8-double records bit-equal
JB_INV_HD inline bool records_equal(const uint64_t a[8], const uint64_t b[8]) {
  bool eq = true;
  for (int q = 0; q < 8; ++q) eq = eq && a[q] == b[q];
  return eq;
}

}  // namespace inv
}  // namespace jb

#if defined(JB_INVARIANTS) && (defined(__HIPCC__) || defined(__HIP__))
namespace jb {
namespace inv {

// the counting buffer of this process on this device (jb_initialize, checked build)
__device__ unsigned long long *jb_inv_buf = nullptr;

__device__ __forceinline__ unsigned long long *count_word(int base, int index) {
  return jb_inv_buf + base + index * kCountWords + (int)(blockIdx.x % kStripes) * kStripeWords;
}

// first violation: the lane that wins the claim writes the record
__device__ __forceinline__ void record_first(int kind, int family, long long b, long long slot, const uint64_t *ids,
                                             int ip, int jp, int kp, double x, double y, double z, int axis = 0) {
  unsigned long long *const B = jb_inv_buf;
  if (atomicCAS(B + kClaim, 0ull, 1ull) != 0ull) return;
  unsigned long long *const r = B + kRecord;
  r[R_KIND] = (unsigned long long)kind;
  r[R_FAMILY] = (unsigned long long)family;
  r[R_BLOCK] = (unsigned long long)b;
  r[R_SLOT] = (unsigned long long)slot;
  r[R_ID] = (ids != nullptr && slot >= 0) ? (unsigned long long)ids[slot] : ~0ull;
  r[R_IP] = (unsigned long long)(long long)ip;
  r[R_JP] = (unsigned long long)(long long)jp;
  r[R_KP] = (unsigned long long)(long long)kp;
  r[R_X] = (unsigned long long)__double_as_longlong(x);
  r[R_Y] = (unsigned long long)__double_as_longlong(y);
  r[R_Z] = (unsigned long long)__double_as_longlong(z);
  r[R_AXIS] = (unsigned long long)axis;
  __threadfence();
}

// one kind evaluated by the lanes where `evaluated`, violated where `evaluated && !ok`: one atomic per
// wave per count (call from every lane that is active at the call site)
__device__ __forceinline__ void count(int kind, bool evaluated, bool ok) {
  const unsigned long long ev = __ballot(evaluated);
  const unsigned long long bad = __ballot(evaluated && !ok);
  const int leader = __ffsll((long long)__ballot(true)) - 1;
  if ((int)(threadIdx.x & 63) == leader) {
    if (ev) atomicAdd(count_word(kEvalBase, kind), (unsigned long long)__popcll(ev));
    if (bad) atomicAdd(count_word(kViolBase, kind), (unsigned long long)__popcll(bad));
  }
}
__device__ __forceinline__ void count_passes(int family, bool running) {
  const unsigned long long ev = __ballot(running);
  const int leader = __ffsll((long long)__ballot(true)) - 1;
  if ((int)(threadIdx.x & 63) == leader && ev)
    atomicAdd(count_word(kPassBase, family), (unsigned long long)__popcll(ev));
}

// POSITION + INDEX at the top of a tracking pass, against the block tables of the mesh (global memory:
// kernels that keep a block copy update only what they use of it).  The block number is range-checked
// before it indexes anything; a bad one counts as an INDEX violation.  Evaluated counts of the two
// kinds are the families' pass counts (the host adds them up).  Returns true for a running lane that
// violates either.
template <class Mesh>
__device__ __forceinline__ bool pass_check(int family, bool running, const Mesh &M, int b, int ip, int jp, int kp,
                                           double x, double y, double z, long long slot, const uint64_t *ids) {
  bool pos = true, idx = true;
  int axis = 0;   // (the first axis that fails: the reference's message names it)
  if (running) {
    const int I[3] = {ip, jp, kp}, first[3] = {M.is, M.js, M.ks}, last[3] = {M.ie, M.je, M.ke};
    idx = block_ok(b, M.nblocks) && index_ok(I, first, last);
    if (block_ok(b, M.nblocks)) {
      const double X[3] = {x, y, z};
      const double lo[3] = {M.blk_xmin[3 * b], M.blk_xmin[3 * b + 1], M.blk_xmin[3 * b + 2]};
      const double hi[3] = {M.blk_xmax[3 * b], M.blk_xmax[3 * b + 1], M.blk_xmax[3 * b + 2]};
      pos = position_ok(M.ndim, X, lo, hi);
      if (!pos) axis = first_axis_out(M.ndim, X, lo, hi);
    }
    if (pos && !idx) axis = !(ip >= M.is && ip <= M.ie) ? 0 : (!(jp >= M.js && jp <= M.je) ? 1 : 2);
  }
  count_passes(family, running);
  const unsigned long long bad_pos = __ballot(running && !pos), bad_idx = __ballot(running && !idx);
  const int leader = __ffsll((long long)__ballot(true)) - 1;
  if ((int)(threadIdx.x & 63) == leader) {
    if (bad_pos) atomicAdd(count_word(kViolBase, JB_INV_POSITION), (unsigned long long)__popcll(bad_pos));
    if (bad_idx) atomicAdd(count_word(kViolBase, JB_INV_INDEX), (unsigned long long)__popcll(bad_idx));
  }
  const bool bad = running && !(pos && idx);
  if (bad) record_first(pos ? JB_INV_INDEX : JB_INV_POSITION, family, b, slot, ids, ip, jp, kp, x, y, z, axis);
  return bad;
}

// POSITION + INDEX at the top of a pass of a kernel that tracks in its own coordinates: the kernel forms the
// two predicates (the condition is documented at the kernel), this counts and records them as pass_check
// does.  Returns true for a running lane that violates either.
__device__ __forceinline__ bool pass_check_pred(int family, bool running, bool pos, bool idx, int axis, int b, int ip,
                                                int jp, int kp, double x, double y, double z, long long slot,
                                                const uint64_t *ids) {
  pos = pos || !running;
  idx = idx || !running;
  count_passes(family, running);
  const unsigned long long bad_pos = __ballot(!pos), bad_idx = __ballot(!idx);
  const int leader = __ffsll((long long)__ballot(true)) - 1;
  if ((int)(threadIdx.x & 63) == leader) {
    if (bad_pos) atomicAdd(count_word(kViolBase, JB_INV_POSITION), (unsigned long long)__popcll(bad_pos));
    if (bad_idx) atomicAdd(count_word(kViolBase, JB_INV_INDEX), (unsigned long long)__popcll(bad_idx));
  }
  const bool bad = !(pos && idx);
  if (bad) record_first(pos ? JB_INV_INDEX : JB_INV_POSITION, family, b, slot, ids, ip, jp, kp, x, y, z, axis);
  return bad;
}

// a cell number (block * ntot + cell, ghost layers included) of the resident blocks: block and cell indices,
// true when it names an interior cell of a resident block (the DDMC kernels' record numbers; the cell-local
// IMC kernels' byte offsets / 8)
template <class Mesh>
__device__ __forceinline__ bool cell_interior(const Mesh &M, unsigned long long c, int &b, int &i, int &j, int &k) {
  const unsigned long long ntot = (unsigned long long)M.ntot;
  b = (int)(c / ntot);
  const long long q = (long long)(c - (unsigned long long)b * ntot);
  k = (int)(q / ((long long)M.ni * M.nj));
  const long long r = q - (long long)k * M.ni * M.nj;
  j = (int)(r / M.ni);
  i = (int)(r - (long long)j * M.ni);
  const int I[3] = {i, j, k}, first[3] = {M.is, M.js, M.ks}, last[3] = {M.ie, M.je, M.ke};
  return block_ok(b, M.nblocks) && index_ok(I, first, last);
}

// POSITION in cell-local coordinates: |p| <= h on the active axes (the photon inside its cell, hence its block)
__device__ __forceinline__ bool local_position_ok(int ndim, const double p[3], const double h[3], int &axis) {
  const double lo[3] = {-h[0], -h[1], -h[2]};
  axis = first_axis_out(ndim, p, lo, h);
  return position_ok(ndim, p, lo, h);
}

// EVENT_OFF_BLOCK at the block-exit branch (called by the lanes in it).  Returns true on a violation.
__device__ __forceinline__ bool off_block_check(int family, bool is_absorbed, bool is_scattered, int b, int ip,
                                                int jp, int kp, double x, double y, double z, long long slot,
                                                const uint64_t *ids) {
  const bool ok = event_off_block_ok(is_absorbed, is_scattered);
  count(JB_INV_EVENT_OFF_BLOCK, true, ok);
  if (!ok) record_first(JB_INV_EVENT_OFF_BLOCK, family, b, slot, ids, ip, jp, kp, x, y, z);
  return !ok;
}

// FACE_SAMPLE after SampleDDMCBlockFace (every lane that resampled calls it)
template <class Mesh>
__device__ __forceinline__ void face_check(const Mesh &M, int b, double x, double y, double z, int ip, int jp,
                                           int kp, long long slot, const uint64_t *ids) {
  bool ok = false;
  int axis = 0;
  if (block_ok(b, M.nblocks)) {
    const double X[3] = {x, y, z};
    const double lo[3] = {M.blk_xmin[3 * b], M.blk_xmin[3 * b + 1], M.blk_xmin[3 * b + 2]};
    const double hi[3] = {M.blk_xmax[3 * b], M.blk_xmax[3 * b + 1], M.blk_xmax[3 * b + 2]};
    ok = position_ok(M.ndim, X, lo, hi);
    if (!ok) axis = first_axis_out(M.ndim, X, lo, hi);
  }
  count_passes(JB_INV_FAM_BLOCK_FACE, true);
  count(JB_INV_FACE_SAMPLE, true, ok);
  if (!ok) record_first(JB_INV_FACE_SAMPLE, JB_INV_FAM_BLOCK_FACE, b, slot, ids, ip, jp, kp, x, y, z, axis);
}

}  // namespace inv
}  // namespace jb

// the call sites in the kernels (nothing at all in the release build)
#define JB_INV_FACE(M, b, x, y, z, ip, jp, kp, slot, ids) ::jb::inv::face_check(M, b, x, y, z, ip, jp, kp, slot, ids)
#define JB_INV_PASS(family, running, M, b, ip, jp, kp, x, y, z, slot, ids, on_violation)                  \
  do {                                                                                                      \
    if (::jb::inv::pass_check(family, running, M, b, ip, jp, kp, x, y, z, slot, ids)) { on_violation; }     \
  } while (0)
#define JB_INV_OFF_BLOCK(family, is_absorbed, is_scattered, b, ip, jp, kp, x, y, z, slot, ids, on_violation) \
  do {                                                                                                      \
    if (::jb::inv::off_block_check(family, is_absorbed, is_scattered, b, ip, jp, kp, x, y, z, slot, ids)) { \
      on_violation;                                                                                         \
    }                                                                                                       \
  } while (0)
#define JB_INV_PASS_PRED(family, running, pos, idx, axis, b, ip, jp, kp, x, y, z, slot, ids, on_violation)      \
  do {                                                                                                      \
    if (::jb::inv::pass_check_pred(family, running, pos, idx, axis, b, ip, jp, kp, x, y, z, slot, ids)) {    \
      on_violation;                                                                                         \
    }                                                                                                       \
  } while (0)
#define JB_INV_STMT(...) __VA_ARGS__
#else
#define JB_INV_PASS_PRED(...) do { } while (0)
#define JB_INV_FACE(...) do { } while (0)
#define JB_INV_PASS(...) do { } while (0)
#define JB_INV_OFF_BLOCK(...) do { } while (0)
#define JB_INV_STMT(...)
#endif
