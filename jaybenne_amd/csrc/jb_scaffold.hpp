// jb_scaffold.hpp -- what the persistent tracking kernels (k_transport, k_imc_cell, k_hybrid, k_ddmc_all,
// k_ddmc_q) share that is not physics: how a wave draws photon slots from the launch's queues, how a workgroup
// keeps and flushes the census tally in LDS, and how finished histories are counted and added to counters[].
// Everything here is __forceinline__ and wave-uniform where it says so: a kernel that uses a piece compiles to
// what it compiled to with the piece written out in its body (registers, scratch and LDS per instantiation are
// held by tests/test_cabi.py).
#pragma once

#include <hip/hip_runtime.h>

#include "jb_device.hpp"

namespace jb {

// counters[]: 0 census, 1 absorbed, 2 escaped, 3 outgoing, 4 events, 5 unfinished
enum { CNT_CENSUS = 0, CNT_ABSORBED, CNT_ESCAPED, CNT_OUTGOING, CNT_EVENTS, CNT_UNFINISHED, CNT_PASSES, CNT_SERVICE, CNT_N };
// Heads of the 8 particle queues of the running transport launch, each in a 128-byte line of its own: the claims
// are returning atomics from every XCD, and atomics on one line are served one after the other -- with the eight
// heads in ONE line (rounds 1 - 5) and 128-slot claims, BASELINE configs[2] as shipped (12-step histories: 7.8e5
// claims per 1e8 photons) ran 10.03 ms whatever else was changed; see DESIGN.md 4.2.
constexpr int CNT_QUEUE = 1024;
constexpr int kQueueStride = 16;
constexpr int kQueues = 8;    // one per XCD (workgroups b and b + 8 share an XCD and its L2)

// lane 0's value in every lane, as a wave-uniform (scalar register) quantity
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v) {
  const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)v);
  const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// -------------------------------------------------------------------------------------------
// The queues.  Particles are dealt from 8 queues, each over one contiguous eighth of the (cell-ordered) range
// [first, last) of the launch.  A workgroup starts on queue blockIdx % 8 -- the workgroups that share an XCD,
// hence an L2 -- and moves on when its queue is drained, so the particles in flight on one XCD form one short
// contiguous window of the swarm and the cell data they gather stays in that XCD's 4 MiB L2.  Placement only
// affects speed, never results.
//
// The wave's cursor over them; every member is wave-uniform (scalar registers).
struct QueueCursor {
  unsigned long long *heads;   // counters + CNT_QUEUE: zeroed by the host before the launch
  long long first, last, per_q;
  int cur;      // queue this wave draws from
  int tried;    // queues found drained so far
  bool more;    // some queue may still hold particles
  __device__ __forceinline__ QueueCursor(unsigned long long *counters, long long first_, long long last_)
      : heads(counters + CNT_QUEUE), first(first_), last(last_), per_q((last_ - first_ + kQueues - 1) / kQueues),
        cur(blockIdx.x % kQueues), tried(0), more(true) {}
  __device__ __forceinline__ unsigned long long *head() const { return &heads[cur * kQueueStride]; }
  // slots [q_first, q_last) of the swarm are the cursor's queue
  __device__ __forceinline__ void range(long long &q_first, long long &q_last) const {
    q_first = first + (long long)cur * per_q;
    q_last = q_first + per_q;
    if (q_last > last) q_last = last;
  }
  // this queue is drained: move on
  __device__ __forceinline__ void next() {
    cur = (cur + 1) % kQueues;
    if (++tried == kQueues) more = false;
  }
};

// The exact claim (k_transport's IMC form, k_imc_cell): one slot per lane of `idle` (the ballot of the idle
// lanes; not empty), one claim of exactly what they need per service phase -- ballot + popcount prefix over the
// idle mask, one returning atomic per wave.  IMC histories are ~1e3 events long: this keeps the particles in
// flight on an XCD one tight window of the swarm and the tail of the launch short.  cand: the slot of this lane
// (its rank among the idle lanes behind the claim's base); returns whether it lies inside the queue.
__device__ __forceinline__ bool claim_exact(QueueCursor &qc, unsigned long long idle, int lane, long long &cand) {
  const int leader = __ffsll((long long)idle) - 1;
  const int want = __popcll(idle);
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(qc.head(), (unsigned long long)want);
  base = __shfl(base, leader, 64);
  long long q_first, q_last;
  qc.range(q_first, q_last);
  cand = q_first + (long long)base + __popcll(idle & ((1ull << lane) - 1ull));
  if (q_first + (long long)base + want >= q_last) qc.next();
  return cand < q_last;
}

// The chunk refill (k_transport's DDMC form, k_hybrid, k_ddmc_all, k_ddmc_q): slots [chunk_pos, chunk_end) of
// the swarm are the wave's to deal out (wave-uniform) over the following service phases; when they are used up
// the wave claims the next CHUNK consecutive slots of its queue with one atomic.  Short DDMC histories claim 128
// at a time (one contended atomic per ~5 service phases); larger chunks lengthen the tail of a hybrid launch
// whose IMC histories are ~1e3 events long.  Returns false when that queue was drained (the cursor has moved on,
// the chunk is empty: the caller goes round again while qc.more), true when the chunk holds slots.  How they are
// dealt to lanes stays with each kernel: the loads sit between the claim and the deal, and a helper that takes
// them as a callable costs k_ddmc_q 36 bytes of scratch per lane.
template <long long CHUNK>
__device__ __forceinline__ bool refill_chunk(QueueCursor &qc, long long &chunk_pos, long long &chunk_end, int lane) {
  if (chunk_pos >= chunk_end) {
    long long q_first, q_last;
    qc.range(q_first, q_last);
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(qc.head(), (unsigned long long)CHUNK);
    chunk_pos = q_first + (long long)uniform_u64(base);
    chunk_end = chunk_pos + CHUNK < q_last ? chunk_pos + CHUNK : q_last;
    if (chunk_pos >= q_last) {
      chunk_pos = chunk_end = 0;
      qc.next();
      return false;
    }
  }
  return true;
}

// -------------------------------------------------------------------------------------------
// The LDS census tally.  Small meshes (the reference's 1-D decks: ~1e2 cells under 1e5..1e8 particles): the
// census tally of every workgroup goes to LDS and is flushed once at the end, instead of 1e8 global atomics
// contending for a handful of cache lines.  lds_tally: the kernel's own __shared__ array (kLdsTally doubles, or
// the head of its dynamic shared memory); tally_in_lds (uniform): whether the mesh is small enough for it.  A
// barrier follows in every kernel before the first photon is loaded (load_math_tables).  (k_ddmc_all and k_ddmc_q
// zero theirs themselves, with the cell count they hold in a register for carving up their dynamic LDS: through
// lds_tally_zero, which reads the mesh view, their 2-D forms take two more vector registers.)
template <bool TALLY>
__device__ __forceinline__ bool lds_tally_fits(const DevMesh &M) {
  return TALLY && (long long)M.nblocks * M.ntot <= (long long)kLdsTally;
}
template <bool TALLY>
__device__ __forceinline__ void lds_tally_zero(const DevMesh &M, double *lds_tally, bool tally_in_lds) {
  if constexpr (TALLY) {
    if (tally_in_lds)
      for (int q = threadIdx.x; q < M.nblocks * (int)M.ntot; q += blockDim.x) lds_tally[q] = 0.0;
  }
}
template <bool TALLY>
__device__ __forceinline__ void lds_tally_flush(const DevMesh &M, const double *lds_tally, bool tally_in_lds) {
  if constexpr (TALLY) {
    if (tally_in_lds) {
      __syncthreads();  // every wave of the workgroup leaves its loop exactly once
      for (int q = threadIdx.x; q < M.nblocks * (int)M.ntot; q += blockDim.x) {
        const double v = lds_tally[q];
        if (v != 0.0) atomicAdd(&M.tally[q / (int)M.ntot][q % (int)M.ntot], v);
      }
    }
  }
}

// -------------------------------------------------------------------------------------------
// Finished histories by outcome.  Either per lane (k_transport, k_imc_cell: counted in the write-back branch,
// summed over the wave at the end) or per wave (k_hybrid, k_ddmc_all, k_ddmc_q: scalar registers, counted from
// ballots outside divergent branches); a kernel uses one form throughout and names it at the flush.
struct OutcomeCounts {
  unsigned int census = 0, absorbed = 0, escaped = 0, outgoing = 0;
  // per lane: this lane's history has ended with `status`
  __device__ __forceinline__ void count(int status) {
    if (status == ST_ACTIVE) ++census;
    else if (status == ST_ABSORBED) ++absorbed;
    else if (status == ST_ESCAPED) ++escaped;
    else ++outgoing;
  }
  // per wave: the lanes with was_done have ended with their `status` (call it where every lane arrives)
  __device__ __forceinline__ void count(bool was_done, int status) {
    const int n_done = __popcll(__ballot(was_done));
    const int n_census = __popcll(__ballot(was_done && status == ST_ACTIVE));
    const int n_abs = __popcll(__ballot(was_done && status == ST_ABSORBED));
    const int n_esc = __popcll(__ballot(was_done && status == ST_ESCAPED));
    census += n_census; absorbed += n_abs; escaped += n_esc;
    outgoing += n_done - n_census - n_abs - n_esc;
  }
  // one atomic per outcome that occurred, from lane 0
  template <bool PER_LANE>
  __device__ __forceinline__ void flush(unsigned long long *counters, int lane) const {
    const unsigned long long r_census = PER_LANE ? wave_sum(census) : census,
                             r_abs = PER_LANE ? wave_sum(absorbed) : absorbed,
                             r_esc = PER_LANE ? wave_sum(escaped) : escaped,
                             r_out = PER_LANE ? wave_sum(outgoing) : outgoing;
    if (lane == 0) {
      if (r_census) atomicAdd(&counters[CNT_CENSUS], r_census);
      if (r_abs) atomicAdd(&counters[CNT_ABSORBED], r_abs);
      if (r_esc) atomicAdd(&counters[CNT_ESCAPED], r_esc);
      if (r_out) atomicAdd(&counters[CNT_OUTGOING], r_out);
    }
  }
};

}  // namespace jb
