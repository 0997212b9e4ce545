// jb_kernel_order.hpp -- the canonical order of the swarm: photons by (resident block, cell) and, within a cell,
// by creation id (include/jaybenne_amd.h: jb_set_cell_order, JB_CELL_ORDER_BY_ID).  The reference has no such task.
//
// A least-significant-digit radix sort of a PERMUTATION: the sort key is (32-bit cell key, 64-bit id, input slot),
// the digits are 8 bits, the id's go first, and every pass is stable -- so the input slot is the last tie-break
// without ever being a digit.  A pass carries 8-byte (word, slot index) pairs: the 32-bit word of the key its
// digit comes from and the slot the pair stands for; the pass that ends a word fetches the next one for the
// pairs it writes (jb_order_plan.hpp), and the last pass writes dest[slot], the inverted permutation, for the move.
//
// Kernel            what it does                                                          bytes per photon
// k_order_check     largest id, largest key, "some slot sorts before its predecessor"     24 read
//   (the one read-back: it decides "not moved at all" and the number of passes)
// k_order_init      the pairs of the first pass                                           4 or 8 read, 8 written
// per pass:
// k_order_count     a workgroup per tile of 2048 slots counts its 256 digit values        8 read
//   (k_scan_tiles / _sums / _add of the sort scan the counts digit-major over all tiles)  ~1/2
// k_order_scatter   re-reads the tile, ranks every pair among those of its digit in the   8 read, 8 written
//                   tile and stores it at base[digit][tile] + rank                        (+ 4 or 8 gathered when
//                                                                                         the word changes)
// k_order_pack      slot s, read in order -> record at dest[s]: the staging of k_sort_pack
//   (k_sort_unpack writes the records back into the swarm arrays)
//
// The rank inside a tile is exact and stable: a wave owns 512 consecutive slots and walks them in 8 rounds of 64;
// in a round the lanes with the same digit find each other by 8 ballots on the digit's bits, a lane's rank is the
// wave's running count of its digit plus the number of such lanes below it, and the lowest of them adds the
// group's size to the running count (in LDS; one writer per digit and round).  The waves' totals are then
// combined in wave order.  No atomic on global memory, no workgroup waits for another, no floating point: the
// same input gives the same permutation whatever the order in which workgroups run.
#pragma once

#include <hip/hip_runtime.h>

#include "jb_kernels.hpp"
#include "jb_order_plan.hpp"

namespace jb {

constexpr int kOrderItems = 8;                    // rounds of a wave
constexpr int kOrderWaveSlots = 64 * kOrderItems; // consecutive slots of a wave
static_assert(kOrderTile == kBlock * kOrderItems && kOrderDigits == kBlock,
              "jb_order_plan.hpp sizes the counts for these tiles; a thread per digit combines the waves' counts");

// the read-back of k_order_check
struct OrderFlags {
  unsigned long long max_id;
  unsigned max_key;
  unsigned unsorted;
};

__device__ __forceinline__ unsigned long long order_pair(unsigned word, unsigned slot) {
  return (unsigned long long)word | ((unsigned long long)slot << 32);
}

// (key, id) of every slot against its predecessor's; the maxima by one integer atomic per wave
__global__ void __launch_bounds__(kBlock)
    k_order_check(const unsigned *key, const uint64_t *id, long long n, OrderFlags *flags) {
  unsigned long long max_id = 0ull;
  unsigned max_key = 0u;
  bool bad = false;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
    const unsigned k = key[p];
    const unsigned long long i = id[p];
    max_id = i > max_id ? i : max_id;
    max_key = k > max_key ? k : max_key;
    if (p > 0) {
      const unsigned kp = key[p - 1];
      const unsigned long long ip = id[p - 1];
      bad = bad || k < kp || (k == kp && i < ip);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long oi = __shfl_down(max_id, off, 64);
    const unsigned ok = __shfl_down(max_key, off, 64);
    max_id = oi > max_id ? oi : max_id;
    max_key = ok > max_key ? ok : max_key;
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&flags->max_id, max_id);
    atomicMax(&flags->max_key, max_key);
    if (any_bad) flags->unsorted = 1u;   // (every writer stores the same word)
  }
}

// the word `which` (OrderWord) of slot s
__device__ __forceinline__ unsigned order_word(int which, const unsigned *key, const uint64_t *id, unsigned s) {
  if (which == ORDER_KEY) return key[s];
  const unsigned long long i = id[s];
  return which == ORDER_ID_HI ? (unsigned)(i >> 32) : (unsigned)i;
}

__global__ void __launch_bounds__(kBlock)
    k_order_init(const unsigned *key, const uint64_t *id, long long n, int which, unsigned long long *pairs) {
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x)
    pairs[p] = order_pair(order_word(which, key, id, (unsigned)p), (unsigned)p);
}

// the lanes of the wave that hold digit d (among the active ones): 8 ballots, one per bit
__device__ __forceinline__ unsigned long long order_match(unsigned d, bool active) {
  unsigned long long m = __ballot(active);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = ((d >> b) & 1u) != 0u;
    const unsigned long long has = __ballot(bit);
    m &= bit ? has : ~has;
  }
  return m;
}

// One round of a wave: the rank of this lane's pair among the pairs with its digit that the wave has seen so far
// (earlier rounds, then lower lanes), and the running counts moved on.  wcnt: the wave's 256 running counts in LDS.
__device__ __forceinline__ unsigned order_rank_round(unsigned *wcnt, unsigned d, bool active, int lane) {
  const unsigned long long m = order_match(d, active);
  unsigned rank = 0u;
  if (active) rank = wcnt[d] + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
  // (LDS operations of one wave complete in order; the fences keep the compiler from moving the group's reads
  // below the leader's store, or the next round's reads above it)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (active && (m & ((1ull << lane) - 1ull)) == 0ull) wcnt[d] += (unsigned)__popcll(m);   // (one lane per digit)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return rank;
}

// cnt[d * ntiles + tile] = pairs of the tile whose digit is d
__global__ void __launch_bounds__(kBlock)
    k_order_count(const unsigned long long *pairs, long long n, int shift, unsigned *cnt, long long ntiles) {
  __shared__ unsigned wcnt[kBlock / 64][kOrderDigits];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kBlock / 64; ++q) wcnt[q][threadIdx.x] = 0u;
  __syncthreads();
  const long long wave0 = (long long)blockIdx.x * kOrderTile + (long long)wave * kOrderWaveSlots;
#pragma unroll
  for (int q = 0; q < kOrderItems; ++q) {
    const long long i = wave0 + 64 * q + lane;
    const bool active = i < n;
    const unsigned d = active ? ((unsigned)pairs[i] >> shift) & 255u : 0u;
    (void)order_rank_round(wcnt[wave], d, active, lane);
  }
  __syncthreads();
  unsigned total = 0u;
#pragma unroll
  for (int q = 0; q < kBlock / 64; ++q) total += wcnt[q][threadIdx.x];
  cnt[(long long)threadIdx.x * ntiles + blockIdx.x] = total;
}

// base: cnt behind its exclusive scan.  Every pair of the tile goes to base[digit][tile] + its rank in the tile --
// as a pair whose word is that of the next pass (NEXT_SAME / _ID_HI / _KEY), or as dest[slot] = position
// (NEXT_DEST, the last pass).
__global__ void __launch_bounds__(kBlock)
    k_order_scatter(const unsigned long long *pairs, long long n, int shift, const unsigned *base, long long ntiles,
                    int next, const unsigned *key, const uint64_t *id, unsigned long long *out, unsigned *dest) {
  __shared__ unsigned wcnt[kBlock / 64][kOrderDigits];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kBlock / 64; ++q) wcnt[q][threadIdx.x] = 0u;
  __syncthreads();
  const long long wave0 = (long long)blockIdx.x * kOrderTile + (long long)wave * kOrderWaveSlots;
  unsigned long long pr[kOrderItems];
  unsigned rank[kOrderItems];
#pragma unroll
  for (int q = 0; q < kOrderItems; ++q) {
    const long long i = wave0 + 64 * q + lane;
    const bool active = i < n;
    pr[q] = active ? pairs[i] : 0ull;
    rank[q] = order_rank_round(wcnt[wave], ((unsigned)pr[q] >> shift) & 255u, active, lane);
  }
  __syncthreads();
  {  // the waves' totals of digit threadIdx.x -> where each wave's pairs of that digit start
    unsigned run = base[(long long)threadIdx.x * ntiles + blockIdx.x];
#pragma unroll
    for (int q = 0; q < kBlock / 64; ++q) {
      const unsigned c = wcnt[q][threadIdx.x];
      wcnt[q][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kOrderItems; ++q) {
    if (wave0 + 64 * q + lane >= n) continue;
    const unsigned word = (unsigned)pr[q], slot = (unsigned)(pr[q] >> 32);
    const unsigned pos = wcnt[wave][(word >> shift) & 255u] + rank[q];
    if ((long long)pos >= n || (long long)slot >= n) continue;   // (cannot happen: the counts are those of these pairs)
    if (next == ORDER_NEXT_DEST) dest[slot] = pos;
    else if (next == ORDER_NEXT_SAME) out[pos] = pr[q];
    else out[pos] = order_pair(order_word(next == ORDER_NEXT_KEY ? ORDER_KEY : ORDER_ID_HI, key, id, slot), slot);
  }
}

// The move: slot s, read in order, becomes the record at dest[s] (k_sort_pack with the destination read, not claimed).
__global__ void __launch_bounds__(kBlock)
    k_order_pack(DevSwarm S, long long n, const unsigned *dest, unsigned long long *rec) {
  typedef unsigned long long u64;
  __shared__ __attribute__((aligned(16))) u64 stage[kBlock / 64][64][kSortRowWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) - lane;
  for (long long base = wave0; base < n; base += (long long)gridDim.x * blockDim.x) {
    const long long s = base + lane;
    const bool active = s < n;
    unsigned d = 0u;
    if (active) {
      d = dest[s];
      sort_stage(&stage[wave][lane][0], S, s, S.w[s]);
    }
    sort_store_rows(stage[wave], lane, base, n, d, rec);
  }
}

}  // namespace jb
