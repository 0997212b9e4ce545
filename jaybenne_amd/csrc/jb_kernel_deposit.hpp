// jb_kernel_deposit.hpp -- exact deposition (include/jaybenne_amd.h: jb_set_deposition): energy_delta and the
// census tally as ONE rounding of the exact sum of their addends, whatever the order the addends arrive in.
// The reference has no such task; the sums are over what its tasks leave in the swarm.
//
// Kernel              what it does
// k_deposit_scale     largest scale exponent of w over a range of slots: one integer atomicMax per wave
// k_deposit_rescale   the accumulators moved to a raised scale (a later sweep of the cycle met a heavier weight)
// k_deposit_sweep     one streaming pass over slots [first, last): the counted slots' w, converted at the scale
//                     (jb_deposit_fixed.hpp), added to the 256-bit accumulator of their cell
// k_deposit_final     one thread per cell: the accumulator, rounded once, into energy_delta (+=) or energy_tally
//                     (= T / dv); the accumulator back to zero
//
// No floating-point atomics.  The adds are 64-bit integer adds with carry: a word add that wraps adds 1 to the
// next word, and since every add is a RETURNING atomic, every wrap is seen by exactly one of them -- the total is
// right under any interleaving.  Integer addition is associative, so a wave may merge what shares a cell before it
// touches memory: a swarm in (block, cell) order gives runs of equal cells in neighbouring lanes, the wave sums each
// run with a segmented shuffle reduction of the 256-bit values and only the run's first lane issues atomics.  An
// unsorted swarm degenerates to one chain of atomics per photon and is as right.  A mesh of at most kDepositLds
// cells accumulates in LDS (32 bytes per cell) and every workgroup flushes its non-zero entries once: the 1-D
// deck puts 7.8e5 photons into one cell, and without this every deposit would land on 128 accumulators
// (DESIGN.md 4.2 item 4).
#pragma once

#include <hip/hip_runtime.h>

#include "jb_deposit_fixed.hpp"
#include "jb_kernels.hpp"
#include "jb_kernel_ledger.hpp"

namespace jb {

// what a sweep counts
enum {
  DEP_ABSORBED = 1,   // ST_ABSORBED, bit 63 of the id clear: absorbed here, in an owned block
  DEP_ARRIVALS = 2,   // ST_ABSORBED with bit 63: absorbed in a halo copy on the sender, deposited by the owner
  DEP_BOTH = 3,       // every ST_ABSORBED slot (the id is not read)
  DEP_CENSUS = 4      // ST_ACTIVE in an owned block
};
// the control words of a mesh's accumulators, in device memory
enum {
  DC_SCALE = 0,        // the cycle's scale exponent E (atomicMax)
  DC_N_ABSORBED = 1,   // addends of the absorbed / arrivals sweeps since the last close
  DC_N_CENSUS = 2,     // ... of the census sweep
  DC_N_TRUNCATED = 3,
  DC_N_REJECTED = 4,
  DC_TOP_BIT = 5,      // adds that left (or brought) a set top bit
  DC_SCALE_NEW = 6,    // largest exponent in the range of a later sweep of the cycle (k_deposit_rescale)
  DC_N = 8
};

__device__ __forceinline__ Dep256 dep_shfl_down(const Dep256 &v, int off) {
  Dep256 r;
#pragma unroll
  for (int q = 0; q < kDepWords; ++q) r.w[q] = (uint64_t)__shfl_down((unsigned long long)v.w[q], off, 64);
  return r;
}

// v added to the four words at acc (global or LDS memory) with returning atomics; a zero word is not sent.
// Returns true when the add brought, or left, a set top bit.
__device__ __forceinline__ bool dep_atomic_add(unsigned long long *acc, const Dep256 &v) {
  unsigned long long carry = 0ull;
  bool top = false;
#pragma unroll
  for (int q = 0; q < kDepWords; ++q) {
    // (v.w[q] + carry wraps only when v.w[q] is all ones and a carry comes in: the word stays, the carry goes on)
    const unsigned long long a = (unsigned long long)v.w[q] + carry;
    unsigned long long next = (carry != 0ull && a == 0ull) ? 1ull : 0ull;
    if (a != 0ull) {
      const unsigned long long old = atomicAdd(acc + q, a);
      const unsigned long long sum = old + a;
      if (sum < a) next = 1ull;
      if (q == kDepWords - 1) top = ((a | sum) >> 63) != 0ull;
    }
    carry = next;
  }
  return top;
}

// ACTIVE: over the ACTIVE slots alone (the census scale of the close); else over every slot of the range.
// A lane takes the largest exponent of its slots, the wave the largest of its lanes: one atomicMax per wave.
template <bool ACTIVE>
__global__ void __launch_bounds__(kBlock)
    k_deposit_scale(DevSwarm S, long long first, long long last, unsigned long long *ctl, int word) {
  int e = 0;
  constexpr long long kTile = (long long)kLedgerUnroll * kBlock;
  for (long long n0 = first + (long long)blockIdx.x * kTile + threadIdx.x; n0 < last;
       n0 += (long long)gridDim.x * kTile) {
#pragma unroll
    for (int u = 0; u < kLedgerUnroll; ++u) {
      const long long n = n0 + (long long)u * kBlock;
      if (n >= last) continue;
      if constexpr (ACTIVE) {
        if (S.status[n] != ST_ACTIVE) continue;
      }
      const int x = dep_exponent(S.w[n]);
      e = x > e ? x : e;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_down(e, off, 64);
    e = o > e ? o : e;
  }
  if ((threadIdx.x & 63) == 0 && e > 0) atomicMax(ctl + word, (unsigned long long)e);
}

// A later sweep of the cycle whose range holds a heavier weight than the scale was taken over -- arrivals from a rank
// with hotter blocks: the cold half of the step deck sources 67 binary orders below the hot half, twice the
// headroom -- RAISES the scale: every accumulator moves down by the difference, in front of the sweep.  Bits that
// fall off the low end are counted in n_truncated (per accumulator); while there are none the sums stay exact.
__global__ void __launch_bounds__(kBlock)
    k_deposit_rescale(long long ncells, unsigned long long *acc, unsigned long long *ctl) {
  const int E = ctl[DC_SCALE] != 0ull ? (int)ctl[DC_SCALE] : 1, En = (int)ctl[DC_SCALE_NEW];
  if (En <= E) return;   // (uniform over the grid)
  unsigned long long n_trunc = 0ull;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < ncells;
       c += (long long)gridDim.x * blockDim.x) {
    Dep256 v;
#pragma unroll
    for (int q = 0; q < kDepWords; ++q) v.w[q] = acc[(size_t)c * kDepWords + q];
    if (dep_is_zero(v)) continue;
    if (dep_shift_right(v, En - E)) ++n_trunc;
#pragma unroll
    for (int q = 0; q < kDepWords; ++q) acc[(size_t)c * kDepWords + q] = v.w[q];
  }
  n_trunc = wave_sum(n_trunc);
  if ((threadIdx.x & 63) == 0 && n_trunc) atomicAdd(ctl + DC_N_TRUNCATED, n_trunc);
}
// ... and behind it, one thread: the raised scale is the scale from now on
__global__ void k_deposit_commit(unsigned long long *ctl) {
  if (ctl[DC_SCALE_NEW] > ctl[DC_SCALE]) ctl[DC_SCALE] = ctl[DC_SCALE_NEW];
  ctl[DC_SCALE_NEW] = 0ull;
}

// WHAT: DEP_ABSORBED / _ARRIVALS / _BOTH / _CENSUS.  LDS: the mesh has at most kDepositLds cells (host).
// The streaming shape of k_ledger_sweep: tiles of kLedgerUnroll x kBlock consecutive slots, the status first;
// w, the indices and the id only for counted slots.  acc: [nblocks * ncell][4] words, cell = blk * ncell +
// interior index.  A slot whose block or indices lie outside the interior of a resident block adds nothing and
// is counted as rejected.
template <int WHAT, bool LDS>
__global__ void __launch_bounds__(kBlock)
    k_deposit_sweep(DevMesh M, DevSwarm S, long long first, long long last, unsigned long long *acc,
                    unsigned long long *ctl) {
  __shared__ unsigned long long lds_acc[LDS ? kDepositLds * kDepWords : 1];
  const int ncells = M.nblocks * M.ncell;
  if constexpr (LDS) {
    for (int q = threadIdx.x; q < ncells * kDepWords; q += kBlock) lds_acc[q] = 0ull;
    __syncthreads();
  }
  const int E = ctl[DC_SCALE] != 0ull ? (int)ctl[DC_SCALE] : 1;   // (no weight > 0 in the range the scale was taken over)
  const int lane = threadIdx.x & 63;
  unsigned long long n_add = 0ull, n_trunc = 0ull, n_rej = 0ull, n_top = 0ull;
  constexpr long long kTile = (long long)kLedgerUnroll * kBlock;
  // (the trip count is uniform over the workgroup: every lane of a wave takes part in the shuffles)
  for (long long t0 = first + (long long)blockIdx.x * kTile; t0 < last; t0 += (long long)gridDim.x * kTile) {
    const long long n0 = t0 + threadIdx.x;
    int st[kLedgerUnroll];
#pragma unroll
    for (int u = 0; u < kLedgerUnroll; ++u) {
      const long long n = n0 + (long long)u * kBlock;
      st[u] = n < last ? S.status[n] : -1;
    }
#pragma unroll
    for (int u = 0; u < kLedgerUnroll; ++u) {
      const long long n = n0 + (long long)u * kBlock;
      bool counted = st[u] == (WHAT == DEP_CENSUS ? ST_ACTIVE : ST_ABSORBED);
      if constexpr (WHAT == DEP_ABSORBED || WHAT == DEP_ARRIVALS) {
        if (counted) counted = ((S.id[n] & kLedgerDepositedBit) != 0ull) == (WHAT == DEP_ARRIVALS);
      }
      if (__ballot(counted) == 0ull) continue;   // (uniform over the wave)
      int cell = -1;
      Dep256 v;
      v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
      if (counted) {
        const int b = S.blk[n], i = S.ip[n] - M.is, j = S.jp[n] - M.js, k = S.kp[n] - M.ks;
        const bool inside = b >= 0 && b < M.nblocks && i >= 0 && i < M.nx[0] && j >= 0 && j < M.nx[1] && k >= 0 &&
                            k < M.nx[2];
        if (WHAT == DEP_CENSUS && inside && !M.owned[b]) {
          // (a census photon in a halo copy belongs to its owner's tally)
        } else if (!inside) {
          ++n_rej;
        } else {
          const int r = dep_from_double(S.w[n], E, v);
          if (r == DEP_REJECTED) {
            ++n_rej;
          } else {
            cell = b * M.ncell + (k * M.nx[1] + j) * M.nx[0] + i;
            ++n_add;
            if (r == DEP_TRUNCATED) ++n_trunc;
          }
        }
      }
      // runs of equal cells in neighbouring lanes: the lane behind the run's last one, then the run's sum
      const int prev = __shfl_up(cell, 1, 64);
      const bool head = lane == 0 || prev != cell;
      const unsigned long long heads = __ballot(head);
      const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1);
      const int end = above != 0ull ? __ffsll((long long)above) - 1 : 64;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const Dep256 o = dep_shfl_down(v, off);
        if (lane + off < end) dep_add(v, o);
      }
      if (head && cell >= 0) {
        // (two calls, not one pointer chosen at run time: each keeps its address space, ds_ or global_ atomics)
        bool top;
        if constexpr (LDS) top = dep_atomic_add(&lds_acc[cell * kDepWords], v);
        else top = dep_atomic_add(acc + (size_t)cell * kDepWords, v);
        if (top) ++n_top;
      }
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int c = threadIdx.x; c < ncells; c += kBlock) {
      Dep256 v;
#pragma unroll
      for (int q = 0; q < kDepWords; ++q) v.w[q] = lds_acc[c * kDepWords + q];
      if (!dep_is_zero(v) && dep_atomic_add(acc + (size_t)c * kDepWords, v)) ++n_top;
    }
  }
  n_add = wave_sum(n_add); n_trunc = wave_sum(n_trunc); n_rej = wave_sum(n_rej); n_top = wave_sum(n_top);
  if (lane == 0) {
    if (n_add) atomicAdd(ctl + (WHAT == DEP_CENSUS ? DC_N_CENSUS : DC_N_ABSORBED), n_add);
    if (n_trunc) atomicAdd(ctl + DC_N_TRUNCATED, n_trunc);
    if (n_rej) atomicAdd(ctl + DC_N_REJECTED, n_rej);
    if (n_top) atomicAdd(ctl + DC_TOP_BIT, n_top);
  }
}

// FIELD 0: energy_delta[q] = energy_delta[q] + D where the cell received something.  FIELD 1: energy_tally[q] =
// T / dv, dv the product the fused tally divides by; cells without census photons get 0.  D, T: the accumulator
// at scale E rounded once (dep_to_double).  One thread per interior cell of the resident blocks, plain stores;
// the accumulator is zero afterwards.
template <int FIELD>
__global__ void __launch_bounds__(kBlock) k_deposit_final(DevMesh M, unsigned long long *acc, int E) {
  const long long total = (long long)M.nblocks * M.ncell;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < total;
       c += (long long)gridDim.x * blockDim.x) {
    int b, k, j, i, cell;
    decode_cell(M, c, b, k, j, i, cell);
    const int ci = cidx(M, k, j, i);
    Dep256 v;
#pragma unroll
    for (int q = 0; q < kDepWords; ++q) v.w[q] = acc[(size_t)c * kDepWords + q];
    const bool any = !dep_is_zero(v);
    if (any) {
#pragma unroll
      for (int q = 0; q < kDepWords; ++q) acc[(size_t)c * kDepWords + q] = 0ull;
    }
    if constexpr (FIELD == 0) {
      if (any) M.edelta[b][ci] = M.edelta[b][ci] + dep_to_double(v, E);
    } else {
      const double dv = M.blk_dx[3 * b] * M.blk_dx[3 * b + 1] * M.blk_dx[3 * b + 2];
      M.tally[b][ci] = any ? dep_to_double(v, E) / dv : 0.0;
    }
  }
}

}  // namespace jb
