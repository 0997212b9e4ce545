// jb_kernel_ledger.hpp -- the energy ledger of a radiation cycle (include/jaybenne_amd.h: jb_energy_ledger):
// where the cycle's energy went, summed on the device.  The reference has no such task; the sums are over
// what its tasks leave in the swarm and the fields.
//
// Kernel            what it sums
// k_ledger_sweep    one pass over the slots [first, last) of the swarm: weight and count per class of status
// k_ledger_fields   tally V, energy_delta and u V over the interior cells of the owned blocks
// k_ledger_final    the workgroups' partial sums of either, in a fixed order, into the running ledger
//
// No floating-point atomics: a lane sums its slots in slot order, a wave sums its
// lanes by shuffles, a workgroup its waves through LDS, and each workgroup writes its sums with plain stores to
// 256 bytes of its own; k_ledger_final, one workgroup, adds those in a fixed order.  The result depends on the
// slot contents, the range and the grid alone -- not on scheduling: the same call on the same swarm gives the
// same bits.  The sweep streams: 4 bytes of status per slot, 8 of weight where the status is counted, the
// position only for the few escaped slots.
#pragma once

#include <hip/hip_runtime.h>

#include "jb_kernels.hpp"

namespace jb {

// classes of a sweep: 0 ACTIVE | 1 ABSORBED or OUTGOING_ABSORBED | 2..7 ESCAPED through face 0..5 |
// 8 ESCAPED, no outflow face found
constexpr int kLedgerClasses = 9;
constexpr int kLedgerFieldSums = 3;       // tally V | energy_delta | u V
constexpr int kLedgerStride = 32;         // words per workgroup in the partials buffer: 256 bytes, two lines of its own
constexpr int kLedgerUnroll = 4;          // status loads a lane has in flight
enum { LEDGER_SOURCED = 0, LEDGER_TRANSPORTED = 1, LEDGER_CENSUS = 2 };
// the running ledger on the device, in 8-byte words: the first 23 words of jb_energy_ledger
enum {
  LW_E_SOURCED = 0, LW_N_SOURCED = 1, LW_E_ESCAPED = 2, LW_N_ESCAPED = 8, LW_E_UNCLASSIFIED = 14,
  LW_N_UNCLASSIFIED = 15, LW_E_ABSORBED = 16, LW_N_ABSORBED = 17, LW_E_CENSUS = 18, LW_N_CENSUS = 19,
  LW_E_TALLY = 20, LW_E_DELTA = 21, LW_E_MATERIAL = 22, LW_N = 23
};
// k_unpack_incoming leaves this bit in the id of the hole an absorbed arrival becomes: its weight was counted
// by the rank whose kernel absorbed it
constexpr unsigned long long kLedgerDepositedBit = 1ull << 63;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// The face an escaped photon left through: the first active axis on which the written-back position lies
// strictly outside the domain -- the test on which apply_swarm_bcs returns false -- if that face is outflow;
// 6 otherwise (unclassified).
__device__ __forceinline__ int ledger_face(const DevMesh &M, double x, double y, double z) {
  const double p[3] = {x, y, z};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d >= M.ndim) break;
    if (p[d] < M.gmin[d]) return M.bc[2 * d] == BC_OUTFLOW ? 2 * d : 6;
    if (p[d] > M.gmax[d]) return M.bc[2 * d + 1] == BC_OUTFLOW ? 2 * d + 1 : 6;
  }
  return 6;
}

// sums of one workgroup -> partials[blockIdx.x * kLedgerStride + ..]: the first NV of the doubles at words 0..,
// the first NC of the counts at words kLedgerClasses..
template <int NV, int NC, int NE, int NCC>
__device__ __forceinline__ void ledger_block_store(double (&e)[NE], unsigned long long (&c)[NCC],
                                                   unsigned long long *partials) {
  static_assert(NV <= NE && NC <= NCC && NV <= kLedgerClasses && kLedgerClasses + NC <= kLedgerStride, "");
  constexpr int kWaves = kBlock / 64;
  __shared__ double lds_e[kWaves][NV];
  __shared__ unsigned long long lds_c[kWaves][NC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const double s = wave_sum_f64(e[q]);
    if (lane == 0) lds_e[wave][q] = s;
  }
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const unsigned long long s = wave_sum(c[q]);
    if (lane == 0) lds_c[wave][q] = s;
  }
  __syncthreads();
  unsigned long long *out = partials + (size_t)blockIdx.x * kLedgerStride;
  if (threadIdx.x < NV) {
    double s = lds_e[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += lds_e[w][threadIdx.x];
    out[threadIdx.x] = (unsigned long long)__double_as_longlong(s);
  } else if (threadIdx.x < NV + NC) {
    const int q = threadIdx.x - NV;
    unsigned long long s = lds_c[0][q];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += lds_c[w][q];
    out[kLedgerClasses + q] = s;
  }
}

// WHAT = LEDGER_SOURCED / LEDGER_CENSUS: the ACTIVE slots; LEDGER_TRANSPORTED: the absorbed and the escaped.
// A lane reads the status first, the weight only where WHAT counts that status, the position only where it
// escaped.  The grid comes from the CU count (grid_for); a workgroup walks the range in tiles of
// kLedgerUnroll x kBlock consecutive slots, every load of a wave 256 or 512 contiguous bytes.
template <int WHAT>
__global__ void __launch_bounds__(kBlock)
    k_ledger_sweep(DevMesh M, DevSwarm S, long long first, long long last, unsigned long long *partials) {
  double e[kLedgerClasses];
  unsigned long long c[kLedgerClasses];
#pragma unroll
  for (int q = 0; q < kLedgerClasses; ++q) { e[q] = 0.0; c[q] = 0ull; }
  constexpr long long kTile = (long long)kLedgerUnroll * kBlock;
  for (long long n0 = first + (long long)blockIdx.x * kTile + threadIdx.x; n0 < last;
       n0 += (long long)gridDim.x * kTile) {
    int st[kLedgerUnroll];
#pragma unroll
    for (int u = 0; u < kLedgerUnroll; ++u) {
      const long long n = n0 + (long long)u * kBlock;
      st[u] = n < last ? S.status[n] : -1;
    }
#pragma unroll
    for (int u = 0; u < kLedgerUnroll; ++u) {
      const long long n = n0 + (long long)u * kBlock;
      if constexpr (WHAT != LEDGER_TRANSPORTED) {
        if (st[u] == ST_ACTIVE) { e[0] += S.w[n]; ++c[0]; }
      } else {
        if (st[u] == ST_OUTGOING_ABSORBED) {
          e[1] += S.w[n]; ++c[1];
        } else if (st[u] == ST_ABSORBED) {
          // (not the hole an arrival absorbed on another rank became: that rank has counted it)
          if (!(S.id[n] & kLedgerDepositedBit)) { e[1] += S.w[n]; ++c[1]; }
        } else if (st[u] == ST_ESCAPED) {
          const double w = S.w[n];
          const int f = ledger_face(M, S.x[n], M.ndim >= 2 ? S.y[n] : 0.0, M.ndim >= 3 ? S.z[n] : 0.0);
#pragma unroll
          for (int q = 0; q < 7; ++q)   // (a compile-time index: the sums stay in registers)
            if (q == f) { e[2 + q] += w; ++c[2 + q]; }
        }
      }
    }
  }
  // (the sourced and the census sweep fill class 0 alone)
  if constexpr (WHAT == LEDGER_TRANSPORTED) ledger_block_store<kLedgerClasses, kLedgerClasses>(e, c, partials);
  else ledger_block_store<1, 1>(e, c, partials);
}

// tally V, energy_delta (an energy per cell already: transport.cpp:159-161) and u V over the interior cells of
// the blocks this rank owns; the cell volume from the block's own widths (they differ by level)
__global__ void __launch_bounds__(kBlock) k_ledger_fields(DevMesh M, unsigned long long *partials) {
  double e[kLedgerFieldSums] = {0.0, 0.0, 0.0};
  unsigned long long none[1] = {0ull};
  const long long total = (long long)M.nblocks * M.ncell;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    int b, k, j, i, cell;
    decode_cell(M, q, b, k, j, i, cell);
    if (!M.owned[b]) continue;
    const double dv = M.blk_dx[3 * b] * M.blk_dx[3 * b + 1] * M.blk_dx[3 * b + 2];
    const int ci = cidx(M, k, j, i);
    e[0] += ((gcptr)M.tally[b])[ci] * dv;
    e[1] += ((gcptr)M.edelta[b])[ci];
    e[2] += ((gcptr)M.u[b])[ci] * dv;
  }
  ledger_block_store<kLedgerFieldSums, 1>(e, none, partials);
}

// One workgroup: the nparts partial sums of the launch before it, added in a fixed order -- thread t takes
// workgroups t, t + kBlock, ..., then a tree over the threads in LDS -- into the running ledger.
// what: LEDGER_SOURCED / _TRANSPORTED / _CENSUS after a sweep, -1 after k_ledger_fields.
__global__ void __launch_bounds__(kBlock)
    k_ledger_final(const unsigned long long *partials, int nparts, int what, unsigned long long *ledger) {
  __shared__ double lds_e[kBlock];
  __shared__ unsigned long long lds_c[kBlock];
  const int nv = what < 0 ? kLedgerFieldSums : (what == LEDGER_TRANSPORTED ? kLedgerClasses : 1);
  const int nc = what < 0 ? 0 : nv;
  for (int q = 0; q < nv; ++q) {
    double s = 0.0;
    unsigned long long cs = 0ull;
    for (int p = threadIdx.x; p < nparts; p += kBlock) {
      s += __longlong_as_double((long long)partials[(size_t)p * kLedgerStride + q]);
      if (q < nc) cs += partials[(size_t)p * kLedgerStride + kLedgerClasses + q];
    }
    lds_e[threadIdx.x] = s;
    lds_c[threadIdx.x] = cs;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
      if ((int)threadIdx.x < h) {
        lds_e[threadIdx.x] += lds_e[threadIdx.x + h];
        lds_c[threadIdx.x] += lds_c[threadIdx.x + h];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      int we = -1, wc = -1;   // the ledger words this sum goes to
      if (what < 0) {
        we = LW_E_TALLY + q;
      } else if (what == LEDGER_TRANSPORTED) {
        if (q == 1) { we = LW_E_ABSORBED; wc = LW_N_ABSORBED; }
        else if (q >= 2 && q < 8) { we = LW_E_ESCAPED + (q - 2); wc = LW_N_ESCAPED + (q - 2); }
        else if (q == 8) { we = LW_E_UNCLASSIFIED; wc = LW_N_UNCLASSIFIED; }
      } else if (q == 0) {
        we = what == LEDGER_SOURCED ? LW_E_SOURCED : LW_E_CENSUS;
        wc = what == LEDGER_SOURCED ? LW_N_SOURCED : LW_N_CENSUS;
      }
      if (we >= 0)
        ledger[we] = (unsigned long long)__double_as_longlong(
            __longlong_as_double((long long)ledger[we]) + lds_e[0]);
      if (wc >= 0) ledger[wc] += lds_c[0];
    }
    __syncthreads();
  }
}

}  // namespace jb
