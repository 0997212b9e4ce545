// jb_kernel_gcomb.hpp -- census population control for the whole mesh: a global comb that holds the swarm near N
// photons of equal weight (include/jaybenne_amd.h: jb_comb_census_weigh / jb_comb_census_plan_global /
// jb_comb_census_apply).  The reference has no such task.  The per-cell comb (jb_kernel_comb.hpp) caps a cell; this
// one deals a target population N to the cells in proportion to the census energy they hold, thins the cells above
// their share and SPLITS the ones below it.  Each cell's energy is conserved.
//
// The rule.  Every operation is individually rounded (-ffp-contract=off); no product is fused with a sum.
//   1. The swarm is in (block, cell) order (the canonical order under JB_CELL_ORDER_BY_ID) and C_j are the running
//      weights of the segmented scan of jb_kernel_comb.hpp -- exact 128-bit sums rounded once under BY_ID.
//   2. Cell key k (ghost cells of the block's array included): m_k = its ACTIVE photons, W_k = C[end - 1].  The cell
//      is VALID iff m_k >= 1 and 0 < W_k < inf; an invalid cell is never touched and adds +0.0 below.
//      e_block[b] = the sum of W_k over the ntot cells of block b in cell-index order with the tree of
//      k_salloc_energy: thread t adds cells t, t + 256, ... from +0.0, then s[t] += s[t + d], d = 128 ... 1.
//      0 for a halo copy.
//   3. (host) W_tot = jb_source_energy_total of the block sums by global block id; scale = (double)N / W_tot.
//   4. nu = W_k scale, f = floor(nu), K_k = f + ((nu - f) > xi'_k) with xi'_k the first uniform of the stream
//      seed_state(seed, kRngDomainCombCount = 9, cell_stream_id(epoch, global block id, cell)); K_k = max(K_k, 1)
//      (no roulette: every occupied cell keeps its energy); K_k = min(K_k, S m_k, 2^32 - 1), compared in double.
//   5. The cell is COMBED iff (double)m_k > r K_k or K_k > r (double)m_k.  Every other cell stays bit for bit.
//   6. A combed cell comes out as exactly K_k copies of weight W_k / K_k by the rule of jb_kernel_comb.hpp:
//      D = W_k / K_k, xi = comb_xi (domain 2), u_0 = 0, u_j = clamp(ceil(C_j / D - xi), 0, K_k), u_m = K_k,
//      k_j = u_j - u_(j-1), C_(j-1) the neighbouring slot's stored value.  The first copy keeps id and stream
//      state; copy q >= 1 takes id_base + idoff + q - 1 (offsets in output-slot order) and that id's stream start.
//
// Kernel              what it does                                                         bytes
// k_gcomb_block_sums  one workgroup per block: e_block[b] (step 2)                         8 per cell + 8 per occupied cell
// k_gcomb_targets     per cell: K_k or 0 ("leave alone") at the cell's FIRST SLOT          8 per cell, 12 per occupied cell
//                     (an array of n + 1 words, indexed as cexp[comb_start(ends, k)] is), and per-workgroup partials
//                     of the report: cells thinned, cells split, largest m_k, largest K_k, and the combed cells' photons
//                     in and copies out (64-bit sums: n_after before the 32-bit scans are trusted)
// k_gcomb_decide      per slot: k_j and max(k_j - 1, 0) with the slot's own cell target    ~24 read, 8 written per slot
//   (k_scan_tiles / _sums / _add of the sort turn both into output slots and id offsets)
// k_gcomb_pack        the move, driven by the OUTPUT record: eight lanes own output record d, find its source slot --
//                     the last s with dest[s] <= d, by binary search in the scanned dest (rising, n + 1 entries) --,
//                     build the record and store its 128 bytes with one instruction per lane.  No loop's trip count
//                     is a photon's copy count: a photon split into 5000 copies is 5000 records of 5000 groups.
//   (k_sort_unpack writes the records back into the swarm arrays)
//
// Determinism: no floating-point atomics, no atomics at all, no workgroup waits for another; every sum is a fixed tree.
#pragma once

#include <hip/hip_runtime.h>

#include "jb_kernel_comb.hpp"

namespace jb {

// (kGcombStats per workgroup: jb_scratch_layout.hpp)
enum { GS_THINNED = 0, GS_SPLIT, GS_MOST, GS_TARGET, GS_IN, GS_OUT };
static_assert(GS_OUT + 1 == kGcombStats, "jb_scratch_layout.hpp sizes the partials");

// xi' of the cell: keyed as comb_xi is, in a domain of its own -- the count draw and the selection draw are independent
__device__ __forceinline__ double gcomb_xi(uint32_t seed, uint32_t epoch, int gblock, unsigned cell) {
  return u52_to_double(rng_seed_state(seed, kRngDomainCombCount, cell_stream_id(epoch, gblock, (int)cell)) >> 12);
}
// m_k and W_k of cell k; false for an invalid cell
__device__ __forceinline__ bool gcomb_cell(const unsigned *ends, const double *C, unsigned k, unsigned &start,
                                           unsigned &m, double &W) {
  start = comb_start(ends, k);
  const unsigned end = ends[k];
  m = end - start;
  W = 0.0;
  if (m == 0u) return false;   // (no slot of C belongs to the cell: nothing is read)
  W = C[end - 1u];
  return W > 0.0 && W < __builtin_huge_val();
}

__global__ void __launch_bounds__(kBlock)
    k_gcomb_block_sums(DevMesh M, const unsigned *ends, const double *C, double *e_block) {
  __shared__ double s[kBlock];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  if (!M.owned[b]) {   // (uniform over the workgroup)
    if (t == 0) e_block[b] = 0.0;
    return;
  }
  double acc = 0.0;
  for (int cell = t; cell < M.ntot; cell += kBlock) {
    unsigned start, m;
    double W;
    const bool valid = gcomb_cell(ends, C, (unsigned)b * (unsigned)M.ntot + (unsigned)cell, start, m, W);
    acc += valid ? W : 0.0;
  }
  s[t] = acc;
  __syncthreads();
#pragma unroll
  for (int d = kBlock / 2; d >= 1; d >>= 1) {
    if (t < d) s[t] += s[t + d];
    __syncthreads();
  }
  if (t == 0) e_block[b] = s[0];
}

// ktgt[first slot of cell k] = K_k of a combed cell, 0 of any other occupied cell; partials[kGcombStats g ..]: the report
__global__ void __launch_bounds__(kBlock)
    k_gcomb_targets(DevMesh M, unsigned nkeys, const unsigned *ends, const double *C, double scale, double band,
                    double split_max, uint32_t seed, uint32_t epoch, unsigned *ktgt, unsigned long long *partials) {
  __shared__ unsigned long long lds[kBlock / 64][kGcombStats];
  unsigned long long thinned = 0ull, split = 0ull, most = 0ull, target = 0ull, in = 0ull, out = 0ull;
  for (unsigned long long kk = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; kk < nkeys;
       kk += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned k = (unsigned)kk;
    unsigned start, m;
    double W;
    const bool valid = gcomb_cell(ends, C, k, start, m, W);
    if (m == 0u) continue;
    if (m > most) most = m;
    unsigned K = 0u;
    if (valid) {
      const unsigned b = k / (unsigned)M.ntot;
      const double xi = gcomb_xi(seed, epoch, M.gid[b], k - b * (unsigned)M.ntot);
      const double nu = W * scale;
      const double f = floor(nu);
      double Kd = f + (double)((nu - f) > xi);
      Kd = Kd > 1.0 ? Kd : 1.0;
      const double cap = split_max * (double)m;
      Kd = Kd < cap ? Kd : cap;
      Kd = Kd < 4294967295.0 ? Kd : 4294967295.0;
      const double md = (double)m;
      const unsigned Ku = (unsigned)Kd;
      if (Ku > target) target = Ku;
      if (md > band * Kd || Kd > band * md) {
        K = Ku;
        in += m;     // (64-bit: the host forms n_after from these before it trusts the 32-bit scans)
        out += Ku;
        if (Ku < m) ++thinned;
        else ++split;
      }
    }
    ktgt[start] = K;
  }
  thinned = wave_sum(thinned);
  split = wave_sum(split);
  in = wave_sum(in);
  out = wave_sum(out);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(most, off, 64), p = __shfl_down(target, off, 64);
    most = o > most ? o : most;
    target = p > target ? p : target;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    lds[wave][GS_THINNED] = thinned;
    lds[wave][GS_SPLIT] = split;
    lds[wave][GS_MOST] = most;
    lds[wave][GS_TARGET] = target;
    lds[wave][GS_IN] = in;
    lds[wave][GS_OUT] = out;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < kBlock / 64; ++q) {
      thinned += lds[q][GS_THINNED];
      split += lds[q][GS_SPLIT];
      in += lds[q][GS_IN];
      out += lds[q][GS_OUT];
      most = lds[q][GS_MOST] > most ? lds[q][GS_MOST] : most;
      target = lds[q][GS_TARGET] > target ? lds[q][GS_TARGET] : target;
    }
    unsigned long long *p = partials + (size_t)kGcombStats * blockIdx.x;
    p[GS_THINNED] = thinned;
    p[GS_SPLIT] = split;
    p[GS_MOST] = most;
    p[GS_TARGET] = target;
    p[GS_IN] = in;
    p[GS_OUT] = out;
  }
}

// kcnt[s] = copies slot s comes out as, extra[s] = new ids it needs; entry n of both is 0 (the scans' totals land
// there).  Slots of cells that are left alone, and the slots behind all cells: one copy, themselves.
__global__ void __launch_bounds__(kBlock)
    k_gcomb_decide(DevMesh M, long long n, unsigned nkeys, const unsigned *key, const unsigned *ends, const double *C,
                   const unsigned *ktgt, uint32_t seed, uint32_t epoch, unsigned *kcnt, unsigned *extra) {
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s <= n; s += (long long)gridDim.x * blockDim.x) {
    unsigned cnt = s < n ? 1u : 0u;
    const unsigned k = s < n ? key[s] : nkeys;
    if (k < nkeys) {
      const unsigned start = comb_start(ends, k);
      const unsigned K = ktgt[start];
      if (K > 0u) {
        const unsigned end = ends[k];
        const double delta = C[end - 1u] / (double)K;
        const unsigned b = k / (unsigned)M.ntot;
        const double xi = comb_xi(seed, epoch, M.gid[b], k - b * (unsigned)M.ntot);
        const unsigned uj = s == (long long)end - 1 ? K : comb_u(C[s], delta, xi, K);
        const unsigned up = s == (long long)start ? 0u : comb_u(C[s - 1], delta, xi, K);
        cnt = uj > up ? uj - up : 0u;
      }
    }
    kcnt[s] = cnt;
    extra[s] = cnt > 1u ? cnt - 1u : 0u;
  }
}

// The move.  A wave takes 64 consecutive OUTPUT records; lane l owns record d = base + l through the search and the
// staging (its LDS row), then eight lanes store one record whole, as k_sort_pack does.  dest[0 .. n]: rising,
// dest[n] = n_after > d, so the search ends at a slot s < n with dest[s] <= d < dest[s + 1].
__global__ void __launch_bounds__(kBlock)
    k_gcomb_pack(DevSwarm S, long long n, long long n_after, unsigned nkeys, const unsigned *key, const unsigned *ends,
                 const double *C, const unsigned *ktgt, const unsigned *dest, const unsigned *idoff, uint32_t seed,
                 unsigned long long id_base, unsigned long long *rec) {
  typedef unsigned long long u64;
  __shared__ __attribute__((aligned(16))) u64 stage[kBlock / 64][64][kSortRowWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) - lane;
  for (long long base = wave0; base < n_after; base += (long long)gridDim.x * blockDim.x) {
    const long long d = base + lane;
    if (d < n_after) {
      const unsigned du = (unsigned)d;
      long long lo = 0, hi = n;   // dest[lo] <= d < dest[hi]
      while (hi - lo > 1) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (dest[mid] <= du) lo = mid;
        else hi = mid;
      }
      const long long s = lo;
      const unsigned q = du - dest[s];
      double w = S.w[s];
      const unsigned k = key[s];
      if (k < nkeys) {
        const unsigned K = ktgt[comb_start(ends, k)];
        if (K > 0u) w = C[ends[k] - 1u] / (double)K;
      }
      u64 *row = &stage[wave][lane][0];
      sort_stage(row, S, s, w);
      if (q > 0u) {
        const u64 id = id_base + (u64)idoff[s] + (u64)(q - 1u);
        row[9] = id;
        row[10] = rng_stream_start(seed, id);
      }
    }
    sort_store_rows(stage[wave], lane, base, n_after, (unsigned)d, rec);
  }
}

}  // namespace jb
