// jb_kernel_moments.hpp -- radiation moments of the census: per cell the photon count, the energy density, the sum
// of squared weights, the flux and the second-moment tensor (include/jaybenne_amd.h:
// jb_evaluate_radiation_moments).  The reference has no such task: its tests copy the swarm to the host.
//
// The swarm is in (block, cell) order -- jb_defrag_particles, or it was already --, so the photons of a cell are a
// RUN of L consecutive slots a_0 .. a_(L-1); start[k] is the first slot of key k (the sort's histogram behind its
// scan), start[k + 1] one past its last.
//
// Kernel          what it does                                                   bytes
// k_mom_chunks    one wave per 64 slots: looks for chunk heads among its keys;    4 + 4 (key, start) per photon;
//                 the whole wave then sums a chunk (up to kMomChunk slots) and    32 per photon of a run longer than G;
//                 stores the cell (runs of one chunk) or the chunk's partial     96 per such cell / 88 per chunk
// k_mom_cells<G>  one wave per 64 consecutive interior cells, G lanes per cell:   8 (start) + 96 per cell;
//                 runs of 1 .. G slots are summed here; runs of more than one    32 per photon of a run of <= G;
//                 chunk have their partials added in chunk order; every cell     88 per chunk of a longer run
//                 that k_mom_chunks did not store is stored (zeros: empty cells,
//                 halo copies), a wave's 64 values of one component contiguous
// G is 1, 2, .. 64, chosen by the host from the mean number of photons per cell (C2: 0.6 -> 4, C3: 48 -> 64), so
// that most runs are summed by k_mom_cells with most of a group's lanes loading; the result does not depend on G.
//
// ORDER OF SUMMATION (the contract: a function of the position within the run alone, never of absolute slots).
// For each of the eleven sums (w; w w; p_d = w v_d; p_i v_j, i <= j -- every product rounded on its own):
//   * the run is cut into chunks of kMomChunk = 4096 slots counted from the run's head;
//   * in a chunk, lane l (0 .. 63) starts from +0.0 and adds the addends of elements l, l + 64, l + 128, .. in
//     rising order;
//   * the 64 lane sums are joined by  for d in 32, 16, 8, 4, 2, 1: s[l] = s[l] + s[l + d] for l < d;
//   * the run's sum is the first chunk's sum, then the further chunks' sums added in chunk order.
// A lane sum is never -0.0 (it starts from +0.0), so adding a lane that holds +0.0 changes no bit: a group of
// G >= L lanes with the joins d = G/2 .. 1 gives the bits of the 64-lane tree, and k_mom_cells<G> may take any run
// of L <= G.  E, F and Q are then the sum divided by dv = (dx0 dx1) dx2, one rounding; N is L; W2 is the sum.
//
// Determinism: no floating-point atomics, no workgroup waits for another; a chunk's partial has one writer and its
// place is a function of the chunk's head slot (two per aligned 4096 slots: at most one run can end and one begin
// with a chunk head in there).  The three integer atomics of k_mom_cells (a sum, a sum, a maximum) feed the
// report alone.
#pragma once

#include <hip/hip_runtime.h>

#include "jb_kernels.hpp"

namespace jb {

// (kMomSums, MS_*: jb_scratch_layout.hpp)
constexpr int kMomRows = 8;   // rows of 64 slots a wave of k_mom_chunks has loads in flight for: 16 KB

__device__ __forceinline__ double mom_load(const double *p) { return __builtin_nontemporal_load(p); }

// s <- s + the eleven addends of one photon
__device__ __forceinline__ void mom_add(double (&s)[kMomSums], double w, double vx, double vy, double vz) {
  const double px = w * vx, py = w * vy, pz = w * vz;
  s[0] = s[0] + w;
  s[1] = s[1] + w * w;
  s[2] = s[2] + px;
  s[3] = s[3] + py;
  s[4] = s[4] + pz;
  s[5] = s[5] + px * vx;
  s[6] = s[6] + px * vy;
  s[7] = s[7] + px * vz;
  s[8] = s[8] + py * vy;
  s[9] = s[9] + py * vz;
  s[10] = s[10] + pz * vz;
}
// the joins d = G/2 .. 1 over groups of G lanes: the group's sum lands in its first lane.  (The shuffle spans the
// wave: a lane whose place in its group is below d reads lane + d of its own group, and no other lane's value is
// used afterwards.)
template <int G>
__device__ __forceinline__ void mom_join(double (&s)[kMomSums]) {
#pragma unroll
  for (int d = G / 2; d > 0; d >>= 1) {
#pragma unroll
    for (int q = 0; q < kMomSums; ++q) s[q] = s[q] + __shfl_down(s[q], d, 64);
  }
}
// where the partial of the chunk whose head is slot s0 lives (first: the chunk is its run's first)
__device__ __forceinline__ size_t mom_part(unsigned s0, bool first) {
  return (size_t)kMomSums * (2u * (size_t)(s0 / (unsigned)kMomChunk) + (first ? 1u : 0u));
}
// component q + 1 of a cell from its sum: W2 is the sum itself
__device__ __forceinline__ double mom_value(int q, double sum, double dv) { return q == 1 ? sum : sum / dv; }

__device__ __forceinline__ double mom_dv(const DevMesh &M, int b) {
  return M.blk_dx[3 * b] * M.blk_dx[3 * b + 1] * M.blk_dx[3 * b + 2];
}

// Runs of more than gshort slots in interior cells of owned blocks, chunk by chunk.
__global__ void __launch_bounds__(kBlock)
    k_mom_chunks(DevMesh M, DevSwarm S, long long n, unsigned nkeys, const unsigned *key, const unsigned *start,
                 unsigned gshort, double *part, double *out) {
  const int lane = threadIdx.x & 63;
  const long long plane = (long long)M.nblocks * M.ncell;
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) - lane;
  for (long long base = wave0; base < n; base += (long long)gridDim.x * blockDim.x) {
    const long long s = base + lane;
    const unsigned k = s < n ? key[s] : nkeys;
    bool head = false;
    unsigned st = 0u, len = 0u;
    int b = 0;
    long long c = 0;
    if (k < nkeys) {
      st = start[k];
      len = start[k + 1] - st;
      if ((((unsigned)s - st) & (unsigned)(kMomChunk - 1)) == 0u && len > gshort) {
        b = (int)(k / (unsigned)M.ntot);
        const int q = (int)(k - (unsigned)b * (unsigned)M.ntot);
        const int kk = q / (M.ni * M.nj), r = q - kk * (M.ni * M.nj);
        const int j = r / M.ni, i = r - j * M.ni;
        head = M.owned[b] != 0 && i >= M.is && i <= M.ie && j >= M.js && j <= M.je && kk >= M.ks && kk <= M.ke;
        c = (long long)b * M.ncell + ((long long)(kk - M.ks) * M.nx[1] + (j - M.js)) * M.nx[0] + (i - M.is);
      }
    }
    unsigned long long heads = __ballot(head);
    while (heads != 0ull) {
      const int src = __ffsll((long long)heads) - 1;
      heads &= heads - 1ull;
      const unsigned st_c = __shfl(st, src, 64), len_c = __shfl(len, src, 64);
      const int b_c = __shfl(b, src, 64);
      const long long c_c = __shfl(c, src, 64);
      const unsigned s0 = (unsigned)(base + src), off = s0 - st_c;
      const unsigned m = len_c - off < (unsigned)kMomChunk ? len_c - off : (unsigned)kMomChunk;
      double acc[kMomSums];
#pragma unroll
      for (int q = 0; q < kMomSums; ++q) acc[q] = 0.0;
      // kMomRows rows of 64 slots in flight
      for (unsigned e0 = 0u; e0 < m; e0 += 64u * kMomRows) {
        double w[kMomRows], vx[kMomRows], vy[kMomRows], vz[kMomRows];
#pragma unroll
        for (int r = 0; r < kMomRows; ++r) {
          const unsigned e = e0 + 64u * (unsigned)r + (unsigned)lane;
          const size_t p = (size_t)s0 + e;
          const bool ok = e < m;
          w[r] = ok ? mom_load(S.w + p) : 0.0;
          vx[r] = ok ? mom_load(S.vx + p) : 0.0;
          vy[r] = ok ? mom_load(S.vy + p) : 0.0;
          vz[r] = ok ? mom_load(S.vz + p) : 0.0;
        }
#pragma unroll
        for (int r = 0; r < kMomRows; ++r)
          if (e0 + 64u * (unsigned)r + (unsigned)lane < m) mom_add(acc, w[r], vx[r], vy[r], vz[r]);
      }
      mom_join<64>(acc);
      if (lane == 0) {
        if (len_c <= (unsigned)kMomChunk) {
          const double dv = mom_dv(M, b_c);
          out[c_c] = (double)len_c;
#pragma unroll
          for (int q = 0; q < kMomSums; ++q) out[(long long)(q + 1) * plane + c_c] = mom_value(q, acc[q], dv);
        } else {
          double *o = part + mom_part(s0, off == 0u);
#pragma unroll
          for (int q = 0; q < kMomSums; ++q) o[q] = acc[q];
        }
      }
    }
  }
}

// Every interior cell of every resident block; stats: MS_COUNTED slots summed, MS_NONEMPTY cells, MS_LONGEST run.
template <int G>
__global__ void __launch_bounds__(kBlock)
    k_mom_cells(DevMesh M, DevSwarm S, const unsigned *start, const double *part, double *out,
                unsigned long long *stats) {
  constexpr int per = 64 / G;   // cells a wave takes per round
  const int lane = threadIdx.x & 63;
  const long long plane = (long long)M.nblocks * M.ncell;
  const long long nwaves = (plane + 63) / 64;
  const long long stride = ((long long)gridDim.x * blockDim.x) >> 6;
  unsigned long long counted = 0ull, nonempty = 0ull, longest = 0ull;
  for (long long wv = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wv < nwaves; wv += stride) {
    const long long c = wv * 64 + lane;
    const bool valid = c < plane;
    unsigned st = 0u, len = 0u;
    double dv = 1.0;
    if (valid) {
      int b, k, j, i, cell;
      decode_cell(M, c, b, k, j, i, cell);
      if (M.owned[b] != 0) {   // halo copies: zeros
        const unsigned key = (unsigned)b * (unsigned)M.ntot + (unsigned)cidx(M, k, j, i);
        st = start[key];
        len = start[key + 1] - st;
      }
      dv = mom_dv(M, b);
    }
    counted += len;
    nonempty += len > 0u ? 1ull : 0ull;
    longest = len > longest ? len : longest;
    double res[kMomSums];
#pragma unroll
    for (int q = 0; q < kMomSums; ++q) res[q] = 0.0;
    if (__ballot(len >= 1u && len <= (unsigned)G) != 0ull) {
#pragma unroll 1
      for (int r = 0; r < G; ++r) {
        const int cc = r * per + lane / G, g = lane % G;   // this group's cell among the wave's 64; my place in it
        const unsigned st_c = __shfl(st, cc, 64), len_c = __shfl(len, cc, 64);
        const bool here = len_c >= 1u && len_c <= (unsigned)G;
        if (__ballot(here) == 0ull) continue;
        double s[kMomSums];
#pragma unroll
        for (int q = 0; q < kMomSums; ++q) s[q] = 0.0;
        if (here && (unsigned)g < len_c) {
          const size_t p = (size_t)st_c + (unsigned)g;
          const double w = mom_load(S.w + p), vx = mom_load(S.vx + p), vy = mom_load(S.vy + p), vz = mom_load(S.vz + p);
          mom_add(s, w, vx, vy, vz);
        }
        if constexpr (G > 1) {
          mom_join<G>(s);
          const int from = ((lane - r * per) * G) & 63;   // the first lane of the group that took MY cell this round
          const bool mine = lane >= r * per && lane < (r + 1) * per;
#pragma unroll
          for (int q = 0; q < kMomSums; ++q) {
            const double v = __shfl(s[q], from, 64);
            if (mine) res[q] = v;
          }
        } else {
#pragma unroll
          for (int q = 0; q < kMomSums; ++q) res[q] = s[q];
        }
      }
    }
    // runs of one chunk that are longer than G are k_mom_chunks'; longer ones are joined below
    if (valid && len <= (unsigned)G) {
      out[c] = (double)len;
#pragma unroll
      for (int q = 0; q < kMomSums; ++q) out[(long long)(q + 1) * plane + c] = mom_value(q, res[q], dv);
    }
    unsigned long long longs = __ballot(len > (unsigned)kMomChunk);
    while (longs != 0ull) {
      const int src = __ffsll((long long)longs) - 1;
      longs &= longs - 1ull;
      const unsigned st_c = __shfl(st, src, 64), len_c = __shfl(len, src, 64);
      const double dv_c = __shfl(dv, src, 64);
      const long long c_c = wv * 64 + src;
      const unsigned nch = (len_c + (unsigned)kMomChunk - 1u) / (unsigned)kMomChunk;
      if (lane < kMomSums) {   // lane q: sum q, the chunks' partials in chunk order
        double acc = part[mom_part(st_c, true) + lane];
        for (unsigned ch = 1u; ch < nch; ++ch) acc = acc + part[mom_part(st_c + ch * (unsigned)kMomChunk, false) + lane];
        out[(long long)(lane + 1) * plane + c_c] = mom_value(lane, acc, dv_c);
      } else if (lane == kMomSums) {
        out[c_c] = (double)len_c;
      }
    }
  }
  counted = wave_sum(counted);
  nonempty = wave_sum(nonempty);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(longest, off, 64);
    longest = o > longest ? o : longest;
  }
  if (lane == 0) {   // integer sums and a maximum: the same whatever their order
    if (counted) atomicAdd(&stats[MS_COUNTED], counted);
    if (nonempty) atomicAdd(&stats[MS_NONEMPTY], nonempty);
    if (longest) atomicMax(&stats[MS_LONGEST], longest);
  }
}

}  // namespace jb
