// jb_kernel_spectrum.hpp -- the radiation spectrum of the census: per cell the energy density of its photons in
// frequency groups (include/jaybenne_amd.h: jb_evaluate_radiation_spectrum).  A sibling of jb_kernel_moments.hpp:
// the same sorted swarm, the same cells' bounds start[k] .. start[k + 1], the same order of summation, applied to
// every bin on its own.
//
// BIN of a photon: the number of edges j = 0 .. ngroups with edges[j] <= e, counted by comparisons alone (no
// logarithm, no reciprocal width): 0 below the first edge -- and for an e that is NaN, for which every comparison
// is false --, g = 1 .. ngroups in [edges[g - 1], edges[g]), ngroups + 1 at or above the last edge.  NB = ngroups + 2.
//
// Kernel            what it does                                                       bytes
// k_spec_chunks     one wave per 64 slots: looks for chunk heads among its keys; the    4 + 4 (key, start) per photon;
//                   whole wave then sums a chunk (up to kMomChunk slots) bin by bin     16 per photon of a run longer
//                   and stores the cell (runs of one chunk) or the chunk's partial      than G; 8 NB per cell / chunk
// k_spec_cells<G>   one wave per 64 consecutive interior cells, G lanes per cell:       8 (start) + 8 NB per cell;
//                   runs of 1 .. G slots are summed here; runs of more than one chunk   16 per photon of a run of <= G;
//                   have their partials added in chunk order; every cell that           8 NB per chunk of a longer run
//                   k_spec_chunks did not store is stored (zeros: empty cells, halo
//                   copies), a wave's 64 values of one bin contiguous
// Both read w and e alone of a photon (non-temporal loads).
//
// ORDER OF SUMMATION: jb_kernel_moments.hpp's, for each bin, over the positions of the cell's run -- chunks of
// kMomChunk slots from the run's head; lane l adds elements l, l + 64, .. in rising order, starting from +0.0; the
// joins d = 32 .. 1; the chunks' sums in chunk order.  A photon's addend to its own bin is w; for every other bin it
// is skipped.  A lane sum that starts from +0.0 is never -0.0, so skipping equals adding +0.0 bit for bit: the chunk
// kernel skips, the joins and the cell kernel add +0.0, and a bin no lane of a wave holds is left at +0.0 unjoined.
//
// The accumulators: a lane's NB sums are indexed by a bin known only at run time, which as a register array would
// go to scratch (jb_kernel_deposit.hpp records what that costs).  They lie in LDS as acc[bin][lane]: a wave's
// access to one bin is 64 consecutive doubles, and whatever bins the lanes hold, lane l's word is in the banks of
// column l.  A workgroup is ONE wave (kSpecBlock = 64): 512 NB + 8 (ngroups + 1) bytes of LDS, 34312 at the most,
// and the barriers between a wave's LDS phases order that wave alone.  The edges come as a kernel argument by value
// (SpecEdges: no copy to the device, nothing to wait for); the wave puts them behind the accumulators and reads them
// at a wave-uniform address, one read per edge for eight rows of photons.
//
// Determinism: no floating-point atomics, no workgroup waits for another; a chunk's partial has one writer and its
// place is a function of the chunk's head slot (jb_kernel_moments.hpp: two per aligned 4096 slots).  The integer
// atomics (sums and a maximum) feed the report alone.
#pragma once

#include <hip/hip_runtime.h>

#include "jb_kernel_moments.hpp"

namespace jb {

// (kSpecMaxGroups, SS_*: jb_scratch_layout.hpp)
constexpr int kSpecBlock = 64;   // threads per workgroup of both kernels: one wave
constexpr int kSpecRows = 8;     // rows of 64 slots a wave of k_spec_chunks has loads in flight for: 8 KB

extern __shared__ double spec_lds[];   // acc[NB][64], then edges[ngroups + 1]

struct SpecEdges {   // edges[0 .. ngroups] of a call, in the kernels' argument segment
  double v[kSpecMaxGroups + 1];
};

// the joins d = G/2 .. 1 over groups of G lanes (mom_join, one sum): the shuffle spans the wave
template <int G>
__device__ __forceinline__ double spec_join(double s) {
#pragma unroll
  for (int d = G / 2; d > 0; d >>= 1) s = s + __shfl_down(s, d, 64);
  return s;
}
// the edges into LDS, by the one wave of the workgroup
__device__ __forceinline__ void spec_edges_to_lds(double *sedges, const SpecEdges &edges, int ngroups, int lane) {
  for (int j = lane; j <= ngroups; j += 64) sedges[j] = edges.v[j];
  __syncthreads();
}

// Runs of more than gshort slots in interior cells of owned blocks, chunk by chunk.  stats: SS_BELOW, SS_ABOVE of
// the photons summed here.
__global__ void __launch_bounds__(kSpecBlock)
    k_spec_chunks(DevMesh M, DevSwarm S, long long n, unsigned nkeys, const unsigned *key, const unsigned *start,
                  unsigned gshort, SpecEdges edges, int ngroups, double *part, double *out,
                  unsigned long long *stats) {
  const int lane = threadIdx.x;
  const int nb = ngroups + 2;
  double *sacc = spec_lds, *sedges = spec_lds + 64 * nb;
  const long long plane = (long long)M.nblocks * M.ncell;
  bool have_edges = false;
  unsigned long long below = 0ull, above = 0ull;
  for (long long base = (long long)blockIdx.x * kSpecBlock; base < n; base += (long long)gridDim.x * kSpecBlock) {
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
    if (heads != 0ull && !have_edges) {   // (wave-uniform)
      spec_edges_to_lds(sedges, edges, ngroups, lane);
      have_edges = true;
    }
    while (heads != 0ull) {
      const int src = __ffsll((long long)heads) - 1;
      heads &= heads - 1ull;
      const unsigned st_c = __shfl(st, src, 64), len_c = __shfl(len, src, 64);
      const int b_c = __shfl(b, src, 64);
      const long long c_c = __shfl(c, src, 64);
      const unsigned s0 = (unsigned)(base + src), off = s0 - st_c;
      const unsigned m = len_c - off < (unsigned)kMomChunk ? len_c - off : (unsigned)kMomChunk;
      for (int q = 0; q < nb; ++q) sacc[64 * q + lane] = 0.0;
      // kSpecRows rows of 64 slots in flight; a lane's sums are its own column of acc
      for (unsigned e0 = 0u; e0 < m; e0 += 64u * kSpecRows) {
        double w[kSpecRows], en[kSpecRows];
        int bin[kSpecRows];
#pragma unroll
        for (int r = 0; r < kSpecRows; ++r) {
          const unsigned e = e0 + 64u * (unsigned)r + (unsigned)lane;
          const size_t p = (size_t)s0 + e;
          const bool ok = e < m;
          w[r] = ok ? mom_load(S.w + p) : 0.0;
          en[r] = ok ? mom_load(S.e + p) : 0.0;
          bin[r] = 0;
        }
        for (int j = 0; j <= ngroups; ++j) {
          const double edge = sedges[j];
#pragma unroll
          for (int r = 0; r < kSpecRows; ++r) bin[r] += edge <= en[r] ? 1 : 0;
        }
#pragma unroll
        for (int r = 0; r < kSpecRows; ++r)
          if (e0 + 64u * (unsigned)r + (unsigned)lane < m) {
            double *a = sacc + 64 * bin[r] + lane;
            *a = *a + w[r];
            below += bin[r] == 0 ? 1ull : 0ull;
            above += bin[r] == nb - 1 ? 1ull : 0ull;
          }
      }
      for (int q = 0; q < nb; ++q) {
        const double t = spec_join<64>(sacc[64 * q + lane]);
        if (lane == 0) sacc[64 * q] = t;
      }
      __syncthreads();
      // lane q, q + 64: bin q of the cell (runs of one chunk) or of the chunk's partial
      const bool single = len_c <= (unsigned)kMomChunk;
      const double dv = mom_dv(M, b_c);
      double *o = part + (size_t)nb * (2u * (size_t)(s0 / (unsigned)kMomChunk) + (off == 0u ? 1u : 0u));
      for (int q = lane; q < nb; q += 64) {
        const double t = sacc[64 * q];
        if (single) out[(long long)q * plane + c_c] = t / dv;
        else o[q] = t;
      }
      __syncthreads();
    }
  }
  below = wave_sum(below);
  above = wave_sum(above);
  if (lane == 0) {
    if (below) atomicAdd(&stats[SS_BELOW], below);
    if (above) atomicAdd(&stats[SS_ABOVE], above);
  }
}

// Every interior cell of every resident block; stats: SS_COUNTED slots summed, SS_NONEMPTY cells, SS_LONGEST run,
// and SS_BELOW, SS_ABOVE of the photons summed here.
template <int G>
__global__ void __launch_bounds__(kSpecBlock)
    k_spec_cells(DevMesh M, DevSwarm S, const unsigned *start, const double *part, SpecEdges edges, int ngroups,
                 double *out, unsigned long long *stats) {
  constexpr int per = 64 / G;   // cells a wave takes per round
  const int lane = threadIdx.x;
  const int nb = ngroups + 2;
  double *sacc = spec_lds, *sedges = spec_lds + 64 * nb;
  const long long plane = (long long)M.nblocks * M.ncell;
  const long long nwaves = (plane + 63) / 64;
  bool have_edges = false;
  unsigned long long counted = 0ull, nonempty = 0ull, longest = 0ull, below = 0ull, above = 0ull;
  for (long long wv = blockIdx.x; wv < nwaves; wv += gridDim.x) {
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
    const bool shorts = __ballot(len >= 1u && len <= (unsigned)G) != 0ull;   // (wave-uniform)
    if (shorts) {
      if (!have_edges) {
        spec_edges_to_lds(sedges, edges, ngroups, lane);
        have_edges = true;
      }
      for (int q = 0; q < nb; ++q) sacc[64 * q + lane] = 0.0;   // acc[bin][cell of the wave]
      __syncthreads();
#pragma unroll 1
      for (int r = 0; r < G; ++r) {
        const int cc = r * per + lane / G, g = lane % G;   // this group's cell among the wave's 64; my place in it
        const unsigned st_c = __shfl(st, cc, 64), len_c = __shfl(len, cc, 64);
        const bool here = len_c >= 1u && len_c <= (unsigned)G;
        if (__ballot(here) == 0ull) continue;
        double w = 0.0;
        int bin = -1;
        if (here && (unsigned)g < len_c) {
          const size_t p = (size_t)st_c + (unsigned)g;
          w = mom_load(S.w + p);
          const double en = mom_load(S.e + p);
          bin = 0;
          for (int j = 0; j <= ngroups; ++j) bin += sedges[j] <= en ? 1 : 0;
          below += bin == 0 ? 1ull : 0ull;
          above += bin == nb - 1 ? 1ull : 0ull;
        }
        for (int q = 0; q < nb; ++q) {
          if (__ballot(bin == q) == 0ull) continue;   // no lane holds it: the cells' +0.0 stand
          const double t = spec_join<G>(bin == q ? 0.0 + w : 0.0);
          if (here && g == 0) sacc[64 * q + cc] = t;
        }
      }
      __syncthreads();
    }
    // runs of one chunk that are longer than G are k_spec_chunks'; longer ones are joined below
    if (valid && len <= (unsigned)G)
      for (int q = 0; q < nb; ++q) out[(long long)q * plane + c] = (shorts ? sacc[64 * q + lane] : 0.0) / dv;
    if (shorts) __syncthreads();
    unsigned long long longs = __ballot(len > (unsigned)kMomChunk);
    while (longs != 0ull) {
      const int src = __ffsll((long long)longs) - 1;
      longs &= longs - 1ull;
      const unsigned st_c = __shfl(st, src, 64), len_c = __shfl(len, src, 64);
      const double dv_c = __shfl(dv, src, 64);
      const long long c_c = wv * 64 + src;
      const unsigned nch = (len_c + (unsigned)kMomChunk - 1u) / (unsigned)kMomChunk;
      const size_t p0 = 2u * (size_t)(st_c / (unsigned)kMomChunk) + 1u;
      for (int q = lane; q < nb; q += 64) {   // lane q, q + 64: bin q, the chunks' partials in chunk order
        double acc = part[(size_t)nb * p0 + q];
        for (unsigned ch = 1u; ch < nch; ++ch)
          acc = acc + part[(size_t)nb * (2u * (size_t)((st_c + ch * (unsigned)kMomChunk) / (unsigned)kMomChunk)) + q];
        out[(long long)q * plane + c_c] = acc / dv_c;
      }
    }
  }
  counted = wave_sum(counted);
  nonempty = wave_sum(nonempty);
  below = wave_sum(below);
  above = wave_sum(above);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(longest, off, 64);
    longest = o > longest ? o : longest;
  }
  if (lane == 0) {   // integer sums and a maximum: the same whatever their order
    if (counted) atomicAdd(&stats[SS_COUNTED], counted);
    if (nonempty) atomicAdd(&stats[SS_NONEMPTY], nonempty);
    if (longest) atomicMax(&stats[SS_LONGEST], longest);
    if (below) atomicAdd(&stats[SS_BELOW], below);
    if (above) atomicAdd(&stats[SS_ABOVE], above);
  }
}

}  // namespace jb
