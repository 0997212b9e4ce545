// jb_kernel_salloc.hpp -- energy-proportional source allocation (include/jaybenne_amd.h: jb_set_source_allocation):
// SourcePhotons gives a cell photons in proportion to the energy it sources instead of the same number to every
// cell (sourcing.cpp:68-69), so the new photons carry nearly equal weights.  Off by default.
//
// k_salloc_energy   one workgroup per block.  Per interior cell, in (k, j, i) order, erad with the expressions and
//                   the product order of k_source_count, stored in src_ew (which stages it for k_salloc_count: both
//                   kernels see the same bits); e_block[b] = the block's sum in a FIXED order -- thread t adds cells
//                   t, t + 256, ... in rising order from +0.0, then an LDS tree s[t] += s[t + d], d = 128 ... 1.
//                   No floating-point atomics; a halo copy gives 0 and writes no field.
// k_salloc_count    one workgroup per block.  Per cell nu = erad scale, n = floor(nu) + ((nu - floor(nu)) > xi) with
//                   xi the one draw of the cell's rounding stream (the stream k_source_count draws from), src_num = n,
//                   src_ew = erad / n (floor(nu) >= 1), erad / nu (roulette: floor(nu) = 0, n = 1) or 0 (n = 0); then
//                   the exclusive prefix and the block's count as k_source_count forms them.
// k_salloc_edelta   energy_delta = -(n src_ew), one product per cell (k_source_edelta subtracts one weight at a
//                   time: up to N trips in one thread when one cell holds the energy); +0 for the thermal source.
//
// Every operation is individually rounded (-ffp-contract=off) and none mixes a product with a sum;
// tests/source_alloc_model.py restates them in numpy.
#pragma once

#include "jb_kernels.hpp"

namespace jb {

// (k, j, i) and the field index of interior cell `cell` of a block, as k_source_count decodes them
__device__ __forceinline__ long long salloc_cell_index(const DevMesh &M, int cell) {
  int k = cell / (M.nx[0] * M.nx[1]);
  const int r = cell - k * (M.nx[0] * M.nx[1]);
  int j = r / M.nx[0];
  int i = r - j * M.nx[0];
  k += M.ks; j += M.js; i += M.is;
  return cidx(M, k, j, i);
}

__global__ void __launch_bounds__(kBlock)
    k_salloc_energy(DevMesh M, DevParams P, int source_type, double dt, double *e_block) {
  __shared__ double s[kBlock];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  if (!M.owned[b]) {   // halo copies source nothing: their owner does (uniform over the workgroup)
    if (t == 0) e_block[b] = 0.0;
    return;
  }
  const double dv = M.blk_dx[3 * b] * M.blk_dx[3 * b + 1] * M.blk_dx[3 * b + 2];
  double acc = 0.0;
  for (int cell = t; cell < M.ncell; cell += kBlock) {
    const long long q = salloc_cell_index(M, cell);
    const double rho = M.rho[b][q];
    const double temp = eos_temperature(P, rho, M.sie[b][q]);
    double erad;
    if (source_type == 0) {  // thermal: (4 sb / c) T^4 dV   (sourcing.cpp:93)
      const double t2 = temp * temp;
      erad = (4.0 * P.sb / P.c) * (t2 * t2) * dv;
    } else {  // emission: f j dV dt   (sourcing.cpp:95-96)
      erad = M.fleck[b][q] * opac_emissivity(P, rho, temp) * dv * dt;
    }
    M.src_ew[b][q] = erad;
    acc += erad;
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

__global__ void __launch_bounds__(kBlock)
    k_salloc_count(DevMesh M, DevParams P, double scale, uint32_t epoch, int *nper_block, int *prefix) {
  __shared__ int wave_tot[kBlock / 64];
  __shared__ int carry_s;
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < M.ncell; base += kBlock) {
    const int cell = base + threadIdx.x;
    int cnt = 0;
    if (cell < M.ncell && M.owned[b]) {
      const long long q = salloc_cell_index(M, cell);
      LcgRng rng(rng_seed_state(P.key0, kRngDomainCell, cell_stream_id(epoch, M.gid[b], cell)));
      const double erad = M.src_ew[b][q];   // staged by k_salloc_energy
      const double nu = erad * scale;
      const double f = floor(nu);
      const double n = f + (double)((nu - f) > rng.drand());
      double ew = 0.0;
      if (f >= 1.0) ew = erad / n;          // the cell's energy is sourced exactly
      else if (n == 1.0) ew = erad / nu;    // roulette: one photon of about E_tot / N with probability nu
      M.src_num[b][q] = n;
      M.src_ew[b][q] = ew;
      cnt = (int)rint(n);
    }
    // inclusive scan within the wave, LDS across the 4 waves, running carry over chunks of 256 cells
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    int wave_off = 0;
    for (int w = 0; w < wv; ++w) wave_off += wave_tot[w];
    const int carry = carry_s;
    if (cell < M.ncell) prefix[(long long)b * M.ncell + cell] = carry + wave_off + incl - cnt;
    __syncthreads();
    if (threadIdx.x == kBlock - 1) carry_s = carry + wave_off + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) nper_block[b] = carry_s;
}

__global__ void __launch_bounds__(kBlock) k_salloc_edelta(DevMesh M, int source_type) {
  const long long total = (long long)M.nblocks * M.ncell;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < total;
       c += (long long)gridDim.x * blockDim.x) {
    int b, k, j, i, cell;
    decode_cell(M, c, b, k, j, i, cell);
    if (!M.owned[b]) continue;
    const long long q = cidx(M, k, j, i);
    M.edelta[b][q] = source_type == 1 ? -(M.src_num[b][q] * M.src_ew[b][q]) : 0.0;
  }
}

}  // namespace jb
