// jb_kernel_comb.hpp -- census population control: an energy-conserving comb per cell
// (include/jaybenne_amd.h: jb_comb_census_plan / jb_comb_census_apply).  The reference has no such task.
//
// The swarm has just been sorted by (block, cell) -- jb_defrag_particles -- so the photons of a cell are a
// SEGMENT of consecutive slots with one key.  A cell that holds more than T ACTIVE photons comes out with
// exactly K: with W the cell's weight, D = W / K, C_j the running weight up to and including photon j of the
// cell (slot order) and xi one uniform per cell and epoch,
//     u_0 = 0,   u_j = clamp(ceil(C_j / D - xi), 0, K)  (j < m),   u_m = K,
// photon j comes out as k_j = u_j - u_(j-1) copies of weight D: sum k_j = K, k_j is floor or ceil of w_j / D,
// the expectation of k_j D over xi is w_j.
//
// Kernel             what it does                                                       bytes per photon
// k_comb_keys        the sort key of every slot                                         36 read, 4 written
// k_comb_unsorted    is the swarm in key order already?  (then the sort's move is left out)   4 read
// k_comb_seg_tiles   segmented inclusive scan of w inside tiles of kScanTile slots      12 read, 8 written
// k_comb_seg_sums    one workgroup: exclusive segmented scan of the tiles' (sum, flag)  -
// k_comb_seg_add     adds a tile's carry to the slots that continue the segment before  12 read, <= 8 written
//   (JB_CELL_ORDER_BY_ID: k_comb_cell_exp and k_comb_xseg_tiles / _sums / _add instead -- the same scan over exact
//   128-bit fixed-point weights, each C_j rounded once: below)
// k_comb_decide      k_j and max(k_j - 1, 0) per slot                                   ~20 read, 8 written
//   (k_scan_tiles / _sums / _add of the sort turn both into output slots and id offsets: 2 x 16)
// k_comb_cells       cells combed, largest cell (per-workgroup partials)                per cell
// k_comb_energy      sum of w over the ACTIVE slots (per-workgroup partials, fixed order)
// k_comb_pack        slot s, read in order -> its k_j records at dest[s] .. (128-byte records, as k_sort_pack)
//   (k_sort_unpack writes the records back into the swarm arrays)
//
// Determinism: no floating-point atomics, no workgroup waits for another.  Every sum is formed by a fixed tree
// -- a lane over its 8 slots in slot order, a wave by shuffles, a workgroup over its waves in wave order, the
// tiles by one workgroup in tile order -- so the same sorted swarm gives the same bits.  C_(j-1) is always the
// value the scan stored for the neighbouring slot, never C_j - w_j: u_j of one photon and u_(j-1) of the next
// are then the same number and the k_j of a cell sum to K exactly.
// A segment may be empty, or longer than a wave, a workgroup or any number of tiles: the carry of a tile is
// the running sum of the segment that is open at its start, whatever the number of tiles it began before.
#pragma once

#include <hip/hip_runtime.h>

#include "jb_kernels.hpp"

namespace jb {

// (sum of the open segment, "a segment started in here")
struct SegPair {
  double s;
  unsigned f;
};
// a, then b
__device__ __forceinline__ SegPair seg_join(SegPair a, SegPair b) {
  return SegPair{b.f ? b.s : a.s + b.s, a.f | b.f};
}
__device__ __forceinline__ SegPair seg_shfl_up(SegPair v, int d) {
  return SegPair{__shfl_up(v.s, d, 64), (unsigned)__shfl_up((int)v.f, d, 64)};
}
// inclusive scan over the wave; `ex` the exclusive one (identity in lane 0)
__device__ __forceinline__ SegPair seg_wave_scan(SegPair mine, int lane, SegPair &ex) {
  SegPair incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const SegPair up = seg_shfl_up(incl, d);
    if (lane >= d) incl = seg_join(up, incl);
  }
  ex = seg_shfl_up(incl, 1);
  if (lane == 0) ex = SegPair{0.0, 0u};
  return incl;
}

__global__ void __launch_bounds__(kBlock)
    k_comb_keys(DevMesh M, DevSwarm S, long long n, unsigned nkeys, unsigned *key) {
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x)
    key[p] = sort_key(M, S, p, nkeys);
}

// *unsorted = 1 when some slot's key is lower than that of the slot before it (every writer stores the same word)
__global__ void __launch_bounds__(kBlock) k_comb_unsorted(const unsigned *key, long long n, unsigned *unsorted) {
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x + 1; p < n; p += (long long)gridDim.x * blockDim.x)
    if (key[p] < key[p - 1]) *unsorted = 1u;
}

// C[i] = sum of w over the slots of i's segment up to i that lie in i's tile; (sum, flag) of the tile
__global__ void __launch_bounds__(kBlock)
    k_comb_seg_tiles(const unsigned *key, const double *w, long long n, double *C, double *tsum, unsigned *tflag) {
  __shared__ double wave_s[kBlock / 64];
  __shared__ unsigned wave_f[kBlock / 64];
  const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
  unsigned prev = (base > 0 && base - 1 < n) ? key[base - 1] : 0u;
  double v[kScanItems], run = 0.0;
  unsigned heads = 0u;   // bit q: slot base + q starts a segment
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    const long long i = base + q;
    bool head = true;    // (slots behind the swarm: empty segments of their own)
    double wi = 0.0;
    if (i < n) {
      const unsigned k = key[i];
      head = i == 0 || k != prev;
      prev = k;
      wi = w[i];
    }
    run = head ? wi : run + wi;
    v[q] = run;
    if (head) heads |= 1u << q;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  SegPair ex;
  const SegPair incl = seg_wave_scan(SegPair{run, heads != 0u ? 1u : 0u}, lane, ex);
  if (lane == 63) {
    wave_s[wave] = incl.s;
    wave_f[wave] = incl.f;
  }
  __syncthreads();
  SegPair before{0.0, 0u}, total{0.0, 0u};
#pragma unroll
  for (int q = 0; q < kBlock / 64; ++q) {
    const SegPair p{wave_s[q], wave_f[q]};
    if (q < wave) before = seg_join(before, p);
    total = seg_join(total, p);
  }
  const SegPair open = seg_join(before, ex);   // what precedes this lane's slots in the tile
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    if (base + q >= n) break;
    const bool continues = (heads & ((2u << q) - 1u)) == 0u;   // no segment started at or before q in this lane
    C[base + q] = continues ? open.s + v[q] : v[q];
  }
  if (threadIdx.x == 0) {
    tsum[blockIdx.x] = total.s;
    tflag[blockIdx.x] = total.f;
  }
}

// one workgroup, any count: tsum[t] <- the sum of the segment that is open where tile t starts
__global__ void __launch_bounds__(1024) k_comb_seg_sums(double *tsum, const unsigned *tflag, int count) {
  __shared__ double wave_s[16];
  __shared__ unsigned wave_f[16];
  __shared__ double carry_s;
  __shared__ unsigned carry_f;
  if (threadIdx.x == 0) {
    carry_s = 0.0;
    carry_f = 0u;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s0 = 0; s0 < count; s0 += 1024) {
    const int q = s0 + (int)threadIdx.x;
    const SegPair mine = q < count ? SegPair{tsum[q], tflag[q]} : SegPair{0.0, 0u};
    SegPair ex;
    const SegPair incl = seg_wave_scan(mine, lane, ex);
    if (lane == 63) {
      wave_s[wave] = incl.s;
      wave_f[wave] = incl.f;
    }
    __syncthreads();
    SegPair before{0.0, 0u}, total{0.0, 0u};
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const SegPair t{wave_s[p], wave_f[p]};
      if (p < wave) before = seg_join(before, t);
      total = seg_join(total, t);
    }
    const SegPair carry{carry_s, carry_f};
    if (q < count) tsum[q] = seg_join(carry, seg_join(before, ex)).s;
    __syncthreads();
    if (threadIdx.x == 0) {
      const SegPair c = seg_join(carry, total);
      carry_s = c.s;
      carry_f = c.f;
    }
    __syncthreads();
  }
}

// the slots at the start of a tile that continue the segment of the slot before the tile
__global__ void __launch_bounds__(kBlock)
    k_comb_seg_add(const unsigned *key, long long n, double *C, const double *tsum) {
  if (blockIdx.x == 0) return;
  const long long tile0 = (long long)blockIdx.x * kScanTile;
  const unsigned kprev = key[tile0 - 1];
  const double add = tsum[blockIdx.x];
  const long long base = tile0 + (long long)threadIdx.x * kScanItems;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q)
    if (base + q < n && key[base + q] == kprev) C[base + q] = add + C[base + q];
}

// ---- the running weights of the canonical order (JB_CELL_ORDER_BY_ID): exact, so that they are a function of the
// cell's photons alone.  The sums above are trees aligned to absolute slots: the same cell at another offset in the
// swarm (another rank count, other cells before it) gets other roundings.  Here every weight becomes a 128-bit
// fixed-point number on a scale set by the largest weight of its cell (its mantissa at bits 42..94: 2^32 photons
// fit below bit 127, weights 2^-95 of the largest and less are truncated), integer addition is associative, and
// C_j is the one rounding of the exact prefix sum.  Negative weights count as zero; a cell with a weight that is
// not finite gets C = inf and is left alone.
struct U128 {
  unsigned long long lo, hi;
};
__device__ __forceinline__ U128 u128_add(U128 a, U128 b) {
  U128 r;
  r.lo = a.lo + b.lo;
  r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ull : 0ull);
  return r;
}
struct XSegPair {
  U128 s;
  unsigned f;
};
__device__ __forceinline__ XSegPair xseg_join(XSegPair a, XSegPair b) {
  return XSegPair{b.f ? b.s : u128_add(a.s, b.s), a.f | b.f};
}
__device__ __forceinline__ XSegPair xseg_shfl_up(XSegPair v, int d) {
  return XSegPair{U128{__shfl_up(v.s.lo, d, 64), __shfl_up(v.s.hi, d, 64)}, (unsigned)__shfl_up((int)v.f, d, 64)};
}
__device__ __forceinline__ XSegPair xseg_wave_scan(XSegPair mine, int lane, XSegPair &ex) {
  XSegPair incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const XSegPair up = xseg_shfl_up(incl, d);
    if (lane >= d) incl = xseg_join(up, incl);
  }
  ex = xseg_shfl_up(incl, 1);
  if (lane == 0) ex = XSegPair{U128{0ull, 0ull}, 0u};
  return incl;
}
// the exponent field of a weight as the cell's scale sees it: 0 for a negative weight, 0x7ff for inf / nan
__device__ __forceinline__ unsigned comb_wexp(double w) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(w);
  const unsigned e = (unsigned)(b >> 52) & 0x7ffu;
  if (e == 0x7ffu) return e;
  return (b >> 63) ? 0u : e;
}
// w on the scale of a cell whose largest exponent field is emax
__device__ __forceinline__ U128 comb_wfixed(double w, unsigned emax) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(w);
  const unsigned e = (unsigned)(b >> 52) & 0x7ffu;
  if ((b >> 63) || emax == 0x7ffu || e > emax) return U128{0ull, 0ull};
  const unsigned long long mant = (b & 0xfffffffffffffull) | (e ? 0x10000000000000ull : 0ull);
  const int sh = (int)(e ? e : 1u) - (int)(emax ? emax : 1u) + 42;   // <= 42
  if (sh >= 0) return U128{mant << sh, sh ? mant >> (64 - sh) : 0ull};
  return U128{-sh < 64 ? mant >> -sh : 0ull, 0ull};
}
__device__ __forceinline__ unsigned comb_start(const unsigned *ends, unsigned k) { return k > 0u ? ends[k - 1] : 0u; }

// cexp[first slot of the cell] = the largest exponent field among the cell's weights (cexp zeroed before; integer
// maxima: the same whatever their order; one atomic per wave where the wave lies within one cell)
__global__ void __launch_bounds__(kBlock)
    k_comb_cell_exp(const unsigned *key, const double *w, const unsigned *ends, long long n, unsigned *cexp) {
  const int lane = threadIdx.x & 63;
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) - lane;
  for (long long base = wave0; base < n; base += (long long)gridDim.x * blockDim.x) {
    const long long s = base + lane;
    const bool active = s < n;
    const unsigned k = active ? key[s] : 0u;
    unsigned e = active ? comb_wexp(w[s]) : 0u;
    const unsigned k0 = (unsigned)__shfl((int)k, 0, 64);
    const bool one_cell = __ballot(active && k != k0) == 0ull;
    if (one_cell) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_down((int)e, off, 64);
        e = o > e ? o : e;
      }
      if (lane == 0) atomicMax(&cexp[comb_start(ends, k0)], e);
    } else if (active) {
      atomicMax(&cexp[comb_start(ends, k)], e);
    }
  }
}

// k_comb_seg_tiles / _sums / _add over the fixed-point weights
__global__ void __launch_bounds__(kBlock)
    k_comb_xseg_tiles(const unsigned *key, const double *w, const unsigned *ends, const unsigned *cexp, long long n,
                      U128 *C, U128 *tsum, unsigned *tflag) {
  __shared__ U128 wave_s[kBlock / 64];
  __shared__ unsigned wave_f[kBlock / 64];
  const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
  unsigned prev = (base > 0 && base - 1 < n) ? key[base - 1] : 0u;
  unsigned emax = 0u;
  U128 v[kScanItems], run{0ull, 0ull};
  unsigned heads = 0u;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    const long long i = base + q;
    bool head = true;
    U128 wi{0ull, 0ull};
    if (i < n) {
      const unsigned k = key[i];
      head = i == 0 || k != prev;
      if (head || q == 0) emax = cexp[comb_start(ends, k)];
      prev = k;
      wi = comb_wfixed(w[i], emax);
    }
    run = head ? wi : u128_add(run, wi);
    v[q] = run;
    if (head) heads |= 1u << q;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  XSegPair ex;
  const XSegPair incl = xseg_wave_scan(XSegPair{run, heads != 0u ? 1u : 0u}, lane, ex);
  if (lane == 63) {
    wave_s[wave] = incl.s;
    wave_f[wave] = incl.f;
  }
  __syncthreads();
  XSegPair before{U128{0ull, 0ull}, 0u}, total{U128{0ull, 0ull}, 0u};
#pragma unroll
  for (int q = 0; q < kBlock / 64; ++q) {
    const XSegPair p{wave_s[q], wave_f[q]};
    if (q < wave) before = xseg_join(before, p);
    total = xseg_join(total, p);
  }
  const XSegPair open = xseg_join(before, ex);
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    if (base + q >= n) break;
    const bool continues = (heads & ((2u << q) - 1u)) == 0u;
    C[base + q] = continues ? u128_add(open.s, v[q]) : v[q];
  }
  if (threadIdx.x == 0) {
    tsum[blockIdx.x] = total.s;
    tflag[blockIdx.x] = total.f;
  }
}
__global__ void __launch_bounds__(1024) k_comb_xseg_sums(U128 *tsum, const unsigned *tflag, int count) {
  __shared__ U128 wave_s[16];
  __shared__ unsigned wave_f[16];
  __shared__ U128 carry_s;
  __shared__ unsigned carry_f;
  if (threadIdx.x == 0) {
    carry_s = U128{0ull, 0ull};
    carry_f = 0u;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s0 = 0; s0 < count; s0 += 1024) {
    const int q = s0 + (int)threadIdx.x;
    const XSegPair mine = q < count ? XSegPair{tsum[q], tflag[q]} : XSegPair{U128{0ull, 0ull}, 0u};
    XSegPair ex;
    const XSegPair incl = xseg_wave_scan(mine, lane, ex);
    if (lane == 63) {
      wave_s[wave] = incl.s;
      wave_f[wave] = incl.f;
    }
    __syncthreads();
    XSegPair before{U128{0ull, 0ull}, 0u}, total{U128{0ull, 0ull}, 0u};
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const XSegPair t{wave_s[p], wave_f[p]};
      if (p < wave) before = xseg_join(before, t);
      total = xseg_join(total, t);
    }
    const XSegPair carry{carry_s, carry_f};
    if (q < count) tsum[q] = xseg_join(carry, xseg_join(before, ex)).s;
    __syncthreads();
    if (threadIdx.x == 0) {
      const XSegPair c = xseg_join(carry, total);
      carry_s = c.s;
      carry_f = c.f;
    }
    __syncthreads();
  }
}
// adds the tile's carry where the slot continues the segment before the tile, and rounds every exact prefix sum
// once: Cd[s] = C[s] * 2^(scale of the cell)
__global__ void __launch_bounds__(kBlock)
    k_comb_xseg_add(const unsigned *key, const unsigned *ends, const unsigned *cexp, long long n, const U128 *C,
                    const U128 *tsum, double *Cd) {
  const long long tile0 = (long long)blockIdx.x * kScanTile;
  const bool first = blockIdx.x == 0;
  const unsigned kprev = first ? 0u : key[tile0 - 1];
  const U128 add = first ? U128{0ull, 0ull} : tsum[blockIdx.x];
  const long long base = tile0 + (long long)threadIdx.x * kScanItems;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    const long long i = base + q;
    if (i >= n) break;
    const unsigned k = key[i];
    U128 c = C[i];
    if (!first && k == kprev) c = u128_add(add, c);
    const unsigned emax = cexp[comb_start(ends, k)];
    double d;
    if (emax == 0x7ffu) d = __builtin_huge_val();
    else d = ldexp((double)c.hi * 18446744073709551616.0 + (double)c.lo, (int)(emax ? emax : 1u) - 42 - 1075);
    Cd[i] = d;
  }
}

// The slots [start, end) of cell k of the sorted swarm (ends[k]: k_sort_pack leaves the histogram's offsets at the
// END of every cell; behind the scan alone they are the cells' starts, and ends is that array from entry 1 on)
// and whether the cell is combed: more than T photons, and a weight the rule can divide.
__device__ __forceinline__ bool comb_cell(const unsigned *ends, const double *C, unsigned k, unsigned T,
                                          unsigned &start, unsigned &end, double &W) {
  start = k > 0u ? ends[k - 1] : 0u;
  end = ends[k];
  if (end - start <= T) return false;
  W = C[end - 1];
  return W > 0.0 && W < __builtin_huge_val();
}
// xi of the cell: one uniform in (0,1) per (epoch, global block, cell index in the block's array)
__device__ __forceinline__ double comb_xi(uint32_t seed, uint32_t epoch, int gblock, unsigned cell) {
  return u52_to_double(rng_seed_state(seed, kRngDomainComb, cell_stream_id(epoch, gblock, (int)cell)) >> 12);
}
__device__ __forceinline__ unsigned comb_u(double C, double delta, double xi, unsigned K) {
  const double r = ceil(C / delta - xi);
  if (!(r > 0.0)) return 0u;
  return r >= (double)K ? K : (unsigned)r;
}

// kcnt[s] = copies slot s comes out as, extra[s] = new ids it needs; entry n of both is 0 (the scans' totals
// land there).  Slots of cells that are not combed, and the slots behind all cells: one copy, themselves.
__global__ void __launch_bounds__(kBlock)
    k_comb_decide(DevMesh M, long long n, unsigned nkeys, const unsigned *key, const unsigned *ends, const double *C,
                  unsigned T, unsigned K, uint32_t seed, uint32_t epoch, unsigned *kcnt, unsigned *extra) {
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s <= n; s += (long long)gridDim.x * blockDim.x) {
    unsigned cnt = s < n ? 1u : 0u;
    const unsigned k = s < n ? key[s] : nkeys;
    if (k < nkeys) {
      unsigned start, end;
      double W;
      if (comb_cell(ends, C, k, T, start, end, W)) {
        const double delta = W / (double)K;
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

// per workgroup: partials[2 g] = cells combed, partials[2 g + 1] = most photons in one cell
__global__ void __launch_bounds__(kBlock)
    k_comb_cells(unsigned nkeys, const unsigned *ends, const double *C, unsigned T, unsigned long long *partials) {
  __shared__ unsigned long long lds_c[kBlock / 64], lds_m[kBlock / 64];
  unsigned long long combed = 0ull, most = 0ull;
  for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < nkeys;
       k += (unsigned long long)gridDim.x * blockDim.x) {
    unsigned start, end;
    double W;
    if (comb_cell(ends, C, (unsigned)k, T, start, end, W)) ++combed;
    if (end - start > most) most = end - start;
  }
  combed = wave_sum(combed);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(most, off, 64);
    most = o > most ? o : most;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    lds_c[wave] = combed;
    lds_m[wave] = most;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < kBlock / 64; ++q) {
      combed += lds_c[q];
      most = lds_m[q] > most ? lds_m[q] : most;
    }
    partials[2 * blockIdx.x] = combed;
    partials[2 * blockIdx.x + 1] = most;
  }
}

// per workgroup: the weight of the ACTIVE slots it walks (the grid is a function of n alone)
__global__ void __launch_bounds__(kBlock) k_comb_energy(DevSwarm S, long long n, double *partials) {
  __shared__ double lds_e[kBlock / 64];
  double e = 0.0;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (long long)gridDim.x * blockDim.x)
    if (S.status[s] == ST_ACTIVE) e += S.w[s];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds_e[wave] = e;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < kBlock / 64; ++q) e += lds_e[q];
    partials[blockIdx.x] = e;
  }
}

// The move: slot s, read in order, becomes kcnt[s] records at dest[s] .. -- the layout and the staging of
// k_sort_pack (one wave stages its 64 records in LDS, eight lanes store one record with one instruction).
// The destinations rise with s, so the stores of a wave are nearly sequential.  Every copy of a photon of a
// combed cell carries the weight W / K; the first keeps id and stream state, copy c >= 1 takes the id
// id_base + idoff[s] + c - 1 and the start of that id's stream.
__global__ void __launch_bounds__(kBlock)
    k_comb_pack(DevSwarm S, long long n, unsigned nkeys, const unsigned *key, const unsigned *ends, const double *C,
                const unsigned *dest, const unsigned *idoff, unsigned T, unsigned K, uint32_t seed,
                unsigned long long id_base, unsigned long long *rec) {
  typedef unsigned long long u64;
  typedef u64 v2u __attribute__((ext_vector_type(2)));
  __shared__ __attribute__((aligned(16))) u64 stage[kBlock / 64][64][kSortRowWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) - lane;
  for (long long base = wave0; base < n; base += (long long)gridDim.x * blockDim.x) {
    const long long s = base + lane;
    const bool active = s < n;
    unsigned d0 = 0u, cnt = 0u, io = 0u;
    if (active) {
      d0 = dest[s];
      cnt = dest[s + 1] - d0;
      io = idoff[s];
      double w = S.w[s];
      const unsigned k = key[s];
      if (k < nkeys) {
        unsigned start, end;
        double W;
        if (comb_cell(ends, C, k, T, start, end, W)) w = W / (double)K;
      }
      sort_stage(&stage[wave][lane][0], S, s, w);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int piece = lane & 7;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = 8 * j + (lane >> 3);                     // the record these eight lanes store
      const unsigned d = __shfl(d0, row, 64);
      const unsigned c = __shfl(cnt, row, 64);
      const unsigned o = __shfl(io, row, 64);
      if (base + row < n && c > 0u) {
        v2u v = *(const v2u *)&stage[wave][row][2 * piece];
        *(v2u *)(rec + (size_t)kSortRecWords * (size_t)d + 2 * piece) = v;
        for (unsigned q = 1u; q < c; ++q) {
          const u64 id = id_base + (u64)o + (u64)(q - 1u);
          if (piece == 4) v.y = id;
          if (piece == 5) v.x = rng_stream_start(seed, id);
          *(v2u *)(rec + (size_t)kSortRecWords * ((size_t)d + q) + 2 * piece) = v;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace jb
