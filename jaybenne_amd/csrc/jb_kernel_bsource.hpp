// jb_kernel_bsource.hpp -- the boundary source: Planckian inflow through chosen domain faces (gfx950, wave64).
//
// The reference sources photons inside the volume only (sourcing.cpp); nothing there comes in through a face.
// Here a face f (0..5 = ix1, ox1, ix2, ox2, ix3, ox3) of the domain that carries a temperature T_f > 0 is a
// black wall: every interior cell c of an owned block whose face f lies on it (a SOURCE FACE CELL) emits
//   E_c = sb T_f^4 A_c dt            (a c / 4 = sb: the one-sided flux of a black body; A_c from the block's widths)
// per cycle, in snpc = floor(npc) + (npc - floor(npc) > xi) photons of weight E_c / snpc, xi the first draw of
// the cell's stream in domain kRngDomainBoundary + f.  A photon is born where the reference leaves one that has
// just crossed that face (eps_imc dx inside the cell, transport_utils.hpp:151-159) with a cosine-law inward
// direction (sample_face_iso_dir in ptcl_ddmc_albedo's cyclic assignment, transport_utils.hpp:280-397), so that
// every tracking kernel takes it as it is: an IMC cell tracks it, a DDMC cell's albedo admits or reflects it.
//
// Kernel              shape
// k_bsource_count     one workgroup per block over the block's ENTRIES -- (face, face cell) in face order, cells in
//                     (k, j, i) order --: snpc, exclusive prefix (wave scan + LDS carry, as k_source_count), and per
//                     (block, face) the photon count and the energy, summed in a fixed order
// k_bsource_fill      one thread per new photon: block and entry by bisection (as k_source_fill), ten draws
#pragma once

#include <hip/hip_runtime.h>

#include "jb_kernels.hpp"

namespace jb {

// entries of one block: face f holds ncell / nx[f / 2] of them (the cells of one layer), all six faces always
struct BsLayout {
  int off[7];   // first entry of face f; off[6] = entries per block (the block's prefix has off[6] + 1 words)
};
__host__ __device__ inline BsLayout bsource_layout(const int nx[3], int ncell) {
  BsLayout L;
  L.off[0] = 0;
  for (int f = 0; f < 6; ++f) L.off[f + 1] = L.off[f] + ncell / nx[f >> 1];
  return L;
}

struct BsFaces {
  double temp[6];   // T_f; 0 = off
};
// (kernel arguments read at a run-time face number: by selects, so that the structs stay in scalar registers)
__device__ __forceinline__ double bsource_temp(const BsFaces &F, int f) {
  double t = F.temp[0];
#pragma unroll
  for (int q = 1; q < 6; ++q) t = f == q ? F.temp[q] : t;
  return t;
}
__device__ __forceinline__ int bsource_off(const BsLayout &L, int f) {
  int o = L.off[0];
#pragma unroll
  for (int q = 1; q < 6; ++q) o = f == q ? L.off[q] : o;
  return o;
}

// a value per axis picked by selects (an array indexed by a run-time axis would live in scratch memory)
template <class T>
__device__ __forceinline__ T sel3(int d, T a, T b, T c) {
  return d == 0 ? a : (d == 1 ? b : c);
}

// entry e of face f -> the interior cell (k, j, i, with ghosts) whose face f it is, and its flat interior index.
// The entries of a face are its cells in (k, j, i) order: the two transverse indices, the slower one first.
__device__ __forceinline__ void bsource_cell(const DevMesh &M, int f, int e, int &k, int &j, int &i, int &cell) {
  const int d = f >> 1;
  const int nlo = d == 0 ? M.nx[1] : M.nx[0];   // extent of the faster transverse axis
  const int q = e / nlo, r = e - q * nlo;
  const int fixed = (f & 1) ? sel3(d, M.nx[0], M.nx[1], M.nx[2]) - 1 : 0;
  const int i0 = d == 0 ? fixed : r;
  const int j0 = d == 0 ? r : (d == 1 ? fixed : q);
  const int k0 = d == 2 ? fixed : q;
  cell = (k0 * M.nx[1] + j0) * M.nx[0] + i0;
  i = i0 + M.is; j = j0 + M.js; k = k0 + M.ks;
}

// does face f of block b lie on the domain boundary?  (block corners are whole numbers of cells from gmin)
__device__ __forceinline__ bool bsource_on_boundary(const DevMesh &M, int b, int f) {
  const int d = f >> 1;
  const double half = 0.5 * M.blk_dx[3 * b + d];
  return (f & 1) ? M.blk_xmax[3 * b + d] > M.gmax[d] - half : M.blk_xmin[3 * b + d] < M.gmin[d] + half;
}

// E_c of a source face cell of block b: ((sb T^4) A) dt, A the product of the two transverse widths
__device__ __forceinline__ double bsource_cell_energy(const DevMesh &M, const DevParams &P, int b, int f, double temp,
                                                      double dt) {
  const int d = f >> 1;
  const double area = M.blk_dx[3 * b + (d + 1) % 3] * M.blk_dx[3 * b + (d + 2) % 3];
  const double t2 = temp * temp;
  return ((P.sb * (t2 * t2)) * area) * dt;
}

// a fixed-order sum over the workgroup: a shuffle tree within each wave, the four wave sums added in wave order
// by every thread (no floating-point atomics: the same call gives the same bits)
__device__ __forceinline__ double bsource_block_sum(double v, double *wave_part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = wave_part[0];
  for (int w = 1; w < kBlock / 64; ++w) s += wave_part[w];
  return s;
}

// prefix: [nblocks][off[6] + 1] -- exclusive over the block's entries, the block's total in the last word
// n_bf / e_bf: [nblocks][6] photons and energy per (block, face); nper_block: [nblocks]
__global__ void __launch_bounds__(kBlock)
    k_bsource_count(DevMesh M, DevParams P, BsFaces F, BsLayout L, double dt, double npc, uint32_t epoch,
                    int *nper_block, int *prefix, long long *n_bf, double *e_bf) {
  __shared__ int wave_tot[kBlock / 64];
  __shared__ int carry_s;
  __shared__ double wave_part[kBlock / 64];
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nent = L.off[6];
  int *pf = prefix + (long long)b * (nent + 1);
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const bool owned = M.owned[b] != 0;   // halo copies source nothing: their owner does
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    // (uniform per face: a face that is off, or not on the boundary, holds entries that count nothing)
    const bool on = owned && f < 2 * M.ndim && F.temp[f] > 0.0 && bsource_on_boundary(M, b, f);
    const double e_cell = on ? bsource_cell_energy(M, P, b, f, F.temp[f], dt) : 0.0;
    const int nface = L.off[f + 1] - L.off[f];
    const int first = carry_s;
    double e_sum = 0.0;   // the face's energy: chunk sums added in chunk order
    for (int base = 0; base < nface; base += kBlock) {
      const int e = base + threadIdx.x;
      int cnt = 0;
      if (on && e < nface) {
        int k, j, i, cell;
        bsource_cell(M, f, e, k, j, i, cell);
        LcgRng rng(rng_seed_state(P.key0, kRngDomainBoundary + (uint32_t)f, cell_stream_id(epoch, M.gid[b], cell)));
        double snpc = floor(npc);
        snpc += (double)((npc - snpc) > rng.drand());
        cnt = (int)rint(snpc);
      }
      // (the weight is e_cell / snpc; k_bsource_fill forms it again from the same operands)
      e_sum += bsource_block_sum(cnt > 0 ? e_cell : 0.0, wave_part);
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
      if (e < nface) pf[L.off[f] + e] = carry + wave_off + incl - cnt;
      __syncthreads();
      if (threadIdx.x == kBlock - 1) carry_s = carry + wave_off + incl;
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      n_bf[6 * b + f] = (long long)(carry_s - first);
      e_bf[6 * b + f] = e_sum;
    }
  }
  if (threadIdx.x == 0) {
    pf[nent] = carry_s;
    nper_block[b] = carry_s;
  }
}

__global__ void __launch_bounds__(kBlock)
    k_bsource_fill(DevMesh M, DevParams P, DevSwarm S, BsFaces F, BsLayout L, double t_start, double dt,
                   const int *prefix, const long long *blk_first, const long long *slot_base,
                   const unsigned long long *id_base, long long total) {
  load_math_tables();
  const int nent = L.off[6];
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total;
       g += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = M.nblocks - 1;  // last b with blk_first[b] <= g
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (blk_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int b = lo;
    const int np = (int)(g - blk_first[b]);
    const int *pf = prefix + (long long)b * (nent + 1);
    lo = 0; hi = nent - 1;  // last entry with pf[entry] <= np (empty entries share a prefix value: the LAST of
                            // them that still satisfies <= is the non-empty one)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pf[mid] <= np) lo = mid; else hi = mid - 1;
    }
    const int ent = lo;
    int f = 0;   // the face whose entries hold ent: off[] ascends
#pragma unroll
    for (int q = 1; q < 6; ++q) f += (int)(L.off[q] <= ent);
    const int d = f >> 1;
    const bool upper = (f & 1) != 0;
    int k, j, i, cell;
    bsource_cell(M, f, ent - bsource_off(L, f), k, j, i, cell);
    Blk B;
    load_block(M, b, B);
    const double temp = bsource_temp(F, f);
    const long long n = slot_base[b] + np;
    const uint64_t id = id_base[b] + (uint64_t)np;
    LcgRng rng(rng_stream_start(P.key0, id));
    S.ip[n] = i; S.jp[n] = j; S.kp[n] = k;
    S.blk[n] = b;
    S.status[n] = ST_ACTIVE;
    // the face's axis d and the transverse axes d + 1, d + 2 (cyclic), by selects
    const double c0 = xc(B, 0, i), c1 = xc(B, 1, j), c2 = xc(B, 2, k);
    const double cd = sel3(d, c0, c1, c2), ca = sel3(d, c1, c2, c0), cb = sel3(d, c2, c0, c1);
    const double wd = sel3(d, B.dx[0], B.dx[1], B.dx[2]), wa = sel3(d, B.dx[1], B.dx[2], B.dx[0]),
                 wb = sel3(d, B.dx[2], B.dx[0], B.dx[1]);
    // draw order: the two transverse coordinates (d + 1, d + 2); direction (2); Planck (5); time
    const double pa = ca + wa * (rng.drand() - 0.5);
    const double pb = cb + wb * (rng.drand() - 0.5);
    // eps_imc dx inside the cell, where a photon that has just crossed the face sits
    const double pd = upper ? (cd + 0.5 * wd) - kEpsImc * wd : (cd - 0.5 * wd) + kEpsImc * wd;
    double v1, v2, v3, px, py, pz, ux, uy, uz;
    sample_face_iso_dir(upper ? -P.c : P.c, rng, v1, v2, v3);
    assign_cyclic(d, pd, pa, pb, px, py, pz);
    assign_cyclic(d, v1, v2, v3, ux, uy, uz);
    S.x[n] = px; S.y[n] = py; S.z[n] = pz;
    S.vx[n] = ux; S.vy[n] = uy; S.vz[n] = uz;
    S.e[n] = sample_planck_energy(rng, P.sb, temp);
    const double snpc = (double)(pf[ent + 1] - pf[ent]);
    S.w[n] = bsource_cell_energy(M, P, b, f, temp, dt) / snpc;
    S.t[n] = t_start + rng.drand() * dt;
    S.id[n] = id;
    S.rng[n] = rng.s;
  }
}

}  // namespace jb
