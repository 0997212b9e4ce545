// jb_kernel_tilt.hpp -- the source tilt (include/jaybenne_amd.h: jb_set_source_tilt): within a cell the emission
// probability of the thermal and the emission source varies linearly along every active axis, following the
// gradient of T^4 taken from the neighbouring cells, instead of being uniform (sourcing.cpp:175-177).  Off by
// default; the boundary source, whose photons start on a face, has none.
//
// k_source_tilt<NDIM>   one thread per interior cell of the owned resident blocks, cells in (k, j, i) order: one
//                       slope s_d in [-1, 1] per active axis into tilt[(b NDIM + d) ncell + cell].  A wave holds 64
//                       consecutive cells of a row along x1, so the centre load and each of the 2 NDIM neighbour
//                       loads (the same row moved by one cell, one row or one plane) is one contiguous run per
//                       row, and so is each of the NDIM stores.  No atomics, no LDS, no scratch.
// k_source_fill_tilt    k_source_fill with the tilted position lines: the same draws in the same order.
//
// Every operation below is individually rounded (-ffp-contract=off); tests/tilt_model.py restates them in numpy.
#pragma once

#include "jb_kernel_bsource.hpp"
#include "jb_kernels.hpp"

namespace jb {

// E = (T T) (T T), T as k_source_count forms it
__device__ __forceinline__ double tilt_e4(const DevMesh &M, const DevParams &P, int b, long long q) {
  // (gcptr: the table entries are pointers loaded from memory; said to be global memory, the loads are global_load)
  const double temp = eos_temperature(P, ((gcptr)M.rho[b])[q], ((gcptr)M.sie[b])[q]);
  const double t2 = temp * temp;
  return t2 * t2;
}

// s = clamp((E_p - E_m) / (4 E_c), -1, 1); 0 where E_c is zero or the quotient is not finite
__device__ __forceinline__ double tilt_slope(double e_c, double e_m, double e_p) {
  const double s_raw = (e_p - e_m) / (4.0 * e_c);
  const double s = fmin(fmax(s_raw, -1.0), 1.0);
  return (e_c == 0.0 || !isfinite(s_raw)) ? 0.0 : s;
}

// The slope of cell (k, j, i) of block b along D.  idx, first, last: the cell's index on D and the block's first
// and last interior one; stride: cells between neighbours on D.  The neighbour behind a block face is the block's
// own ghost cell (the hosts keep it current; k_face_prob reads the same cells) -- except behind a NON-PERIODIC DOMAIN
// face, where it counts as the cell itself and the ghost cell, whose content nobody defines, is not read.
template <int D>
__device__ __forceinline__ double tilt_axis(const DevMesh &M, const DevParams &P, int b, long long q, double e_c,
                                            int idx, int first, int last, long long stride) {
  const bool wall_m = idx == first && M.bc[2 * D] != BC_PERIODIC && bsource_on_boundary(M, b, 2 * D);
  const bool wall_p = idx == last && M.bc[2 * D + 1] != BC_PERIODIC && bsource_on_boundary(M, b, 2 * D + 1);
  double e_m = e_c, e_p = e_c;
  if (!wall_m) e_m = tilt_e4(M, P, b, q - stride);
  if (!wall_p) e_p = tilt_e4(M, P, b, q + stride);
  return tilt_slope(e_c, e_m, e_p);
}

template <int NDIM>
__global__ void __launch_bounds__(kBlock) k_source_tilt(DevMesh M, DevParams P, double *tilt) {
  const long long total = (long long)M.nblocks * M.ncell;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < total;
       c += (long long)gridDim.x * blockDim.x) {
    int b, k, j, i, cell;
    decode_cell(M, c, b, k, j, i, cell);
    if (!M.owned[b]) continue;   // halo copies source nothing: their owner does
    const long long q = cidx(M, k, j, i);
    const double e_c = tilt_e4(M, P, b, q);
    double *o = tilt + (long long)b * NDIM * M.ncell + cell;
    o[0] = tilt_axis<0>(M, P, b, q, e_c, i, M.is, M.ie, 1);
    if constexpr (NDIM >= 2) o[M.ncell] = tilt_axis<1>(M, P, b, q, e_c, j, M.js, M.je, M.ni);
    if constexpr (NDIM >= 3) o[2ll * M.ncell] = tilt_axis<2>(M, P, b, q, e_c, k, M.ks, M.ke, (long long)M.ni * M.nj);
  }
}

// u in [-1, 1 - 2^-52] with density (1 + s u) / 2 from one uniform draw xi in [0, 1): the inverse of
// (u + 1) / 2 + s (u^2 - 1) / 4 = xi in the form that does not cancel for small s (the denominator is >= 1).
// s = 0 gives 2 xi - 1 exactly.  A function of (s, xi) alone: the project's exactly rounded sqrt and division.
// (the radicand (1 - s)^2 + 4 s xi is >= 0 before rounding; one that rounding took to 0 or below has the root 0)
__device__ __forceinline__ double tilt_sample_u(double s, double xi) {
  const double a = 1.0 - s;
  const double arg = a * a + (4.0 * s) * xi;
  const double root = arg > 0.0 ? m_sqrt(arg) : 0.0;
  const double u = m_div((4.0 * xi - 2.0) + s, 1.0 + root);
  return fmax(fmin(u, 1.0 - 0x1p-52), -1.0);
}

// the position on axis d of a photon of cell `cell` of block b from the draw of that axis
// (an inactive axis has the slope 0, for which the tilted form has the bits of xc + dx (xi - 0.5))
__device__ __forceinline__ double tilt_position(const DevMesh &M, const double *tilt, int b, int cell, int d,
                                                double xcen, double dx, double xi) {
  const double s = d < M.ndim ? tilt[((long long)b * M.ndim + d) * M.ncell + cell] : 0.0;
  return xcen + (0.5 * dx) * tilt_sample_u(s, xi);
}

// k_source_fill (jb_kernels.hpp), which stays as it is, with the three position lines replaced; tilt:
// k_source_tilt's slopes of the count call this fill belongs to.  A sibling rather than a template argument of
// k_source_fill: the default kernel keeps its machine code, instruction for instruction.
__global__ void __launch_bounds__(kBlock)
    k_source_fill_tilt(DevMesh M, DevParams P, DevSwarm S, int source_type, double t_start, double dt,
                       const int *prefix, const long long *blk_first, const long long *slot_base,
                       const unsigned long long *id_base, const long long *ord_first, long long total,
                       const double *tilt) {
  load_math_tables();
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total;
       g += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = M.nblocks - 1;  // last b with blk_first[b] <= g
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (blk_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int b = lo;
    const int nq = (int)(g - blk_first[b]);
    const int np = nq + (ord_first ? (int)ord_first[b] : 0);
    const int *pf = prefix + (long long)b * M.ncell;
    lo = 0; hi = M.ncell - 1;  // last cell with pf[cell] <= np
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pf[mid] <= np) lo = mid; else hi = mid - 1;
    }
    const int cell = lo;
    int k = cell / (M.nx[0] * M.nx[1]);
    const int r = cell - k * (M.nx[0] * M.nx[1]);
    int j = r / M.nx[0];
    int i = r - j * M.nx[0];
    k += M.ks; j += M.js; i += M.is;
    const long long q = cidx(M, k, j, i);
    Blk B;
    load_block(M, b, B);
    const long long n = slot_base[b] + nq;
    const uint64_t id = id_base[b] + (uint64_t)np;
    LcgRng rng(rng_stream_start(P.key0, id));
    S.ip[n] = i; S.jp[n] = j; S.kp[n] = k;
    S.blk[n] = b;
    S.status[n] = ST_ACTIVE;
    // the draws of k_source_fill in its order: x, y, z; theta, phi; Planck (5); emission: time
    S.x[n] = tilt_position(M, tilt, b, cell, 0, xc(B, 0, i), B.dx[0], rng.drand());
    S.y[n] = tilt_position(M, tilt, b, cell, 1, xc(B, 1, j), B.dx[1], rng.drand());
    S.z[n] = tilt_position(M, tilt, b, cell, 2, xc(B, 2, k), B.dx[2], rng.drand());
    const double theta = m_acos(2.0 * rng.drand() - 1.0);
    const double xi_phi = rng.drand();  // phi = 2 pi xi
    double sth, cth, sph, cph;
    m_sincos(theta, sth, cth);
    m_sincos2pi(xi_phi, sph, cph);
    S.vx[n] = P.c * sth * cph;
    S.vy[n] = P.c * sth * sph;
    S.vz[n] = P.c * cth;
    const double rho = M.rho[b][q];
    const double temp = eos_temperature(P, rho, M.sie[b][q]);
    S.e[n] = sample_planck_energy(rng, P.sb, temp);
    S.w[n] = M.src_ew[b][q];
    if (source_type == 1) {
      S.t[n] = t_start + rng.drand() * dt;
    } else {
      S.t[n] = 0.0;
    }
    S.id[n] = id;
    S.rng[n] = rng.s;
  }
}

}  // namespace jb
