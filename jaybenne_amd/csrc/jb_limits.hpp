// jb_limits.hpp -- the mesh-size limits that the tracking kernels are compiled for and that the host's
// kernel selection (jb_select.hpp) tests.  Plain C++: a host compiler reads it without HIP.
#pragma once

namespace jb {

// resident blocks whose per-block tables a kernel keeps in LDS (LdsBlockTableT, jb_device.hpp)
#ifndef JB_LDS_BLOCKS
#define JB_LDS_BLOCKS 128
#endif
constexpr int kLdsBlocks = JB_LDS_BLOCKS;
constexpr int kQBlocks = 64;   // ... of k_ddmc_q (k_ddmc_all: 128): with the queues the workgroup stays under
                               // 40 KB of LDS, i.e. four workgroups per CU
constexpr int kLdsTally = 1024;  // cells (all resident blocks, ghosts included) tallied in LDS
// interior cells (all resident blocks) whose 256-bit deposition accumulators a sweep keeps in LDS
// (jb_kernel_deposit.hpp): 32 bytes per cell, 32 KB per workgroup -- five workgroups per CU still fit
constexpr int kDepositLds = kLdsTally;
// cell codes of the all-DDMC kernel (DevMesh::ddmc_code)
constexpr int kMaxClasses = 256;            // 16 KB of LDS per workgroup at most
constexpr int kLdsRecCells = 256;    // cells whose step records k_ddmc_all<.., GATHER 2> copies to LDS (jb_kernel_ddmc.hpp)
constexpr int kLdsCodeCells = 1024;  // cells whose codes k_ddmc_q<.., LCODES> copies to LDS (jb_kernel_ddmc_q.hpp)
// elements a workgroup of the scan kernels takes (k_scan_*, jb_kernels.hpp: kBlock threads x kScanItems); the scratch
// layouts (jb_order_plan.hpp, jb_scratch_layout.hpp) size the scans' tile sums by it
constexpr int kScanTile = 2048;
// radiation moments (jb_kernel_moments.hpp): components per cell (JB_MOMENTS), and the slots of a cell's run that
// one wave sums -- a run is cut into chunks of this many slots from its head (a power of two, a multiple of 64)
constexpr int kMoments = 12;
constexpr int kMomChunk = 4096;
// radiation spectrum (jb_kernel_spectrum.hpp): frequency groups at the most (JB_SPECTRUM_MAX_GROUPS); a call with
// ngroups groups has ngroups + 1 edges and ngroups + 2 bins
constexpr int kSpecMaxGroups = 64;

}  // namespace jb
