// jb_scratch_layout.hpp -- where the arrays of the swarm sort (jb_defrag_particles), of the census comb
// (jb_comb_census_plan / _apply), of the radiation moments (jb_evaluate_radiation_moments) and of the radiation
// spectrum (jb_evaluate_radiation_spectrum) lie in the library's scratch memory: the single statement of that
// layout.  An array is a Span -- its first byte from the start of the scratch memory, its elements and their size
// --; jb_api.hip turns a layout into pointers and asks it for the size, so the two cannot disagree.  Pure functions
// of a few scalars; tests/scratch_layout_test.cpp holds every offset to the arithmetic these functions replaced.
// Plain C++17: no HIP include.
#pragma once

#include <cstddef>

#include "jb_limits.hpp"
#include "jb_order_plan.hpp"

namespace jb {

constexpr int kSortRecWords = 16;        // 8-byte words per particle record of the sort's move (jb_kernels.hpp)
constexpr int kCombParts = 1024;         // workgroups of k_comb_cells / k_comb_energy at the most
constexpr int kMomSums = kMoments - 1;   // the rounded sums: components 1 .. 11 (component 0 is the count)
enum { MS_COUNTED = 0, MS_NONEMPTY, MS_LONGEST, MS_N };   // the counts of k_mom_cells' report
enum { SS_COUNTED = 0, SS_NONEMPTY, SS_LONGEST, SS_BELOW, SS_ABOVE, SS_N };   // ... of the spectrum kernels'

struct Span {
  size_t off = 0;     // first byte, from the start of the scratch memory
  size_t count = 0;   // elements
  size_t elem = 0;    // bytes per element
  size_t end() const { return off + count * elem; }
};

// The sort keys of a mesh: one per cell of every resident block (ghosts included), and the bin behind all cells
// for the slots that are not ACTIVE.  Keys and slot indices are 32-bit words on the device.
enum CellKeysOver { KEYS_FIT = 0, KEYS_PARTICLES, KEYS_CELLS };   // n >= 2^32 | nkeys >= 2^32 - 1
struct CellKeys {
  unsigned nkeys = 0;
  long long nbins = 0;   // nkeys + 1
  int sort_tiles = 0;    // tiles of kScanTile over the bins
  int over = KEYS_FIT;   // (then the other members are not set)
};
inline CellKeys cell_keys(long long nblocks, long long ntot, long long n) {
  CellKeys k;
  const unsigned long long nkeys = (unsigned long long)nblocks * (unsigned long long)ntot;
  if (n >= (1ll << 32)) k.over = KEYS_PARTICLES;
  else if (nkeys >= (1ull << 32) - 1ull) k.over = KEYS_CELLS;
  if (k.over) return k;
  k.nkeys = (unsigned)nkeys;
  k.nbins = (long long)nkeys + 1;
  k.sort_tiles = (int)((k.nbins + kScanTile - 1) / kScanTile);
  return k;
}

// The sort: the particle records (128 bytes each, from the first byte of the scratch memory), then three arrays of
// 4-byte words -- the histogram of the keys, which its scan turns into the cells' starts and the move into their
// ends; the scan's tile sums; the keys -- and, under JB_CELL_ORDER_BY_ID, the arrays of the canonical sort behind
// them (jb_order_plan.hpp: order_layout, whose offsets are 8-byte words from the same start).
struct SortLayout {
  int sort_tiles = 0;
  Span rec, hist, sums, key;
  bool by_id = false;
  OrderLayout order;   // (by_id)
  size_t words = 0;    // 8-byte words in all
};
inline SortLayout sort_layout(long long n, long long nbins, bool by_id) {
  SortLayout L;
  if (n < 0) n = 0;
  L.sort_tiles = (int)((nbins + kScanTile - 1) / kScanTile);
  L.rec = {0, (size_t)n, 8 * (size_t)kSortRecWords};
  L.hist = {L.rec.end(), (size_t)nbins, 4};
  L.sums = {L.hist.end(), (size_t)L.sort_tiles, 4};
  L.key = {L.sums.end(), (size_t)n, 4};
  L.words = (size_t)kSortRecWords * (size_t)n + (size_t)((nbins + L.sort_tiles + n) / 2 + 16);
  L.by_id = by_id;
  if (by_id) {
    L.order = order_layout(n, L.words);
    L.words = L.order.end;
  }
  return L;
}

// The comb, behind the sort: the running weights C, the copies kept / ids drawn per slot (n + 1 entries each: their
// scans leave the totals in the last), those scans' tile sums, the segmented scan's tile sums and flags, the
// per-workgroup parts of the report and of the energy.  C128 and tsum128 are the 128-bit running weights of the
// canonical order: they lie IN the records, which nothing uses before the move (fits_records()).
struct CombLayout {
  SortLayout sort;
  int ntiles = 0;   // tiles of kScanTile over the n + 1 slots
  Span C, kcnt, extra, ssum, tsum, tflag, cpart, epart;
  Span C128, tsum128;
  size_t words = 0;
  bool fits_records() const { return C128.end() <= tsum128.off && tsum128.end() <= sort.rec.end(); }
};
inline CombLayout comb_layout(long long n, long long nbins, bool by_id) {
  CombLayout c;
  if (n < 0) n = 0;
  c.sort = sort_layout(n, nbins, by_id);
  c.ntiles = (int)((n + 1 + kScanTile - 1) / kScanTile);
  const size_t nt = (size_t)c.ntiles, slots = (size_t)n + 1;
  size_t o = 8 * c.sort.words;
  auto take = [&o](size_t count, size_t elem) {   // (every array starts on an 8-byte word)
    const Span s{o, count, elem};
    o += (count * elem + 7) / 8 * 8;
    return s;
  };
  c.C = take((size_t)n, 8);
  c.kcnt = take(slots, 4);
  c.extra = take(slots, 4);
  c.ssum = take(nt, 4);
  c.tsum = take(nt, 8);
  c.tflag = take(nt, 4);
  c.cpart = take(2 * (size_t)kCombParts, 8);
  c.epart = take((size_t)kCombParts, 8);
  c.words = o / 8;
  c.C128 = {0, (size_t)n, 16};
  c.tsum128 = {c.C128.end(), nt, 16};
  return c;
}

// The global comb (jb_comb_census_weigh / _plan_global / _apply), behind the comb: everything comb_layout(n) has
// where it is -- the plan's kernels use those arrays as the comb's do, the report's kGcombStats counts per workgroup
// (kGcombParts workgroups) lie in cpart --, then the cells' targets (n + 1 words, one at the first slot of every
// occupied cell) and, when the move may fill more records than the swarm had slots (n_room > n), an output-record
// span of n_room records of its own: the comb's records end where the histogram begins.  For n_room <= n the move
// goes to the sort's records and `out` is empty.
constexpr int kGcombStats = 6;   // per workgroup: cells thinned, cells split, largest m_k, largest K_k, and of the
                                 // combed cells the photons they hold and the copies they come out as
constexpr int kGcombParts = 2 * kCombParts / kGcombStats;   // workgroups whose counts fit the comb's 2 x kCombParts words
struct GcombLayout {
  CombLayout comb;
  Span ktgt, out;
  size_t words = 0;
  const Span &records() const { return out.count ? out : comb.sort.rec; }   // where the move writes
};
inline GcombLayout gcomb_layout(long long n, long long n_room, long long nbins, bool by_id) {
  GcombLayout g;
  if (n < 0) n = 0;
  g.comb = comb_layout(n, nbins, by_id);
  size_t o = 8 * g.comb.words;
  g.ktgt = {o, (size_t)n + 1, 4};
  o += (g.ktgt.count * 4 + 7) / 8 * 8;
  o = (o + 15) / 16 * 16;   // (records are stored 16 bytes at a time)
  g.out = {o, n_room > n ? (size_t)n_room : 0, 8 * (size_t)kSortRecWords};
  g.words = g.out.end() / 8;
  return g;
}

// The moments, behind the sort: the chunks' partial sums (two places of kMomSums doubles per kMomChunk slots), the
// counts of the report, the "out of order" flag.
struct MomLayout {
  SortLayout sort;
  Span part, stats, flag;
  size_t words = 0;
};
inline MomLayout mom_layout(long long n, long long nbins, bool by_id) {
  MomLayout m;
  if (n < 0) n = 0;
  m.sort = sort_layout(n, nbins, by_id);
  m.part = {8 * m.sort.words, (size_t)kMomSums * 2 * (size_t)((n + kMomChunk - 1) / kMomChunk), 8};
  m.stats = {m.part.end(), (size_t)MS_N, 8};
  m.flag = {m.stats.end(), 1, 4};
  m.words = m.flag.off / 8 + 1;
  return m;
}

// The spectrum, behind the sort: the chunks' partial sums (two places of nbins_e = ngroups + 2 doubles per
// kMomChunk slots, as the moments'), the counts of the report, the "out of order" flag.  (The edges are a kernel
// argument.)
struct SpecLayout {
  SortLayout sort;
  Span part, stats, flag;
  size_t words = 0;
};
inline SpecLayout spectrum_layout(long long n, long long nbins, bool by_id, int ngroups) {
  SpecLayout s;
  if (n < 0) n = 0;
  s.sort = sort_layout(n, nbins, by_id);
  s.part = {8 * s.sort.words, (size_t)(ngroups + 2) * 2 * (size_t)((n + kMomChunk - 1) / kMomChunk), 8};
  s.stats = {s.part.end(), (size_t)SS_N, 8};
  s.flag = {s.stats.end(), 1, 4};
  s.words = s.flag.off / 8 + 1;
  return s;
}

}  // namespace jb
