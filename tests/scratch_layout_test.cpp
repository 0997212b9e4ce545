// The scratch layouts of the sort, the comb and the moments (jaybenne_amd/csrc/jb_scratch_layout.hpp) on the host
// (tests/test_scratch_layout_host.py).  The arithmetic the header replaced -- it stood in jb_api.hip, written out at
// every user -- is restated here with literal numbers, and every offset and size must equal it: the header moved no
// array.  Then what that arithmetic only implied: alignment, no overlap, everything inside the size asked for, the
// 128-bit overlays inside the records.  And cell_keys from both sides of its limits.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../jaybenne_amd/csrc/jb_scratch_layout.hpp"

using namespace jb;

static int failures = 0, rows = 0;
static long long case_n = 0, case_nbins = 0;
static int case_by_id = 0;
#define EXPECT(cond)                                                                                          \
  do {                                                                                                        \
    ++rows;                                                                                                   \
    if (!(cond)) {                                                                                            \
      std::printf("FAILED line %d (n %lld nbins %lld by_id %d): %s\n", __LINE__, case_n, case_nbins, case_by_id, #cond); \
      ++failures;                                                                                             \
    }                                                                                                         \
  } while (0)

// ---- the earlier arithmetic, in 8-byte words unless it says bytes ------------------------------------------
struct Frozen {
  int ntiles;
  size_t sort_words;                      // sort_scratch_words
  size_t hist_b, sums_b, key_b;           // jb_defrag_particles, order_sort, comb_scratch, mom_scratch: bytes
  size_t pairs0, pairs1, dest, cnt, csum, flags;   // order_layout behind the counting sort's arrays
  long long order_tiles, order_ncnt, order_scan_tiles;
};
static Frozen frozen_sort(long long n, long long nbins, bool by_id) {
  Frozen f{};
  f.ntiles = (int)((nbins + 2048 - 1) / 2048);
  const size_t words = (size_t)16 * (size_t)n + (size_t)((nbins + f.ntiles + n) / 2 + 16);
  const size_t rec_words = (size_t)16 * (size_t)n;
  f.hist_b = 8 * rec_words;                        // hist = (unsigned *)(rec + rec_words)
  f.sums_b = f.hist_b + 4 * (size_t)nbins;         // sums = hist + nbins
  f.key_b = f.sums_b + 4 * (size_t)f.ntiles;       // key = sums + ntiles
  f.sort_words = words;
  if (by_id) {
    f.order_tiles = (n + 2047) / 2048;
    f.order_ncnt = 256 * f.order_tiles;
    f.order_scan_tiles = (f.order_ncnt + 2047) / 2048;
    size_t o = words;
    f.pairs0 = o; o += (size_t)n;
    f.pairs1 = o; o += (size_t)n;
    f.dest = o; o += ((size_t)n + 1) / 2;
    f.cnt = o; o += ((size_t)f.order_ncnt + 1) / 2;
    f.csum = o; o += ((size_t)f.order_scan_tiles + 1) / 2;
    f.flags = o; o += 2;
    f.sort_words = o;
  }
  return f;
}
struct FrozenComb {
  int ntiles;
  size_t C, kcnt, extra, ssum, tsum, tflag, cpart, epart, words;
};
static FrozenComb frozen_comb(long long n, size_t sort_words) {
  FrozenComb c{};
  c.ntiles = (int)((n + 1 + 2048 - 1) / 2048);
  const size_t nt = (size_t)c.ntiles, half = (size_t)(n + 2) / 2;
  size_t o = sort_words;
  c.C = o; o += (size_t)n;
  c.kcnt = o; o += half;
  c.extra = o; o += half;
  c.ssum = o; o += (nt + 1) / 2;
  c.tsum = o; o += nt;
  c.tflag = o; o += (nt + 1) / 2;
  c.cpart = o; o += 2 * 1024;
  c.epart = o; o += 1024;
  c.words = o;
  return c;
}
struct FrozenMom {
  size_t part, stats, flag, words;
};
static FrozenMom frozen_mom(long long n, size_t sort_words) {
  FrozenMom m{};
  size_t o = sort_words;
  m.part = o; o += (size_t)11 * 2 * (size_t)((n + 4096 - 1) / 4096);
  m.stats = o; o += 3;
  m.flag = o; o += 1;
  m.words = o;
  return m;
}

// ---- what the arithmetic only implied -----------------------------------------------------------------------
struct Named {
  const char *name;
  Span a;
};
static void sort_arrays(const SortLayout &L, std::vector<Named> &v) {
  v.push_back({"rec", L.rec});
  v.push_back({"hist", L.hist});
  v.push_back({"sums", L.sums});
  v.push_back({"key", L.key});
  if (!L.by_id) return;
  const OrderLayout &O = L.order;
  const size_t n = L.key.count;
  v.push_back({"pairs0", {8 * O.pairs[0], n, 8}});
  v.push_back({"pairs1", {8 * O.pairs[1], n, 8}});
  v.push_back({"dest", {8 * O.dest, n, 4}});
  v.push_back({"cnt", {8 * O.cnt, (size_t)O.ncnt, 4}});
  v.push_back({"csum", {8 * O.csum, (size_t)O.scan_tiles, 4}});
  v.push_back({"flags", {8 * O.flags, 2, 8}});
}
static void well_formed(std::vector<Named> v, size_t words) {
  for (const Named &x : v) {
    EXPECT(x.a.elem > 0 && x.a.off % x.a.elem == 0);
    EXPECT(x.a.elem < 8 || x.a.off % 8 == 0);
    EXPECT(x.a.end() <= 8 * words);
  }
  std::sort(v.begin(), v.end(), [](const Named &x, const Named &y) {
    return x.a.off != y.a.off ? x.a.off < y.a.off : x.a.count < y.a.count;   // (an empty array may share its offset)
  });
  for (size_t q = 0; q + 1 < v.size(); ++q) {
    ++rows;
    if (v[q].a.end() > v[q + 1].a.off) {
      std::printf("FAILED (n %lld nbins %lld by_id %d): %s [%zu, %zu) overlaps %s at %zu\n", case_n, case_nbins, case_by_id,
                  v[q].name, v[q].a.off, v[q].a.end(), v[q + 1].name, v[q + 1].a.off);
      ++failures;
    }
  }
}

static void one_case(long long n, long long nbins, bool by_id) {
  case_n = n; case_nbins = nbins; case_by_id = by_id ? 1 : 0;
  const Frozen f = frozen_sort(n, nbins, by_id);
  // ---- the sort
  const SortLayout S = sort_layout(n, nbins, by_id);
  EXPECT(S.sort_tiles == f.ntiles && S.words == f.sort_words && S.by_id == by_id);
  EXPECT(S.rec.off == 0 && S.rec.elem == 128 && S.rec.count == (size_t)n);
  EXPECT(S.hist.off == f.hist_b && S.hist.elem == 4 && S.hist.count == (size_t)nbins);
  EXPECT(S.sums.off == f.sums_b && S.sums.elem == 4 && S.sums.count == (size_t)f.ntiles);
  EXPECT(S.key.off == f.key_b && S.key.elem == 4 && S.key.count == (size_t)n);
  // (order_sort: key = (unsigned *)(base + 16 n) + nbins + ntiles)
  EXPECT(S.key.off == 8 * (size_t)16 * (size_t)n + 4 * ((size_t)nbins + (size_t)f.ntiles));
  if (by_id) {
    const OrderLayout &O = S.order;
    EXPECT(O.pairs[0] == f.pairs0 && O.pairs[1] == f.pairs1 && O.dest == f.dest && O.cnt == f.cnt);
    EXPECT(O.csum == f.csum && O.flags == f.flags && O.end == f.sort_words);
    EXPECT(O.tiles == f.order_tiles && O.ncnt == f.order_ncnt && O.scan_tiles == f.order_scan_tiles);
  }
  std::vector<Named> v;
  sort_arrays(S, v);
  well_formed(v, S.words);
  // ---- the comb
  const FrozenComb fc = frozen_comb(n, f.sort_words);
  const CombLayout C = comb_layout(n, nbins, by_id);
  EXPECT(C.sort.words == S.words && C.sort.key.off == S.key.off && C.sort.hist.off == S.hist.off &&
         C.sort.sums.off == S.sums.off && C.sort.order.flags == S.order.flags);
  EXPECT(C.ntiles == fc.ntiles && C.words == fc.words);
  EXPECT(C.C.off == 8 * fc.C && C.C.elem == 8 && C.C.count == (size_t)n);
  EXPECT(C.kcnt.off == 8 * fc.kcnt && C.kcnt.elem == 4 && C.kcnt.count == (size_t)n + 1);
  EXPECT(C.extra.off == 8 * fc.extra && C.extra.elem == 4 && C.extra.count == (size_t)n + 1);
  EXPECT(C.ssum.off == 8 * fc.ssum && C.ssum.elem == 4 && C.ssum.count == (size_t)fc.ntiles);
  EXPECT(C.tsum.off == 8 * fc.tsum && C.tsum.elem == 8 && C.tsum.count == (size_t)fc.ntiles);
  EXPECT(C.tflag.off == 8 * fc.tflag && C.tflag.elem == 4 && C.tflag.count == (size_t)fc.ntiles);
  EXPECT(C.cpart.off == 8 * fc.cpart && C.cpart.elem == 8 && C.cpart.count == 2 * 1024);
  EXPECT(C.epart.off == 8 * fc.epart && C.epart.elem == 8 && C.epart.count == 1024);
  // (U128 *C128 = (U128 *)c.rec, *tsum128 = C128 + n)
  EXPECT(C.C128.off == 0 && C.C128.elem == 16 && C.C128.count == (size_t)n);
  EXPECT(C.tsum128.off == 16 * (size_t)n && C.tsum128.elem == 16 && C.tsum128.count == (size_t)fc.ntiles);
  EXPECT(C.tsum128.count == ((size_t)n + 1 + 2047) / 2048);
  if (n >= 1) EXPECT(C.fits_records() && C.C128.end() <= C.sort.rec.end() && C.tsum128.end() <= C.sort.rec.end());
  EXPECT(C.C128.off % 16 == 0 && C.tsum128.off % 16 == 0);
  v.clear();
  sort_arrays(C.sort, v);
  for (const Named &x : {Named{"C", C.C}, Named{"kcnt", C.kcnt}, Named{"extra", C.extra}, Named{"ssum", C.ssum},
                         Named{"tsum", C.tsum}, Named{"tflag", C.tflag}, Named{"cpart", C.cpart}, Named{"epart", C.epart}})
    v.push_back(x);
  well_formed(v, C.words);
  // ---- the moments
  const FrozenMom fm = frozen_mom(n, f.sort_words);
  const MomLayout M = mom_layout(n, nbins, by_id);
  EXPECT(M.sort.words == S.words && M.sort.key.off == S.key.off && M.sort.hist.off == S.hist.off &&
         M.sort.sums.off == S.sums.off);
  EXPECT(M.words == fm.words);
  EXPECT(M.part.off == 8 * fm.part && M.part.elem == 8 && M.part.count == (size_t)22 * (size_t)((n + 4095) / 4096));
  EXPECT(M.stats.off == 8 * fm.stats && M.stats.elem == 8 && M.stats.count == 3);
  EXPECT(M.flag.off == 8 * fm.flag && M.flag.elem == 4 && M.flag.count == 1);
  v.clear();
  sort_arrays(M.sort, v);
  for (const Named &x : {Named{"part", M.part}, Named{"stats", M.stats}, Named{"flag", M.flag}}) v.push_back(x);
  well_formed(v, M.words);
}

int main() {
  static_assert(kScanTile == 2048 && kSortRecWords == 16 && kCombParts == 1024 && kMomSums == 11 && MS_N == 3 &&
                    kMomChunk == 4096,
                "the constants the frozen arithmetic spells out");
  for (long long n : {0ll, 1ll, 2ll, 63ll, 64ll, 2047ll, 2048ll, 2049ll, 4095ll, 4096ll, 4097ll, (1ll << 20) + 1,
                      (1ll << 32) - 1})
    for (long long nbins : {2ll, 3ll, 2048ll, 2049ll, 2050ll, 4097ll, (1ll << 22) + 1, (1ll << 32) - 1})
      for (bool by_id : {false, true}) one_case(n, nbins, by_id);

  // ---- cell_keys: both sides of each limit, and of a scan tile of bins
  case_n = case_nbins = case_by_id = -1;
  {
    const CellKeys k = cell_keys(2, 4, (1ll << 32) - 1);
    EXPECT(k.over == KEYS_FIT && k.nkeys == 8u && k.nbins == 9 && k.sort_tiles == 1);
    EXPECT(cell_keys(2, 4, 1ll << 32).over == KEYS_PARTICLES);
  }
  {
    const CellKeys k = cell_keys(2, (1ll << 31) - 1, 5);   // 2^32 - 2 cells
    EXPECT(k.over == KEYS_FIT && k.nkeys == 0xFFFFFFFEu && k.nbins == (1ll << 32) - 1 && k.sort_tiles == (1 << 21));
    EXPECT(cell_keys(3, 1431655765ll, 5).over == KEYS_CELLS);   // 2^32 - 1
    EXPECT(cell_keys(1 << 16, 1 << 16, 5).over == KEYS_CELLS);  // 2^32
    EXPECT(cell_keys(3, 1431655765ll, 1ll << 32).over == KEYS_PARTICLES);   // (the particles are asked first)
  }
  {
    const CellKeys a = cell_keys(1, 2047, 0), b = cell_keys(1, 2048, 0);   // nbins = kScanTile | kScanTile + 1
    EXPECT(a.over == KEYS_FIT && a.nbins == kScanTile && a.sort_tiles == 1);
    EXPECT(b.over == KEYS_FIT && b.nbins == kScanTile + 1 && b.sort_tiles == 2);
    EXPECT(sort_layout(7, a.nbins, false).sort_tiles == 1 && sort_layout(7, b.nbins, false).sort_tiles == 2);
  }

  if (failures) {
    std::printf("%d of %d checks failed\n", failures, rows);
    return 1;
  }
  std::printf("ok: %d checks\n", rows);
  return 0;
}
