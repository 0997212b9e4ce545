// The scratch layout of the global comb (jaybenne_amd/csrc/jb_scratch_layout.hpp: gcomb_layout) on the host
// (tests/test_gcomb_layout_host.py).  Everything comb_layout(n) has lies where comb_layout(n) puts it; the cells'
// targets and the output records come behind it, at offsets restated here with literal numbers; nothing overlaps and
// everything lies inside the size asked for; with n_room <= n there is no output span and the move goes to the
// sort's records.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../jaybenne_amd/csrc/jb_scratch_layout.hpp"

using namespace jb;

static int failures = 0, rows = 0;
static long long case_n = 0, case_room = 0, case_nbins = 0;
static int case_by_id = 0;
#define EXPECT(cond)                                                                                              \
  do {                                                                                                            \
    ++rows;                                                                                                       \
    if (!(cond)) {                                                                                                \
      std::printf("FAILED line %d (n %lld n_room %lld nbins %lld by_id %d): %s\n", __LINE__, case_n, case_room,   \
                  case_nbins, case_by_id, #cond);                                                                 \
      ++failures;                                                                                                 \
    }                                                                                                             \
  } while (0)

static bool same(const Span &a, const Span &b) { return a.off == b.off && a.count == b.count && a.elem == b.elem; }

static void check(long long n, long long n_room, long long nbins, bool by_id) {
  case_n = n; case_room = n_room; case_nbins = nbins; case_by_id = by_id;
  const GcombLayout g = gcomb_layout(n, n_room, nbins, by_id);
  const CombLayout c = comb_layout(n, nbins, by_id);
  // the comb's arrays, where the comb has them
  EXPECT(g.comb.words == c.words && g.comb.ntiles == c.ntiles && g.comb.sort.words == c.sort.words);
  EXPECT(same(g.comb.sort.rec, c.sort.rec) && same(g.comb.sort.hist, c.sort.hist) && same(g.comb.sort.sums, c.sort.sums) &&
         same(g.comb.sort.key, c.sort.key));
  EXPECT(same(g.comb.C, c.C) && same(g.comb.kcnt, c.kcnt) && same(g.comb.extra, c.extra) && same(g.comb.ssum, c.ssum) &&
         same(g.comb.tsum, c.tsum) && same(g.comb.tflag, c.tflag) && same(g.comb.cpart, c.cpart) &&
         same(g.comb.epart, c.epart) && same(g.comb.C128, c.C128) && same(g.comb.tsum128, c.tsum128));
  EXPECT(n == 0 || g.comb.fits_records());   // (an empty swarm is never scanned)
  // the targets: n + 1 words right behind the comb
  EXPECT(g.ktgt.off == 8 * c.words && g.ktgt.count == (size_t)n + 1 && g.ktgt.elem == 4);
  // the output records: behind the targets, on a 16-byte boundary, n_room of 128 bytes -- or none
  const size_t behind = (8 * c.words + ((size_t)(n + 1) * 4 + 7) / 8 * 8 + 15) / 16 * 16;
  EXPECT(g.out.off == behind && g.out.elem == 128 && g.out.off % 16 == 0);
  if (n_room > n) {
    EXPECT(g.out.count == (size_t)n_room);
    EXPECT(same(g.records(), g.out));
    EXPECT(g.words == (behind + 128 * (size_t)n_room) / 8);
  } else {   // the comb's own layout and the targets: the move fits the sort's records
    EXPECT(g.out.count == 0);
    EXPECT(same(g.records(), c.sort.rec));
    EXPECT(g.words == behind / 8);
    EXPECT((size_t)n_room * 128 <= c.sort.rec.end() - c.sort.rec.off);
  }
  EXPECT(g.records().count >= (size_t)n_room);
  // the report's partials fit the comb's cpart
  EXPECT((size_t)kGcombStats * (size_t)kGcombParts <= c.cpart.count && kGcombStats == 6 && kGcombParts == 341);
  // nothing overlaps, everything inside
  std::vector<Span> all = {c.sort.rec, c.sort.hist, c.sort.sums, c.sort.key, c.C, c.kcnt, c.extra, c.ssum,
                           c.tsum, c.tflag, c.cpart, c.epart, g.ktgt, g.out};
  std::sort(all.begin(), all.end(), [](const Span &a, const Span &b) { return a.off < b.off || (a.off == b.off && a.end() < b.end()); });
  for (size_t q = 0; q + 1 < all.size(); ++q) EXPECT(all[q].end() <= all[q + 1].off);
  for (const Span &s : all) EXPECT(s.end() <= 8 * g.words);
  EXPECT(g.ktgt.off % 8 == 0);
}

int main() {
  const long long ns[] = {0, 1, 2, 7, 2047, 2048, 2049, 99999, 100000, 12345677};
  const long long bins[] = {1, 2, 19, 2048, 2049, 1000001};
  for (long long n : ns)
    for (long long nbins : bins)
      for (int by_id = 0; by_id < 2; ++by_id)
        for (long long room : {0ll, n / 2, n - 1, n, n + 1, 2 * n + 3, 64 * n})
          if (room >= 0) check(n, room, nbins, by_id != 0);
  if (failures) {
    std::printf("%d of %d checks failed\n", failures, rows);
    return 1;
  }
  std::printf("ok: %d checks\n", rows);
  return 0;
}
