// The spectrum's arrays in the library's scratch memory (jaybenne_amd/csrc/jb_scratch_layout.hpp: spectrum_layout)
// without a GPU: behind the sort's arrays, in order, 8-byte aligned, without overlap, inside the words the layout
// asks for, and with the partials the kernels index -- 2 (ngroups + 2) doubles per 4096 slots.  Stand-alone: prints
// "ok" or the first failure.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../jaybenne_amd/csrc/jb_scratch_layout.hpp"

using namespace jb;

#define CHECK(c)                                                                                       \
  do {                                                                                                 \
    if (!(c)) {                                                                                        \
      std::printf("FAILED %s (n = %lld, nbins = %lld, by_id = %d, ngroups = %d)\n", #c, n, nbins, (int)by_id, ng); \
      return 1;                                                                                        \
    }                                                                                                  \
  } while (0)

int main() {
  const long long ns[] = {0, 1, 63, 4095, 4096, 4097, 8193, 100000, 12345679};
  const long long bins[] = {2, 13, 2049, 2054, 16777217};
  const int groups[] = {1, 2, 7, 16, 33, 64};
  for (long long n : ns)
    for (long long nbins : bins)
      for (bool by_id : {false, true})
        for (int ng : groups) {
          const SpecLayout s = spectrum_layout(n, nbins, by_id, ng);
          const SortLayout sort = sort_layout(n, nbins, by_id);
          const MomLayout m = mom_layout(n, nbins, by_id);
          const size_t chunks = (size_t)((n + kMomChunk - 1) / kMomChunk);
          CHECK(s.sort.words == sort.words && s.part.off == 8 * sort.words && s.part.off == m.part.off);
          CHECK(s.part.elem == 8 && s.part.count == 2 * (size_t)(ng + 2) * chunks);
          // the last partial a kernel can touch: head slot n - 1, its run's first chunk
          if (n > 0) CHECK((size_t)(ng + 2) * (2 * (size_t)((n - 1) / kMomChunk) + 1) + (size_t)(ng + 2) <= s.part.count);
          CHECK(s.stats.off == s.part.end() && s.stats.elem == 8 && s.stats.count == (size_t)SS_N);
          CHECK(s.flag.off == s.stats.end() && s.flag.elem == 4 && s.flag.count == 1);
          CHECK(s.part.off % 8 == 0 && s.stats.off % 8 == 0 && s.flag.off % 8 == 0);
          CHECK(s.flag.end() <= 8 * s.words && 8 * s.words <= s.flag.end() + 8);
        }
  static_assert((int)SS_COUNTED == 0 && (int)SS_ABOVE == 4 && (int)SS_N == 5, "the five counts of the report");
  std::printf("ok\n");
  return 0;
}
