// The host side of the canonical sort (jaybenne_amd/csrc/jb_order_plan.hpp) on the host (tests/test_cell_order_host.py):
// the pass counts from both sides of every threshold -- the expected counts are literals --, the scratch layout, and
// the plan's passes carried out on the host (a stable counting sort per pass over (word, slot) pairs, the word
// fetched anew where the plan says so) against std::stable_sort of (key, id).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../jaybenne_amd/csrc/jb_order_plan.hpp"

using namespace jb;

static int failures = 0, rows = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    ++rows;                                                             \
    if (!(cond)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static void passes(int line, long long n, unsigned long long max_id, unsigned max_key, int want_id, int want_key) {
  const OrderPlan p = plan_order(n, max_id, max_key);
  ++rows;
  bool ok = p.id_passes == want_id && p.key_passes == want_key && p.npasses == want_id + want_key &&
            p.npasses <= kOrderMaxPasses;
  // the passes themselves: id digits from bit 0 up, then key digits from bit 0 up; the last one writes dest
  for (int q = 0; ok && q < p.npasses; ++q) {
    const OrderPass &s = p.pass[q];
    if (q < want_id) ok = s.word == (q < 4 ? ORDER_ID_LO : ORDER_ID_HI) && s.shift == 8 * (q % 4);
    else ok = s.word == ORDER_KEY && s.shift == 8 * (q - want_id);
    if (!ok) break;
    if (q + 1 == p.npasses) ok = s.next == ORDER_NEXT_DEST;
    else if (q + 1 == want_id) ok = s.next == ORDER_NEXT_KEY;
    else if (q == 3 && want_id > 4) ok = s.next == ORDER_NEXT_ID_HI;
    else ok = s.next == ORDER_NEXT_SAME;
  }
  if (!ok) {
    std::printf("FAILED line %d: n %lld max id %llu max key %u -> %d + %d passes (want %d + %d)\n", line, n, max_id,
                max_key, p.id_passes, p.key_passes, want_id, want_key);
    ++failures;
  }
}
#define PASSES(...) passes(__LINE__, __VA_ARGS__)

// the plan's passes on the host
static std::vector<unsigned> run_plan(const std::vector<unsigned> &key, const std::vector<uint64_t> &id) {
  const size_t n = key.size();
  uint64_t max_id = 0;
  unsigned max_key = 0;
  for (size_t i = 0; i < n; ++i) {
    max_id = std::max(max_id, id[i]);
    max_key = std::max(max_key, key[i]);
  }
  const OrderPlan p = plan_order((long long)n, max_id, max_key);
  auto word = [&](int which, unsigned s) {
    return which == ORDER_KEY ? key[s] : which == ORDER_ID_HI ? (unsigned)(id[s] >> 32) : (unsigned)id[s];
  };
  std::vector<unsigned> dest(n);
  for (size_t i = 0; i < n; ++i) dest[i] = (unsigned)i;
  if (p.npasses == 0) return dest;
  std::vector<std::pair<unsigned, unsigned>> a(n), b(n);
  for (size_t i = 0; i < n; ++i) a[i] = {word(p.pass[0].word, (unsigned)i), (unsigned)i};
  for (int q = 0; q < p.npasses; ++q) {
    const OrderPass &s = p.pass[q];
    size_t start[257] = {0};
    for (size_t i = 0; i < n; ++i) ++start[((a[i].first >> s.shift) & 255u) + 1];
    for (int d = 0; d < 256; ++d) start[d + 1] += start[d];
    for (size_t i = 0; i < n; ++i) {
      const size_t pos = start[(a[i].first >> s.shift) & 255u]++;
      const unsigned slot = a[i].second;
      if (s.next == ORDER_NEXT_DEST) dest[slot] = (unsigned)pos;
      else if (s.next == ORDER_NEXT_SAME) b[pos] = a[i];
      else b[pos] = {word(s.next == ORDER_NEXT_KEY ? ORDER_KEY : ORDER_ID_HI, slot), slot};
    }
    a.swap(b);
  }
  return dest;
}

static uint64_t hash64(uint64_t x) {
  x = (x + 0x9E3779B97F4A7C15ull) * 0xBF58476D1CE4E5B9ull;
  x ^= x >> 29;
  x *= 0x94D049BB133111EBull;
  return x ^ (x >> 32);
}

static void sorted_as_stable_sort(int line, const std::vector<unsigned> &key, const std::vector<uint64_t> &id) {
  const size_t n = key.size();
  std::vector<unsigned> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = (unsigned)i;
  std::stable_sort(order.begin(), order.end(), [&](unsigned x, unsigned y) {
    return key[x] != key[y] ? key[x] < key[y] : id[x] < id[y];
  });
  const std::vector<unsigned> dest = run_plan(key, id);
  ++rows;
  for (size_t r = 0; r < n; ++r)
    if (dest[order[r]] != r) {
      std::printf("FAILED line %d: slot %u goes to %u, not %zu\n", line, order[r], dest[order[r]], r);
      ++failures;
      return;
    }
}

int main() {
  const unsigned long long one = 1ull;
  // ---- the id: 0, 255 | 256, 2^16 - 1 | 2^16, 2^32 - 1 | 2^32, 2^63, 2^64 - 1
  PASSES(1000, 0ull, 0u, 0, 0);
  PASSES(1000, 255ull, 0u, 1, 0);
  PASSES(1000, 256ull, 0u, 2, 0);
  PASSES(1000, (one << 16) - 1, 0u, 2, 0);
  PASSES(1000, one << 16, 0u, 3, 0);
  PASSES(1000, (one << 24) - 1, 0u, 3, 0);
  PASSES(1000, one << 24, 0u, 4, 0);
  PASSES(1000, (one << 32) - 1, 0u, 4, 0);
  PASSES(1000, one << 32, 0u, 5, 0);
  PASSES(1000, (one << 40) - 1, 0u, 5, 0);
  PASSES(1000, one << 40, 0u, 6, 0);
  PASSES(1000, one << 63, 0u, 8, 0);
  PASSES(1000, ~0ull, 0u, 8, 0);
  // ---- the key: 0, 255 | 256, 2^24 - 1 | 2^24, 2^32 - 2
  PASSES(1000, 7ull, 255u, 1, 1);
  PASSES(1000, 7ull, 256u, 1, 2);
  PASSES(1000, 7ull, 65535u, 1, 2);
  PASSES(1000, 7ull, 65536u, 1, 3);
  PASSES(1000, 7ull, (1u << 24) - 1u, 1, 3);
  PASSES(1000, 7ull, 1u << 24, 1, 4);
  PASSES(1000, 7ull, 0xFFFFFFFEu, 1, 4);
  PASSES(1000, 0ull, 0xFFFFFFFEu, 0, 4);
  // ---- both at their largest, and the case of the design note: 1e8 photons in 128^3 cells
  PASSES(1000, ~0ull, 0xFFFFFFFEu, 8, 4);
  PASSES(100000000, 99999999ull, 128u * 128u * 128u, 4, 3);
  // ---- n = 1 (and 0): nothing to sort, whatever the slot holds
  PASSES(1, ~0ull, 0xFFFFFFFEu, 0, 0);
  PASSES(1, 0ull, 0u, 0, 0);
  PASSES(0, 5ull, 5u, 0, 0);
  PASSES(2, 5ull, 5u, 1, 1);
  EXPECT(order_digits(0ull) == 0 && order_digits(1ull) == 1 && order_digits(one << 56) == 8);

  // ---- the layout: arrays in order, none overlapping, sized for their contents
  for (long long n : {0ll, 1ll, 2ll, 2047ll, 2048ll, 2049ll, 4096ll, 4097ll, 100000000ll, (1ll << 32) - 1}) {
    const size_t start = 12345;
    const OrderLayout L = order_layout(n, start);
    EXPECT(L.tiles == (n + 2047) / 2048 && L.ncnt == 256 * L.tiles && L.scan_tiles == (L.ncnt + 2047) / 2048);
    EXPECT(L.pairs[0] == start && L.pairs[1] - L.pairs[0] >= (size_t)n && L.dest - L.pairs[1] >= (size_t)n);
    EXPECT(8 * (L.cnt - L.dest) >= 4 * (size_t)n && 8 * (L.csum - L.cnt) >= 4 * (size_t)L.ncnt);
    EXPECT(8 * (L.flags - L.csum) >= 4 * (size_t)L.scan_tiles && L.end - L.flags == 2);
    EXPECT(8 * (L.end - start) <= 21 * (size_t)n + 8 * 200);   // 20 1/8 bytes per photon and a few words
  }

  // ---- the passes carried out: ids that differ only above bit 32, only in one digit, holes with bit 63, ties
  {
    std::vector<unsigned> key;
    std::vector<uint64_t> id;
    for (unsigned i = 0; i < 5000; ++i) {
      const uint64_t h = hash64(i);
      key.push_back((unsigned)(h % 7u) * (i % 3u == 0 ? 70000u : 1u));
      const unsigned kind = i % 5u;
      id.push_back(kind == 0 ? h % 256u : kind == 1 ? (h % 1000u) << 32 | 5u : kind == 2 ? (h >> 2) : kind == 3 ? (h % 64u) << 8
                                                                                                              : h | (one << 63));
    }
    for (unsigned i = 0; i < 40; ++i) {   // equal (key, id): the input slot decides
      key.push_back(3u);
      id.push_back(77ull);
    }
    sorted_as_stable_sort(__LINE__, key, id);
    std::vector<unsigned> k2(key.begin(), key.begin() + 1);
    std::vector<uint64_t> i2(id.begin(), id.begin() + 1);
    sorted_as_stable_sort(__LINE__, k2, i2);
    std::vector<unsigned> k3(300, 0u);
    std::vector<uint64_t> i3(300);
    for (unsigned i = 0; i < 300; ++i) i3[i] = (uint64_t)(299 - i) * 256u;   // one digit value in the first pass
    sorted_as_stable_sort(__LINE__, k3, i3);
    for (unsigned i = 0; i < 300; ++i) i3[i] = ((uint64_t)hash64(i) % 50u) << 33;   // only above bit 32, with ties
    sorted_as_stable_sort(__LINE__, k3, i3);
  }

  if (failures) {
    std::printf("%d of %d checks failed\n", failures, rows);
    return 1;
  }
  std::printf("ok: %d checks\n", rows);
  return 0;
}
