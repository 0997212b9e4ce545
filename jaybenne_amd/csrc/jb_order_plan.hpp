// jb_order_plan.hpp -- the host side of the canonical sort (jb_kernel_order.hpp; include/jaybenne_amd.h:
// jb_set_cell_order): which radix passes a call runs and where its arrays lie in the library's scratch memory.
// Pure functions of a few scalars; tests/order_test.cpp walks the thresholds on the host.  Plain C++17: no HIP
// include.
#pragma once

#include <cstddef>

#include "jb_limits.hpp"

namespace jb {

constexpr int kOrderTile = 2048;      // slots per workgroup of a radix pass (256 threads x 8: jb_kernel_order.hpp)
constexpr int kOrderDigits = 256;     // 8-bit digits
constexpr int kOrderMaxPasses = 12;   // 8 of the id + 4 of the cell key

// The sort key is (32-bit cell key, 64-bit id), taken as three 32-bit words: a pass carries (word, slot index)
// pairs, and the pass that ends a word fetches the next one for the pairs it writes.
enum OrderWord { ORDER_ID_LO = 0, ORDER_ID_HI = 1, ORDER_KEY = 2 };
// what a pass writes: pairs with the same word, pairs with the next word, or (the last pass) dest[slot]
enum OrderNext { ORDER_NEXT_SAME = 0, ORDER_NEXT_ID_HI = 1, ORDER_NEXT_KEY = 2, ORDER_NEXT_DEST = 3 };

struct OrderPass {
  int word = ORDER_ID_LO;   // OrderWord the digit is taken from
  int shift = 0;            // ... at this bit
  int next = ORDER_NEXT_SAME;
};
struct OrderPlan {
  int id_passes = 0, key_passes = 0, npasses = 0;
  OrderPass pass[kOrderMaxPasses];
};

// 8-bit digits up to and including the highest set bit: 0 for 0, 8 for anything with bit 56 or above
inline int order_digits(unsigned long long v) {
  int d = 0;
  for (; v != 0ull; v >>= 8) ++d;
  return d;
}

// Least significant digit first: the id's digits, then the cell key's; digits above the highest set bit of the
// largest value are the same (zero) in every slot and are left out.  n <= 1: nothing to sort.
inline OrderPlan plan_order(long long n, unsigned long long max_id, unsigned max_key) {
  OrderPlan p;
  if (n <= 1) return p;
  p.id_passes = order_digits(max_id);
  p.key_passes = order_digits((unsigned long long)max_key);
  for (int q = 0; q < p.id_passes; ++q) {
    OrderPass &s = p.pass[p.npasses++];
    s.word = q < 4 ? ORDER_ID_LO : ORDER_ID_HI;
    s.shift = 8 * (q & 3);
  }
  for (int q = 0; q < p.key_passes; ++q) {
    OrderPass &s = p.pass[p.npasses++];
    s.word = ORDER_KEY;
    s.shift = 8 * q;
  }
  for (int q = 0; q < p.npasses; ++q) {
    if (q + 1 == p.npasses) p.pass[q].next = ORDER_NEXT_DEST;
    else if (p.pass[q + 1].word == p.pass[q].word) p.pass[q].next = ORDER_NEXT_SAME;
    else p.pass[q].next = p.pass[q + 1].word == ORDER_ID_HI ? ORDER_NEXT_ID_HI : ORDER_NEXT_KEY;
  }
  return p;
}

// The sort's arrays behind those of the counting sort, as offsets in 8-byte words from `start`:
//   pairs[2]  n words each      the double-buffered (word, slot index) pairs
//   dest      n x 4 bytes       the new slot of every slot (the inverted permutation)
//   cnt       256 x tiles x 4   digit counts per tile, digit-major; scanned in place
//   csum      scan tiles x 4    tile sums of that scan
//   flags     2 words           largest id | largest key, "not in canonical order" (the one read-back)
// 20 bytes per photon plus 1/8 byte of counts.
struct OrderLayout {
  long long tiles = 0;        // radix tiles over the n slots
  long long ncnt = 0;         // entries of cnt
  long long scan_tiles = 0;   // tiles of the scan over cnt
  size_t pairs[2] = {0, 0}, dest = 0, cnt = 0, csum = 0, flags = 0;
  size_t end = 0;             // first word behind the arrays
};
inline OrderLayout order_layout(long long n, size_t start) {
  OrderLayout L;
  if (n < 0) n = 0;
  L.tiles = (n + kOrderTile - 1) / kOrderTile;
  L.ncnt = (long long)kOrderDigits * L.tiles;
  L.scan_tiles = (L.ncnt + kScanTile - 1) / kScanTile;   // (the counts are scanned by k_scan_*)
  size_t o = start;
  L.pairs[0] = o; o += (size_t)n;
  L.pairs[1] = o; o += (size_t)n;
  L.dest = o; o += ((size_t)n + 1) / 2;
  L.cnt = o; o += ((size_t)L.ncnt + 1) / 2;
  L.csum = o; o += ((size_t)L.scan_tiles + 1) / 2;
  L.flags = o; o += 2;
  L.end = o;
  return L;
}

}  // namespace jb
