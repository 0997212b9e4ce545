// The fixed-point arithmetic of exact deposition (jaybenne_amd/csrc/jb_deposit_fixed.hpp) on the host
// (tests/test_deposit_host.py): every conversion against vectors written by the Python model
// (tests/deposit_model.py), one record per line of the file named on the command line, words in hexadecimal:
//   F <bits of w> <E> <status> <a0> <a1> <a2> <a3>     dep_from_double(w, E)
//   T <a0> <a1> <a2> <a3> <E> <bits of the result>    dep_to_double(a, E)
//   A <a0..a3> <b0..b3> <s0..s3>                      dep_add(a, b)
//   R <a0..a3> <s> <r0..r3> <dropped>                 dep_shift_right(a, s)
//   S <E> <n> <bits of w> x n <bits of the result>    the sum of n addends, converted, added and rounded once
// and a few literal rows of its own.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../jaybenne_amd/csrc/jb_deposit_fixed.hpp"

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

static double from_bits(uint64_t b) {
  double v;
  memcpy(&v, &b, sizeof v);
  return v;
}
static bool same(const Dep256 &a, const uint64_t (&w)[4]) {
  return a.w[0] == w[0] && a.w[1] == w[1] && a.w[2] == w[2] && a.w[3] == w[3];
}
static bool read_words(FILE *f, uint64_t *w, int n) {
  for (int q = 0; q < n; ++q)
    if (std::fscanf(f, "%" SCNx64, &w[q]) != 1) return false;
  return true;
}

int main(int argc, char **argv) {
  // literal rows: the layout itself
  {
    Dep256 a;
    EXPECT(dep_from_double(1.0, 1023, a) == DEP_ADDED);           // top bit at 222: word 3, bit 30
    EXPECT(a.w[3] == (1ull << 30) && a.w[2] == 0 && a.w[1] == 0 && a.w[0] == 0);
    EXPECT(dep_high_bit(a) == kDepTopBit);
    EXPECT(dep_to_double(a, 1023) == 1.0);
    EXPECT(dep_from_double(0.0, 1023, a) == DEP_REJECTED && dep_is_zero(a));
    EXPECT(dep_from_double(-1.0, 1023, a) == DEP_REJECTED && dep_is_zero(a));
    EXPECT(dep_from_double(from_bits(0x7ff0000000000000ull), 1023, a) == DEP_REJECTED);
    EXPECT(dep_from_double(from_bits(0x7ff8000000000000ull), 1023, a) == DEP_REJECTED);
    EXPECT(dep_exponent(1.0) == 1023 && dep_exponent(0.0) == 0 && dep_exponent(from_bits(1)) == 1);
    // an addend exactly at E - 170 is whole; one bit below it loses its last bit
    EXPECT(dep_from_double(from_bits(((uint64_t)(1023 - 170) << 52) | 1ull), 1023, a) == DEP_ADDED);
    EXPECT(a.w[0] == ((1ull << 52) | 1ull) && a.w[1] == 0);
    EXPECT(dep_from_double(from_bits(((uint64_t)(1023 - 171) << 52) | 1ull), 1023, a) == DEP_TRUNCATED);
    EXPECT(a.w[0] == (1ull << 51));
    EXPECT(dep_from_double(from_bits((uint64_t)(1023 - 171) << 52), 1023, a) == DEP_ADDED && a.w[0] == (1ull << 51));
    // 33 orders above the scale: the top bit; beyond: the top bit alone
    EXPECT(dep_from_double(from_bits((uint64_t)(1023 + 33) << 52), 1023, a) == DEP_ADDED && dep_top_bit(a));
    EXPECT(dep_from_double(from_bits((uint64_t)(1023 + 32) << 52), 1023, a) == DEP_ADDED && !dep_top_bit(a));
    EXPECT(dep_from_double(from_bits((uint64_t)(1023 + 600) << 52), 1023, a) == DEP_ADDED && a.w[3] == (1ull << 63) &&
           a.w[2] == 0);
    // a carry through three words
    Dep256 x = {{~0ull, ~0ull, ~0ull, 0}}, one = {{1, 0, 0, 0}};
    dep_add(x, one);
    EXPECT(x.w[0] == 0 && x.w[1] == 0 && x.w[2] == 0 && x.w[3] == 1);
  }
  if (argc < 2) {
    std::printf("usage: deposit_test <vectors>\n");
    return 2;
  }
  FILE *f = std::fopen(argv[1], "r");
  if (!f) {
    std::printf("cannot open %s\n", argv[1]);
    return 2;
  }
  char kind[8];
  int nF = 0, nT = 0, nA = 0, nS = 0, nR = 0;
  while (std::fscanf(f, "%7s", kind) == 1) {
    if (kind[0] == 'F') {
      uint64_t w, e, st, a[4];
      if (!read_words(f, &w, 1) || !read_words(f, &e, 1) || !read_words(f, &st, 1) || !read_words(f, a, 4)) break;
      Dep256 got;
      const int r = dep_from_double(from_bits(w), (int)e, got);
      ++rows;
      if (r != (int)st || !same(got, a)) {
        std::printf("FAILED F %016" PRIx64 " E=%d: status %d (want %d)\n", w, (int)e, r, (int)st);
        ++failures;
      }
      ++nF;
    } else if (kind[0] == 'T') {
      uint64_t a[4], e, want;
      if (!read_words(f, a, 4) || !read_words(f, &e, 1) || !read_words(f, &want, 1)) break;
      const Dep256 v = {{a[0], a[1], a[2], a[3]}};
      const double got = dep_to_double(v, (int)e);
      ++rows;
      if (dep_bits(got) != want) {
        std::printf("FAILED T E=%d: %016" PRIx64 " (want %016" PRIx64 ")\n", (int)e, dep_bits(got), want);
        ++failures;
      }
      ++nT;
    } else if (kind[0] == 'A') {
      uint64_t a[4], b[4], s[4];
      if (!read_words(f, a, 4) || !read_words(f, b, 4) || !read_words(f, s, 4)) break;
      Dep256 x = {{a[0], a[1], a[2], a[3]}};
      const Dep256 y = {{b[0], b[1], b[2], b[3]}};
      dep_add(x, y);
      EXPECT(same(x, s));
      ++nA;
    } else if (kind[0] == 'R') {
      uint64_t a[4], s, r[4], dropped;
      if (!read_words(f, a, 4) || !read_words(f, &s, 1) || !read_words(f, r, 4) || !read_words(f, &dropped, 1)) break;
      Dep256 x = {{a[0], a[1], a[2], a[3]}};
      const bool d = dep_shift_right(x, (int)s);
      EXPECT(same(x, r) && d == (dropped != 0));
      ++nR;
    } else if (kind[0] == 'S') {
      uint64_t e, n, want;
      if (!read_words(f, &e, 1) || !read_words(f, &n, 1)) break;
      std::vector<uint64_t> w((size_t)n);
      if (!read_words(f, w.data(), (int)n) || !read_words(f, &want, 1)) break;
      Dep256 fwd = {{0, 0, 0, 0}}, bwd = {{0, 0, 0, 0}}, v;
      for (size_t q = 0; q < w.size(); ++q) {
        if (dep_from_double(from_bits(w[q]), (int)e, v) != DEP_REJECTED) dep_add(fwd, v);
        if (dep_from_double(from_bits(w[w.size() - 1 - q]), (int)e, v) != DEP_REJECTED) dep_add(bwd, v);
      }
      EXPECT(dep_bits(dep_to_double(fwd, (int)e)) == want);
      EXPECT(fwd.w[0] == bwd.w[0] && fwd.w[1] == bwd.w[1] && fwd.w[2] == bwd.w[2] && fwd.w[3] == bwd.w[3]);
      ++nS;
    } else {
      std::printf("unknown record %s\n", kind);
      ++failures;
      break;
    }
  }
  std::fclose(f);
  EXPECT(nF > 0 && nT > 0 && nA > 0 && nS > 0 && nR > 0);
  if (failures) {
    std::printf("%d of %d rows failed\n", failures, rows);
    return 1;
  }
  std::printf("ok %d rows (%d F, %d T, %d A, %d S, %d R)\n", rows, nF, nT, nA, nS, nR);
  return 0;
}
