// jb_deposit_fixed.hpp -- the fixed-point arithmetic of exact deposition (include/jaybenne_amd.h:
// jb_set_deposition; kernels: jb_kernel_deposit.hpp).  A 256-bit unsigned accumulator per cell, four 64-bit
// words, least significant first; an addend w is placed at the cycle's scale exponent E so that a weight of
// exponent E has the top bit of its 53-bit significand at bit 222.  Integer adds are associative: the sum does not
// depend on the order of the adds, and the one rounding is the conversion back to double.
// Plain C++17, no HIP include: tests/deposit_test.cpp walks the edge cases on the host against the vectors of
// tests/deposit_model.py.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define JB_DEP_HD __host__ __device__ inline
#else
#define JB_DEP_HD inline
#endif

namespace jb {

constexpr int kDepWords = 4;
constexpr int kDepTopBit = 222;               // top significand bit of a weight of exponent E
constexpr int kDepShift0 = kDepTopBit - 52;   // 170: left shift of such a weight's significand
constexpr int kDepMaxShift = 255 - 52;        // above it the addend does not fit: it sets the top bit alone
constexpr int kDepBias = 1075 + kDepShift0;   // accumulator A at scale E stands for A * 2^(E - kDepBias)

enum { DEP_ADDED = 0, DEP_TRUNCATED = 1, DEP_REJECTED = 2 };

struct Dep256 {
  uint64_t w[kDepWords];
};

JB_DEP_HD uint64_t dep_bits(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof b);
  return b;
}

// The scale exponent of w: the biased exponent field of a finite w > 0 (1 for a subnormal, which has the scale of
// the smallest normal number); 0 for everything that adds nothing (w <= 0, infinities, NaN).
JB_DEP_HD int dep_exponent(double w) {
  const uint64_t b = dep_bits(w);
  const int e = (int)((b >> 52) & 0x7ffu);
  if ((b >> 63) != 0 || e == 0x7ff || (b << 1) == 0) return 0;
  return e == 0 ? 1 : e;
}

// w at scale E (1 <= E <= 2046) -> out.  DEP_REJECTED: w <= 0 or not finite, out = 0.  DEP_TRUNCATED: non-zero
// bits of w lay below bit 0 and were dropped (never rounded) -- a function of (w, E) alone.  An addend more than
// 33 binary orders above the scale does not fit: it becomes 2^255, the top bit the close turns down.
JB_DEP_HD int dep_from_double(double w, int E, Dep256 &out) {
  out.w[0] = out.w[1] = out.w[2] = out.w[3] = 0;
  int e = dep_exponent(w);
  if (e == 0) return DEP_REJECTED;
  const uint64_t b = dep_bits(w);
  uint64_t sig = b & ((1ull << 52) - 1);
  if (((b >> 52) & 0x7ffu) != 0) sig |= 1ull << 52;
  const int shift = kDepShift0 + (e - E);
  if (shift > kDepMaxShift) {
    out.w[3] = 1ull << 63;
    return DEP_ADDED;
  }
  if (shift < 0) {
    const int s = -shift;
    if (s >= 53) return DEP_TRUNCATED;   // (sig != 0: a finite w > 0)
    const bool dropped = (sig & ((1ull << s) - 1)) != 0;
    out.w[0] = sig >> s;
    return dropped ? DEP_TRUNCATED : DEP_ADDED;
  }
  // (the words are named one by one, here and below: an index computed at run time would put the four words of a
  // lane into scratch memory on the device)
  const int wi = shift >> 6, r = shift & 63;
  const uint64_t lo = sig << r, hi = r > 11 ? sig >> (64 - r) : 0;   // (hi: 53 + r > 64)
  out.w[0] = wi == 0 ? lo : 0;
  out.w[1] = wi == 1 ? lo : (wi == 0 ? hi : 0);
  out.w[2] = wi == 2 ? lo : (wi == 1 ? hi : 0);
  out.w[3] = wi == 3 ? lo : (wi == 2 ? hi : 0);
  return DEP_ADDED;
}

// a += b with carries rippling through the words (a carry out of the top word is lost)
JB_DEP_HD uint64_t dep_add_word(uint64_t &a, uint64_t b, uint64_t carry) {
  const uint64_t s = a + b;
  const uint64_t c1 = s < b ? 1u : 0u;
  const uint64_t t = s + carry;
  const uint64_t c2 = t < carry ? 1u : 0u;
  a = t;
  return c1 | c2;
}
JB_DEP_HD void dep_add(Dep256 &a, const Dep256 &b) {
  uint64_t carry = dep_add_word(a.w[0], b.w[0], 0);
  carry = dep_add_word(a.w[1], b.w[1], carry);
  carry = dep_add_word(a.w[2], b.w[2], carry);
  (void)dep_add_word(a.w[3], b.w[3], carry);
}

JB_DEP_HD bool dep_is_zero(const Dep256 &a) { return (a.w[0] | a.w[1] | a.w[2] | a.w[3]) == 0; }
JB_DEP_HD bool dep_top_bit(const Dep256 &a) { return (a.w[kDepWords - 1] >> 63) != 0; }

// position of the highest set bit (a != 0)
JB_DEP_HD int dep_high_bit(const Dep256 &a) {
  if (a.w[3] != 0) return 255 - __builtin_clzll(a.w[3]);
  if (a.w[2] != 0) return 191 - __builtin_clzll(a.w[2]);
  if (a.w[1] != 0) return 127 - __builtin_clzll(a.w[1]);
  if (a.w[0] != 0) return 63 - __builtin_clzll(a.w[0]);
  return -1;
}

// the 64 bits of a from bit k upwards (0 <= k < 256)
JB_DEP_HD uint64_t dep_bits_from(const Dep256 &a, int k) {
  const int wi = k >> 6, r = k & 63;
  const uint64_t lo = wi == 0 ? a.w[0] : (wi == 1 ? a.w[1] : (wi == 2 ? a.w[2] : a.w[3]));
  const uint64_t hi = wi == 0 ? a.w[1] : (wi == 1 ? a.w[2] : (wi == 2 ? a.w[3] : 0));
  return r != 0 ? (lo >> r) | (hi << (64 - r)) : lo;
}
// any bit of a below bit k set (0 <= k <= 256)
JB_DEP_HD bool dep_any_below(const Dep256 &a, int k) {
  const int wi = k >> 6, r = k & 63;
  const uint64_t part = wi == 0 ? a.w[0] : (wi == 1 ? a.w[1] : (wi == 2 ? a.w[2] : (wi == 3 ? a.w[3] : 0)));
  uint64_t any = r != 0 ? part & ((1ull << r) - 1) : 0;
  if (wi > 0) any |= a.w[0];
  if (wi > 1) any |= a.w[1];
  if (wi > 2) any |= a.w[2];
  if (wi > 3) any |= a.w[3];
  return any != 0;
}

// a at scale E -> a at scale E + s (s > 0): the bits below the new bit 0 are dropped; true when any of them was set
JB_DEP_HD bool dep_shift_right(Dep256 &a, int s) {
  const int k = s > 256 ? 256 : s;
  const bool dropped = dep_any_below(a, k);
  Dep256 r;
  r.w[0] = k < 256 ? dep_bits_from(a, k) : 0;
  r.w[1] = k + 64 < 256 ? dep_bits_from(a, k + 64) : 0;
  r.w[2] = k + 128 < 256 ? dep_bits_from(a, k + 128) : 0;
  r.w[3] = k + 192 < 256 ? dep_bits_from(a, k + 192) : 0;
  a = r;
  return dropped;
}

// The accumulator at scale E as a double: ONE round-to-nearest-even of the 256-bit integer to 53 bits, then
// ldexp -- a subnormal or overflowing result is what ldexp makes of that 53-bit value.
JB_DEP_HD double dep_to_double(const Dep256 &a, int E) {
  const int p = dep_high_bit(a);
  if (p < 0) return 0.0;
  if (p <= 52) return ldexp((double)a.w[0], E - kDepBias);
  const int drop = p - 52;                       // bits below the 53 kept
  uint64_t q = dep_bits_from(a, drop) & ((1ull << 53) - 1);
  const bool guard = ((dep_bits_from(a, drop - 1)) & 1u) != 0;
  const bool sticky = dep_any_below(a, drop - 1);   // bits [0, drop - 1) lie under the guard bit
  if (guard && (sticky || (q & 1u) != 0)) ++q;   // (2^53 is a double too)
  return ldexp((double)q, drop + E - kDepBias);
}

}  // namespace jb
