// The transport-invariant predicates of jaybenne_amd/csrc/jb_invariants.hpp, compiled for the host
// (tests/test_invariants_host.py): each kind fires on its violating input and on nothing else; the
// boundary equalities the reference's <= admits pass.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "../jaybenne_amd/csrc/jb_invariants.hpp"

using namespace jb::inv;

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

// one photon state and the block it claims to be in
struct State {
  int ndim = 3;
  double x[3] = {0.5, 0.5, 0.5};
  double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {1.0, 1.0, 1.0};
  int idx[3] = {4, 4, 4};
  int first[3] = {2, 2, 2}, last[3] = {9, 9, 9};
  long long blk = 3, nblocks = 8;
  int status = JB_ST_ACTIVE;
  double w = 1.0, e = 2.0, t = 0.5, t_end = 1.0;
  bool absorbed = false, scattered = false;
};

// which kinds fire on a state (the SWARM sweep's own conditions: block, status, attributes)
struct Fired {
  bool position, index, off_block, block, status, attributes;
};
static Fired fire(const State &s) {
  Fired f;
  f.position = !position_ok(s.ndim, s.x, s.lo, s.hi);
  f.index = !index_ok(s.idx, s.first, s.last);
  f.off_block = !event_off_block_ok(s.absorbed, s.scattered);
  f.block = !block_ok(s.blk, s.nblocks);
  f.status = !status_ok(s.status);
  f.attributes = !attributes_ok(s.w, s.e, s.t, s.t_end);
  return f;
}
static bool none(const Fired &f) {
  return !f.position && !f.index && !f.off_block && !f.block && !f.status && !f.attributes;
}
static bool only(const Fired &f, bool Fired::*which) {
  Fired g = f;
  if (!(g.*which)) return false;
  g.*which = false;
  return none(g);
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double inf = std::numeric_limits<double>::infinity();
  {
    State s;
    EXPECT(none(fire(s)));
  }
  // boundary equalities pass (x_min <= x <= x_max, ib.s <= ip <= ib.e, t <= t_end, w = e = 0)
  for (int d = 0; d < 3; ++d) {
    State s;
    s.x[d] = s.hi[d];
    s.idx[d] = s.last[d];
    EXPECT(none(fire(s)));
    s.x[d] = s.lo[d];
    s.idx[d] = s.first[d];
    EXPECT(none(fire(s)));
  }
  {
    State s;
    s.t = s.t_end; s.w = 0.0; s.e = 0.0; s.blk = 0;
    EXPECT(none(fire(s)));
    s.blk = s.nblocks - 1;
    EXPECT(none(fire(s)));
  }
  // POSITION: each axis, each side, NaN; the first failing axis is named
  for (int d = 0; d < 3; ++d) {
    State s;
    s.x[d] = std::nextafter(s.hi[d], 2.0);
    EXPECT(only(fire(s), &Fired::position));
    EXPECT(first_axis_out(s.ndim, s.x, s.lo, s.hi) == d);
    s.x[d] = std::nextafter(s.lo[d], -1.0);
    EXPECT(only(fire(s), &Fired::position));
    s.x[d] = nan;
    EXPECT(only(fire(s), &Fired::position));
  }
  {  // an inactive axis is not checked
    State s;
    s.ndim = 1;
    s.x[1] = 5.0; s.x[2] = -5.0;
    EXPECT(none(fire(s)));
    s.x[0] = 1.5;
    EXPECT(only(fire(s), &Fired::position));
  }
  // INDEX: one past either end on each axis (a ghost cell inside the allocation)
  for (int d = 0; d < 3; ++d) {
    State s;
    s.idx[d] = s.last[d] + 1;
    EXPECT(only(fire(s), &Fired::index));
    s.idx[d] = s.first[d] - 1;
    EXPECT(only(fire(s), &Fired::index));
  }
  // EVENT_OFF_BLOCK
  {
    State s;
    s.absorbed = true;
    EXPECT(only(fire(s), &Fired::off_block));
    s.absorbed = false; s.scattered = true;
    EXPECT(only(fire(s), &Fired::off_block));
  }
  // block range
  {
    State s;
    s.blk = s.nblocks;
    EXPECT(only(fire(s), &Fired::block));
    s.blk = -1;
    EXPECT(only(fire(s), &Fired::block));
  }
  // status: JB_ST_ACTIVE .. JB_ST_OUTGOING_ABSORBED are defined
  for (int st = JB_ST_ACTIVE; st <= JB_ST_OUTGOING_ABSORBED; ++st) {
    State s;
    s.status = st;
    EXPECT(none(fire(s)));
  }
  for (int st : {-1, JB_ST_OUTGOING_ABSORBED + 1, 77}) {
    State s;
    s.status = st;
    EXPECT(only(fire(s), &Fired::status));
  }
  // attributes: w, e finite and >= 0, t <= t_end
  for (double bad : {nan, inf, -1e-300}) {
    State s;
    s.w = bad;
    EXPECT(only(fire(s), &Fired::attributes));
    State r;
    r.e = bad;
    EXPECT(only(fire(r), &Fired::attributes));
  }
  {
    State s;
    s.t = std::nextafter(s.t_end, 2.0);
    EXPECT(only(fire(s), &Fired::attributes));
    s.t = nan;
    EXPECT(only(fire(s), &Fired::attributes));
  }
  // DDMC_CLASS: bit equality (not ==: -0.0 and 0.0 differ, a NaN equals itself)
  {
    uint64_t a[8], b[8];
    for (int q = 0; q < 8; ++q) a[q] = b[q] = 0x3ff0000000000000ull + (uint64_t)q;
    EXPECT(records_equal(a, b));
    for (int q = 0; q < 8; ++q) {
      b[q] ^= 1ull;
      EXPECT(!records_equal(a, b));
      b[q] ^= 1ull;
    }
    a[3] = 0x0000000000000000ull; b[3] = 0x8000000000000000ull;
    EXPECT(!records_equal(a, b));
    a[3] = b[3] = 0x7ff8000000000000ull;
    EXPECT(records_equal(a, b));
  }
  std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
