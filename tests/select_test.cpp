// The transport kernel selection of jaybenne_amd/csrc/jb_select.hpp on the host (tests/test_select_host.py):
// every threshold from both sides.  The expected plans and names are literals, written out by hand from the
// rules -- not computed by a second copy of them.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../jaybenne_amd/csrc/jb_select.hpp"

using namespace jb;

static int failures = 0, rows = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

// the name as the library reports it: through a buffer of exactly the size given (the sanitized build of this
// program sees a write past it)
static std::vector<char> name_of(const TransportPlan &p, size_t n = 64) {
  std::vector<char> buf(n, '#');
  variant_name(p, buf.data(), n);
  return buf;
}

static void check(int line, const TransportInputs &in, const TransportPlan &want, const char *name) {
  const TransportPlan got = select_transport(in);
  const std::vector<char> got_name = name_of(got);
  const bool same = got.family == want.family && got.ndim == want.ndim && got.ddmc == want.ddmc &&
                    got.tally == want.tally && got.gray == want.gray && got.exact == want.exact &&
                    got.lean == want.lean && got.noabs == want.noabs && got.uniform == want.uniform &&
                    got.gather == want.gather && got.lcodes == want.lcodes && got.mode == want.mode &&
                    got.dyn_lds == want.dyn_lds && got.occ_cap3 == want.occ_cap3;
  ++rows;
  if (same && std::strcmp(got_name.data(), name) == 0) return;
  ++failures;
  std::printf("FAILED row at line %d: got \"%s\" (family %d gray %d exact %d lean %d noabs %d uniform %d gather %d "
              "lcodes %d mode %d lds %zu cap %d), expected \"%s\"\n",
              line, got_name.data(), (int)got.family, got.gray, got.exact, got.lean, got.noabs, got.uniform,
              got.gather, got.lcodes, got.mode, got.dyn_lds, got.occ_cap3, name);
}
#define ROW(in, want, name) check(__LINE__, in, want, name)

// a gray mesh whose every cell takes DDMC steps, entered through jb_transport_photons_ddmc; the context's
// defaults (coop_gather -1, queues on, codes in LDS on, max_classes 256)
static TransportInputs all_ddmc(int ndim, bool tally, int nblocks, long long ntot, int nclass) {
  TransportInputs in;
  in.ndim = ndim;
  in.ddmc = true;
  in.tally = tally;
  in.gray = in.has_ddmc_cell = in.has_ddmc_code = true;
  in.nblocks = nblocks;
  in.ntot = ntot;
  in.last = 100000;
  in.nclass = nclass;
  return in;
}
static TransportPlan plan(Family f, int ndim, bool ddmc, bool tally) {
  TransportPlan p;
  p.family = f;
  p.ndim = ndim;
  p.ddmc = ddmc;
  p.tally = tally;
  return p;
}
static TransportPlan ddmc_plan(Family f, int ndim, bool tally, int gather, bool lcodes, size_t lds, bool cap = false) {
  TransportPlan p = plan(f, ndim, true, tally);
  p.gather = gather;
  p.lcodes = lcodes;
  p.dyn_lds = lds;
  p.occ_cap3 = cap;
  return p;
}

static void test_queues_and_codes_in_lds() {
  ROW(all_ddmc(1, true, 1, 128, 1), ddmc_plan(Family::k_ddmc_q, 1, true, 4, true, 8 * 128 + 64 * 1 + 4 * 128),
      "k_ddmc_all<1, true, cell codes, queues, codes in LDS>");
  // (an odd number of cells: tally and codes rounded up to a whole number of 16-byte pieces)
  ROW(all_ddmc(1, true, 1, 127, 2), ddmc_plan(Family::k_ddmc_q, 1, true, 4, true, 8 * 128 + 64 * 2 + 4 * 128),
      "k_ddmc_all<1, true, cell codes, queues, codes in LDS>");
  // kLdsCodeCells = 1024 cells; kLdsTally = 1024 cells
  ROW(all_ddmc(2, false, 1, 1024, 64), ddmc_plan(Family::k_ddmc_q, 2, false, 4, true, 64 * 64 + 4 * 1024),
      "k_ddmc_all<2, false, cell codes, queues, codes in LDS>");
  ROW(all_ddmc(2, true, 4, 256, 64), ddmc_plan(Family::k_ddmc_q, 2, true, 4, true, 8 * 1024 + 64 * 64 + 4 * 1024),
      "k_ddmc_all<2, true, cell codes, queues, codes in LDS>");
  ROW(all_ddmc(2, true, 1, 1025, 64), ddmc_plan(Family::k_ddmc_q, 2, true, 4, false, 64 * 64),
      "k_ddmc_all<2, true, cell codes, queues>");
  // 64 classes
  ROW(all_ddmc(3, true, 1, 1024, 65), ddmc_plan(Family::k_ddmc_q, 3, true, 4, false, 8 * 1024 + 64 * 65),
      "k_ddmc_all<3, true, cell codes, queues>");
  // JB_DDMC_LDS_CODES=0
  TransportInputs in = all_ddmc(1, false, 1, 128, 1);
  in.ddmc_lds_codes = false;
  ROW(in, ddmc_plan(Family::k_ddmc_q, 1, false, 4, false, 64), "k_ddmc_all<1, false, cell codes, queues>");
}

static void test_queues_off() {
  // kLdsRecCells = 256 cells
  TransportInputs in = all_ddmc(1, true, 1, 256, 1);
  in.ddmc_queues = false;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 1, true, 2, false, 8 * 256 + 64 * 256), "k_ddmc_all<1, true, records in LDS>");
  in.ntot = 257;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 1, true, 4, false, 8 * 258 + 64 * 1), "k_ddmc_all<1, true, cell codes>");
  in.tally = false;
  in.ndim = 2;
  in.nblocks = 2;
  in.ntot = 128;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 2, false, 2, false, 64 * 256), "k_ddmc_all<2, false, records in LDS>");
  // no cell codes on this mesh: the records, in LDS or gathered
  in.has_ddmc_code = false;
  in.ntot = 129;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 2, false, 0, false, 0), "k_ddmc_all<2, false>");
}

static void test_more_classes_than_max() {
  // 16384 cells: 1 MiB of records
  ROW(all_ddmc(3, false, 1, 16383, 257), ddmc_plan(Family::k_ddmc_all, 3, false, 0, false, 0), "k_ddmc_all<3, false>");
  ROW(all_ddmc(3, false, 1, 16384, 257), ddmc_plan(Family::k_ddmc_all, 3, false, 1, false, 0),
      "k_ddmc_all<3, false, quad gather>");
  ROW(all_ddmc(3, false, 1, 16384, 256), ddmc_plan(Family::k_ddmc_q, 3, false, 4, false, 64 * 256),
      "k_ddmc_all<3, false, cell codes, queues>");
  // JB_DDMC_MAX_CLASSES=4; no class counted yet
  TransportInputs in = all_ddmc(2, true, 8, 2048, 4);
  in.max_classes = 4;
  ROW(in, ddmc_plan(Family::k_ddmc_q, 2, true, 4, false, 64 * 4), "k_ddmc_all<2, true, cell codes, queues>");
  in.nclass = 5;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 2, true, 1, false, 0), "k_ddmc_all<2, true, quad gather>");
  in.nclass = 0;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 2, true, 1, false, 0), "k_ddmc_all<2, true, quad gather>");
}

static void test_coop_gather_forced() {
  TransportInputs in = all_ddmc(2, true, 1, 16384, 1);
  in.coop_gather = 0;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 2, true, 0, false, 0, true), "k_ddmc_all<2, true>");
  in.ntot = 16383;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 2, true, 0, false, 0, false), "k_ddmc_all<2, true>");
  in = all_ddmc(1, true, 1, 128, 1);
  in.coop_gather = 0;   // (not the records in LDS either)
  ROW(in, ddmc_plan(Family::k_ddmc_all, 1, true, 0, false, 8 * 128), "k_ddmc_all<1, true>");
  in.coop_gather = 1;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 1, true, 1, false, 8 * 128), "k_ddmc_all<1, true, quad gather>");
  in.coop_gather = 2;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 1, true, 3, false, 8 * 128), "k_ddmc_all<1, true, quad gather>");
  in.coop_gather = 4;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 1, true, 4, false, 8 * 128 + 64), "k_ddmc_all<1, true, cell codes>");
}

static void test_large_tables() {
  // 2^26 cells: 4 GiB of records
  ROW(all_ddmc(3, true, 1, (1ll << 26) - 1, 257), ddmc_plan(Family::k_ddmc_all, 3, true, 1, false, 0),
      "k_ddmc_all<3, true, quad gather>");
  ROW(all_ddmc(3, true, 1, 1ll << 26, 257), ddmc_plan(Family::k_ddmc_all, 3, true, 3, false, 0),
      "k_ddmc_all<3, true, quad gather>");
  // 2^32 cells: record numbers no longer fit 32 bits
  ROW(all_ddmc(3, true, 1, (1ll << 32) - 1, 257), ddmc_plan(Family::k_ddmc_all, 3, true, 3, false, 0),
      "k_ddmc_all<3, true, quad gather>");
  ROW(all_ddmc(3, true, 64, 1ll << 26, 257), ddmc_plan(Family::k_ddmc_all, 3, true, 0, false, 0, true),
      "k_ddmc_all<3, true>");
  // kQBlocks = 64 resident blocks
  ROW(all_ddmc(2, false, 64, 100, 1), ddmc_plan(Family::k_ddmc_q, 2, false, 4, false, 64),
      "k_ddmc_all<2, false, cell codes, queues>");
  ROW(all_ddmc(2, false, 65, 100, 1), ddmc_plan(Family::k_ddmc_all, 2, false, 4, false, 64),
      "k_ddmc_all<2, false, cell codes>");
  // 2^32 slots
  TransportInputs in = all_ddmc(3, true, 8, 4096, 3);
  in.last = 1ll << 32;
  ROW(in, ddmc_plan(Family::k_ddmc_q, 3, true, 4, false, 64 * 3), "k_ddmc_all<3, true, cell codes, queues>");
  in.last = (1ll << 32) + 1;
  ROW(in, ddmc_plan(Family::k_ddmc_all, 3, true, 4, false, 64 * 3), "k_ddmc_all<3, true, cell codes>");
  // kLdsBlocks resident blocks: beyond them the general kernel, GRAY 1 or 2
  in = all_ddmc(2, true, kLdsBlocks, 10, 3);
  ROW(in, ddmc_plan(Family::k_ddmc_all, 2, true, 4, false, 64 * 3), "k_ddmc_all<2, true, cell codes>");
  in.nblocks = kLdsBlocks + 1;
  TransportPlan general = plan(Family::k_transport, 2, true, true);
  general.gray = 1;
  ROW(in, general, "k_transport<2, true, 1, false, false>");
  in.noabs = true;
  in.exact_geom = in.cell_ok = true;   // (EXACT and LEAN are not for the DDMC entry)
  general.gray = 2;
  ROW(in, general, "k_transport<2, true, 2, false, false>");
}

static void test_mixed_mesh() {
  TransportInputs in = all_ddmc(1, true, 4, 64, 2);
  in.not_all_ddmc = true;
  in.exact_geom = in.cell_ok = true;
  TransportPlan want = plan(Family::k_hybrid, 1, true, true);
  in.lean_arith = false;
  ROW(in, want, "k_hybrid<1, exact>");
  in.lean_arith = true;
  in.ndim = want.ndim = 2;
  want.mode = 3;
  ROW(in, want, "k_hybrid<2, lean, cell-local>");
  in.ndim = want.ndim = 3;
  in.tally = want.tally = false;
  in.no_imc_cell = true;
  want.mode = 2;
  ROW(in, want, "k_hybrid<3, lean, exact geometry>");
  in.no_imc_cell = false;
  in.cell_ok = false;
  in.noabs = want.noabs = true;
  ROW(in, want, "k_hybrid<3, lean, exact geometry>");
  in.cell_ok = true;
  in.exact_geom = false;
  want.mode = 1;
  ROW(in, want, "k_hybrid<3, lean>");
  // the launches of a plan: PHASE 2 is <.., true, 0, 2> whatever the plan says; the others follow it
  for (const bool noabs : {false, true})
    for (int mode = 0; mode < 4; ++mode) {
      want.noabs = noabs;
      want.mode = mode;
      EXPECT(hybrid_phase(want, 2).noabs && hybrid_phase(want, 2).mode == 0);
      for (const int phase : {0, 1}) EXPECT(hybrid_phase(want, phase).noabs == noabs && hybrid_phase(want, phase).mode == mode);
    }
  // ... and the launch behind k_ddmc_all / k_ddmc_q is <.., NOABS, 0, 0>
  TransportInputs all = all_ddmc(3, true, 1, 4096, 1);
  all.lean_arith = all.exact_geom = all.cell_ok = true;
  all.noabs = true;
  EXPECT(hybrid_phase(select_transport(all), 0).noabs && hybrid_phase(select_transport(all), 0).mode == 0);
  all.noabs = false;
  EXPECT(!hybrid_phase(select_transport(all), 0).noabs && hybrid_phase(select_transport(all), 0).mode == 0);
  // not a gray mesh, or one without the packed cell records: the general kernel
  in = all_ddmc(1, false, 4, 64, 2);
  in.not_all_ddmc = true;
  in.has_ddmc_cell = false;
  want = plan(Family::k_transport, 1, true, false);
  want.gray = 1;
  ROW(in, want, "k_transport<1, false, 1, false, false>");
  in.has_ddmc_cell = true;
  in.gray = false;
  in.noabs = true;
  want.gray = 0;
  ROW(in, want, "k_transport<1, false, 0, false, false>");
}

static void test_imc_entry() {
  TransportInputs in;
  in.ndim = 3;
  in.tally = true;
  in.gray = true;
  in.nblocks = 8;
  in.ntot = 4096;
  in.last = 100000;
  in.cell_ok = in.uniform_geom = true;
  // k_imc_cell: gray, lean, cell_ok, not switched off -- whatever the geometry
  TransportPlan cell = plan(Family::k_imc_cell, 3, false, true);
  cell.uniform = true;
  ROW(in, cell, "k_imc_cell<3, true, false, lean>");
  in.has_ddmc_cell = in.has_ddmc_code = in.not_all_ddmc = true;   // (the DDMC tables are nothing to this entry)
  ROW(in, cell, "k_imc_cell<3, true, false, lean>");
  in.ndim = cell.ndim = 1;
  in.tally = cell.tally = false;
  in.exact_geom = true;
  in.uniform_geom = cell.uniform = false;
  in.noabs = cell.noabs = true;
  ROW(in, cell, "k_imc_cell<1, false, true, lean>");
  in.ndim = cell.ndim = 2;
  in.tally = cell.tally = true;
  ROW(in, cell, "k_imc_cell<2, true, true, lean>");
  // otherwise k_transport<N, T, G, exact_geom, lean>
  TransportPlan want = plan(Family::k_transport, 2, false, true);
  in.noabs = false;
  in.no_imc_cell = true;
  want.gray = 1;
  want.exact = want.lean = true;
  ROW(in, want, "k_transport<2, true, 1, true, true>");
  in.no_imc_cell = false;
  in.cell_ok = false;
  in.exact_geom = want.exact = false;
  in.tally = want.tally = false;
  ROW(in, want, "k_transport<2, false, 1, false, true>");
  in.cell_ok = true;
  in.lean_arith = want.lean = false;
  in.exact_geom = want.exact = true;
  in.ndim = want.ndim = 3;
  in.tally = want.tally = true;
  ROW(in, want, "k_transport<3, true, 1, true, false>");
  in.exact_geom = want.exact = false;
  in.noabs = true;
  want.gray = 2;
  in.ndim = want.ndim = 1;
  in.tally = want.tally = false;
  ROW(in, want, "k_transport<1, false, 2, false, false>");
  // frequency-dependent opacities: <N, T, 0, false, false>
  in.gray = false;
  in.lean_arith = in.exact_geom = true;
  in.ndim = want.ndim = 3;
  in.tally = want.tally = true;
  want.gray = 0;
  ROW(in, want, "k_transport<3, true, 0, false, false>");
}

static void test_name_buffer() {
  // the longest name fits the 64 bytes the mesh keeps for it
  const TransportPlan longest = ddmc_plan(Family::k_ddmc_q, 3, false, 4, true, 0);
  const std::vector<char> full = name_of(longest);
  EXPECT(std::strcmp(full.data(), "k_ddmc_all<3, false, cell codes, queues, codes in LDS>") == 0);
  EXPECT(std::strlen(full.data()) < 64);
  // a shorter buffer gets the head of it, terminated
  const std::vector<char> cut = name_of(longest, 12);
  EXPECT(std::strcmp(cut.data(), "k_ddmc_all<") == 0);
}

int main() {
  test_queues_and_codes_in_lds();
  test_queues_off();
  test_more_classes_than_max();
  test_coop_gather_forced();
  test_large_tables();
  test_mixed_mesh();
  test_imc_entry();
  test_name_buffer();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("ok: %d rows\n", rows);
  return 0;
}
