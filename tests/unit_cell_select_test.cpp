// When select_transport (jaybenne_amd/csrc/jb_select.hpp) asks for k_imc_cell's unit-cell form, on the host
// (tests/test_unit_cell_select_host.py): every combination of the inputs that could bear on it.  The rule is written
// out here by hand -- a gray IMC call in lean arithmetic on a mesh the cell-local kernel takes, whose resident blocks
// all have one cell size, with power-of-two widths -- not computed by a second copy of select_transport.
#include <cstdio>
#include <cstring>

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

static void name_of(const TransportPlan &p, char (&buf)[64]) {
  std::memset(buf, '#', sizeof buf);
  variant_name(p, buf, sizeof buf);
}

int main() {
  // 2^12 combinations: entry point, opacities, DDMC tables, the five conditions, equal widths, the library switch,
  // absorption, tally
  for (unsigned bits = 0; bits < (1u << 12); ++bits) {
    const auto bit = [&](int i) { return ((bits >> i) & 1u) != 0; };
    for (int ndim = 1; ndim <= 3; ++ndim) {
      TransportInputs in;
      in.ndim = ndim;
      in.nblocks = 8;
      in.ntot = 4096;
      in.last = 100000;
      in.ddmc = bit(0);
      in.gray = bit(1);
      in.has_ddmc_cell = in.has_ddmc_code = in.not_all_ddmc = bit(2);
      in.uniform_geom = bit(3);
      in.exact_geom = bit(4);
      in.cell_ok = bit(5);
      in.lean_arith = bit(6);
      in.no_imc_cell = bit(7);
      in.equal_h = bit(8);
      in.unit_cell_form = bit(9);
      in.noabs = bit(10);
      in.tally = bit(11);
      in.nclass = 2;
      const TransportPlan p = select_transport(in);
      ++rows;
      const bool gray_imc_call = in.gray && !in.ddmc;
      const bool want = gray_imc_call && in.uniform_geom && in.exact_geom && in.cell_ok && in.lean_arith &&
                        !in.no_imc_cell && in.unit_cell_form;
      EXPECT(p.unit_cell == want);
      EXPECT(p.equal_h == (want && in.equal_h));
      if (p.unit_cell) {
        EXPECT(p.family == Family::k_imc_cell && p.uniform && p.noabs == in.noabs && p.tally == in.tally);
      }
      // the name does not depend on the new fields, nor on the inputs behind them
      TransportInputs off = in;
      off.unit_cell_form = false;
      off.equal_h = false;
      const TransportPlan q = select_transport(off);
      EXPECT(!q.unit_cell && !q.equal_h);
      EXPECT(q.family == p.family && q.uniform == p.uniform && q.noabs == p.noabs && q.mode == p.mode &&
             q.gray == p.gray && q.exact == p.exact && q.lean == p.lean);
      char a[64], b[64];
      name_of(p, a);
      name_of(q, b);
      EXPECT(std::strcmp(a, b) == 0);
    }
  }
  // the defaults: a library with the form; nothing known about the widths
  EXPECT(TransportInputs{}.unit_cell_form && !TransportInputs{}.equal_h);
  EXPECT(!TransportPlan{}.unit_cell && !TransportPlan{}.equal_h);
  // the headline call by name, as bench.py reads it, with and without the form
  TransportInputs c2;
  c2.ndim = 3;
  c2.tally = c2.gray = c2.noabs = true;
  c2.nblocks = 64;
  c2.ntot = 68 * 68 * 68;
  c2.last = 10000000;
  c2.exact_geom = c2.cell_ok = c2.uniform_geom = c2.equal_h = true;
  char name[64];
  name_of(select_transport(c2), name);
  EXPECT(std::strcmp(name, "k_imc_cell<3, true, true, lean>") == 0);
  EXPECT(select_transport(c2).unit_cell && select_transport(c2).equal_h);
  c2.exact_geom = false;   // (cell width 1 / 24)
  name_of(select_transport(c2), name);
  EXPECT(std::strcmp(name, "k_imc_cell<3, true, true, lean>") == 0);
  EXPECT(!select_transport(c2).unit_cell && !select_transport(c2).equal_h && select_transport(c2).uniform);
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("ok: %d rows\n", rows);
  return 0;
}
