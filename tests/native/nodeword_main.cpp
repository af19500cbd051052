// Stand-alone check of pylatticedso_amd/csrc/pl_nodeword.h (lever arms as three signed bytes), built by
// tests/test_nodeword_host.py with -fsanitize=address,undefined.  Prints OK and returns 0 when every check holds.
//
// With arguments "overflow nx ny nz cell" it answers instead whether the lever arms of ONE aggregate over an nx x ny x nz
// lattice of cubic cells (corner + centre nodes, reference point = the middle of the box) overflow the bytes: exit 0 and
// "overflow" if they do, exit 3 and "fits e" if not.  The GPU fall-back test sizes its long lattice with it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../pylatticedso_amd/csrc/pl_nodeword.h"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static std::vector<double> box_arms(int nx, int ny, int nz, double cell) {
  std::vector<double> d;
  const double c[3] = {0.5 * nx * cell, 0.5 * ny * cell, 0.5 * nz * cell};
  for (int i = 0; i <= 2 * nx; ++i)
    for (int j = 0; j <= 2 * ny; ++j)
      for (int k = 0; k <= 2 * nz; ++k) {
        if ((i & 1) != (j & 1) || (i & 1) != (k & 1)) continue;   // corners (all even) and cell centres (all odd)
        d.push_back(0.5 * i * cell - c[0]);
        d.push_back(0.5 * j * cell - c[1]);
        d.push_back(0.5 * k * cell - c[2]);
      }
  return d;
}

int main(int argc, char **argv) {
  if (argc == 6 && std::strcmp(argv[1], "overflow") == 0) {
    const std::vector<double> d = box_arms(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atof(argv[5]));
    std::vector<uint32_t> w;
    int e = -1;
    if (pl::pack_rel_bytes(d.data(), d.size() / 3, w, e)) {
      std::printf("fits %d\n", e);
      return 3;
    }
    std::printf("overflow\n");
    return 0;
  }
  std::vector<uint32_t> w;
  int e = -7;
  {   // exact round trip on dyadic inputs, and the smallest e is chosen
    const std::vector<double> d = {0.0, 1.0, -2.0, 0.5, -0.25, 3.75, 127.0 / 4, -127.0 / 4, 0.0};
    CHECK(pl::rel_byte_exponent(d.data(), d.size()) == 2);
    CHECK(pl::pack_rel_bytes(d.data(), 3, w, e));
    CHECK(e == 2 && w.size() == 3);
    for (size_t i = 0; i < 3 && w.size() == 3; ++i) {
      CHECK((w[i] >> 24) == 0u);
      for (int k = 0; k < 3; ++k) CHECK(pl::same_bits(pl::rel_byte_value(pl::node_word_byte(w[i], k), e), d[3 * i + k]));
    }
    const std::vector<double> ints = {3.0, -4.0, 100.0};
    CHECK(pl::rel_byte_exponent(ints.data(), 3) == 0);
    const std::vector<double> halves = {3.0, -4.5, 10.0};          // the entry that needs e = 1 comes second
    CHECK(pl::rel_byte_exponent(halves.data(), 3) == 1);
    const std::vector<double> finest = {1.0 / 256, 0.0, -0.25};
    CHECK(pl::rel_byte_exponent(finest.data(), 3) == 8);
    const std::vector<double> finer = {1.0 / 512, 0.0, 0.0};
    CHECK(pl::rel_byte_exponent(finer.data(), 3) == -1);
  }
  {   // 0.7-spaced inputs are not dyadic: refused, and the outputs stay as they were
    std::vector<double> d;
    for (int i = -4; i <= 4; ++i) d.push_back(0.7 * i);
    const std::vector<uint32_t> before = w;
    const int e_before = e;
    CHECK(pl::rel_byte_exponent(d.data(), d.size()) == -1);
    CHECK(!pl::pack_rel_bytes(d.data(), 3, w, e));
    CHECK(w == before && e == e_before);
  }
  {   // magnitude 127 is accepted, 128 refused - also when a LATER entry raises e past what an earlier one can bear
    const std::vector<double> ok = {127.0, -127.0, 0.0};
    CHECK(pl::pack_rel_bytes(ok.data(), 1, w, e) && e == 0);
    CHECK(pl::node_word_byte(w[0], 0) == 127 && pl::node_word_byte(w[0], 1) == -127 && pl::node_word_byte(w[0], 2) == 0);
    const std::vector<double> over = {128.0, 0.0, 0.0}, under = {0.0, -128.0, 0.0};
    CHECK(!pl::pack_rel_bytes(over.data(), 1, w, e));
    CHECK(!pl::pack_rel_bytes(under.data(), 1, w, e));
    const std::vector<double> late = {100.0, 0.0, 0.5};             // 100 fits at e = 0 but is 200 units at e = 1
    CHECK(pl::rel_byte_exponent(late.data(), 3) == -1);
    const std::vector<double> scaled_ok = {63.5, 0.0, 0.0}, scaled_over = {64.0, 0.5, 0.0};
    CHECK(pl::rel_byte_exponent(scaled_ok.data(), 3) == 1);
    CHECK(pl::rel_byte_exponent(scaled_over.data(), 3) == -1);
  }
  {   // what no byte can hold
    const std::vector<double> negzero = {-0.0, 1.0, 2.0};
    CHECK(!pl::pack_rel_bytes(negzero.data(), 1, w, e));
    const std::vector<double> bad = {std::numeric_limits<double>::infinity(), 0.0, 0.0};
    CHECK(pl::rel_byte_exponent(bad.data(), 3) == -1);
    CHECK(pl::rel_byte_exponent(nullptr, 0) == 0);                  // no lever arm at all: nothing to refuse
  }
  {   // lattices: unit cells fit, one aggregate along a 300-cell lattice does not
    std::vector<double> d = box_arms(4, 4, 4, 1.0);
    CHECK(pl::pack_rel_bytes(d.data(), d.size() / 3, w, e) && e == 1);
    d = box_arms(4, 4, 4, 0.7);
    CHECK(!pl::pack_rel_bytes(d.data(), d.size() / 3, w, e));
    d = box_arms(300, 1, 1, 1.0);
    CHECK(!pl::pack_rel_bytes(d.data(), d.size() / 3, w, e));
  }
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
