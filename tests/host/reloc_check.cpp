// reloc_check.cpp -- nemo_score_relocations' host-side argument check
// (nemo::host::check_w_full, nemo_host.h) as a stand-alone program: built with
// the host sanitizers by tests/test_reloc_cpu.py.  No device, no library.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "nemo_host.h"

using nemo::host::check_w_full;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                    \
    }                                                                \
  } while (0)

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (int S : {2, 5}) {
    // NaN on the diagonal, valid values everywhere else: accepted
    std::vector<double> w(2 * S * S);
    for (int b = 0; b < 2; ++b)
      for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j) w[(b * S + i) * S + j] = i == j ? nan : (i + 2 * j + b) % 3 * 0.5;
    CHECK(check_w_full(w.data(), 2, S) == 0);
    // each off-diagonal entry in turn: NaN, infinities and values outside [0, 1] are found, at its index
    for (int b = 0; b < 2; ++b)
      for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j) {
          if (i == j) continue;
          const size_t k = (size_t)(b * S + i) * S + j;
          const double keep = w[k];
          for (double bad : {nan, inf, -inf, -1e-300, std::nextafter(1.0, 2.0), 2.0}) {
            w[k] = bad;
            CHECK(check_w_full(w.data(), 2, S) == k + 1);
          }
          for (double good : {0.0, -0.0, 1.0, 5e-324}) {
            w[k] = good;
            CHECK(check_w_full(w.data(), 2, S) == 0);
          }
          w[k] = keep;
        }
  }
  CHECK(check_w_full(nullptr, 0, 4) == 0);
  if (failures) return 1;
  std::printf("reloc_check: ok\n");
  return 0;
}
