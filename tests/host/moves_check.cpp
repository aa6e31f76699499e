// moves_check.cpp -- nemo_score_moves' host-side argument check
// (nemo::host::check_w_alt, nemo_host.h) as a stand-alone program: built with
// the host sanitizers by tests/test_moves_cpu.py.  No device, no library.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "nemo_host.h"

using nemo::host::check_w_alt;

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
  const int S = 4;
  // two evaluations: order 2 0 3 1 (pos = 1 3 0 2) and the identity
  const std::vector<int32_t> pos = {1, 3, 0, 2, 0, 1, 2, 3};
  auto permissible = [&](int b, int i, int j, int cap) {
    const int d = pos[b * S + i] - pos[b * S + j];
    return d > 0 && (cap == 0 || cap >= S - 1 || d <= cap);
  };
  for (int cap : {0, 1, 2, 3, 9}) {
    // NaN everywhere off the permissible set, valid values on it: accepted
    std::vector<double> w(2 * S * S, nan);
    for (int b = 0; b < 2; ++b)
      for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j)
          if (permissible(b, i, j, cap)) w[(b * S + i) * S + j] = (i + j) % 3 * 0.5;
    CHECK(check_w_alt(pos.data(), w.data(), 2, S, cap) == 0);
    // each permissible entry in turn: NaN, infinities and values outside [0, 1] are found, at its index
    for (int b = 0; b < 2; ++b)
      for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j) {
          if (!permissible(b, i, j, cap)) continue;
          const size_t k = (size_t)(b * S + i) * S + j;
          const double keep = w[k];
          for (double bad : {nan, inf, -inf, -1e-300, std::nextafter(1.0, 2.0), 2.0}) {
            w[k] = bad;
            CHECK(check_w_alt(pos.data(), w.data(), 2, S, cap) == k + 1);
          }
          for (double good : {0.0, -0.0, 1.0, 5e-324}) {
            w[k] = good;
            CHECK(check_w_alt(pos.data(), w.data(), 2, S, cap) == 0);
          }
          w[k] = keep;
        }
  }
  CHECK(check_w_alt(nullptr, nullptr, 0, S, 0) == 0);
  if (failures) return 1;
  std::printf("moves_check: ok\n");
  return 0;
}
