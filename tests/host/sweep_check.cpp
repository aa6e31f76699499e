// sweep_check.cpp -- nemo_edge_sweep's host-side threshold check
// (nemo::host::check_sweep_thr, nemo_host.h) as a stand-alone program: built
// with the host sanitizers by tests/test_sweep_cpu.py.  No device, no library.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "nemo_host.h"

using nemo::host::check_sweep_thr;

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
    // NaN everywhere off the permissible set: not looked at
    std::vector<double> t(2 * S * S, nan);
    for (int b = 0; b < 2; ++b)
      for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j)
          if (permissible(b, i, j, cap)) t[(b * S + i) * S + j] = (i + j) % 3 - 1.0;
    CHECK(check_sweep_thr(pos.data(), t.data(), 2, S, cap) == 0);
    // each permissible entry in turn: a NaN is found at its index; the infinities are decisions
    for (int b = 0; b < 2; ++b)
      for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j) {
          if (!permissible(b, i, j, cap)) continue;
          const size_t k = (size_t)(b * S + i) * S + j;
          const double keep = t[k];
          t[k] = nan;
          CHECK(check_sweep_thr(pos.data(), t.data(), 2, S, cap) == k + 1);
          for (double good : {inf, -inf, 0.0, -0.0, 1e300, -5e-324}) {
            t[k] = good;
            CHECK(check_sweep_thr(pos.data(), t.data(), 2, S, cap) == 0);
          }
          t[k] = keep;
        }
  }
  CHECK(check_sweep_thr(nullptr, nullptr, 0, S, 0) == 0);
  if (failures) return 1;
  std::printf("sweep_check: ok\n");
  return 0;
}
