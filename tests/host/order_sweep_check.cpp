// order_sweep_check.cpp -- nemo_order_sweep's host-side argument checks
// (nemo::host::check_visit and check_sweep_u, nemo_host.h) as a stand-alone
// program: built with the host sanitizers by tests/test_order_sweep_cpu.py.  No
// device, no library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "nemo_host.h"

using nemo::host::check_sweep_u;
using nemo::host::check_visit;

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
    for (int nv : {1, 3, 2 * S + 1}) {
      const int batch = 3;
      // repeated labels and lists that are no permutation: accepted
      std::vector<int32_t> visit((size_t)batch * nv);
      for (size_t k = 0; k < visit.size(); ++k) visit[k] = (int32_t)((k / 2) % S);
      CHECK(check_visit(visit.data(), batch, nv, S) == 0);
      std::vector<double> u((size_t)batch * nv);
      for (size_t k = 0; k < u.size(); ++k) u[k] = (double)(k % 7) / 7.0;
      CHECK(check_sweep_u(u.data(), batch, nv) == 0);
      // each entry in turn: found at its index
      for (size_t k = 0; k < visit.size(); ++k) {
        const int32_t keep = visit[k];
        for (int32_t bad : {-1, S, S + 7, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max()}) {
          visit[k] = bad;
          CHECK(check_visit(visit.data(), batch, nv, S) == k + 1);
        }
        for (int32_t good : {0, S - 1}) {
          visit[k] = good;
          CHECK(check_visit(visit.data(), batch, nv, S) == 0);
        }
        visit[k] = keep;
      }
      for (size_t k = 0; k < u.size(); ++k) {
        const double keep = u[k];
        for (double bad : {nan, inf, -inf, -5e-324, -1.0}) {
          u[k] = bad;
          CHECK(check_sweep_u(u.data(), batch, nv) == k + 1);
        }
        for (double good : {0.0, -0.0, 1.0, 2.0, std::numeric_limits<double>::max(), 5e-324}) {
          u[k] = good;
          CHECK(check_sweep_u(u.data(), batch, nv) == 0);
        }
        u[k] = keep;
      }
    }
  }
  // no visits, no batch: nothing is read
  CHECK(check_visit(nullptr, 0, 4, 4) == 0);
  CHECK(check_visit(nullptr, 3, 0, 4) == 0);
  CHECK(check_sweep_u(nullptr, 0, 4) == 0);
  CHECK(check_sweep_u(nullptr, 3, 0) == 0);
  if (failures) return 1;
  std::printf("order_sweep_check: ok\n");
  return 0;
}
