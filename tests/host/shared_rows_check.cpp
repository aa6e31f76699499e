// shared_rows_check.cpp -- the host side of a row-shared real-valued table
// (option exact_generic, csrc/nemo_host.h), stand-alone:
//   * parts_lm1_rows: the plan-ordered lv - 1 rows hold lv - 1 of every
//     element exactly once and 0 at every other position;
//   * detect_row_shared accepts the broadcast of R and rejects it after one
//     element of one child's copy changed (a last-bit change and a sign of
//     zero included);
//   * detect_factored_rows on R gives what detect_factored gives on the
//     broadcast table, for a real-valued R (neither factorable) and a
//     two-valued one (the same bits, lo / hi values and exponentials).
// Prints one line per E and returns the number of failures.
//   g++ -O2 -std=c++17 -I csrc tests/host/shared_rows_check.cpp && ./a.out
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "nemo_host.h"

using namespace nemo::host;

static int failures = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      ++failures;                     \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");              \
    }                                 \
  } while (0)

static std::vector<double> broadcast(int S, int E, const std::vector<double>& R) {
  std::vector<double> T((size_t)S * S * E);
  for (int i = 0; i < S; ++i)
    for (int j = 0; j < S; ++j) std::memcpy(&T[((size_t)i * S + j) * E], &R[(size_t)j * E], (size_t)E * 8);
  return T;
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * 8) == 0);
}

static void check_lm1(int S, int E, std::mt19937_64& rng) {
  std::vector<PairwisePlan> parts;
  CHECK(build_pairwise_parts(E, parts), "E=%d: no plan", E);
  if (parts.empty()) return;
  const size_t pd = parts.size() * (size_t)parts_slots(parts) * 17 * 64;
  // lv > 0 and != 1, so lv - 1 is never the 0 of an empty position
  std::uniform_real_distribution<double> lvd(1.5, 90.0);
  std::vector<double> X((size_t)S * E), rows;
  for (double& v : X) v = lvd(rng);
  parts_lm1_rows(parts, S, E, X.data(), rows);
  CHECK(rows.size() == (size_t)S * pd, "E=%d: %zu doubles, expected %zu", E, rows.size(), (size_t)S * pd);
  std::vector<int32_t> pos;
  parts_positions(parts, E, pos);
  for (int k = 0; k < S; ++k) {
    std::vector<int> hits(pd, 0);
    const double* row = &rows[(size_t)k * pd];
    for (int e = 0; e < E; ++e) {
      const size_t q = (size_t)pos[(size_t)e];
      CHECK(q < pd, "E=%d: element %d at %zu past the row set", E, e, q);
      if (q >= pd) return;
      ++hits[q];
      const double want = X[(size_t)k * E + e] - 1.0;
      CHECK(std::memcmp(&row[q], &want, 8) == 0, "E=%d row %d element %d: %a, expected %a", E, k, e, row[q], want);
    }
    size_t filled = 0;
    for (size_t q = 0; q < pd; ++q) {
      CHECK(hits[q] <= 1, "E=%d: position %zu holds %d elements", E, q, hits[q]);
      filled += hits[q] ? 1 : 0;
      const double zero = 0.0;
      if (!hits[q]) CHECK(std::memcmp(&row[q], &zero, 8) == 0, "E=%d row %d: padding %zu holds %a", E, k, q, row[q]);
    }
    CHECK(filled == (size_t)E, "E=%d row %d: %zu positions filled", E, k, filled);
  }
}

static void check_detection(int S, int E, std::mt19937_64& rng) {
  std::normal_distribution<double> nd(0.0, 1.0);
  std::vector<double> R((size_t)S * E);
  for (double& v : R) v = nd(rng);
  R[(size_t)(S - 1) * E + E / 2] = 0.0;   // (for the sign-of-zero case)
  std::vector<double> T = broadcast(S, E, R);
  CHECK(detect_row_shared(S, E, T.data()), "E=%d: the broadcast is not row-shared", E);
  // one changed element in one child's copy: the first and the last child of
  // a parent, the first and the last effect, the diagonal rows left alone
  const int cases[4][3] = {{1, 0, 0}, {S - 1, 0, E - 1}, {0, S - 1, E / 2}, {S - 2, S - 1, E - 1}};
  for (const auto& cs : cases) {
    const size_t at = ((size_t)cs[0] * S + cs[1]) * E + cs[2];
    const double keep = T[at];
    uint64_t b;
    std::memcpy(&b, &keep, 8);
    b ^= 1ull;   // the last bit
    std::memcpy(&T[at], &b, 8);
    CHECK(!detect_row_shared(S, E, T.data()), "E=%d: a last-bit change at [%d][%d][%d] is accepted", E, cs[0], cs[1],
          cs[2]);
    T[at] = keep;
  }
  {
    const size_t at = ((size_t)0 * S + (S - 1)) * E + E / 2;   // holds +0.0
    T[at] = -0.0;
    CHECK(!detect_row_shared(S, E, T.data()), "E=%d: -0.0 against +0.0 is accepted", E);
    T[at] = 0.0;
  }
  T[((size_t)1 * S + 1) * E] += 1.0;   // a diagonal row is nobody's parent row
  CHECK(detect_row_shared(S, E, T.data()), "E=%d: a changed diagonal row is rejected", E);

  // factored detection: R against the broadcast
  std::vector<uint64_t> d1a, d1b;
  std::vector<double> loa, hia, tla, tha, lob, hib, tlb, thb;
  T = broadcast(S, E, R);
  const bool fa = detect_factored_rows(S, E, R.data(), d1a, loa, hia, &tla, &tha);
  const bool fb = detect_factored(S, E, T.data(), d1b, lob, hib, &tlb, &thb);
  CHECK(!fa && !fb, "E=%d: a real-valued R detected as factored (%d, %d)", E, (int)fa, (int)fb);
  std::vector<double> R2((size_t)S * E);
  for (int j = 0; j < S; ++j) {
    const double lo = nd(rng), hi = nd(rng);
    for (int e = 0; e < E; ++e) R2[(size_t)j * E + e] = (rng() & 1) ? hi : lo;
  }
  for (int e = 0; e < E; ++e) R2[e] = R2[0];   // a constant row: hi never seen
  T = broadcast(S, E, R2);
  const bool ga = detect_factored_rows(S, E, R2.data(), d1a, loa, hia, &tla, &tha);
  const bool gb = detect_factored(S, E, T.data(), d1b, lob, hib, &tlb, &thb);
  CHECK(ga && gb, "E=%d: a two-valued R not detected as factored (%d, %d)", E, (int)ga, (int)gb);
  CHECK(d1a == d1b && same_bits(loa, lob) && same_bits(hia, hib) && same_bits(tla, tlb) && same_bits(tha, thb),
        "E=%d: detect_factored_rows differs from detect_factored on the broadcast", E);
  R2[(size_t)(S - 1) * E + E - 1] = 7.25;   // a third value in one row
  T = broadcast(S, E, R2);
  CHECK(detect_factored_rows(S, E, R2.data(), d1a, loa, hia) == detect_factored(S, E, T.data(), d1b, lob, hib),
        "E=%d: three-valued row", E);
}

int main() {
  std::mt19937_64 rng(20240607);
  const int S = 4;
  for (int E : {130, 8192, 8193, 8200, 16500}) {
    const int before = failures;
    check_lm1(S, E, rng);
    check_detection(S, E, rng);
    std::printf("E=%d: %s\n", E, failures == before ? "ok" : "FAILED");
  }
  return failures ? 1 : 0;
}
