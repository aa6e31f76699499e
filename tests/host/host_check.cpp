// host_check.cpp -- the C-ABI's host logic (nem-mcmc-optimization_amd/csrc/
// nemo_host.h) driven on the CPU, built by tests/test_host_sanitizers.py with
// g++ under -fsanitize=address,undefined and, separately, -fsanitize=thread.
// Prints "ok <checks>" and exits 0, or names the first failed check and
// exits 1.  No HIP: this is the part of libnemo.so that never touches a GPU.
#include "nemo_host.h"

#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <random>
#include <map>
#include <set>
#include <tuple>

using namespace nemo::host;

static int g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

// ---- argument checks -------------------------------------------------------
static void check_pos_rows() {
  std::vector<int32_t> pos = {0, 1, 2, 2, 0, 1, 1, 1, 0};
  CHECK(first_bad_pos_row(pos.data(), 2, 3) == -1);
  CHECK(first_bad_pos_row(pos.data(), 3, 3) == 2);
  std::vector<int32_t> neg = {0, -1};
  CHECK(first_bad_pos_row(neg.data(), 1, 2) == 0);
  std::vector<int32_t> big = {0, 2};
  CHECK(first_bad_pos_row(big.data(), 1, 2) == 0);
  CHECK(first_bad_pos_row(nullptr, 0, 5) == -1);
}

// ---- staging validation --------------------------------------------------------
// A table built the way nem.py builds it (off-diagonal row j = where(D[j] == 0,
// B, -A) for every child) is detected as factored with exactly the D1 bits and
// exp values the knockdown staging derives from D itself; any perturbation of
// one off-diagonal entry breaks the structure.
static void check_staging(std::mt19937_64& rng) {
  for (int trial = 0; trial < 30; ++trial) {
    const int S = 2 + (int)(rng() % 20), E = 1 + (int)(rng() % 200);
    const double A = -2.8904, B = -2.2513 - 0.01 * trial;
    std::vector<uint8_t> D((size_t)S * E);
    for (auto& d : D) d = (uint8_t)(rng() % 3 == 0);
    std::vector<double> T((size_t)S * S * E);
    for (int i = 0; i < S; ++i)
      for (int j = 0; j < S; ++j)
        for (int e = 0; e < E; ++e)
          T[((size_t)i * S + j) * E + e] =
              i == j ? 0.25 * (double)(rng() % 9) : (D[(size_t)j * E + e] ? -A : B);
    std::vector<uint64_t> d1a, d1b;
    std::vector<double> loa, hia, lob, hib;
    CHECK(detect_factored(S, E, T.data(), d1a, loa, hia));
    knockdown_factored(S, E, D.data(), A, B, d1b, lob, hib);
    CHECK(d1a == d1b && loa == lob);
    for (int j = 0; j < S; ++j) {
      bool any = false;
      for (int e = 0; e < E; ++e) any |= ((d1a[(size_t)j * ((E + 63) / 64) + e / 64] >> (e % 64)) & 1) != 0;
      if (any) CHECK(hia[j] == hib[j]);  // hi_j only matters where a bit is set
    }
    if (S > 2) {
      const int j = (int)(rng() % S), i = (j + 1 + (int)(rng() % (S - 1))) % S, e = (int)(rng() % E);
      std::vector<double> T2 = T;
      T2[((size_t)i * S + j) * E + e] += 1e-12;
      CHECK(!detect_factored(S, E, T2.data(), d1a, loa, hia));
    }
  }
  const std::vector<double> ch = knockdown_chains(3, 0.5, -1.0);
  CHECK(ch.size() == 8 && ch[0] == 0.0 && ch[3] == 1.5 && ch[4] == -1.0 && ch[7] == 0.5);
}

// ---- error bounds ------------------------------------------------------------
static void check_bounds(std::mt19937_64& rng) {
  for (int trial = 0; trial < 20; ++trial) {
    const int S = 2 + (int)(rng() % 70), E = 1 + (int)(rng() % 300);
    const int nwords = (E + 63) / 64;
    std::vector<uint64_t> d1((size_t)S * nwords);
    const uint64_t dens = rng() % 4;
    for (auto& w : d1) {
      w = rng();
      for (uint64_t k = 0; k < dens; ++k) w &= rng();
    }
    // bits past E are padding: the colsums must not read them
    for (int j = 0; j < S; ++j)
      if (E % 64) d1[(size_t)j * nwords + nwords - 1] &= (1ull << (E % 64)) - 1;
    const std::vector<double> cs = fixed_point_colsums(S, E, d1.data(), nwords);
    CHECK(cs.size() == (size_t)S + 1);
    for (int k = 0; k <= S; ++k) {
      double ref = 0.0;
      for (int e = 0; e < E; ++e) {
        int n = 0;
        for (int j = 0; j < S; ++j) n += (int)((d1[(size_t)j * nwords + e / 64] >> (e % 64)) & 1);
        ref += std::min(n, k);
      }
      CHECK(cs[(size_t)k] == ref);
    }
    // a cap never raises the bound; no cap equals cap >= S - 1
    const int cexp = (int)(rng() % 6);
    for (int kind : {kFxLog2, kFxNatural}) {
      const double b0 = fixed_point_bound(kind, cexp, cs, S, E, 0);
      CHECK(b0 > 0.0 && std::isfinite(b0));
      CHECK(fixed_point_bound(kind, cexp, cs, S, E, S - 1) == b0);
      double prev = 0.0;
      for (int cap = 1; cap < S - 1; ++cap) {
        const double b = fixed_point_bound(kind, cexp, cs, S, E, cap);
        CHECK(b <= b0 && b >= prev);
        prev = b;
      }
    }
    // the worst case the formula can reach: every row's bit set everywhere
    const double full = fixed_point_bound(kFxLog2, 0, std::vector<double>(cs.size(), 0.0), S, E, 0);
    CHECK(full > 0.0);
  }
  // a colsum vector of the wrong size is no bound at all
  CHECK(std::isinf(fixed_point_bound(kFxLog2, 0, std::vector<double>(3, 0.0), 5, 10, 0)));
}

// ---- InverseMethod level schedule ---------------------------------------------
// The reference's pair loop (methods.py:125-127) updates the pairs one at a
// time, each reading the entries its objective depends on (b ~> c and r ~> a
// in the graph of lower-triangle pairs).  The schedule runs a level's pairs
// together, all reading the state before the level.  Simulate both with an
// opaque update (a hash of everything read) and require the same final state.
static uint64_t mix(uint64_t h, uint64_t v) {
  h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
  return h * 0xff51afd7ed558ccdull;
}

static void check_inverse_schedule_case(std::mt19937_64& rng, int S, int nprob) {
  {
    std::vector<int32_t> pos((size_t)nprob * S);
    for (int b = 0; b < nprob; ++b) {
      std::vector<int32_t> perm(S);
      for (int i = 0; i < S; ++i) perm[i] = i;
      std::shuffle(perm.begin(), perm.end(), rng);
      for (int i = 0; i < S; ++i) pos[(size_t)b * S + perm[i]] = i;
    }
    InverseSchedule sch;
    CHECK(!build_inverse_schedule(sch, S, nprob, pos.data()));
    CHECK(build_inverse_schedule(sch, S, nprob, pos.data()));  // cached
    std::set<int32_t> seen;
    for (int32_t e : sch.list) CHECK(seen.insert(e).second);
    for (int32_t e : sch.skip) CHECK(seen.insert(e).second);
    CHECK(sch.level_off.front() == 0 && sch.level_off.back() == (int)sch.list.size());
    for (size_t l = 0; l + 1 < sch.level_off.size(); ++l) CHECK(sch.level_off[l] < sch.level_off[l + 1]);
    for (int b = 0; b < nprob; ++b) {
      const int32_t* pb = pos.data() + (size_t)b * S;
      std::vector<int> perm(S);
      for (int i = 0; i < S; ++i) perm[pb[i]] = i;
      // the reference's loop order, lower-triangle pairs only
      std::vector<int32_t> loop;
      std::vector<char> edge((size_t)S * S, 0);
      size_t nperm = 0;
      for (int i = 0; i < S; ++i)
        for (int p = 0; p < pb[i]; ++p) {
          const int k = perm[p];
          const int32_t ent = (b << 16) | (i << 8) | k;
          ++nperm;
          CHECK(seen.count(ent));
          if (perm[i] > perm[k]) {
            loop.push_back(ent);
            edge[(size_t)perm[i] * S + perm[k]] = 1;
          }
        }
      // reachability by Floyd-Warshall (y ~> x: a chain of entries x -> .. -> y)
      std::vector<char> reach((size_t)S * S, 0);
      for (int x = 0; x < S; ++x) {
        reach[(size_t)x * S + x] = 1;
        for (int y = 0; y < S; ++y)
          if (edge[(size_t)x * S + y]) reach[(size_t)x * S + y] = 1;
      }
      for (int m = 0; m < S; ++m)
        for (int x = 0; x < S; ++x)
          if (reach[(size_t)x * S + m])
            for (int y = 0; y < S; ++y)
              if (reach[(size_t)m * S + y]) reach[(size_t)x * S + y] = 1;
      auto ab = [&](int32_t ent) {
        const int i = (ent >> 8) & 0xff, k = ent & 0xff;
        return std::make_pair(perm[i], perm[k]);
      };
      // reads(p) = entries (r, c) with b_p ~> c and r ~> a_p: pair p reads
      // pair q when reach[b_q][b_p] && reach[a_p][a_q]
      std::vector<uint64_t> seq((size_t)S * S), par;
      for (size_t k = 0; k < seq.size(); ++k) seq[k] = k * 0x1234567ull + 1;
      par = seq;
      std::vector<std::vector<size_t>> rd(loop.size());  // entries each pair reads
      std::map<int32_t, size_t> at;
      // ab() of the loop's pairs, once (the S > 64 cases have ~10^8 (p, q))
      std::vector<int> la(loop.size()), lb(loop.size());
      for (size_t p = 0; p < loop.size(); ++p) std::tie(la[p], lb[p]) = ab(loop[p]);
      for (size_t p = 0; p < loop.size(); ++p) {
        at[loop[p]] = p;
        const char* from_b = &reach[0] + lb[p];            // reach[c][b_p]
        const char* to_a = &reach[(size_t)la[p] * S];      // reach[a_p][r]
        for (size_t q = 0; q < loop.size(); ++q)
          if (from_b[(size_t)lb[q] * S] && to_a[la[q]]) rd[p].push_back((size_t)la[q] * S + lb[q]);
      }
      auto update = [&](const std::vector<uint64_t>& st, int32_t p) {
        uint64_t h = (uint64_t)p;
        for (size_t e : rd[at[p]]) h = mix(h, st[e]);
        return h;
      };
      for (int32_t p : loop) {
        const auto [a, bb] = ab(p);
        seq[(size_t)a * S + bb] = update(seq, p);
      }
      for (size_t l = 0; l + 1 < sch.level_off.size(); ++l) {
        std::vector<std::pair<size_t, uint64_t>> commit;
        for (int o = sch.level_off[l]; o < sch.level_off[l + 1]; ++o) {
          const int32_t p = sch.list[o];
          if ((p >> 16) != b) continue;
          const auto [a, bb] = ab(p);
          commit.push_back({(size_t)a * S + bb, update(par, p)});
        }
        for (auto& cv : commit) par[cv.first] = cv.second;
      }
      CHECK(seq == par);
      (void)nperm;
    }
    CHECK(seen.size() == sch.list.size() + sch.skip.size());
  }
}

static void check_inverse_schedule(std::mt19937_64& rng) {
  for (int trial = 0; trial < 60; ++trial) {
    const int S = 2 + (int)(rng() % 24), nprob = 1 + (int)(rng() % 3);
    check_inverse_schedule_case(rng, S, nprob);
  }
  // reachability rows of W = (S + 63) / 64 words: W = 1 at its upper edge,
  // W = 2 at its lower edge, W = 3 and W = 4 (the orders of 64 < S <= 256
  // that column_solve<2> / <4> serve); two problems merge their levels
  const int wide[][2] = {{64, 2}, {65, 1}, {65, 2}, {130, 2}, {200, 1}};
  for (const auto& c : wide) check_inverse_schedule_case(rng, c[0], c[1]);
}

// ---- the asynchronous step queue ---------------------------------------------
struct Job {
  int id;
  double* out;
  int rc = 0;
};

// the pipelined form (nemo_optimal_weights_begin): start() puts a job "on the
// device" (a deadline) unless it fails at once, ready() polls the deadline,
// finish() waits for it and writes the output.  At most `depth` jobs in
// flight, started in submission order, finished in the same order, each
// collected after its finish; shutdown still drains everything
struct PJob {
  int id;
  double* out;
  int rc = 0;
  std::chrono::steady_clock::time_point due{};
  bool started = false, finished = false;
};

static void check_pipelined_queue(std::mt19937_64& rng) {
  using clk = std::chrono::steady_clock;
  for (int depth : {1, 2, 3}) {
    std::atomic<int> in_flight{0}, max_flight{0}, last_started{-1}, last_finished{-1};
    std::atomic<bool> order_ok{true};
    std::mutex rmu;
    std::mt19937_64 jr(rng());
    auto start = [&](PJob& j) {
      if (j.id != last_started + 1) order_ok = false;
      last_started = j.id;
      j.started = true;
      if (j.id % 7 == 6) {  // fails at start: complete at once, never in flight
        j.rc = -3;
        *j.out = -3.0;
        return false;
      }
      unsigned us;
      {
        std::lock_guard<std::mutex> g(rmu);
        us = (unsigned)(jr() % 120);
      }
      j.due = clk::now() + std::chrono::microseconds(us);
      const int f = ++in_flight;
      int m = max_flight.load();
      while (f > m && !max_flight.compare_exchange_weak(m, f)) {
      }
      return true;
    };
    auto ready = [](PJob& j) { return clk::now() >= j.due; };
    auto finish = [&](PJob& j) {
      std::this_thread::sleep_until(j.due);
      if (j.id <= last_finished) order_ok = false;
      last_finished = j.id;
      *j.out = 10.0 * j.id;
      j.finished = true;
      --in_flight;
    };
    {
      StepQueue<PJob> q(start, ready, finish, depth);
      std::vector<double> out(300, -1.0);
      std::vector<std::unique_ptr<PJob>> back;
      int next = 0, got = 0;
      while (got < 300) {
        const int burst = 1 + (int)(rng() % 4);
        for (int k = 0; k < burst && next < 300; ++k, ++next)
          CHECK(q.submit(std::unique_ptr<PJob>(new PJob{next, &out[next]}), nullptr));
        if (rng() % 3 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 200));
        const int take = (int)(rng() % 3);
        for (int k = 0; k < take && got < next; ++k, ++got) {
          std::unique_ptr<PJob> j = q.collect();
          const bool failed = got % 7 == 6;
          CHECK(j && j->id == got && j->started && j->finished == !failed);
          CHECK(out[got] == (failed ? -3.0 : 10.0 * got) && j->rc == (failed ? -3 : 0));
        }
      }
      CHECK(q.collect() == nullptr && q.pending() == 0);
    }
    CHECK(order_ok.load() && max_flight.load() <= depth && in_flight.load() == 0);
    // shutdown with jobs queued and in flight: all of them finish
    {
      std::vector<double> out(40, -1.0);
      last_started = -1;
      last_finished = -1;
      StepQueue<PJob> q(start, ready, finish, depth);
      const int n = 1 + (int)(rng() % 40);
      for (int k = 0; k < n; ++k) CHECK(q.submit(std::unique_ptr<PJob>(new PJob{k, &out[k]}), nullptr));
      q.shutdown();
      for (int k = 0; k < n; ++k) CHECK(out[k] == (k % 7 == 6 ? -3.0 : 10.0 * k));
      CHECK(in_flight.load() == 0);
    }
  }
}

static void check_step_queue(std::mt19937_64& rng) {
  // collected in submission order, each after it ran
  {
    std::atomic<int> ran{0};
    StepQueue<Job> q([&](Job& j) {
      std::this_thread::sleep_for(std::chrono::microseconds(50 * (j.id % 3)));
      *j.out = 10.0 * j.id;
      j.rc = j.id % 5 == 4 ? -5 : 0;
      ++ran;
    });
    std::vector<double> out(200, -1.0);
    int next = 0, got = 0;
    while (got < 200) {
      const int burst = 1 + (int)(rng() % 4);
      for (int k = 0; k < burst && next < 200; ++k, ++next) {
        std::string err;
        CHECK(q.submit(std::unique_ptr<Job>(new Job{next, &out[next]}), &err));
      }
      const int take = (int)(rng() % 3);
      for (int k = 0; k < take && got < next; ++k, ++got) {
        std::unique_ptr<Job> j = q.collect();
        CHECK(j && j->id == got && out[got] == 10.0 * got && j->rc == (got % 5 == 4 ? -5 : 0));
      }
    }
    CHECK(q.collect() == nullptr);
    CHECK(q.pending() == 0 && ran == 200);
  }
  // shutdown with steps queued and not collected: every one still runs
  for (int trial = 0; trial < 20; ++trial) {
    std::vector<double> out(16, -1.0);
    {
      StepQueue<Job> q([](Job& j) {
        std::this_thread::sleep_for(std::chrono::microseconds(20));
        *j.out = j.id;
      });
      const int n = 1 + (int)(rng() % 16);
      for (int k = 0; k < n; ++k) CHECK(q.submit(std::unique_ptr<Job>(new Job{k, &out[k]}), nullptr));
      if (trial % 2) (void)q.collect();
      q.shutdown();
      for (int k = 0; k < n; ++k) CHECK(out[k] == k);
      std::string err;
      CHECK(!q.submit(std::unique_ptr<Job>(new Job{0, &out[0]}), &err) && !err.empty());
    }  // the destructor after shutdown: nothing left to join or free twice
  }
  // a queue destroyed without shutdown or any job
  { StepQueue<Job> q([](Job&) {}); }
  check_pipelined_queue(rng);
}

// ---- the device's fixed-order partial sum on the host ------------------------
// sum_partials_host restates sum_partials (nemo_internal.h): 64 strided lane
// sums, then xor butterflies with o = 32, 16, ..., 1, lane 0's value.  Checked
// against the same tree written backwards as a recursion: lane l's value
// after the stages down to o is its value and lane (l ^ o)'s after the stages
// down to 2o, added.  Values whose sums round, so another association shows.
static double after_stages(const double* lanes, int l, int o) {
  if (o == 64) return lanes[l];
  return after_stages(lanes, l, 2 * o) + after_stages(lanes, l ^ o, 2 * o);
}
static void check_sum_partials(std::mt19937_64& rng) {
  std::uniform_real_distribution<double> u(-1e3, 1e3);
  for (int n : {0, 1, 5, 63, 64, 65, 127, 200, 1000}) {
    std::vector<double> p(n);
    for (auto& x : p) x = u(rng) * (1.0 + 1e-9 * u(rng));
    double lanes[64];
    for (int l = 0; l < 64; ++l) {
      double s = 0.0;
      for (int t = l; t < n; t += 64) s += p[t];
      lanes[l] = s;
    }
    CHECK(sum_partials_host(p.data(), n) == after_stages(lanes, 0, 1));
  }
  const double small[3] = {1.0, 2.0, 3.0};
  CHECK(sum_partials_host(small, 3) == 6.0);
  CHECK(sum_partials_host(small, 0) == 0.0);
}

// ---- the fact_kernel table against the decision code it replaced ---------------
// nemo_fact_kernels.h describes the 20 factored score-kernel variants in one
// table.  Before it, the same decisions were range tests on the option's
// integer in resolve_fact_kernel, score_partials, factored_partials and
// launch_score_factored, which handed launch_score_i8o a private code (0
// register-stationary, -3 persistent, -8 eight waves at occupancy 6, -2 two
// tiles, -20 split, else a wave count).  That code is restated here literally
// as the specification, over the same FactModel, and the table-driven
// functions must agree with it on every call it is defined on.
namespace spec {
constexpr int kFactWaves = 8, kPipeTilesPerWave = 8, kWideSetT = 2, kWinMaxCap = 6;

static int factored_partials(int E) {
  const int cols = kFactWaves * 16;
  const int nt = (E + 15) / 16;
  int n = ((E + cols - 1) / cols) * kFactWaves;
  for (int wv : {4, 8}) n = std::max(n, ((nt + kPipeTilesPerWave * wv - 1) / (kPipeTilesPerWave * wv)) * wv);
  return std::max(n, (E + 63) / 64);
}

static int score_partials(int E, int nwords, int fk) {
  const int nt = (E + 15) / 16;
  if (fk == 9 || fk == 15) return nwords;
  if (fk == 18 || fk == 19) return (nt + kWideSetT - 1) / kWideSetT;
  if (fk >= 4) return (nt + 7) / 8;
  if (fk == 2 || fk == 3) {
    const int wv = fk == 3 ? 8 : 4, tpb = kPipeTilesPerWave * wv;
    return ((nt + tpb - 1) / tpb) * wv;
  }
  const int cols = kFactWaves * 16;
  return ((E + cols - 1) / cols) * kFactWaves;
}

static int resolve(const FactModel& c, int option, int cap, bool ll_only, double* bound) {
  *bound = 0.0;
  if (cap >= c.S - 1) cap = 0;
  const bool i8cap = c.fspad <= 64 && c.b8 && ll_only;
  const bool wincap = ll_only && c.win_ok && cap >= 1 && cap <= kWinMaxCap;
  auto bnd = [&](int kind) { return kind == kFxLog2 ? c.bound_log2 : c.bound_natural; };
  const bool i8wcap = c.fspad == 128 && c.i8w_ok && c.b8 && ll_only;
  int fk = option;
  if (fk == 0) {
    if (wincap) fk = 9;
    else if (i8wcap && bnd(kFxLog2) <= c.err_budget) fk = 18;
    else if (!i8cap) fk = 1;
    else if (c.i8o_ok && c.i8l_ok && bnd(kFxLog2) <= c.err_budget) fk = 10;
    else if (c.i8o_ok && bnd(kFxNatural) <= c.err_budget) fk = 8;
    else if (!c.i8o_ok && bnd(kFxNatural) <= c.err_budget) fk = 4;
    else fk = 2;
  } else if (fk == 18 || fk == 19) {
    if (!ll_only || c.fspad != 128) fk = 1;
    else if (!i8wcap) return -1;
  } else if (fk == 9 || fk == 15) {
    if (!wincap) return -1;
  } else if (fk == 2 || fk == 3) {
    if (!(ll_only && c.fspad <= 64)) fk = 1;
  } else if (fk >= 4) {
    if (!i8cap) fk = 1;
    else if ((fk == 7 || fk == 8) && !c.i8o_ok) return -1;
    else if (fk >= 10 && !(c.i8o_ok && c.i8l_ok)) return -1;
  }
  const bool l2 = fk >= 10 && fk != 15, nat = fk >= 4 && fk <= 8;
  *bound = l2 ? bnd(kFxLog2) : nat ? bnd(kFxNatural) : 0.0;
  return fk;
}

// what launch_score_factored did with a resolved fk
struct Launch {
  FactFamily family;
  int waves, tiles, occ, pairs;
  bool round1, split, skip_prep;
  int bound_kind;
};

static Launch launch(int fk, bool is_auto, int batch) {
  const bool win = fk == 9 || fk == 15;
  const bool wide = fk == 18 || fk == 19;
  const bool l2 = fk >= 10 && fk != 15 && !wide;
  const bool i8o = fk == 7 || fk == 8 || l2;
  const bool i8 = fk >= 4 && fk <= 6;
  const bool pipe = fk == 2 || fk == 3;
  Launch L{FactFamily::kChunked, -1, -1, -1, -1, false, false, false, kFxNone};
  L.skip_prep = !(!i8 && !i8o && !win && !wide);
  L.bound_kind = (fk >= 10 && fk != 15) ? kFxLog2 : (fk >= 4 && fk <= 8) ? kFxNatural : kFxNone;
  if (win) {
    L.family = FactFamily::kWindow;
    L.round1 = fk == 15;
  } else if (wide) {
    L.family = FactFamily::kI8w;
    L.tiles = fk == 18 ? 2 : 1;
  } else if (i8o) {
    const int waves = fk == 20 ? -20 : fk == 17 ? -3 : fk == 13 ? 0 : fk == 14 ? -8 : fk == 16 ? 8 : fk == 12 ? 16
                    : (fk == 7 || fk == 11) ? 4 : fk == 10 ? -2 : 8;
    // launch_score_i8o's decoding: launch_i8s_t / launch_i8p_t, launch_i8l_t<NR, WAVES, OCC, TT, SPLIT>
    // (defaults NEMO_I8O_WAVES_PER_SIMD, 1, false), launch_i8o_t<NR, WAVES, DIAG>
    const int d = NEMO_I8O_WAVES_PER_SIMD, o2 = NEMO_I8L2_OCC;
    if (l2) {
      if (waves == 0) L.family = FactFamily::kI8s;
      else if (waves == 16) L = Launch{FactFamily::kI8l, 16, 1, d, -1, false, false, L.skip_prep, L.bound_kind};
      else if (waves == -3) L.family = FactFamily::kI8p;
      else if (waves == 8) L = Launch{FactFamily::kI8l, 8, 1, d, -1, false, false, L.skip_prep, L.bound_kind};
      else if (waves == -8) L = Launch{FactFamily::kI8l, 8, 1, 6, -1, false, false, L.skip_prep, L.bound_kind};
      else if (waves == -2) L = Launch{FactFamily::kI8l, 8, 2, o2, -1, false, false, L.skip_prep, L.bound_kind};
      else if (waves == -20) L = Launch{FactFamily::kI8l, 8, 2, o2, -1, false, true, L.skip_prep, L.bound_kind};
      else L = Launch{FactFamily::kI8l, 4, 1, d, -1, false, false, L.skip_prep, L.bound_kind};
    } else {
      L.family = FactFamily::kI8o;
      L.waves = waves == 8 ? 8 : 4;
    }
  } else if (i8) {
    L.family = FactFamily::kI8;
    L.waves = fk == 6 ? 8 : (fk == 4 && is_auto && batch < 384 ? 8 : 4);
    L.pairs = fk == 5 ? 5 : 4;
  } else if (pipe) {
    L.family = FactFamily::kPipe;
    L.waves = fk == 3 ? 8 : 4;
  }
  return L;
}
}  // namespace spec

static void check_fact_kernels() {
  CHECK(kFactKernelMax == 20);
  const int sizes[] = {2, 16, 17, 64, 65, 128, 129, 256};
  const double bounds[3][2] = {{1e-9, 1e-8}, {1e-6, 1e-8}, {1e-6, 1e-5}};  // (log2, natural) against a budget of 1e-7
  for (int S : sizes)
    for (int flags = 0; flags < 32; ++flags)
      for (const auto& bd : bounds) {
        const int E = 2000;
        const FactModel m{S, E, nemo::factored_spad(S), (E + 63) / 64, (flags & 1) != 0, (flags & 2) != 0,
                          (flags & 4) != 0, (flags & 8) != 0, (flags & 16) != 0, bd[0], bd[1], 1e-7};
        for (int cap : {0, 1, 6, 7, S - 2, S - 1, S})
          for (int ll_only = 0; ll_only < 2; ++ll_only)
            for (int option = 0; option <= kFactKernelMax; ++option)
              for (int batch : {1, 383, 384}) {
                if (cap < 0) continue;
                double sb = 0.0;
                const int sfk = spec::resolve(m, option, cap, ll_only != 0, &sb);
                const FactChoice ch = resolve_fact(m, option, cap, ll_only != 0, batch);
                CHECK(ch.fk == sfk);
                if (sfk < 0) continue;
                const FactKernel& k = ch.k;
                const spec::Launch L = spec::launch(sfk, option == 0, batch);
                CHECK(k.family == L.family && k.self_prep == L.skip_prep);
                CHECK((int)k.bound == L.bound_kind && fact_bound(k, m) == sb);
                CHECK(k.split == L.split && k.round1 == L.round1);
                // the fields each family's launcher reads
                switch (k.family) {
                  case FactFamily::kI8l: CHECK(k.waves == L.waves && k.tiles == L.tiles && k.occ == L.occ); break;
                  case FactFamily::kI8: CHECK(k.waves == L.waves && k.pairs == L.pairs); break;
                  case FactFamily::kI8o:
                  case FactFamily::kPipe: CHECK(k.waves == L.waves); break;
                  case FactFamily::kI8w: CHECK(k.tiles == L.tiles); break;
                  case FactFamily::kChunked: CHECK(k.waves == spec::kFactWaves); break;
                  default: break;
                }
              }
      }
  for (int E : {1, 15, 16, 17, 127, 128, 129, 2000, 8193, 524288}) {
    const int nwords = (E + 63) / 64;
    CHECK(fact_partials_max(E) == spec::factored_partials(E));
    for (int fk = 1; fk <= kFactKernelMax; ++fk) {
      CHECK(fact_partials(kFactKernels[fk], E, nwords) == spec::score_partials(E, nwords, fk));
      CHECK(fact_partials(kFactKernels[fk], E, nwords) <= fact_partials_max(E));
    }
    // auto's small-batch form of 4 (8 waves) writes 4's partials
    const FactModel m{64, E, 64, nwords, true, false, false, false, false, 1.0, 0.0, 1e-7};
    const FactChoice ch = resolve_fact(m, 0, 0, true, 1);
    CHECK(ch.fk == 4 && ch.k.waves == 8 && fact_partials(ch.k, E, nwords) == spec::score_partials(E, nwords, 4));
  }
  // only the split variant needs the prep image
  for (int fk = 0; fk <= kFactKernelMax; ++fk) CHECK(kFactKernels[fk].split == (fk == 20));
}

int main() {
  std::mt19937_64 rng(20261017);
  check_pos_rows();
  check_staging(rng);
  check_bounds(rng);
  check_inverse_schedule(rng);
  check_step_queue(rng);
  check_sum_partials(rng);
  check_fact_kernels();
  printf("ok %d\n", g_checks);
  return 0;
}
