// nemo_fact_kernels.h -- what each value of the option "fact_kernel" means:
// one row per factored score-kernel variant, the resolver that picks a row
// for a call (auto's preference order included) and the partial count of a
// row.  Host-only and header-only (no HIP), so tests/host/host_check.cpp
// checks every decision on the CPU.  The launchers (nemo_factored.hip,
// nemo_factored_i8.hip) dispatch on a row's fields, nemo_abi.cpp takes the
// option's range and the image-buffer reservation from the table; nothing
// else in csrc/ compares a fact_kernel value against a number.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <utility>

namespace nemo {

constexpr int kFactWaves = 8;         // waves per chunked factored-score block (16 effects each)
constexpr int kWinMaxCap = 6;         // capped lookup-table kernel: parents per child
constexpr int kWideSetT = 2;          // 16-effect tiles per partial of score_i8w_kernel
// tiles per wave of the pipelined kernel: fixed, so the tile -> wave ->
// partial assignment (hence every bit of ll) does not depend on the batch
constexpr int kPipeTilesPerWave = 8;

// S rounded up to the factored kernels' MFMA row blocking (-1: S > 256)
inline int factored_spad(int S) {
  const int nr = (S + 15) / 16;
  const int sizes[] = {1, 2, 4, 8, 16};
  for (int v : sizes)
    if (nr <= v) return v * 16;
  return -1;
}

// waves per SIMD the offset / log2 int8 kernels are compiled for
#ifndef NEMO_I8O_WAVES_PER_SIMD
#define NEMO_I8O_WAVES_PER_SIMD 4
#endif
#ifndef NEMO_I8L2_OCC  // ... and the two-tile log2 kernel
#define NEMO_I8L2_OCC 4
#endif

namespace host {

enum FixedPointKind { kFxLog2 = 0, kFxNatural = 1, kFxNone = 2 };  // (fixed_point_bound, nemo_host.h)

enum class FactFamily : uint8_t { kChunked, kPipe, kI8, kI8o, kI8l, kI8s, kI8p, kI8w, kWindow };

// what a variant needs from the call and the staged model
enum FactNeed : unsigned {
  kNeedLl = 1u << 0,       // no cs / cells / order-weight outputs
  kNeedSpad64 = 1u << 1,   // fspad <= 64
  kNeedSpad128 = 1u << 2,  // fspad == 128
  kNeedB8 = 1u << 3,       // d_B8 staged
  kNeedI8o = 1u << 4,      // i8o_ok
  kNeedI8l = 1u << 5,      // i8l_ok
  kNeedI8w = 1u << 6,      // i8w_ok
  kNeedWin = 1u << 7,      // win_ok and 1 <= cap <= kWinMaxCap
};
constexpr unsigned kNeedInt8 = kNeedLl | kNeedSpad64 | kNeedB8;  // "int8-capable"

// partials per evaluation (nt = ceil(E / 16) tiles)
enum class FactPartials : uint8_t {
  kChunkWave,  // ceil(E / (16 waves)) * waves           launch_fact_w
  kPipeWave,   // ceil(nt / (kPipeTilesPerWave waves)) * waves   launch_pipe_t
  kSet8,       // ceil(nt / 8)                            launch_i8_t / i8o_t / i8l_t / i8s_t / i8p_t
  kWideSet,    // ceil(nt / kWideSetT)                    launch_i8w_t
  kWord,       // nwords                                  launch_score_window
};

struct FactKernel {
  FactFamily family;
  int waves;           // per block
  int tiles;           // effect tiles per iteration
  int occ;             // waves per SIMD the instantiation is compiled for (0: the family has one build)
  int pairs;           // digit pairs (kI8)
  bool round1;         // kWindow: the round-1 form
  bool split;          // a prep-only then a walk-only launch: needs the prep image (i8img_reserve)
  FixedPointKind bound;
  bool self_prep;      // derives its inputs itself: no prep_factored_kernel
  unsigned soft;       // needs that, unmet, send the call to the chunked kernel (1)
  unsigned hard;       // needs that, unmet (the soft ones met), refuse the call (-1)
  FactPartials partials;
  const char* what;
};

constexpr int kOccI8o = NEMO_I8O_WAVES_PER_SIMD, kOccI8l2 = NEMO_I8L2_OCC;
constexpr unsigned kNeedLog2 = kNeedI8o | kNeedI8l;
#define NEMO_FK_I8L(FAM, WV, TT, OCC, SPLIT, WHAT) \
  {FactFamily::FAM, WV, TT, OCC, 0, false, SPLIT, kFxLog2, true, kNeedInt8, kNeedLog2, FactPartials::kSet8, WHAT}
#define NEMO_FK_I8(WV, PAIRS, WHAT) \
  {FactFamily::kI8, WV, 1, 0, PAIRS, false, false, kFxNatural, true, kNeedInt8, 0, FactPartials::kSet8, WHAT}

// index = the option's value; row 0 stands for auto (resolve_fact)
constexpr FactKernel kFactKernels[] = {
    // family, waves, tiles, occ, pairs, round1, split, bound, self_prep, soft, hard, partials
    {FactFamily::kChunked, kFactWaves, 1, 0, 0, false, false, kFxNone, false, 0, 0, FactPartials::kChunkWave,
     "auto: the fastest variant that serves the call within err_budget"},
    {FactFamily::kChunked, kFactWaves, 1, 0, 0, false, false, kFxNone, false, 0, 0, FactPartials::kChunkWave,
     "chunked fp64: any call (cs / cells / order weights too)"},
    {FactFamily::kPipe, 4, 1, 0, 0, false, false, kFxNone, false, kNeedLl | kNeedSpad64, 0, FactPartials::kPipeWave,
     "fp64 pipelined, 4 waves"},
    {FactFamily::kPipe, 8, 1, 0, 0, false, false, kFxNone, false, kNeedLl | kNeedSpad64, 0, FactPartials::kPipeWave,
     "fp64 pipelined, 8 waves"},
    NEMO_FK_I8(4, 4, "int8, max offset, 4 digit pairs, 4 waves (auto's pick: 8 waves below batch 384)"),
    NEMO_FK_I8(4, 5, "int8, max offset, 5 digit pairs, 4 waves"),
    NEMO_FK_I8(8, 4, "int8, max offset, 4 digit pairs, 8 waves"),
    {FactFamily::kI8o, 4, 1, kOccI8o, 0, false, false, kFxNatural, true, kNeedInt8, kNeedI8o, FactPartials::kSet8,
     "int8, offset log-sum-exp, 4 waves"},
    {FactFamily::kI8o, 8, 1, kOccI8o, 0, false, false, kFxNatural, true, kNeedInt8, kNeedI8o, FactPartials::kSet8,
     "int8, offset log-sum-exp, 8 waves"},
    {FactFamily::kWindow, 0, 0, 0, 0, false, false, kFxNone, true, 0, kNeedLl | kNeedWin, FactPartials::kWord,
     "capped lookup tables"},
    NEMO_FK_I8L(kI8l, 8, 2, kOccI8l2, false, "log2 fixed point, 8 waves, two tiles per iteration (auto's pick)"),
    NEMO_FK_I8L(kI8l, 4, 1, kOccI8o, false, "log2 fixed point, 4 waves"),
    NEMO_FK_I8L(kI8l, 16, 1, kOccI8o, false, "log2 fixed point, 16 waves"),
    NEMO_FK_I8L(kI8s, 8, 1, kOccI8o, false, "log2 fixed point, register-stationary"),
    NEMO_FK_I8L(kI8l, 8, 1, 6, false, "log2 fixed point, 8 waves compiled for 6 waves per SIMD"),
    {FactFamily::kWindow, 0, 0, 0, 0, true, false, kFxNone, true, 0, kNeedLl | kNeedWin, FactPartials::kWord,
     "capped lookup tables, round-1 form (row bits re-read from LDS)"},
    NEMO_FK_I8L(kI8l, 8, 1, kOccI8o, false, "log2 fixed point, 8 waves, one tile per iteration"),
    NEMO_FK_I8L(kI8p, 8, 2, kOccI8l2, false,
                "log2 fixed point, persistent blocks (grid min(batch, 3 CUs)) that prep the next evaluation"),
    {FactFamily::kI8w, 16, 2, kOccI8o, 0, false, false, kFxLog2, true, kNeedLl | kNeedSpad128, kNeedI8w | kNeedB8,
     FactPartials::kWideSet, "log2 fixed point for 64 < S <= 128, two tiles per iteration (auto's pick there)"},
    {FactFamily::kI8w, 16, 1, kOccI8o, 0, false, false, kFxLog2, true, kNeedLl | kNeedSpad128, kNeedI8w | kNeedB8,
     FactPartials::kWideSet, "log2 fixed point for 64 < S <= 128, one tile per iteration"},
    NEMO_FK_I8L(kI8l, 8, 2, kOccI8l2, true, "10 as a prep-only launch then a walk-only launch"),
};
#undef NEMO_FK_I8L
#undef NEMO_FK_I8
constexpr int kFactKernelMax = (int)(sizeof(kFactKernels) / sizeof(kFactKernels[0])) - 1;

// the staged model as the resolver sees it (filled from Ctx by fact_model in
// nemo_factored.hip); the bounds are those of the call's cap
struct FactModel {
  int S, E, fspad, nwords;
  bool b8, i8o_ok, i8l_ok, i8w_ok, win_ok;
  double bound_log2, bound_natural, err_budget;
};

// a parent cap that cuts nothing is no cap (same lists, same bits)
inline int fact_effective_cap(int S, int cap) { return cap >= S - 1 ? 0 : cap; }

// the needs this call on this model meets
inline unsigned fact_have(const FactModel& m, int cap, bool ll_only) {
  cap = fact_effective_cap(m.S, cap);
  return (ll_only ? kNeedLl : 0u) | (m.fspad <= 64 ? kNeedSpad64 : 0u) | (m.fspad == 128 ? kNeedSpad128 : 0u) |
         (m.b8 ? kNeedB8 : 0u) | (m.i8o_ok ? kNeedI8o : 0u) | (m.i8l_ok ? kNeedI8l : 0u) |
         (m.i8w_ok ? kNeedI8w : 0u) | (m.win_ok && cap >= 1 && cap <= kWinMaxCap ? kNeedWin : 0u);
}

// 0: row k serves the call; 1: the chunked kernel runs in its place; -1: refused
inline int fact_unmet(const FactKernel& k, unsigned have) {
  return (k.soft & ~have) ? 1 : (k.hard & ~have) ? -1 : 0;
}

inline double fact_bound(const FactKernel& k, const FactModel& m) {
  return k.bound == kFxLog2 ? m.bound_log2 : k.bound == kFxNatural ? m.bound_natural : 0.0;
}

// what a call runs: fk = the resolved option value (-1: the requested variant
// cannot serve the call) and its row, with anything the resolver adjusts
struct FactChoice {
  int fk;
  FactKernel k;
};

// the variant of a factored call: the option's row if it serves the call
// (else chunked or refused, as the row says); for auto (option 0) the capped
// lookup-table kernel for capped calls, else the fastest int8 kernel whose
// worst-case |ll error| stays within err_budget -- log2 fixed point (10; 18
// for S > 64), natural units (8; 4 where the offset form is not staged) --
// else the fp64 MFMA kernels
inline FactChoice resolve_fact(const FactModel& m, int option, int cap, bool ll_only, int batch) {
  const unsigned have = fact_have(m, cap, ll_only);
  auto ok = [&](int fk) { return fact_unmet(kFactKernels[fk], have) == 0; };
  auto within = [&](int fk) { return fact_bound(kFactKernels[fk], m) <= m.err_budget; };
  int fk = option;
  if (option == 0) {
    if (ok(9)) fk = 9;
    else if (ok(18) && within(18)) fk = 18;
    else if (!ok(4)) fk = 1;  // not int8-capable
    else if (ok(10) && within(10)) fk = 10;
    else if (ok(8) && within(8)) fk = 8;
    else if (within(4)) fk = 4;  // (8's bound too: taken only where 8 is not staged)
    else fk = 2;
  } else {
    const int u = fact_unmet(kFactKernels[fk], have);
    if (u) fk = u > 0 ? 1 : -1;
  }
  FactChoice ch{fk, kFactKernels[fk < 0 ? 0 : fk]};
  // auto's int8 pick: 4 waves per block for large batches, 8 (fewer splits) below
  if (option == 0 && fk == 4 && batch < 384) ch.k.waves = 8;
  return ch;
}

inline int fact_partials(const FactKernel& k, int E, int nwords) {
  const int nt = (E + 15) / 16;
  auto ceil_div = [](int a, int b) { return (a + b - 1) / b; };
  switch (k.partials) {
    case FactPartials::kWord: return nwords;
    case FactPartials::kWideSet: return ceil_div(nt, kWideSetT);
    case FactPartials::kSet8: return ceil_div(nt, 8);
    case FactPartials::kPipeWave: return ceil_div(nt, kPipeTilesPerWave * k.waves) * k.waves;
    case FactPartials::kChunkWave: break;
  }
  return ceil_div(E, 16 * k.waves) * k.waves;
}

// partials per evaluation every partial buffer holds: the largest count of
// any row (one lookup-table partial per 64-effect word); unrolled over the
// rows, so each row's rule and wave count are constants where it is compiled
template <size_t... I>
inline int fact_partials_max(int E, std::index_sequence<I...>) {
  int n = 0;
  for (int nk : {fact_partials(kFactKernels[I], E, (E + 63) / 64)...}) n = nk > n ? nk : n;
  return n;
}
inline int fact_partials_max(int E) { return fact_partials_max(E, std::make_index_sequence<kFactKernelMax + 1>{}); }

}  // namespace host
}  // namespace nemo
