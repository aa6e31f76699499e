// nemo_sweep.hip -- one sequential sweep over the single-weight moves of an
// order: every permissible pair is visited once, its move is scored at the
// CURRENT state and taken when the gain clears the pair's threshold.
//
// With x_e = ow[i][e] kappa_ij(e) and t_e = log1p(x_e) (nemo_moves.hip), taking
// move (i, j) changes the state exactly:
//     cs[e]    += t_e
//     ow[i][e] *= (1 + kappa_ij(e)) / (1 + x_e),   1 + kappa = f_ij(w') / f_ij(w)
//     ow[k][e] /= (1 + x_e) = exp(-t_e)            (every other row)
// A sweep takes the children by order position and visits each once, so one
// number per effect is enough: c[e], the change of cs[e] so far.  When child
// i's turn comes its row is ow0[i][e] exp(-c[e]) (ow0: the forward's order
// weights), and it is kept current across the child's own parents.  The swept
// weights score ll0 + sum_e c[e].
//
// One block per evaluation; the block size follows from E alone.  Thread tid
// owns the effects tid, tid + T, ... (NPT of them) for the whole sweep: c, the
// current child's row and the pair's t_e live in its registers.  Per pair: one
// log1p per owned effect summed in ascending effect order, the wave's sum
// (wsum_dpp, all VALU), the waves' partials through double-buffered LDS slots
// (one barrier per pair), and every thread adds the partials in wave order and
// takes the same decision from the same bits.  The next pair's operands are
// loaded before the current pair's barrier.  Every trip count follows from S,
// E and cap: the kernel waits on nothing but its own barriers.
//
// Every sum has a fixed order that depends on the staged model alone.
#include "nemo_grad_fwd.h"
#include "nemo_internal.h"

#include <math.h>

namespace nemo {

namespace {

constexpr int kSweepMaxThreads = 1024;
constexpr int kSweepMaxWaves = kSweepMaxThreads / kWave;
constexpr int kSweepMaxNpt = kSweepMaxE / kSweepMaxThreads;
static_assert(kSweepMaxNpt * kSweepMaxThreads == kSweepMaxE, "the bound on E is whole effects per thread");

// From kSweepLeanNpt effects per thread on, the registers hold c and the
// child's row alone: the pair's D1 words / exp(T) are read where they are used
// and t_e is formed again on acceptance (the same operations on the same
// operands).  Below it they are loaded one pair ahead and t_e is kept.
constexpr int kSweepLeanNpt = 8;

// what a pair's visit reads, loaded one pair ahead
template <bool FACT, int NPT>
struct SweepPair {
  static constexpr int NH = NPT >= kSweepLeanNpt ? 1 : NPT;
  int i, j;
  double w, wa, thr;
  uint64_t word[FACT ? NH : 1];  // the parent's D1 words of the owned effects
  double v[FACT ? 1 : NH];       // the staged exp(T) of the owned effects
};

template <bool FACT, int NPT>
__device__ __forceinline__ void sweep_load(SweepPair<FACT, NPT>& pr, int S, int E, int T, int tid, int i, int j,
                                           const double* w01, const double* walt, const double* thr,
                                           const uint64_t* __restrict__ D1w, int nwords,
                                           const double* __restrict__ eT) {
  const size_t o = (size_t)i * S + j;
  pr.i = i;
  pr.j = j;
  pr.w = w01[o];
  pr.wa = walt[o];
  pr.thr = thr[o];
  if (NPT < kSweepLeanNpt) {
#pragma unroll
    for (int k = 0; k < SweepPair<FACT, NPT>::NH; ++k) {
      const int e = min(tid + k * T, E - 1);
      if (FACT)
        pr.word[k] = D1w[(size_t)j * nwords + (e >> 6)];
      else
        pr.v[k] = eT[o * E + e];
    }
  }
}

// grid = batch, block = T (a multiple of 64 that depends on E alone)
template <bool FACT, int NPT>
__global__ __launch_bounds__(kSweepMaxThreads) void edge_sweep_kernel(
    int S, int E, int cap, const int32_t* __restrict__ pos, const double* w01, const double* walt,
    const double* __restrict__ thr, const double* __restrict__ ow, const uint64_t* __restrict__ D1w, int nwords,
    const double* __restrict__ e_lo, const double* __restrict__ e_hi, const double* __restrict__ eT,
    const double* __restrict__ ll0, double* w_out, double* alt_out, double* __restrict__ ll_out,
    double* __restrict__ gain_out, int32_t* __restrict__ nacc_out) {
  __shared__ double2 ltab[128];
  __shared__ int perm[kMaxS];
  __shared__ double red[2][kSweepMaxWaves];
  const int T = blockDim.x, tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave), nw = T / kWave;
  const int b = blockIdx.x;
  const size_t SS = (size_t)S * S;
  const int32_t* pb = pos + (size_t)b * S;
  w01 += b * SS;
  walt += b * SS;
  thr += b * SS;
  w_out += b * SS;
  alt_out += b * SS;
  if (gain_out) gain_out += b * SS;
  const double* owb = ow + (size_t)b * (S + 1) * E;

  fill_log_table(ltab, tid, T);
  for (int i = tid; i < S; i += T) perm[i] = 0;
  __syncthreads();
  for (int i = tid; i < S; i += T) perm[clamp_pos(pb[i], S)] = i;
  // off the permissible pairs: the inputs' bits carried through, +0.0 gains
  // (each permissible pair is written at its visit, so no entry is written twice)
  for (int k = tid; k < (int)SS; k += T) {
    const int i = k / S, j = k - i * S;
    const int q = clamp_pos(pb[i], S), p = clamp_pos(pb[j], S);
    if (p < q && (cap == 0 || q - p <= cap)) continue;
    if (w_out != w01) {
      const uint64_t* s = reinterpret_cast<const uint64_t*>(w01);
      reinterpret_cast<uint64_t*>(w_out)[k] = s[k];
    }
    if (alt_out != walt) {
      const uint64_t* s = reinterpret_cast<const uint64_t*>(walt);
      reinterpret_cast<uint64_t*>(alt_out)[k] = s[k];
    }
    if (gain_out) gain_out[k] = 0.0;
  }
  __syncthreads();

  constexpr bool LEAN = NPT >= kSweepLeanNpt;
  constexpr int NH = SweepPair<FACT, NPT>::NH;
  double c[NPT], owc[NPT], t[NH];
  bool own[NPT];
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    c[k] = 0.0;
    owc[k] = 0.0;
    own[k] = tid + k * T < E;
  }
#pragma unroll
  for (int k = 0; k < NH; ++k) t[k] = 0.0;
  int nacc = 0, buf = 0;

  // the visits in order: child position q = 1 .. S - 1, parent position p ascending
  int q = 1, p = (cap > 0 && q > cap) ? q - cap : 0;
  SweepPair<FACT, NPT> cur, nxt;
  sweep_load<FACT, NPT>(cur, S, E, T, tid, perm[q], perm[p], w01, walt, thr, D1w, nwords, eT);
  bool first = true;  // the first parent of a child: its row is formed
  while (q < S) {
    // the next visit and its operands
    int q2 = q, p2 = p + 1;
    if (p2 >= q) {
      ++q2;
      p2 = (cap > 0 && q2 > cap) ? q2 - cap : 0;
    }
    if (q2 < S) sweep_load<FACT, NPT>(nxt, S, E, T, tid, perm[q2], perm[p2], w01, walt, thr, D1w, nwords, eT);

    const int i = cur.i, j = cur.j;
    if (first) {
      const double* orow = owb + (size_t)i * E;
#pragma unroll
      for (int k = 0; k < NPT; ++k) owc[k] = own[k] ? orow[tid + k * T] * exp(-c[k]) : 0.0;
    }
    const double w = cur.w, wa = cur.wa, d = wa - w;
    double gain = 0.0;
    const bool moves = d != 0.0;  // block-uniform: a pair with w_alt == w01 takes no log1p
    double klo = 0.0, khi = 0.0, rlo = 1.0, rhi = 1.0;
    const double s1 = 1.0 - w, sa = 1.0 - wa;
    // owned effect k of this pair: kappa, and r = 1 + kappa = f(w') / f(w) without the cancellation
    auto factor = [&](int k, double& kap, double& r) {
      const int e = min(tid + k * T, E - 1);
      if (FACT) {
        const uint64_t word = LEAN ? D1w[(size_t)j * nwords + (e >> 6)] : cur.word[LEAN ? 0 : k];
        const bool hi = (word >> (uint32_t)(e & 63)) & 1ull;
        kap = hi ? khi : klo;
        r = hi ? rhi : rlo;
      } else {
        const double v = LEAN ? eT[((size_t)i * S + j) * E + e] : cur.v[LEAN ? 0 : k];
        const double f = fma(w, v, s1);
        kap = d * ((v - 1.0) / f);
        r = fma(wa, v, sa) / f;
      }
    };
    if (moves) {
      if (FACT) {
        const double vlo = e_lo[j], vhi = e_hi[j];
        const double flo = fma(w, vlo, s1), fhi = fma(w, vhi, s1);
        klo = d * ((vlo - 1.0) / flo);
        khi = d * ((vhi - 1.0) / fhi);
        rlo = fma(wa, vlo, sa) / flo;
        rhi = fma(wa, vhi, sa) / fhi;
      }
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < NPT; ++k) {
        double kap, r;
        factor(k, kap, r);
        const double tk = own[k] ? log1p_fast(owc[k] * kap, ltab) : 0.0;
        if (!LEAN) t[k] = tk;
        s += tk;
      }
      s = wsum_dpp(s);
      if (lane == 0) red[buf][wv] = s;
      __syncthreads();
      for (int ww = 0; ww < nw; ++ww) gain += red[buf][ww];
      buf ^= 1;
    }
    const bool acc = gain > cur.thr;  // (a NaN threshold never accepts)
    if (acc) ++nacc;
    if (acc && moves) {
#pragma unroll
      for (int k = 0; k < NPT; ++k) {
        double kap, r;
        factor(k, kap, r);
        c[k] += LEAN ? (own[k] ? log1p_fast(owc[k] * kap, ltab) : 0.0) : t[LEAN ? 0 : k];
        // (1 + x rounds to 0 where ow = 1 and e^T < 2^-53: log1p_fast's floor)
        owc[k] = fmin(owc[k] * r / fmax(1.0 + owc[k] * kap, 0x1p-54), 1.0);
      }
    }
    if (tid == 0) {
      const size_t o = (size_t)i * S + j;
      const uint64_t bw = __builtin_bit_cast(uint64_t, w), ba = __builtin_bit_cast(uint64_t, wa);
      reinterpret_cast<uint64_t*>(w_out)[o] = acc ? ba : bw;
      reinterpret_cast<uint64_t*>(alt_out)[o] = acc ? bw : ba;
      if (gain_out) gain_out[o] = gain;
    }
    first = q2 != q;
    q = q2;
    p = p2;
    cur = nxt;
  }

  // ll = ll0 + sum_e c[e], in the gains' order
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < NPT; ++k) s += c[k];
  s = wsum_dpp(s);
  if (lane == 0) red[buf][wv] = s;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int ww = 0; ww < nw; ++ww) tot += red[buf][ww];
    ll_out[b] = ll0[b] + tot;
    if (nacc_out) nacc_out[b] = nacc;
  }
}

template <bool FACT, int NPT>
void launch_t(Ctx& c, int batch, int cap, int T, const int32_t* d_pos, const double* d_w01, const double* d_walt,
              const double* d_thr, const double* d_ll0, double* d_wout, double* d_altout, double* d_ll,
              double* d_gain, int32_t* d_nacc, hipStream_t st) {
  edge_sweep_kernel<FACT, NPT><<<batch, T, 0, st>>>(
      c.S, c.E, cap, d_pos, d_w01, d_walt, d_thr, c.d_ow, FACT ? c.d_D1w : nullptr, FACT ? c.nwords : 0,
      FACT ? c.d_elo : nullptr, FACT ? c.d_ehi : nullptr, FACT ? nullptr : (const double*)c.d_eT, d_ll0, d_wout,
      d_altout, d_ll, d_gain, d_nacc);
}

template <bool FACT>
hipError_t launch_f(Ctx& c, int batch, int cap, const int32_t* d_pos, const double* d_w01, const double* d_walt,
                    const double* d_thr, const double* d_ll0, double* d_wout, double* d_altout, double* d_ll,
                    double* d_gain, int32_t* d_nacc, hipStream_t st) {
  const int T = sweep_threads(c.E);
  const int npt = (c.E + T - 1) / T;
#define NEMO_SWEEP_CASE(N)                                                                                    \
  launch_t<FACT, N>(c, batch, cap, T, d_pos, d_w01, d_walt, d_thr, d_ll0, d_wout, d_altout, d_ll, d_gain, d_nacc, st)
  if (npt <= 1)
    NEMO_SWEEP_CASE(1);
  else if (npt <= 2)
    NEMO_SWEEP_CASE(2);
  else if (npt <= 4)
    NEMO_SWEEP_CASE(4);
  else if (npt <= 8)
    NEMO_SWEEP_CASE(8);
  else if (npt <= kSweepMaxNpt)
    NEMO_SWEEP_CASE(16);
  else
    return hipErrorInvalidValue;
#undef NEMO_SWEEP_CASE
  return hipGetLastError();
}
static_assert(kSweepMaxNpt == 16, "the instances above end at 16 effects per thread");

}  // namespace

hipError_t launch_edge_sweep(Ctx& c, int batch, int cap, bool factored, const int32_t* d_pos, const double* d_w01,
                             const double* d_walt, const double* d_thr, const double* d_ll0, double* d_wout,
                             double* d_altout, double* d_ll, double* d_gain, int32_t* d_nacc, hipStream_t st) {
  if (c.dtype != 0 || c.E > kSweepMaxE) return hipErrorInvalidValue;
  if (cap >= c.S - 1) cap = 0;  // a cap that cuts nothing (same visits, same bits)
  return factored ? launch_f<true>(c, batch, cap, d_pos, d_w01, d_walt, d_thr, d_ll0, d_wout, d_altout, d_ll, d_gain,
                                   d_nacc, st)
                  : launch_f<false>(c, batch, cap, d_pos, d_w01, d_walt, d_thr, d_ll0, d_wout, d_altout, d_ll,
                                    d_gain, d_nacc, st);
}

}  // namespace nemo
