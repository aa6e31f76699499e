// nemo_realscore.hip -- the pair solves of NEM.compute_real_score (nem.py:
// 112-125) on the GPU: the L-BFGS-B fit of the true graph's parent weights
// the reference runs twice per model as its yardstick.
//
// One sweep (nem.py:113-121): the order score and the order weights ow
// [S+1][E] at the current weights, then for every permissible pair (child i,
// parent j), with v = exp(T[i][j]) [E] and w = the pair's weight,
//     a = (v - 1) * ow          -- the WHOLE (S+1, E) matrix, v broadcast over
//                                  the rows (nem.py:117), not row i or j
//     b = 1 - w a + w (v - 1)
//     c = a / b
//     minimize(-sum log(c x + 1), x0 = 0.5, bounds [(0, 1)], L-BFGS-B, tol 0.1)
// with no jac: scipy's bound-aware forward difference, step 1e-8.  The pairs
// are independent (each reads the sweep's ow and its own w).
//
// The objective sums (S+1) E logs, so it streams ow (the context's d_ow, left
// by the fp64 forward; shared by all pairs of a problem, it stays in L2)
// instead of holding c in registers as the one-row objectives of
// nemo_methods.hip do: E is bounded only by what the context stages.
//
// Algebra.  With B = 1 + w (v - 1) (> 0 on [0, 1]) and u = a / B:
//     b = B (1 - w u),  b + x a = B (1 + (x - w) u)
//     log(c x + 1) = log(1 + (x - w) u) - log(1 - w u)
// u = alpha * ow with alpha = (v - 1) / B per effect -- one division per effect
// (two per pair for a factored model: alpha takes the values of lo_j and
// hi_j), none per element -- kept in a register across the S + 1 rows.  The
// second term does not depend on x: L0 = sum log(1 - w u) is taken once per
// pair.  An evaluation costs one fma and one log per element and point.  The
// arguments are 1 + (small), rounded as the reference's c x + 1.0 is, so the
// difference f(x + h) - f(x) carries the same kind of error as its own
// (a form with log(b + x a) would round at |log B| instead).
//
// Sums: lane t of the block takes e = t, t + 256, ..., all rows of an effect
// in row order; the wave sum is the fixed DPP tree, the four waves are added
// in wave order through LDS, and every lane reads the totals back: the
// optimiser's control is the same in all waves.  No atomics: a pair's bits
// depend on the staged model, the order and the weights alone.
#include "nemo_internal.h"
#include "lbfgsb1.h"

#include <math.h>

namespace nemo {

namespace {

constexpr int kRealWaves = 4;
constexpr int kRealThreads = kRealWaves * kWave;

// the table log where it is defined, else the library log
__device__ __forceinline__ double log_real(double t, const double2* ltab) {
  return (t >= 2.2250738585072014e-308 && t < __builtin_inf()) ? log_fast(t, ltab) : log(t);
}

template <bool FACT>
struct RealObjective {
  const double* owb;      // the problem's order weights [rows][E]
  const double* vrow;     // !FACT: exp(T[i][j]) [E]
  const uint64_t* bits;   // FACT: parent j's D1 bits
  double a_lo, a_hi;      // FACT: alpha of lo_j / hi_j
  double w, L0;
  int rows, E;
  const double2* ltab;
  double* red;            // LDS [2 * kRealWaves]

  __device__ __forceinline__ double alpha(int e) const {
#pragma clang fp contract(off)
    if (FACT) return ((bits[e >> 6] >> (e & 63)) & 1ull) ? a_hi : a_lo;
    const double vm1 = vrow[e] - 1.0;
    return vm1 / (1.0 + w * vm1);
  }

  // sum over all elements of log(1 + d0 u) (and of log(1 + d1 u) with TWO),
  // identical in every lane of the block
  template <bool TWO>
  __device__ __forceinline__ void sums(double d0, double d1, double& s0, double& s1) const {
    double p0 = 0.0, p1 = 0.0;
    for (int e = threadIdx.x; e < E; e += kRealThreads) {
      const double al = alpha(e);
      const double* col = owb + e;
#pragma unroll 4
      for (int r = 0; r < rows; ++r) {
        const double u = al * col[(size_t)r * E];
        p0 += log_real(fma(d0, u, 1.0), ltab);
        if (TWO) p1 += log_real(fma(d1, u, 1.0), ltab);
      }
    }
    p0 = wsum_dpp(p0);
    if (TWO) p1 = wsum_dpp(p1);
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    if (lane == 0) {
      red[wv] = p0;
      if (TWO) red[kRealWaves + wv] = p1;
    }
    __syncthreads();
    s0 = ((red[0] + red[1]) + red[2]) + red[3];
    s1 = TWO ? ((red[kRealWaves] + red[kRealWaves + 1]) + red[kRealWaves + 2]) + red[kRealWaves + 3] : 0.0;
    __syncthreads();  // red is free for the next evaluation
  }

  __device__ __forceinline__ void operator()(double x, double x1, double& f0, double& f1) const {
    double s0, s1;
    sums<true>(x - w, x1 - w, s0, s1);
    f0 = -(s0 - L0);
    f1 = -(s1 - L0);
  }
};

__device__ __forceinline__ int32_t pack_info_r(const LbfgsResult& r) {
  const int nit = r.nit < 4095 ? r.nit : 4095;
  const int nfev = r.nfev < 32767 ? r.nfev : 32767;
  return (int32_t)(r.status | (nit << 4) | (nfev << 16));
}

// grid = nprob * npairs, one block per (problem, permissible pair)
template <bool FACT>
__global__ __launch_bounds__(kRealThreads) void real_pairs_kernel(
    int S, int E, int npairs, const int32_t* __restrict__ pairs, const double* __restrict__ w,
    const double* __restrict__ ow, const uint64_t* __restrict__ D1w, int nwords, const double* __restrict__ e_lo,
    const double* __restrict__ e_hi, const double* __restrict__ eT, double* __restrict__ wout,
    int32_t* __restrict__ info) {
  __shared__ double2 ltab[128];
  __shared__ double red[2 * kRealWaves];
  fill_log_table(ltab, threadIdx.x, blockDim.x);
  __syncthreads();
  const int b = blockIdx.x / npairs;
  const int n = blockIdx.x - b * npairs;
  const int pk = pairs[(size_t)b * S * S + n];
  const int i = pk >> 16;
  const int j = pk & 0xffff;  // the parent node (prep_child_list)
  const size_t idx = ((size_t)b * S + i) * S + j;
  RealObjective<FACT> obj;
  obj.owb = ow + (size_t)b * (S + 1) * E;
  obj.w = w[idx];
  obj.rows = S + 1;
  obj.E = E;
  obj.ltab = ltab;
  obj.red = red;
  obj.L0 = 0.0;
  if (FACT) {
#pragma clang fp contract(off)
    obj.vrow = nullptr;
    obj.bits = D1w + (size_t)j * nwords;
    const double lo1 = e_lo[j] - 1.0, hi1 = e_hi[j] - 1.0;
    obj.a_lo = lo1 / (1.0 + obj.w * lo1);
    obj.a_hi = hi1 / (1.0 + obj.w * hi1);
  } else {
    obj.vrow = eT + ((size_t)i * S + j) * E;
    obj.bits = nullptr;
    obj.a_lo = obj.a_hi = 0.0;
  }
  double l0, unused;
  obj.template sums<false>(-obj.w, 0.0, l0, unused);
  obj.L0 = l0;
  LbOpts o;  // minimize(..., bounds=[(0, 1)], tol=0.1): ftol = gtol = 0.1, eps 1e-8
  o.ftol = 0.1;
  o.gtol = 0.1;
  o.lo = 0.0;
  o.hi = 1.0;
  const LbfgsResult r = lbfgsb1_minimize_opts<true, false>(obj, 0.5, o);  // x0 = 0.5 always (nem.py:120)
  if (threadIdx.x == 0) {
    wout[idx] = r.x;
    info[idx] = pack_info_r(r);
  }
}

}  // namespace

hipError_t launch_real_pairs(Ctx& c, int nprob, int npairs, bool factored, const int32_t* d_pairs,
                             const double* d_w, const double* d_ow, double* d_wout, int32_t* d_info,
                             hipStream_t st) {
  if (c.dtype != 0) return hipErrorInvalidValue;
  if (nprob * (size_t)npairs == 0) return hipSuccess;
  hipEvent_t e0 = nullptr, e1 = nullptr;  // (option timing_kernel 2)
  if (c.timing && c.timing_kernel == 2 && c.ev_used + 2 <= c.ev_pool.size()) {
    e0 = c.ev_pool[c.ev_used++];
    e1 = c.ev_pool[c.ev_used++];
    const hipError_t re = hipEventRecord(e0, st);
    if (re != hipSuccess) return re;
  }
  const dim3 grid((unsigned)(nprob * (size_t)npairs));
  if (factored)
    real_pairs_kernel<true><<<grid, kRealThreads, 0, st>>>(c.S, c.E, npairs, d_pairs, d_w, d_ow, c.d_D1w, c.nwords,
                                                           c.d_elo, c.d_ehi, nullptr, d_wout, d_info);
  else
    real_pairs_kernel<false><<<grid, kRealThreads, 0, st>>>(c.S, c.E, npairs, d_pairs, d_w, d_ow, nullptr, 0,
                                                            nullptr, nullptr, (const double*)c.d_eT, d_wout, d_info);
  if (e1) {
    const hipError_t re = hipEventRecord(e1, st);
    if (re != hipSuccess) return re;
    ++c.launches;
  }
  return hipGetLastError();
}

}  // namespace nemo
