// nemo_order_sweep.hip -- a list of node relocations walked in sequence inside
// one launch: at each visit the visited node's S positions are scored exactly
// at the CURRENT order (nemo_reloc.hip's closed form), one position is chosen
// (a Gibbs draw from a caller-supplied uniform, or greedily) and the move is
// applied to the order and to the device-resident cells.
//
// One block per evaluation.  The block owns the evaluation's slice of the cells
// [S+1][E] and of cs [E] (the forward's scratch) as mutable state, in global
// memory; thread tid owns the effects tid + T k: only it reads and writes those
// columns, so the state needs no ordering beyond the block barriers of a visit.
// Per visit of node a at position p:
//   1. a thread per position forms the pair constants of (a, node at q);
//   2. every thread walks up and down from p for each owned effect; a step's
//      terms are summed over the wave and added to the wave's running sum of the
//      step's target position, owned chunks ascending;
//   3. r[q] = the waves' sums added in wave order, +0.0 at p;
//   4. one wave takes the decision: the exps in parallel, the prefix adds by one
//      lane in ascending q;
//   5. on a move the walk to q* is redone to apply the cell updates (each passed
//      node's cell -+log f_ma, a's cell +-log f_am step by step), cs[e] is formed
//      AFRESH as the log-sum-exp of the updated column (rows 0 .. S ascending,
//      the maximum subtracted) and the order shifts in the LDS.
// cs is not carried as cs + log(1 + X): where 1 + X has no correct fp64 digit the
// state after the move must still be as good as a forward's.
//
// Every sum has a fixed order that depends on S and E alone.
#include "nemo_grad_fwd.h"
#include "nemo_internal.h"
#include "nemo_reloc_math.h"

#include <math.h>

namespace nemo {

namespace {

#ifndef NEMO_ORDER_SWEEP_MAX_THREADS
#define NEMO_ORDER_SWEEP_MAX_THREADS 1024
#endif
constexpr int kOsMaxThreads = NEMO_ORDER_SWEEP_MAX_THREADS;
constexpr int kOsMaxWaves = kOsMaxThreads / kWave;
static_assert(kOsMaxThreads % kWave == 0 && kOsMaxThreads >= kWave && kOsMaxThreads <= 1024, "whole waves");

// the block size: the smallest power-of-two number of waves that gives every
// effect a thread, up to kOsMaxThreads (a function of E alone)
inline int order_sweep_threads(int E) {
  int t = kWave;
  while (t < kOsMaxThreads && t < E) t *= 2;
  return t;
}

// sum of v over the block in a fixed order (the wave's DPP tree, then the waves
// in order), in every thread; red: nw doubles of LDS, free before and after
__device__ __forceinline__ double block_sum(double v, double* red, int lane, int wv, int nw) {
  v = wsum_dpp(v);
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < nw; ++w) s += red[w];
  return s;
}

// grid = batch, block = T = order_sweep_threads(E)
template <bool FACT>
__global__ __launch_bounds__(kOsMaxThreads) void order_sweep_kernel(
    int S, int E, int nvisit, const int32_t* pos, const double* __restrict__ w01,
    const int32_t* __restrict__ visit, const double* __restrict__ u, double beta, double min_gain, double* cells,
    double* cs, const uint64_t* __restrict__ D1w, int nwords, const double* __restrict__ e_lo,
    const double* __restrict__ e_hi, const double* __restrict__ eT, int32_t* pos_out, double* __restrict__ ll0_out,
    double* __restrict__ ll_out, int32_t* __restrict__ q_out, double* __restrict__ dll_out,
    double* __restrict__ ll_vis_out, int32_t* __restrict__ nmoved_out) {
  __shared__ double2 ltab[128];
  __shared__ double etab[256];
  __shared__ int perm[kMaxS];        // node at each position
  __shared__ int posn[kMaxS];        // position of each node
  // by position q != p.  FACT: [0, 1] the sum's factor by a's bit, [2, 3] the signed log f_am by
  // m's bit, [4, 5] the signed log f_ma by a's bit (the passed node's cell update); else w_ma, w_am
  __shared__ double ctab[kMaxS * 6];
  __shared__ double accw[kOsMaxWaves][kMaxS];
  __shared__ double row[kMaxS];      // r[q] of the visit, then pq[q]
  __shared__ double red[kOsMaxWaves];
  __shared__ int qsel;
  const int T = blockDim.x, tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave), nw = T / kWave;
  const int b = blockIdx.x;
  const bool greedy = isinf(beta);

  fill_log_table(ltab, tid, T);
  for (int k = tid; k < 256; k += T) etab[k] = exp2((double)k * (1.0 / 256.0));
  const int32_t* pb = pos + (size_t)b * S;
  for (int i = tid; i < S; i += T) perm[i] = 0;
  __syncthreads();
  for (int i = tid; i < S; i += T) {
    const int p = clamp_pos(pb[i], S);
    posn[i] = p;
    perm[p] = i;
  }
  __syncthreads();
  // (a malformed pos: every later index comes from perm and posn made consistent here)
  for (int p = tid; p < S; p += T) posn[perm[p]] = p;
  __syncthreads();

  const double* wb = w01 + (size_t)b * S * S;
  double* cb = cells + (size_t)b * (S + 1) * E;
  double* csb = cs + (size_t)b * E;
  const int32_t* vb = visit + (size_t)b * nvisit;
  const double* ub = u ? u + (size_t)b * nvisit : nullptr;

  // the score held: sum_e cs[e], owned effects ascending, then the block's order
  double mine = 0.0;
  for (int e = tid; e < E; e += T) mine += csb[e];
  double ll = block_sum(mine, red, lane, wv, nw);
  if (tid == 0 && ll0_out) ll0_out[b] = ll;
  int nmoved = 0;

  for (int k = 0; k < nvisit; ++k) {
    const int a = clamp_pos(vb[k], S);
    const int p = posn[a];
    // ---- 1. the pair constants, a thread per position
    for (int q = tid; q < S; q += T) {
#pragma unroll
      for (int w = 0; w < kOsMaxWaves; ++w) accw[w][q] = 0.0;
      if (q == p) continue;
      const int m = perm[q];
      const bool up = q > p;
      const double w_ma = wb[(size_t)m * S + a], w_am = wb[(size_t)a * S + m];
      if (FACT) {
        const double l0 = log_factor(w_am, e_lo[m], ltab), l1 = log_factor(w_am, e_hi[m], ltab);
        const double g0 = log_factor(w_ma, e_lo[a], ltab), g1 = log_factor(w_ma, e_hi[a], ltab);
        ctab[6 * q + 0] = sum_factor(up, w_ma, e_lo[a]);
        ctab[6 * q + 1] = sum_factor(up, w_ma, e_hi[a]);
        ctab[6 * q + 2] = up ? l0 : -l0;
        ctab[6 * q + 3] = up ? l1 : -l1;
        ctab[6 * q + 4] = up ? -g0 : g0;
        ctab[6 * q + 5] = up ? -g1 : g1;
      } else {
        ctab[6 * q + 0] = w_ma;
        ctab[6 * q + 1] = w_am;
      }
    }
    __syncthreads();
    // ---- 2. the walks (nemo_reloc.hip's, at the current state)
    for (int e0 = wv * kWave; e0 < E; e0 += T) {  // wave-uniform
      const int e = e0 + lane;
      const bool valid = e < E;
      const int ec = valid ? e : E - 1;
      const double c0 = csb[ec];
      const double za = cb[(size_t)a * E + ec] - c0;
      const double owa = exp_lse(za, etab);
      int abit = 0;
      if (FACT) abit = (int)((D1w[(size_t)a * nwords + (ec >> 6)] >> (ec & 63)) & 1ull);
      for (int dir = 0; dir < 2; ++dir) {
        const bool up = dir == 0;
        const int n = up ? S - 1 - p : p;
        double sumv = -owa, y = za;
        for (int s = 1; s <= n; ++s) {
          const int q = up ? p + s : p - s;
          const int m = perm[q];
          const double owm = exp_lse(cb[(size_t)m * E + ec] - c0, etab);
          double cf, lf;
          if (FACT) {
            const int mbit = (int)((D1w[(size_t)m * nwords + (ec >> 6)] >> (ec & 63)) & 1ull);
            cf = ctab[6 * q + abit];
            lf = ctab[6 * q + 2 + mbit];
          } else {
            const double w_ma = ctab[6 * q], w_am = ctab[6 * q + 1];
            cf = sum_factor(up, w_ma, eT[((size_t)m * S + a) * E + ec]);
            lf = log_factor(w_am, eT[((size_t)a * S + m) * E + ec], ltab);
            lf = up ? lf : -lf;
          }
          sumv = fma(owm, cf, sumv);
          y += lf;
          const double term = wsum_dpp(valid ? reloc_term(sumv, y, etab, ltab) : 0.0);
          if (lane == 0) accw[wv][q] += term;
        }
      }
    }
    __syncthreads();
    // ---- 3. the row: the waves in order, +0.0 at p
    for (int q = tid; q < S; q += T) {
      double r = 0.0;
      for (int w = 0; w < nw; ++w) r += accw[w][q];
      r = q == p ? 0.0 : r;
      row[q] = r;
      if (dll_out) dll_out[((size_t)b * nvisit + k) * S + q] = r;
    }
    __syncthreads();
    // ---- 4. the decision, wave 0
    if (wv == 0) {
      bool bad = false;
      double mx = -INFINITY;
      for (int q = lane; q < S; q += kWave) {
        const double r = row[q];
        bad |= r != r;
        mx = fmax(mx, r);
      }
      bad = __any(bad);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, kWave));
      int qs = p;
      if (greedy) {
        if (lane == 0 && !bad) {
          int best = 0;
          double rb = row[0];
          for (int q = 1; q < S; ++q) {
            const double r = row[q];
            if (r > rb) {
              rb = r;
              best = q;
            }
          }
          qs = rb > min_gain ? best : p;
        }
      } else {
        // pq in place of r (the row is in dll_out already); g = beta r, the maximum of g is beta mx
        const double gmx = __dmul_rn(beta, mx);
        for (int q = lane; q < S; q += kWave) row[q] = exp(__dmul_rn(beta, row[q]) - gmx);
        // lane 0 reads what the wave's other lanes wrote: make the LDS writes visible within the wave
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0 && !bad) {
          double tot = 0.0;
          for (int q = 0; q < S; ++q) tot += row[q];
          const double thr = ub[k] * tot;
          int cnt = 0;
          double cdf = 0.0;
          for (int q = 0; q < S; ++q) {
            cdf += row[q];
            cnt += cdf < thr ? 1 : 0;
          }
          qs = tot == tot ? min(cnt, S - 1) : p;
        }
      }
      if (lane == 0) qsel = qs;
    }
    __syncthreads();
    const int qs = clamp_pos(qsel, S);
    // ---- 5. the move
    if (qs != p) {  // block-uniform
      const bool up = qs > p;
      const int n = up ? qs - p : p - qs;
      mine = 0.0;
      for (int e = tid; e < E; e += T) {
        int abit = 0;
        if (FACT) abit = (int)((D1w[(size_t)a * nwords + (e >> 6)] >> (e & 63)) & 1ull);
        double ca = cb[(size_t)a * E + e];
        for (int s = 1; s <= n; ++s) {
          const int q = up ? p + s : p - s;
          const int m = perm[q];
          double lf, lm;
          if (FACT) {
            const int mbit = (int)((D1w[(size_t)m * nwords + (e >> 6)] >> (e & 63)) & 1ull);
            lf = ctab[6 * q + 2 + mbit];
            lm = ctab[6 * q + 4 + abit];
          } else {
            const double w_ma = ctab[6 * q], w_am = ctab[6 * q + 1];
            lf = log_factor(w_am, eT[((size_t)a * S + m) * E + e], ltab);
            lm = log_factor(w_ma, eT[((size_t)m * S + a) * E + e], ltab);
            lf = up ? lf : -lf;
            lm = up ? -lm : lm;
          }
          cb[(size_t)m * E + e] += lm;
          ca += lf;
        }
        cb[(size_t)a * E + e] = ca;
        // cs[e] afresh: rows 0 .. S ascending, the maximum subtracted
        double mx = cb[e];
        for (int i = 1; i <= S; ++i) mx = fmax(mx, cb[(size_t)i * E + e]);
        double se = 0.0;
        for (int i = 0; i <= S; ++i) se += exp_lse(cb[(size_t)i * E + e] - mx, etab);
        const double c1 = mx + log_fast(se, ltab);
        csb[e] = c1;
        mine += c1;
      }
      ll = block_sum(mine, red, lane, wv, nw);
      ++nmoved;
      // the order shifts by one between p and q*
      // (every position is read before any is written: a thread holds up to kMaxS / kWave of them)
      int node[kMaxS / kWave];
#pragma unroll
      for (int c = 0; c < kMaxS / kWave; ++c) {
        const int t = tid + c * T;
        node[c] = -1;
        if (t < S) {
          const bool in = up ? (t >= p && t < qs) : (t > qs && t <= p);
          node[c] = t == qs ? a : (in ? perm[up ? t + 1 : t - 1] : perm[t]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < kMaxS / kWave; ++c) {
        const int t = tid + c * T;
        if (t < S) {
          perm[t] = node[c];
          posn[node[c]] = t;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (q_out) q_out[(size_t)b * nvisit + k] = qs;
      if (ll_vis_out) ll_vis_out[(size_t)b * nvisit + k] = ll;
    }
    __syncthreads();  // the next visit rewrites ctab, accw, row and qsel
  }

  for (int i = tid; i < S; i += T) pos_out[(size_t)b * S + i] = posn[i];
  if (tid == 0) {
    ll_out[b] = ll;
    if (nmoved_out) nmoved_out[b] = nmoved;
  }
}

// (option timing_kernel 5) the events around the sweep kernel of one call
struct OrderSweepTimer {
  Ctx& c;
  hipStream_t st;
  hipEvent_t e1 = nullptr;
  hipError_t begin() {
    if (!(c.timing && c.timing_kernel == 5 && c.ev_used + 2 <= c.ev_pool.size())) return hipSuccess;
    hipEvent_t e0 = c.ev_pool[c.ev_used++];
    e1 = c.ev_pool[c.ev_used++];
    return hipEventRecord(e0, st);
  }
  hipError_t end() {
    if (!e1) return hipSuccess;
    ++c.launches;
    return hipEventRecord(e1, st);
  }
};

}  // namespace

hipError_t launch_order_sweep(Ctx& c, int batch, bool factored, const int32_t* d_pos, const double* d_w01, int nvisit,
                              const int32_t* d_visit, const double* d_u, double beta, double min_gain, double* d_cells,
                              double* d_cs, int32_t* d_posout, double* d_ll0, double* d_ll, int32_t* d_q,
                              double* d_dll, double* d_llvis, int32_t* d_nmoved, hipStream_t st) {
  if (c.dtype != 0 || c.S > kMaxS) return hipErrorInvalidValue;
  OrderSweepTimer tm{c, st};
  hipError_t err = tm.begin();
  if (err != hipSuccess) return err;
  const int T = order_sweep_threads(c.E);
  if (factored)
    order_sweep_kernel<true><<<batch, T, 0, st>>>(c.S, c.E, nvisit, d_pos, d_w01, d_visit, d_u, beta, min_gain,
                                                  d_cells, d_cs, c.d_D1w, c.nwords, c.d_elo, c.d_ehi, nullptr,
                                                  d_posout, d_ll0, d_ll, d_q, d_dll, d_llvis, d_nmoved);
  else
    order_sweep_kernel<false><<<batch, T, 0, st>>>(c.S, c.E, nvisit, d_pos, d_w01, d_visit, d_u, beta, min_gain,
                                                   d_cells, d_cs, nullptr, 0, nullptr, nullptr, (const double*)c.d_eT,
                                                   d_posout, d_ll0, d_ll, d_q, d_dll, d_llvis, d_nmoved);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  return tm.end();
}

}  // namespace nemo
