// nemo_moves.hip -- the exact score change of every single-weight move.
//
// With cell[i][e] = U[i][e] + sum_j log f_ij(e), f_ij(e) = 1 - w_ij + w_ij v_ij(e),
// v = e^T, and ow = exp(cell - cs), replacing ONE weight w_ij by w'_ij moves
// only row i of the cells, by log(f'/f) = log1p(kappa), so cs[e] moves by
// log1p(ow[i][e] kappa_ij(e)) and
//     ll(w with w_ij := w'_ij) - ll(w) = sum_e log1p(ow[i][e] kappa_ij(e)),
//     kappa_ij(e) = (w'_ij - w_ij) (v_ij(e) - 1) / f_ij(e)
// in closed form, with no differencing of two scores: exact to fp64 rounding
// however small the move's effect.  (v - 1) / f is the gradient's f' (fprime):
// the gradient is this sum's first-order term.  The sum is not linear in ow, so
// it is no matrix product: one log1p per (pair, effect).
//
// Fused kernel (factored model, S <= 64).  The first half is the fused gradient
// kernel's forward (nemo_grad_fwd.h): cells^T on the fp64 matrix cores, the
// column log-sum-exp, ow in the C-fragment registers.  The second half works in
// rounds of kMovesRoundTiles 16-effect tiles: wave w < kMovesRoundTiles runs the
// forward of the round's tile w and writes its order weights to the LDS as
// [effect][q]; after a barrier every lane owns up to NSLOT pairs (q, p), p < q in
// order positions -- pair slot n = q (q - 1) / 2 + p = k * 512 + tid, a function
// of SPAD alone; the cap and S < SPAD leave slots idle and renumber nothing --
// with kappa_lo and kappa_hi in registers (a factored row has two values, picked
// by the bit D1[p][e]), and adds log1p(ow[e][q] kappa) to the pair's accumulator,
// the effects in ascending order.  Lanes of a wave hold consecutive slots: their
// q are one value (a broadcast read) or a run of fewer than 32 consecutive ones
// (different banks).  Per-part sums go to the parts buffer; the finish adds the
// parts in order and writes [S][S] by node, +0.0 off the permissible set.
//
// Two-pass (everything else): the forward leaves ow in HBM and
// moves_reduce_kernel has grad_reduce_kernel's shape.
//
// Every sum has a fixed order that depends on the staged model alone.
#include "nemo_grad_fwd.h"
#include "nemo_internal.h"

#include <math.h>

namespace nemo {

namespace {

constexpr int kMovesThreads = kGradWaves * kWave;

// pair slot n -> (q, p), p < q: n = q (q - 1) / 2 + p
__device__ __forceinline__ void slot_pair(int n, int& q, int& p) {
  int qq = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)n)) * 0.5f);
  while (qq * (qq - 1) / 2 > n) --qq;
  while ((qq + 1) * qq / 2 <= n) ++qq;
  q = qq;
  p = n - qq * (qq - 1) / 2;
}

// ---------------------------------------------------------------------------
// fused: grid = batch * nparts (evaluation-major, XCD remap), block =
// kGradWaves waves.  part_out [b][part][NSLOT * 512] by pair slot, llpart [b][part].
// ---------------------------------------------------------------------------
template <int NR>
__global__ __launch_bounds__(kMovesThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void score_moves_fused_kernel(
    int S, int E, int cap, int ntiles, int nparts, const double* __restrict__ Dp, const int32_t* __restrict__ permo,
    const uint64_t* __restrict__ D1w, int nwords, const double* __restrict__ U, const double* __restrict__ w01,
    const double* __restrict__ walt, const double* __restrict__ e_lo, const double* __restrict__ e_hi,
    double* __restrict__ part_out, double* __restrict__ llpart, int remap) {
  using L = GradFwdLds<NR>;
  constexpr int SPAD = L::SPAD;
  constexpr int RT = kMovesRoundTiles, RE = RT * 16;  // a round's tiles and effects
  constexpr int LDO = SPAD + 1;
  constexpr int NPAIR = SPAD * (SPAD - 1) / 2;
  constexpr int NSLOT = (NPAIR + kMovesThreads - 1) / kMovesThreads;
  static_assert(64 % RE == 0, "a round's bits come from one D1 word");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const double* etab = lds + L::kEtab;
  const double2* ltab = (const double2*)(lds + L::kLtab);
  double* llw = lds + L::kLlw;
  const double* A = lds + L::kA;
  const uint64_t* words = (const uint64_t*)(lds + L::kWords);
  double* owb = lds + L::kEnd;  // [RE][LDO] the round's order weights

  const int work = gxcd_work_index((int)blockIdx.x, (int)gridDim.x, remap);
  const int b = work / nparts;
  const int part = work - b * nparts;
  const int t_begin = part * L::TPB;
  const int t_end = min(ntiles, t_begin + L::TPB);
  const int w_lo = part * L::NWB;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int col = lane & 15, rg = lane >> 4;

  const int32_t* pm = permo + (size_t)b * SPAD;
  grad_fwd_stage<NR>(lds, S, nwords, w_lo, pm, Dp + (size_t)b * SPAD * SPAD, D1w);
  uint32_t urow[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) urow[r] = (uint32_t)pm[16 * r + col] * (uint32_t)E;

  // this lane's pairs: kappa by bit, the child's column of owb, the parent's word column
  double klo[NSLOT], khi[NSLOT], sum[NSLOT];
  int qs[NSLOT], ps[NSLOT];
  bool any[NSLOT];  // wave-uniform: some lane of the wave holds a live pair in this slot
#pragma unroll
  for (int k = 0; k < NSLOT; ++k) {
    const int n = k * kMovesThreads + tid;
    int q = 0, p = 0;
    if (n < NPAIR) slot_pair(n, q, p);
    const bool live = n < NPAIR && q < S && (cap == 0 || q - p <= cap);
    klo[k] = khi[k] = 0.0;
    sum[k] = 0.0;
    if (live) {
      const int i = pm[q], j = pm[p];
      const size_t o = ((size_t)b * S + i) * S + j;
      const double wv = w01[o], d = walt[o] - wv;
      klo[k] = d * fprime(wv, e_lo[j]);
      khi[k] = d * fprime(wv, e_hi[j]);
    }
    qs[k] = live ? q : 0;
    ps[k] = live ? p : 0;
    any[k] = __ballot(live) != 0ull;
  }
  __syncthreads();

  double csum = 0.0;
  const uint32_t diag = lane >= 48 ? 1u : 0u;
  for (int t0 = t_begin; t0 < t_end; t0 += RT) {
    if (w < RT) {
      // ---- the forward of tile t0 + w (all zeros past the last tile)
      const int t = t0 + w;
      double* orow = owb + (size_t)(16 * w) * LDO;
      if (t < t_end) {
        f64x4 acc[NR];
        const int uidx = ((t * 16) >> 6) - w_lo;
        const int bit0 = (t * 16) & 63;
        grad_fwd_uinit<NR>(acc, t, E, U, urow, rg);
        grad_fwd_mfma<NR>(acc, words + (size_t)uidx * SPAD, bit0, A, col, rg, diag);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int e = t * 16 + 4 * g + rg;
          const bool valid = e < E;
          const double unull = U[(size_t)S * E + (valid ? e : E - 1)];
          double cl[NR];
#pragma unroll
          for (int r = 0; r < NR; ++r) cl[r] = acc[r][g];
          const double cs = grad_fwd_lse<NR>(cl, unull, etab, ltab);
          if (valid && col == 0) csum += cs;
#pragma unroll
          for (int r = 0; r < NR; ++r)
            orow[(4 * g + rg) * LDO + 16 * r + col] = valid ? exp_lse(cl[r] - cs, etab) : 0.0;
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int r = 0; r < NR; ++r) orow[(4 * g + rg) * LDO + 16 * r + col] = 0.0;
      }
    }
    __syncthreads();
    // ---- one pair per lane and slot: the round's RE effects in ascending order
    const int e0 = t0 * 16;
    const uint64_t* wr = words + (size_t)((e0 >> 6) - w_lo) * SPAD;
    const int bit0 = e0 & 63;
    uint32_t bits[NSLOT];
#pragma unroll
    for (int k = 0; k < NSLOT; ++k) bits[k] = (uint32_t)(wr[ps[k]] >> bit0);
#pragma unroll 4
    for (int ee = 0; ee < RE; ++ee) {
      const double* orow = owb + ee * LDO;
#pragma unroll
      for (int k = 0; k < NSLOT; ++k) {
        if (any[k]) {
          const double kap = ((bits[k] >> ee) & 1u) ? khi[k] : klo[k];
          sum[k] += log1p_fast(orow[qs[k]] * kap, ltab);
        }
      }
    }
    __syncthreads();
  }

  csum = gwave_sum(csum);
  if (lane == 0) llw[w] = csum;
  double* out = part_out + ((size_t)b * nparts + part) * (NSLOT * kMovesThreads);
#pragma unroll
  for (int k = 0; k < NSLOT; ++k) out[k * kMovesThreads + tid] = sum[k];
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int ww = 0; ww < RT; ++ww) s += llw[ww];
    llpart[(size_t)b * nparts + part] = s;
  }
}

// grid = batch * ceil(S S / 256), block = 256: one entry of dll per thread
// (every entry is written) and, in an evaluation's first block, its ll; the
// parts are added in part order
__global__ __launch_bounds__(256) void moves_finish_kernel(int S, int cap, int nparts, size_t pd,
                                                           const int32_t* __restrict__ pos,
                                                           const double* __restrict__ part,
                                                           const double* __restrict__ llpart, double* __restrict__ ll,
                                                           double* __restrict__ dll) {
  const int nblk = (S * S + 255) / 256;
  const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk, tid = threadIdx.x;
  if (blk == 0 && tid < kWave) {
    const double s = sum_partials(llpart + (size_t)b * nparts, nparts, tid);
    if (tid == 0) ll[b] = s;
  }
  const int32_t* pb = pos + (size_t)b * S;
  const int k = blk * 256 + tid;
  if (k < S * S) {
    const int i = k / S, j = k - i * S;
    const int q = clamp_pos(pb[i], S), p = clamp_pos(pb[j], S);
    double d = 0.0;
    if (p < q && (cap == 0 || q - p <= cap)) {
      const double* src = part + (size_t)b * nparts * pd + (size_t)(q * (q - 1) / 2 + p);
      for (int t = 0; t < nparts; ++t) d += src[t * pd];
    }
    dll[(size_t)b * S * S + k] = d;
  }
}

// ---------------------------------------------------------------------------
// two-pass: grid = batch * S (one child per block), one wave per parent in
// turn; lane sums over e = lane, lane + 64, ... then the xor tree
// ---------------------------------------------------------------------------
template <bool FACT>
__global__ __launch_bounds__(256) void moves_reduce_kernel(
    int S, int E, int cap, const int32_t* __restrict__ pos, const double* __restrict__ w01,
    const double* __restrict__ walt, const double* __restrict__ ow, const uint64_t* __restrict__ D1w, int nwords,
    const double* __restrict__ e_lo, const double* __restrict__ e_hi, const double* __restrict__ eT,
    double* __restrict__ dll) {
  __shared__ double2 ltab[128];
  fill_log_table(ltab, threadIdx.x, blockDim.x);
  __syncthreads();
  const int b = blockIdx.x / S, i = blockIdx.x - b * S;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int32_t* pb = pos + (size_t)b * S;
  const int q = clamp_pos(pb[i], S);
  const double* orow = ow + ((size_t)b * (S + 1) + i) * E;
  for (int j = wv; j < S; j += 4) {
    const int p = clamp_pos(pb[j], S);
    const size_t k = ((size_t)b * S + i) * S + j;
    if (!(p < q && (cap == 0 || q - p <= cap))) {
      if (lane == 0) dll[k] = 0.0;
      continue;
    }
    const double w = w01[k], d = walt[k] - w;
    double s = 0.0;
    if (FACT) {
      const uint64_t* bits = D1w + (size_t)j * nwords;
      const double klo = d * fprime(w, e_lo[j]), khi = d * fprime(w, e_hi[j]);
      for (int e = lane; e < E; e += kWave) {
        const bool hi = (bits[e >> 6] >> lane) & 1ull;
        s += log1p_fast(orow[e] * (hi ? khi : klo), ltab);
      }
    } else {
      const double* vrow = eT + ((size_t)i * S + j) * E;
      const double s1 = 1.0 - w;
      for (int e = lane; e < E; e += kWave) {
        const double v = vrow[e];
        s += log1p_fast(orow[e] * (d * ((v - 1.0) / fma(w, v, s1))), ltab);
      }
    }
    s = gwave_sum(s);
    if (lane == 0) dll[k] = s;
  }
}

template <int NR>
size_t moves_lds_bytes() {
  return (size_t)(GradFwdLds<NR>::kEnd + kMovesRoundTiles * 16 * (NR * 16 + 1)) * 8;
}
static_assert((GradFwdLds<4>::kEnd + kMovesRoundTiles * 16 * 65) * 8 <= 65536, "the fused kernel's LDS at NR = 4");

template <int NR>
hipError_t launch_moves_fused_t(Ctx& c, int batch, int cap, const double* d_w01, const double* d_walt,
                                hipStream_t st) {
  const int ntiles = (c.E + 15) / 16;
  const int nparts = grad_parts(c.E);
  score_moves_fused_kernel<NR><<<dim3(batch * nparts), kMovesThreads, moves_lds_bytes<NR>(), st>>>(
      c.S, c.E, cap, ntiles, nparts, c.d_fDp, c.d_fperm, c.d_D1w, c.nwords, (const double*)c.d_U64, d_w01, d_walt,
      c.d_elo, c.d_ehi, c.d_movep, c.d_movell, c.xcd_remap);
  return hipGetLastError();
}

// (option timing_kernel 3) the events around the move-score kernels of one call
struct MovesTimer {
  Ctx& c;
  hipStream_t st;
  hipEvent_t e1 = nullptr;
  hipError_t begin() {
    if (!(c.timing && c.timing_kernel == 3 && c.ev_used + 2 <= c.ev_pool.size())) return hipSuccess;
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

hipError_t launch_score_moves_fused(Ctx& c, int batch, int cap, const int32_t* d_pos, const double* d_w01,
                                    const double* d_walt, double* d_ll, double* d_dll, hipStream_t st) {
  if (!c.factored || c.dtype != 0 || c.fspad > 64 || !moves_ready(c)) return hipErrorInvalidValue;
  if (cap >= c.S - 1) cap = 0;  // a cap that cuts nothing (same lists, same bits)
  hipError_t err = launch_prep_factored(c, batch, cap, d_pos, d_w01, st);
  if (err != hipSuccess) return err;
  MovesTimer tm{c, st};
  if ((err = tm.begin()) != hipSuccess) return err;
  switch (c.fspad / 16) {
    case 1: err = launch_moves_fused_t<1>(c, batch, cap, d_w01, d_walt, st); break;
    case 2: err = launch_moves_fused_t<2>(c, batch, cap, d_w01, d_walt, st); break;
    case 4: err = launch_moves_fused_t<4>(c, batch, cap, d_w01, d_walt, st); break;
    default: return hipErrorInvalidValue;
  }
  if (err != hipSuccess) return err;
  moves_finish_kernel<<<batch * ((c.S * c.S + 255) / 256), 256, 0, st>>>(
      c.S, cap, grad_parts(c.E), moves_part_doubles(c.fspad), d_pos, c.d_movep, c.d_movell, d_ll, d_dll);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  return tm.end();
}

hipError_t launch_moves_reduce(Ctx& c, int batch, int cap, bool factored, const int32_t* d_pos,
                               const double* d_w01, const double* d_walt, const double* d_ow, double* d_dll,
                               hipStream_t st) {
  if (c.dtype != 0) return hipErrorInvalidValue;
  if (cap >= c.S - 1) cap = 0;
  MovesTimer tm{c, st};
  hipError_t err = tm.begin();
  if (err != hipSuccess) return err;
  if (factored)
    moves_reduce_kernel<true><<<batch * c.S, 256, 0, st>>>(c.S, c.E, cap, d_pos, d_w01, d_walt, d_ow, c.d_D1w,
                                                           c.nwords, c.d_elo, c.d_ehi, nullptr, d_dll);
  else
    moves_reduce_kernel<false><<<batch * c.S, 256, 0, st>>>(c.S, c.E, cap, d_pos, d_w01, d_walt, d_ow, nullptr, 0,
                                                            nullptr, nullptr, (const double*)c.d_eT, d_dll);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  return tm.end();
}

}  // namespace nemo
