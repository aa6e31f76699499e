// nemo_factored.hip -- order score as a dense fp64 MFMA contraction.
//
// Every score table the reference builds (nem.py:36-47) has, for a parent
// j != child i, T[i][j][e] = L[j][e] independent of i, and L[j][e] takes two
// values (B where D[j][e] == 0, -A where D[j][e] == 1).  So each log factor of
// compute_cell_ratios (nem_order_mcmc.py:83-86) is one of two numbers per
// (i, j):  g_lo(i,j) = log(1 - w + w e^{lo_j}),  g_hi(i,j) = log(1 - w + w e^{hi_j}),
// and the cell ratios become
//     cell[i][e] = U[i][e] + G[i] + sum_j Delta[i][j] * D1[j][e],
//     G[i] = sum_{j in pa(i)} g_lo(i,j),   Delta = g_hi - g_lo (0 off pa(i)),
// a (S x S) . (S x E) product with K = S.  Staging detects the structure and
// keeps D1 as a bit matrix; the product runs on v_mfma_f64_16x16x4_f64 and
// the column log-sum-exp is fused into the epilogue.
//
// Children and parents are taken in ORDER position (pi), so Delta is strictly
// lower triangular (a band of width `cap` with a parent cap) and the MFMA
// k-loop of row block r stops at the diagonal: ~half the square's work.
//
// Geometry: one block = one evaluation x (WAVES*16) effects; each wave owns
// 16 effects and ALL children (NR row blocks of 16), so the log-sum-exp over
// children stays inside the wave (two xor-shuffles).  Delta is staged
// through LDS per 64-parent chunk (row stride 66 doubles: conflict-free
// ds_read_b64 A-fragments); the B fragments are bits of D1, expanded in
// registers once per chunk.
#include "nemo_internal.h"

#include <math.h>

#include <algorithm>

namespace nemo {

namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

__device__ __forceinline__ double fwave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// v_max_f64 without the sNaN canonicalisation hipcc wraps around fmax: the
// operands here are MFMA results and loads of finite tables
__device__ __forceinline__ double vmax(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ int fxcd_work_index(int L, int N, int remap) {
  if (!remap) return L;
  const int x = L & 7, k = L >> 3;
  const int q = N >> 3, r = N & 7;
  return x * q + (x < r ? x : r) + k;
}

// ---------------------------------------------------------------------------
// prep: Delta, G and pi of every evaluation.  grid = batch, block = 256.
// Dp [b][SPAD][SPAD] (row = child position q, col = parent position p),
// G  [b][SPAD], permo [b][SPAD] (node at position q; S for padding rows).
// ---------------------------------------------------------------------------
// one wave: row q (child position q) of Delta and its G, for the order in
// perm (LDS); padding rows (q >= S) carry zeros and a finite "no row" G
__device__ __forceinline__ void delta_row(int S, int SPAD, int cap, int b, int q, const int* perm,
                                          const double* __restrict__ w01, const double* __restrict__ e_lo,
                                          const double* __restrict__ e_hi, double* __restrict__ Dp,
                                          double* __restrict__ G, int lane) {
  const int i = q < S ? perm[q] : 0;
  const double* wrow = w01 + ((size_t)b * S + i) * S;
  double* drow = Dp + ((size_t)b * SPAD + q) * SPAD;
  double gsum = 0.0;
  for (int p0 = 0; p0 < SPAD; p0 += kWave) {
    const int p = p0 + lane;
    double d = 0.0, glo = 0.0;
    const bool ok = q < S && p < q && (cap == 0 || q - p <= cap);
    if (ok) {
      const int j = perm[p];
      const double s = wrow[j];
      // 1 - s + s e^t with 1 - s formed first (exact for s >= 0.5): fma(s, e^t - 1, 1)
      // rounds e^t - 1 to 2^-53, which is all of a small e^t once s reaches 1
      const double s1 = 1.0 - s;
      const double lo = log(fma(s, e_lo[j], s1));
      const double hi = log(fma(s, e_hi[j], s1));
      d = hi - lo;
      glo = lo;
    }
    if (p < SPAD && p != (q | 15)) drow[p] = d;
    gsum += fwave_sum(glo);
  }
  if (lane == 0) {
    G[(size_t)b * SPAD + q] = gsum;
    // column 16r+15 of row block r is never a parent of rows 16r..16r+15:
    // it carries G (the score kernels multiply it by 1), and a finite
    // "no row" value on padding rows
    drow[q | 15] = q < S ? gsum : kPadG;
  }
}

__global__ __launch_bounds__(256) void prep_factored_kernel(
    int S, int SPAD, int cap, const int32_t* __restrict__ pos, const double* __restrict__ w01,
    const double* __restrict__ e_lo, const double* __restrict__ e_hi, double* __restrict__ Dp,
    double* __restrict__ G, int32_t* __restrict__ permo) {
  __shared__ int perm[kMaxS];
  __shared__ int scan[kMaxS];
  // block = (evaluation, group of 4 child positions); one row per wave (the
  // rows of one evaluation spread over SPAD / 4 blocks: a lone evaluation's
  // prep is a quarter of the serial work per wave it was with 16-row blocks)
  const int ngroups = SPAD / 4;
  const int b = blockIdx.x / ngroups;
  const int grp = blockIdx.x - b * ngroups;
  const int tid = threadIdx.x;
  prep_order_lds(S, cap, pos + (size_t)b * S, perm, scan, false);
  if (grp == 0)
    for (int k = tid; k < SPAD; k += blockDim.x) permo[(size_t)b * SPAD + k] = k < S ? perm[k] : S;
  const int q = 4 * grp + tid / kWave;
  delta_row(S, SPAD, cap, b, q, perm, w01, e_lo, e_hi, Dp, G, tid & (kWave - 1));
}

// nemo_score_rates' prep (S <= 64): prep_factored_kernel with each evaluation's
// own two values per parent row, e_lo = e^{B_j} (D[j][e] = 0) and e_hi =
// e^{-A_j} (D[j][e] = 1), from rates [b][2][S] (A row, B row).  Every block
// forms them in LDS; group 0 leaves them in rexp [b][2][S] (e^B row, e^-A row)
// for the finish.
__global__ __launch_bounds__(256) void prep_rates_kernel(
    int S, int SPAD, int cap, const int32_t* __restrict__ pos, const double* __restrict__ w01,
    const double* __restrict__ rates, double* __restrict__ Dp, double* __restrict__ G,
    int32_t* __restrict__ permo, double* __restrict__ rexp) {
  __shared__ int perm[kMaxS];
  __shared__ int scan[kMaxS];
  __shared__ double ev[2 * 64];
  const int ngroups = SPAD / 4;
  const int b = blockIdx.x / ngroups;
  const int grp = blockIdx.x - b * ngroups;
  const int tid = threadIdx.x;
  if (tid < 2 * S) {
    const int hi = tid >= S, j = tid - (hi ? S : 0);
    const double* rb = rates + (size_t)b * 2 * S;
    const double v = hi ? exp(-rb[j]) : exp(rb[S + j]);
    ev[64 * hi + j] = v;
    if (grp == 0) rexp[(size_t)b * 2 * S + tid] = v;
  }
  prep_order_lds(S, cap, pos + (size_t)b * S, perm, scan, false);  // (its barriers publish ev)
  if (grp == 0)
    for (int k = tid; k < SPAD; k += blockDim.x) permo[(size_t)b * SPAD + k] = k < S ? perm[k] : S;
  const int q = 4 * grp + tid / kWave;
  delta_row(S, SPAD, cap, b, q, perm, w01, ev, ev + 64, Dp, G, tid & (kWave - 1));
}

// the fused step's prep (nemo_optimal_weights_dev): prep_kernel's work for
// children 4 g .. 4 g + 3 and prep_factored_kernel's for positions 4 g ..
// 4 g + 3 in one block g of the evaluation -- the same arithmetic, one
// launch (a graph node costs ~5 us however small its kernel)
__global__ __launch_bounds__(256) void step_prep_kernel(
    int S, int SPAD, int cap, const int32_t* __restrict__ pos, const double* __restrict__ w01,
    const double* __restrict__ e_lo, const double* __restrict__ e_hi, int32_t* __restrict__ rows,
    double* __restrict__ sw, int32_t* __restrict__ cnt, int32_t* __restrict__ pairs, int32_t* __restrict__ info,
    double* __restrict__ Dp, double* __restrict__ G, int32_t* __restrict__ permo) {
  __shared__ int perm[kMaxS];
  __shared__ int scan[kMaxS];
  const int ngroups = max((S + 3) / 4, SPAD / 4);
  const int b = blockIdx.x / ngroups;
  const int grp = blockIdx.x - b * ngroups;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int32_t* pb = pos + (size_t)b * S;
  prep_order_lds(S, cap, pb, perm, scan, true);
  if (grp == 0)
    for (int k = tid; k < SPAD; k += blockDim.x) permo[(size_t)b * SPAD + k] = k < S ? perm[k] : S;
  const int r = 4 * grp + tid / kWave;  // this wave's child and position
  if (r < S) prep_child_list(S, cap, pb, w01, rows, sw, cnt, pairs, info, b, r, perm, scan, lane);
  if (r < SPAD) delta_row(S, SPAD, cap, b, r, perm, w01, e_lo, e_hi, Dp, G, lane);
}

// ---------------------------------------------------------------------------
// score: grid = batch * ntiles (1-D, XCD remap, evaluation-major so the
// blocks of one evaluation share its Delta in L2), block = WAVES waves.
// ---------------------------------------------------------------------------
template <int NR, int WAVES>
__global__ __launch_bounds__(WAVES * kWave) void score_factored_kernel(
    int S, int E, int ntiles, int cap, const double* __restrict__ Dp,
    const int32_t* __restrict__ permo,
    const uint64_t* __restrict__ D1w, int nwords, const double* __restrict__ U,
    double* __restrict__ partial, double* __restrict__ cs_out, double* __restrict__ cells,
    double* __restrict__ ow, int remap) {
  constexpr int SPAD = NR * 16;
  constexpr int KC = SPAD < 64 ? SPAD : 64;  // parents per LDS chunk
  constexpr int LDA = KC + 1;                // odd row stride: conflict-free A reads
  constexpr int NS = KC / 4;                 // k-steps per chunk
  constexpr int COLS = WAVES * 16;
  constexpr int WPR = (COLS + 63) / 64 + 1;  // D1 words per parent row a block can touch
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* A = lds;                                       // [SPAD][LDA]
  uint64_t* words = (uint64_t*)(A + SPAD * LDA);         // [SPAD][WPR]
  double* etab = (double*)(words + SPAD * WPR);          // [64] 2^(j/64)
  int* perm_s = (int*)(etab + 64);                       // [SPAD]

  const int work = fxcd_work_index((int)blockIdx.x, (int)gridDim.x, remap);
  const int b = work / ntiles;  // evaluation-major
  const int tile = work - b * ntiles;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int e_blk = tile * COLS;
  const int e_w0 = e_blk + w * 16;
  const int col = lane & 15;
  const int e = e_w0 + col;
  const bool valid = e < E;
  const int ec = valid ? e : E - 1;
  const int word0 = e_blk >> 6;
  const int shift = (e_w0 >> 6) - word0;  // which of the block's words this wave reads
  const int bitpos = (e_w0 & 63) + col;
  const uint32_t diag = lane >= 48 ? 1u : 0u;

  if (tid < 64) etab[tid] = exp2((double)tid * (1.0 / 64.0));
  for (int k = tid; k < SPAD; k += blockDim.x) {
    const int node = permo[(size_t)b * SPAD + k];
    perm_s[k] = node;
    for (int u = 0; u < WPR; ++u) {
      const int wi = word0 + u;
      words[k * WPR + u] = (node < S && wi < nwords) ? D1w[(size_t)node * nwords + wi] : 0ull;
    }
  }

  f64x4 acc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = f64x4{0.0, 0.0, 0.0, 0.0};

  const double* Db = Dp + (size_t)b * SPAD * SPAD;
  constexpr int NCH = SPAD / KC;
  // the epilogue's U values, loaded once perm_s is visible (the first chunk's
  // barrier) so their latency hides behind the staging and the MFMAs instead
  // of following them (a lone evaluation's launch is a chain of such waits)
  double uv[NR][4];
  double unull = 0.0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int c0 = c * KC;
    __syncthreads();
    if (c == 0) {
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int q = 16 * r + (lane >> 4) + 4 * g;
          uv[r][g] = q < S ? U[(size_t)perm_s[q] * E + ec] : 0.0;
        }
      unull = U[(size_t)S * E + ec];
    }
    // stage Delta[:, c0 .. c0+KC) (coalesced rows); only rows that have
    // parents in this chunk (row q needs p < q, i.e. q > c0)
    for (int k = tid; k < SPAD * KC; k += blockDim.x) {
      const int row = k / KC, kk = k - row * KC;
      if (c0 + kk <= (row | 15))  // only the k range row's block reads
        A[row * LDA + kk] = Db[(size_t)row * SPAD + c0 + kk];
    }
    __syncthreads();
    // B fragments of this chunk: lane holds D1[parent at 4s + lane/16][its effect]
    uint32_t bits[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int p = c0 + 4 * s + (lane >> 4);
      const uint64_t wd = words[p * WPR + shift];
      bits[s] = (uint32_t)((wd >> bitpos) & 1ull);
    }
    // lower-triangular k-loop, fully static: row block r (positions
    // 16r..16r+15) has parents only at positions <= 16r+14, and column
    // 16r+15 holds G (B = 1 there: lanes 48..63 of the diagonal k-step).
    // k-steps outer, row blocks inner: consecutive MFMAs use independent
    // accumulators.
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (c0 + 4 * s <= 16 * r + 12) {
          const uint32_t bv = (c0 + 4 * s == 16 * r + 12) ? (bits[s] | diag) : bits[s];
          const double a = A[(16 * r + (lane & 15)) * LDA + 4 * s + (lane >> 4)];
          acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)bv, acc[r], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: cells, column log-sum-exp, order weights --------------
  // f64 16x16x4 C layout: col = lane & 15, row = (lane >> 4) + 4 * reg
  double cell[NR][4];
  double m = -INFINITY;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int q = 16 * r + (lane >> 4) + 4 * g;
      double v = -INFINITY;
      if (q < S) v = uv[r][g] + acc[r][g];
      cell[r][g] = v;
      m = v > m ? v : m;
    }
  }
  m = m > unull ? m : unull;
  m = fmax(m, __shfl_xor(m, 16, kWave));
  m = fmax(m, __shfl_xor(m, 32, kWave));
  double l = 0.0;
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int g = 0; g < 4; ++g) l += exp_tab(cell[r][g] - m, etab);
  l += __shfl_xor(l, 16, kWave);
  l += __shfl_xor(l, 32, kWave);
  l += exp_tab(unull - m, etab);
  const double cs = m + log(l);
  if (valid && lane < 16 && cs_out) cs_out[(size_t)b * E + e] = cs;
  // per-wave partial over its 16 effects (lanes 0..15 hold one copy each)
  double part = (valid && lane < 16) ? cs : 0.0;
  part = fwave_sum(part);
  const int ntw = ntiles * WAVES;
  if (lane == 0) partial[(size_t)b * ntw + tile * WAVES + w] = part;
  if ((cells || ow) && valid) {
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int q = 16 * r + (lane >> 4) + 4 * g;
        if (q < S) {
          const size_t k = ((size_t)b * (S + 1) + perm_s[q]) * E + e;
          if (cells) cells[k] = cell[r][g];
          if (ow) ow[k] = exp_tab(cell[r][g] - cs, etab);
        }
      }
    if (lane < 16) {
      const size_t k = ((size_t)b * (S + 1) + S) * E + e;
      if (cells) cells[k] = unull;
      if (ow) ow[k] = exp_tab(unull - cs, etab);
    }
  }
}

__global__ void finalize_factored_kernel(int batch, int n, const double* __restrict__ partial,
                                         double* __restrict__ ll) {
  // one wave per evaluation: strided lane sums, then a fixed xor tree --
  // bitwise reproducible, and ~n/64 dependent adds instead of n
  const int b = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  if (b >= batch) return;
  const double s = sum_partials(partial + (size_t)b * n, n, lane);
  if (lane == 0) ll[b] = s;
}

// ---------------------------------------------------------------------------
// pipelined kernel (SPAD <= 64, the C1-C3 shapes): a block owns one
// evaluation x a contiguous range of 16-effect tiles and stages that
// evaluation's Delta (+ G column) and the D1 words of its range ONCE; each
// wave then walks its tiles (t_begin + w, + WAVES, ...) with no further
// barrier; the U rows of the next tile are prefetched.  (On gfx950 the f64
// MFMA pipe and the VALU do not overlap -- tools/ubench/overlap.hip -- so
// the cost is MFMA cycles + VALU cycles, and the epilogue is kept lean.)
// The MFMA accumulators start at U[perm[q]][e] (the C operand), and the G
// column rides in the diagonal k-step, so a cell leaves the MFMA complete.
// Per tile the epilogue keeps sum(m) and prod(l) per column (l in [1, S+1],
// the product as mantissa x 2^exp), so the log of the log-sum-exp runs once
// per wave, not per tile.  ll only: calls that want cs / cells / order
// weights take the chunked kernel.
// ---------------------------------------------------------------------------
template <int NR, int WAVES>
__global__ __launch_bounds__(WAVES * kWave, 2) void score_factored_pipe_kernel(
    int S, int E, int ntiles, int split, const double* __restrict__ Dp,
    const int32_t* __restrict__ permo, const uint64_t* __restrict__ D1w, int nwords,
    const double* __restrict__ U, double* __restrict__ partial, int remap) {
  // block = (evaluation b, tile range [t_begin, t_begin + WAVES * 8))
  constexpr int SPAD = NR * 16;
  constexpr int LDA = SPAD + 2;  // == 2 mod 32: conflict-free b64 A fragments
  constexpr int NS = SPAD / 4;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* etab = lds;                            // [256] 2^(j/256)
  double* A = etab + 256;                        // [SPAD][LDA]
  uint64_t* words = (uint64_t*)(A + SPAD * LDA); // [nwb][SPAD] D1 words, word-major

  const int work = fxcd_work_index((int)blockIdx.x, (int)gridDim.x, remap);
  const int b = work / split;
  const int part = work - b * split;
  const int tpb = kPipeTilesPerWave * WAVES;
  const int t_begin = part * tpb;
  const int t_end = min(ntiles, t_begin + tpb);
  const int w_lo = (t_begin * 16) >> 6;
  const int nwb = t_end > t_begin ? (((t_end * 16 - 1) >> 6) - w_lo + 1) : 0;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int col = lane & 15, rg = lane >> 4;

  const int32_t* pm = permo + (size_t)b * SPAD;
  for (int k = tid; k < 256; k += blockDim.x) etab[k] = exp2((double)k * (1.0 / 256.0));
  for (int k = tid; k < SPAD * nwb; k += blockDim.x) {
    const int u = k / SPAD, p = k - u * SPAD;
    const int node = pm[p];
    const int wi = w_lo + u;
    words[k] = (node < S && wi < nwords) ? D1w[(size_t)node * nwords + wi] : 0ull;
  }
  const double* Db = Dp + (size_t)b * SPAD * SPAD;
  for (int k = tid; k < SPAD * SPAD; k += blockDim.x) {
    const int row = k / SPAD, kk = k - row * SPAD;
    if (kk <= (row | 15)) A[row * LDA + kk] = Db[k];
  }
  // byte offsets of this lane's 16 cells in U: row perm[q] (S = the
  // "attached to nothing" row for padding), column = its effect in the tile
  uint32_t uoff[NR][4];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      uoff[r][g] = ((uint32_t)pm[16 * r + rg + 4 * g] * (uint32_t)E + col) * 8u;
  const uint32_t unoff = ((uint32_t)S * E + col) * 8u;
  __syncthreads();

  const int ntw = split * WAVES;
  double* part_out = partial + (size_t)b * ntw + part * WAVES + w;
  int t = t_begin + w;
  if (t >= t_end) {
    if (lane == 0) *part_out = 0.0;
    return;
  }

  const uint32_t diag = lane >= 48 ? 1u : 0u;
  const int arow = col * LDA + rg;
  const uint32_t* w32 = (const uint32_t*)words;
  const char* Ub = (const char*)U;

  // U rows of tile tt: the MFMA chain's C-init (prefetched one tile ahead)
  auto load_u = [&](int tt, double (&u)[NR][4], double& un) {
    const char* base = Ub + (size_t)tt * 128;  // 16 effects x 8 B (uniform)
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int g = 0; g < 4; ++g) u[r][g] = *(const double*)(base + uoff[r][g]);
    un = *(const double*)(base + unoff);
  };

  double msum = 0.0, lprod = 1.0;
  int lexp = 0;
  double uc[NR][4], unc;
  load_u(t, uc, unc);
  for (; t < t_end; t += WAVES) {
    // ---- cells of tile t: U + G + Delta . D1 on the MFMA (G rides in the
    // diagonal k-step: column 16r+15 of row block r, B = 1 in lanes 48..63)
    f64x4 acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = f64x4{uc[r][0], uc[r][1], uc[r][2], uc[r][3]};
    const double unull = unc;
    {
      const int uidx = ((t * 16) >> 6) - w_lo;
      const int half = (t >> 1) & 1;
      const uint32_t bit = ((t & 1) << 4) + col;
      const uint32_t* wp = w32 + ((size_t)uidx * SPAD + rg) * 2 + half;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const uint32_t bv = __builtin_amdgcn_ubfe(wp[8 * s], bit, 1);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          if (4 * s <= 16 * r + 12) {
            const uint32_t bb = (4 * s == 16 * r + 12) ? (bv | diag) : bv;
            const double a = A[arow + 16 * r * LDA + 4 * s];
            acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)bb, acc[r], 0, 0, 0);
          }
        }
      }
    }
    if (t + WAVES < t_end) load_u(t + WAVES, uc, unc);
    // ---- column log-sum-exp (over the NR*16 rows and the null row)
    const bool valid = t * 16 + col < E;
    double m = unull;
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int g = 0; g < 4; ++g) m = vmax(m, acc[r][g]);
    m = vmax(m, __shfl_xor(m, 16, kWave));
    m = vmax(m, __shfl_xor(m, 32, kWave));
    double l = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int g = 0; g < 4; ++g) l += exp_lse(acc[r][g] - m, etab);
    l += __shfl_xor(l, 16, kWave);
    l += __shfl_xor(l, 32, kWave);
    l += exp_lse(unull - m, etab);
    // prod(l) kept as mantissa * 2^lexp: branch-free, no overflow
    msum += valid ? m : 0.0;
    lprod *= valid ? l : 1.0;
    lexp += __builtin_amdgcn_frexp_exp(lprod);
    lprod = __builtin_amdgcn_frexp_mant(lprod);
  }
  double v = msum + (log(lprod) + (double)lexp * 0.69314718055994530942);
  v = lane < 16 ? v : 0.0;
  v = fwave_sum(v);
  if (lane == 0) *part_out = v;
}

template <int NR, int WAVES>
hipError_t launch_fact_w(Ctx& c, int batch, int cap, double* d_cs, double* d_cells,
                         double* d_ow, hipStream_t st, int* nparts) {
  constexpr int SPAD = NR * 16;
  constexpr int KC = SPAD < 64 ? SPAD : 64;
  constexpr int COLS = WAVES * 16;
  constexpr int WPR = (COLS + 63) / 64 + 1;
  const int nt = (c.E + COLS - 1) / COLS;
  const size_t lds = (size_t)SPAD * (KC + 1) * 8 + (size_t)SPAD * WPR * 8 + 64 * 8 + SPAD * 4;
  score_factored_kernel<NR, WAVES><<<dim3(nt * batch), WAVES * kWave, lds, st>>>(
      c.S, c.E, nt, cap, c.d_fDp, c.d_fperm, c.d_D1w, c.nwords, (const double*)c.d_U64,
      fpartial(c), d_cs, d_cells, d_ow, c.xcd_remap);
  *nparts = nt * WAVES;
  return hipGetLastError();
}

// partial t of an evaluation is its 16-effect tile t's sum whatever WAVES
// is (sum_partials adds the zero padding of the last block exactly), so any
// WAVES gives the same bits.  Tried: 2 waves (32 effects) per block for the
// fused step of one chain (63 blocks instead of 16): 23 against 18 us per
// launch -- each block stages the whole Delta (32 KB) with a quarter of the
// threads -- so every batch takes 8 waves per block.
template <int NR>
hipError_t launch_fact_t(Ctx& c, int batch, int cap, double* d_cs, double* d_cells,
                         double* d_ow, hipStream_t st, int* nparts) {
  return launch_fact_w<NR, kFactWaves>(c, batch, cap, d_cs, d_cells, d_ow, st, nparts);
}

template <int NR, int WAVES>
hipError_t launch_pipe_t(Ctx& c, int batch, hipStream_t st, int* nparts) {
  constexpr int SPAD = NR * 16;
  const int ntiles = (c.E + 15) / 16;
  const int tpb = kPipeTilesPerWave * WAVES;
  const int split = (ntiles + tpb - 1) / tpb;
  const int nwb_max = (tpb * 16 + 63) / 64 + 1;
  const size_t lds = 256 * 8 + (size_t)SPAD * (SPAD + 2) * 8 + (size_t)nwb_max * SPAD * 8;
  score_factored_pipe_kernel<NR, WAVES><<<dim3(batch * split), WAVES * kWave, lds, st>>>(
      c.S, c.E, ntiles, split, c.d_fDp, c.d_fperm, c.d_D1w, c.nwords, (const double*)c.d_U64,
      fpartial(c), c.xcd_remap);
  *nparts = split * WAVES;
  return hipGetLastError();
}

}  // namespace

// ---- the variant of a call: adapters of nemo_fact_kernels.h over Ctx ----
static host::FactModel fact_model(const Ctx& c, int cap) {
  auto bnd = [&](int kind) { return host::fixed_point_bound(kind, c.i8_cexp, c.fx_colsum, c.S, c.E, cap); };
  return {c.S, c.E, c.fspad, c.nwords, c.d_B8 != nullptr, c.i8o_ok, c.i8l_ok, c.i8w_ok, c.win_ok,
          bnd(host::kFxLog2), bnd(host::kFxNatural), c.err_budget};
}

int factored_partials(const Ctx& c) { return host::fact_partials_max(c.E); }

int score_partials(const Ctx& c, int fk) { return host::fact_partials(host::kFactKernels[fk], c.E, c.nwords); }

int resolve_fact_kernel(const Ctx& c, int cap, bool ll_only, double* bound) {
  if (bound) *bound = 0.0;
  if (!c.factored) return -1;
  const host::FactModel m = fact_model(c, cap);
  const host::FactChoice ch = host::resolve_fact(m, c.fact_kernel, cap, ll_only, 0);  // (the batch only shapes the row)
  if (bound && ch.fk >= 0) *bound = host::fact_bound(ch.k, m);
  return ch.fk;
}

hipError_t launch_prep_factored(Ctx& c, int batch, int cap, const int32_t* d_pos, const double* d_w01,
                                hipStream_t st) {
  const int spad = c.fspad;
  prep_factored_kernel<<<batch * (spad / 4), 256, 0, st>>>(c.S, spad, cap, d_pos, d_w01, c.d_elo, c.d_ehi,
                                                           c.d_fDp, c.d_fG, c.d_fperm);
  return hipGetLastError();
}

hipError_t launch_prep_rates(Ctx& c, int batch, int cap, const int32_t* d_pos, const double* d_w01,
                             const double* d_rates, hipStream_t st) {
  const int spad = c.fspad;
  if (spad > 64 || !c.d_rexp) return hipErrorInvalidValue;
  prep_rates_kernel<<<batch * (spad / 4), 256, 0, st>>>(c.S, spad, cap, d_pos, d_w01, d_rates, c.d_fDp, c.d_fG,
                                                        c.d_fperm, c.d_rexp);
  return hipGetLastError();
}

hipError_t launch_score_factored(Ctx& c, int batch, int cap, const int32_t* d_pos,
                                 const double* d_w01, double* d_ll, double* d_cs, double* d_cells,
                                 double* d_ow, hipStream_t st, bool prepped, int* defer_np) {
  const int spad = c.fspad;
  if (cap >= c.S - 1) cap = 0;  // every predecessor is within the cap: no cap (same bits)
  const bool ll_only = !d_cs && !d_cells && !d_ow;
  if (!c.factored) return hipErrorInvalidValue;
  const host::FactChoice ch = host::resolve_fact(fact_model(c, cap), c.fact_kernel, cap, ll_only, batch);
  if (ch.fk < 0) return hipErrorInvalidValue;  // asked for a kernel the staged model does not support
  const host::FactKernel& k = ch.k;
  // every partial buffer (d_fpartial, a redirected part_out) holds
  // factored_partials per evaluation: checked before anything is launched
  const int np_pred = host::fact_partials(k, c.E, c.nwords);
  if (np_pred > factored_partials(c)) return hipErrorInvalidValue;
  hipError_t err = hipSuccess;
  if (!k.self_prep && !prepped)  // the int8 and lookup-table kernels derive their inputs themselves
    err = launch_prep_factored(c, batch, cap, d_pos, d_w01, st);
  if (err != hipSuccess) return err;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (c.timing && c.timing_kernel == 0 && c.ev_used + 2 <= c.ev_pool.size()) {
    e0 = c.ev_pool[c.ev_used++];
    e1 = c.ev_pool[c.ev_used++];
    { hipError_t re = hipEventRecord(e0, st); if (re != hipSuccess) return re; }
  }
  int np = 0;
  bool finalized = false;
  using host::FactFamily;
  switch (k.family) {
    case FactFamily::kWindow:
      err = launch_score_window(c, batch, cap, d_pos, d_w01, d_ll, st, &np, &finalized, k.round1);
      break;
    case FactFamily::kI8w:
      err = launch_score_i8w(c, batch, cap, d_pos, d_w01, d_ll, k.tiles == 2, st, &np, &finalized);
      break;
    case FactFamily::kI8o:
    case FactFamily::kI8l:
    case FactFamily::kI8s:
    case FactFamily::kI8p:
      err = launch_score_i8o(c, batch, cap, d_pos, d_w01, d_ll, k, st, &np, &finalized);
      break;
    case FactFamily::kI8:
      err = launch_score_i8(c, batch, cap, d_pos, d_w01, d_ll, k, st, &np, &finalized);
      break;
    case FactFamily::kPipe:
      switch (spad / 16) {
#define NEMO_PIPE(NRV)                                                               \
  case NRV:                                                                          \
    err = k.waves == 8 ? launch_pipe_t<NRV, 8>(c, batch, st, &np)                    \
                       : launch_pipe_t<NRV, 4>(c, batch, st, &np);                   \
    break;
        NEMO_PIPE(1)
        NEMO_PIPE(2)
        NEMO_PIPE(4)
#undef NEMO_PIPE
        default: return hipErrorInvalidValue;
      }
      break;
    case FactFamily::kChunked:
      switch (spad / 16) {
        case 1: err = launch_fact_t<1>(c, batch, cap, d_cs, d_cells, d_ow, st, &np); break;
        case 2: err = launch_fact_t<2>(c, batch, cap, d_cs, d_cells, d_ow, st, &np); break;
        case 4: err = launch_fact_t<4>(c, batch, cap, d_cs, d_cells, d_ow, st, &np); break;
        case 8: err = launch_fact_t<8>(c, batch, cap, d_cs, d_cells, d_ow, st, &np); break;
        case 16: err = launch_fact_t<16>(c, batch, cap, d_cs, d_cells, d_ow, st, &np); break;
        default: return hipErrorInvalidValue;
      }
      break;
  }
  if (err != hipSuccess) return err;
  if (np != np_pred) return hipErrorUnknown;  // the row's partial rule out of step with its launcher: a build bug
  if (e1) {
    (void)hipEventRecord(e1, st);
    c.launches++;
  }
  // per-evaluation partials, summed in a fixed order
  if (defer_np) *defer_np = finalized ? 0 : np;
  else if (!finalized)
    finalize_factored_kernel<<<(batch + 3) / 4, 256, 0, st>>>(batch, np, fpartial(c), d_ll);
  return hipGetLastError();
}

hipError_t launch_step_prep(Ctx& c, int batch, int cap, const int32_t* d_pos, const double* d_w01,
                            int32_t* d_info, hipStream_t st) {
  const int spad = c.fspad;
  if (cap >= c.S - 1) cap = 0;  // as launch_score_factored (same lists: a cap >= S - 1 cuts nothing)
  const int ngroups = std::max((c.S + 3) / 4, spad / 4);
  step_prep_kernel<<<batch * ngroups, 256, 0, st>>>(c.S, spad, cap, d_pos, d_w01, c.d_elo, c.d_ehi, c.d_rows,
                                                    c.d_sw, c.d_cnt, c.d_pairs, d_info, c.d_fDp, c.d_fG,
                                                    c.d_fperm);
  return hipGetLastError();
}

}  // namespace nemo
