// nemo_grad_fwd.h -- the transposed fp64 MFMA forward shared by the fused
// gradient kernel (nemo_grad.hip) and the fused move-score kernel
// (nemo_moves.hip): the block's LDS image (tables, D1 words, Delta), the cells
// of one 16-effect tile in the C-fragment registers, and the column
// log-sum-exp with the order weights.  The layouts are nemo_grad.hip's header's.
#pragma once

#include "nemo_internal.h"

namespace nemo {

using f64x4 = __attribute__((ext_vector_type(4))) double;

__device__ __forceinline__ double gwave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// max over each 16-lane row, in every lane of the row (rowsum16's moves)
__device__ __forceinline__ double rowmax16(double v) {
  v = fmax(v, dpp_d<0xB1>(v));
  v = fmax(v, dpp_d<0x4E>(v));
  v = fmax(v, dpp_d<0x141>(v));
  v = fmax(v, dpp_d<0x140>(v));
  return v;
}

__device__ __forceinline__ int gxcd_work_index(int L, int N, int remap) {
  if (!remap) return L;
  const int x = L & 7, k = L >> 3;
  const int q = N >> 3, r = N & 7;
  return x * q + (x < r ? x : r) + k;
}

// f' of one value v = e^t of a pair's table row at weight w
__device__ __forceinline__ double fprime(double w, double v) { return (v - 1.0) / fma(w, v, 1.0 - w); }

// position of a node in the order, clamped as the prep kernels clamp it
__device__ __forceinline__ int clamp_pos(int p, int S) { return p < 0 ? 0 : (p >= S ? S - 1 : p); }

// the forward's LDS image of a block of kGradWaves waves: in doubles from the
// start of the dynamic LDS, etab [256] 2^(j/256), ltab [128] log_fast's table,
// llw [kGradWaves], A [SPAD][LDA] Delta, words [NWB][SPAD] D1 words (word-major);
// kEnd: the first double past it
template <int NR>
struct GradFwdLds {
  static constexpr int SPAD = NR * 16;
  static constexpr int LDA = SPAD + 2;  // == 2 mod 32: conflict-free b64 Delta fragments
  static constexpr int NS = SPAD / 4;
  static constexpr int TPB = kGradWaves * kGradTilesPerWave;
  static constexpr int NWB = TPB * 16 / 64;  // D1 words per parent row of a part (parts start on a word)
  static constexpr int kEtab = 0, kLtab = 256, kLlw = 256 + 2 * 128, kA = kLlw + kGradWaves;
  static constexpr int kWords = kA + SPAD * LDA, kEnd = kWords + NWB * SPAD;
};

// fills the image for evaluation b's part whose first D1 word is w_lo (the
// caller's barrier follows): pm = the evaluation's perm, Db its Delta
template <int NR>
__device__ __forceinline__ void grad_fwd_stage(double* lds, int S, int nwords, int w_lo,
                                               const int32_t* pm, const double* Db,
                                               const uint64_t* D1w) {
  using L = GradFwdLds<NR>;
  constexpr int SPAD = L::SPAD, LDA = L::LDA, NWB = L::NWB;
  double* etab = lds + L::kEtab;
  double2* ltab = (double2*)(lds + L::kLtab);
  double* A = lds + L::kA;
  uint64_t* words = (uint64_t*)(lds + L::kWords);
  const int tid = threadIdx.x;
  if (tid < 256) etab[tid] = exp2((double)tid * (1.0 / 256.0));
  fill_log_table(ltab, tid, blockDim.x);
  for (int k = tid; k < SPAD * NWB; k += blockDim.x) {
    const int u = k / SPAD, p = k - u * SPAD;
    const int node = pm[p];
    const int wi = w_lo + u;
    words[k] = (node < S && wi < nwords) ? D1w[(size_t)node * nwords + wi] : 0ull;
  }
  for (int k = tid; k < SPAD * SPAD; k += blockDim.x) {
    const int row = k / SPAD, kk = k - row * SPAD;
    if (kk <= (row | 15)) A[row * LDA + kk] = Db[k];
  }
}

// the C-init of tile t from the staged U: acc[r][g] = U[q = 16 r + col][e = 16 t + 4 g + rg]
template <int NR>
__device__ __forceinline__ void grad_fwd_uinit(f64x4 (&acc)[NR], int t, int E, const double* U,
                                               const uint32_t (&urow)[NR], int rg) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int ec = min(t * 16 + 4 * g + rg, E - 1);
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r][g] = U[urow[r] + ec];
  }
}

// cells^T of a tile on top of the C-init: acc[r][g] += sum_p D1[p][e] Delta[p][q]
// (wt: the tile's word row, bit0: its first bit; diag = lane >= 48)
template <int NR>
__device__ __forceinline__ void grad_fwd_mfma(f64x4 (&acc)[NR], const uint64_t* wt, int bit0, const double* A,
                                              int col, int rg, uint32_t diag) {
  using L = GradFwdLds<NR>;
#pragma unroll
  for (int s = 0; s < L::NS; ++s) {
    const uint32_t bv = (uint32_t)((wt[4 * s + rg] >> (bit0 + col)) & 1ull);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (4 * s <= 16 * r + 12) {
        // column 16 r + 15 of Delta's row block r holds G: the bit is 1 there
        const uint32_t bb = (4 * s == 16 * r + 12) ? (bv | diag) : bv;
        const double d = A[(16 * r + col) * L::LDA + 4 * s + rg];
        acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)bb, d, acc[r], 0, 0, 0);
      }
    }
  }
}

// the log-sum-exp of one effect's cells: cl = the lane's NR cells of the
// effect (child positions 16 r + col; the effect's 16 lanes hold the rest) and
// the null row's unull.  Returns cs in every lane of the row.
template <int NR>
__device__ __forceinline__ double grad_fwd_lse(const double (&cl)[NR], double unull, const double* etab,
                                               const double2* ltab) {
  double m = cl[0];
#pragma unroll
  for (int r = 1; r < NR; ++r) m = fmax(m, cl[r]);
  m = fmax(rowmax16(m), unull);
  double l = 0.0;
#pragma unroll
  for (int r = 0; r < NR; ++r) l += exp_lse(cl[r] - m, etab);
  l = rowsum16(l) + exp_lse(unull - m, etab);
  return m + log_fast(l, ltab);  // l in [1, SPAD + 1]
}

}  // namespace nemo
