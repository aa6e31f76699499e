// nemo_grad.hip -- gradient of the order score in the mapped parent weights.
//
// With cell[i][e] = U[i][e] + sum_{j in pa(i)} log(1 - w_ij + w_ij v_ij(e)),
// v = e^T, and ll = sum_e logsumexp_i cell[i][e] (null row included),
//     d ll / d w_ij = sum_e ow[i][e] f'_ij(e),
//     f'_ij(e) = (v - 1) / fma(w_ij, v, 1 - w_ij),   ow = exp(cell - cs),
// at the permissible pairs (pos[j] < pos[i], within the cap) and 0 elsewhere.
// The denominator is the forward's own factor (delta_row, score_kernel).
//
// Factored model (nemo_factored.hip): v takes two values per parent row, by
// the bit D1[j][e], so with M[i][j] = sum_e ow[i][e] D1[j][e] and the row sum
// R[i] = sum_e ow[i][e]
//     g_ij = f'_lo (R_i - M_ij) + f'_hi M_ij.
// M = OW . D1^T is an (S x E) . (E x S) product with K = E: the transpose of
// the forward's contraction.
//
// Fused kernel (S <= 64).  The forward runs TRANSPOSED on the fp64 matrix
// cores: cells^T[e][q] = sum_p D1^T[e][p] Delta^T[p][q] -- the forward's own
// two fragments with the MFMA operands swapped.  In the 16x16x4 C layout (col
// = lane & 15, row = (lane >> 4) + 4 reg) register g of row block r then holds
// the cell of child position q = 16 r + (lane & 15) at the tile's effect
// 4 g + (lane >> 4), and after the column log-sum-exp (now a sum over the 16
// lanes of a row and the row blocks) the order weight ow[q][e] there: exactly
// the B fragment of k-step g of M^T[p][q] += sum_e D1[p][e] ow[q][e], whose A
// fragment is the bit D1[p = 16 rp + (lane & 15)][e = 4 g + (lane >> 4)].  No
// order weight crosses lanes, the LDS or HBM.  Only the tiles with p-block <=
// q-block hold permissible pairs: NR (NR + 1) / 2 accumulator tiles (10 at
// S = 64), and as many MFMAs per 16-effect tile as the forward.  Row p = 16 r
// + 15 of the diagonal tile (r, r) is never a parent of its columns, so A = 1
// there and the tile's row 15 is R[q].
//
// Every sum runs in a fixed order, with no atomics: a wave folds its tiles
// (t_begin + w, + kGradWaves, ...) into its accumulators, the block adds its
// waves' accumulators in wave order through the LDS, and grad_finish_kernel
// adds the parts in order.  The parts are a function of E alone (grad_parts).
//
// The same kernel with RATES set serves nemo_score_rates: the score at each
// evaluation's own per-gene error rates with its derivatives in them, from M,
// R and the diagonal M_kk (rates_finish_kernel below).
#include "nemo_grad_fwd.h"
#include "nemo_internal.h"

#include <math.h>

namespace nemo {

namespace {

// ---------------------------------------------------------------------------
// fused: grid = batch * nparts (evaluation-major, XCD remap), block =
// kGradWaves waves.  Mpart [b][part][tile (rq, rp), rq (rq + 1) / 2 + rp][reg][lane],
// llpart [b][part].
//
// RATES (nemo_score_rates): the offset form at this evaluation's own rates.
// D1w holds D's own bits (Ctx::d_Dw), Delta and G come from prep_rates_kernel,
// and x[q][e] = cell - U[S][e] leaves the MFMA chain complete: its C-init is
// the own term (D[q][e] ? -A_q : B_q; 0 on padding rows, whose G hides them),
// picked by the child's own bit -- bit 4 g of pb[r], the second contraction's A
// fragment.  No U is read and the null row is the constant 0; the finish adds
// sum_k A_k n_k.  Each lane also sums ow[q][e] D[q][e], the diagonal M_qq that
// d/dA_q and d/dB_q need: the diagonal tile holds it except at q = 15 mod 16,
// where row 15 carries R; Dpart [b][part][SPAD] takes all of them.  The lane
// sums live in per-wave LDS slots (one per lane and row block: no VGPR, which
// NR = 4 has none to give, and no conflict).
// ---------------------------------------------------------------------------
template <int NR, bool RATES>
__global__ __launch_bounds__(kGradWaves* kWave) void score_grad_fused_kernel(
    int S, int E, int ntiles, int nparts, const double* __restrict__ Dp, const int32_t* __restrict__ permo,
    const uint64_t* __restrict__ D1w, int nwords, const double* __restrict__ U, double* __restrict__ Mpart,
    double* __restrict__ llpart, int remap, const double* __restrict__ rates, double* __restrict__ Dpart) {
  using L = GradFwdLds<NR>;
  constexpr int SPAD = L::SPAD;
  constexpr int LDA = L::LDA;
  constexpr int NT = NR * (NR + 1) / 2;
  constexpr int TPB = L::TPB;
  constexpr int NWB = L::NWB;
  static_assert(SPAD * LDA >= NT * 256, "the wave reduction reuses Delta's LDS");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* etab = lds;                              // [256] 2^(j/256)
  double2* ltab = (double2*)(etab + 256);          // [128] log_fast's table
  double* llw = (double*)(ltab + 128);             // [kGradWaves]
  double* A = llw + kGradWaves;                    // [SPAD][LDA], then the reduction's [NT][4][64]
  uint64_t* words = (uint64_t*)(A + SPAD * LDA);   // [NWB][SPAD] D1 words, word-major
  double* own = (double*)(words + NWB * SPAD);     // RATES: [2][SPAD] own term by bit
  double* dg = own + 2 * SPAD;                     // RATES: [kGradWaves][NR][64] each lane's share of M_qq

  const int work = gxcd_work_index((int)blockIdx.x, (int)gridDim.x, remap);
  const int b = work / nparts;
  const int part = work - b * nparts;
  const int t_begin = part * TPB;
  const int t_end = min(ntiles, t_begin + TPB);
  const int w_lo = part * NWB;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int col = lane & 15, rg = lane >> 4;

  const int32_t* pm = permo + (size_t)b * SPAD;
  grad_fwd_stage<NR>(lds, S, nwords, w_lo, pm, Dp + (size_t)b * SPAD * SPAD, D1w);
  // rows of U of this lane's NR child positions (S = the null row: padding)
  // (element offsets: (S + 1) E < 2^31 for S <= 64 at every E the staging takes)
  uint32_t urow[NR];
  if constexpr (!RATES) {
#pragma unroll
    for (int r = 0; r < NR; ++r) urow[r] = (uint32_t)pm[16 * r + col] * (uint32_t)E;
  } else {
    // own[0][q] = B of the node at position q, own[1][q] = -A of it
    const double* rb = rates + (size_t)b * 2 * S;
    for (int k = tid; k < 2 * SPAD; k += blockDim.x) {
      const int bit = k / SPAD, q = k - bit * SPAD;
      const int node = pm[q];
      own[k] = node < S ? (bit ? -rb[node] : rb[S + node]) : 0.0;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) dg[(w * NR + r) * kWave + lane] = 0.0;
  }
  __syncthreads();

  f64x4 acc2[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) acc2[k] = f64x4{0.0, 0.0, 0.0, 0.0};
  double csum = 0.0;
  const uint32_t diag = lane >= 48 ? 1u : 0u;

  for (int t = t_begin + w; t < t_end; t += kGradWaves) {
    // ---- cells^T of tile t: acc[r][g] = cell[q = 16 r + col][e = 16 t + 4 g + rg]
    f64x4 acc[NR];
    const int uidx = ((t * 16) >> 6) - w_lo;
    const int bit0 = (t * 16) & 63;
    const uint64_t* wt = words + (size_t)uidx * SPAD;
    if constexpr (!RATES) {
      grad_fwd_uinit<NR>(acc, t, E, U, urow, rg);
    } else {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const uint32_t ob = (uint32_t)(wt[16 * r + col] >> (bit0 + rg));
        const double o0 = own[16 * r + col], o1 = own[SPAD + 16 * r + col];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[r][g] = ((ob >> (4 * g)) & 1u) ? o1 : o0;
      }
    }
    grad_fwd_mfma<NR>(acc, wt, bit0, A, col, rg, diag);
    // the D1 bits of the second contraction's A fragments: bit 4 g of pb[rp] is
    // D1[p = 16 rp + col][effect 4 g + rg]
    uint32_t pb[NR];
#pragma unroll
    for (int rp = 0; rp < NR; ++rp) pb[rp] = (uint32_t)(wt[16 * rp + col] >> (bit0 + rg));
    // ---- per k-step g (the lane's effect 4 g + rg): the log-sum-exp over the
    // children, the order weights, then M^T[p][q] += D1[p][e] ow[q][e]
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int e = t * 16 + 4 * g + rg;
      const bool valid = e < E;
      double unull = 0.0;
      if constexpr (!RATES) unull = U[(size_t)S * E + (valid ? e : E - 1)];
      // (grad_fwd_lse's text, kept in line: through the call this kernel's NR = 4
      // instance goes from 254 VGPRs to 256 with scratch spills)
      double m = acc[0][g];
#pragma unroll
      for (int r = 1; r < NR; ++r) m = fmax(m, acc[r][g]);
      m = fmax(rowmax16(m), unull);
      double l = 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) l += exp_lse(acc[r][g] - m, etab);
      l = rowsum16(l) + exp_lse(unull - m, etab);
      const double cs = m + log_fast(l, ltab);  // l in [1, SPAD + 1]
      if (valid && col == 0) csum += cs;
      double ow[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) ow[r] = valid ? exp_lse(acc[r][g] - cs, etab) : 0.0;
      if constexpr (RATES) {
#pragma unroll
        for (int r = 0; r < NR; ++r) dg[(w * NR + r) * kWave + lane] += ((pb[r] >> (4 * g)) & 1u) ? ow[r] : 0.0;
      }
#pragma unroll
      for (int rp = 0; rp < NR; ++rp) {
        const uint32_t av = (pb[rp] >> (4 * g)) & 1u;
#pragma unroll
        for (int rq = rp; rq < NR; ++rq) {
          // row 16 r + 15 of the diagonal tile: never a parent there, A = 1 makes it R[q]
          const uint32_t aa = (rq == rp && col == 15) ? 1u : av;
          acc2[rq * (rq + 1) / 2 + rp] =
              __builtin_amdgcn_mfma_f64_16x16x4f64((double)aa, ow[rq], acc2[rq * (rq + 1) / 2 + rp], 0, 0, 0);
        }
      }
    }
  }

  // ---- the block's sums, waves in order (A's LDS reused once every wave is done with it)
  csum = gwave_sum(csum);
  if (lane == 0) llw[w] = csum;
  if constexpr (RATES) {
    // M_qq: the four row groups of a wave into its slots' first 16 lanes (the
    // wave's own reads come first), then the waves in order below
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const double v = rowsum4(dg[(w * NR + r) * kWave + lane]);
      if (rg == 0) dg[(w * NR + r) * kWave + col] = v;
    }
  }
  double* red = A;
  for (int ww = 0; ww < kGradWaves; ++ww) {
    __syncthreads();
    if (w == ww) {
#pragma unroll
      for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int idx = (k * 4 + g) * kWave + lane;
          red[idx] = ww == 0 ? acc2[k][g] : red[idx] + acc2[k][g];
        }
    }
  }
  __syncthreads();
  double* out = Mpart + ((size_t)b * nparts + part) * (NT * 256);
  for (int k = tid; k < NT * 256; k += blockDim.x) out[k] = red[k];
  if (tid == 0) {
    double s = 0.0;
    for (int ww = 0; ww < kGradWaves; ++ww) s += llw[ww];
    llpart[(size_t)b * nparts + part] = s;
  }
  if constexpr (RATES) {
    if (tid < SPAD) {
      double s = 0.0;
      for (int ww = 0; ww < kGradWaves; ++ww) s += dg[(ww * NR + (tid >> 4)) * kWave + (tid & 15)];
      Dpart[((size_t)b * nparts + part) * SPAD + tid] = s;
    }
  }
}

// grid = batch * ceil(S S / 256), block = 256: one entry of grad per thread
// (every entry is written) and, in an evaluation's first block, its ll; the
// parts are added in part order
__global__ __launch_bounds__(256) void grad_finish_kernel(
    int S, int SPAD, int cap, int nparts, const int32_t* __restrict__ pos, const double* __restrict__ w01,
    const double* __restrict__ e_lo, const double* __restrict__ e_hi, const double* __restrict__ Mpart,
    const double* __restrict__ llpart, double* __restrict__ ll, double* __restrict__ grad) {
  const int nblk = (S * S + 255) / 256;
  const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk, tid = threadIdx.x;
  const int nr = SPAD / 16;
  const size_t pd = (size_t)nr * (nr + 1) / 2 * 256;
  const double* Mb = Mpart + (size_t)b * nparts * pd;
  if (blk == 0 && tid < kWave) {
    const double s = sum_partials(llpart + (size_t)b * nparts, nparts, tid);
    if (tid == 0) ll[b] = s;
  }
  const int32_t* pb = pos + (size_t)b * S;
  const int k = blk * 256 + tid;
  if (k < S * S) {
    const int i = k / S, j = k - i * S;
    const int q = clamp_pos(pb[i], S), p = clamp_pos(pb[j], S);
    double g = 0.0;
    if (p < q && (cap == 0 || q - p <= cap)) {
      const int rq = q >> 4, rp = p >> 4, c = q & 15, row = p & 15;
      const size_t om = (size_t)(rq * (rq + 1) / 2 + rp) * 256 + (row >> 2) * kWave + (row & 3) * 16 + c;
      const size_t orr = (size_t)(rq * (rq + 1) / 2 + rq) * 256 + 3 * kWave + 48 + c;
      double m = 0.0, r = 0.0;
      for (int t = 0; t < nparts; ++t) {
        m += Mb[t * pd + om];
        r += Mb[t * pd + orr];
      }
      const double w = w01[(size_t)b * S * S + k];
      g = fprime(w, e_lo[j]) * (r - m) + fprime(w, e_hi[j]) * m;
    }
    grad[(size_t)b * S * S + k] = g;
  }
}

// nemo_score_rates' finish, grid and grad as grad_finish_kernel with this
// evaluation's e^{B_j} / e^{-A_j} (rexp [b][2][S], prep_rates_kernel) in place
// of the staged e_lo / e_hi; ll gains sum_k A_k n_k (strided lane sums, then the
// xor tree).  One wave per gene k (blk * 4 + wave, + 4 nblk, ...): lane l takes
// the child at position pos[k] + 1 + l -- the children in order position --
//     dA_k = n_k - M_kk - sum_i h_ik M_ik,   dB_k = (R_k - M_kk) + sum_i k_ik (R_i - M_ik),
// h = w e^{-A_k} / fma(w, e^{-A_k}, 1 - w), k = w e^{B_k} / fma(w, e^{B_k}, 1 - w): the
// forward's own denominators.  R - M is a difference of two sums of the same
// non-negative terms, as in g_ij: its error is relative to R, which the
// tolerance carries.  drates [b][2][S]; grad may be null.
__global__ __launch_bounds__(256) void rates_finish_kernel(
    int S, int SPAD, int cap, int nparts, const int32_t* __restrict__ pos, const double* __restrict__ w01,
    const int32_t* __restrict__ permo, const double* __restrict__ rates, const double* __restrict__ rexp,
    const double* __restrict__ nk, const double* __restrict__ Mpart, const double* __restrict__ Dpart,
    const double* __restrict__ llpart, double* __restrict__ ll, double* __restrict__ drates,
    double* __restrict__ grad) {
  const int nblk = (S * S + 255) / 256;
  const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk, tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wv = tid / kWave;
  const int nr = SPAD / 16;
  const size_t pd = (size_t)nr * (nr + 1) / 2 * 256;
  const double* Mb = Mpart + (size_t)b * nparts * pd;
  const double* Db = Dpart + (size_t)b * nparts * SPAD;
  const double* ra = rates + (size_t)b * 2 * S;
  const double* eB = rexp + (size_t)b * 2 * S;
  const double* enA = eB + S;
  // M[q][p] (p < q) and R[q], the parts in order
  auto m_of = [&](int q, int p) {
    const int rq = q >> 4, rp = p >> 4, c = q & 15, row = p & 15;
    const size_t o = (size_t)(rq * (rq + 1) / 2 + rp) * 256 + (row >> 2) * kWave + (row & 3) * 16 + c;
    double m = 0.0;
    for (int t = 0; t < nparts; ++t) m += Mb[t * pd + o];
    return m;
  };
  auto r_of = [&](int q) {
    const int rq = q >> 4, c = q & 15;
    const size_t o = (size_t)(rq * (rq + 1) / 2 + rq) * 256 + 3 * kWave + 48 + c;
    double r = 0.0;
    for (int t = 0; t < nparts; ++t) r += Mb[t * pd + o];
    return r;
  };
  if (blk == 0 && tid < kWave) {
    double base = 0.0;
    for (int k = tid; k < S; k += kWave) base += ra[k] * nk[k];
    base = gwave_sum(base);
    const double s = sum_partials(llpart + (size_t)b * nparts, nparts, tid);
    if (tid == 0) ll[b] = s + base;
  }
  const int32_t* pb = pos + (size_t)b * S;
  const int k = blk * 256 + tid;
  if (grad && k < S * S) {
    const int i = k / S, j = k - i * S;
    const int q = clamp_pos(pb[i], S), p = clamp_pos(pb[j], S);
    double g = 0.0;
    if (p < q && (cap == 0 || q - p <= cap)) {
      const double m = m_of(q, p), r = r_of(q);
      const double w = w01[(size_t)b * S * S + k];
      g = fprime(w, eB[j]) * (r - m) + fprime(w, enA[j]) * m;
    }
    grad[(size_t)b * S * S + k] = g;
  }
  const int32_t* pm = permo + (size_t)b * SPAD;
  for (int gene = blk * 4 + wv; gene < S; gene += nblk * 4) {
    const int p = clamp_pos(pb[gene], S);
    const int q = p + 1 + lane;
    double ta = 0.0, tb = 0.0;
    if (q < S && (cap == 0 || q - p <= cap)) {
      const int i = pm[q];
      const double m = m_of(q, p), r = r_of(q);
      const double w = w01[((size_t)b * S + i) * S + gene];
      const double s1 = 1.0 - w;
      ta = w * enA[gene] / fma(w, enA[gene], s1) * m;
      tb = w * eB[gene] / fma(w, eB[gene], s1) * (r - m);
    }
    ta = gwave_sum(ta);
    tb = gwave_sum(tb);
    if (lane == 0) {
      double mkk = 0.0;
      for (int t = 0; t < nparts; ++t) mkk += Db[t * SPAD + p];
      drates[(size_t)b * 2 * S + gene] = nk[gene] - mkk - ta;
      drates[(size_t)b * 2 * S + S + gene] = (r_of(p) - mkk) + tb;
    }
  }
}

// ---------------------------------------------------------------------------
// two-pass: grid = batch * S (one child per block), one wave per parent in
// turn; lane sums over e = lane, lane + 64, ... then the xor tree
// ---------------------------------------------------------------------------
template <bool FACT>
__global__ __launch_bounds__(256) void grad_reduce_kernel(
    int S, int E, int cap, const int32_t* __restrict__ pos, const double* __restrict__ w01,
    const double* __restrict__ ow, const uint64_t* __restrict__ D1w, int nwords, const double* __restrict__ e_lo,
    const double* __restrict__ e_hi, const double* __restrict__ eT, double* __restrict__ grad) {
  const int b = blockIdx.x / S, i = blockIdx.x - b * S;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int32_t* pb = pos + (size_t)b * S;
  const int q = clamp_pos(pb[i], S);
  const double* orow = ow + ((size_t)b * (S + 1) + i) * E;
  for (int j = wv; j < S; j += 4) {
    const int p = clamp_pos(pb[j], S);
    const size_t k = ((size_t)b * S + i) * S + j;
    if (!(p < q && (cap == 0 || q - p <= cap))) {
      if (lane == 0) grad[k] = 0.0;
      continue;
    }
    const double w = w01[k];
    double g;
    if (FACT) {
      const uint64_t* bits = D1w + (size_t)j * nwords;
      double s_lo = 0.0, s_hi = 0.0;
      for (int e = lane; e < E; e += kWave) {
        const double o = orow[e];
        const bool hi = (bits[e >> 6] >> lane) & 1ull;
        s_hi += hi ? o : 0.0;
        s_lo += hi ? 0.0 : o;
      }
      g = fprime(w, e_lo[j]) * gwave_sum(s_lo) + fprime(w, e_hi[j]) * gwave_sum(s_hi);
    } else {
      const double* vrow = eT + ((size_t)i * S + j) * E;
      const double s1 = 1.0 - w;
      double s = 0.0;
      for (int e = lane; e < E; e += kWave) {
        const double v = vrow[e];
        s += orow[e] * ((v - 1.0) / fma(w, v, s1));
      }
      g = gwave_sum(s);
    }
    if (lane == 0) grad[k] = g;
  }
}

template <int NR, bool RATES>
hipError_t launch_fused_t(Ctx& c, int batch, hipStream_t st, const double* d_rates = nullptr) {
  constexpr int SPAD = NR * 16;
  const int ntiles = (c.E + 15) / 16;
  const int nparts = grad_parts(c.E);
  const size_t lds = (256 + 2 * 128 + kGradWaves) * 8 + (size_t)SPAD * (SPAD + 2) * 8 +
                     (size_t)(kGradWaves * kGradTilesPerWave / 4) * SPAD * 8 +
                     (RATES ? (size_t)(2 * SPAD + kGradWaves * NR * kWave) * 8 : 0);
  static_assert((256 + 2 * 128 + kGradWaves + 64 * 66 + (kGradWaves * kGradTilesPerWave / 4) * 64 + 2 * 64 +
                 kGradWaves * 4 * kWave) * 8 <= 65536, "the rates variant's LDS at NR = 4");
  score_grad_fused_kernel<NR, RATES><<<dim3(batch * nparts), kGradWaves * kWave, lds, st>>>(
      c.S, c.E, ntiles, nparts, c.d_fDp, c.d_fperm, RATES ? c.d_Dw : c.d_D1w, c.nwords,
      RATES ? nullptr : (const double*)c.d_U64, c.d_gradM, c.d_gradll, c.xcd_remap, d_rates, c.d_rdiag);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_score_grad_fused(Ctx& c, int batch, int cap, const int32_t* d_pos, const double* d_w01,
                                   double* d_ll, double* d_grad, hipStream_t st) {
  if (!c.factored || c.fspad > 64 || !c.d_gradM || !c.d_gradll) return hipErrorInvalidValue;
  if (cap >= c.S - 1) cap = 0;  // a cap that cuts nothing (same lists, same bits)
  hipError_t err = launch_prep_factored(c, batch, cap, d_pos, d_w01, st);
  if (err != hipSuccess) return err;
  switch (c.fspad / 16) {
    case 1: err = launch_fused_t<1, false>(c, batch, st); break;
    case 2: err = launch_fused_t<2, false>(c, batch, st); break;
    case 4: err = launch_fused_t<4, false>(c, batch, st); break;
    default: return hipErrorInvalidValue;
  }
  if (err != hipSuccess) return err;
  grad_finish_kernel<<<batch * ((c.S * c.S + 255) / 256), 256, 0, st>>>(c.S, c.fspad, cap, grad_parts(c.E), d_pos, d_w01, c.d_elo, c.d_ehi,
                                            c.d_gradM, c.d_gradll, d_ll, d_grad);
  return hipGetLastError();
}

hipError_t launch_score_rates(Ctx& c, int batch, int cap, const int32_t* d_pos, const double* d_w01,
                              const double* d_rates, double* d_ll, double* d_drates, double* d_grad,
                              hipStream_t st) {
  if (!rates_ready(c) || c.dtype != 0 || c.fspad > 64) return hipErrorInvalidValue;
  if (cap >= c.S - 1) cap = 0;  // a cap that cuts nothing (same lists, same bits)
  hipError_t err = launch_prep_rates(c, batch, cap, d_pos, d_w01, d_rates, st);
  if (err != hipSuccess) return err;
  switch (c.fspad / 16) {
    case 1: err = launch_fused_t<1, true>(c, batch, st, d_rates); break;
    case 2: err = launch_fused_t<2, true>(c, batch, st, d_rates); break;
    case 4: err = launch_fused_t<4, true>(c, batch, st, d_rates); break;
    default: return hipErrorInvalidValue;
  }
  if (err != hipSuccess) return err;
  rates_finish_kernel<<<batch * ((c.S * c.S + 255) / 256), 256, 0, st>>>(
      c.S, c.fspad, cap, grad_parts(c.E), d_pos, d_w01, c.d_fperm, d_rates, c.d_rexp, c.d_nk, c.d_gradM, c.d_rdiag,
      c.d_gradll, d_ll, d_drates, d_grad);
  return hipGetLastError();
}

hipError_t launch_grad_reduce(Ctx& c, int batch, int cap, bool factored, const int32_t* d_pos,
                              const double* d_w01, const double* d_ow, double* d_grad, hipStream_t st) {
  if (c.dtype != 0) return hipErrorInvalidValue;
  if (cap >= c.S - 1) cap = 0;
  if (factored)
    grad_reduce_kernel<true><<<batch * c.S, 256, 0, st>>>(c.S, c.E, cap, d_pos, d_w01, d_ow, c.d_D1w, c.nwords,
                                                          c.d_elo, c.d_ehi, nullptr, d_grad);
  else
    grad_reduce_kernel<false><<<batch * c.S, 256, 0, st>>>(c.S, c.E, cap, d_pos, d_w01, d_ow, nullptr, 0, nullptr,
                                                           nullptr, (const double*)c.d_eT, d_grad);
  return hipGetLastError();
}

}  // namespace nemo
