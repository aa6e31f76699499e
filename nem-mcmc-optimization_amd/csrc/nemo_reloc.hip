// nemo_reloc.hip -- the exact score change of every single-node relocation of
// an order.
//
// Fix a full weight matrix W: W[i][j] is the weight pair (i, j) carries whenever
// j precedes i.  Moving node a from position p to position q changes only these
// rows of the cells: for q > p the nodes m at positions p+1 .. q lose parent a
// and a gains them all; for q < p the nodes m at positions q .. p-1 gain parent
// a and a loses them all.  With f_ij(e) = 1 - w_ij + w_ij e^{T[i][j][e]}, z =
// cell - cs and ow = exp(z),
//     ll(a moved to q) - ll = sum_e log(1 + X_aq(e)),
//     q > p:  X = -ow[a] + sum_m ow[m] (1 / f_ma - 1) + exp(z_a + sum_m log f_am)
//     q < p:  X = -ow[a] + sum_m ow[m] (f_ma - 1)     + exp(z_a - sum_m log f_am)
// and both the sum and the exponent grow by one term per step away from p: the
// S - 1 targets of a node are one walk.  The gained and lost factors of a are
// carried as a sum of logs on top of z_a (never as a running product, which
// leaves fp64 at (S - 1) max|T| past 709), and where y = z_a +- sum log f is
// positive the log is formed as y + log1p((1 + sum) e^{-y}): no exp overflows.
//
// One path serves every model (factored at every S, generic and row-shared
// tables): the existing two-pass forward leaves the cells and cs in HBM and
// reloc_reduce_kernel, one block per (evaluation, node), walks with its lanes
// over the effects and a gwave_sum per step.  (A fused kernel on the forward of
// nemo_grad_fwd.h, a wave's halves walking node p up and node S - 1 - p down,
// was built and measured: never faster than this path)
//
// Every sum has a fixed order that depends on the staged model alone.
#include "nemo_grad_fwd.h"
#include "nemo_internal.h"
#include "nemo_reloc_math.h"

#include <math.h>

namespace nemo {

namespace {

// ---------------------------------------------------------------------------
// grid = batch * S (one node a per block), 4 waves.  Wave wv takes the
// effects wv * 64 + lane + 256 k and walks both directions for each; a step's
// terms are summed over the wave (gwave_sum) and added to the wave's running sum
// of the step's target position, effects ascending; the four waves' sums are
// added in wave order.  cells [batch][S+1][E], cs [batch][E].
// ---------------------------------------------------------------------------
template <bool FACT>
__global__ __launch_bounds__(256) void reloc_reduce_kernel(
    int S, int E, const int32_t* __restrict__ pos, const double* __restrict__ w01,
    const double* __restrict__ cells, const double* __restrict__ cs, const uint64_t* __restrict__ D1w, int nwords,
    const double* __restrict__ e_lo, const double* __restrict__ e_hi, const double* __restrict__ eT,
    double* __restrict__ dll) {
  __shared__ double2 ltab[128];
  __shared__ double etab[256];
  __shared__ int perm[kMaxS];
  __shared__ double ctab[kMaxS * 4];  // by position: FACT the four pair constants, else w_ma, w_am
  __shared__ double accw[4][kMaxS];
  const int tid = threadIdx.x;
  fill_log_table(ltab, tid, blockDim.x);
  etab[tid] = exp2((double)tid * (1.0 / 256.0));
  const int b = blockIdx.x / S, a = blockIdx.x - b * S;
  const int lane = tid & (kWave - 1), wv = tid / kWave;
  const int32_t* pb = pos + (size_t)b * S;
  if (tid < S) perm[tid] = 0;
  for (int k = tid; k < 4 * kMaxS; k += 256) (&accw[0][0])[k] = 0.0;
  __syncthreads();
  if (tid < S) perm[clamp_pos(pb[tid], S)] = tid;
  __syncthreads();
  const int p = clamp_pos(pb[a], S);
  const double* wb = w01 + (size_t)b * S * S;
  if (tid < S && tid != p) {
    const int m = perm[tid];
    const bool up = tid > p;
    const double w_ma = wb[(size_t)m * S + a], w_am = wb[(size_t)a * S + m];
    if (FACT) {
      const double l0 = log_factor(w_am, e_lo[m], ltab), l1 = log_factor(w_am, e_hi[m], ltab);
      ctab[4 * tid + 0] = sum_factor(up, w_ma, e_lo[a]);
      ctab[4 * tid + 1] = sum_factor(up, w_ma, e_hi[a]);
      ctab[4 * tid + 2] = up ? l0 : -l0;
      ctab[4 * tid + 3] = up ? l1 : -l1;
    } else {
      ctab[4 * tid + 0] = w_ma;
      ctab[4 * tid + 1] = w_am;
    }
  }
  __syncthreads();
  const double* cb = cells + (size_t)b * (S + 1) * E;
  const double* csb = cs + (size_t)b * E;
  for (int e0 = wv * kWave; e0 < E; e0 += 4 * kWave) {  // wave-uniform
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
          cf = ctab[4 * q + abit];
          lf = ctab[4 * q + 2 + mbit];
        } else {
          const double w_ma = ctab[4 * q], w_am = ctab[4 * q + 1];
          cf = sum_factor(up, w_ma, eT[((size_t)m * S + a) * E + ec]);
          lf = log_factor(w_am, eT[((size_t)a * S + m) * E + ec], ltab);
          lf = up ? lf : -lf;
        }
        sumv = fma(owm, cf, sumv);
        y += lf;
        const double term = gwave_sum(valid ? reloc_term(sumv, y, etab, ltab) : 0.0);
        if (lane == 0) accw[wv][q] += term;
      }
    }
  }
  __syncthreads();
  if (tid < S)
    dll[((size_t)b * S + a) * S + tid] =
        tid == p ? 0.0 : ((accw[0][tid] + accw[1][tid]) + accw[2][tid]) + accw[3][tid];
}

// (option timing_kernel 4) the events around the relocation kernels of one call
struct RelocTimer {
  Ctx& c;
  hipStream_t st;
  hipEvent_t e1 = nullptr;
  hipError_t begin() {
    if (!(c.timing && c.timing_kernel == 4 && c.ev_used + 2 <= c.ev_pool.size())) return hipSuccess;
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

hipError_t launch_reloc_reduce(Ctx& c, int batch, bool factored, const int32_t* d_pos, const double* d_w01,
                               const double* d_cells, const double* d_cs, double* d_dll, hipStream_t st) {
  if (c.dtype != 0 || c.S > kMaxS) return hipErrorInvalidValue;
  RelocTimer tm{c, st};
  hipError_t err = tm.begin();
  if (err != hipSuccess) return err;
  if (factored)
    reloc_reduce_kernel<true><<<batch * c.S, 256, 0, st>>>(c.S, c.E, d_pos, d_w01, d_cells, d_cs, c.d_D1w, c.nwords,
                                                           c.d_elo, c.d_ehi, nullptr, d_dll);
  else
    reloc_reduce_kernel<false><<<batch * c.S, 256, 0, st>>>(c.S, c.E, d_pos, d_w01, d_cells, d_cs, nullptr, 0,
                                                            nullptr, nullptr, (const double*)c.d_eT, d_dll);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  return tm.end();
}

}  // namespace nemo
