// nemo_reloc_math.h -- the step arithmetic of a relocation walk,
// shared by the relocation scores (nemo_reloc.hip) and the order sweep
// (nemo_order_sweep.hip): the log of a factor, the sum's factor of a passed node
// and log(1 + X) without an overflowing exp.
#pragma once

#include "nemo_internal.h"

#include <math.h>

namespace nemo {

// log f for f = 1 - w + w v, v = e^T > 0: relative to itself where f is near 1
// (the series of log1p_fast on x = w (v - 1)), log_fast's ulp of max(|log f|,
// 0.5) elsewhere
__device__ __forceinline__ double log_factor(double w, double v, const double2* __restrict__ ltab) {
  const double x = w * (v - 1.0);
  double p = fma(x, -1.0 / 6.0, 0.2);
  p = fma(x, p, -0.25);
  p = fma(x, p, 1.0 / 3.0);
  p = fma(x, p, -0.5);
  p = fma(x, p, 1.0);
  p *= x;
  const double big = log_fast(fmax(fma(w, v, 1.0 - w), 0x1p-1022), ltab);
  return fabs(x) < 0x1p-8 ? p : big;
}

// the sum's factor of node m when a leaves its parents (up: 1 / f_ma - 1) or
// joins them (f_ma - 1), without the cancellation of either difference
__device__ __forceinline__ double sum_factor(bool up, double w, double v) {
  const double d = w * (v - 1.0);
  return up ? -d / fmax(fma(w, v, 1.0 - w), 0x1p-1022) : d;
}

// log(1 + X), X = sumv + e^y, sumv = -ow[a] + sum_m ow[m] c_m: one table exp of
// -|y| and one log1p
__device__ __forceinline__ double reloc_term(double sumv, double y, const double* __restrict__ etab,
                                             const double2* __restrict__ ltab) {
  const double ey = exp_lse(-fabs(y), etab);
  const bool pos = y > 0.0;
  const double x = pos ? (1.0 + sumv) * ey : sumv + ey;
  const double r = log1p_fast(x, ltab);
  return pos ? y + r : r;
}

}  // namespace nemo
