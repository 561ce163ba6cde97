// The once-per-instance decision of a fast round between pass 1 and pass 2: the two reliabilities
// (contract.cairo:365-368, 436-439) and the status ladder of the contract's asserts (:588-603), with the
// qr reduction that feeds them.  The ladder and its arithmetic are host code too: the CPU twin
// (engine/reference_cpu.cpp fast_round_one) and selftest/verdict_selftest.cpp call them.
#pragma once

#include <math.h>

#include "svoc/status.hpp"

#ifndef SVOC_HD
#if defined(__HIPCC__)
#define SVOC_HD __host__ __device__ __forceinline__
#else
#define SVOC_HD inline
#endif
#endif

namespace svoc {

// The two reliabilities of a round -- rel1 from the sum of qr over all N oracles, rel2 over the R reliable ones
// -- in the three arithmetic forms of the kernels.  They round differently and stay apart: a kernel's outputs
// are pinned bit for bit.  For a sum s over n oracles:
//   constrained:    1 - 2 sqrt(s / n / rd),  rd = the dimension (1 for the legacy contract)
//   unconstrained:  1 - min(max_spread, sqrt(s / n)) / max_spread
template <class T, class I>
SVOC_HD T rel_divisor(bool legacy, I rel_dim, I D) { return legacy ? (T)1 : (T)(rel_dim > 0 ? rel_dim : D); }

struct RelF32 {   // fp32 with divisions (consensus_fast_reg / _win)
  bool cons;
  float rd, ms;
  int N, R;
  SVOC_HD float of(float s, int n) const {
    return cons ? 1.f - 2.f * sqrtf(s / (float)n / rd) : 1.f - fminf(ms, sqrtf(s / (float)n)) / ms;
  }
  SVOC_HD float rel1(float s_all) const { return of(s_all, N); }
  SVOC_HD float rel2(float s_rel) const { return of(s_rel, R); }
};

// fp32 with reciprocals (consensus_fast_small).  The divisors are launch-uniform: one reciprocal each, formed up
// front, instead of a full-precision division per use (the divisions were ~20% of that kernel's VALU
// instructions; profiles/r2_pmc_c5.md).
struct RelF32Rcp {
  bool cons;
  float ms, inv_nrd, inv_rrd, inv_ms;
  int N, R;
  SVOC_HD RelF32Rcp(bool cons_, float rd, float ms_, int N_, int R_)
      : cons(cons_), ms(ms_), inv_nrd(1.f / ((float)N_ * rd)), inv_rrd(1.f / ((float)R_ * rd)), inv_ms(1.f / ms_),
        N(N_), R(R_) {}
  // Unconstrained, sd = sqrt(s / n).  Where the spread is clamped (sd >= ms) the contract's value is 1 - ms / ms = 0,
  // but 1 - ms * inv_ms is contracted to fma(-ms, inv_ms, 1): the exact residual of the rounded reciprocal, below
  // zero for every ms whose reciprocal rounds up (3, 5, 24, 0.3 ...) -- a RELIABILITY_INTERVAL revert of a round
  // the contract commits.  The clamped residual is floored at 0; every other value (NaN included) is as it was.
  SVOC_HD float unc(float sd) const {
    const float r = 1.f - fminf(ms, sd) * inv_ms;
    return sd >= ms && r < 0.f ? 0.f : r;
  }
  SVOC_HD float rel1(float s_all) const {
    return cons ? 1.f - 2.f * sqrtf(s_all * inv_nrd) : unc(sqrtf(s_all * (1.f / (float)N)));
  }
  SVOC_HD float rel2(float s_rel) const {
    return cons ? 1.f - 2.f * sqrtf(s_rel * inv_rrd) : unc(sqrtf(s_rel * (1.f / (float)R)));
  }
};

struct RelF64 {   // fp64 over the fp32 qr (consensus_fast_winf / _f32 and the CPU twin)
  bool cons;
  double rd, ms;
  int N, R;
  SVOC_HD float of(double mean_qr) const {
    return cons ? (float)(1.0 - 2.0 * sqrt(mean_qr / rd)) : (float)(1.0 - fmin(ms, sqrt(mean_qr)) / ms);
  }
  SVOC_HD float rel1(double s_all) const { return of(s_all / (double)N); }
  SVOC_HD float rel2(double s_rel) const { return of(s_rel / (double)R); }
};

struct Verdict {
  int status;
  float rel1, rel2;   // rel2 = 0 where the ladder ends before it
};

// The status ladder.  s_all / s_rel: the qr sums over all N rows / the R = N - f reliable ones; rel2 is evaluated
// only where R >= 2.  (R <= 0: consensus_fast_f32 and the CPU twin answer f > N with USIZE_UNDERFLOW before
// anything is computed, so they reach this with R >= 0 and the guard is their `R == 0`.)  NaN fails both
// interval checks.
template <class Rel, class S>
SVOC_HD Verdict round_verdict(const Rel& rel, S s_all, S s_rel, int R, bool legacy) {
  Verdict v{ST_OK, rel.rel1(s_all), 0.f};
  if (!(v.rel1 >= 0.f && v.rel1 <= 1.f)) v.status = ST_RELIABILITY_INTERVAL;
  else if (R < 2) v.status = R <= 0 ? ST_USIZE_UNDERFLOW : ST_INDEX_OOB;
  else {
    v.rel2 = rel.rel2(s_rel);
    if (!(v.rel2 >= 0.f && v.rel2 <= 1.f)) v.status = ST_RELIABILITY_INTERVAL;
    else if (R < 4 && !legacy) v.status = ST_TOO_FEW_RELIABLE;   // legacy: no moments
  }
  return v;
}

}  // namespace svoc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoc/launch.hpp"
#include "svoc/sortnet.hpp"

namespace svoc {

// Per-oracle qr from the waves' partials (MODE 2: the all-reduced qr of the D-sharded round) into qr_lds, rows
// past N zero.  MODE 1 ends here: this shard's qr partials out; true = the kernel returns.
template <int NT, int NPAD, int WAVES, int MODE>
SVOC_DEV bool reduce_qr(const FastParams& p, int b, int N, int tid, const float* qr_part, float* qr_lds) {
  for (int t = tid; t < NPAD; t += NT) {
    float q = 0.f;
    if (MODE == 2) {
      q = t < N ? p.qr[(int64_t)b * N + t] : 0.f;
    } else {
#pragma unroll
      for (int w = 0; w < WAVES; ++w) q += qr_part[w * NPAD + t];
    }
    qr_lds[t] = q;
  }
  __syncthreads();
  if (MODE == 1) {
    for (int t = tid; t < N; t += NT) p.qr[(int64_t)b * N + t] = qr_lds[t];
    if (tid == 0) p.status[b] = ST_OK;
    return true;
  }
  return false;
}

}  // namespace svoc
#endif
