// Per-oracle track record (documentation/README.md:114 "replace only the worst oracle", :366-370 the reward
// score 1 - |c_i - e|^2 / max_i |c_i - e|^2), maintained after every committed round, host+device.
//
// Per instance b that ran (active[b] != 0) and committed (status[b] == OK):
//   rounds[b] += 1
//   u = (reliable[b][i] == 0):  flagged[b][i] += u;  streak[b][i] = u ? streak[b][i] + 1 : 0
//   score[b][i] += s_i, with qmax = max_i qr[b][i]
//     exact (qr int64, wsad):   s_i = WSAD - wsad_div(qr_i, qmax)      (track_score_exact)
//     fast  (qr fp32, 2^-32):   s_i = (int64)(clamp(1 - qr_i / qmax) * 2^32)   (track_score_fast)
// An inactive or reverted instance is not touched.  Every cell has one writer: no atomics.
#pragma once

#include <math.h>
#include <stdint.h>

#include "status.hpp"
#include "wsad.hpp"  // SVOC_HD, WSAD, u128

namespace svoc {

struct TrackUpdate {
  const uint8_t* active;    // [B]
  const int32_t* status;    // [B]
  const uint8_t* reliable;  // [B, N]
  const void* qr;           // [B, N] int64 (exact) / fp32 (fast)
  int32_t* rounds;          // [B]
  int32_t* flagged;         // [B, N]
  int32_t* streak;          // [B, N]
  int64_t* score;           // [B, N]
  int64_t B;
  int N;
  int exact;
};

constexpr int64_t kTrackFastOne = (int64_t)1 << 32;

// WSAD - wsad_div(q, qmax) (signed_decimal.cairo:114-116: trunc((a * 1e6 + b / 2) / b)).  q reaches 2^62, so
// the product needs 128 bits; below 2^43 everything fits in 64 and takes the cheap division.
// qmax <= 0 (every oracle at the centre, or a truncated i128 sum): WSAD; a negative q under a positive qmax: 0.
SVOC_HD int64_t track_score_exact(int64_t q, int64_t qmax) {
  if (qmax <= 0) return WSAD;
  if (q < 0) return 0;
  const uint64_t half = (uint64_t)qmax >> 1;
  if ((((uint64_t)q | (uint64_t)qmax) >> 43) == 0)
    return WSAD - (int64_t)(((uint64_t)q * (uint64_t)WSAD + half) / (uint64_t)qmax);
  const u128 num = (u128)(uint64_t)q * (u128)(uint64_t)WSAD + (u128)half;
  return WSAD - (int64_t)(num / (u128)(uint64_t)qmax);
}

// (int64)(clamp(1 - q / qmax, 0, 1) * 2^32): one correctly rounded division and one subtraction, so a float32
// model reproduces it bit for bit; the scaling by 2^32 is exact and the conversion truncates.
// qmax not a positive finite number: 2^32; then a non-finite q: 0.
SVOC_HD int64_t track_score_fast(float q, float qmax) {
  if (!(qmax > 0.f && qmax <= 3.402823466e+38f)) return kTrackFastOne;
  if (!(q >= -3.402823466e+38f && q <= 3.402823466e+38f)) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
  float s = __fsub_rn(1.f, __fdiv_rn(q, qmax));
#else
  float s = 1.f - q / qmax;   // (IEEE fp32 on the host: the same two roundings)
#endif
  s = s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
  return (int64_t)(s * 4294967296.f);
}

// the maximum that ignores NaN (all NaN, or N == 0: -inf)
SVOC_HD float track_fmax(float a, float b) { return (b > a || a != a) ? b : a; }

template <typename Q> SVOC_HD Q track_lowest();
template <> SVOC_HD int64_t track_lowest<int64_t>() { return INT64_MIN; }
template <> SVOC_HD float track_lowest<float>() { return -INFINITY; }

SVOC_HD int64_t track_max(int64_t a, int64_t b) { return a > b ? a : b; }
SVOC_HD float track_max(float a, float b) { return track_fmax(a, b); }

SVOC_HD int64_t track_score(int64_t q, int64_t qmax) { return track_score_exact(q, qmax); }
SVOC_HD int64_t track_score(float q, float qmax) { return track_score_fast(q, qmax); }

// one (instance, oracle) cell of a committed round
template <typename Q>
SVOC_HD void track_cell(const TrackUpdate& p, int64_t cell, Q q, Q qmax) {
  const int32_t u = p.reliable[cell] == 0;
  p.flagged[cell] += u;
  p.streak[cell] = u ? p.streak[cell] + 1 : 0;
  p.score[cell] += track_score(q, qmax);
}

// the scalar twin of track.hip (the CPU op; the kernel's reference)
template <typename Q>
SVOC_HD void track_update_one_t(const TrackUpdate& p, int64_t b) {
  if (p.active[b] == 0 || p.status[b] != ST_OK) return;
  const int64_t row = b * p.N;
  const Q* qr = (const Q*)p.qr + row;
  Q qmax = track_lowest<Q>();
  for (int i = 0; i < p.N; ++i) qmax = track_max(qmax, qr[i]);
  for (int i = 0; i < p.N; ++i) track_cell<Q>(p, row + i, qr[i], qmax);
  p.rounds[b] += 1;
}

SVOC_HD void track_update_one(const TrackUpdate& p, int64_t b) {
  if (p.exact) track_update_one_t<int64_t>(p, b);
  else track_update_one_t<float>(p, b);
}

}  // namespace svoc
