// Which kernel runs a round, and what that kernel supports: pure functions of the round's shape, stated once.
// The .hip dispatchers switch on them, the torch bindings size their buffers and choose their fall-backs from
// them, and Python asks for them through the ops fast_route / exact_route (svoc.ops), so no kernel limit is
// written down anywhere else.  Plain C++: no HIP includes.
#pragma once

#include "svoc/launch.hpp"

namespace svoc {

// Lane groups of 64 oracles a column (pair) is spread over: 1, 2, 4, ... 64 for N <= 64, 128, 256, ... 4096.
inline int lane_groups(int N) {
  int g = 1;
  while (64 * g < N && g < 64) g *= 2;
  return g;
}

// ------------------------------------------------------------------------------------------------- fast rounds
enum FastStorage { kStoreBf16 = 0, kStoreF32 = 1 };
enum FastWork { kWorkNone = 0, kWorkCaller = 1, kWorkFresh = 2 };   // fresh: holds no pass-1 state
enum FastKernel { kFastSmall = 0, kFastWindow = 1, kFastTwoNet = 2 };

constexpr int kSmallMaxN = 16, kSmallMaxD = 128;     // consensus_fast_small.hip: several instances per wave
constexpr int kWindowMaxN = 256, kWindowMaxF = 32;   // consensus_fast_win.hip / _winf.hip
constexpr int kFusedMaxU = 256, kDeferMaxU = 127;    // piece map of the fused path (9 bits; 8 with a pending bit)

struct FastShape {
  int storage;   // FastStorage
  int N, D, ld;
  int n_failing, constrained;
  int legacy;    // (carried for completeness: no fast kernel's route depends on it)
  int mode;      // FastParams::mode
  int wave_hint;
  int work;      // FastWork: what the caller passes
};

struct FastRoute {
  int kernel;        // FastKernel
  int lane_groups;   // window / two-network kernel: its NSEG; small kernel: 0
  // the window kernel's half-width for this shape and workspace, 0 where it does not apply -- also stated where
  // another kernel is preferred (small instances, wave_hint -7), for direct callers of the window entry points
  int win_h;
  int needs_work;    // the kernel stages its outputs in the workspace: without the caller's, a fresh one is needed
  int pruned;        // the pruned window network runs (fp32, N = 256, H = 17)
  int rollback;      // the kernel rolls back a saved batch itself (FastParams.rst_saved)
  int fused_max_u;   // most updates per instance the fused path takes (FastParams.upd_rows); 0: not fused
  int defer_max_u;   // ... and the deferred commit (FastParams.pend_rows); 0: none
};

inline FastRoute fast_route(const FastShape& s) {
  FastRoute r{};
  const bool f32 = s.storage == kStoreF32;
  const bool small = !f32 && s.wave_hint == 0 && s.mode == 0 && s.N <= kSmallMaxN && s.D <= kSmallMaxD;
  r.needs_work = !small && s.mode != 1;
  const int work = s.work == kWorkNone && r.needs_work ? kWorkFresh : s.work;
  const bool win = work != kWorkNone && s.N >= 2 && s.N <= kWindowMaxN && s.D <= s.ld &&
                   (f32 ? (int64_t)s.N * s.ld * 4 < (1ll << 31) : s.ld % 8 == 0) &&   // 32-bit offsets; 16-B rows
                   !(s.mode == 2 && work == kWorkFresh) &&   // pass 1 ran elsewhere: no windows to read
                   s.n_failing >= 0 && s.n_failing <= kWindowMaxF && s.n_failing <= s.N - 2;
  r.win_h = win ? fast_win_h(s.N, s.n_failing) : 0;
  r.kernel = small ? kFastSmall : (r.win_h && s.wave_hint != -7) ? kFastWindow : kFastTwoNet;
  r.lane_groups = small ? 0 : lane_groups(s.N);
  if (r.kernel != kFastWindow || s.mode != 0) return r;
  r.rollback = !f32;
  r.pruned = f32 && s.constrained && s.N == 256 && r.win_h == 17;
  // fused streaming: the kernel's 32-bit batch offsets (U * D * 4 B) and 24-bit row-offset multiplies (ld * 4 B)
  if (f32 && s.constrained && s.D > 0 && (int64_t)s.ld * 4 < (1ll << 24)) {
    const int64_t fit = ((1ll << 31) - 1) / ((int64_t)s.D * 4);
    r.fused_max_u = (int)(fit < kFusedMaxU ? fit : kFusedMaxU);
    if (s.D % 4 == 0) r.defer_max_u = r.fused_max_u < kDeferMaxU ? r.fused_max_u : kDeferMaxU;   // 16-B write-back
  }
  return r;
}

inline FastShape fast_shape(const FastParams& p, int storage) {
  return {storage, p.N, p.D, p.ld, p.n_failing, p.constrained, p.legacy, p.mode, p.wave_hint,
          !p.work ? kWorkNone : p.work_fresh ? kWorkFresh : kWorkCaller};
}

// ------------------------------------------------------------------------------- rank-weighted (L-estimator) rounds
// consensus_fast_lest.hip: a weight per rank instead of the smooth median's middle pair.  fp32 storage, whole rounds,
// the current contract only; every rank of a column is sorted, at 64 rows per lane and at most 4 lanes per column.
constexpr int kLestMaxN = 256;

struct LestRoute {
  int supported;     // the kernel takes this shape
  int lane_groups;   // its NSEG: 1 / 2 / 4
  int max_n;         // kLestMaxN
  int needs_work;    // it stages its outputs in the workspace (always)
};

inline LestRoute lest_route(const FastShape& s) {
  LestRoute r{};
  r.max_n = kLestMaxN;
  r.needs_work = 1;
  r.lane_groups = lane_groups(s.N);
  r.supported = s.storage == kStoreF32 && s.N >= 2 && s.N <= kLestMaxN && s.D >= 1 && s.D <= s.ld &&
                s.n_failing >= 0 && s.n_failing <= s.N - 2 && s.mode == 0 && !s.legacy &&
                (int64_t)s.N * s.ld * 4 < (1ll << 31);   // 32-bit buffer offsets, as fast_route
  return r;
}

// ------------------------------------------------------------------------------------------------ exact rounds
constexpr int kWsadMinD = 64;   // fewest columns the column kernel takes for N <= 32 (one lane per column)

struct ExactShape {
  int N, D, elem_bytes;   // 8: int64 wsad, 4: int32
  int n_failing, constrained, legacy;
  int mode;               // ExactParams::mode
  int wsad_min_d;         // ExactParams::wsad_min_d
  int force_i128;         // the i128 kernel everywhere (tests, A/B)
};

struct ExactRoute {
  int column;        // the column-parallel kernel applies (consensus_wsad.hip); else the i128 kernel alone
  int lane_groups;   // 1 / 2 / 4: the window-capable groups; 8 .. 64: the wide groups (two networks)
  int win_h;         // exact_win_h of a whole constrained round (the stage holds 4 + 2 win_h rows)
  int verdict;       // the verdict form of the column kernel applies (svoc_exact_verdict)
};

inline ExactRoute exact_route(const ExactShape& s) {
  ExactRoute r{};
  r.lane_groups = lane_groups(s.N);
  // lane = column: with few columns most lanes idle, and for N <= 32 the i128 kernel packs 2-8 instances per
  // wave instead (profiles/r2_exact_crossover.json: 7 x 6 140 M vs 10 M rounds/s, 16 x 16 27 M vs 10 M; but
  // 64 x 16 already 8.3 M vs 6.0 M for the column kernel)
  r.column = !s.force_i128 && s.N >= 4 && s.N <= 4096 &&
             !(r.lane_groups > 4 && s.mode != 0 && !s.constrained) &&   // wide groups: D-sharded halves constrained
             !(s.N <= 32 && s.D < s.wsad_min_d) &&
             (int64_t)s.N * s.D * s.elem_bytes < (1ll << 31);            // 32-bit buffer offsets
  if (!r.column) return r;
  const bool whole = s.mode == 0 && s.constrained && !s.legacy;
  r.win_h = whole ? exact_win_h(s.N, s.n_failing) : 0;
  r.verdict = whole && r.lane_groups <= 4;
  return r;
}

inline ExactShape exact_shape(const ExactParams& p, int force_i128 = 0) {
  return {p.N, p.D, p.val32 ? 4 : 8, p.n_failing, p.constrained, p.legacy, p.mode, p.wsad_min_d, force_i128};
}

}  // namespace svoc
