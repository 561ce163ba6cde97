// Exact UNCONSTRAINED rounds over wide columns (VERDICT r5 missing item 1): the instances the column
// kernel (consensus_wsad.hip) hands on because a column's values spread more than 2^30 wsad (1,073 real
// units) around its row-0 base -- price-like columns of 60,000 +- 20,000 units, or a failing oracle's draw
// five standard deviations out -- before they reach the i128 kernel (consensus_exact.hip), which is ~100x
// slower at the c2 shape.  Bit-identical to the i128 kernel and to the CPU golden engine
// (csrc/engine/reference_cpu.cpp exact_round_one) on every round it commits.
//
// Semantics: contract/src/contract.cairo:370-434 (update_unconstrained_consensus) in the arithmetic of
// signed_decimal.cairo:52-116 and math.cairo:113-398: pass 1 smooth median (math.cairo:113-126), quadratic
// risk (math.cairo:225-238), the unconstrained reliability (contract.cairo:365-368), the rank cut
// (sort.cairo:96-101 tie rule, contract.cairo:345-363), pass 2 the reliable mean (math.cairo:240-254),
// rel2 from the reliable rows' qr, then variance / sqrt / z-scores / skewness / kurtosis (math.cairo:208-222,
// 271-292, 320-398).
//
// Layout: one workgroup per instance (4 waves), N <= 64 (64 < N <= 256: consensus_wsadx_groups.hip, 2 / 4 lanes
// per column), a lane owns one column per slab (the column kernel's NSEG = 1 layout), values taken relative to the
// column's row-0 value B as int64.  Domain (else
// the i128 kernel): |x| < 2^62 and |x - B| < 2^37 (137,438 real units), so that
//   - the pass-1 keys are exact doubles (the 64-key odd-even merge network of sortnet.hpp on v_min/max_f64,
//     pruned by dead-code elimination to the median pair),
//   - every deviation d from c1 or from the mean is below 2^38 and qdev(d) = floor((d^2 + 500000) / 1e6) <
//     2^56.1: the fp64 double-double square and a remainder-corrected quotient (qdev_dd),
//   - the per-oracle qr sums (transposing butterfly over the wave's 64 columns, then across waves and slabs)
//     stay in uint64 -- a carry out of any sum hands the instance to the i128 kernel,
//   - the variance (< 2^56.1) takes the contract's Newton sqrt with 128-bit dividends v 1e6 + g / 2 done as an
//     fp64 estimate plus the exact remainder modulo 2^64 (wsqrt_x), and z = wsad_div(d, sd) has an int64
//     dividend d 1e6 + sd / 2 < 2^58 (wdiv_z: reciprocal estimate, exact remainder) and, on the reliable rows,
//     |z| < 2^31 -- the other rows' deviations are cleared before the division (wdiv_z_masked); z^2, z^3, z^4
//     take the half-offset fp64 products of wsad_fast.hpp (int64 for the rare z^2 >= 2^25).
// The arithmetic named here lives in svoc/wsad_wide.hpp, host and device, and is checked against the i128
// routines by the host self-test (csrc/selftest/engine_selftest.cpp wsadx_paths).
// The kernel commits only rounds that succeed; anything else (a reliability outside [0, 1], R < 4, a
// zero-variance column, a value outside the domain) stays flagged and the i128 kernel computes it, status
// included.  Pass 2 runs in two sweeps (means and sqrt into the staging buffer, checked; then the moments and
// the outputs), so a round that would revert never touches the outputs.  The halves of a D-sharded round
// (svoc/parallel/dshard.py) are the MODE 1 / 2 instantiations below, with the same rule: a half is done whole or
// stays flagged.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "svoc/bufload.hpp"
#include "svoc/launch.hpp"
#include "svoc/sortnet.hpp"
#include "svoc/status.hpp"
#include "svoc/wsad.hpp"
#include "svoc/wsad_fast.hpp"
#include "svoc/wsad_wide.hpp"

namespace svoc {


// 64-row odd-even merge sort on exact double keys (the shared comparator table of sortnet.hpp)
SVOC_DEV void sort64_f64(double (&r)[64]) {
  constexpr CmpNet<64> T = make_oem<64>();
#pragma unroll
  for (int c = 0; c < T.n; ++c) {
    const double x = r[T.a[c]], y = r[T.b[c]];
    r[T.a[c]] = __builtin_fmin(x, y);
    r[T.b[c]] = __builtin_fmax(x, y);
  }
}

template <int M>
SVOC_DEV uint64_t xor_lane_u64(uint64_t v) {
  const uint32_t lo = xor_lane_u32<M>((uint32_t)v), hi = xor_lane_u32<M>((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
// Transposing butterfly over the wave's 64 columns: lane l ends with the sum of row l over the 64 columns.
// `ovf` collects a carry out of any partial sum.
template <int MSK, int H>
SVOC_DEV void qr_fold(uint64_t (&q)[64], int lane, bool& ovf) {
  if constexpr (MSK >= 1) {
    const bool up = (lane & MSK) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const uint64_t lo_v = q[i], hi_v = q[i + H];
      const uint64_t send = up ? lo_v : hi_v, keep = up ? hi_v : lo_v;
      const uint64_t s = keep + xor_lane_u64<MSK>(send);
      ovf = ovf || s < keep;
      q[i] = s;
    }
    qr_fold<MSK / 2, H / 2>(q, lane, ovf);
  }
}

template <bool V32>
SVOC_DEV int64_t xload(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  if constexpr (V32) {
    return (int64_t)(int32_t)bload(rs, voff, soff);
  } else {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0);
    return (int64_t)(((uint64_t)v[1] << 32) | v[0]);
  }
}

// a double whose bits are blended by an all-ones / zero lane mask (no compare, no SGPR mask)
SVOC_DEV double dblend(double a, double b, uint32_t m) {   // m ? a : b
  const uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
  const uint64_t mm = ((uint64_t)m << 32) | m;
  return __builtin_bit_cast(double, (ua & mm) | (ub & ~mm));
}

// FULLN: N = 64 (every row real, no row masks: the c2 shape); otherwise rows >= N are masked arithmetically
// MODE (launch.hpp ExactParams::mode, the halves of a D-sharded round as the i128 kernel splits it): 0 the whole
// round.  1: pass 1 over this shard's columns -- c1 (staged, written only with the rest) and the per-oracle qr
// PARTIALS, each below kExactQrPartialMax, status OK; anything else (out of the domain, a carry, a partial at 2^58)
// stays flagged and writes nothing.  2: the all-reduced qr comes in (each below 2^62, else flagged), then the rank
// mask, the reliabilities and pass 2 as in a whole round; no pass 1 has validated the values, so pass 2a checks the
// domain over every row < N itself, before its sqrt and long before the z division of pass 2b.
template <bool V32, bool FULLN, int MODE = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void consensus_wsadx_kernel(ExactParams p, int handle) {
  constexpr int NT = 256, WAVES = 4, W = WAVES * 64;
  constexpr int ESZ = V32 ? 4 : 8;
  __shared__ uint64_t qr_part[WAVES][64];
  __shared__ uint64_t qr_lds[64];
  __shared__ uint64_t relmask;
  __shared__ int64_t rels[2];
  __shared__ int flag;

  const int b = blockIdx.x;
  if (!p.fallback[b]) return;   // (the column kernel took it, or the instance is inactive)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!handle) {   // (counting only: rounds left to the i128 kernel)
    if (tid == 0 && p.xstats) atomicAdd(&p.xstats[1], 1u);
    return;
  }
  if constexpr (MODE == 2) {   // a shard's first half failed: the round reverts everywhere, nothing to compute
    if (p.status[b] != ST_OK) {
      if (tid == 0) p.fallback[b] = 0;
      return;
    }
  }
  const int N = FULLN ? 64 : p.N, D = p.D;
  const int rowb = D * ESZ;
  const __amdgpu_buffer_rsrc_t rs =
      instance_rsrc((const unsigned char*)p.values + (int64_t)b * N * rowb, (uint32_t)(N * rowb));
  const int64_t ob = (int64_t)b * D;
  // the staging buffer (int32 [SROWS = 6][D]: this kernel's per-column mean / sd as int64 word pairs)
  int32_t* const stg = p.stage + (int64_t)b * 6 * D;
  if (tid == 0) flag = 0;
  uint64_t oob = 0;   // out-of-domain bits (or a carry out of a qr sum)
  const int nslab = (D + W - 1) / W;
  const int lo1 = (64 - N + 1) >> 1;   // sentinel split: the middle of the padded sort = the middle of the rows

  // ------------------------------------------------------------ pass 1 (contract.cairo:383-395)
  uint64_t acc = 0;   // row `lane`'s qr over the wave's columns
  for (int s = 0; s < (MODE == 2 ? 0 : nslab); ++s) {   // (mode 2: no pass 1, the all-reduced qr is read below)
    const int col = s * W + wave * 64 + lane;
    const bool vc = col < D;
    const int vo = (vc ? col : 0) * ESZ;
    const uint32_t mc = vc ? 0xffffffffu : 0u;
    const int64_t B = xload<V32>(rs, vo, 0);
    // (an opaque row stride and row count per slab: the 64 row offsets / masks are recomputed, not hoisted out of
    // the loop as 64 live SGPRs that spill to VGPR lanes)
    int rowb1 = rowb, n1 = N, nl1 = N + lo1;
    asm volatile("" : "+s"(rowb1), "+v"(n1), "+v"(nl1));
    int64_t c1r;
    // domain: |B| < 2^61 and |x - B| < 2^37 (so |x| < 2^62 and x - B cannot wrap); rows past N read row 0: r = 0
    double rmax = 0.0;
    oob |= (vc && (uint64_t)(B + (1ll << 61)) >= (1ull << 62)) ? 1ull : 0ull;
    {
      double k[64];
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        const int64_t x = xload<V32>(rs, vo, (FULLN || i < N ? i : 0) * rowb1);   // (row 0 again past N: masked)
        const double rd = (double)(x - B);   // (exact while |x - B| < 2^53; the domain check below)
        rmax = __builtin_fmax(rmax, __builtin_fabs(rd));
        if (FULLN) {
          k[i] = rd;
        } else {   // rows N .. N + lo1 - 1: -inf, then +inf
          k[i] = dblend(rd, dblend(-INFINITY, INFINITY, lt_mask(i, nl1)), lt_mask(i, n1));
        }
      }
      oob |= (vc && !(rmax < 137438953472.0)) ? 1ull : 0ull;   // 2^37
      sort64_f64(k);
      // smooth median (math.cairo:113-126): I128Div(s[N/2 - 1] + s[N/2], 2) on the absolute values (|B| < 2^61:
      // the sum fits int64; C's division truncates toward zero, as I128Div)
      const int64_t c1a = ((B + (int64_t)k[31]) + (B + (int64_t)k[32])) / 2;
      c1r = c1a - B;
      if constexpr (MODE == 1) {   // (p.c1 is the output itself: staged here, written where the half succeeds)
        if (vc) {
          stg[col] = (int32_t)(uint32_t)c1a;
          stg[D + col] = (int32_t)(uint32_t)((uint64_t)c1a >> 32);
        }
      } else {
        if (vc) p.c1[ob + col] = c1a;   // (mode 0: the staged c1, committed where the round succeeds)
      }
    }
    // quadratic risk (math.cairo:225-238): qdev(x, c1) of every row, summed over the columns.  (The re-read's
    // offset depends on c1 through an empty asm: otherwise the loads are hoisted above the network and 128 more
    // VGPRs are live across it.)
    uint64_t q[64];
    const double c1d = (double)c1r;
    int vo2 = vo;
    asm volatile("" : "+v"(vo2) : "v"(c1r));
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const int64_t r = xload<V32>(rs, vo2, (FULLN || i < N ? i : 0) * rowb1) - B;
      const uint32_t m = FULLN ? mc : (mc & lt_mask(i, n1));
      q[i] = qdev_dd((double)r - c1d) & (((uint64_t)m << 32) | m);
    }
    bool ovf = false;
    qr_fold<32, 32>(q, lane, ovf);
    const uint64_t t = acc + q[0];
    oob |= (ovf || t < acc) ? 1ull : 0ull;
    acc = t;
  }
  qr_part[wave][lane] = acc;
  if (oob) flag = 1;
  __syncthreads();
  if (tid < 64) {
    uint64_t v = 0;
    bool o = false;
    if constexpr (MODE == 2) {   // the all-reduced qr (int64; a negative one reads as >= 2^63)
      v = tid < N ? (uint64_t)p.qr[(int64_t)b * N + tid] : 0ull;
    } else {
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        const uint64_t u = v + qr_part[w][tid];
        o = o || u < v;
        v = u;
      }
    }
    // (int64 qr, i128 sums below; mode 1: a partial the all-reduce of 32 shards could not hold)
    if (o || v >= (MODE == 1 ? (uint64_t)kExactQrPartialMax : (1ull << 62))) flag = 1;
    qr_lds[tid] = v;
  }
  __syncthreads();
  if constexpr (MODE == 1) {   // first half done: c1 and the qr partials out, nothing else
    if (flag) {
      if (tid == 0 && p.xstats) atomicAdd(&p.xstats[1], 1u);
      return;
    }
    for (int s = 0; s < nslab; ++s) {   // (each lane reads back the columns it staged)
      const int col = s * W + wave * 64 + lane;
      if (col < D)
        p.c1[ob + col] = (int64_t)(((uint64_t)(uint32_t)stg[D + col] << 32) | (uint32_t)stg[col]);
    }
    for (int t = tid; t < N; t += NT) p.qr[(int64_t)b * N + t] = (int64_t)qr_lds[t];
    if (tid == 0) {
      p.status[b] = ST_OK;
      p.fallback[b] = 0;
      if (p.xstats) atomicAdd(&p.xstats[0], 1u);
    }
    return;
  }

  // ------------------------------------------------------------ rank mask (contract.cairo:345-363)
  const int f = p.n_failing;
  const int R = N - f;
  if (tid < 64) {
    bool rel = false;
    if (tid < N) {
      const uint64_t myq = qr_lds[tid];
      int rank = 0;
      for (int j = 0; j < N; ++j) {
        const uint64_t qj = qr_lds[j];
        rank += (qj < myq || (qj == myq && j > tid)) ? 1 : 0;   // (qr asc, idx desc)
      }
      rel = rank < R;
    }
    const uint64_t bal = __ballot(rel);
    if (tid == 0) relmask = bal;
  }
  if (tid == 0 && (MODE != 2 || !flag)) {   // (mode 2: only below 2^62, wsqrt_x's precondition)
    // reliabilities (contract.cairo:365-368) with the wsad.hpp routines; every revert goes to the i128 kernel,
    // which reports the stage-ordered status
    // (the means of the qr are below 2^62: the contract's sqrt in the int64 / fp64-estimate form, wsqrt_x)
    int st = ST_OK;
    i128 s_all = 0, s_rel = 0;
    for (int t = 0; t < N; ++t) {
      const i128 qv = (i128)qr_lds[t];
      s_all += qv;
      if ((relmask >> t) & 1) s_rel += qv;
    }
    int64_t sd1 = 0, sd2 = 0;
    bool ok = f >= 0 && R >= 4 && !p.legacy && p.max_spread > 0 && wsqrt_x((int64_t)idiv_pos64(s_all, N, st), sd1);
    const i128 rel1 = ok ? unconstrained_reliability(sd1, (i128)p.max_spread, st) : 0;
    ok = ok && st == ST_OK && in_unit_interval(rel1) && wsqrt_x((int64_t)idiv_pos64(s_rel, R, st), sd2);
    i128 rel2 = 0;
    if (ok) {
      rel2 = unconstrained_reliability(sd2, (i128)p.max_spread, st);
      ok = st == ST_OK && in_unit_interval(rel2);
    }
    rels[0] = (int64_t)rel1;
    rels[1] = (int64_t)rel2;
    if (!ok) flag = 1;
  }
  __syncthreads();
  if (flag) {
    if (tid == 0 && p.xstats) atomicAdd(&p.xstats[1], 1u);
    return;
  }

  // ------------------------------------------------------------ pass 2a: means, variances, sqrt
  const uint64_t rm = relmask;   // (only rows < N are set)
  bool bad = false;
  // (the per-instance divisors are recomputed in each slab loop: live across the whole kernel they held 16 VGPRs)
  for (int s = 0; s < nslab; ++s) {
    const int col = s * W + wave * 64 + lane;
    const bool vc = col < D;
    const int vo = (vc ? col : 0) * ESZ;
    const int64_t B = xload<V32>(rs, vo, 0);
    int rowb1 = rowb;
    uint64_t rm1 = rm;
    asm volatile("" : "+s"(rowb1), "+v"(rm1));
    // the reliable mean (math.cairo:240-254): I128Div of the absolute sum by R (the relative sum is exact in
    // fp64: below 64 * 2^37).  The column is read twice (sum, then variance) rather than held: 64 doubles live across
    // the variance loop pushed the kernel past 256 VGPRs (scratch in this loop)
    double Sd = 0.0;
    double rmax = 0.0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const int64_t x = xload<V32>(rs, vo, (FULLN || i < N ? i : 0) * rowb1);
      const double rd = (double)(x - B);
      if constexpr (MODE == 2) rmax = __builtin_fmax(rmax, __builtin_fabs(rd));   // (rows past N read row 0: 0)
      Sd += dblend(rd, 0.0, bit_mask(rm1, i));
    }
    if constexpr (MODE == 2) {
      // the domain of pass 1, over every row: |B| < 2^61 and |x - B| < 2^37.  Outside it the column's sum and mask
      // are cleared, so the mean is 0, the variance 0 and its sqrt returns at once; the instance is flagged below
      const bool od = (uint64_t)(B + (1ll << 61)) >= (1ull << 62) || !(rmax < 137438953472.0);
      if (od) {
        Sd = 0.0;
        rm1 = 0;
      }
      bad = bad || (vc && od);
    }
    const double Rd = (double)R, invR = recip_lo(Rd);
    // trunc((R B + S) / R) - B from trunc(S / R) (wsad_fast.hpp tdiv_rel_fix: no R B product)
    const double qd = trunc_div_d(Sd, Rd, invR);
    const int64_t mur = tdiv_rel_fix((int64_t)qd, fma(-qd, Rd, Sd) == 0.0, Sd < 0.0, B);
    const double mud = (double)mur;
    // population variance (math.cairo:208-222): floor of the mean qdev (non-negative)
    int vo2 = vo;
    asm volatile("" : "+v"(vo2) : "v"(mur));   // (the re-read after the mean, not hoisted above it)
    uint64_t sv = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const int64_t x = xload<V32>(rs, vo2, (FULLN || i < N ? i : 0) * rowb1);
      const uint32_t m = bit_mask(rm1, i);
      sv += qdev_dd((double)(x - B) - mud) & (((uint64_t)m << 32) | m);
    }
    int64_t var = (int64_t)((double)sv * invR);   // floor(sv / R): an estimate, fixed by the exact remainder
    int64_t vr = (int64_t)sv - var * R;
    while (vr < 0) { --var; vr += R; }
    while (vr >= R) { ++var; vr -= R; }
    int64_t sd = 0;
    const bool ok = wsqrt_x(var, sd) && sd != 0;   // sqrt(0) -> wsad_div by 0; sqrt(1) divides by 0
    if (vc) {
      bad = bad || !ok;
      stg[col] = (int32_t)(uint32_t)mur;
      stg[D + col] = (int32_t)(uint32_t)((uint64_t)mur >> 32);
      stg[2 * D + col] = (int32_t)(uint32_t)sd;
      stg[3 * D + col] = (int32_t)(uint32_t)((uint64_t)sd >> 32);
    }
  }
  if (bad) flag = 1;
  __syncthreads();
  if (flag) {   // a zero-variance column (DIV_BY_ZERO; mode 2: or a value out of the domain): nothing written yet
    if (tid == 0 && p.xstats) atomicAdd(&p.xstats[1], 1u);
    return;
  }

  // ------------------------------------------------------------ pass 2b: z-score powers, outputs
  // (no failure is possible from here: a RELIABLE row's |z| <= sqrt(R) 1e6 (1 + 2^-20) keeps every product in
  // int64 and wdiv_z inside its |z| < 2^31.  Nothing bounds the other rows -- a failing oracle 2^37 wsad out over
  // an sd of a few thousand, or a padding row re-reading such a row 0 -- so wdiv_z_masked clears their deviation
  // before the division: rm holds reliable rows < N only, and no row outside it ever reaches wdiv_z.)
  for (int s = 0; s < nslab; ++s) {
    const int col = s * W + wave * 64 + lane;
    const bool vc = col < D;
    const int cc = vc ? col : 0;
    const int vo = cc * ESZ;
    const int64_t B = xload<V32>(rs, vo, 0);
    const int64_t mur = (int64_t)(((uint64_t)(uint32_t)stg[D + cc] << 32) | (uint32_t)stg[cc]);
    const int64_t sd = (int64_t)(((uint64_t)(uint32_t)stg[3 * D + cc] << 32) | (uint32_t)stg[2 * D + cc]);
    const double h = (double)(sd / 2), inv = 1.0 / (double)sd;
    int rowb1 = rowb;
    uint64_t rm1 = rm;
    asm volatile("" : "+s"(rowb1), "+v"(rm1));
    // z^2 < 2^46 and |z^2 z| < 2^49: the half-offset fp64 forms (wsad_fast.hpp) are exact; z^4 too while z^2 <
    // 2^25 (|z| < 5.8), the rare larger ones in int64
    double s3 = 0.0, s4 = 0.0;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const int64_t di = xload<V32>(rs, vo, (FULLN || i < N ? i : 0) * rowb1) - B - mur;
      const uint32_t m = bit_mask(rm1, i);
      const double zd = (double)wdiv_z_masked(di, m, sd, h, inv);     // wsad_div(x - mean, sd); 0 off the mask
      double z2, z3, z4;
      zpow_x(zd, z2, z3, z4);                                         // wsad_mul(z, z), (z^2, z), (z^2, z^2)
      s3 += dblend(z3, 0.0, m);
      s4 += dblend(z4, 0.0, m);
    }
    // skewness and kurtosis from the sums (math.cairo:336-337, 359-362): the exact fp64 divisions of skew_kurt_x
    double sk, ku;
    skew_kurt_x(s3, s4, (double)R, sk, ku);
    if (vc) {
      p.consensus[ob + col] = B + mur;
      p.skew[ob + col] = (int64_t)sk;
      p.kurt[ob + col] = (int64_t)ku;
    }
  }
  // ------------------------------------------------------------ commit
  for (int t = tid; t < N; t += NT) {
    p.reliable[(int64_t)b * N + t] = (rm >> t) & 1;
    p.qr[(int64_t)b * N + t] = (int64_t)qr_lds[t];
  }
  if (tid == 0) {
    p.rel[2 * (int64_t)b] = rels[0];
    p.rel[2 * (int64_t)b + 1] = rels[1];
    p.status[b] = ST_OK;
    p.fallback[b] = 0;
    if (p.xstats) atomicAdd(&p.xstats[0], 1u);
  }
}

}  // namespace svoc

using namespace svoc;

extern "C" int svoc_exact_round_wsadx_groups(const ExactParams* p, hipStream_t stream);   // consensus_wsadx_groups.hip

namespace svoc {
template <int MODE>
static auto wsadx_kernel_of(const ExactParams& p) {
  return p.N == 64 ? (p.val32 ? consensus_wsadx_kernel<true, true, MODE> : consensus_wsadx_kernel<false, true, MODE>)
                   : (p.val32 ? consensus_wsadx_kernel<true, false, MODE> : consensus_wsadx_kernel<false, false, MODE>);
}
}  // namespace svoc

// After the column kernel: its flagged instances of unconstrained rounds (N <= 256) -- whole ones and either half of
// a D-sharded one (ExactParams::mode) -- are taken here where they fit the domain above: N <= 64 by the kernel of
// this file, 64 < N <= 256 by its lane-group form (consensus_wsadx_groups.hip).  `xstats` counts per launch [0] the
// instances these kernels took (a whole round committed, or a half done), [1] the ones left to the i128 kernel
// (every flagged instance, whatever the round's shape).  -2: nothing launched.
extern "C" int svoc_exact_round_wsadx(const ExactParams* p, hipStream_t stream) {
  if (p->B <= 0 || !p->fallback || !p->stage) return -2;
  const bool shape = p->mode >= 0 && p->mode <= 2 && !p->constrained && !p->legacy && p->N >= 4 && p->win_h == 0 &&
                     (int64_t)p->N * p->D * (p->val32 ? 4 : 8) < (1ll << 31);
  if (shape && p->N > 64 && p->N <= 256) return svoc_exact_round_wsadx_groups(p, stream);
  const bool handle = shape && p->N <= 64;
  if (!handle && !p->xstats) return -2;
  // (a shape not taken here runs the whole-round kernel's counting branch only)
  auto k = !handle || p->mode == 0 ? wsadx_kernel_of<0>(*p) : p->mode == 1 ? wsadx_kernel_of<1>(*p) : wsadx_kernel_of<2>(*p);
  hipLaunchKernelGGL(k, dim3(p->B), dim3(256), 0, stream, *p, handle ? 1 : 0);
  return (int)hipGetLastError();
}
