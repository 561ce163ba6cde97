// Exact UNCONSTRAINED rounds over wide columns with 64 < N <= 256 oracles: the lane-group form of the int64
// wide-column kernel (consensus_wsadx.hip, which keeps N <= 64).  Same semantics (contract.cairo:370-434), same
// domain (|B| < 2^61, |x - B| < 2^37, int64 or int32 storage), same hand-offs (anything out of the domain, a carry
// out of a qr sum, every revert stays flagged for the i128 kernel), and bit-identical to the i128 kernel and the CPU
// golden engine on every round it commits.
//
// Layout: one workgroup per instance (4 waves); a column is owned by NSEG lanes (NSEG = 2 for N <= 128, 4 for
// N <= 256), lane `seg` of the group holding rows [64 seg, 64 seg + 64) -- the column kernel's lane groups
// (sortnet.hpp): lane = seg P + pw with P = 64 / NSEG columns per wave, so the group's lanes are lane ^ 32
// (and lane ^ 16 for NSEG = 4).  A slab is 4 P columns.
//   - Pass-1 smooth median: the keys are the exact doubles (double)(x - B) (38-bit signed integers), padding rows
//     -inf / +inf split around the middle as in the N <= 64 kernel.  The network is median_group<2> / <4> of
//     sortnet.hpp on v_min_f64 / v_max_f64: the 64-key odd-even merge sort in the lane, the cross-lane
//     half-cleaners on v_permlane{16,32}_swap (two per double), the last stage folded into a running max / min.
//     The "complemented" polarity of the u32 networks is the negated double (order-reversing and exact, the
//     infinities included).
//   - Per-oracle qr: the transposing butterfly of the N <= 64 kernel over the P lanes that share a segment; lane l
//     ends with the sums of rows NSEG l .. NSEG l + NSEG - 1 over the wave's columns (uint64, carries flagged).
//   - Rank mask: thread t ranks row t over the N qr in LDS (qr ascending, index descending); one ballot per wave
//     gives the four 64-bit words of the mask.
//   - Pass 2a / 2b / commit as in the N <= 64 kernel, the per-column sums reduced over the group's lanes (the sums
//     are exact in fp64, so their order does not matter); a row outside the mask never reaches the z division
//     (wdiv_z_masked).
// The arithmetic for R <= 256 reliable rows (var_floor_g, zpow_g, skew_kurt_g) is in svoc/wsad_wide.hpp, host and
// device, with its preconditions; csrc/selftest/wsadx_groups_selftest.cpp compares it with the i128 routines.
// Rows past N are never addressed: a masked row re-reads row i < 64 of the same column (always present: N > 64).
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
namespace wxg {

SVOC_DEV uint64_t dbits(double v) { return __builtin_bit_cast(uint64_t, v); }
SVOC_DEV double bitsd(uint64_t v) { return __builtin_bit_cast(double, v); }

template <int M>
SVOC_DEV uint64_t xor_lane_u64(uint64_t v) {
  const uint32_t lo = xor_lane_u32<M>((uint32_t)v), hi = xor_lane_u32<M>((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
template <int M>
SVOC_DEV double xor_lane_f64(double v) { return bitsd(xor_lane_u64<M>(dbits(v))); }

// a double whose bits are blended by an all-ones / zero lane mask (no compare, no SGPR mask)
SVOC_DEV double dblend(double a, double b, uint32_t m) {   // m ? a : b
  const uint64_t mm = ((uint64_t)m << 32) | m;
  return bitsd((dbits(a) & mm) | (dbits(b) & ~mm));
}

// 64-row odd-even merge sort on exact double keys (the comparator table of sortnet.hpp), all 64 outputs
SVOC_DEV void sort64_f64(double (&r)[64]) {
  constexpr CmpNet<64> T = make_oem<64>();
#pragma unroll
  for (int c = 0; c < T.n; ++c) {
    const double x = r[T.a[c]], y = r[T.b[c]];
    r[T.a[c]] = __builtin_fmin(x, y);
    r[T.b[c]] = __builtin_fmax(x, y);
  }
}
// ascending half-cleaner cascade: sorts a bitonic in-lane sequence (sortnet.hpp merge64)
SVOC_DEV void merge64_f64(double (&r)[64]) {
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const int l = i ^ j;
      if (l > i) {
        const double a = r[i], b = r[l];
        r[i] = __builtin_fmin(a, b);
        r[l] = __builtin_fmax(a, b);
      }
    }
  }
}
// sortnet.hpp xswap on a double: afterwards x is the lower lane's value and y the upper lane's, in both lanes
template <int XM>
SVOC_DEV void xswap_f64(double& x, double& y) {
  const uint64_t ux = dbits(x), uy = dbits(y);
  uint32_t xl = (uint32_t)ux, xh = (uint32_t)(ux >> 32), yl = (uint32_t)uy, yh = (uint32_t)(uy >> 32);
  xswap<XM>(xl, yl);
  xswap<XM>(xh, yh);
  x = bitsd(((uint64_t)xh << 32) | xl);
  y = bitsd(((uint64_t)yh << 32) | yl);
}
// sortnet.hpp xhc_swap: half-cleaner between lanes l and l ^ XM, the upper lane's keys negated on the way in;
// both lanes leave in the lower lane's polarity
template <int XM>
SVOC_DEV void xhc_swap_f64(double (&r)[64]) {
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    double x = r[2 * k], y = r[2 * k + 1];
    xswap_f64<XM>(x, y);
    y = -y;
    double lo = __builtin_fmin(x, y), hi = __builtin_fmax(x, y);
    xswap_f64<XM>(lo, hi);
    r[2 * k] = lo;
    r[2 * k + 1] = hi;
  }
}
// sortnet.hpp xhc_middle: the last half-cleaner folded into max(lower half) / min(upper half)
template <int XM>
SVOC_DEV void xhc_middle_f64(const double (&r)[64], double& mx, double& mn) {
  mx = -INFINITY;
  mn = INFINITY;
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    double x = r[2 * k], y = r[2 * k + 1];
    xswap_f64<XM>(x, y);
    y = -y;
    mx = __builtin_fmax(mx, __builtin_fmin(x, y));
    mn = __builtin_fmin(mn, __builtin_fmax(x, y));
  }
}
// The two middle order statistics (sorted positions 32 NSEG - 1 and 32 NSEG) of the group's 64 NSEG keys, in
// every lane of the group.  r: the lane's keys, negated where group_polarity<NSEG>(seg) is set.
template <int NSEG>
SVOC_DEV void median_group_f64(double (&r)[64], double& lo, double& hi) {
  static_assert(NSEG == 2 || NSEG == 4, "lane groups of 2 or 4");
  sort64_f64(r);
  if constexpr (NSEG == 4) {
    xhc_swap_f64<16>(r);
    merge64_f64(r);
  }
  double mx, mn;
  xhc_middle_f64<32>(r, mx, mn);
  if constexpr (NSEG == 4) {
    mx = __builtin_fmax(mx, xor_lane_f64<16>(mx));
    mn = __builtin_fmin(mn, xor_lane_f64<16>(mn));
  }
  lo = __builtin_fmax(mx, xor_lane_f64<32>(mx));
  hi = __builtin_fmin(mn, xor_lane_f64<32>(mn));
}

// the sum of v over the group's lanes (exact fp64 sums of integers: any order)
template <int NSEG>
SVOC_DEV double group_sum_f64(double v) {
  if constexpr (NSEG == 4) v += xor_lane_f64<16>(v);
  return v + xor_lane_f64<32>(v);
}
template <int NSEG>
SVOC_DEV uint64_t group_sum_u64(uint64_t v) {
  if constexpr (NSEG == 4) v += xor_lane_u64<16>(v);
  return v + xor_lane_u64<32>(v);
}

// Transposing butterfly over the P lanes that share a segment (consensus_wsadx.hip qr_fold): from MSK = P / 2,
// H = 32, lane pw ends with rows (64 / P) pw .. of its segment summed over the P columns, in q[0 .. 64 / P).
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

// FULLN: N = 64 NSEG (every row real, no row masks: the c3 shape); otherwise the rows >= N are masked arithmetically
// MODE: 0 the whole round; 1 / 2 the halves of a D-sharded round, as in the N <= 64 kernel (consensus_wsadx.hip):
// 1 writes c1 and the qr partials (each below kExactQrPartialMax) or nothing; 2 reads the all-reduced qr (each
// below 2^62) and runs the rank mask, the reliabilities and pass 2, pass 2a checking the domain over every row.
template <bool V32, int NSEG, bool FULLN, int MODE = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void consensus_wsadx_group_kernel(ExactParams p) {
  constexpr int NT = 256, WAVES = 4, P = 64 / NSEG, W = WAVES * P, NPAD = 64 * NSEG, KEEP = NSEG;
  constexpr int ESZ = V32 ? 4 : 8;
  __shared__ uint64_t qr_part[WAVES][NPAD];
  __shared__ uint64_t qr_lds[NPAD];
  __shared__ uint64_t relmask[4];
  __shared__ int64_t rels[2];
  __shared__ int flag;

  const int b = blockIdx.x;
  if (!p.fallback[b]) return;   // (the column kernel took it, or the instance is inactive)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int seg = lane / P, pw = lane % P;
  if constexpr (MODE == 2) {   // a shard's first half failed: the round reverts everywhere, nothing to compute
    if (p.status[b] != ST_OK) {
      if (tid == 0) p.fallback[b] = 0;
      return;
    }
  }
  const int N = FULLN ? NPAD : p.N, D = p.D;
  const int rowb = D * ESZ;
  const __amdgpu_buffer_rsrc_t rs =
      instance_rsrc((const unsigned char*)p.values + (int64_t)b * N * rowb, (uint32_t)(N * rowb));
  const int64_t ob = (int64_t)b * D;
  // the staging buffer (int32 [6][D]: this kernel's per-column mean / sd as int64 word pairs)
  int32_t* const stg = p.stage + (int64_t)b * 6 * D;
  if (tid == 0) flag = 0;
  __syncthreads();
  uint64_t oob = 0;  // out-of-domain bits (or a carry out of a qr sum)
  const int nslab = (D + W - 1) / W;
  const int lo1 = (NPAD - N + 1) >> 1;   // sentinel split: the middle of the padded sort = the middle of the rows
  // the lane's rows are 64 seg + i: real while i < N - 64 seg; the segment's byte offset only where it has a real row
  const int nloc = N - 64 * seg;
  const int segoff = nloc > 0 ? 64 * seg * rowb : 0;
  const uint64_t pol = (seg == 1 || (NSEG == 4 && seg == 2)) ? 0x8000000000000000ull : 0ull;   // group_polarity
  const bool first = seg == 0;

  // ------------------------------------------------------------ pass 1 (contract.cairo:383-395)
  uint64_t acc[KEEP];   // rows KEEP lane .. KEEP lane + KEEP - 1: their qr over the wave's columns
#pragma unroll
  for (int j = 0; j < KEEP; ++j) acc[j] = 0;
  for (int s = 0; s < (MODE == 2 ? 0 : nslab); ++s) {   // (mode 2: no pass 1, the all-reduced qr is read below)
    const int col = s * W + wave * P + pw;
    const bool vc = col < D;
    const int vo = (vc ? col : 0) * ESZ;
    const uint32_t mc = vc ? 0xffffffffu : 0u;
    const int64_t B = xload<V32>(rs, vo, 0);
    // (an opaque row stride and row counts per slab: the 64 row offsets / masks are recomputed, not hoisted out of
    // the loop and spilled)
    int rowb1 = rowb, n1 = nloc, nl1 = nloc + lo1, so1 = segoff;
    asm volatile("" : "+s"(rowb1), "+v"(n1), "+v"(nl1), "+v"(so1));
    int64_t c1r;
    // domain: |B| < 2^61 and |x - B| < 2^37 (so |x| < 2^62 and x - B cannot wrap); a masked row reads a real row
    // of the column, checked like every other
    double rmax = 0.0;
    oob |= (vc && (uint64_t)(B + (1ll << 61)) >= (1ull << 62)) ? 1ull : 0ull;
    {
      double k[64];
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        const uint32_t mr = FULLN ? 0xffffffffu : lt_mask(i, n1);
        const int64_t x = xload<V32>(rs, vo + (so1 & (int)mr), i * rowb1);
        const double rd = (double)(x - B);   // (exact while |x - B| < 2^53; the domain check below)
        rmax = __builtin_fmax(rmax, __builtin_fabs(rd));
        // rows N .. N + lo1 - 1: -inf, then +inf; the key negated in the lanes of opposite polarity
        const double kd = FULLN ? rd : dblend(rd, dblend(-INFINITY, INFINITY, lt_mask(i, nl1)), mr);
        k[i] = bitsd(dbits(kd) ^ pol);
      }
      oob |= (vc && !(rmax < 137438953472.0)) ? 1ull : 0ull;   // 2^37
      double klo, khi;
      median_group_f64<NSEG>(k, klo, khi);
      // smooth median (math.cairo:113-126): I128Div(s[N/2 - 1] + s[N/2], 2) on the absolute values (|B| < 2^61:
      // the sum fits int64; C's division truncates toward zero, as I128Div).  (Out of the domain the keys may
      // be anything: the conversions saturate, and the instance is flagged.)
      const int64_t c1a = ((B + (int64_t)klo) + (B + (int64_t)khi)) / 2;
      c1r = c1a - B;
      if constexpr (MODE == 1) {   // (p.c1 is the output itself: staged here, written where the half succeeds)
        if (vc && first) {
          stg[col] = (int32_t)(uint32_t)c1a;
          stg[D + col] = (int32_t)(uint32_t)((uint64_t)c1a >> 32);
        }
      } else {
        if (vc && first) p.c1[ob + col] = c1a;   // (the staged c1, committed where the round succeeds)
      }
    }
    // quadratic risk (math.cairo:225-238): qdev(x, c1) of every row, summed over the columns.  (The re-read's
    // offset depends on c1 through an empty asm: the loads stay below the network.)
    uint64_t q[64];
    const double c1d = (double)c1r;
    int vo2 = vo;
    asm volatile("" : "+v"(vo2) : "v"(c1r));
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const uint32_t mr = FULLN ? 0xffffffffu : lt_mask(i, n1);
      const int64_t r = xload<V32>(rs, vo2 + (so1 & (int)mr), i * rowb1) - B;
      const uint32_t m = mc & mr;
      q[i] = qdev_dd((double)r - c1d) & (((uint64_t)m << 32) | m);
    }
    bool ovf = false;
    qr_fold<P / 2, 32>(q, lane, ovf);
#pragma unroll
    for (int j = 0; j < KEEP; ++j) {
      const uint64_t t = acc[j] + q[j];
      ovf = ovf || t < acc[j];
      acc[j] = t;
    }
    oob |= ovf ? 1ull : 0ull;
  }
#pragma unroll
  for (int j = 0; j < KEEP; ++j) qr_part[wave][KEEP * lane + j] = acc[j];   // (row 64 seg + KEEP pw + j)
  if (oob) flag = 1;
  __syncthreads();
  if (tid < NPAD) {
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
    if (tid < N && (o || v >= (MODE == 1 ? (uint64_t)kExactQrPartialMax : (1ull << 62)))) flag = 1;
    qr_lds[tid] = v;
  }
  __syncthreads();
  if constexpr (MODE == 1) {   // first half done: c1 and the qr partials out, nothing else
    if (flag) {
      if (tid == 0 && p.xstats) atomicAdd(&p.xstats[1], 1u);
      return;
    }
    for (int s = 0; s < nslab; ++s) {   // (the group's first lane reads back the columns it staged)
      const int col = s * W + wave * P + pw;
      if (col < D && first)
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
  {
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
    if (lane == 0) relmask[wave] = bal;   // rows 64 wave .. 64 wave + 63 (only rows < N are set)
  }
  __syncthreads();
  if (tid == 0 && !flag) {
    // reliabilities (contract.cairo:365-368) with the wsad.hpp routines; every revert goes to the i128 kernel,
    // which reports the stage-ordered status
    // (only where no sum was flagged: then each qr is below 2^62 and so are their means, which is wsqrt_x's
    // precondition -- past 2^63 the int64 mean is negative and the Newton quotient's correction loops have no bound)
    int st = ST_OK;
    i128 s_all = 0, s_rel = 0;
    for (int t = 0; t < N; ++t) {
      const i128 qv = (i128)qr_lds[t];
      s_all += qv;
      if ((relmask[t >> 6] >> (t & 63)) & 1) s_rel += qv;
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
  const uint64_t rm = relmask[seg];   // the lane's 64 rows (only rows < N are set)
  bool bad = false;
  for (int s = 0; s < nslab; ++s) {
    const int col = s * W + wave * P + pw;
    const bool vc = col < D;
    const int vo = (vc ? col : 0) * ESZ;
    const int64_t B = xload<V32>(rs, vo, 0);
    int rowb1 = rowb, n1 = nloc, so1 = segoff;
    uint64_t rm1 = rm;
    asm volatile("" : "+s"(rowb1), "+v"(rm1), "+v"(n1), "+v"(so1));
    // the reliable mean (math.cairo:240-254): I128Div of the absolute sum by R.  The relative sum is exact in
    // fp64: below 64 * 2^37 in the lane, below 2^45 over the group.  The column is read twice (sum, then variance).
    double Sl = 0.0;
    double rmax = 0.0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const uint32_t mr = FULLN ? 0xffffffffu : lt_mask(i, n1);
      const int64_t x = xload<V32>(rs, vo + (so1 & (int)mr), i * rowb1);
      const double rd = (double)(x - B);
      if constexpr (MODE == 2) rmax = __builtin_fmax(rmax, __builtin_fabs(rd));   // (a masked row reads a real one)
      Sl += dblend(rd, 0.0, bit_mask(rm1, i));
    }
    double Sd = group_sum_f64<NSEG>(Sl);
    if constexpr (MODE == 2) {
      // the domain of pass 1, over every row of the group's lanes: |B| < 2^61 and |x - B| < 2^37.  Outside it the
      // column's sum and mask are cleared, so the mean is 0, the variance 0 and its sqrt returns at once; the
      // instance is flagged below
      if constexpr (NSEG == 4) rmax = __builtin_fmax(rmax, xor_lane_f64<16>(rmax));
      rmax = __builtin_fmax(rmax, xor_lane_f64<32>(rmax));
      const bool od = (uint64_t)(B + (1ll << 61)) >= (1ull << 62) || !(rmax < 137438953472.0);
      if (od) {
        Sd = 0.0;
        rm1 = 0;
      }
      bad = bad || (vc && od);
    }
    const double Rd = (double)R, invR = recip_lo(Rd);
    // trunc((R B + S) / R) - B from trunc(S / R) (wsad_fast.hpp tdiv_rel_fix; |S| < 2^45 < 2^51, R <= 256)
    const double qd = trunc_div_d(Sd, Rd, invR);
    const int64_t mur = tdiv_rel_fix((int64_t)qd, fma(-qd, Rd, Sd) == 0.0, Sd < 0.0, B);
    const double mud = (double)mur;
    // population variance (math.cairo:208-222): floor of the mean qdev (non-negative)
    int vo2 = vo;
    asm volatile("" : "+v"(vo2) : "v"(mur));   // (the re-read after the mean, not hoisted above it)
    uint64_t svl = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const uint32_t mr = FULLN ? 0xffffffffu : lt_mask(i, n1);
      const int64_t x = xload<V32>(rs, vo2 + (so1 & (int)mr), i * rowb1);
      const uint32_t m = bit_mask(rm1, i);
      svl += qdev_dd((double)(x - B) - mud) & (((uint64_t)m << 32) | m);
    }
    // (the reliable rows' sum of qdev around their mean is below 2^62.1 < 2^63: Popoviciu, see var_floor_g)
    const int64_t var = var_floor_g(group_sum_u64<NSEG>(svl), R);
    int64_t sd = 0;
    const bool ok = wsqrt_x(var, sd) && sd != 0;   // sqrt(0) -> wsad_div by 0; sqrt(1) divides by 0
    if (vc) {
      bad = bad || !ok;
      if (first) {
        stg[col] = (int32_t)(uint32_t)mur;
        stg[D + col] = (int32_t)(uint32_t)((uint64_t)mur >> 32);
        stg[2 * D + col] = (int32_t)(uint32_t)sd;
        stg[3 * D + col] = (int32_t)(uint32_t)((uint64_t)sd >> 32);
      }
    }
  }
  if (bad) flag = 1;
  __syncthreads();
  if (flag) {   // a zero-variance column (DIV_BY_ZERO; mode 2: or a value out of the domain): nothing written yet
    if (tid == 0 && p.xstats) atomicAdd(&p.xstats[1], 1u);
    return;
  }

  // ------------------------------------------------------------ pass 2b: z-score powers, outputs
  // (no failure is possible from here: a RELIABLE row's |z| <= sqrt(R (1 + 1 / var)) 1e6 / 0.999 + 1 < 2e7 keeps
  // wdiv_z inside its |z| < 2^31 and zpow_g / skew_kurt_g inside int64.  Nothing bounds the other rows, so
  // wdiv_z_masked clears their deviation before the division: rm holds reliable rows < N only, and no row outside
  // it ever reaches wdiv_z.)
  for (int s = 0; s < nslab; ++s) {
    const int col = s * W + wave * P + pw;
    const bool vc = col < D;
    const int cc = vc ? col : 0;
    const int vo = cc * ESZ;
    const int64_t B = xload<V32>(rs, vo, 0);
    const int64_t mur = (int64_t)(((uint64_t)(uint32_t)stg[D + cc] << 32) | (uint32_t)stg[cc]);
    const int64_t sd = (int64_t)(((uint64_t)(uint32_t)stg[3 * D + cc] << 32) | (uint32_t)stg[2 * D + cc]);
    const double h = (double)(sd / 2), inv = 1.0 / (double)sd;
    int rowb1 = rowb, n1 = nloc, so1 = segoff;
    uint64_t rm1 = rm;
    asm volatile("" : "+s"(rowb1), "+v"(rm1), "+v"(n1), "+v"(so1));
    double s3 = 0.0, s4 = 0.0;   // (the lane's 64 rows: |s3| < 2^40, s4 < 2^44, exact)
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const uint32_t mr = FULLN ? 0xffffffffu : lt_mask(i, n1);
      const int64_t di = xload<V32>(rs, vo + (so1 & (int)mr), i * rowb1) - B - mur;
      const uint32_t m = bit_mask(rm1, i);
      const double zd = (double)wdiv_z_masked(di, m, sd, h, inv);     // wsad_div(x - mean, sd); 0 off the mask
      double z2, z3, z4;
      zpow_g(zd, z2, z3, z4);                                         // wsad_mul(z, z), (z^2, z), (z^2, z^2)
      s3 += dblend(z3, 0.0, m);
      s4 += dblend(z4, 0.0, m);
    }
    // skewness and kurtosis from the group's sums (math.cairo:336-337, 359-362) in int64
    int64_t sk, ku;
    skew_kurt_g((int64_t)group_sum_f64<NSEG>(s3), (int64_t)group_sum_f64<NSEG>(s4), (int64_t)R, sk, ku);
    if (vc && first) {
      p.consensus[ob + col] = B + mur;
      p.skew[ob + col] = sk;
      p.kurt[ob + col] = ku;
    }
  }
  // ------------------------------------------------------------ commit
  for (int t = tid; t < N; t += NT) {
    p.reliable[(int64_t)b * N + t] = (relmask[t >> 6] >> (t & 63)) & 1;
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

}  // namespace wxg
}  // namespace svoc

using namespace svoc;

namespace svoc {
template <int MODE>
static auto wsadx_group_kernel_of(const ExactParams& p) {
  void (*k)(ExactParams);
  if (p.N <= 128) {
    k = p.N == 128 ? (p.val32 ? wxg::consensus_wsadx_group_kernel<true, 2, true, MODE> : wxg::consensus_wsadx_group_kernel<false, 2, true, MODE>)
                   : (p.val32 ? wxg::consensus_wsadx_group_kernel<true, 2, false, MODE> : wxg::consensus_wsadx_group_kernel<false, 2, false, MODE>);
  } else {
    k = p.N == 256 ? (p.val32 ? wxg::consensus_wsadx_group_kernel<true, 4, true, MODE> : wxg::consensus_wsadx_group_kernel<false, 4, true, MODE>)
                   : (p.val32 ? wxg::consensus_wsadx_group_kernel<true, 4, false, MODE> : wxg::consensus_wsadx_group_kernel<false, 4, false, MODE>);
  }
  return k;
}
}  // namespace svoc

// The flagged instances of unconstrained rounds with 64 < N <= 256, whole or either half of a D-sharded one (the
// caller, svoc_exact_round_wsadx, has checked the round's shape): `xstats` [0] += instances taken here,
// [1] += instances left to the i128 kernel.
extern "C" int svoc_exact_round_wsadx_groups(const ExactParams* p, hipStream_t stream) {
  if (p->N <= 64 || p->N > 256 || p->mode < 0 || p->mode > 2) return -1;
  auto k = p->mode == 0 ? wsadx_group_kernel_of<0>(*p) : p->mode == 1 ? wsadx_group_kernel_of<1>(*p) : wsadx_group_kernel_of<2>(*p);
  hipLaunchKernelGGL(k, dim3(p->B), dim3(256), 0, stream, *p);
  return (int)hipGetLastError();
}
