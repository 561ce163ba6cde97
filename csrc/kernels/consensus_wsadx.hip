// Exact UNCONSTRAINED rounds over wide columns (VERDICT r5 missing item 1), N <= 256 oracles: the instances the
// column kernel (consensus_wsad.hip) hands on because a column's values spread more than 2^30 wsad (1,073 real
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
// Layout: one workgroup per instance (4 waves); a column is owned by NSEG lanes (1 for N <= 64, 2 for N <= 128, 4 for
// N <= 256), lane `seg` of the group holding rows [64 seg, 64 seg + 64) -- the column kernel's lane groups
// (sortnet.hpp): lane = seg P + pw with P = 64 / NSEG columns per wave, so the group's lanes are lane ^ 32 (and
// lane ^ 16 for NSEG = 4).  A slab is 4 P columns.  Values (int64 or int32 storage) are taken relative to the column's
// row-0 value B as int64.
//   - Pass-1 smooth median: the keys are the exact doubles (double)(x - B), padding rows -inf / +inf split around
//     the middle.  The network is median_group<NSEG> of sortnet.hpp on v_min_f64 / v_max_f64: the 64-key odd-even
//     merge sort in the lane (NSEG = 1: pruned by dead-code elimination to the median pair), then the cross-lane
//     half-cleaners on v_permlane{16,32}_swap (two per double), the last stage folded into a running max / min.  The
//     "complemented" polarity of the u32 networks is the negated double (order-reversing and exact, infinities too).
//   - Per-oracle qr: a transposing butterfly over the P lanes that share a segment; lane l ends with the sums of
//     rows NSEG l .. NSEG l + NSEG - 1 over the wave's columns; then across waves and slabs.
//   - Rank mask: thread t < 64 NSEG ranks row t over the N qr in LDS (qr ascending, index descending); one ballot
//     per wave gives the NSEG 64-bit words of the mask.
//   - Pass 2a / 2b / commit: the per-column sums are reduced over the group's lanes (exact in fp64: any order).
// Rows past N are never addressed: a masked row re-reads a real row of the same column (xrow below).
//
// Domain (else the i128 kernel): |B| < 2^61 and |x - B| < 2^37 (137,438 real units; so |x| < 2^62), so that
//   - the pass-1 keys are exact doubles (38-bit signed integers),
//   - every deviation d from c1 or from the mean is below 2^38 and qdev(d) = floor((d^2 + 500000) / 1e6) <
//     2^56.1: the fp64 double-double square and a remainder-corrected quotient (qdev_dd),
//   - the per-oracle qr sums stay in uint64 -- a carry out of any sum hands the instance to the i128 kernel,
//   - the variance (< 2^56.1) takes the contract's Newton sqrt with 128-bit dividends v 1e6 + g / 2 done as an
//     fp64 estimate plus the exact remainder modulo 2^64 (wsqrt_x), and z = wsad_div(d, sd) has an int64
//     dividend d 1e6 + sd / 2 < 2^58 (wdiv_z: reciprocal estimate, exact remainder) and, on the reliable rows,
//     |z| < 2^31 -- the other rows' deviations are cleared before the division (wdiv_z_masked); z^2, z^3, z^4
//     take the half-offset fp64 products of wsad_fast.hpp (int64 for the rare z^2 >= 2^25).
// The arithmetic named here lives in svoc/wsad_wide.hpp, host and device, with its preconditions, in a form for
// R <= 64 reliable rows (NSEG = 1; host self-test csrc/selftest/engine_selftest.cpp wsadx_paths) and one for R <= 256
// (NSEG > 1: var_floor_g, zpow_g, skew_kurt_g; csrc/selftest/wsadx_groups_selftest.cpp), both against the i128 routines.
//
// Hand-offs: the kernel commits only rounds that succeed; anything else (a reliability outside [0, 1], R < 4, a
// zero-variance column, a value outside the domain, a carry out of a qr sum) stays flagged and the i128 kernel
// computes it, status included.  Pass 2 runs in two sweeps (means and sqrt into the staging buffer, checked; then
// the moments and the outputs), so a round that would revert never touches the outputs.
//
// MODE (launch.hpp ExactParams::mode): 0 the whole round; 1 / 2 the halves of a D-sharded round as the i128 kernel
// splits it (svoc/parallel/dshard.py), each done whole or left flagged.  1: pass 1 over this shard's columns -- c1
// (staged, written only with the rest) and the per-oracle qr PARTIALS, each below kExactQrPartialMax, status OK;
// anything else (out of the domain, a carry, a partial at 2^58) writes nothing.  2: the all-reduced qr comes in (each
// below 2^62, else flagged), then the rank mask, the reliabilities and pass 2 as in a whole round; no pass 1 has
// validated the values, so pass 2a checks the domain over every row < N itself, before its sqrt and long before the
// z division of pass 2b.
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
  static_assert(NSEG == 1 || NSEG == 2 || NSEG == 4, "lane groups of 1, 2 or 4");
  sort64_f64(r);
  if constexpr (NSEG == 1) {   // (the comparators that reach neither output are dead code)
    lo = r[31];
    hi = r[32];
  } else {
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
}

// the sum / the maximum of v over the group's lanes (exact fp64 sums of integers: any order)
template <int NSEG>
SVOC_DEV double group_sum_f64(double v) {
  if constexpr (NSEG == 4) v += xor_lane_f64<16>(v);
  if constexpr (NSEG >= 2) v += xor_lane_f64<32>(v);
  return v;
}
template <int NSEG>
SVOC_DEV uint64_t group_sum_u64(uint64_t v) {
  if constexpr (NSEG == 4) v += xor_lane_u64<16>(v);
  if constexpr (NSEG >= 2) v += xor_lane_u64<32>(v);
  return v;
}
template <int NSEG>
SVOC_DEV double group_max_f64(double v) {
  if constexpr (NSEG == 4) v = __builtin_fmax(v, xor_lane_f64<16>(v));
  if constexpr (NSEG >= 2) v = __builtin_fmax(v, xor_lane_f64<32>(v));
  return v;
}

// Transposing butterfly over the P lanes that share a segment: from MSK = P / 2, H = 32, lane pw ends with rows
// (64 / P) pw .. of its segment summed over the P columns, in q[0 .. 64 / P).  `ovf` collects a carry out of any
// partial sum.
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

// Row i of the lane's 64: its value, and in `mr` all ones where the row is real (i < n, n the lane's row count) or
// zero.  A masked row re-reads a real row of the column at byte offset vo, checked like every other.  NSEG = 1: row 0,
// by a wave-uniform offset from the instance's N (N may be below 64, and a load past the buffer would return 0, which
// reads as x - B = -B and flags the domain).  NSEG > 1: row i of segment 0 (always present: N > 64), the segment's
// byte offset `so` cleared through the per-lane mask.
template <bool V32, int NSEG, bool FULLN>
SVOC_DEV int64_t xrow(__amdgpu_buffer_rsrc_t rs, int vo, int so, int i, int rowb, int n, int N, uint32_t& mr) {
  mr = FULLN ? 0xffffffffu : lt_mask(i, n);
  if constexpr (NSEG == 1) {
    return xload<V32>(rs, vo, (FULLN || i < N ? i : 0) * rowb);
  } else {
    return xload<V32>(rs, vo + (so & (int)mr), i * rowb);
  }
}

// FULLN: N = 64 NSEG (every row real, no row masks: the c2 / c3 shapes); otherwise the rows >= N are masked
// arithmetically.  MODE: see the header.  handle = 0: counting only, for rounds left to the i128 kernel.
template <bool V32, int NSEG, bool FULLN, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void consensus_wsadx_kernel(ExactParams p, int handle) {
  constexpr int NT = 256, WAVES = 4, P = 64 / NSEG, W = WAVES * P, NPAD = 64 * NSEG, KEEP = NSEG;
  constexpr int ESZ = V32 ? 4 : 8;
  __shared__ uint64_t qr_part[WAVES][NPAD];
  __shared__ uint64_t qr_lds[NPAD];
  __shared__ uint64_t relmask[NSEG];
  __shared__ int64_t rels[2];
  __shared__ int flag;

  const int b = blockIdx.x;
  if (!p.fallback[b]) return;   // (the column kernel took it, or the instance is inactive)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int seg = lane / P, pw = lane % P;
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
    // the loop as 64 live SGPRs that spill to VGPR lanes)
    int rowb1 = rowb, n1 = nloc, nl1 = nloc + lo1, so1 = segoff;
    asm volatile("" : "+s"(rowb1), "+v"(n1), "+v"(nl1), "+v"(so1));
    int64_t c1r;
    // domain: |B| < 2^61 and |x - B| < 2^37 (so |x| < 2^62 and x - B cannot wrap)
    double rmax = 0.0;
    oob |= (vc && (uint64_t)(B + (1ll << 61)) >= (1ull << 62)) ? 1ull : 0ull;
    {
      double k[64];
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        uint32_t mr;
        const int64_t x = xrow<V32, NSEG, FULLN>(rs, vo, so1, i, rowb1, n1, N, mr);
        const double rd = (double)(x - B);   // (exact while |x - B| < 2^53; the domain check below)
        rmax = __builtin_fmax(rmax, __builtin_fabs(rd));
        // rows N .. N + lo1 - 1: -inf, then +inf; the key negated in the lanes of opposite polarity
        const double kd = FULLN ? rd : dblend(rd, dblend(-INFINITY, INFINITY, lt_mask(i, nl1)), mr);
        if constexpr (NSEG == 1) k[i] = kd; else k[i] = bitsd(dbits(kd) ^ pol);
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
    // offset depends on c1 through an empty asm: otherwise the loads are hoisted above the network and 128 more
    // VGPRs are live across it.)
    uint64_t q[64];
    const double c1d = (double)c1r;
    int vo2 = vo;
    asm volatile("" : "+v"(vo2) : "v"(c1r));
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      uint32_t mr;
      const int64_t r = xrow<V32, NSEG, FULLN>(rs, vo2, so1, i, rowb1, n1, N, mr) - B;
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
  if (tid < NPAD) {
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
    relmask[wave] = bal;   // rows 64 wave .. 64 wave + 63 (only rows < N are set); every lane stores the same word
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
  // (the per-instance divisors are recomputed in each slab loop: live across the whole kernel they held 16 VGPRs)
  for (int s = 0; s < nslab; ++s) {
    const int col = s * W + wave * P + pw;
    const bool vc = col < D;
    const int vo = (vc ? col : 0) * ESZ;
    const int64_t B = xload<V32>(rs, vo, 0);
    int rowb1 = rowb, n1 = nloc, so1 = segoff;
    uint64_t rm1 = rm;
    asm volatile("" : "+s"(rowb1), "+v"(rm1));
    if constexpr (NSEG > 1) asm volatile("" : "+v"(n1), "+v"(so1));   // (NSEG = 1 uses neither here)
    // the reliable mean (math.cairo:240-254): I128Div of the absolute sum by R.  The relative sum is exact in
    // fp64: below 64 * 2^37 in the lane, below 2^45 over the group.  The column is read twice (sum, then variance)
    // rather than held: 64 doubles live across the variance loop pushed the kernel past 256 VGPRs (scratch in this
    // loop)
    double Sl = 0.0;
    double rmax = 0.0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      uint32_t mr;
      const int64_t x = xrow<V32, NSEG, FULLN>(rs, vo, so1, i, rowb1, n1, N, mr);
      const double rd = (double)(x - B);
      if constexpr (MODE == 2) rmax = __builtin_fmax(rmax, __builtin_fabs(rd));   // (a masked row reads a real one)
      Sl += dblend(rd, 0.0, bit_mask(rm1, i));
    }
    double Sd = group_sum_f64<NSEG>(Sl);
    if constexpr (MODE == 2) {
      // the domain of pass 1, over every row of the group's lanes: |B| < 2^61 and |x - B| < 2^37.  Outside it the
      // column's sum and mask are cleared, so the mean is 0, the variance 0 and its sqrt returns at once; the
      // instance is flagged below
      rmax = group_max_f64<NSEG>(rmax);
      const bool od = (uint64_t)(B + (1ll << 61)) >= (1ull << 62) || !(rmax < 137438953472.0);
      if (od) {
        Sd = 0.0;
        rm1 = 0;
      }
      bad = bad || (vc && od);
    }
    const double Rd = (double)R, invR = recip_lo(Rd);
    // trunc((R B + S) / R) - B from trunc(S / R) (wsad_fast.hpp tdiv_rel_fix: no R B product; |S| < 2^45 < 2^51,
    // R <= 256)
    const double qd = trunc_div_d(Sd, Rd, invR);
    const int64_t mur = tdiv_rel_fix((int64_t)qd, fma(-qd, Rd, Sd) == 0.0, Sd < 0.0, B);
    const double mud = (double)mur;
    // population variance (math.cairo:208-222): floor of the mean qdev (non-negative)
    int vo2 = vo;
    asm volatile("" : "+v"(vo2) : "v"(mur));   // (the re-read after the mean, not hoisted above it)
    uint64_t svl = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      uint32_t mr;
      const int64_t x = xrow<V32, NSEG, FULLN>(rs, vo2, so1, i, rowb1, n1, N, mr);
      const uint32_t m = bit_mask(rm1, i);
      svl += qdev_dd((double)(x - B) - mud) & (((uint64_t)m << 32) | m);
    }
    int64_t var;
    if constexpr (NSEG == 1) {   // floor(sv / R), R <= 64: an estimate, fixed by the exact remainder
      var = (int64_t)((double)svl * invR);
      int64_t vr = (int64_t)svl - var * R;
      while (vr < 0) { --var; vr += R; }
      while (vr >= R) { ++var; vr -= R; }
    } else {
      // (the reliable rows' sum of qdev around their mean is below 2^62.1 < 2^63: Popoviciu, see var_floor_g)
      var = var_floor_g(group_sum_u64<NSEG>(svl), R);
    }
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
  // wdiv_z inside its |z| < 2^31 and the powers and sums of zpow_x / skew_kurt_x (R <= 64) and zpow_g / skew_kurt_g
  // (R <= 256) inside their exact ranges.  Nothing bounds the other rows -- a failing oracle 2^37 wsad out over an sd
  // of a few thousand, or a masked row re-reading such a row -- so wdiv_z_masked clears their deviation before the
  // division: rm holds reliable rows < N only, and no row outside it ever reaches wdiv_z.)
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
    asm volatile("" : "+s"(rowb1), "+v"(rm1));
    if constexpr (NSEG > 1) asm volatile("" : "+v"(n1), "+v"(so1));   // (NSEG = 1 uses neither here)
    double s3 = 0.0, s4 = 0.0;   // (the lane's 64 rows: |s3| < 2^40, s4 < 2^44, exact)
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      uint32_t mr;
      const int64_t di = xrow<V32, NSEG, FULLN>(rs, vo, so1, i, rowb1, n1, N, mr) - B - mur;
      const uint32_t m = bit_mask(rm1, i);
      const double zd = (double)wdiv_z_masked(di, m, sd, h, inv);     // wsad_div(x - mean, sd); 0 off the mask
      double z2, z3, z4;                                              // wsad_mul(z, z), (z^2, z), (z^2, z^2)
      if constexpr (NSEG == 1) zpow_x(zd, z2, z3, z4); else zpow_g(zd, z2, z3, z4);
      s3 += dblend(z3, 0.0, m);
      s4 += dblend(z4, 0.0, m);
    }
    // skewness and kurtosis from the group's sums (math.cairo:336-337, 359-362): the exact fp64 divisions of
    // skew_kurt_x for R <= 64, int64 for R <= 256
    int64_t sk, ku;
    if constexpr (NSEG == 1) {
      double skd, kud;
      skew_kurt_x(s3, s4, (double)R, skd, kud);
      sk = (int64_t)skd;
      ku = (int64_t)kud;
    } else {
      skew_kurt_g((int64_t)group_sum_f64<NSEG>(s3), (int64_t)group_sum_f64<NSEG>(s4), (int64_t)R, sk, ku);
    }
    if (vc && first) {
      p.consensus[ob + col] = B + mur;
      p.skew[ob + col] = sk;
      p.kurt[ob + col] = ku;
    }
  }
  // ------------------------------------------------------------ commit
  for (int t = tid; t < N; t += NT) {
    p.reliable[(int64_t)b * N + t] = ((NSEG == 1 ? rm : relmask[t >> 6]) >> (t & 63)) & 1;   // (NSEG = 1: rm is that word)
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

template <int NSEG, int MODE>
static auto wsadx_kernel_of(const ExactParams& p) {
  return p.N == 64 * NSEG ? (p.val32 ? consensus_wsadx_kernel<true, NSEG, true, MODE> : consensus_wsadx_kernel<false, NSEG, true, MODE>)
                          : (p.val32 ? consensus_wsadx_kernel<true, NSEG, false, MODE> : consensus_wsadx_kernel<false, NSEG, false, MODE>);
}
template <int NSEG>
static auto wsadx_kernel_of(const ExactParams& p, int mode) {
  return mode == 0 ? wsadx_kernel_of<NSEG, 0>(p) : mode == 1 ? wsadx_kernel_of<NSEG, 1>(p) : wsadx_kernel_of<NSEG, 2>(p);
}

}  // namespace svoc

using namespace svoc;

// After the column kernel: its flagged instances of unconstrained rounds (N <= 256) -- whole ones and either half of
// a D-sharded one (ExactParams::mode) -- are taken here where they fit the domain above.  `xstats` counts per launch
// [0] the instances this kernel took (a whole round committed, or a half done), [1] the ones left to the i128 kernel
// (every flagged instance, whatever the round's shape).  -2: nothing launched.
extern "C" int svoc_exact_round_wsadx(const ExactParams* p, hipStream_t stream) {
  if (p->B <= 0 || !p->fallback || !p->stage) return -2;
  const bool handle = p->mode >= 0 && p->mode <= 2 && !p->constrained && !p->legacy && p->N >= 4 && p->N <= 256 &&
                      p->win_h == 0 && (int64_t)p->N * p->D * (p->val32 ? 4 : 8) < (1ll << 31);
  if (!handle && !p->xstats) return -2;
  // (a shape not taken here runs the counting branch of the NSEG = 1 whole-round kernel only)
  auto k = !handle ? wsadx_kernel_of<1>(*p, 0)
           : p->N <= 64 ? wsadx_kernel_of<1>(*p, p->mode)
           : p->N <= 128 ? wsadx_kernel_of<2>(*p, p->mode) : wsadx_kernel_of<4>(*p, p->mode);
  hipLaunchKernelGGL(k, dim3(p->B), dim3(256), 0, stream, *p, handle ? 1 : 0);
  return (int)hipGetLastError();
}
