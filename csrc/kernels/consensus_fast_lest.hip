// Rank-weighted (L-estimator) consensus round over fp32 storage: one workgroup per instance, one lane per
// column, whole rounds only.
//
// The essence estimator of the contract is the smooth median -- two of a column's N order statistics.  This round
// takes a weight per rank instead: for a column with sorted values x(0) <= ... <= x(n-1),
//   L_w(x) = sum_k w[k] x(k).
// w1 [N] weighs pass 1 (c1), w2 [R = N - f] the constrained pass 2 (the consensus over the reliable rows).  The bell
// weights of svoc/estimators.py give the "super smooth median" the reference documents and never builds
// (documentation/README.md:150; the commented-out super_smooth_median of math.cairo:128-129); the smooth median,
// the mean, a trimmed mean, the minimum and the maximum are other weight rows.  Everything around the estimator is
// the fast fp32 round (consensus_fast_f32.hip; CPU twin: reference_cpu.cpp lest_round_one): qr about c1, rel1, the
// rank mask, the verdict ladder, rel2, the moments of the reliable rows, commit on OK.
//
// MI355X mapping (consensus_fast_f32.hip's layout):
//   * lane = column; NSEG = lane_groups(N) lanes share a column (64 rows per lane, N <= 256: NSEG 1 / 2 / 4); row
//     offsets ride in SGPR soffsets of one buffer resource per instance;
//   * the selection networks of the other fast kernels yield the middle pair or a window; this one needs every
//     rank, so it runs the full sorts of sortnet.hpp on the f32_key keys: sort_oem<64> in the lane, sort_group
//     across the lane group.  Afterwards register i of segment s holds rank 64 s + i (group_select's mapping);
//   * rows past N (pass 2: unreliable rows too) sort as ~0 keys to the top ranks.  Their key decodes to NaN, so
//     they are selected out, not multiplied: a term enters the sum only where its weight is non-zero, and the
//     staged weights are zero from the count on.  A zero weight contributes exactly zero for the same reason;
//   * w1 / w2 are staged into LDS once per workgroup, one 64-float row per segment at a 68-float pitch (16-byte
//     aligned float4 reads; the segments of a wave read disjoint banks);
//   * the weighted sum is an fp64 fma chain in ascending rank inside the lane, then a butterfly over the group's
//     lanes, rounded to fp32 once;
//   * pass 2 reads each column once: the power sums of the reliable rows shifted by c1, their min / max key (a
//     constant column is ZERO_VARIANCE, decided exactly) and the sort keys come from the same registers; the
//     cancellation guard re-reads a column whose mean sits far from c1;
//   * outputs are staged in the workspace and committed only when the round's status is OK.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "svoc/bufload.hpp"
#include "svoc/route.hpp"
#include "svoc/sortnet.hpp"
#include "svoc/rankmask.hpp"
#include "svoc/status.hpp"
#include "svoc/verdict.hpp"

namespace svoc {
namespace lest {

constexpr int kPitch = 68;   // floats between the segments' weight rows in LDS

// qtree / qtree_all, load_col and seg_sum below, and the pass-2 power sums with their cancellation guard in the
// kernel, are copies of consensus_fast_f32.hip's (kept there untouched, so that kernel compiles as before): the two
// must stay in step, with ONE difference, the guard's re-read.  There c1 is a median of the column and the re-read
// stays in fp32 about c1 + dl; here the weights may put c1 anywhere, so the guard also fires on sums that are not
// finite and the re-read works in fp64 about the fp64 mean of the reliable rows (see the guard in pass 2).
// reduce_qr, rank_mask_general, round_verdict, stage_out / commit_staged are the shared headers.

// Transposing butterfly over the wave's P columns (consensus_fast_f32.hip qtree_f): the lane ends with rows
// I + base(lane) summed over all P columns.
template <int L, int I, int P>
SVOC_DEV float qtree(const float (&q)[64], int lane) {
  if constexpr (L == 0) {
    return q[I];
  } else {
    constexpr int msk = P >> L;
    const float lo_v = qtree<L - 1, I, P>(q, lane);
    const float hi_v = qtree<L - 1, I + (64 >> L), P>(q, lane);
    const bool up = (lane & msk) != 0;
    const float send = up ? lo_v : hi_v;
    const float keep = up ? hi_v : lo_v;
    return keep + xor_lane<msk>(send);
  }
}
template <int P, int... Is>
SVOC_DEV void qtree_all(const float (&q)[64], int lane, float* acc, std::integer_sequence<int, Is...>) {
  ((acc[Is] += qtree<__builtin_ctz(P), Is, P>(q, lane)), ...);
}

// The lane's 64 rows of one column, every load issued before any is consumed.
SVOC_DEV void load_col(__amdgpu_buffer_rsrc_t rs, int vo, int rowb, uint32_t (&x)[64]) {
  asm volatile("" : "+s"(rowb));   // the 64 row soffsets are recomputed here, not kept live across the slab loop
#pragma unroll
  for (int i = 0; i < 64; ++i) x[i] = bload(rs, vo, i * rowb);
  __builtin_amdgcn_sched_barrier(0);
}

template <int NSEG, int P, class T>
SVOC_DEV T seg_sum(T v) {
#pragma unroll
  for (int t = 1; t < NSEG; t <<= 1) v += __shfl_xor(v, t * P);
  return v;
}

// Full ascending sort of the group's 64 NSEG keys: register i of segment s ends as rank 64 s + i.
template <int NSEG, int P>
SVOC_DEV void sort_col(uint32_t (&r)[64], int seg) {
  if constexpr (NSEG == 1) sort_oem<64>(r);
  else sort_group<NSEG, P>(r, seg);
}

// sum_k w[k] x(k) over the group's sorted keys; w: this segment's 64 weights in LDS (16-byte aligned).  A term
// enters only where its weight is non-zero: the sentinel keys (NaN) sit at ranks whose staged weight is zero.
// Accumulated in fp64 and rounded to fp32 once: an fp32 chain rounds at the size of its partial sums, ~ w x the
// largest |x|, and under weights that are not robust (outliers of both signs at weighted ranks) that is far more
// than an ulp of the result -- enough to move the qr of the rows next to the centre past their tolerance.
template <int NSEG, int P>
SVOC_DEV float weighted_sum(const uint32_t (&r)[64], const float* w) {
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 64; i += 4) {
    const float4 w4 = *(const float4*)(w + i);
    const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x = fand(key_f32(r[i + j]), wv[j] != 0.f ? 0xffffffffu : 0u);
      acc = __builtin_fma((double)wv[j], (double)x, acc);   // the product of two fp32 values is exact in fp64
    }
  }
  return (float)seg_sum<NSEG, P>(acc);
}

template <int NSEG, int WAVES, bool CONS>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(1))) void consensus_fast_lest_kernel(LestParams lp) {
  const FastParams& p = lp.f;
  constexpr int P = 64 / NSEG;      // columns per wave
  constexpr int NPAD = 64 * NSEG;   // padded oracle rows
  constexpr int W = WAVES * P;      // columns per slab
  constexpr int NT = WAVES * 64;
  constexpr int KEEP = 64 / P;      // qr rows a lane holds after the butterfly
  static_assert(NT == 256, "the weight staging covers 256 ranks with one thread each");
  __shared__ float qr_part[WAVES * NPAD];
  __shared__ __attribute__((aligned(16))) float qr_lds[NPAD];   // (float4 reads: rank_mask_general)
  __shared__ __attribute__((aligned(16))) float wts[2][4 * kPitch];
  constexpr int NM = 4;   // 64-row mask words
  __shared__ uint64_t relmask[NM];
  __shared__ float rels[2];
  __shared__ int st_sh, zv_sh;

  const int b = blockIdx.x;
  if (p.active && !p.active[b]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = p.N, D = p.D;
  if (p.n_failing > N) {   // reference_cpu.cpp lest_round_one: checked before anything is computed
    if (tid == 0) p.status[b] = ST_USIZE_UNDERFLOW;
    return;
  }
  const int R = N - p.n_failing;
  if (tid == 0) zv_sh = 0;
  {
    // rank tid's weights, zero from the count on (pass 1: N ranks, pass 2: R)
    const int at = (tid >> 6) * kPitch + (tid & 63);
    wts[0][at] = tid < N ? lp.weights[tid] : 0.f;
    wts[1][at] = tid < R ? lp.weights[256 + tid] : 0.f;
  }
  __syncthreads();
  const int seg = lane / P, cw = lane % P;
  const int rowb = p.ld * 4;
  const __amdgpu_buffer_rsrc_t rs =
      instance_rsrc((const float*)p.values + (int64_t)b * p.inst_stride, (uint32_t)(N * rowb));
  const int nslab = (D + W - 1) / W;
  const int nv = N - seg * 64;           // this lane's rows < nv are real
  const int seg_off = seg * 64 * rowb;
  const float* w1 = &wts[0][seg * kPitch];
  const float* w2 = &wts[1][seg * kPitch];

  float acc[KEEP];
#pragma unroll
  for (int k = 0; k < KEEP; ++k) acc[k] = 0.f;

  // ------------------------------------------------------------ pass 1
#pragma nounroll
  for (int s = 0; s < nslab; ++s) {
    const int col = s * W + wave * P + cw;
    const bool vc = col < D;
    const int vo = seg_off + (vc ? col : 0) * 4;
    int nvl = nv;
    asm volatile("" : "+v"(nvl));   // opaque per slab: stop LICM from hoisting 64 row masks
    const uint32_t vcm = vc ? 0xffffffffu : 0u;
    float q[64];
    // the raw column stays in registers across the sort: no re-read for the quadratic risk
    uint32_t xs[64], r[64];
    load_col(rs, vo, rowb, xs);
#pragma unroll
    for (int i = 0; i < 64; ++i) r[i] = f32_key(xs[i]) | ~lt_mask(i, nvl);   // rows >= N: ~0, the top ranks
    sort_col<NSEG, P>(r, seg);
    const float c1 = weighted_sum<NSEG, P>(r, w1);
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const float y = __builtin_bit_cast(float, xs[i]) - c1;
      q[i] = fand(y * y, vcm & lt_mask(i, nvl));   // a mask, not a multiply: columns past D may hold anything
    }
    if (seg == 0 && vc) p.c1[(int64_t)b * D + col] = c1;
    qtree_all<P>(q, lane, acc, std::make_integer_sequence<int, KEEP>{});
  }
  {
    int base = 0;
#pragma unroll
    for (int h = 32, msk = P / 2; msk >= 1; h >>= 1, msk >>= 1) base += (lane & msk) ? h : 0;
#pragma unroll
    for (int k = 0; k < KEEP; ++k) qr_part[wave * NPAD + seg * 64 + base + k] = acc[k];
  }
  __syncthreads();
  reduce_qr<NT, NPAD, WAVES, 0>(p, b, N, tid, qr_part, qr_lds);

  // ------------------------------------------------------------ rank mask, verdict (rankmask.hpp, verdict.hpp)
  rank_mask_general<NT, NPAD, NM>(qr_lds, N, R, tid, relmask);   // (NT = 256: the four waves write the four words)
  __syncthreads();
  if (tid == 0) {
    // fp64 sums of the fp32 qr, sequential: the CPU twin's order (reference_cpu.cpp lest_round_one)
    double s_all = 0.0, s_rel = 0.0;
    for (int t = 0; t < N; ++t) {
      s_all += (double)qr_lds[t];
      if ((relmask[t >> 6] >> (t & 63)) & 1) s_rel += (double)qr_lds[t];
    }
    const RelF64 rel{CONS, rel_divisor<double>(false, p.rel_dim, D), (double)p.max_spread, N, R};
    const Verdict v = round_verdict(rel, s_all, s_rel, R, false);
    rels[0] = v.rel1;
    rels[1] = v.rel2;
    st_sh = v.status;
  }
  __syncthreads();
  if (st_sh != ST_OK) {
    if (tid == 0) p.status[b] = st_sh;
    return;   // revert: outputs untouched
  }

  // ------------------------------------------------------------ pass 2
  const int Dp = p.work_pairs, D2 = 2 * Dp;
  const int STG = Dp * (2 * 17 + 8 + 2) * 4;   // launch.hpp: fast_work_stage_word
  const __amdgpu_buffer_rsrc_t ws = instance_rsrc(p.work + (int64_t)b * p.work_stride, (uint32_t)(p.work_stride * 4));
  const uint64_t mymask = relmask[seg];
  const double n = (double)R, inv_n = 1.0 / n;
  const double k3 = n / ((n - 1.0) * (n - 2.0));
  const double k4a = n * (n + 1.0) / (n - 1.0), k4b = 3.0 * (n - 1.0) * (n - 1.0), k4c = (n - 2.0) * (n - 3.0);
  bool zv = false;
#pragma nounroll
  for (int s = 0; s < nslab; ++s) {
    const int col = s * W + wave * P + cw;
    const bool vc = col < D;
    const int vo = seg_off + (vc ? col : 0) * 4;
    uint64_t mm = mymask;
    asm volatile("" : "+v"(mm));   // keep the 64 row masks out of the slab loop's live set
    float sh = 0.f;       // constrained: the pass-2 estimate (the consensus)
    // ONE read of the column: the sort keys of pass 2 and, from the same registers, the reliable rows' power sums
    // shifted by c1 (written by pass 1) plus their min / max key (a constant column is decided exactly)
    const float c1c = vc ? p.c1[(int64_t)b * D + col] : 0.f;
    float s1f = 0.f, s2f = 0.f, s3f = 0.f, s4f = 0.f;
    uint32_t kmn = ~0u, kmx = 0u;
    {
      uint32_t r[64];
      load_col(rs, vo, rowb, r);
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        if ((i & 7) == 0) __builtin_amdgcn_sched_barrier(0);   // stream the rows: raw value -> key in place
        const uint32_t mk = bit_mask(mm, i);
        const float y = fand(__builtin_bit_cast(float, r[i]) - c1c, mk);
        const float y2 = y * y;
        s1f += y;
        s2f += y2;
        s3f = __builtin_fmaf(y2, y, s3f);
        s4f = __builtin_fmaf(y2, y2, s4f);
        const uint32_t key = f32_key(r[i]);
        kmn = min(kmn, key | ~mk);
        kmx = max(kmx, key & mk);
        if constexpr (CONS) r[i] = key | ~mk;   // reliable: key; else ~0, the top ranks
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (CONS) {
        sort_col<NSEG, P>(r, seg);
        sh = weighted_sum<NSEG, P>(r, w2);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 1; t < NSEG; t <<= 1) {
      kmn = min(kmn, (uint32_t)__shfl_xor((int)kmn, t * P));
      kmx = max(kmx, (uint32_t)__shfl_xor((int)kmx, t * P));
    }
    const bool constant = kmn == kmx;
    double s1 = seg_sum<NSEG, P>((double)s1f), s2 = seg_sum<NSEG, P>((double)s2f);
    double s3 = seg_sum<NSEG, P>((double)s3f), s4 = seg_sum<NSEG, P>((double)s4f);
    double shift = (double)c1c;
    // cancellation guard: when the reliable rows' mean sits far from c1 relative to their spread
    // (mean offset^2 > 16 x variance), or the sums about c1 are not finite (s4 is the first to overflow, and it
    // can only come out finite or +inf; the negated comparison is true for a NaN variance, but false for +inf),
    // re-read the column once and take the moments as the CPU twin does: in fp64
    // about the fp64 mean of the reliable rows.  The weights decide how far c1 follows the failing rows -- mean
    // weights put it at (f / N) x the outliers -- so neither c1 + dl (dl carries the fp32 rounding of R terms ~ c1,
    // which can exceed the reliable rows' spread) nor an fp32 power sum about it (2^80: y^2 overflows) will do.
    {
      const double dl = s1 * inv_n, mu2 = s2 * inv_n - dl * dl;
      if (!constant && (!(dl * dl <= 16.0 * mu2) || !__builtin_isfinite(s4))) {
        uint64_t mm2 = mymask;
        asm volatile("" : "+v"(mm2));
        // 16 rows at a time, the column read once for the mean and once for the moments: 64 raw values held
        // across fp64 arithmetic would cost this (rare) branch more registers than the rest of the kernel needs
        int rb2 = rowb;
        asm volatile("" : "+s"(rb2));
        double m = 0.0;
#pragma unroll
        for (int c = 0; c < 64; c += 16) {
          uint32_t xr[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) xr[k] = bload(rs, vo, (c + k) * rb2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int k = 0; k < 16; ++k) m += (double)fand(__builtin_bit_cast(float, xr[k]), bit_mask(mm2, c + k));
          __builtin_amdgcn_sched_barrier(0);
        }
        m = seg_sum<NSEG, P>(m) * inv_n;
        double t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;
#pragma unroll
        for (int c = 0; c < 64; c += 16) {
          uint32_t xr[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) xr[k] = bload(rs, vo, (c + k) * rb2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const double y = bit_mask(mm2, c + k) ? (double)__builtin_bit_cast(float, xr[k]) - m : 0.0;
            const double y2 = y * y;
            t1 += y;
            t2 += y2;
            t3 = __builtin_fma(y2, y, t3);
            t4 = __builtin_fma(y2, y2, t4);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        s1 = seg_sum<NSEG, P>(t1); s2 = seg_sum<NSEG, P>(t2);
        s3 = seg_sum<NSEG, P>(t3); s4 = seg_sum<NSEG, P>(t4);
        shift = m;
      }
    }
    // central moments from the shifted sums
    const double dl = s1 * inv_n, e2 = s2 * inv_n, e3 = s3 * inv_n, e4 = s4 * inv_n;
    const double mu2 = e2 - dl * dl;
    const double mu3 = e3 - 3.0 * dl * e2 + 2.0 * dl * dl * dl;
    const double mu4 = e4 - 4.0 * dl * e3 + 6.0 * dl * dl * e2 - 3.0 * dl * dl * dl * dl;
    if (seg == 0 && vc) {
      float sk = 0.f, ku = 0.f;
      if (constant || mu2 <= 0.0) {
        zv = true;
      } else {
        const double sd = sqrt(mu2);
        const double z3 = n * mu3 / (mu2 * sd), z4 = n * mu4 / (mu2 * mu2);
        sk = (float)(z3 * k3);
        ku = (float)((z4 * k4a - k4b) / k4c);
      }
      stage_out(ws, STG, D2, 0, col, CONS ? sh : (float)(shift + dl));
      stage_out(ws, STG, D2, 1, col, sk);
      stage_out(ws, STG, D2, 2, col, ku);
    }
  }
  if (zv) zv_sh = 1;
  __syncthreads();
  // ------------------------------------------------------------ commit (a successful round only)
  if (zv_sh) {
    if (tid == 0) p.status[b] = ST_ZERO_VARIANCE;
    return;
  }
  const int64_t ob = (int64_t)b * D;
  commit_staged<NT>(ws, STG, D2, D, tid, p.consensus + ob, p.skew + ob, p.kurt + ob);
  for (int t = tid; t < N; t += NT) {
    p.reliable[(int64_t)b * N + t] = (relmask[t >> 6] >> (t & 63)) & 1;
    p.qr[(int64_t)b * N + t] = qr_lds[t];
  }
  if (tid == 0) {
    p.rel[2 * (int64_t)b] = rels[0];
    p.rel[2 * (int64_t)b + 1] = rels[1];
    p.status[b] = ST_OK;
  }
}

template <int NSEG>
static int launch(const LestParams& p, hipStream_t stream) {
  constexpr int WAVES = 4;
  auto k = p.f.constrained ? consensus_fast_lest_kernel<NSEG, WAVES, true> : consensus_fast_lest_kernel<NSEG, WAVES, false>;
  hipLaunchKernelGGL(k, dim3(p.f.B), dim3(WAVES * 64), 0, stream, p);
  return (int)hipGetLastError();
}

}  // namespace lest
}  // namespace svoc

using namespace svoc;

// -1: shape / workspace outside what the kernel supports (lest_route; the binding checks these first).
extern "C" int svoc_lest_round_f32(const LestParams* lp, hipStream_t stream) {
  const FastParams& p = lp->f;
  if (p.B <= 0) return 0;
  const LestRoute r = lest_route(fast_shape(p, kStoreF32));
  if (!r.supported || !lp->weights || !p.c1 || !p.c1_out) return -1;
  if (!p.work || p.work_pairs < fast_work_pairs(p.D) || p.work_stride < fast_work_words(p.D))
    return -1;   // pass 2 stages its outputs in the workspace
  int rc;
  switch (r.lane_groups) {
    case 1: rc = lest::launch<1>(*lp, stream); break;
    case 2: rc = lest::launch<2>(*lp, stream); break;
    default: rc = lest::launch<4>(*lp, stream);
  }
  // c1 was staged: committed where the round succeeded
  if (rc == 0) rc = svoc_commit_rows(p.c1, p.c1_out, p.status, p.active, p.B, p.D, stream);
  return rc;
}
