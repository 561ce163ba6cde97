// Per-oracle track record after a committed round (track.hpp): rounds / flagged / streak / score of every
// instance whose round ran and came out OK; every other instance's rows are not read or written.
//
// L lanes per instance, L = the power of two covering the N oracles, capped at 64 -- the lookup kernel's
// shape (address_lookup.hip): the deployed 7-oracle instances run 8 per wave, and consecutive lanes touch
// consecutive oracles of every array (qr, reliable, flagged, streak, score: ~45 B per oracle and round, all
// streamed once).  qmax is a __shfl_xor max over the aligned lane group (offsets below L stay inside it);
// for N > 64 the wave takes one pass over the row for the max and a second for the update (the row is hot
// in cache).  N is uniform per launch: every lane of a wave runs the same number of chunks and reaches every
// shuffle; out-of-range, inactive and reverted instances are masked, never returned early.  One writer per
// cell and no atomics: results are deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "svoc/track.hpp"

namespace svoc {

__device__ __forceinline__ int64_t group_shfl_xor(int64_t v, int off) { return (int64_t)__shfl_xor((long long)v, off); }
__device__ __forceinline__ float group_shfl_xor(float v, int off) { return __shfl_xor(v, off); }

template <int L, bool EXACT>
__global__ __launch_bounds__(256) void track_update_kernel(TrackUpdate p) {
  using Q = typename std::conditional<EXACT, int64_t, float>::type;
  const int64_t b = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
  const int sub = threadIdx.x & (L - 1);
  const bool in = b < p.B;
  const bool go = in && p.active[b] != 0 && p.status[b] == ST_OK;
  const int64_t row = (go ? b : 0) * (int64_t)p.N;
  const Q* qr = (const Q*)p.qr + row;
  Q q0 = track_lowest<Q>();   // the lane's cell of the first chunk (the only chunk when N <= L)
  Q qmax = track_lowest<Q>();
  for (int base = 0; base < p.N; base += L) {
    const int i = base + sub;
    if (go && i < p.N) {
      const Q q = qr[i];
      if (base == 0) q0 = q;
      qmax = track_max(qmax, q);
    }
  }
#pragma unroll
  for (int off = L >> 1; off > 0; off >>= 1) qmax = track_max(qmax, group_shfl_xor(qmax, off));
  if (!go) return;   // (after the last cross-lane operation)
  for (int base = 0; base < p.N; base += L) {
    const int i = base + sub;
    if (i < p.N) track_cell<Q>(p, row + i, base == 0 ? q0 : qr[i], qmax);
  }
  if (sub == 0) p.rounds[b] += 1;
}

template <int L>
static int launch_track(const TrackUpdate& p, hipStream_t stream) {
  const int64_t blocks = (p.B * L + 255) / 256;
  if (p.exact)
    hipLaunchKernelGGL((track_update_kernel<L, true>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL((track_update_kernel<L, false>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
  return (int)hipGetLastError();
}

}  // namespace svoc

using namespace svoc;

extern "C" int svoc_track_update(const TrackUpdate* p, hipStream_t stream) {
  if (p->B <= 0 || p->N <= 0) return 0;
  if (p->B >= (0x7fffffffll * 256) / 64) return -1;   // the grid's x extent, at 64 lanes per instance
  if (p->N <= 1) return launch_track<1>(*p, stream);
  if (p->N <= 2) return launch_track<2>(*p, stream);
  if (p->N <= 4) return launch_track<4>(*p, stream);
  if (p->N <= 8) return launch_track<8>(*p, stream);
  if (p->N <= 16) return launch_track<16>(*p, stream);
  if (p->N <= 32) return launch_track<32>(*p, stream);
  return launch_track<64>(*p, stream);
}
