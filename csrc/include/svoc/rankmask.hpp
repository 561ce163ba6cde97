// Rank mask of a round (contract.cairo:345-363; sort.cairo:96-101): sort the oracles by (qr asc, index desc),
// the first R = N - f are reliable.  One workgroup per instance, the per-oracle qr in LDS, and what the kernels
// read off the mask before pass 2.  relmask[w] = ballot of rows 64 w .. 64 w + 63 (rows past N: 0).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svoc {

// General form, any qr: an oracle's rank is the count of oracles before it in (qr asc, index desc).  qr: 16-byte
// aligned (float4 steps).  Writes every word w < MW that the threads t = base + tid < NPAD cover.
template <int NT, int NPAD, int MW>
SVOC_DEV void rank_mask_general(const float* qr, int N, int R, int tid, uint64_t* relmask) {
  for (int base = 0; base < NPAD; base += NT) {   // NT >= 64: one ballot word per wave-chunk
    const int t = base + tid;
    bool rel = false;
    if (t < N) {
      const float myq = qr[t];
      int rank = 0;
      const int n4 = N & ~3;
      for (int j = 0; j < n4; j += 4) {
        const float4 q4 = *(const float4*)(qr + j);
        rank += (q4.x < myq || (q4.x == myq && j > t)) ? 1 : 0;
        rank += (q4.y < myq || (q4.y == myq && j + 1 > t)) ? 1 : 0;
        rank += (q4.z < myq || (q4.z == myq && j + 2 > t)) ? 1 : 0;
        rank += (q4.w < myq || (q4.w == myq && j + 3 > t)) ? 1 : 0;
      }
      for (int j = n4; j < N; ++j) {
        const float qj = qr[j];
        rank += (qj < myq || (qj == myq && j > t)) ? 1 : 0;
      }
      rel = rank < R;
    }
    const uint64_t bal = __ballot(rel);
    if ((tid & 63) == 0 && (t >> 6) < MW) relmask[t >> 6] = bal;
  }
}

// For non-negative qr (every constrained round: sums of squares, never -0.0 or NaN) the float bits are
// order-preserving, so (qr asc, index desc) is the single 64-bit key  bits(qr) : ~index  and an oracle's rank is
// one 64-bit compare and one add per other oracle -- instead of two float compares, an index compare and the
// selects of the general form (~4x fewer VALU; the loop ran on one wave while the others waited at the barrier).
// key: LDS scratch of N uint64 (8-byte aligned).  Writes the words w < 4, exactly as the general form does.
template <int NT, int NPAD>
SVOC_DEV void rank_mask_nonneg(const float* qr, uint64_t* key, int N, int R, int tid, uint64_t* relmask) {
  for (int t = tid; t < N; t += NT) key[t] = ((uint64_t)__float_as_uint(qr[t]) << 32) | (uint32_t)~t;
  __syncthreads();
  for (int base = 0; base < NPAD; base += NT) {
    const int t = base + tid;
    bool rel = false;
    if (t < N) {
      const uint64_t my = key[t];
      int rank = 0;
      const int n2 = N & ~1;
      for (int j = 0; j < n2; j += 2) {
        rank += key[j] < my ? 1 : 0;
        rank += key[j + 1] < my ? 1 : 0;
      }
      if (N & 1) rank += key[N - 1] < my ? 1 : 0;
      rel = rank < R;
    }
    const uint64_t bal = __ballot(rel);
    if ((tid & 63) == 0 && (t >> 6) < 4) relmask[t >> 6] = bal;
  }
}

// The first reliable row (0 when there is none): the shift of the pass-2 power sums, the row a constant column
// is compared with.
template <int MW>
SVOC_DEV int first_reliable_row(const uint64_t* relmask) {
  for (int w = 0; w < MW; ++w)
    if (relmask[w]) return 64 * w + __builtin_ctzll(relmask[w]);
  return 0;
}

// Pass-2 sentinel split of the two-network kernels (one thread): of the 64 NSEG - R rows that are not reliable,
// padding included, the first `need` = ceil of half of them in row order sort low (-inf), the others high.
template <int NSEG, int MW>
SVOC_DEV void low_sentinel_mask(const uint64_t* relmask, int need, uint64_t* lowmask) {
  for (int w = 0; w < MW; ++w) {
    uint64_t nr = w < NSEG ? ~relmask[w] : 0ull, lm = 0ull;
    while (need > 0 && nr) {
      const uint64_t bit = nr & (0ull - nr);
      lm |= bit;
      nr ^= bit;
      --need;
    }
    lowmask[w] = lm;
  }
}

}  // namespace svoc
