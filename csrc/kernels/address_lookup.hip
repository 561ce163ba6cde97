// Batched address lookup (find_oracle_index, contract.cairo:505-518): out[k] = the lowest index of addr[k]
// in table[inst[k]], -1 when absent or when the instance is unknown (address_lookup.hpp).
//
// L lanes per lookup, L = the power of two covering the table's M entries, capped at 64 -- the update
// kernels' shape (updates.hip): the deployed 7-oracle tables run 8 lookups per wave, wide tables (256,
// 4096) a whole wave per lookup.  Each lane loads one 32-B entry (two 16-B vector loads; consecutive
// lanes read consecutive entries) and compares it; a ballot masked to the lane group names the chunk's
// first match.  Chunks of L entries go in ascending order and a group stops loading after its first hit,
// so the result is the linear scan's.  M is uniform per launch: every lane of a wave runs the same
// number of chunks and reaches every ballot (no lane returns before the last one).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svoc/address_lookup.hpp"

namespace svoc {

typedef int64_t i64x2 __attribute__((ext_vector_type(2)));

template <int L>
__global__ __launch_bounds__(256) void find_address_kernel(AddrLookup p) {
  const int64_t k = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
  const int sub = threadIdx.x & (L - 1);
  const int lane = threadIdx.x & 63;
  const int g0 = lane & ~(L - 1);   // the group's first lane
  const uint64_t gm = (L == 64) ? ~0ull : (((1ull << (L & 63)) - 1ull) << g0);
  const bool in = k < p.K;
  int64_t b = -1;
  int64_t a[4] = {0, 0, 0, 0};
  if (in) {
    b = p.inst[k];
    const i64x2* ap = (const i64x2*)(p.addr + k * 4);
    const i64x2 lo = ap[0], hi = ap[1];
    a[0] = lo.x; a[1] = lo.y; a[2] = hi.x; a[3] = hi.y;
  }
  const bool known = in && b >= 0 && b < p.B;   // unknown instance: the table is not read
  const i64x2* row = (const i64x2*)(p.table + (known ? b : 0) * p.M * 4);
  int64_t found = -1;   // uniform over the group (taken from the group's ballot bits)
  for (int base = 0; base < p.M; base += L) {
    const int i = base + sub;
    bool hit = false;
    if (known && found < 0 && i < p.M) {
      const i64x2 lo = row[(int64_t)i * 2], hi = row[(int64_t)i * 2 + 1];
      const int64_t e[4] = {lo.x, lo.y, hi.x, hi.y};
      hit = addr_eq(e, a);
    }
    const uint64_t m = __ballot(hit) & gm;
    if (found < 0 && m) found = base + (__builtin_ctzll(m) - g0);
  }
  if (in && sub == 0) p.out[k] = found;
}

template <int L>
static int launch_find(const AddrLookup& p, hipStream_t stream) {
  const int64_t blocks = (p.K * L + 255) / 256;
  hipLaunchKernelGGL(find_address_kernel<L>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
  return (int)hipGetLastError();
}

}  // namespace svoc

using namespace svoc;

extern "C" int svoc_find_address(const AddrLookup* p, hipStream_t stream) {
  if (p->K <= 0) return 0;
  if (p->K * 64 / 256 >= 0x7fffffffll) return -1;
  if (p->M <= 1) return launch_find<1>(*p, stream);
  if (p->M <= 2) return launch_find<2>(*p, stream);
  if (p->M <= 4) return launch_find<4>(*p, stream);
  if (p->M <= 8) return launch_find<8>(*p, stream);
  if (p->M <= 16) return launch_find<16>(*p, stream);
  if (p->M <= 32) return launch_find<32>(*p, stream);
  return launch_find<64>(*p, stream);
}
