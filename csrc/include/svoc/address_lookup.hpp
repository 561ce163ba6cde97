// Batched find_oracle_index / admin lookup (contract/src/contract.cairo:505-518 find_oracle_index, the
// linear scan behind update_prediction's 'not an oracle'): K (instance, address) pairs against a
// [B, M, 4] table of 4 x int64 limb addresses, host+device.
//
//   out[k] = the lowest i with table[inst[k]][i] == addr[k] on all four limbs, -1 when there is none,
//            -1 when inst[k] is outside [0, B) (the table is not read for such an entry).
#pragma once

#include <stdint.h>

#include "governance.hpp"  // addr_eq

namespace svoc {

struct AddrLookup {
  const int64_t* table;  // [B, M, 4]
  const int64_t* inst;   // [K]
  const int64_t* addr;   // [K, 4]
  int64_t* out;          // [K]
  int64_t B;
  int64_t K;
  int M;
};

// the scalar twin of address_lookup.hip (the CPU op; the kernel's reference)
SVOC_HD int64_t find_address_one(const AddrLookup& p, int64_t k) {
  const int64_t b = p.inst[k];
  if (b < 0 || b >= p.B) return -1;
  const int64_t* row = p.table + b * p.M * 4;
  const int64_t* a = p.addr + k * 4;
  for (int i = 0; i < p.M; ++i)
    if (addr_eq(row + (int64_t)i * 4, a)) return i;
  return -1;
}

}  // namespace svoc
