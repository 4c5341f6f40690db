// apply_records.hpp — raft_apply_open(RAFT_APPLY_FROM_RECORDS): the host-side
// check of the caller's [G][R] records and their packing into the device's
// [G][nm] layout (one record per group and replica of the mask, in replica
// order). HIP-free: engine.cpp includes it, and tests/apply_records_driver.cpp
// builds it alone under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace raftstep {

struct HostApplyRecord {   // raft_apply_record's layout
  int32_t applied, base;
  uint64_t chain;
  int64_t sum;
  int32_t div_index;
  uint16_t gaps;
  uint8_t div_peer, reserved;
};
static_assert(sizeof(HostApplyRecord) == 32, "raft_apply_record is 32 B");

// Every record of a masked replica must have 0 <= base <= applied and reserved
// == 0. Returns G * R when all do, else the position g * R + r of the first
// that does not; `out` (may be null: check only) is written only up to there.
inline uint64_t apply_records_pack(const HostApplyRecord* in, uint64_t G, uint32_t R, uint32_t mask,
                                   HostApplyRecord* out) {
  size_t k = 0;
  for (uint64_t g = 0; g < G; ++g)
    for (uint32_t r = 0; r < R; ++r) {
      if (!((mask >> r) & 1u)) continue;
      const HostApplyRecord& x = in[g * R + r];
      if (x.base < 0 || x.applied < x.base || x.reserved != 0) return g * R + r;
      if (out) out[k] = x;
      ++k;
    }
  return G * R;
}

}  // namespace raftstep
