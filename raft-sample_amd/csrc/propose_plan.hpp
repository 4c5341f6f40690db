// propose_plan.hpp — the host-side plan of a raft_propose call: the list
// positions in a stable order by group, and where each distinct group's
// segment of that order starts. propose_kernel (k_slow.inc) gives one lane to
// each segment, and the lane walks its proposals in list order.
// HIP-free (the C++ standard library alone), so the plan is tested on its own
// under the host sanitizers (tests/propose_plan_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace raftstep {

constexpr uint64_t PROPOSE_MAX = uint64_t(1) << 31;   // list positions are uint32, and so are the segment starts

struct ProposePlan {
  std::vector<uint32_t> perm;   // [n] list positions, by (group, list position)
  std::vector<uint32_t> seg;    // [segments + 1] starts in perm; seg[segments] = n (one 0 for an empty list)
  uint32_t segments() const { return uint32_t(seg.size() - 1); }
};

enum : int { PLAN_OK = 0, PLAN_TOO_LONG = 1, PLAN_RANGE = 2 };

// The group ids sit `stride` bytes apart from `first` on (the first member of
// raft_proposal). G: the engine's groups, at most 2^32. PLAN_RANGE: *bad is
// the first list position whose id is >= G; nothing of *out is meaningful then.
// O(n) for a list whose ids never descend, O(n log n) otherwise: one sort of
// the keys id << 32 | position, which are distinct, so the order is the stable
// one whatever the sort does with equal elements, and one hot group costs no
// more than n distinct ones.
inline int propose_plan(const void* first, size_t stride, uint64_t n, uint64_t G, ProposePlan* out, uint64_t* bad) {
  out->perm.clear();
  out->seg.assign(1, 0u);
  if (n > PROPOSE_MAX) return PLAN_TOO_LONG;
  auto id_at = [first, stride](uint64_t i) {
    uint64_t g;
    std::memcpy(&g, static_cast<const char*>(first) + i * stride, sizeof g);
    return g;
  };
  bool ascending = true;
  uint64_t prev = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t g = id_at(i);
    if (g >= G) {
      if (bad) *bad = i;
      return PLAN_RANGE;
    }
    ascending &= g >= prev;
    prev = g;
  }
  if (!n) return PLAN_OK;
  out->perm.resize(n);
  if (ascending) {
    for (uint64_t i = 0; i < n; ++i) out->perm[i] = uint32_t(i);
  } else {
    std::vector<uint64_t> keys(n);
    for (uint64_t i = 0; i < n; ++i) keys[i] = (id_at(i) << 32) | i;
    std::sort(keys.begin(), keys.end());
    for (uint64_t i = 0; i < n; ++i) out->perm[i] = uint32_t(keys[i]);
  }
  out->seg.clear();
  prev = ~uint64_t(0);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t g = id_at(out->perm[i]);
    if (g != prev) out->seg.push_back(uint32_t(i));
    prev = g;
  }
  out->seg.push_back(uint32_t(n));   // (n = 2^31 fits)
  return PLAN_OK;
}

}  // namespace raftstep
