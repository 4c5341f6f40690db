// feed_range.hpp — the log-entry range (lo, hi] a consumer of committed
// entries takes from one (group, replica) pair: the commit feed's rule
// (include/raftstep.h, "commit feed"), shared by the feed (k_feed.hip) and the
// applied state (k_apply.hip) so that both derive it alike.
#pragma once
#include "canon_view.hpp"

namespace raftstep {

// A pair whose consumer stands at c, with CommitIndex cm, LastApplied l,
// high-water mark hwm and ring depth K: hi = min(cm, l); false (stalled, lo =
// c, n = 0) when hi < c; otherwise lo = min(max(c, hwm - K), hi), the lo - c
// entries before it have left the ring, and the n = hi - lo entries lo+1 ..
// lo+n are there to take.
__device__ __forceinline__ bool feed_pair_range(int c, int cm, int l, int hwm, int K, int* lo, int* n) {
  const int hi = min(cm, l);
  *lo = c;
  *n = 0;
  if (hi < c) return false;
  *lo = min(max(c, hwm - K), hi);
  *n = hi - *lo;
  return true;
}

}  // namespace raftstep
