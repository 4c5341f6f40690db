// scatter_view.hpp — the engine's internal words of a group, derived from its
// canonical view (raft_state_view). The one device-side writer, twin of
// canon_view.hpp: the scatter kernels behind raft_load_groups, raft_load_state
// and raft_checkpoint_load (k_groups.hip) take every word they store from the
// functions below, so the rule for a loaded group lives here alone. A loaded
// group is in plain form: record planes authoritative (no MSYNC / SSYNC),
// ring rotation 0 in one segment, no shared entries, no virtual suffix.
#pragma once
#include "tick_common.hpp"

namespace raftstep {

// The rs word: role:2 | vote:4 | timer duration (canon_view.hpp reads it back)
__device__ __forceinline__ int32_t scat_rs(uint32_t role, uint32_t voted, int timeout) {
  return int32_t(role | (voted << 2) | (uint32_t(timeout) << 6));
}
// Timer start: the view's deadline is start + timeout (hb = HB_NONE never moves it)
__device__ __forceinline__ int32_t scat_tstart(int deadline, int timeout) { return deadline - timeout; }
// gmeta: primary (the lowest-id Leader, NO_PRIMARY without one) | fault << 4 |
// STEADY when every other replica is a Follower with a timeout above 0 (one
// of 0 fires in the tick of the heartbeat that resets it). No other flag: DEFER, MSYNC,
// SSYNC, VX and the one-exception forms are the tick kernels' to set.
__device__ __forceinline__ uint16_t scat_meta(int primary, uint32_t fault, bool steady) {
  return uint16_t(uint32_t(primary) | (fault << 4) | (steady ? uint32_t(M_STEADY) : 0u));
}
// RAFT NextIndex of a leader's peer: as given, absent or 0 (not positive)
// derives MatchIndex + 1 (the host refuses a row where that is 2^31)
__device__ __forceinline__ int32_t scat_next(const int32_t* next, size_t k, int32_t m) {
  const int32_t nx = next ? next[k] : 0;
  return nx > 0 ? nx : m + 1;
}
// RAFT high-water mark: absent or below LastApplied means LastApplied
__device__ __forceinline__ int32_t scat_hwm(const int32_t* hwm, size_t k, int32_t last) {
  const int32_t h = hwm ? hwm[k] : last;
  return h > last ? h : last;
}
// View slot of the last entry (index last >= 1)
__device__ __forceinline__ uint32_t scat_last_slot(int32_t last, uint32_t K) { return uint32_t(last - 1) & (K - 1u); }
// Which view slot a physical ring slot ps of a loaded group (rotation 0)
// takes its entry from, -1: none (the slot is written 0). KP == K: slot ps,
// whatever it holds. KP == 2K: view slot s = ps mod K holds the largest index
// idx <= last with (idx - 1) mod K == s; it is placed at (idx - 1) mod KP, so
// ps receives it iff that is ps (indices above LastApplied are never read).
__device__ __forceinline__ int scat_view_slot(uint32_t ps, int32_t last, uint32_t K, uint32_t KP) {
  if (KP == K) return int(ps);
  const uint32_t s = ps & (K - 1u);
  if (last < 1) return -1;
  const int32_t idx = last - int32_t(uint32_t(last - 1 - int32_t(s)) & (K - 1u));
  return (idx >= 1 && (uint32_t(idx - 1) & (KP - 1u)) == ps) ? int(s) : -1;
}
// The feed cursor of a replica of a loaded group (the restart's rule and
// RAFT_FEED_FROM_COMMIT's): everything committed so far counts as delivered
__device__ __forceinline__ int32_t scat_cursor(int32_t commit, int32_t last) { return min(commit, last); }

}  // namespace raftstep
