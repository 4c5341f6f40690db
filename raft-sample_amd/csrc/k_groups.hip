// k_groups.hip — the group directory (raft_group_scan, raft_store_groups,
// raft_restart_groups): find groups by their fault code or lack of a leader,
// read the canonical view of a list of groups, restart listed groups.
//
// Scan: count, scan, emit, like the commit feed (k_feed.hip); no block waits
// for another.
//   group_count_kernel<R>  one lane per group decides hit or not from gmeta's
//        fault field and the R role words of the group's record (the rows
//        raft_store_state reports: gmeta's primary field is not read, it names
//        a leader only under STEADY / ONECAND / ONESTALE) and writes the
//        block's number of hits;
//   feed_scan_kernel       (k_feed.hip) the exclusive scan of the block sums
//        and the total;
//   group_emit_kernel<R>   every block below the cap decides again, places
//        its hits by ballot and prefix inside the wave (consecutive hits are
//        consecutive 16-B records) and the lane that writes the last record
//        stores the id after it.
// Gather: the canonical view (canon_view.hpp) of ids[0..n), or of the range
// [first, first + n), into a staging buffer in the view's layout: one lane per
// listed group for the scalars and the match / next rows, one wave per listed
// group for the logs. Every host read of the view goes through it
// (raft_store_state / _range / _groups, raft_nodelog).
// Restart: init_new_group (tick_common.hpp) for g = ids[i], feed cursors to 0.
// Scatter: the inverse of the gather, the one writer of a loaded group
// (raft_load_groups, raft_load_state, raft_checkpoint_load): the view's rows
// in a staging buffer, indexed by list position, become the internal words of
// ids[0..n) or of the range [first, first + n) (scatter_view.hpp); one lane
// per listed group for the per-group words, one wave per listed group for its
// ring tile column. Distinct ids: no two lanes or waves store the same word.
#include "canon_view.hpp"
#include "scatter_view.hpp"

namespace raftstep {

namespace {

// Is group g a hit, and the lowest-id replica whose State is Leader (0xFF: none).
template <int R>
__device__ __forceinline__ bool group_hit(const DevPlanes& P, uint32_t g, uint32_t select, uint32_t* fault,
                                          uint32_t* leader) {
  const uint32_t f = (uint32_t(at(P.gmeta, g)) >> 4) & 7u;
  uint32_t ld = 0xFFu;
#pragma unroll
  for (int r = R - 1; r >= 0; --r)
    if ((uint32_t(at(P.rs, rix<R>(g, r))) & 3u) == uint32_t(ROLE_L)) ld = uint32_t(r);
  *fault = f;
  *leader = ld;
  return ((select & 1u) && f != 0u) || ((select & 2u) && f == 0u && ld == 0xFFu);
}

}  // namespace

// Blocks cover groups from block b0 = first / 256 on; groups below `first` are no hits.
template <int R>
__global__ __launch_bounds__(256) void group_count_kernel(DevPlanes P, uint32_t select, uint32_t first, uint32_t b0,
                                                          uint32_t* bsum) {
  __shared__ uint32_t s_w[4];
  const uint32_t g = (b0 + blockIdx.x) * 256u + threadIdx.x;
  bool hit = false;
  if (g < P.G && g >= first) {
    uint32_t f, ld;
    hit = group_hit<R>(P, g, select, &f, &ld);
  }
  const uint32_t n = uint32_t(__popcll(__ballot(hit)));
  if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// cap >= 1: the records this scan writes (min of the caller's cap and the
// total); hit p of the ascending group order is written iff p < cap, and the
// lane that writes hit cap - 1 stores its group's id + 1 to *next.
template <int R>
__global__ __launch_bounds__(256) void group_emit_kernel(DevPlanes P, uint32_t select, uint32_t first, uint32_t b0,
                                                         const uint64_t* boff, uint64_t cap, uint32_t* out,
                                                         unsigned long long* next) {
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  __shared__ uint32_t s_w[4];
  const uint64_t base = boff[blockIdx.x];
  if (base >= cap) return;   // (the whole block: nothing of it is written)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t g = (b0 + blockIdx.x) * 256u + threadIdx.x;
  bool hit = false;
  uint32_t f = 0, ld = 0xFFu;
  if (g < P.G && g >= first) hit = group_hit<R>(P, g, select, &f, &ld);
  const unsigned long long b = __ballot(hit);
  if (lane == 0) s_w[wave] = uint32_t(__popcll(b));
  __syncthreads();
  uint64_t pos = base + uint32_t(__popcll(b & ((1ull << lane) - 1ull)));
  for (uint32_t w = 0; w < wave; ++w) pos += s_w[w];
  if (!hit || pos >= cap) return;
  const uint64_t gid = P.gbase + g;
  // raft_group_hit: group, local, fault | leader << 8 | reserved 0
  reinterpret_cast<u4*>(out)[pos] = u4{uint32_t(gid), uint32_t(gid >> 32), g, f | (ld << 8)};
  if (pos == cap - 1) *next = uint64_t(g) + 1u;
}

// The scalars and the match / next rows of listed group i < n, one lane each
// (ids null: the range g = first + i).
template <int R>
__global__ __launch_bounds__(256) void gather_scalar_kernel(DevPlanes P, int raft, uint32_t first, const uint32_t* ids,
                                                            uint32_t n, GatherOut o) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = ids ? ids[i] : first + i;
  const CanonGroup<R> c(P, g);
  const int hb = o.deadline ? c.hb(P) : 0;
  int last[R];
#pragma unroll
  for (int r = 0; r < R; ++r) last[r] = c.last(P, r);
  if (o.fault) o.fault[i] = uint8_t(c.fault);
  if (o.iso_victim) o.iso_victim[i] = uint8_t(at(P.giso, g));
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    const uint32_t x = at(P.rs, rix<R>(g, r));
    const int role = rs_role(x), dur = rs_timeout(x);
    const int l = sel(last, r);
    const uint32_t k = i * uint32_t(R) + uint32_t(r);
    if (o.role) o.role[k] = uint8_t(role);
    if (o.voted) o.voted[k] = uint8_t(rs_voted(x));
    if (o.term) o.term[k] = c.term(P, r);
    if (o.last) o.last[k] = l;
    if (o.commit) o.commit[k] = c.commit(P, r);
    if (o.deadline) o.deadline[k] = canon_deadline(role, at(P.tstart, rix<R>(g, r)), hb, dur);
    if (o.timeout) o.timeout[k] = dur;
    if (o.hwm) o.hwm[k] = c.hwm(P, r, raft, l);
    if (o.match || o.next) {
#pragma unroll 1
      for (int p = 0; p < R; ++p) {
        int m, nx;
        c.match_next(P, raft, role, r, p, last, &m, &nx);
        if (o.match) o.match[size_t(k) * R + p] = m;
        if (o.next) o.next[size_t(k) * R + p] = nx;
      }
    }
  }
}

// The log fields of listed groups, one wave per group: lane j of a pass is
// (replica, slot) = (j / K, j % K), so the wave writes output rows
// [(i R + r) K + s] contiguously; the reads are scattered over the group's
// ring tile (its R-word runs, 64 R words apart). Slot s holds the largest
// index idx <= last with (idx - 1) mod K == s, live when idx > max(0, hwm - K).
// bad (may be null; with log_term only): the last-entry term check. Lane r < R
// compares the term the engine caches for replica r's last entry with the
// ring's entry at `last`; a mismatch records ~(g R + r) with atomicMax, so
// the word, zero before the launch, stays zero when clean and otherwise names
// the lowest (group, replica).
template <int R>
__global__ __launch_bounds__(256) void gather_log_kernel(DevPlanes P, int raft, uint32_t first, const uint32_t* ids,
                                                         uint32_t n, GatherOut o, uint32_t* bad) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= n) return;   // (wave-uniform)
  const uint32_t g = ids ? ids[i] : first + i;
  const CanonGroup<R> c(P, g);
  const RingForm rf = ring_form(P, g);
  // (a view without a field reads none of its ring words)
  const int want = (o.log_term ? EW_TERM : 0) | (o.log_value ? EW_VALUE : 0) | (o.log_crc ? EW_CRC : 0);
  if (bad && o.log_term && lane < uint32_t(R)) {
    const int l = c.last(P, int(lane));
    if (l > 0 && canon_entry<R>(P, rf, g, lane, l, EW_TERM).term != c.last_term(P, int(lane)))
      atomicMax(bad, ~(g * uint32_t(R) + lane));
  }
  const uint32_t K = P.K, RK = uint32_t(R) * K;
  const size_t ob = size_t(i) * RK;
  for (uint32_t j = lane; j < RK; j += 64u) {
    const uint32_t r = j / K, s = j & (K - 1u);
    const int l = c.last(P, int(r));
    const int hwm = c.hwm(P, int(r), raft, l);
    const int idx = l >= 1 ? l - int(uint32_t(l - 1 - int(s)) & (K - 1u)) : 0;
    const bool live = idx >= 1 && idx > hwm - int(K);
    const Entry e = live ? canon_entry<R>(P, rf, g, r, idx, want) : Entry{0, 0, 0};
    if (o.log_term) o.log_term[ob + j] = e.term;
    if (o.log_value) o.log_value[ob + j] = e.value;
    if (o.log_crc) o.log_crc[ob + j] = e.crc;
  }
}

// NewNode x R for the listed groups (distinct ids); cur (may be null): the
// commit feed's cursors [G][nm], the listed groups' become 0 =
// min(CommitIndex, LastApplied) of the new state.
template <int R>
__global__ __launch_bounds__(256) void restart_kernel(DevPlanes P, Trace T, const uint32_t* ids, uint32_t n, int32_t* cur,
                                                      uint32_t nm) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = ids[i];
  init_new_group<R>(P, T, g);
  if (cur)
    for (uint32_t k = 0; k < nm; ++k) cur[size_t(g) * nm + k] = 0;
}

// Every per-group word of listed group i < n but its ring column, one lane
// each (ids null: the range g = first + i): the record rows, gmeta, hb, the
// cold ring words, giso, the leaders' match / next rows (the primary's in the
// record, every further leader's in xmatch / xnext and 0 in every other row
// there) and, with cur, the open feed's cursors of the group. The term of a
// replica's last entry (lterm) is read from the view's log_term row here.
template <int R>
__global__ __launch_bounds__(256) void scatter_scalar_kernel(DevPlanes P, int raft, uint32_t first, const uint32_t* ids,
                                                             uint32_t n, ScatterIn in, int32_t* cur, uint32_t mask,
                                                             uint32_t nm) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = ids ? ids[i] : first + i;
  const uint32_t K = P.K;
  int primary = NO_PRIMARY;
#pragma unroll 1
  for (int r = R - 1; r >= 0; --r)
    if (in.role[i * uint32_t(R) + uint32_t(r)] == uint8_t(ROLE_L)) primary = r;
  bool steady = primary != NO_PRIMARY;
  uint32_t ck = 0;
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    const uint32_t k = i * uint32_t(R) + uint32_t(r);
    const uint32_t x = rix<R>(g, r);
    const uint32_t role = in.role[k];
    const int32_t last = in.last[k], commit = in.commit[k], timeout = in.timeout[k];
    // (a follower with timeout 0 fires in the tick of the heartbeat that resets it: not a STEADY group)
    if (r != primary && (role != uint32_t(ROLE_F) || timeout == 0)) steady = false;
    at(P.term, x) = in.term[k];
    at(P.last, x) = last;
    at(P.commit, x) = commit;
    at(P.tstart, x) = scat_tstart(in.deadline[k], timeout);
    at(P.lterm, x) = last > 0 ? in.log_term[size_t(k) * K + scat_last_slot(last, K)] : 0;
    at(P.rs, x) = scat_rs(role, in.voted[k], timeout);
    if (raft) at(P.hwm, x) = scat_hwm(in.hwm, k, last);
    // the primary's row for peer r (0: no primary, or r is the primary itself)
    const bool prow_live = primary != NO_PRIMARY && r != primary;
    const size_t pk = (size_t(i) * R + uint32_t(prow_live ? primary : 0)) * R + uint32_t(r);
    const int32_t pm = prow_live ? in.match[pk] : 0;
    at(P.lmatch, x) = pm;
    if (raft) at(P.lnext, x) = prow_live ? scat_next(in.next, pk, pm) : 0;
    // replica r's own row: live for a further leader, 0 otherwise
    const bool xrow = role == uint32_t(ROLE_L) && r != primary;
#pragma unroll 1
    for (int p = 0; p < R; ++p) {
      const size_t xk = size_t(k) * R + uint32_t(p);
      const bool live = xrow && p != r;
      const int32_t m = live ? in.match[xk] : 0;
      at(prow(P.xmatch, r * R + p, P.Gp), g) = m;
      if (raft) at(prow(P.xnext, r * R + p, P.Gp), g) = live ? scat_next(in.next, xk, m) : 0;
    }
    if (cur && ((mask >> r) & 1u)) cur[size_t(g) * nm + ck++] = scat_cursor(commit, last);
  }
  at(P.gmeta, g) = scat_meta(primary, in.fault[i], steady);
  at(P.hb, g) = HB_NONE;
  at(P.giso, g) = in.iso_victim ? in.iso_victim[i] : uint8_t(0);
  P.gseg[g] = GSeg{};   // (grota, grotb, gsb2, gshf: the cold words)
  at(P.grot, g) = 0;
  at(P.gsb, g) = 0;
}

// The ring tile column of listed groups, one wave per group: lane j of a pass
// is (physical slot, replica) = (j / R, j % R), so the wave stores runs of R
// contiguous words, 64 R words apart (the gather's reads mirrored), and reads
// R input rows at consecutive slots. Every physical slot of the column is
// written: the entry scat_view_slot names for it, else 0 (term, value, stamp).
// Stamps (P.crc_on): the view's, or without log_crc computed from the CRC
// table the tick kernels use.
template <int R>
__global__ __launch_bounds__(256) void scatter_log_kernel(DevPlanes P, uint32_t first, const uint32_t* ids, uint32_t n,
                                                          ScatterIn in) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= n) return;   // (wave-uniform)
  const uint32_t g = ids ? ids[i] : first + i;
  const uint32_t K = P.K, KP = P.KP, RKP = uint32_t(R) * KP;
  const uint64_t rb = ring_tile(g, KP, R);
  const size_t ib = size_t(i) * R * K;
  for (uint32_t j = lane; j < RKP; j += 64u) {
    const uint32_t ps = j / uint32_t(R), r = j - ps * uint32_t(R);
    const int s = scat_view_slot(ps, in.last[i * uint32_t(R) + r], K, KP);
    int32_t t = 0;
    int64_t v = 0;
    uint32_t c = 0;
    if (s >= 0) {
      const size_t k = ib + size_t(r) * K + uint32_t(s);
      t = in.log_term[k];
      v = in.log_value[k];
      if (P.crc_on) c = in.log_crc ? in.log_crc[k] : crc_entry(P.crc_tab, t, v);
    }
    const uint32_t q = ring_in_tile(g, R, ps, r);
    at(P.log_term + rb, q) = t;
    at(P.log_value + rb, q) = v;
    if (P.crc_on) at(P.log_crc + rb, q) = c;
  }
}

hipError_t launch_group_count(int R, const DevPlanes& P, uint32_t select, uint32_t first, uint32_t* bsum, hipStream_t s) {
  const uint32_t b0 = first >> 8, nb = uint32_t((P.G + 255) / 256) - b0;
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(group_count_kernel<RR>, dim3(nb), dim3(256), 0, s, P, select, first, b0, bsum));
  return hipGetLastError();
}
hipError_t launch_group_emit(int R, const DevPlanes& P, uint32_t select, uint32_t first, const uint64_t* boff,
                             uint64_t cap, void* out, unsigned long long* next, hipStream_t s) {
  const uint32_t b0 = first >> 8, nb = uint32_t((P.G + 255) / 256) - b0;
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(group_emit_kernel<RR>, dim3(nb), dim3(256), 0, s, P, select, first, b0, boff, cap,
                                        static_cast<uint32_t*>(out), next));
  return hipGetLastError();
}
hipError_t launch_gather(int R, const DevPlanes& P, int raft, uint32_t first, const uint32_t* ids, uint32_t n,
                         const GatherOut& o, uint32_t* bad, hipStream_t s) {
  const bool scalars = o.role || o.voted || o.term || o.last || o.commit || o.deadline || o.timeout || o.match ||
                       o.fault || o.next || o.hwm || o.iso_victim;
  if (scalars) {
    RAFT_DISPATCH_R(R, hipLaunchKernelGGL(gather_scalar_kernel<RR>, grid_for(n), dim3(256), 0, s, P, raft, first, ids, n, o));
    if (hipError_t rc = hipGetLastError()) return rc;
  }
  if (o.log_term || o.log_value || o.log_crc) {   // (no log pointer: no ring word is read)
    RAFT_DISPATCH_R(R, hipLaunchKernelGGL(gather_log_kernel<RR>, dim3((n + 3u) / 4u), dim3(256), 0, s, P, raft, first, ids,
                                          n, o, bad));
  }
  return hipGetLastError();
}
hipError_t launch_scatter(int R, const DevPlanes& P, int raft, uint32_t first, const uint32_t* ids, uint32_t n,
                          const ScatterIn& in, int32_t* cursors, uint32_t mask, uint32_t nm, hipStream_t s) {
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(scatter_scalar_kernel<RR>, grid_for(n), dim3(256), 0, s, P, raft, first, ids, n, in,
                                        cursors, mask, nm));
  if (hipError_t rc = hipGetLastError()) return rc;
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(scatter_log_kernel<RR>, dim3((n + 3u) / 4u), dim3(256), 0, s, P, first, ids, n, in));
  return hipGetLastError();
}
hipError_t launch_restart(int R, const DevPlanes& P, const Trace& T, const uint32_t* ids, uint32_t n, int32_t* cursors,
                          uint32_t nm, hipStream_t s) {
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(restart_kernel<RR>, grid_for(n), dim3(256), 0, s, P, T, ids, n, cursors, nm));
  return hipGetLastError();
}

}  // namespace raftstep
