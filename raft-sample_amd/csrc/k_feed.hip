// k_feed.hip — the commit feed (raft_feed_*): a stream compaction of every
// replica's newly committed entries into dense 32-B records, ordered by
// (group, replica, index).
//
// Three launches per poll, none of which waits for another block:
//   feed_count_kernel<R>  one lane per group derives (lo, hi] of every masked
//        replica from the canonical view (canon_view.hpp: last, commit, hwm)
//        and the cursor, moves cursors
//        past entries that left the ring (`lost`), counts pairs whose cursor
//        is ahead (`stalled`) and writes the block's number of entries;
//   feed_scan_kernel      one block: the exclusive scan of the block sums and
//        the poll's total;
//   feed_emit_kernel<R>   every block below the cap re-derives its groups'
//        ranges, flattens each wave's entries (a wave prefix over the 64
//        counts, lane j takes the wave's j-th entry, so consecutive lanes write
//        consecutive records) and stores the new cursors.
// Order and cap come from the scan alone, so the same state and cursors give
// the same bytes.
#include "feed_range.hpp"

namespace raftstep {

namespace {

// The log-entry range of one group: per masked replica r the cursor c[r] as
// read, lo[r] (the cursor moved past what left the ring) and n[r] entries
// lo+1 .. lo+n to deliver; n = 0 and stalled for a pair whose cursor is ahead
// of min(CommitIndex, LastApplied), all of the canonical view (canon_view.hpp);
// the pair's arithmetic is feed_range.hpp's.
template <int R>
struct FeedRange {
  int c[R], lo[R], n[R];
  uint32_t stalled;
};

template <int R>
__device__ __forceinline__ void feed_range(const DevPlanes& P, uint32_t g, int raft, uint32_t mask, uint32_t nm,
                                           const int32_t* cur, FeedRange<R>& f) {
  const CanonGroup<R> cg(P, g);
  f.stalled = 0;
  uint32_t k = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    f.c[r] = f.lo[r] = f.n[r] = 0;
    if (!((mask >> r) & 1u)) continue;
    const int l = cg.last(P, r);
    const int cm = cg.commit(P, r);
    const int hwm = cg.hwm(P, r, raft, l);
    const int c = cur[size_t(g) * nm + k];
    ++k;
    f.c[r] = c;
    if (!feed_pair_range(c, cm, l, hwm, int(P.K), &f.lo[r], &f.n[r])) ++f.stalled;
  }
}

__device__ __forceinline__ unsigned long long feed_wave_sum(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

}  // namespace

// mode 0: a poll's count pass. mode 1: raft_feed_open FROM_COMMIT — every
// cursor becomes min(CommitIndex, LastApplied), nothing is counted.
// tot: [1] lost, [2] stalled (zero between polls: feed_scan_kernel re-zeroes them).
template <int R>
__global__ __launch_bounds__(256) void feed_count_kernel(DevPlanes P, int raft, uint32_t mask, uint32_t nm, int32_t* cur,
                                                         uint32_t* bsum, unsigned long long* tot, int mode) {
  __shared__ uint32_t s_w[4];
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  uint32_t n = 0, stalled = 0;
  unsigned long long lost = 0;   // (R cursors may each be 2^31 behind: 64 bits per group already)
  if (g < P.G) {
    if (mode == 1) {
      // cursor 0 never stalls and loses what the ring no longer holds: lo + n = min(cm, l)
      uint32_t k = 0;
#pragma unroll
      for (int r = 0; r < R; ++r)
        if ((mask >> r) & 1u) cur[size_t(g) * nm + k++] = 0;
    }
    FeedRange<R> f;
    feed_range<R>(P, g, raft, mask, nm, cur, f);
    uint32_t k = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!((mask >> r) & 1u)) continue;
      if (mode == 1) cur[size_t(g) * nm + k] = f.lo[r] + f.n[r];
      else if (f.lo[r] != f.c[r]) cur[size_t(g) * nm + k] = f.lo[r];
      ++k;
      n += uint32_t(f.n[r]);
      lost += uint32_t(f.lo[r] - f.c[r]);
    }
    stalled = f.stalled;
  }
  if (mode == 1) return;
  const unsigned long long wn = feed_wave_sum(n), wl = feed_wave_sum(lost), ws = feed_wave_sum(stalled);
  if ((threadIdx.x & 63u) == 0) {
    s_w[threadIdx.x >> 6] = uint32_t(wn);
    if (wl) atomicAdd(&tot[1], wl);
    if (ws) atomicAdd(&tot[2], ws);
  }
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// boff[b] = entries of the blocks before b. One block. The poll's totals go to
// `res` (pinned, coherent host memory the engine reads after its synchronise):
// res[0] = all entries, res[1] = lost, res[2] = stalled; the count pass's
// accumulators tot[1], tot[2] are zeroed for the next poll.
__global__ __launch_bounds__(256) void feed_scan_kernel(const uint32_t* bsum, uint64_t* boff, uint32_t nb,
                                                        unsigned long long* tot, unsigned long long* res) {
  __shared__ unsigned long long s_w[4];
  unsigned long long carry = 0;
  const int lane = int(threadIdx.x & 63u), wave = int(threadIdx.x >> 6);
  for (uint32_t base = 0; base < nb; base += 256u) {
    const uint32_t i = base + threadIdx.x;
    const unsigned long long v = i < nb ? bsum[i] : 0u;
    unsigned long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    unsigned long long pre = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      pre += w < wave ? s_w[w] : 0ull;
      all += s_w[w];
    }
    if (i < nb) boff[i] = carry + pre + x - v;
    carry += all;
    __syncthreads();   // s_w is rewritten by the next chunk
  }
  if (threadIdx.x == 0) {
    res[0] = carry;
    res[1] = tot[1];
    res[2] = tot[2];
    tot[1] = tot[2] = 0ull;
    __threadfence_system();
  }
}

struct __attribute__((aligned(16))) FeedRec {   // raft_feed_entry
  uint64_t group;
  uint32_t replica;
  int32_t index;
  int32_t term;
  uint32_t crc;
  int64_t value;
};
static_assert(sizeof(FeedRec) == 32, "raft_feed_entry is 32 B");

// cap: the records this poll delivers (min of the caller's cap and the total):
// record p of the (group, replica, index) order is written iff p < cap.
// PAIRED: the records of 64 entries leave as two store instructions of 1 KiB
// each, lane j writing half (j & 1) of entry (j >> 1) (+ 32), fetched from the
// lane that read the entry; otherwise every lane writes its own entry's two
// halves (two instructions of 16 B at a 32-B stride).
template <int R, bool PAIRED>
__global__ __launch_bounds__(256) void feed_emit_kernel(DevPlanes P, int raft, uint32_t mask, uint32_t nm, int32_t* cur,
                                                        const uint64_t* boff, uint64_t cap, FeedRec* out) {
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  __shared__ int s_lo[R][256], s_n[R][256];
  __shared__ uint32_t s_ex[256];        // entries of the wave's lanes before this one
  __shared__ uint32_t s_rot[256];       // grot | grota << 16
  __shared__ uint32_t s_rotb[256];
  __shared__ int s_sb[256], s_sb2[256], s_shf[256];
  __shared__ uint32_t s_w[4];
  const uint64_t base = boff[blockIdx.x];
  if (base >= cap) return;   // (the whole block: nothing of it is delivered, no cursor moves)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t g = blockIdx.x * 256u + tid;
  FeedRange<R> f;
  uint32_t n = 0;
  if (g < P.G) {
    feed_range<R>(P, g, raft, mask, nm, cur, f);
#pragma unroll
    for (int r = 0; r < R; ++r) n += uint32_t(f.n[r]);
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) f.c[r] = f.lo[r] = f.n[r] = 0;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    s_lo[r][tid] = f.lo[r];
    s_n[r][tid] = f.n[r];
  }
  if (n) {   // the ring form (canon_view.hpp), staged for the lanes that fetch this group's entries
    const RingForm rf = ring_form(P, g);
    s_rot[tid] = rf.rot | (rf.rota << 16);
    s_rotb[tid] = rf.rotb;
    s_sb[tid] = rf.sb;
    s_sb2[tid] = rf.sb2;
    s_shf[tid] = rf.sh ? rf.shf : -1;   // (-1: not in shared form; no index is negative)
  }
  uint32_t inc = n;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o);
    if (int(lane) >= o) inc += y;
  }
  const uint32_t ex = inc - n;
  const uint32_t wtot = __shfl(inc, 63);
  s_ex[tid] = ex;
  if (lane == 63) s_w[wave] = wtot;
  __syncthreads();
  uint64_t woff = base;
  for (uint32_t w = 0; w < wave; ++w) woff += s_w[w];
  // the cursors advance by exactly what is written (a pair may be cut)
  if (n) {
    uint64_t po = woff + ex;
    uint32_t k = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!((mask >> r) & 1u)) continue;
      const uint64_t room = po < cap ? cap - po : 0u;
      const int take = room < uint64_t(f.n[r]) ? int(room) : f.n[r];
      if (take) cur[size_t(g) * nm + k] = f.lo[r] + take;
      po += uint32_t(f.n[r]);
      ++k;
    }
  }
  const uint32_t* wex = s_ex + wave * 64u;
  // (a wave-uniform loop: the paired stores exchange the records across lanes)
  for (uint32_t jb = 0; jb < wtot && woff + jb < cap; jb += 64u) {
    const uint32_t j = jb + lane;
    const bool mine = j < wtot && woff + j < cap;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (mine) {
      uint32_t s = 0;   // the last lane whose entries start at or before j
#pragma unroll
      for (uint32_t step = 32; step > 0; step >>= 1)
        if (wex[s + step] <= j) s += step;
      const uint32_t t = wave * 64u + s;
      uint32_t q = j - wex[s];
      int r = 0;
      while (r < R - 1 && q >= uint32_t(s_n[r][t])) {
        q -= uint32_t(s_n[r][t]);
        ++r;
      }
      const int idx = s_lo[r][t] + 1 + int(q);
      const uint32_t gs = blockIdx.x * 256u + t;
      const uint32_t rw = s_rot[t];
      const RingForm rf{rw & 0xFFFFu, rw >> 16, s_rotb[t], s_sb[t], s_sb2[t], s_shf[t], s_shf[t] >= 0};
      const Entry e = canon_entry<R>(P, rf, gs, uint32_t(r), idx);
      const uint64_t gid = P.gbase + gs;
      w[0] = uint32_t(gid);
      w[1] = uint32_t(gid >> 32);
      w[2] = uint32_t(r);
      w[3] = uint32_t(idx);
      w[4] = uint32_t(e.term);
      w[5] = e.crc;
      w[6] = uint32_t(uint64_t(e.value));
      w[7] = uint32_t(uint64_t(e.value) >> 32);
    }
    if (PAIRED) {
#pragma unroll
      for (uint32_t h = 0; h < 2; ++h) {
        const uint32_t src = h * 32u + (lane >> 1);
        const bool second = lane & 1u;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t a = __shfl(w[k], int(src)), b = __shfl(w[4 + k], int(src));
          v[k] = second ? b : a;
        }
        const uint32_t js = jb + src;
        if (js < wtot && woff + js < cap)
          reinterpret_cast<u4*>(out + (woff + js))[lane & 1u] = u4{v[0], v[1], v[2], v[3]};
      }
    } else if (mine) {
      u4* dst = reinterpret_cast<u4*>(out + (woff + j));
      dst[0] = u4{w[0], w[1], w[2], w[3]};
      dst[1] = u4{w[4], w[5], w[6], w[7]};
    }
  }
}

hipError_t launch_feed_count(int R, const DevPlanes& P, int raft, uint32_t mask, uint32_t nm, int32_t* cursors,
                             uint32_t* bsum, unsigned long long* tot, int mode, hipStream_t s) {
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(feed_count_kernel<RR>, grid_for(P.G), dim3(256), 0, s, P, raft, mask, nm,
                                        cursors, bsum, tot, mode));
  return hipGetLastError();
}
hipError_t launch_feed_scan(const uint32_t* bsum, uint64_t* boff, uint32_t nb, unsigned long long* tot,
                            unsigned long long* res, hipStream_t s) {
  hipLaunchKernelGGL(feed_scan_kernel, dim3(1), dim3(256), 0, s, bsum, boff, nb, tot, res);
  return hipGetLastError();
}
hipError_t launch_feed_emit(int R, const DevPlanes& P, int raft, uint32_t mask, uint32_t nm, int32_t* cursors,
                            const uint64_t* boff, uint64_t cap, void* out, int paired, hipStream_t s) {
  if (paired) {
    RAFT_DISPATCH_R(R, hipLaunchKernelGGL((feed_emit_kernel<RR, true>), grid_for(P.G), dim3(256), 0, s, P, raft, mask,
                                          nm, cursors, boff, cap, static_cast<FeedRec*>(out)));
  } else {
    RAFT_DISPATCH_R(R, hipLaunchKernelGGL((feed_emit_kernel<RR, false>), grid_for(P.G), dim3(256), 0, s, P, raft, mask,
                                          nm, cursors, boff, cap, static_cast<FeedRec*>(out)));
  }
  return hipGetLastError();
}

}  // namespace raftstep
