// k_apply.hip — the applied state (raft_apply_*): one 32-B record per fed
// (group, replica) that says how far the replica has applied, an
// order-sensitive digest (the chain) of everything it applied and the plain
// sum of the values; every step folds the newly committed entries into the
// records and compares the replicas of a group wherever their applied prefixes
// meet (include/raftstep.h, "applied state"). No entry leaves the device.
//
//   apply_reset_kernel<R>  the records of listed groups (or of all) become the
//        FROM_START or the FROM_COMMIT state: raft_apply_open, and the reset
//        raft_restart_groups / raft_load_groups launch after their own writes;
//   apply_step_kernel<R>   one lane per group (consecutive lanes on consecutive
//        groups of a ring tile): derives (lo, hi] of every fed replica as the
//        feed does (feed_range.hpp), re-seeds the pairs whose entries left the
//        ring, then walks the group's replicas in lockstep by log index, the R
//        running chains in registers, folding entry i of every replica whose
//        range holds it and comparing the chains of the replicas that stand at
//        i; a changed record leaves as two 16-B stores. The five counters are
//        summed per wave and added with one atomic per wave and counter;
//   apply_publish_kernel   one wave behind the step: the totals to pinned host
//        memory, the accumulators zeroed (as feed_scan_kernel does for a poll);
//   apply_read_kernel      a gather of 32-B records by (list position, replica);
//   apply_count_kernel / apply_emit_kernel  raft_apply_scan: count, scan
//        (feed_scan_kernel, k_feed.hip), emit, as the directory and the audit.
#include "feed_range.hpp"

namespace raftstep {

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

// raft_apply_record; tail = gaps | div_peer << 16 | reserved << 24
struct __attribute__((aligned(16))) ApplyRec {
  int32_t applied, base;
  uint64_t chain;
  int64_t sum;
  int32_t div_index;
  uint32_t tail;
};
static_assert(sizeof(ApplyRec) == 32, "raft_apply_record is 32 B");
constexpr uint32_t TAIL_NO_PEER = 0xFFu << 16;

__device__ __forceinline__ ApplyRec rec_load(const ApplyRec* p) {
  const u4 a = reinterpret_cast<const u4*>(p)[0], b = reinterpret_cast<const u4*>(p)[1];
  ApplyRec x;
  x.applied = int32_t(a.x);
  x.base = int32_t(a.y);
  x.chain = uint64_t(a.z) | (uint64_t(a.w) << 32);
  x.sum = int64_t(uint64_t(b.x) | (uint64_t(b.y) << 32));
  x.div_index = int32_t(b.z);
  x.tail = b.w;
  return x;
}
__device__ __forceinline__ void rec_store(ApplyRec* p, const ApplyRec& x) {
  reinterpret_cast<u4*>(p)[0] = u4{uint32_t(x.applied), uint32_t(x.base), uint32_t(x.chain), uint32_t(x.chain >> 32)};
  reinterpret_cast<u4*>(p)[1] =
      u4{uint32_t(uint64_t(x.sum)), uint32_t(uint64_t(x.sum) >> 32), uint32_t(x.div_index), x.tail};
}

// The chain (all 64-bit, wrapping; sm64: the digest's splitmix64 step)
__device__ __forceinline__ uint64_t apply_seed(uint64_t gid, int base) {
  return sm64(sm64(gid) ^ uint64_t(uint32_t(base)));
}
__device__ __forceinline__ uint64_t apply_fold(uint64_t chain, int i, int32_t term, int64_t value) {
  return sm64(sm64(chain ^ ((uint64_t(uint32_t(term)) << 32) | uint64_t(uint32_t(i)))) ^ uint64_t(value));
}

__device__ __forceinline__ unsigned long long apply_wave_sum(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

}  // namespace

// Listed group i < n (ids null: g = i): every fed record becomes applied =
// base = 0 (from_commit: min(CommitIndex, LastApplied) of the canonical view),
// chain = seed(gid, base), no divergence, no gap.
template <int R>
__global__ __launch_bounds__(256) void apply_reset_kernel(DevPlanes P, int from_commit, const uint32_t* ids, uint32_t n,
                                                          uint32_t mask, uint32_t nm, ApplyRec* rec) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = ids ? ids[i] : i;
  const CanonGroup<R> cg(P, g);
  const uint64_t gid = P.gbase + g;
  uint32_t k = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!((mask >> r) & 1u)) continue;
    const int b = from_commit ? min(cg.commit(P, r), cg.last(P, r)) : 0;
    rec_store(rec + (size_t(g) * nm + k), ApplyRec{b, b, apply_seed(gid, b), 0, 0, TAIL_NO_PEER});
    ++k;
  }
}

// tot: the step's accumulators folded, lost, stalled, gapped, diverged (zero
// between steps: apply_publish_kernel re-zeroes them).
template <int R>
__global__ __launch_bounds__(256) void apply_step_kernel(DevPlanes P, int raft, uint32_t mask, uint32_t nm, ApplyRec* rec,
                                                         unsigned long long* tot) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  unsigned long long folded = 0, lost = 0;
  uint32_t stalled = 0, gapped = 0, diverged = 0;
  if (g < P.G) {
    const CanonGroup<R> cg(P, g);
    const uint64_t gid = P.gbase + g;
    ApplyRec x[R];
    int lo[R], hi[R];         // the trajectory of replica r holds the indices lo .. hi (unfed: none, lo > hi)
    uint32_t changed = 0;     // bit r: the record has to be stored
    uint32_t todo = 0;
    ApplyRec* const grec = rec + size_t(g) * nm;
    {
      uint32_t k = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        lo[r] = 1;
        hi[r] = 0;
        x[r] = ApplyRec{0, 0, 0, 0, 0, 0};
        if (!((mask >> r) & 1u)) continue;
        x[r] = rec_load(grec + k);
        ++k;
        const int l = cg.last(P, r);
        const int cm = cg.commit(P, r);
        const int hwm = cg.hwm(P, r, raft, l);
        const int c = x[r].applied;
        int n;
        if (!feed_pair_range(c, cm, l, hwm, int(P.K), &lo[r], &n)) {
          ++stalled;          // left alone: its trajectory is {c: chain}
          hi[r] = c;
          continue;
        }
        hi[r] = lo[r] + n;
        if (lo[r] > c) {      // the entries c+1 .. lo have left the ring: the chain starts again at lo
          lost += uint32_t(lo[r] - c);
          ++gapped;
          const uint32_t gp = x[r].tail & 0xFFFFu;
          x[r].tail = (x[r].tail & ~0xFFFFu) | (gp < 0xFFFFu ? gp + 1u : gp);
          x[r].base = lo[r];
          x[r].chain = apply_seed(gid, lo[r]);
          x[r].sum = 0;
          changed |= 1u << r;
        }
        if (n) changed |= 1u << r;
        x[r].applied = hi[r];
        todo += uint32_t(n);
      }
    }
    folded = todo;
    RingForm rf{0, 0, 0, 0, 0, 0, false};
    if (todo) rf = ring_form(P, g);
    // The walk: index i ascends over every index some trajectory holds (at most
    // the sum of their lengths, counted by the trajectories themselves: no
    // i <= hi loop, hi may be 2^31-1). At i every replica whose range (lo, hi]
    // holds i folds its entry i, then the replicas standing at i are compared.
    bool any = false, marked = false;
    int i = 0;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (lo[r] <= hi[r] && (!any || lo[r] < i)) {
        i = lo[r];
        any = true;
      }
    while (any) {
      uint32_t here = 0;      // bit r: replica r's trajectory holds i
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!(lo[r] <= i && i <= hi[r])) continue;
        here |= 1u << r;
        if (lo[r] < i) {
          const Entry e = canon_entry<R>(P, rf, g, uint32_t(r), i, EW_TERM | EW_VALUE);
          x[r].chain = apply_fold(x[r].chain, i, e.term, e.value);
          x[r].sum = int64_t(uint64_t(x[r].sum) + uint64_t(e.value));
        }
      }
      // (the common case first: everyone here has the same base and chain)
      bool same = true;
      {
        bool got = false;
        int b0 = 0;
        uint64_t c0 = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (!((here >> r) & 1u)) continue;
          if (!got) {
            got = true;
            b0 = x[r].base;
            c0 = x[r].chain;
          } else if (x[r].base != b0 || x[r].chain != c0) {
            same = false;
          }
        }
      }
      if (!same) {
#pragma unroll
        for (int a = 0; a < R; ++a) {
          if (!((here >> a) & 1u) || x[a].div_index != 0) continue;
          int peer = -1;
#pragma unroll
          for (int b = R - 1; b >= 0; --b)
            if (b != a && ((here >> b) & 1u) && x[b].base == x[a].base && x[b].chain != x[a].chain) peer = b;
          if (peer < 0) continue;
          // (i >= 1: equal bases have equal chains at the base, and no base is negative)
          x[a].div_index = i;
          x[a].tail = (x[a].tail & 0xFF00FFFFu) | (uint32_t(peer) << 16);
          changed |= 1u << a;
          marked = true;
        }
      }
      bool mid = false, jump = false;
      int nxt = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (lo[r] > hi[r]) continue;
        if (lo[r] <= i && i < hi[r]) mid = true;
        else if (lo[r] > i && (!jump || lo[r] < nxt)) {
          nxt = lo[r];
          jump = true;
        }
      }
      if (mid) ++i;           // (i < some hi <= 2^31-1)
      else if (jump) i = nxt;
      else any = false;
    }
    diverged = marked ? 1u : 0u;
    {
      uint32_t k = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!((mask >> r) & 1u)) continue;
        if ((changed >> r) & 1u) rec_store(grec + k, x[r]);
        ++k;
      }
    }
  }
  const unsigned long long wf = apply_wave_sum(folded), wl = apply_wave_sum(lost), ws = apply_wave_sum(stalled),
                           wg = apply_wave_sum(gapped), wd = apply_wave_sum(diverged);
  if ((threadIdx.x & 63u) == 0) {
    if (wf) atomicAdd(&tot[0], wf);
    if (wl) atomicAdd(&tot[1], wl);
    if (ws) atomicAdd(&tot[2], ws);
    if (wg) atomicAdd(&tot[3], wg);
    if (wd) atomicAdd(&tot[4], wd);
  }
}

// The step's totals to `res` (pinned, coherent host memory the engine reads
// after its synchronise), the accumulators zeroed for the next step: one wave,
// launched behind the step kernel as feed_scan_kernel is behind the count pass.
__global__ __launch_bounds__(64) void apply_publish_kernel(unsigned long long* tot, unsigned long long* res) {
  if (threadIdx.x < 5) {
    res[threadIdx.x] = tot[threadIdx.x];
    tot[threadIdx.x] = 0ull;
  }
  __threadfence_system();
}

// out[(i R + r)] = the record of replica r of listed group i < n (ids null: g
// = first + i); a replica outside the mask reads applied = -1 and zeroes.
__global__ __launch_bounds__(256) void apply_read_kernel(const ApplyRec* rec, const uint32_t* ids, uint32_t first,
                                                         uint32_t n, uint32_t R, uint32_t mask, uint32_t nm, u4* out) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n * R) return;
  const uint32_t i = j / R, r = j - i * R;
  const uint32_t g = ids ? ids[i] : first + i;
  u4 a{0xFFFFFFFFu, 0, 0, 0}, b{0, 0, 0, 0};
  if ((mask >> r) & 1u) {
    const u4* src = reinterpret_cast<const u4*>(rec + (size_t(g) * nm + uint32_t(__popc(mask & ((1u << r) - 1u)))));
    a = src[0];
    b = src[1];
  }
  out[size_t(j) * 2] = a;
  out[size_t(j) * 2 + 1] = b;
}

namespace {

// What raft_apply_scan says of group g: flags (RAFT_APPLY_DIVERGED |
// RAFT_APPLY_GAPPED, whatever was asked for), and with `w` the witness words
// a | b << 8, index and the gaps summed over the fed replicas.
struct ApplyWitness {
  uint32_t ab;
  int32_t index;
  uint32_t gaps;
};
__device__ __forceinline__ uint32_t apply_flags(const ApplyRec* rec, uint32_t g, uint32_t R, uint32_t mask, uint32_t nm,
                                                ApplyWitness* w) {
  uint32_t flags = 0, k = 0, gaps = 0, ab = 0;
  int32_t index = 0;
  for (uint32_t r = 0; r < R; ++r) {
    if (!((mask >> r) & 1u)) continue;
    const ApplyRec* p = rec + (size_t(g) * nm + k);
    ++k;
    const u2 t = reinterpret_cast<const u2*>(p)[3];   // div_index, tail
    const uint32_t gp = t.y & 0xFFFFu;
    gaps += gp;
    if (t.x != 0u && !(flags & 1u)) {                 // the lowest diverged replica: it is the witness
      flags |= 1u;
      ab = r | (((t.y >> 16) & 0xFFu) << 8);
      index = int32_t(t.x);
    }
    if (gp != 0u && !(flags & 2u)) {
      flags |= 2u;
      if (!(flags & 1u)) {
        ab = r | (0xFFu << 8);
        index = w ? p->base : 0;
      }
    }
  }
  if (w) *w = ApplyWitness{ab, index, gaps};
  return flags;
}

}  // namespace

__global__ __launch_bounds__(256) void apply_count_kernel(const ApplyRec* rec, uint32_t G, uint32_t R, uint32_t mask,
                                                          uint32_t nm, uint32_t select, uint32_t first, uint32_t b0,
                                                          uint32_t* bsum) {
  __shared__ uint32_t s_w[4];
  const uint32_t g = (b0 + blockIdx.x) * 256u + threadIdx.x;
  bool hit = false;
  if (g < G && g >= first) hit = (apply_flags(rec, g, R, mask, nm, nullptr) & select) != 0u;
  const uint32_t n = uint32_t(__popcll(__ballot(hit)));
  if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// cap >= 1 and at most the total: hit p of the ascending group order is
// written iff p < cap; the lane that writes hit cap - 1 stores its group's id
// + 1 to *next. A raft_apply_hit is three 8-B words. gmeta: for the fault code.
__global__ __launch_bounds__(256) void apply_emit_kernel(DevPlanes P, const ApplyRec* rec, uint32_t R, uint32_t mask,
                                                         uint32_t nm, uint32_t select, uint32_t first, uint32_t b0,
                                                         const uint64_t* boff, uint64_t cap, uint32_t* out,
                                                         unsigned long long* next) {
  __shared__ uint32_t s_w[4];
  const uint64_t base = boff[blockIdx.x];
  if (base >= cap) return;   // (the whole block: nothing of it is written)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t g = (b0 + blockIdx.x) * 256u + threadIdx.x;
  ApplyWitness w{0, 0, 0};
  uint32_t flags = 0;
  if (g < P.G && g >= first) flags = apply_flags(rec, g, R, mask, nm, &w);
  const bool hit = (flags & select) != 0u;
  const unsigned long long b = __ballot(hit);
  if (lane == 0) s_w[wave] = uint32_t(__popcll(b));
  __syncthreads();
  uint64_t pos = base + uint32_t(__popcll(b & ((1ull << lane) - 1ull)));
  for (uint32_t k = 0; k < wave; ++k) pos += s_w[k];
  if (!hit || pos >= cap) return;
  const uint64_t gid = P.gbase + g;
  const uint32_t fault = (uint32_t(at(P.gmeta, g)) >> 4) & 7u;
  // raft_apply_hit: group | local, a, b, flags, fault | index, gaps
  u2* o = reinterpret_cast<u2*>(out) + pos * 3u;
  o[0] = u2{uint32_t(gid), uint32_t(gid >> 32)};
  o[1] = u2{g, w.ab | (flags << 16) | (fault << 24)};
  o[2] = u2{uint32_t(w.index), w.gaps};
  if (pos == cap - 1) *next = uint64_t(g) + 1u;
}

hipError_t launch_apply_reset(int R, const DevPlanes& P, int from_commit, const uint32_t* ids, uint32_t n, uint32_t mask,
                              uint32_t nm, void* rec, hipStream_t s) {
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(apply_reset_kernel<RR>, grid_for(n), dim3(256), 0, s, P, from_commit, ids, n, mask,
                                        nm, static_cast<ApplyRec*>(rec)));
  return hipGetLastError();
}
hipError_t launch_apply_step(int R, const DevPlanes& P, int raft, uint32_t mask, uint32_t nm, void* rec,
                             unsigned long long* tot, unsigned long long* res, hipStream_t s) {
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(apply_step_kernel<RR>, grid_for(P.G), dim3(256), 0, s, P, raft, mask, nm,
                                        static_cast<ApplyRec*>(rec), tot));
  if (hipError_t rc = hipGetLastError()) return rc;
  hipLaunchKernelGGL(apply_publish_kernel, dim3(1), dim3(64), 0, s, tot, res);
  return hipGetLastError();
}
hipError_t launch_apply_read(int R, const void* rec, const uint32_t* ids, uint32_t first, uint32_t n, uint32_t mask,
                             uint32_t nm, void* out, hipStream_t s) {
  hipLaunchKernelGGL(apply_read_kernel, grid_for(uint64_t(n) * uint32_t(R)), dim3(256), 0, s,
                     static_cast<const ApplyRec*>(rec), ids, first, n, uint32_t(R), mask, nm, static_cast<u4*>(out));
  return hipGetLastError();
}
hipError_t launch_apply_count(int R, const DevPlanes& P, const void* rec, uint32_t mask, uint32_t nm, uint32_t select,
                              uint32_t first, uint32_t* bsum, hipStream_t s) {
  const uint32_t b0 = first >> 8, nb = uint32_t((P.G + 255) / 256) - b0;
  hipLaunchKernelGGL(apply_count_kernel, dim3(nb), dim3(256), 0, s, static_cast<const ApplyRec*>(rec), uint32_t(P.G),
                     uint32_t(R), mask, nm, select, first, b0, bsum);
  return hipGetLastError();
}
hipError_t launch_apply_emit(int R, const DevPlanes& P, const void* rec, uint32_t mask, uint32_t nm, uint32_t select,
                             uint32_t first, const uint64_t* boff, uint64_t cap, void* out, unsigned long long* next,
                             hipStream_t s) {
  const uint32_t b0 = first >> 8, nb = uint32_t((P.G + 255) / 256) - b0;
  hipLaunchKernelGGL(apply_emit_kernel, dim3(nb), dim3(256), 0, s, P, static_cast<const ApplyRec*>(rec), uint32_t(R), mask,
                     nm, select, first, b0, boff, cap, static_cast<uint32_t*>(out), next);
  return hipGetLastError();
}

}  // namespace raftstep
