// k_audit.hip — the group audit (raft_group_audit): six safety invariants per
// group, evaluated on the canonical view (canon_view.hpp: every group word
// through CanonGroup, every entry through ring_form / canon_entry), violating
// groups out as dense records in ascending group order. Read-only but for the
// audit's own per-group scratch record; no block waits for another.
//   audit_scalar_kernel<R>  one lane per group from block first / 256 on:
//        TWO_LEADERS and COMMIT_BEYOND_LOG from the record words, and the
//        group's scratch record (AuditRec: violated mask, witness, fault);
//   audit_log_kernel<R>     one wave per group of [first, G), only when a log
//        check is asked for: the lanes take 64 consecutive log indices, each
//        lane loads its index's entry of every replica once, and LOG_MATCHING,
//        COMMIT_DIVERGED, TERM_ORDER and STAMP all come from those registers
//        (per pair two ballots: entries unequal, terms equal); what is the
//        same in all 64 lanes (a wave has one group) is read once per wave
//        and kept in scalar registers; lane 0 merges the result into the
//        scratch record;
//   audit_count_kernel      per block its hits (bsum) and, per check bit, the
//        groups violating it (popcounts of ballots, one integer atomicAdd per
//        block and bit: order-independent, so deterministic);
//   feed_scan_kernel        (k_feed.hip) the exclusive scan of the block sums;
//   audit_emit_kernel       hits [0, cap) as consecutive 24-B records, the lane
//        writing the last one stores the id after it.
// The rules are include/raftstep.h's ("group audit"); tests/audit_model.py
// restates them in numpy. Indices reach 2^31-1: the chunk base and a lane's
// index are int64, nothing adds to an int32 index.
#include "canon_view.hpp"

namespace raftstep {

namespace {

enum : uint32_t {
  AUD_TWO_LEADERS = 1u, AUD_LOG_MATCHING = 2u, AUD_COMMIT_DIVERGED = 4u, AUD_TERM_ORDER = 8u, AUD_STAMP = 16u,
  AUD_COMMIT_BEYOND_LOG = 32u,
  AUD_PAIR = AUD_LOG_MATCHING | AUD_COMMIT_DIVERGED,
  AUD_LOG = AUD_PAIR | AUD_TERM_ORDER | AUD_STAMP
};

// The scratch record: w = violated | a << 8 | b << 16 | fault << 24, and the
// witness index of the lowest violated check.
struct __attribute__((aligned(8))) AuditRec {
  uint32_t w;
  int32_t index;
};
static_assert(sizeof(AuditRec) == 8, "AuditRec is 8 B");

__device__ __forceinline__ uint32_t rec_word(uint32_t violated, uint32_t a, uint32_t b, uint32_t fault) {
  return violated | (a << 8) | (b << 16) | (fault << 24);
}

constexpr int pairs_of(int R) { return R > 1 ? R * (R - 1) / 2 : 1; }
constexpr int pair_ix(int R, int a, int b) { return a * R - a * (a + 1) / 2 + (b - a - 1); }

}  // namespace

template <int R>
__global__ __launch_bounds__(256) void audit_scalar_kernel(DevPlanes P, uint32_t checks, uint32_t first, uint32_t b0,
                                                           AuditRec* rec) {
  const uint32_t g = (b0 + blockIdx.x) * 256u + threadIdx.x;
  if (g >= P.G || g < first) return;
  const CanonGroup<R> c(P, g);
  uint32_t viol = 0, wa = 0xFFu, wb = 0xFFu;
  int32_t widx = 0;
  if (checks & AUD_COMMIT_BEYOND_LOG) {
#pragma unroll 1
    for (int r = R - 1; r >= 0; --r) {
      const int cm = c.commit(P, r);
      if (cm > c.last(P, r)) {
        viol |= AUD_COMMIT_BEYOND_LOG;
        wa = uint32_t(r);
        widx = cm;
      }
    }
  }
  if (checks & AUD_TWO_LEADERS) {   // (the lower bit: its witness replaces the other)
    bool found = false;
#pragma unroll 1
    for (int a = 0; a < R - 1 && !found; ++a) {
      if (rs_role(uint32_t(at(P.rs, rix<R>(g, a)))) != ROLE_L) continue;
      const int ta = c.term(P, a);
#pragma unroll 1
      for (int b = a + 1; b < R && !found; ++b) {
        if (rs_role(uint32_t(at(P.rs, rix<R>(g, b)))) != ROLE_L || c.term(P, b) != ta) continue;
        found = true;
        viol |= AUD_TWO_LEADERS;
        wa = uint32_t(a);
        wb = uint32_t(b);
        widx = ta;
      }
    }
  }
  rec[g] = AuditRec{rec_word(viol, wa, wb, uint32_t(c.fault)), widx};
}

template <int R>
__global__ __launch_bounds__(256) void audit_log_kernel(DevPlanes P, int raft, uint32_t checks, uint32_t first,
                                                        AuditRec* rec) {
  constexpr int NP = pairs_of(R);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wi = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6);
  if (wi >= uint64_t(P.G - first)) return;   // (wave-uniform)
  const uint32_t g = first + uint32_t(wi);
  const CanonGroup<R> c(P, g);
  const RingForm rf = ring_form(P, g);
  const bool stamps = (checks & AUD_STAMP) && P.crc_on;
  const bool pairs = (checks & AUD_PAIR) && R > 1;
  const bool order = checks & AUD_TERM_ORDER;
  const int want = EW_TERM | ((pairs || stamps) ? EW_VALUE : 0) | (stamps ? EW_CRC : 0);
  const int K = int(P.K);
  int last[R], lo[R], commit[R], rterm[R];
  bool live_r[R];
  int64_t gh = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    // (one group per wave: the same in every lane, so kept in scalar registers)
    last[r] = __builtin_amdgcn_readfirstlane(c.last(P, r));
    const int top = max(__builtin_amdgcn_readfirstlane(c.hwm(P, r, raft, last[r])), last[r]);
    lo[r] = max(1, top - K + 1);
    live_r[r] = last[r] >= lo[r];
    commit[r] = __builtin_amdgcn_readfirstlane(c.commit(P, r));
    rterm[r] = __builtin_amdgcn_readfirstlane(c.term(P, r));
    if (live_r[r]) gh = max(gh, int64_t(last[r]));
  }
  // wave-uniform running results: 0 = none (indices are >= 1)
  int p_uneq[NP], p_eqt[NP];   // per pair: smallest unequal index, largest index with equal terms
  int o_desc[R], s_bad[R];     // per replica: smallest descending index, smallest index with a wrong stamp
  bool o_last[R];              // per replica: the last entry's term is above the replica's
  int carry[R];                // per replica: the term at the index before the chunk
#pragma unroll
  for (int p = 0; p < NP; ++p) p_uneq[p] = p_eqt[p] = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    o_desc[r] = s_bad[r] = carry[r] = 0;
    o_last[r] = false;
  }
  int64_t cb = 1;
  while (cb <= gh) {
    // the chunk starts at the smallest live index >= cb (the replica whose last is gh has one)
    int64_t m = gh;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (live_r[r] && int64_t(last[r]) >= cb) m = min(m, max(int64_t(lo[r]), cb));
    cb = m;
    const int64_t i = cb + lane;
    int32_t t[R];
    int64_t v[R];
    bool live[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      live[r] = live_r[r] && i >= int64_t(lo[r]) && i <= int64_t(last[r]);
      Entry e{0, 0, 0};
      if (live[r]) e = canon_entry<R>(P, rf, g, uint32_t(r), int(i), want);
      t[r] = e.term;
      v[r] = e.value;
      if (stamps) {
        const unsigned long long bad = __ballot(live[r] && crc_entry(P.crc_tab, e.term, e.value) != e.crc);
        if (bad && !s_bad[r]) s_bad[r] = int(cb + __ffsll(bad) - 1);
      }
      if (order) {
        // i > lo and live: i - 1 is live too, in the lane below or in the chunk before (then contiguous)
        int prev = __shfl_up(t[r], 1);
        if (lane == 0) prev = carry[r];
        const unsigned long long d = __ballot(live[r] && i > int64_t(lo[r]) && t[r] < prev);
        if (d && !o_desc[r]) o_desc[r] = int(cb + __ffsll(d) - 1);
        if (__ballot(live[r] && i == int64_t(last[r]) && t[r] > rterm[r])) o_last[r] = true;
        carry[r] = __builtin_amdgcn_readlane(t[r], 63);
      }
    }
    if (pairs) {
#pragma unroll
      for (int a = 0; a < R - 1; ++a)
#pragma unroll
        for (int b = a + 1; b < R; ++b) {
          const int p = pair_ix(R, a, b);
          const bool in = live[a] && live[b];
          const unsigned long long un = __ballot(in && (t[a] != t[b] || v[a] != v[b]));
          const unsigned long long eq = __ballot(in && t[a] == t[b]);
          if (un && !p_uneq[p]) p_uneq[p] = int(cb + __ffsll(un) - 1);
          if (eq) p_eqt[p] = int(cb + 63 - __clzll(eq));
        }
    }
    cb += 64;
  }
  if (lane != 0) return;
  // the lowest violated log check's witness: pairs and replicas in ascending order, the first found
  uint32_t viol = 0, wa = 0xFFu, wb = 0xFFu;
  int32_t widx = 0;
  if (stamps) {
#pragma unroll
    for (int r = R - 1; r >= 0; --r)
      if (s_bad[r]) {
        viol |= AUD_STAMP;
        wa = uint32_t(r);
        widx = s_bad[r];
      }
  }
  if (order) {
    bool any = false;
#pragma unroll
    for (int r = R - 1; r >= 0; --r)
      if (o_desc[r] || o_last[r]) {
        any = true;
        wa = uint32_t(r);
        widx = o_desc[r] ? o_desc[r] : last[r];
      }
    if (any) viol |= AUD_TERM_ORDER;
  }
  if (pairs) {
    for (int pass = 0; pass < 2; ++pass) {   // COMMIT_DIVERGED, then the lower bit LOG_MATCHING
      const uint32_t bit = pass ? AUD_LOG_MATCHING : AUD_COMMIT_DIVERGED;
      if (!(checks & bit)) continue;
      bool found = false;
#pragma unroll
      for (int a = 0; a < R - 1; ++a)
#pragma unroll
        for (int b = a + 1; b < R; ++b) {
          const int p = pair_ix(R, a, b);
          const int u = p_uneq[p];
          const bool bad = u && (pass ? (p_eqt[p] && u <= p_eqt[p]) : u <= min(commit[a], commit[b]));
          if (bad && !found) {
            found = true;
            viol |= bit;
            wa = uint32_t(a);
            wb = uint32_t(b);
            widx = u;
          }
        }
    }
  }
  if (!viol) return;
  AuditRec x = rec[g];
  const uint32_t old = x.w & 0xFFu;
  if (old & AUD_TWO_LEADERS) x.w |= viol;   // (the scalar pass's witness is the lowest check's)
  else {
    x.w = rec_word(old | viol, wa, wb, x.w >> 24);
    x.index = widx;
  }
  rec[g] = x;
}

// tot[8 + k] += groups of the block violating check bit k.
__global__ __launch_bounds__(256) void audit_count_kernel(const AuditRec* rec, uint32_t G, uint32_t first, uint32_t b0,
                                                          uint32_t* bsum, unsigned long long* tot) {
  __shared__ uint32_t s_n[4], s_k[4][6];
  const uint32_t g = (b0 + blockIdx.x) * 256u + threadIdx.x;
  const uint32_t viol = (g < G && g >= first) ? (rec[g].w & 0xFFu) : 0u;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t n = uint32_t(__popcll(__ballot(viol != 0u)));
  if (lane == 0) s_n[wave] = n;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const uint32_t nk = uint32_t(__popcll(__ballot((viol >> k) & 1u)));
    if (lane == 0) s_k[wave][k] = nk;
  }
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
  if (threadIdx.x < 6) {
    const uint32_t k = threadIdx.x;
    const uint32_t nk = s_k[0][k] + s_k[1][k] + s_k[2][k] + s_k[3][k];
    if (nk) atomicAdd(&tot[8 + k], (unsigned long long)nk);
  }
}

// cap >= 1 and at most the total: hit p of the ascending group order is
// written iff p < cap; the lane that writes hit cap - 1 stores its group's id
// + 1 to *next. A raft_audit_hit is three 8-B words.
__global__ __launch_bounds__(256) void audit_emit_kernel(const AuditRec* rec, uint32_t G, uint64_t gbase, uint32_t first,
                                                         uint32_t b0, const uint64_t* boff, uint64_t cap, uint32_t* out,
                                                         unsigned long long* next) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  __shared__ uint32_t s_w[4];
  const uint64_t base = boff[blockIdx.x];
  if (base >= cap) return;   // (the whole block: nothing of it is written)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t g = (b0 + blockIdx.x) * 256u + threadIdx.x;
  AuditRec x{0, 0};
  if (g < G && g >= first) x = rec[g];
  const uint32_t viol = x.w & 0xFFu;
  const bool hit = viol != 0u;
  const unsigned long long b = __ballot(hit);
  if (lane == 0) s_w[wave] = uint32_t(__popcll(b));
  __syncthreads();
  uint64_t pos = base + uint32_t(__popcll(b & ((1ull << lane) - 1ull)));
  for (uint32_t w = 0; w < wave; ++w) pos += s_w[w];
  if (!hit || pos >= cap) return;
  const uint64_t gid = gbase + g;
  // raft_audit_hit: group | local, violated, fault, a, b | index, check
  const uint32_t w3 = viol | ((x.w >> 24) << 8) | (((x.w >> 8) & 0xFFFFu) << 16);
  u2* o = reinterpret_cast<u2*>(out) + pos * 3u;
  o[0] = u2{uint32_t(gid), uint32_t(gid >> 32)};
  o[1] = u2{g, w3};
  o[2] = u2{uint32_t(x.index), viol & (0u - viol)};
  if (pos == cap - 1) *next = uint64_t(g) + 1u;
}

hipError_t launch_audit_scalar(int R, const DevPlanes& P, uint32_t checks, uint32_t first, void* rec, hipStream_t s) {
  const uint32_t b0 = first >> 8, nb = uint32_t((P.G + 255) / 256) - b0;
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(audit_scalar_kernel<RR>, dim3(nb), dim3(256), 0, s, P, checks, first, b0,
                                        static_cast<AuditRec*>(rec)));
  return hipGetLastError();
}
hipError_t launch_audit_log(int R, const DevPlanes& P, int raft, uint32_t checks, uint32_t first, void* rec,
                            hipStream_t s) {
  const uint32_t n = uint32_t(P.G) - first;
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(audit_log_kernel<RR>, dim3((n + 3u) / 4u), dim3(256), 0, s, P, raft, checks,
                                        first, static_cast<AuditRec*>(rec)));
  return hipGetLastError();
}
hipError_t launch_audit_count(const DevPlanes& P, uint32_t first, const void* rec, uint32_t* bsum,
                              unsigned long long* tot, hipStream_t s) {
  const uint32_t b0 = first >> 8, nb = uint32_t((P.G + 255) / 256) - b0;
  hipLaunchKernelGGL(audit_count_kernel, dim3(nb), dim3(256), 0, s, static_cast<const AuditRec*>(rec), uint32_t(P.G),
                     first, b0, bsum, tot);
  return hipGetLastError();
}
hipError_t launch_audit_emit(const DevPlanes& P, uint32_t first, const void* rec, const uint64_t* boff, uint64_t cap,
                             void* out, unsigned long long* next, hipStream_t s) {
  const uint32_t b0 = first >> 8, nb = uint32_t((P.G + 255) / 256) - b0;
  hipLaunchKernelGGL(audit_emit_kernel, dim3(nb), dim3(256), 0, s, static_cast<const AuditRec*>(rec), uint32_t(P.G),
                     uint64_t(P.gbase), first, b0, boff, cap, static_cast<uint32_t*>(out), next);
  return hipGetLastError();
}

}  // namespace raftstep
