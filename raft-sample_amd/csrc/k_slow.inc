// k_slow.inc — general tick kernel over the worklist and the message-level
// handler kernel, instantiated for one semantics per translation unit
// (k_ref.hip / k_raft.hip) so the two compile in parallel.
#pragma once
#include "seg_tick.hpp"
#include "tick_common.hpp"

#ifndef RAFT_SLOW_ATTR
#define RAFT_SLOW_ATTR
#endif

namespace raftstep {

// General tick over the worklist: every deferred group is caught up, tick
// by tick in order, from the tick it was deferred at to `last_tick`, with
// the full semantics of run_tick() (elections, candidates, step-downs,
// faults, EXT drops); stats go to each tick's own record. The worklist is
// dense (the kernel is register-heavy, so every resident lane must have work).
// A group's scalar state is loaded once, kept in the lane's registers / LDS
// column across its catch-up ticks and stored once (the per-tick
// begin/load/store of the reference order would re-read and re-write every
// plane of a scattered group each tick). Row placement (which leader owns
// the coalesced MatchIndex planes) is settled once at the end; it is
// placement only, every access goes through `primary`.
// Stats: per-(tick, stat) LDS counters for the window [win_first,
// last_tick], flushed with one global atomic per non-zero counter per block
// (direct global atomics only when the window exceeds SLOW_WIN ticks).
constexpr int SLOW_WIN = 32;

template <int R, int SEM>
__global__ __launch_bounds__(256, 2) void tick_slow_kernel(DevPlanes P, Trace T0, int64_t first_tick, int64_t win_first,
                                                        int64_t last_tick, unsigned long long* stats,
                                                        const uint32_t* work, const int32_t* work_tick,
                                                        const uint32_t* work_count, uint32_t* next_count) {
  __shared__ int glds[group_lds_ints<R>() * 256];
  __shared__ unsigned long long hst[SLOW_WIN * NSTAT];
  const bool lds_stats = stats && last_tick - win_first < SLOW_WIN;
  for (int k = threadIdx.x; k < SLOW_WIN * NSTAT; k += 256) hst[k] = 0;
  __syncthreads();
  __shared__ uint32_t pre[NSHARD + 1];
  const uint32_t n = shard_prefix(work_count, pre);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t w = shard_locate(pre, P.scap, i);
    const uint32_t g = work[w];
    int64_t t = work_tick[w];
    // (a VX group's virtual suffix into the ring first: this kernel reads rings)
    if constexpr (SEM == SEM_RAFT) vx_materialize<R>(P, g, T0.entries_before(t), T0.entries, T0.period, T0.seed);
    sh_materialize<R>(P, g, T0.at_tick(t - 1).now);   // (and a group's shared entries, ROT_SH)
    Group<R, SEM> G;
    G.bind(glds);
    G.begin(P, T0.at_tick(t), g);
    if (G.fault) continue;      // frozen: nothing to catch up (the window tail clears DEFER)
    G.load(P, false);
    for (; t <= last_tick; ++t) {
      const Trace T = T0.at_tick(t);
      G.next_tick(T);
      run_tick<R, SEM>(G, P, T, T.client_entries());
      if (lds_stats && t >= win_first) {
        unsigned long long* h = hst + (t - win_first) * NSTAT;
#pragma unroll
        for (int s = 0; s < NSTAT; ++s)
          if (G.st[s]) atomicAdd(&h[s], (unsigned long long)G.st[s]);
      } else if (stats) {
        unsigned long long* rec = stats + size_t(t - first_tick) * STAT_TICK + (g % STAT_SLOTS) * NSTAT;
#pragma unroll
        for (int s = 0; s < NSTAT; ++s)
          if (G.st[s]) atomicAdd(&rec[s], (unsigned long long)G.st[s]);
      }
      if (!G.alive()) break;    // frozen from this tick on
    }
    G.store(P, uint32_t(T0.entries_before(last_tick + 1)));
  }
  if (lds_stats) {
    __syncthreads();
    const int64_t nt = last_tick - win_first + 1;
    for (int k = threadIdx.x; k < nt * NSTAT; k += 256) {
      const unsigned long long x = hst[k];
      if (x) {
        const int64_t tt = win_first + k / NSTAT;
        atomicAdd(&stats[size_t(tt - first_tick) * STAT_TICK + (blockIdx.x % STAT_SLOTS) * NSTAT + k % NSTAT], x);
      }
    }
  }
}

// The same catch-up over the worklist, replica-parallel (seg_tick.hpp): one
// 8-lane segment per deferred group, 32 groups per 256-lane block.
#ifndef RAFT_SEG_WAVES_PER_SIMD
#define RAFT_SEG_WAVES_PER_SIMD 4   // 128 VGPRs at R=7 with a few spills: measured faster than 3 (C4 8.7e9 vs 8.2e9)
#endif
template <int R, int SEM>
__global__ __launch_bounds__(256, RAFT_SEG_WAVES_PER_SIMD) void tick_seg_kernel(DevPlanes P, Trace T0, int64_t first_tick, int64_t win_first,
                                                       int64_t last_tick, unsigned long long* stats,
                                                       const uint32_t* work, const int32_t* work_tick,
                                                       const uint32_t* work_count, uint32_t* next_count) {
  __shared__ unsigned long long hst[SLOW_WIN * NSTAT];
  const bool lds_stats = stats && last_tick - win_first < SLOW_WIN;
  for (int k = threadIdx.x; k < SLOW_WIN * NSTAT; k += 256) hst[k] = 0;
  __syncthreads();
  __shared__ uint32_t pre[NSHARD + 1];
  const uint32_t n = shard_prefix(work_count, pre);
  constexpr uint32_t SPB = 256 / SEGW;   // segments per block
  for (uint32_t i = blockIdx.x * SPB + threadIdx.x / SEGW; i < n; i += gridDim.x * SPB) {
    const uint32_t w = shard_locate(pre, P.scap, i);
    const uint32_t g = work[w];
    int64_t t = work_tick[w];
    // (a VX group's virtual suffix into the ring first, by every lane of the
    // segment: the same values, and each lane then reads its own stores)
    if constexpr (SEM == SEM_RAFT) vx_materialize<R>(P, g, T0.entries_before(t), T0.entries, T0.period, T0.seed);
    sh_materialize<R>(P, g, T0.at_tick(t - 1).now);
    Seg<R, SEM> S;
    S.begin(P, T0.at_tick(t), g);
    if (S.fault) continue;   // frozen: nothing to catch up (the window tail clears DEFER)
    S.load(P);
    for (; t <= last_tick; ++t) {
      const Trace T = T0.at_tick(t);
      S.next_tick(T);
      S.run(P, T, T.client_entries());
      if (S.me == 0 && stats) {
        if (lds_stats && t >= win_first) {
          unsigned long long* h = hst + (t - win_first) * NSTAT;
#pragma unroll
          for (int s = 0; s < NSTAT; ++s)
            if (S.stat(s)) atomicAdd(&h[s], (unsigned long long)S.stat(s));
        } else {
          unsigned long long* rec = stats + size_t(t - first_tick) * STAT_TICK + (g % STAT_SLOTS) * NSTAT;
#pragma unroll
          for (int s = 0; s < NSTAT; ++s)
            if (S.stat(s)) atomicAdd(&rec[s], (unsigned long long)S.stat(s));
        }
      }
      if (!S.alive()) break;    // frozen from this tick on
    }
    S.store(P, uint32_t(T0.entries_before(last_tick + 1)));
  }
  if (lds_stats) {
    __syncthreads();
    const int64_t nt = last_tick - win_first + 1;
    for (int k = threadIdx.x; k < nt * NSTAT; k += 256) {
      const unsigned long long x = hst[k];
      if (x) {
        const int64_t tt = win_first + k / NSTAT;
        atomicAdd(&stats[size_t(tt - first_tick) * STAT_TICK + (blockIdx.x % STAT_SLOTS) * NSTAT + k % NSTAT], x);
      }
    }
  }
}

template <int R, int SEM>
__global__ __launch_bounds__(256) void ops_kernel(DevPlanes P, Trace T, const DevOp* ops, uint32_t n,
                                                  const int32_t* et, const int64_t* ev, const uint32_t* ec,
                                                  DevRes* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const DevOp op = ops[i];
  DevRes res{0, 0, 0, 0, 0};
  __shared__ int glds[group_lds_ints<R>() * 256];
  Group<R, SEM> G;
  G.bind(glds);
  G.begin(P, T, uint32_t(op.group));
  if (G.fault) {
    res.fault = G.fault;
    out[i] = res;
    return;
  }
  G.load(P, true);
  // the trace's EXT isolation windows at now_tick apply to node steps too
  // (messages to / from an isolated replica are dropped, as in the fused tick)
  if (T.iso_p) G.iso = tick_iso_mask<R>(G.key, T, G.giso, 0u, false);
  const int x = int(op.replica);
  const int ro = G.role(x);
  const TickSrc ring_only{P.log_term, P.log_value, P.log_crc, P.crc_tab, P.crc_on, uint32_t(R), G.g, P.KP, P.kmask, G.rot, G.rota, G.rotb, G.sb, G.sb2, 0, 1,
                          -1, 0, 0, 0, 0};
  auto make_src = [ring_only](int c) {
    TickSrc s = ring_only;
    s.leader = c;
    return s;
  };
  switch (op.kind) {
    case OP_AE: {
      AEReq q{op.term, op.prev_idx, op.prev_term, op.lc, int(op.n), 0};
      HostSrc src{et, ev, ec, op.off, op.voff, op.skip, 0};
      with_replica<R>(x, [&](auto PI) {
        constexpr int p = decltype(PI)::value;
        AEResp a;
        if constexpr (SEM == SEM_RAFT) a = G.template r_deliver_ae<p>(P, T, q, src);
        else a = G.template deliver_ae<p>(P, T, q, src);
        res.term = a.term; res.ok = a.ok; res.value = a.match;
      });
      break;
    }
    case OP_VR: {
      with_replica<R>(x, [&](auto PI) {
        constexpr int p = decltype(PI)::value;
        int rt;
        int gr;
        // RAFT: CandidateId = arg, LastLogIndex = prev_idx, LastLogTerm = prev_term
        if constexpr (SEM == SEM_RAFT) gr = G.template r_deliver_vr<p>(P, T, op.term, int(op.arg), op.prev_idx, op.prev_term, &rt);
        else gr = G.template deliver_vr<p>(T, op.term, &rt);
        res.term = rt; res.ok = gr; res.value = gr;
      });
      break;
    }
    case OP_CLIENT_APPEND:
      if (ro != ROLE_L) { res.status = -22; break; }
      G.client_append_value(P, x, op.arg);
      res.value = sel(G.last, x);
      break;
    case OP_LEADER_ROUND:
      if (ro != ROLE_L) { res.status = -22; break; }
      if constexpr (SEM == SEM_RAFT) G.r_leader_round(P, T, x, make_src);
      else G.leader_round(P, T, x, make_src);
      res.value = sel(G.commit, x);
      break;
    case OP_CANDIDATE_ROUND:
      if (ro != ROLE_C) { res.status = -22; break; }
      if constexpr (SEM == SEM_RAFT) res.value = G.r_candidate_round(P, T, x);
      else res.value = G.candidate_round(P, T, x);
      break;
    case OP_TIMEOUT:
      if (ro == ROLE_L) { res.status = -22; break; }
      if constexpr (SEM == SEM_RAFT) G.r_timeout_fire(T, x);
      else G.timeout_fire(T, x);
      res.value = sel(G.term, x);
      break;
    case OP_LEADER_COMMIT: {
      if (ro != ROLE_L) { res.status = -22; break; }
      int m[R];
      G.load_match(P, x, m);
      const int lc = sel(G.commit, x);
      int nc;
      if constexpr (SEM == SEM_RAFT) nc = G.r_commit_rule(P, m, x, lc);
      else nc = G.commit_rule(m, x, lc);
      if (nc != lc) { put(G.commit, x, nc); G.d_commit |= 1u << x; }
      res.value = nc;
      break;
    }
    default:
      res.status = -22;
  }
  G.store(P, uint32_t(T.entries_before(T.tick + 1)));
  res.fault = G.fault;
  if (G.fault) res.ok = 0;
  out[i] = res;
}

// raft_propose: one lane per distinct group of the batch. Lane i owns the
// list positions perm[seg[i] .. seg[i + 1]) (the host's plan, propose_plan.hpp:
// all of one group, in list order) and runs each proposal's LogReq
// (main.go:327-329) on every replica whose State is Leader, in ascending id,
// through client_append_value: what OP_CLIENT_APPEND does to one replica. The
// group is loaded once and stored once; a proposal sees the state the one
// before it left, a fault (F_OVERFLOW at LastApplied 2^31-1) included. Each
// 32-B raft_ticket goes to its own list position as two 16-B stores.
template <int R, int SEM>
__global__ __launch_bounds__(256) void propose_kernel(DevPlanes P, Trace T, const DevProposal* props, const uint32_t* perm,
                                                      const uint32_t* seg, uint32_t nseg, uint4* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nseg) return;
  const uint32_t b = seg[i], e = seg[i + 1];
  const uint32_t g = uint32_t(props[perm[b]].group);
  const uint64_t gid = P.gbase + g;
  __shared__ int glds[group_lds_ints<R>() * 256];
  Group<R, SEM> G;
  G.bind(glds);
  G.begin(P, T, g);
  const bool loaded = !G.fault;
  if (loaded) G.load(P, false);
  for (uint32_t j = b; j < e; ++j) {
    const uint32_t pos = perm[j];
    const int64_t v = props[pos].value;
    uint32_t leaders = 0, leader = 0xFFu;
    int index = 0, term = 0;
    if (!G.fault) {
#pragma unroll 1
      for (int r = 0; r < R; ++r) {
        if (G.role(r) != ROLE_L) continue;
        G.client_append_value(P, r, v);
        if (G.fault) break;   // (frozen at this append: later leaders append nothing)
        if (!leaders) {
          leader = uint32_t(r);
          index = sel(G.last, r);
          term = sel(G.term, r);
        }
        leaders |= 1u << r;
      }
    }
    // RAFT_PROPOSE_ACCEPTED = 1, _NO_LEADER = 2, _FROZEN = 3
    const uint32_t status = leaders ? 1u : (G.fault ? 3u : 2u);
    const uint32_t w = status | (leader << 8) | (leaders << 16) | (uint32_t(G.fault) << 24);
    out[size_t(pos) * 2u] = uint4{uint32_t(gid), uint32_t(gid >> 32), uint32_t(uint64_t(v)), uint32_t(uint64_t(v) >> 32)};
    out[size_t(pos) * 2u + 1u] = uint4{g, uint32_t(index), uint32_t(term), w};
  }
  if (loaded) G.store(P, uint32_t(T.entries_before(T.tick + 1)));
}

// One resident wave of blocks (resident_blocks, tick_common.hpp) grid-striding
// over the worklist: an empty worklist costs one short wave of blocks, a long
// one has no partial block-round tail.
template <int R, int SEM>
static void launch_slow_t(const DevPlanes& P, const Trace& T0, int64_t first_tick, int64_t win_first,
                          int64_t last_tick, unsigned long long* stats, const uint32_t* work, const int32_t* work_tick,
                          const uint32_t* work_count, uint32_t* next_count, int lane_per_group, hipStream_t s) {
  if (lane_per_group) {   // one lane per group (Group, raft_device.hpp)
    const unsigned blocks = unsigned(std::min<uint64_t>((P.G + 255) / 256, resident_blocks(tick_slow_kernel<R, SEM>)));
    hipLaunchKernelGGL((tick_slow_kernel<R, SEM>), dim3(blocks), dim3(256), 0, s, P, T0, first_tick, win_first,
                       last_tick, stats, work, work_tick, work_count, next_count);
  } else {                // one 8-lane segment per group (Seg, seg_tick.hpp)
    const unsigned blocks =
        unsigned(std::min<uint64_t>((P.G + 255 / SEGW) / (256 / SEGW), resident_blocks(tick_seg_kernel<R, SEM>)));
    hipLaunchKernelGGL((tick_seg_kernel<R, SEM>), dim3(blocks), dim3(256), 0, s, P, T0, first_tick, win_first,
                       last_tick, stats, work, work_tick, work_count, next_count);
  }
}

template <int SEM>
hipError_t launch_tick_slow_sem(int R, const DevPlanes& P, const Trace& T0, int64_t first_tick, int64_t win_first, int64_t last_tick,
                                unsigned long long* stats, const uint32_t* work, const int32_t* work_tick,
                                const uint32_t* work_count, uint32_t* next_count, int lane_per_group, hipStream_t s) {
  RAFT_DISPATCH_R(R, (launch_slow_t<RR, SEM>(P, T0, first_tick, win_first, last_tick, stats, work, work_tick,
                                               work_count, next_count, lane_per_group, s)));
  return hipGetLastError();
}
template <int SEM>
hipError_t launch_ops_sem(int R, const DevPlanes& P, const Trace& T, const DevOp* ops, uint32_t n, const int32_t* et,
                          const int64_t* ev, const uint32_t* ec, DevRes* out, hipStream_t s) {
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL((ops_kernel<RR, SEM>), grid_for(n), dim3(256), 0, s, P, T, ops, n, et, ev,
                                        ec, out));
  return hipGetLastError();
}
template <int SEM>
hipError_t launch_propose_sem(int R, const DevPlanes& P, const Trace& T, const DevProposal* props, const uint32_t* perm,
                              const uint32_t* seg, uint32_t nseg, void* out, hipStream_t s) {
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL((propose_kernel<RR, SEM>), grid_for(nseg), dim3(256), 0, s, P, T, props, perm,
                                        seg, nseg, static_cast<uint4*>(out)));
  return hipGetLastError();
}

}  // namespace raftstep
