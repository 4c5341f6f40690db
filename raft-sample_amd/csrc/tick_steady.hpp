// tick_steady.hpp — the steady form of the one-tick lean kernel (k_fast.hip
// tick_lean_kernel<R, CRC, SEM, true, SH>).
//
// A list-skipping call (engine.cpp, steady-state list skip) has proven every
// live group compressed and takeable with no isolation and no corruption
// configured; when the engine can also prove every live group in the global
// ring phase (raft_engine::phase_ok), the lean kernel's normal class, in
// phase, is the whole tick of every group. This body is that class alone,
// with the one-tick form's stores: a lane that fits leaves memory bit for
// bit as the general body does. It has no isolation windows, no LXS / SXS /
// HWX classes, no drifted rings or segment switches, no corruption draw, no
// pipelined-tick marks, no diagnostics and no block-wide list prefix, and it
// reads its launch constants from two small argument records instead of
// DevPlanes / Trace (a scalar prologue of a few loads).
// A lane that does not fit (which the proofs exclude) leaves its group alone
// and appends its id to the block's list shard, one atomic per such lane, as
// tick_fused_kernel does: the end-of-call check turns it into RAFT_EINTERNAL.
#pragma once
#include "tick_common.hpp"

namespace raftstep {

// What the steady body reads of DevPlanes (constant between launches but for
// dbg_pass / rec_nt, which the host sets between calls).
struct SteadyPlanes {
  const uint16_t* gmeta;
  SsRec* gss;
  uint16_t* grot;
  int32_t* hb;
  Strided<int32_t, 16> gshf;
  int32_t* term;       // the entries' planes: the shared ring (SH, one row per slot: sh_cs = 0) or the replica rings
  int64_t* value;
  uint32_t* crc;
  const uint32_t* crc_tab;
  uint64_t gbase;
  uint64_t cv_stride;  // staged client values: between a group's entries e and e+1 (0: the trace RNG)
  uint32_t G, K, KP, kmask;
  uint32_t dbg_pass, rec_nt;
  uint32_t scap, shard_sb;
};
// ... and of Trace, with the tick's client entries, ring phase and staged
// values' row worked out by the host.
struct SteadyTick {
  uint64_t seed;
  int64_t tick;
  const int64_t* cv;   // staged client values: entry 0 of group 0 at this tick (null: the trace RNG)
  int32_t now;
  uint32_t n;          // this tick's client entries
  uint32_t ph;         // global ring phase of this tick's first entry
};

inline SteadyPlanes steady_planes(const DevPlanes& P) {
  SteadyPlanes S{};
  S.gmeta = P.gmeta; S.gss = P.gss; S.grot = P.grot; S.hb = P.hb; S.gshf = P.gshf;
  S.term = P.sh ? P.sh_term : P.log_term;
  S.value = P.sh ? P.sh_value : P.log_value;
  S.crc = P.sh ? P.sh_crc : P.log_crc;
  S.crc_tab = P.crc_tab;
  S.gbase = P.gbase;
  S.cv_stride = P.cv ? P.cv_stride : 0u;
  S.G = uint32_t(P.G); S.K = P.K; S.KP = P.KP; S.kmask = P.kmask;
  S.dbg_pass = P.dbg_pass; S.rec_nt = P.rec_nt;
  S.scap = P.scap; S.shard_sb = P.shard_sb;
  return S;
}
inline SteadyTick steady_tick_args(const DevPlanes& P, const Trace& T) {
  SteadyTick S{};
  S.seed = T.seed; S.tick = T.tick; S.now = T.now;
  S.n = T.n_tick;
  S.ph = uint32_t(T.eb_tick) & P.kmask;
  S.cv = P.cv ? P.cv + uint64_t(T.tick - P.cv_t0) * P.cv_tstride : nullptr;
  return S;
}

template <int R, bool CRC, bool RAFT, bool SH>
__device__ __forceinline__ void steady_tick(const SteadyPlanes& P, const SteadyTick& T, unsigned long long* stats,
                                            uint32_t* list, uint32_t* count, uint32_t gofs) {
  const uint32_t gblk = (gofs >> 8) + blockIdx.x;   // this block's 256 groups (gofs: tick_lean_kernel)
  const uint32_t g = gblk * 256u + threadIdx.x;
  __shared__ uint32_t tab[CRC ? 2048 : 1];
  if constexpr (CRC) {   // (stage_crc_tab)
    const uint4* src = reinterpret_cast<const uint4*>(P.crc_tab);
    uint4* dst = reinterpret_cast<uint4*>(tab);
    for (uint32_t i = threadIdx.x; i < 512u; i += 256u) dst[i] = src[i];
    __syncthreads();
  }
  const int n = int(T.n), ph = int(T.ph);
  bool fit = false, pass = false;
  int committed = 0, term = 0;
  uint64_t vb = 0;
  int64_t cv0 = 0;   // staged client values: the group's entry 0 of this tick
  if (g < P.G) {
    // one round trip: gmeta, the record, the ring rotation, the staged value
    const int meta = at(P.gmeta, g);
    const SsRec s = P.gss[g];
    const int rot = at(P.grot, g);
    if (T.cv && n) cv0 = __builtin_nontemporal_load(T.cv + g);
    const uint64_t key = group_key(T.seed, P.gbase + g);
    const int c = meta & 0xF, L = s.last;
    const bool skip = (meta & (M_DEFER | (7 << 4))) != 0;   // pending catch-up / frozen group
    const bool shm = (uint32_t(rot) & ROT_SH) != 0u;
    // (bitwise: one straight line of compares instead of a branch per term)
    // SSYNC and neither LXS nor SXS (uses_glx: SXS is SSYNC with ONESTALE) nor, RAFT, HWX
    constexpr int other = M_LXS | M_ONESTALE | (RAFT ? M_HWX : 0);
    const int ln = int(uint32_t(L) + uint32_t(n));   // (L + n; used only where it does not overflow)
    fit = !skip & ((meta & (M_SSYNC | other)) == M_SSYNC) & (c < R) & (g != P.dbg_pass) &
          (L > 0) & (L <= I32MAX - n) & (n < int(P.K)) & (s.cl <= ln) &
          ((n == 0) | (((uint32_t(L) + uint32_t(rot)) & P.kmask) == uint32_t(ph)));
    pass = !skip & !fit;
    if (fit) {
      // the closed form of tick_lean_kernel's normal class
      const int nl = L + n;
      const int cl2 = (RAFT ? nl > s.cl : (2 * (R - 1) > R && nl > s.cl)) ? nl : s.cl;
      const int cf2 = s.cl > s.cf ? s.cl : s.cf;
      const bool shw = SH && n > 0;                // this tick's entries go to the shared ring
      const bool hbw = !(shw || shm);              // (SH: a group in shared form implies its heartbeat time)
      if (P.rec_nt) {
        typedef int32_t i4 __attribute__((ext_vector_type(4)));
        if (nl != L || cl2 != s.cl || cf2 != s.cf)
          __builtin_nontemporal_store(i4{nl, s.term, cl2, cf2}, reinterpret_cast<i4*>(&P.gss[g]));
        if (hbw) __builtin_nontemporal_store(int32_t(T.now), &P.hb[g]);
      } else {
        if (nl != L || cl2 != s.cl || cf2 != s.cf) P.gss[g] = SsRec{nl, s.term, cl2, cf2};
        if (hbw) at(P.hb, g) = T.now;
      }
      if (shw && !shm) {   // SH from this tick's first entry on
        at(P.grot, g) = uint16_t(uint32_t(rot) | ROT_SH);
        at(P.gshf, g) = L + 1;
      }
      committed = cl2 - s.cl;
      if (n) {
        term = s.term;
        vb = P.cv_stride ? uint64_t(reinterpret_cast<uintptr_t>(T.cv + g))
                         : rng_k(key, uint32_t(c), ST_VALUE, uint64_t(T.tick));
        if constexpr (SH) {
          // one copy per entry in the shared ring: 64 consecutive groups'
          // entries are one row (sh_in_tile with one slot per chunk; the gate
          // keeps engines with slot chunks on the general body)
          const uint64_t shb = sh_tile(__builtin_amdgcn_readfirstlane(g), P.KP);
          const uint32_t lane = threadIdx.x & 63u;
          uint32_t cs = 0;
          if constexpr (CRC) cs = crc_term_state(tab, term);
          auto put = [&](int e, int64_t v) {
            const uint32_t so = (uint32_t((ph + e) & int(P.kmask)) << 6) + lane;
            __builtin_nontemporal_store(term, &(P.term + shb)[so]);
            __builtin_nontemporal_store(v, &(P.value + shb)[so]);
            if constexpr (CRC) __builtin_nontemporal_store(crc_value_final(tab, cs, v), &(P.crc + shb)[so]);
          };
          // (one loop per value source: the trace RNG's has no load in it, so
          // no entry's stores wait for the memory counter of the one before)
          if (P.cv_stride) {
            put(0, cv0);
            for (int e = 1; e < n; ++e) put(e, cv_value(vb, uint32_t(e), P.cv_stride));
          } else {
            for (int e = 0; e < n; ++e) put(e, cv_value(vb, uint32_t(e), 0u));
          }
        }
      }
    }
  }
  if constexpr (!SH) {
    const bool wr = fit && n;
    if (n && __ballot(wr)) {   // (n: wave-uniform)
      const int lane = threadIdx.x & 63;
      const uint32_t g0 = __builtin_amdgcn_readfirstlane(g);
      const uint64_t cvs = P.cv_stride;
      uint32_t cs = 0;
      if constexpr (CRC) cs = crc_term_state(tab, term);
      // RAFTSTEP_SH=0: whole ring rows, all R replicas (holes for the lanes that do not fit)
      const uint64_t tb = ring_tile(g0, P.KP, R);
      int32_t* const rt = P.term + tb;
      int64_t* const rv = P.value + tb;
      uint32_t* const rc = CRC ? P.crc + tb : nullptr;
      int k_src[R], k_term[R];
      bool k_on[R];
#pragma unroll
      for (int k = 0; k < R; ++k) {
        k_src[k] = (k * 64 + lane) / R;
        k_term[k] = __shfl(term, k_src[k]);
        k_on[k] = __shfl(int(wr), k_src[k]) != 0;
      }
      for (int e = 0; e < n; ++e) {
        const int64_t v = (cvs && e == 0) ? cv0 : cv_value(vb, uint32_t(e), cvs);
        uint32_t stamp = 0;
        if constexpr (CRC) stamp = crc_value_final(tab, cs, v);
        const uint32_t row = uint32_t((ph + e) & int(P.kmask)) * 64u * R;
        const int vlo = int(uint32_t(uint64_t(v))), vhi = int(uint32_t(uint64_t(v) >> 32));
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const int lo = __shfl(vlo, k_src[k]), hi = __shfl(vhi, k_src[k]);
          uint32_t sk = 0;
          if constexpr (CRC) sk = uint32_t(__shfl(int(stamp), k_src[k]));
          if (k_on[k]) {
            const uint32_t o = row + uint32_t(k * 64 + lane);
            __builtin_nontemporal_store(k_term[k], &rt[o]);
            __builtin_nontemporal_store(int64_t((uint64_t(uint32_t(hi)) << 32) | uint32_t(lo)), &rv[o]);
            if constexpr (CRC) __builtin_nontemporal_store(sk, &rc[o]);
          }
        }
      }
    }
  }
  // passed on (a proof violated): the id alone, one atomic per such lane
  if (pass) {
    const uint32_t k = shard_of_block(gblk, P.shard_sb);
    list[k * P.scap + atomicAdd(&count[k * SHARD_STRIDE], 1u)] = g;
  }
  if (stats) lean_stats<RAFT>(g < P.G, committed - lean_base_committed(RAFT, R, uint32_t(n)), fit, false, false, stats);
}

}  // namespace raftstep
