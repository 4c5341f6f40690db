// tick_steady.hpp — the steady form of the one-tick lean kernel (k_fast.hip
// tick_lean_kernel<R, CRC, SEM, true, SH, ONE>).
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
// DevPlanes / Trace.
// A lane that does not fit (which the proofs exclude) leaves its group alone
// and appends its id to the block's list shard, one atomic per such lane, as
// tick_fused_kernel does: the end-of-call check turns it into RAFT_EINTERNAL.
//
// The body is one straight line for a fitting lane:
//   1. every scalar argument the fitting path uses is fetched in one batch at
//      entry and pinned in SGPRs (STEADY_PIN_*), so that no scalar load is
//      left behind the vector loads;
//   2. the group's words are loaded (gmeta, the record, the rotation, the
//      staged value) — a lane past the last group reads the last group's
//      words, in bounds, and stores nothing, so there is no branch around them;
//   3. in the loads' shadow the group's RNG key is hashed (two of the five
//      splitmix64 rounds: everything that needs no loaded word; only the
//      leader id enters later) and pinned in VGPRs ahead of the first use of a
//      loaded word, i.e. ahead of the wait for the loads;
//   4. the fit test, the closed form and the stores.
// ONE is the instantiation of the launch-uniform case that is the whole tick
// of the headline shape: trace-RNG values, exactly one client entry this
// tick, plain (cached) record stores, the shared ring. There the entry loop,
// both store forms and the staged / trace selection are gone at compile time;
// every other launch runs the generic instantiation, which decides them at
// run time as before (they are uniform over a launch). steady_one() is the
// host's rule for it.
#pragma once
#include "tick_common.hpp"

namespace raftstep {

// (SteadyPlanes, SteadyTick, SteadyCall: kernels.h)
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
inline SteadyTick steady_tick_args(const SteadyCall& C, const Trace& T) {
  SteadyTick S{};
  S.seed = T.seed; S.tick = T.tick; S.now = T.now;
  S.n = T.n_tick;
  S.ph = uint32_t(T.eb_tick) & C.planes.kmask;
  S.cv = C.cv ? C.cv + uint64_t(T.tick - C.cv_t0) * C.cv_tstride : nullptr;
  return S;
}
// The launches the ONE instantiation may run: what it assumes of the planes
// (constant over a call) and of a tick.
inline bool steady_one(const SteadyPlanes& S, bool sh) { return sh && !S.cv_stride && !S.rec_nt; }
inline bool steady_one(const SteadyTick& T) { return T.n == 1u && !T.cv; }

// The values are in scalar registers at this point (an empty statement the
// compiler cannot move their loads below): one statement for up to eight
// values, so that their loads are issued as one batch and waited for once.
// This is a request the compiler honours today, not a guarantee: the order
// DESIGN §4 quotes was read from the generated code (hipcc -O3 -S, gfx950) and
// nothing keeps a later toolchain from scheduling around these statements
// differently. The results do not depend on it, only the kernel's time.
#define STEADY_PIN_S2(a, b) asm volatile("" : "+s"(a), "+s"(b))
#define STEADY_PIN_S3(a, b, c) asm volatile("" : "+s"(a), "+s"(b), "+s"(c))
#define STEADY_PIN_S4(a, b, c, d) asm volatile("" : "+s"(a), "+s"(b), "+s"(c), "+s"(d))
#define STEADY_PIN_S8(a, b, c, d, e, f, g, h) \
  asm volatile("" : "+s"(a), "+s"(b), "+s"(c), "+s"(d), "+s"(e), "+s"(f), "+s"(g), "+s"(h))

// A pinned pointer is opaque to the compiler, which would make its accesses
// flat ones and drop their non-temporal hint: the pointers are pinned as
// integers and become pointers to global memory (what a kernel argument
// points to) afterwards.
template <typename T>
__device__ __forceinline__ uint64_t steady_addr(T* p) { return uint64_t(reinterpret_cast<uintptr_t>(p)); }
template <typename T>
__device__ __forceinline__ T* steady_global(uint64_t a) {
  return (T*)(__attribute__((address_space(1))) T*)a;
}

template <int R, bool CRC, bool RAFT, bool SH, bool ONE>
__device__ __forceinline__ void steady_tick(const SteadyPlanes& PA, const SteadyTick& TA, unsigned long long* stats_a,
                                            uint32_t* list_a, uint32_t* count_a, uint32_t gofs) {
  static_assert(!ONE || SH, "the one-entry instantiation writes the shared ring");
  // 1. the scalar prologue (ONE: what it assumes is a constant, not an argument)
  uint64_t a_gmeta = steady_addr(PA.gmeta), a_gss = steady_addr(PA.gss), a_grot = steady_addr(PA.grot);
  uint64_t a_hb = steady_addr(PA.hb), a_gshf = steady_addr(PA.gshf.p), a_term = steady_addr(PA.term);
  uint64_t a_value = steady_addr(PA.value), a_crc = steady_addr(PA.crc), a_tab = steady_addr(PA.crc_tab);
  uint64_t a_stats = steady_addr(stats_a), a_list = steady_addr(list_a), a_count = steady_addr(count_a);
  uint64_t a_cv = ONE ? 0u : steady_addr(TA.cv);
  uint64_t gbase = PA.gbase, seed = TA.seed;
  int64_t tick = TA.tick;
  uint32_t G = PA.G, K = PA.K, KP = PA.KP, kmask = PA.kmask, dbg_pass = PA.dbg_pass;
  uint32_t scap = PA.scap, shard_sb = PA.shard_sb;   // (the lane that does not fit: no load left for it either)
  uint32_t ph_u = TA.ph;
  uint64_t cvs = ONE ? 0u : PA.cv_stride;
  uint32_t rec_nt = ONE ? 0u : PA.rec_nt, n_u = ONE ? 1u : TA.n;
  int32_t now = TA.now;
  STEADY_PIN_S8(a_gmeta, a_gss, a_grot, a_term, a_value, gbase, seed, tick);
  STEADY_PIN_S8(G, K, KP, kmask, dbg_pass, ph_u, gofs, a_stats);
  STEADY_PIN_S4(a_list, a_count, scap, shard_sb);
  if constexpr (CRC) STEADY_PIN_S2(a_crc, a_tab);
  if constexpr (!ONE) {
    STEADY_PIN_S4(cvs, a_cv, rec_nt, n_u);
    STEADY_PIN_S3(a_hb, a_gshf, now);
  } else {
    STEADY_PIN_S2(a_gshf, now);
  }
  const uint16_t* const gmeta = steady_global<const uint16_t>(a_gmeta);
  SsRec* const gss = steady_global<SsRec>(a_gss);
  uint16_t* const grot = steady_global<uint16_t>(a_grot);
  int32_t* const hb = steady_global<int32_t>(a_hb);
  int32_t* const gshf = steady_global<int32_t>(a_gshf);
  int32_t* const ring_t = steady_global<int32_t>(a_term);
  int64_t* const ring_v = steady_global<int64_t>(a_value);
  uint32_t* const ring_c = steady_global<uint32_t>(a_crc);
  const uint32_t* const crc_tab = steady_global<const uint32_t>(a_tab);
  const int64_t* const cv = steady_global<const int64_t>(a_cv);
  unsigned long long* const stats = steady_global<unsigned long long>(a_stats);
  uint32_t* const list = steady_global<uint32_t>(a_list);
  uint32_t* const count = steady_global<uint32_t>(a_count);
  const uint32_t gblk = (gofs >> 8) + blockIdx.x;   // this block's 256 groups (gofs: tick_lean_kernel)
  const uint32_t g = gblk * 256u + threadIdx.x;
  __shared__ uint32_t tab[CRC ? 2048 : 1];
  if constexpr (CRC) {   // (stage_crc_tab)
    const uint4* src = reinterpret_cast<const uint4*>(crc_tab);
    uint4* dst = reinterpret_cast<uint4*>(tab);
    for (uint32_t i = threadIdx.x; i < 512u; i += 256u) dst[i] = src[i];
    __syncthreads();
  }
  const int n = int(n_u), ph = int(ph_u);
  // 2. one round trip: gmeta, the record, the ring rotation, the staged value
  // (a lane past the last group: the last group's words, never used)
  const bool live = g < G;
  const uint32_t gi = live ? g : G - 1u;
  const int meta = at(gmeta, gi);
  const SsRec s = gss[gi];
  const int rot = at(grot, gi);
  int64_t cv0 = 0;   // staged client values: the group's entry 0 of this tick
  if constexpr (!ONE) {
    if (cv && n) cv0 = __builtin_nontemporal_load(cv + gi);
  }
  // 3. in their shadow: the value stream's key but for the leader id
  // (rng_k(key, c, ST_VALUE, tick) = sm64(sm64(key ^ (ST_VALUE << 32 | c)) ^ tick), c < 16)
  uint64_t kq = group_key(seed, gbase + g) ^ (uint64_t(ST_VALUE) << 32);
  asm volatile("" : "+v"(kq));
  // 4. the fit test and the closed form of tick_lean_kernel's normal class
  const int c = meta & 0xF, L = s.last;
  const bool skip = (meta & (M_DEFER | (7 << 4))) != 0;   // pending catch-up / frozen group
  const bool shm = (uint32_t(rot) & ROT_SH) != 0u;
  // (bitwise: one straight line of compares instead of a branch per term)
  // SSYNC and neither LXS nor SXS (uses_glx: SXS is SSYNC with ONESTALE) nor, RAFT, HWX
  constexpr int other = M_LXS | M_ONESTALE | (RAFT ? M_HWX : 0);
  const int ln = int(uint32_t(L) + uint32_t(n));   // (L + n; used only where it does not overflow)
  const bool fit = live & !skip & ((meta & (M_SSYNC | other)) == M_SSYNC) & (c < R) & (g != dbg_pass) &
                   (L > 0) & (L <= I32MAX - n) & (n < int(K)) & (s.cl <= ln) &
                   ((n == 0) | (((uint32_t(L) + uint32_t(rot)) & kmask) == uint32_t(ph)));
  const bool pass = live & !skip & !fit;
  int committed = 0, term = 0;
  uint64_t vb = 0;
  if (fit) {
    const int nl = L + n;
    const int cl2 = (RAFT ? nl > s.cl : (2 * (R - 1) > R && nl > s.cl)) ? nl : s.cl;
    const int cf2 = s.cl > s.cf ? s.cl : s.cf;
    const bool shw = SH && n > 0;                // this tick's entries go to the shared ring
    const bool hbw = !(shw || shm);              // (SH: a group in shared form implies its heartbeat time)
    if (rec_nt) {
      typedef int32_t i4 __attribute__((ext_vector_type(4)));
      if (nl != L || cl2 != s.cl || cf2 != s.cf)
        __builtin_nontemporal_store(i4{nl, s.term, cl2, cf2}, reinterpret_cast<i4*>(&gss[g]));
      if (hbw) __builtin_nontemporal_store(int32_t(now), &hb[g]);
    } else {
      if (nl != L || cl2 != s.cl || cf2 != s.cf) gss[g] = SsRec{nl, s.term, cl2, cf2};
      if (hbw) at(hb, g) = now;
    }
    if (shw && !shm) {   // SH from this tick's first entry on
      at(grot, g) = uint16_t(uint32_t(rot) | ROT_SH);
      *reinterpret_cast<int32_t*>(reinterpret_cast<char*>(gshf) + uint32_t(g * 16u)) = L + 1;
    }
    committed = cl2 - s.cl;
    if (n) {
      term = s.term;
      vb = cvs ? uint64_t(reinterpret_cast<uintptr_t>(cv + g)) : sm64(sm64(kq ^ uint64_t(uint32_t(c))) ^ uint64_t(tick));
      if constexpr (SH) {
        // one copy per entry in the shared ring: 64 consecutive groups'
        // entries are one row (sh_in_tile with one slot per chunk; the gate
        // keeps engines with slot chunks on the general body)
        const uint64_t shb = sh_tile(__builtin_amdgcn_readfirstlane(g), KP);
        const uint32_t lane = threadIdx.x & 63u;
        uint32_t cs = 0;
        if constexpr (CRC) cs = crc_term_state(tab, term);
        auto put = [&](int e, int64_t v) {
          const uint32_t so = (uint32_t((ph + e) & int(kmask)) << 6) + lane;
          __builtin_nontemporal_store(term, &(ring_t + shb)[so]);
          __builtin_nontemporal_store(v, &(ring_v + shb)[so]);
          if constexpr (CRC) __builtin_nontemporal_store(crc_value_final(tab, cs, v), &(ring_c + shb)[so]);
        };
        // (one loop per value source: the trace RNG's has no load in it, so
        // no entry's stores wait for the memory counter of the one before)
        if constexpr (ONE) {
          put(0, cv_value(vb, 0u, 0u));
        } else if (cvs) {
          put(0, cv0);
          for (int e = 1; e < n; ++e) put(e, cv_value(vb, uint32_t(e), cvs));
        } else {
          for (int e = 0; e < n; ++e) put(e, cv_value(vb, uint32_t(e), 0u));
        }
      }
    }
  }
  if constexpr (!SH) {
    const bool wr = fit && n;
    if (n && __ballot(wr)) {   // (n: wave-uniform)
      const int lane = threadIdx.x & 63;
      const uint32_t g0 = __builtin_amdgcn_readfirstlane(g);
      uint32_t cs = 0;
      if constexpr (CRC) cs = crc_term_state(tab, term);
      // RAFTSTEP_SH=0: whole ring rows, all R replicas (holes for the lanes that do not fit)
      const uint64_t tb = ring_tile(g0, KP, R);
      int32_t* const rt = ring_t + tb;
      int64_t* const rv = ring_v + tb;
      uint32_t* const rc = CRC ? ring_c + tb : nullptr;
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
        const uint32_t row = uint32_t((ph + e) & int(kmask)) * 64u * R;
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
    const uint32_t k = shard_of_block(gblk, shard_sb);
    list[k * scap + atomicAdd(&count[k * SHARD_STRIDE], 1u)] = g;
  }
  if (stats) lean_stats<RAFT>(live, committed - lean_base_committed(RAFT, R, uint32_t(n)), fit, false, false, stats);
}

}  // namespace raftstep
