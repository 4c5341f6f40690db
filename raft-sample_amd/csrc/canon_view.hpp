// canon_view.hpp — the canonical view (raft_state_view) of a group, derived
// from the engine's compressed state. The one device-side reader: the digest
// (k_init.hip), the commit feed (k_feed.hip) and the gather kernels behind
// raft_store_state / _range / _groups and raft_nodelog (k_groups.hip) all read
// a group through CanonGroup and its entries through canon_entry; a new
// storage form is taught to this file alone. The tick kernels keep their own
// readers (raft_device.hpp Group) and do not include it.
#pragma once
#include "tick_common.hpp"

namespace raftstep {

// What every reader loads first for group g: gmeta, and under SSYNC (the
// compressed state) the gss record, with glx for LXS / SXS.
template <int R>
struct CanonGroup {
  uint32_t g;
  int meta, primary, fault;
  bool msync, ssync;
  SsRec ss;
  LxRec lx;

  __device__ __forceinline__ CanonGroup(const DevPlanes& P, uint32_t g_) : g(g_) {
    meta = at(P.gmeta, g);
    primary = meta & 0xF;
    fault = (meta >> 4) & 7;
    msync = (meta & M_MSYNC) && primary < R;
    ssync = (meta & M_SSYNC) && primary < R;
    ss = ssync ? P.gss[g] : SsRec{0, 0, 0, 0};
    lx = (ssync && uses_glx(meta)) ? P.glx[g] : LxRec{0, 0};
  }
  // time of the last heartbeat that reset every follower (SH: implied, now of the last tick run)
  __device__ __forceinline__ int hb(const DevPlanes& P) const {
    return (P.sh && (at(P.grot, g) & ROT_SH)) ? P.sh_hb : at(P.hb, g);
  }
  __device__ __forceinline__ int last(const DevPlanes& P, int r) const {
    return ssync ? ss_last(ss, r, primary, meta, lx) : at(P.last, rix<R>(g, r));
  }
  __device__ __forceinline__ int term(const DevPlanes& P, int r) const {
    return ssync ? ss_term(ss, r, meta, lx) : at(P.term, rix<R>(g, r));
  }
  // term of the last entry as the engine caches it (SSYNC: the replica's term)
  __device__ __forceinline__ int last_term(const DevPlanes& P, int r) const {
    return ssync ? ss_term(ss, r, meta, lx) : at(P.lterm, rix<R>(g, r));
  }
  // (the commit plane of an SSYNC group is read for SXS's stale leader only)
  __device__ __forceinline__ int commit(const DevPlanes& P, int r) const {
    const bool plane = !ssync || (is_sxs(meta) && r == lx.dl);
    const int pc = plane ? at(P.commit, rix<R>(g, r)) : 0;
    return ssync ? ss_commit(ss, r, primary, meta, lx, pc) : pc;
  }
  // high-water mark of a replica whose LastApplied is l; MSYNC: max(plane, LastApplied)
  // (HWX; the plane is at most LastApplied without it); REF has none: LastApplied
  __device__ __forceinline__ int hwm(const DevPlanes& P, int r, int raft, int l) const {
    if (!raft) return l;
    const int h = at(P.hwm, rix<R>(g, r));
    return msync ? max(h, l) : h;
  }
  // MatchIndex / NextIndex of replica r (its role given) for peer p; last: every replica's
  // LastApplied. 0 for non-leaders and p == r. The primary's rows are implicit under MSYNC
  // (SXS: the stale leader's row is explicit), further leaders' rows sit in xmatch / xnext,
  // REF derives NextIndex = MatchIndex + 1.
  __device__ __forceinline__ void match_next(const DevPlanes& P, int raft, int role, int r, int p,
                                             const int (&last)[R], int* m, int* nx) const {
    *m = *nx = 0;
    if (role != ROLE_L || p == r) return;
    const int lp = sel(last, p);
    const bool mp = msync && msync_peer(meta, lx, p);
    if (r == primary) *m = mp ? lp : at(P.lmatch, rix<R>(g, p));
    else *m = at(prow(P.xmatch, r * R + p, P.Gp), g);
    if (!raft) *nx = *m + 1;
    else if (r == primary) *nx = mp ? lp + 1 : at(P.lnext, rix<R>(g, p));
    else *nx = at(prow(P.xnext, r * R + p, P.Gp), g);
  }
};

// The rs word: role:2 | vote:4 | timer duration
__device__ __forceinline__ int rs_role(uint32_t x) { return int(x & 3u); }
__device__ __forceinline__ uint32_t rs_voted(uint32_t x) { return (x >> 2) & 15u; }
__device__ __forceinline__ int rs_timeout(uint32_t x) { return int(x >> 6); }
// deadline = effective timer start + timeout; followers / candidates also count the heartbeat
__device__ __forceinline__ int canon_deadline(int role, int tstart, int hb, int timeout) {
  return (role == ROLE_L ? tstart : max(tstart, hb)) + timeout;
}

// Where a group's entries are: the three ring phase segments (ring_slot) and,
// in shared form (SH), the first index that lives in the shared ring.
struct RingForm {
  uint32_t rot, rota, rotb;
  int sb, sb2, shf;
  bool sh;   // shared form; a flag, not a sentinel in shf: 2^31-1 is a log index
};
__device__ __forceinline__ RingForm ring_form(const DevPlanes& P, uint32_t g) {
  RingForm f;
  f.rot = at(P.grot, g);
  f.rota = at(P.grota, g);
  f.rotb = at(P.grotb, g);
  f.sb = at(P.gsb, g);
  f.sb2 = at(P.gsb2, g);
  f.sh = P.sh && (f.rot & ROT_SH);
  f.shf = f.sh ? at(P.gshf, g) : 0;
  return f;
}
// Entry idx of replica r's log, from the shared ring for idx >= shf and the
// replica ring otherwise; `want` names the words to read (the others are 0),
// and the stamp is read only with payload_crc.
enum : int { EW_TERM = 1, EW_VALUE = 2, EW_CRC = 4, EW_ALL = 7 };
struct Entry {
  int32_t term;
  int64_t value;
  uint32_t crc;
};
template <int R>
__device__ __forceinline__ Entry canon_entry(const DevPlanes& P, const RingForm& f, uint32_t g, uint32_t r, int idx,
                                             int want = EW_ALL) {
  Entry e{0, 0, 0};
  const uint32_t slot = ring_slot(idx, f.rot, f.rota, f.rotb, f.sb, f.sb2, P.kmask);
  if (f.sh && idx >= f.shf) {
    const uint64_t shb = sh_tile(g, P.KP);
    const uint32_t so = sh_in_tile(g, slot, P.sh_cs);
    if (want & EW_TERM) e.term = at(P.sh_term + shb, so);
    if (want & EW_VALUE) e.value = at(P.sh_value + shb, so);
    if ((want & EW_CRC) && P.crc_on) e.crc = at(P.sh_crc + shb, so);
  } else {
    const uint64_t rb = ring_tile(g, P.KP, R);
    const uint32_t q = ring_in_tile(g, R, slot, r);
    if (want & EW_TERM) e.term = at(P.log_term + rb, q);
    if (want & EW_VALUE) e.value = at(P.log_value + rb, q);
    if ((want & EW_CRC) && P.crc_on) e.crc = at(P.log_crc + rb, q);
  }
  return e;
}

}  // namespace raftstep
