// kernels.h — host-side launchers and device argument records of the engine.
//
//  tick_fast_kernel<R,CRC,SEM> (k_fast.hip): steady-state tick, one lane
//        per group, HBM-bound (~233 B per group-step at R=5, E=1); groups it
//        cannot take go to a worklist.
//  tick_slow_kernel<R,SEM> (k_ref.hip / k_raft.hip): the general tick
//        (elections, step-downs, faults, EXT drops) over the worklist.
//  ops_kernel<R,SEM>: the message-level handler API (AppendEntries /
//        RequestVote receivers, node steps) over distinct groups.
//  init_*_kernel<R> (k_init.hip): NewNode state / post-election state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raft_device.hpp"

namespace raftstep {

enum : uint32_t {
  OP_CLIENT_APPEND = 1, OP_LEADER_ROUND = 2, OP_CANDIDATE_ROUND = 3, OP_TIMEOUT = 4,
  OP_LEADER_COMMIT = 5, OP_AE = 100, OP_VR = 101
};

// One handler-batch element after host-side range checks (int64 -> int32).
struct DevOp {
  uint64_t group;
  uint32_t replica;   // receiving / acting replica
  uint32_t kind;
  int64_t arg;        // CLIENT_APPEND value
  int32_t term, prev_idx, prev_term, lc;  // AE / VR request fields
  uint32_t n;         // AE: len(Logs)
  uint32_t skip;      // AE: values/stamps of Logs[0..skip) are not staged (only the last K can land in the ring)
  uint64_t off;       // AE: offset of Logs[0] in the term array
  uint64_t voff;      // AE: offset of Logs[skip] in the value / stamp arrays
};
struct DevRes {
  int32_t status, fault, ok, term;
  int64_t value;      // AE: MatchIndex; VR: granted; ops: see raft_op_result
};

// Steady-state fast kernel; groups it does not take are DEFERred to `work`.
// ev_start/ev_stop (may be null) time the dispatch itself (hipExtLaunchKernel).
hipError_t launch_tick_fast(int R, int sem, const DevPlanes& P, const Trace& T, unsigned long long* stats, uint32_t* work,
                            int32_t* work_tick, uint32_t* work_count, int force_slow, hipStream_t s,
                            hipEvent_t ev_start, hipEvent_t ev_stop);
// Two-pass tick: tick_lean_kernel (launch_tick_lean) takes the compressed
// steady groups and appends every other live group to `list` (counter
// `count`), then tick_list_kernel (launch_tick_list) runs the full fast_group
// over that list and zeroes `next_count`. Events (may be null) time each
// dispatch. A list-skipping call launches the lean kernel alone; the in-line
// and the pipelined tick launch both (engine.cpp tick_skip / tick_inline /
// tick_pipelined).
// lflags bit 0 = leave the groups marked in P.glst alone (and clear the
// marks), bit 1 = mark the groups passed on (both the pipelined tick's). With
// `next` the list kernel runs its groups through the following tick too (a
// second fast_group step on the staged state; its stats and deferrals go to
// next's record and worklist), so that the next lean kernel can run beside it.
struct ListNext {
  unsigned long long* stats;    // the following tick's stats slots
  uint32_t* work;               // the worklist of the following tick's window
  int32_t* work_tick;
  uint32_t* work_count;
};
// Fused steady ticks (steady-state list skip): nticks ticks of every
// compressed steady group in one launch; stats of tick j at stats + j slots.
hipError_t launch_tick_fused(int R, int sem, const DevPlanes& P, const Trace& T, int nticks, unsigned long long* stats,
                             uint32_t* list, uint32_t* count, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop);
// (g0, ng: the launch covers groups [g0, g0 + ng) only; g0 a multiple of 256;
// zero_count: list counters the launch zeroes, block 0, before anything else)
hipError_t launch_tick_lean(int R, int sem, const DevPlanes& P, const Trace& T, unsigned long long* stats, uint32_t* list,
                            uint32_t* count, int lflags, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop,
                            uint64_t g0 = 0, uint64_t ng = ~0ull, uint32_t* zero_count = nullptr);

// The lean kernel's steady form (tick_steady.hpp) — only for the ticks of a
// list-skipping call with every live group in the global ring phase, no
// device counters and no timing diagnostics. Its launch arguments: what the
// body reads of DevPlanes (constant between launches but for dbg_pass /
// rec_nt, which the host sets between calls) ...
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
// What a call's steady launches share, worked out once per call
// (steady_resolve): the planes' record, the instantiations for the engine's
// (R, semantics, CRC, shared ring) — the generic one and, where the planes
// admit it, the one-entry one (null otherwise; picked per launch by the
// tick's entries) — and what a tick's record needs of DevPlanes.
struct SteadyCall {
  SteadyPlanes planes;
  const void* generic;
  const void* one;
  const int64_t* cv;
  int64_t cv_t0;
  uint64_t cv_tstride;
};
hipError_t steady_resolve(int R, int sem, const DevPlanes& P, SteadyCall* out);
// One launch over groups [g0, g0 + ng): fills the tick's record and the group
// offset, nothing else. Returns the launch call's own status; *one_launches
// (may be null) counts the launches of the one-entry instantiation.
hipError_t launch_tick_steady(const SteadyCall& C, const Trace& T, unsigned long long* stats, uint32_t* list,
                              uint32_t* count, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop, uint64_t g0 = 0,
                              uint64_t ng = ~0ull, uint64_t* one_launches = nullptr);

hipError_t launch_tick_list(int R, int sem, const DevPlanes& P, const Trace& T, unsigned long long* stats, uint32_t* work,
                            int32_t* work_tick, uint32_t* work_count, uint32_t* list, uint32_t* count,
                            uint32_t* next_count, const ListNext* next, hipStream_t s, hipEvent_t ev_start,
                            hipEvent_t ev_stop);
// General kernel: catches every worklisted group up to last_tick; zeroes
// `next_count`. lane_per_group: the one-lane-per-group form (tick_slow_kernel)
// instead of the replica-parallel one (tick_seg_kernel).
hipError_t launch_tick_slow(int R, int sem, const DevPlanes& P, const Trace& T0, int64_t first_tick, int64_t win_first, int64_t last_tick,
                            unsigned long long* stats, const uint32_t* work, const int32_t* work_tick,
                            const uint32_t* work_count, uint32_t* next_count, int lane_per_group, hipStream_t s);
hipError_t launch_ops(int R, int sem, const DevPlanes& P, const Trace& T, const DevOp* ops, uint32_t n,
                      const int32_t* et, const int64_t* ev, const uint32_t* ec, DevRes* out, hipStream_t s);
// Client proposals (raft_propose; propose_kernel<R,SEM>, k_ref.hip /
// k_raft.hip). props: the call's raft_proposal list as it came, ids range-
// checked by the host; perm / seg: the plan of propose_plan.hpp (list
// positions by group, nseg + 1 segment starts); out: 32 B per proposal
// (raft_ticket), indexed by list position, 16-B aligned.
struct DevProposal {
  uint64_t group;
  int64_t value;
};
hipError_t launch_propose(int R, int sem, const DevPlanes& P, const Trace& T, const DevProposal* props,
                          const uint32_t* perm, const uint32_t* seg, uint32_t nseg, void* out, hipStream_t s);
// raft_ticket_status (ticket_status_kernel<R>, k_propose.hip): one lane per
// ticket of tickets[0..n) (32 B each, checked by the host: local < G), read on
// the canonical view. out (may be null): 8 B per ticket (raft_ticket_result);
// tot (may be null): 8 words, tot[k] += the tickets in state k.
hipError_t launch_ticket_status(int R, const DevPlanes& P, int raft, const void* tickets, uint32_t n, void* out,
                                unsigned long long* tot, hipStream_t s);
hipError_t launch_init_new(int R, const DevPlanes& P, const Trace& T, hipStream_t s);
// Per-group state digest (same definition as oracle_state_digest) + wrapping sum.
hipError_t launch_digest(int R, const DevPlanes& P, int raft, uint64_t* per_group, unsigned long long* total,
                         hipStream_t s);
// End-of-call check record (one more block of the stats reduce launch):
// out[CHK_LISTED] = groups on the two-pass list counters (both parities),
// out[CHK_DEFERRED] = groups the last general window's worklist held,
// out[CHK_LAST_LIST] = groups on list llast alone (what the lean kernel passed
// on at the call's last tick; the engine's pipeline choice, RAFTSTEP_PIPELINE=2),
// out[CHK_MAGIC] = a constant proving the record was written this call.
// zero_lists: zero both list counters afterwards (a list-skipping call).
enum : int { CHK_LISTED = 0, CHK_DEFERRED = 1, CHK_LAST_LIST = 2, CHK_MAGIC = 7 };
struct CallCheck {
  uint32_t* wcount;             // the engine's counter block (raft_device.hpp WCOUNT_WORDS)
  int wlast;                    // parity of the worklist the last window tail took
  int zero_lists;
  unsigned long long* out;      // NSTAT words
  int llast;                    // list set of the call's last tick
  // host mirror (a call whose records are all reduced by this one launch, no
  // communicator): every block also writes its record to hout (pinned,
  // coherent host memory, same layout as `out` of the launch), and the last
  // block to finish stores `seq` to *hdone (system scope), so that the host
  // reads the call's records without a device-to-host copy and sees the end
  // of the call without waiting for the stream's completion signal
  unsigned long long* hout;
  uint32_t* hdone;
  unsigned int* ctr;            // device counter of finished blocks (zero between launches)
  uint32_t seq;
};
// Sums the STAT_SLOTS slots of nticks consecutive per-tick records of `hist`
// into out[nticks][NSTAT] and zeroes those slots; with `chk` also writes the
// check record (nticks may then be 0).
// Clears DEFER of the groups on worklist `parity` (work), records their
// number and zeroes that worklist's counters (k_init.hip window_tail_kernel).
hipError_t launch_window_tail(const DevPlanes& P, const uint32_t* work, uint32_t* wcount, int parity, hipStream_t s);
// The base the lean / fused kernels' exception statistics are relative to
// (tick_common.hpp lean_stats): every tick of a two-pass call, G live groups
// each taking a normal tick.
struct LeanBase {
  uint64_t G;          // groups (0: no lean kernel ran, no base)
  int64_t t0;          // tick of the reduce's first record
  uint32_t E, period;  // client entries per client tick, ticks per client tick
  uint32_t R, raft;
};
hipError_t launch_stats_reduce(unsigned long long* hist, unsigned long long* out, uint32_t nticks, const LeanBase& lb,
                               hipStream_t s, const CallCheck* chk = nullptr);
hipError_t launch_init_steady(int R, const DevPlanes& P, const Trace& T, int32_t leader, hipStream_t s);
hipError_t launch_vx_flush(int R, const DevPlanes& P, uint64_t Qb, uint32_t E, uint32_t period, uint64_t seed,
                           hipStream_t s);
// SH (raft_device.hpp ROT_SH): every group's shared entries into its replica rings
hipError_t launch_sh_flush(int R, const DevPlanes& P, hipStream_t s);
// Commit feed (k_feed.hip; raft_feed_*). cursors: [G][nm] int32, one per
// group and replica of `mask` (nm = its bits, in replica order).
// launch_feed_count: per block the entries it has to deliver (bsum), the
// poll's lost entries and stalled pairs (added to tot[1], tot[2], zero between
// polls), cursors moved past lost entries; mode 1 instead sets every cursor
// to min(CommitIndex, LastApplied) and counts nothing.
// launch_feed_scan: boff = exclusive scan of bsum[nb]; res (pinned host
// memory) = {the total, lost, stalled}; tot[1], tot[2] zeroed again.
// launch_feed_emit: records [0, cap) of the (group, replica, index) order to
// `out` (32 B each, raft_feed_entry), cursors advanced by what was written;
// paired: the store form (k_feed.hip).
hipError_t launch_feed_count(int R, const DevPlanes& P, int raft, uint32_t mask, uint32_t nm, int32_t* cursors,
                             uint32_t* bsum, unsigned long long* tot, int mode, hipStream_t s);
hipError_t launch_feed_scan(const uint32_t* bsum, uint64_t* boff, uint32_t nb, unsigned long long* tot,
                            unsigned long long* res, hipStream_t s);
hipError_t launch_feed_emit(int R, const DevPlanes& P, int raft, uint32_t mask, uint32_t nm, int32_t* cursors,
                            const uint64_t* boff, uint64_t cap, void* out, int paired, hipStream_t s);
// Group directory (k_groups.hip; raft_group_scan / raft_store_groups /
// raft_restart_groups). select: enum raft_group_select; the launches cover the
// 256-group blocks from the one holding `first` on (nb = ceil(G / 256) -
// first / 256 block sums; first < G).
// launch_group_count: per block its hits in [first, G) (bsum).
// launch_group_emit: hits [0, cap) of the ascending group order to `out`
// (16 B each, raft_group_hit), cap >= 1 and at most the total (boff: the
// exclusive scan of bsum, launch_feed_scan); *next = the local id after hit
// cap - 1.
hipError_t launch_group_count(int R, const DevPlanes& P, uint32_t select, uint32_t first, uint32_t* bsum, hipStream_t s);
hipError_t launch_group_emit(int R, const DevPlanes& P, uint32_t select, uint32_t first, const uint64_t* boff,
                             uint64_t cap, void* out, unsigned long long* next, hipStream_t s);
// The canonical view (raft_state_view's fields and shapes, indexed by list
// position; derived in canon_view.hpp) of groups ids[0..n), or with ids null
// of the range [first, first + n), into device buffers; null fields are
// skipped, and without a log field no ring word is read. bad (may be null): a
// device word, zero before the launch, for the last-entry term check; nonzero
// afterwards = ~(g R + r) of the lowest group and replica whose cached
// last-entry term differs from the ring's (checked only with log_term).
struct GatherOut {
  uint8_t *role, *voted;
  int32_t *term, *last, *commit, *deadline, *timeout, *match;
  uint8_t* fault;
  int32_t* log_term;
  int64_t* log_value;
  uint32_t* log_crc;
  int32_t *next, *hwm;
  uint8_t* iso_victim;
};
hipError_t launch_gather(int R, const DevPlanes& P, int raft, uint32_t first, const uint32_t* ids, uint32_t n,
                         const GatherOut& o, uint32_t* bad, hipStream_t s);
// The inverse: the canonical view of the distinct groups ids[0..n), or with
// ids null of the range [first, first + n), in device buffers of the view's
// layout indexed by list position, becomes those groups' internal words
// (derived in scatter_view.hpp): what raft_load_state gives a group from the
// same rows. role, voted, term, last, commit, deadline, timeout, match, fault,
// log_term and log_value are required; log_crc, next, hwm and iso_victim may
// be null (stamps computed with payload_crc, match + 1, last, 0). The rows are
// range-checked by the host before the launch. cursors (may be null): the open
// commit feed's, [G][nm] over the replicas of mask; the listed groups' become
// min(CommitIndex, LastApplied) of the loaded rows.
struct ScatterIn {
  const uint8_t *role, *voted;
  const int32_t *term, *last, *commit, *deadline, *timeout, *match;
  const uint8_t* fault;
  const int32_t* log_term;
  const int64_t* log_value;
  const uint32_t* log_crc;
  const int32_t *next, *hwm;
  const uint8_t* iso_victim;
};
hipError_t launch_scatter(int R, const DevPlanes& P, int raft, uint32_t first, const uint32_t* ids, uint32_t n,
                          const ScatterIn& in, int32_t* cursors, uint32_t mask, uint32_t nm, hipStream_t s);
// NewNode x R (init_new_group) for the distinct groups ids[0..n); cursors (may
// be null): the open commit feed's, [G][nm], set to 0 for those groups.
hipError_t launch_restart(int R, const DevPlanes& P, const Trace& T, const uint32_t* ids, uint32_t n, int32_t* cursors,
                          uint32_t nm, hipStream_t s);
// Group audit (k_audit.hip; raft_group_audit). checks: enum raft_audit_check;
// rec: the audit's scratch, 8 B per group of the engine; the launches cover
// the 256-group blocks from the one holding `first` on, as the scan's do.
// launch_audit_scalar: every group of [first, G) gets its record (violated
// checks, the lowest one's witness, the fault code) from the scalar checks,
// one lane per group. launch_audit_log (after it, when `checks` has a log
// bit): the log checks, one wave per group, merged into the records.
// launch_audit_count: per block its hits (bsum), and tot[8 + k] += the groups
// violating check bit k (tot: 16 words, zero before the launch).
// launch_audit_emit: hits [0, cap) of the ascending group order to `out`
// (24 B each, raft_audit_hit), cap >= 1 and at most the total; *next = the
// local id after hit cap - 1.
hipError_t launch_audit_scalar(int R, const DevPlanes& P, uint32_t checks, uint32_t first, void* rec, hipStream_t s);
hipError_t launch_audit_log(int R, const DevPlanes& P, int raft, uint32_t checks, uint32_t first, void* rec,
                            hipStream_t s);
hipError_t launch_audit_count(const DevPlanes& P, uint32_t first, const void* rec, uint32_t* bsum,
                              unsigned long long* tot, hipStream_t s);
hipError_t launch_audit_emit(const DevPlanes& P, uint32_t first, const void* rec, const uint64_t* boff, uint64_t cap,
                             void* out, unsigned long long* next, hipStream_t s);
// Applied state (k_apply.hip; raft_apply_*). rec: [G][nm] records of 32 B
// (raft_apply_record), one per group and replica of `mask` (nm = its bits, in
// replica order).
// launch_apply_reset: the records of the groups ids[0..n) (ids null: groups
// [0, n)) become the FROM_START state or, with from_commit, the FROM_COMMIT
// state of the canonical view as it is.
// launch_apply_step: one step over every group, then one wave that publishes
// the totals; tot: 5 device words, zero between steps (the accumulators); res:
// 5 words of pinned host memory = folded, lost, stalled, gapped, diverged.
// launch_apply_read: out[i R + r] (32 B each) = the record of replica r of
// group ids[i] (ids null: first + i), i < n; applied = -1 and zeroes outside
// the mask.
// launch_apply_count / _emit: raft_apply_scan over the 256-group blocks from
// the one holding `first` on, as the directory's scan: per block its hits
// (bsum); hits [0, cap) of the ascending group order to `out` (24 B each,
// raft_apply_hit), cap >= 1 and at most the total, *next = the local id after
// hit cap - 1.
hipError_t launch_apply_reset(int R, const DevPlanes& P, int from_commit, const uint32_t* ids, uint32_t n, uint32_t mask,
                              uint32_t nm, void* rec, hipStream_t s);
hipError_t launch_apply_step(int R, const DevPlanes& P, int raft, uint32_t mask, uint32_t nm, void* rec,
                             unsigned long long* tot, unsigned long long* res, hipStream_t s);
hipError_t launch_apply_read(int R, const void* rec, const uint32_t* ids, uint32_t first, uint32_t n, uint32_t mask,
                             uint32_t nm, void* out, hipStream_t s);
hipError_t launch_apply_count(int R, const DevPlanes& P, const void* rec, uint32_t mask, uint32_t nm, uint32_t select,
                              uint32_t first, uint32_t* bsum, hipStream_t s);
hipError_t launch_apply_emit(int R, const DevPlanes& P, const void* rec, uint32_t mask, uint32_t nm, uint32_t select,
                             uint32_t first, const uint64_t* boff, uint64_t cap, void* out, unsigned long long* next,
                             hipStream_t s);
hipError_t launch_stream_probe(int R, const uint16_t* a, SsRec* b, const uint16_t* c, int32_t* d, int32_t* rt,
                               int64_t* rv, uint32_t n, uint32_t slot, uint32_t kslots, hipStream_t s,
                               uint32_t mode = 0);

}  // namespace raftstep
