/*
 * raftstep.h — C-ABI of the MI355X-native batched Raft step engine.
 *
 * This is the drop-in boundary for the hot path of eastwd/raft-sample:
 * the RequestVote / AppendEntries handlers and the leader commit logic of
 * main.go (FollowerRun main.go:111-180, CandidateRun main.go:193-287,
 * LeaderRun main.go:304-397). The reference has no exported API: its
 * handlers are inline `select` cases over `*Node` (main.go:14-39) and the
 * message structs (main.go:42-49, 182-191, 289-302). Each entry point below
 * names the reference code it replaces; INTEGRATION.md shows the cgo stub a
 * maintainer adds to main.go's package to call it.
 *
 * Rules of the ABI:
 *  - plain C types only; no torch / HIP types in any signature;
 *  - every function returns 0 on success or a negative errno-style code
 *    (RAFT_E*); the message is available from raft_last_error();
 *  - caller-owned host buffers are only borrowed for the duration of a call
 *    (cgo pointer rules: nothing is retained after return);
 *  - one engine = one GPU = one host thread at a time (not re-entrant).
 *
 * Semantics are the reference's ("REF") bit for bit,
 * including its quirks; where the reference would panic or deadlock the
 * group is frozen with a per-group fault code instead of killing the process.
 */
#ifndef RAFTSTEP_H
#define RAFTSTEP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAFT_ABI_VERSION 6u
#define RAFT_MAX_REPLICAS 8u

/* Node.State (main.go:51-57). */
enum raft_role { RAFT_FOLLOWER = 0, RAFT_CANDIDATE = 1, RAFT_LEADER = 2 };

/* Per-group fault codes. The reference panics or blocks forever instead;
 * the engine freezes the group from that point on (no further state change). */
enum raft_fault {
  RAFT_F_NONE = 0,
  RAFT_F_PANIC_GETLOG = 1,        /* GetLog(i) out of range: main.go:142 -> 403-405 */
  RAFT_F_DEADLOCK_VRES = 2,       /* candidate answers a VoteRequest into its own VRes: main.go:242 */
  RAFT_F_DEADLOCK_LEADER_VREQ = 3,/* leader has no VReq case: main.go:308-332 */
  RAFT_F_RING_EVICTED = 4,        /* EXT: entry older than the ring depth K was needed */
  RAFT_F_OVERFLOW = 5             /* EXT: a term/index would leave int32 (Go int is 64-bit) */
};
/* RAFT_F_OVERFLOW, the one value that does not fit. Terms and log indices
 * reach 2^31-1; NextIndex = MatchIndex + 1 can be 2^31.
 *   REF derives NextIndex at every use and compares it in 64 bits, as Go
 *   does: a leader with MatchIndex 2^31-1 sends heartbeats with PrevLogIndex
 *   2^31-1, no fault.
 *   RAFT stores NextIndex as int32. An assignment that would store 2^31
 *   freezes the group with RAFT_F_OVERFLOW at that assignment: winning an
 *   election at LastApplied 2^31-1 (the votes stay granted, the candidate
 *   stays a candidate, no row is written), and next = match + 1 after a
 *   success at match 2^31-1 (the follower keeps what it appended, the
 *   leader's rows and counters keep their values, later peers are not
 *   reached). raft_load_state refuses (RAFT_EINVAL) a RAFT leader row whose
 *   NextIndex is absent and whose MatchIndex is 2^31-1. */

/* REF = main.go bit for bit (the drop-in). RAFT = EXT mode with the
 * Raft-paper rules (votedFor, up-to-date check, truncate-on-conflict,
 * nextIndex backoff, majority commit with the current-term rule) on the same
 * tick model and layout, for churn workloads where REF faults (config C4). */
enum raft_semantics { RAFT_SEM_REF = 0, RAFT_SEM_RAFT = 1 };

/* Error codes (negative returns). */
#define RAFT_OK 0
#define RAFT_EINVAL (-22)
#define RAFT_ENOMEM (-12)
#define RAFT_ERANGE (-34)
#define RAFT_ETIMEDOUT (-110) /* a communicator did not complete in time (RAFTSTEP_COMM_TIMEOUT_S) */
#define RAFT_ENODEV (-19)
#define RAFT_EHIP (-1000)
#define RAFT_ERCCL (-2000)
#define RAFT_EINTERNAL (-3000)  /* an engine invariant failed its run-time check (a bug: report it) */

/* Statistics of one or more ticks (summed over groups, and over GPUs once a
 * communicator is attached). Index names: */
enum raft_stat {
  RAFT_STAT_COMMITTED = 0,      /* sum of leader CommitIndex advances (main.go:389) */
  RAFT_STAT_ELECTIONS_WON = 1,  /* candidate -> leader (main.go:273-282) */
  RAFT_STAT_TERM_BUMPS = 2,     /* election timeouts, Term++ (main.go:176, 250) */
  RAFT_STAT_AE_OK = 3,          /* AppendEntries answered Success:true */
  RAFT_STAT_AE_FAIL = 4,        /* AppendEntries answered false (or dropped, EXT) */
  RAFT_STAT_VOTES_GRANTED = 5,  /* VoteResponse vote:true */
  RAFT_STAT_FAULTS = 6,         /* groups that faulted during the tick(s) */
  RAFT_STAT_LEADER_GROUPS = 7,  /* groups with >=1 leader at the end of each tick (summed over ticks) */
  RAFT_NSTATS = 8
};
typedef struct raft_tick_stats { int64_t v[RAFT_NSTATS]; } raft_tick_stats;

/* Engine configuration. Zero-initialise, then set fields; see
 * raft_config_default(). Virtual time: one tick = tick_seconds virtual
 * seconds (the leader heartbeat period, main.go:394). */
typedef struct raft_config {
  uint32_t abi_version;        /* = RAFT_ABI_VERSION */
  uint32_t replicas;           /* R = len(Nodes), 1..8 (main.go:81 uses 3) */
  uint64_t groups;             /* independent Raft groups on this engine */
  uint64_t group_base;         /* global id of local group 0 (sharding across GPUs) */
  uint32_t ring_depth;         /* K: log entries kept per replica, power of two */
  uint32_t entries_per_tick;   /* E: client entries appended per client event (main.go:92) */
  uint32_t client_period;      /* ticks between client events; 0 = no client */
  uint32_t semantics;          /* enum raft_semantics */
  uint64_t seed;               /* trace seed (splitmix64 counter RNG) */
  int32_t tick_seconds;        /* 2 (main.go:394) */
  int32_t follower_timeout_min;   /* 10 s  (main.go:114: rand.Intn(20)+10) */
  int32_t follower_timeout_span;  /* 20    */
  int32_t candidate_timeout_min;  /* 10 s  (main.go:194: rand.Intn(4)+10) */
  int32_t candidate_timeout_span; /* 4     */
  uint32_t isolate_per_65536;  /* EXT: probability (x/65536) per 32-tick epoch that one replica is isolated */
  uint32_t isolate_min_ticks;  /* EXT: isolation length range, 1..32 */
  uint32_t isolate_max_ticks;
  int32_t device;              /* HIP device ordinal */
  uint32_t payload_crc;        /* EXT (config C5): stamp every entry with CRC32C(term||value), followers verify */
  uint32_t corrupt_per_65536;  /* EXT: probability that an AppendEntries' last entry arrives with a flipped bit */
  uint32_t isolate_leader;     /* EXT: 1 = an isolation window cuts off the group's leader at the window's first
                                  tick (the lowest-id Leader then; no leader: nobody), 0 = a hashed replica */
  uint32_t ticks_per_launch;   /* 1 (default; 0 reads as 1): one tick per kernel launch, every group's state read
                                  from and written back to HBM every tick (the metric's form).
                                  2..64: while the steady-state list skip holds (no isolation, no CRC), up to this
                                  many steady ticks run in one launch of the fused kernel (state kept in registers
                                  between them; results identical, not the §8(d) form) */
  uint32_t debug_flags;        /* RAFT_DEBUG_*; 0 in production */
  uint32_t client_source;      /* enum raft_client_source: where the client's values (main.go:92) come from */
  uint32_t reserved[2];        /* must be 0 */
} raft_config;

/* raft_config.client_source. The reference's client sends rand.Int() to
 * every node whose State is Leader (main.go:87-93 -> LogReq -> 327-329).
 *  RAFT_CLIENT_TRACE  (0): the values come from the seeded trace RNG on the
 *      device (splitmix64 keyed by seed, group, replica, tick, entry);
 *  RAFT_CLIENT_STAGED (1): the caller supplies them. Before raft_tick runs
 *      ticks [t0, t0+n) the caller stages n x E x G int64 values with
 *      raft_stage_values; every Leader of group g at tick t appends
 *      values[((t - t0) * E + e) * G + g] as its e-th entry of that tick (one
 *      client request per group and entry, sent to whichever replicas are
 *      leaders, like main.go:90-93). The engine never regenerates an entry in
 *      this mode: entries are read from the staged buffer when appended and
 *      from the rings afterwards. */
enum raft_client_source { RAFT_CLIENT_TRACE = 0, RAFT_CLIENT_STAGED = 1 };

/* raft_config.debug_flags */
#define RAFT_DEBUG_ALLOW_WRONG_RESULTS 1u  /* accept the timing-only environment knob RAFTSTEP_DIAG_LEAN, whose modes
                                              skip work and make results WRONG; without this flag
                                              raft_engine_create refuses it (RAFT_EINVAL) */

/* Canonical host view of engine state, group-major:
 *   per-replica arrays are indexed [g*R + r], match is [(g*R + leader)*R + peer],
 *   log arrays are [(g*R + r)*K + slot] where log index i (1-based) lives at
 *   slot (i-1) mod K and only i in (max(0,hwm-K), last] is meaningful (other
 *   slots read back as 0). match rows of replicas that are not leaders read
 *   back as 0. Any pointer may be NULL on store (field skipped). */
typedef struct raft_state_view {
  uint8_t* role;      /* Node.State (main.go:16) */
  uint8_t* voted;     /* REF: Node.Voted (main.go:20); RAFT: votedFor + 1 (0 = none) */
  int32_t* term;      /* Node.Term (main.go:19) */
  int32_t* last;      /* Node.LastApplied == len(Node.Log) (main.go:25, 148-149, 328-329) */
  int32_t* commit;    /* Node.CommitIndex (main.go:24) */
  int32_t* deadline;  /* election timer deadline, virtual seconds */
  int32_t* timeout;   /* current timer duration d, seconds (main.go:114, 194). A load accepts 0..1023 (the
                       * 10-bit duration field; the configured ranges end at min + span <= 1024) and
                       * refuses anything else with RAFT_EINVAL. 0, which no configured range draws, is a
                       * timer that a reset at `now` leaves at deadline == now: the same tick's timer step
                       * fires it, so a follower with timeout 0 stands for election in the tick of every
                       * heartbeat or vote that resets it, until a new role draws it a duration */
  int32_t* match;     /* Node.MatchIndex (main.go:29); NextIndex == MatchIndex+1 (main.go:280-281, 376-377) */
  uint8_t* fault;     /* per group, enum raft_fault */
  int32_t* log_term;  /* Log.Term (main.go:47) */
  int64_t* log_value; /* Log.Value (main.go:48) */
  uint32_t* log_crc;  /* EXT: CRC32C of each ring entry (0 when payload_crc is off) */
  int32_t* next;      /* Node.NextIndex [(g*R + leader)*R + peer] (REF: match+1); 0 for non-leaders.
                         Optional on load: absent or 0 derives match+1 (REF ignores it).
                         REF with match == 2^31-1: the derived value is 2^31, and the view and the
                         digest carry its low 32 bits (INT32_MIN); see RAFT_F_OVERFLOW */
  int32_t* hwm;       /* [g*R + r] highest LastApplied ever (== last in REF); the ring holds (hwm-K, last].
                         Optional on load: absent or < last means last (REF ignores it) */
  uint8_t* iso_victim;/* per group, EXT leader-isolation mode: victims of the windows in flight, one nibble
                         per epoch parity (8 | replica, 0 = none). Optional on load (absent: 0) */
} raft_state_view;

typedef struct raft_engine raft_engine;

/* ---- lifecycle ---------------------------------------------------------- */
void raft_config_default(raft_config* cfg);
int raft_engine_create(const raft_config* cfg, raft_engine** out);
int raft_engine_destroy(raft_engine* e);
const char* raft_last_error(void);              /* thread-local message of the last failure */
int raft_engine_info(const raft_engine* e, raft_config* cfg_out, uint64_t* device_bytes);
/* Storage forms this engine uses (bit set = on; results are identical either
 * way): RAFT_FEATURE_SHARED_ENTRIES — the steady kernels store the entries
 * every replica of an in-step group holds alike once (shared ring, copied
 * back into the replica rings before any other reader); RAFT_FEATURE_
 * VIRTUAL_SUFFIXES — a cut-off leader's own entries are regenerated instead
 * of stored (RAFT leader isolation). */
#define RAFT_FEATURE_SHARED_ENTRIES 1u
#define RAFT_FEATURE_VIRTUAL_SUFFIXES 2u
int raft_engine_features(const raft_engine* e, uint32_t* flags);

/* NewNode x R for every group (main.go:59-76) followed by FollowerRun entry
 * (timer drawn, main.go:113-115) at virtual tick `tick0`. */
int raft_init_new_nodes(raft_engine* e, int64_t tick0);
/* Post-election state (KAT-1 generalised): replica `leader` (or a per-group
 * hashed replica when leader < 0) is Leader with Term 1, the others are
 * Followers with Term 1 and Voted, MatchIndex 0 / NextIndex 1, empty logs. */
int raft_init_steady(raft_engine* e, int32_t leader, int64_t tick0);

int raft_load_state(raft_engine* e, const raft_state_view* v);
int raft_store_state(raft_engine* e, raft_state_view* v);
/* The canonical view of groups [first_group, first_group + n_groups) only,
 * indexed by the local group (g - first_group) with the same per-group shapes
 * as raft_store_state; the view of that slice alone is derived on the device
 * and copied out (as for raft_store_state and raft_store_groups), so a slice
 * of a multi-million-group engine can be compared with a CPU run of the same
 * groups (RAFT_ERANGE when the range leaves the engine). */
int raft_store_state_range(raft_engine* e, uint64_t first_group, uint64_t n_groups, raft_state_view* v);

/* ---- audit: digests, nodelog, checkpoints ---------------------------------
 * raft_state_digest: per-group 64-bit digest of the canonical view that
 * raft_store_state would return (splitmix64 chain keyed by the global group
 * id; words listed in oracle/raft_oracle.c oracle_state_digest), computed on
 * the device without copying the state out. `per_group` (u64[groups], may be
 * NULL) receives the digests, `total` (may be NULL) their wrapping sum, which
 * is independent of how groups are sharded over engines. */
int raft_state_digest(raft_engine* e, uint64_t* per_group, uint64_t* total);
/* nodelog (main.go:399-401) lines of every replica of one group:
 * "[Server<r>:<Term>:<CommitIndex>:<LastApplied>][<state>]\n". Returns the
 * number of bytes written (NUL-terminated when it fits) or a negative code;
 * RAFT_ERANGE if `cap` is too small. */
int raft_nodelog(raft_engine* e, uint64_t group, char* buf, size_t cap);
/* Checkpoint = the canonical view of every group plus the engine's config,
 * written to / read from a file (header + fields + CRC32C trailer). The
 * persistent Node fields of main.go:18-21 (Term, Voted, Log) and the volatile
 * ones (22-29) survive a save/load round trip bit for bit. Loading checks
 * replicas / groups / ring depth / semantics / payload_crc against the
 * engine's config (RAFT_EINVAL on mismatch, on a bad magic/version or CRC). */
int raft_checkpoint_save(raft_engine* e, const char* path);
int raft_checkpoint_load(raft_engine* e, const char* path);

/* ---- the tick (the metric path) -----------------------------------------
 * Advances every group by `nticks` ticks starting at virtual tick
 * `first_tick`. One tick per kernel launch (config.ticks_per_launch = 1, the
 * default; see there for the fused steady form); per tick and group, in order:
 *   1. client append to leaders (main.go:87-93 -> 327-329),
 *   2. replicas in ascending id: leader replication round + commit
 *      (main.go:332-391) / candidate vote round (main.go:253-284), every
 *      message delivered through the receiver's handler,
 *   3. election timers that expired, in (deadline, id) order, each followed
 *      at once by the new candidate's vote round (main.go:171-177, 248-251).
 * `out` (may be NULL) receives the stats summed over the ticks. */
int raft_tick(raft_engine* e, int64_t first_tick, uint32_t nticks, raft_tick_stats* out);
/* RAFT_CLIENT_STAGED engines: the client values of ticks [first_tick,
 * first_tick + nticks), laid out [nticks][E][G] int64 (E = entries_per_tick,
 * G = groups of this engine, indexed by the local group; the value stream of
 * main.go:92, one request per group, tick and entry, LogReq at main.go:327-329).
 * Copied into HBM (the host buffer is only borrowed for the call); replaces
 * whatever was staged before. raft_tick then accepts calls whose ticks lie
 * inside the staged range (RAFT_EINVAL otherwise). RAFT_EINVAL on a
 * RAFT_CLIENT_TRACE engine. */
int raft_stage_values(raft_engine* e, int64_t first_tick, uint32_t nticks, const int64_t* values);
/* Per-tick statistics of the last raft_tick call that asked for stats: record
 * t (0 <= t < nticks of that call) holds tick first_tick+t, summed over groups
 * and, with a communicator, over GPUs (the 64-B record the all-reduce carries). */
int raft_tick_records(raft_engine* e, uint32_t nticks, raft_tick_stats* per_tick);
int raft_sync(raft_engine* e);

/* ---- message-level handlers (drop-in for the select cases) --------------
 * Batched: element i is applied to group reqs[i].group; all groups of one
 * batch must be distinct (RAFT_EINVAL otherwise). `now_tick` is the virtual
 * time used for timer resets / redraws. */
typedef struct raft_log_entry { int64_t term; int64_t value; } raft_log_entry; /* Log (main.go:46-49) */

typedef struct raft_ae_req {     /* AppendEntriesRequest (main.go:289-296) */
  uint64_t group;
  uint32_t to;                   /* receiving replica */
  uint32_t leader_id;            /* LeaderId (routing only) */
  int64_t term;                  /* Term */
  int64_t prev_log_index;        /* PrevLogIndex */
  int64_t prev_log_term;         /* PrevLogTerm */
  int64_t leader_commit;         /* LeaderCommit */
  uint64_t entries_offset;       /* Logs = entries[entries_offset .. +n_entries) */
  uint64_t n_entries;
} raft_ae_req;
typedef struct raft_ae_resp {    /* AppendEntriesResponse (main.go:298-302) */
  int64_t term;
  int64_t match_index;
  int32_t success;
  int32_t fault;                 /* enum raft_fault raised while handling (0 = none) */
} raft_ae_resp;
/* FollowerRun case AEReq (main.go:121-156), CandidateRun case AEReq
 * (main.go:200-223), LeaderRun case AEReq (main.go:309-326), dispatched on
 * the receiver's State like Run (main.go:98-109). */
int raft_append_entries_batch(raft_engine* e, int64_t now_tick, const raft_ae_req* reqs, size_t n,
                              const raft_log_entry* entries, size_t n_entries_total, raft_ae_resp* out);

typedef struct raft_vote_req {   /* VoteRequest (main.go:182-187) */
  uint64_t group;
  uint32_t to;
  uint32_t candidate_id;         /* CandidateId (routing only) */
  int64_t term;
  int64_t last_log_index;        /* never read by the reference (main.go:185-186, 264) */
  int64_t last_log_term;
} raft_vote_req;
typedef struct raft_vote_resp {  /* VoteResponse (main.go:188-191) */
  int64_t term;
  int32_t vote_granted;
  int32_t fault;
} raft_vote_resp;
/* FollowerRun case VReq (main.go:157-170), CandidateRun case VReq
 * (main.go:224-246); a leader has no VReq case (main.go:308) -> fault. */
int raft_request_vote_batch(raft_engine* e, int64_t now_tick, const raft_vote_req* reqs, size_t n,
                            raft_vote_resp* out);

/* Whole-node steps, batched over distinct groups. LEADER_ROUND and
 * CANDIDATE_ROUND honour the config's EXT isolation windows at now_tick
 * (messages to or from an isolated replica are dropped), like raft_tick. */
enum raft_op_kind {
  RAFT_OP_CLIENT_APPEND = 1,   /* LeaderRun case LogReq (main.go:327-329); arg = Value */
  RAFT_OP_LEADER_ROUND = 2,    /* LeaderRun default: AE to each peer + commit (main.go:332-391) */
  RAFT_OP_CANDIDATE_ROUND = 3, /* CandidateRun default: vote round + tally (main.go:253-284) */
  RAFT_OP_TIMEOUT = 4,         /* timer.C: follower -> candidate / candidate Term++ (main.go:171-177, 248-251) */
  RAFT_OP_LEADER_COMMIT = 5    /* commit rule alone (main.go:381-391) */
};
typedef struct raft_group_op {
  uint64_t group;
  uint32_t replica;
  uint32_t kind;
  int64_t arg;
} raft_group_op;
typedef struct raft_op_result {
  int32_t status;   /* 0 applied; RAFT_EINVAL if the replica's State does not run this step */
  int32_t fault;    /* group fault code after the op */
  int64_t value;    /* CommitIndex after LEADER_ROUND/LEADER_COMMIT; 1 if elected by CANDIDATE_ROUND */
} raft_op_result;
int raft_group_ops_batch(raft_engine* e, int64_t now_tick, const raft_group_op* ops, size_t n,
                         raft_op_result* out);

/* ---- commit feed ----------------------------------------------------------
 * The way out of the log: every entry a replica has committed, handed over
 * once and in order, to apply or to acknowledge (main.go:330: "this is where
 * the leader should answer the client once CommitIndex has advanced"; the
 * CommitIndex updates at main.go:151-153 and 387-390). The device keeps one
 * int32 cursor per (group, replica of the mask) from raft_feed_open to
 * raft_feed_close / raft_engine_destroy; an engine without an open feed
 * allocates nothing for it.
 *
 * A poll treats one pair with cursor c, CommitIndex cm, LastApplied l and
 * high-water mark h (REF: h = l; ring depth K) like this:
 *   hi = min(cm, l)           (a REF follower's CommitIndex may be l+1,
 *                              main.go:152: that entry is delivered once it exists)
 *   hi < c:  the pair is counted in `stalled` and left alone (a cursor never
 *            moves backwards: a pair's stream is strictly increasing in index)
 *   else     lo = min(max(c, h - K), hi); the lo - c entries that have left
 *            the ring are counted in `lost` and skipped whatever `cap` is;
 *            entries lo+1 .. hi are deliverable.
 * The deliverable entries of all pairs, ordered by (group, replica, index),
 * are cut at `cap`: the first `cap` are written to `out` and the cursors
 * advance by exactly what was written (a pair may be cut in the middle).
 * info->delivered is that number, info->pending the deliverable entries left.
 * cap = 0 (out may then be NULL) only counts. The same state and cursors
 * give the same bytes. Faulted groups are read like any other. */
typedef struct raft_feed_entry {   /* 32 B */
  uint64_t group;     /* global id: config.group_base + local group */
  uint32_t replica;
  int32_t  index;     /* 1-based log index */
  int32_t  term;      /* Log.Term  (main.go:47) */
  uint32_t crc;       /* the entry's CRC32C stamp; 0 when payload_crc is off */
  int64_t  value;     /* Log.Value (main.go:48) */
} raft_feed_entry;
typedef struct raft_feed_info { uint64_t delivered, pending, lost, stalled; } raft_feed_info;
/* Where the cursors start: at 0, at the current min(CommitIndex, LastApplied)
 * (only what commits from now on), or at the caller's array ([G][R] int32,
 * read for the replicas of the mask, none negative; what raft_feed_cursors
 * returned resumes a feed exactly). */
enum raft_feed_start { RAFT_FEED_FROM_START = 0, RAFT_FEED_FROM_COMMIT = 1, RAFT_FEED_FROM_CURSORS = 2 };
/* replica_mask: bit r = replica r is fed (RAFT_EINVAL when 0 or with bits at
 * or above R). Opening an open feed replaces it. */
int raft_feed_open(raft_engine* e, uint32_t replica_mask, uint32_t start, const int32_t* cursors);
/* RAFT_EINVAL without an open feed. Handler batches and raft_tick leave the
 * feed open (and a poll leaves the steady tick's forms alone); whatever
 * replaces the state (raft_init_*, raft_load_state, raft_checkpoint_load)
 * closes it. No collective: each engine feeds its own shard. */
int raft_feed_poll(raft_engine* e, raft_feed_entry* out, uint64_t cap, raft_feed_info* info);
/* The cursors, [G][R] int32; -1 for replicas outside the mask. */
int raft_feed_cursors(raft_engine* e, int32_t* out);
int raft_feed_close(raft_engine* e);   /* (no open feed: nothing to do) */

/* ---- client proposals -----------------------------------------------------
 * The way into the log for a caller that owns its own requests: a list of
 * (group, value) per call, several for hot groups and none for cold ones
 * (main.go:87-93 sends each LogReq to every node that is Leader), a ticket per
 * request with the index and term its entry received, and a cheap read-only
 * question about outstanding tickets (main.go:330: the leader answers the
 * client once CommitIndex has advanced). The commit feed delivers what was
 * committed; raft_ticket_status also says that a ticket never will be.
 *
 * raft_propose(now_tick, props[0..n), out[0..n)): out[i] is the ticket of
 * props[i]. Rules:
 *   Proposals are applied in list order. A group may appear any number of
 *     times; its k-th proposal sees the state its (k-1)-th left. Different
 *     groups are independent.
 *   One proposal for group g:
 *     g frozen (fault code not 0): RAFT_PROPOSE_FROZEN, nothing appended,
 *       leader 0xFF, leaders 0.
 *     Otherwise every replica whose State is Leader, in ascending id, runs
 *       LogReq (main.go:327-329): exactly what RAFT_OP_CLIENT_APPEND does to
 *       one replica (the entry's Term = the Leader's Term, the value, with
 *       payload_crc its stamp; LastApplied + 1; RAFT: the high-water mark).
 *     An append that would leave int32 (LastApplied == 2^31-1) freezes the
 *       group with RAFT_F_OVERFLOW at that append: later Leaders of this
 *       proposal append nothing, nor do later proposals of the group.
 *     RAFT_PROPOSE_ACCEPTED <=> the lowest-id Leader appended <=> leaders != 0;
 *       index and term are that Leader's. With leaders == 0 the status is
 *       RAFT_PROPOSE_FROZEN when the group is frozen after the proposal (the
 *       lowest-id Leader's append overflowed), RAFT_PROPOSE_NO_LEADER otherwise
 *       (no replica is Leader).
 *     fault is the group's code after the proposal in every case (ACCEPTED
 *       with fault 5: a higher-id Leader's append overflowed).
 *   n = 0 changes nothing, and the steady tick's forms stay.
 *   Every argument error is found before anything is written: a NULL argument
 *     (with n > 0) or n > 2^31 is RAFT_EINVAL, an id >= G is RAFT_ERANGE, a
 *     now_tick that is negative or leaves int32 seconds is RAFT_ERANGE.
 *   A poisoned engine answers RAFT_EINTERNAL.
 *   Allowed with any client_source and any client_period (the proposals are in
 *     addition to whatever the ticks append).
 *   The call takes the handler batches' route: like one, it ends the steady
 *     tick's list skip and steady form until the next raft_init_steady. An
 *     open feed stays open and no cursor moves: logs only grow. */
typedef struct raft_proposal { uint64_t group; int64_t value; } raft_proposal;   /* 16 B; group = local id */
enum raft_propose_status { RAFT_PROPOSE_NONE = 0, RAFT_PROPOSE_ACCEPTED = 1,
                           RAFT_PROPOSE_NO_LEADER = 2, RAFT_PROPOSE_FROZEN = 3 };
typedef struct raft_ticket {          /* 32 B */
  uint64_t group;    /* global id: config.group_base + local */
  int64_t  value;    /* the proposal's value, echoed */
  uint32_t local;
  int32_t  index;    /* 1-based log index the entry got at the lowest-id Leader; 0 unless ACCEPTED */
  int32_t  term;     /* that Leader's Term = the entry's Log.Term; 0 unless ACCEPTED */
  uint8_t  status;   /* enum raft_propose_status */
  uint8_t  leader;   /* the lowest-id replica that appended, 0xFF: none */
  uint8_t  leaders;  /* mask of the replicas that appended (main.go:90-93 sends to every Leader) */
  uint8_t  fault;    /* the group's fault code after this proposal */
} raft_ticket;
int raft_propose(raft_engine* e, int64_t now_tick, const raft_proposal* props, uint64_t n, raft_ticket* out);
/* raft_ticket_status(tickets[0..n), out, info): read-only and stateless, on
 * the canonical view; K, top_r, lo_r, "live" and entry equality are the group
 * audit's (below). Rules:
 *   A ticket with status != RAFT_PROPOSE_ACCEPTED or index <= 0 is
 *     RAFT_TICKET_INVALID: replica 0xFF, masks 0 (raft_propose's output can be
 *     passed back as it is).
 *   Otherwise replica r (l = last_r, cm = commit_r) is
 *     absent   when index > l;
 *     gone     when index <= l and index < lo_r (the entry has left the ring);
 *     same or other when the entry is live (lo_r <= index <= l), by comparing
 *              its Term and Value with the ticket's;
 *     decided  when index <= min(cm, l).
 *   The result is the first of these that applies:
 *     1. some replica is decided and live: the lowest-id such replica is the
 *        witness; RAFT_TICKET_COMMITTED if it is same, else _SUPERSEDED;
 *     2. some replica is decided and gone: RAFT_TICKET_EVICTED, 0xFF (the
 *        outcome can no longer be read from the rings);
 *     3. some replica is same: RAFT_TICKET_PENDING, the lowest-id holder;
 *     4. some replica is gone: RAFT_TICKET_EVICTED, 0xFF;
 *     5. RAFT_TICKET_DROPPED, 0xFF: no replica holds the entry and no
 *        committed prefix reaches an entry that is still readable. Final.
 *   holders and committed are filled in every state but INVALID; fault is the
 *     group's code now in every state.
 *   info->per_state[k] = the tickets in state k. Tickets come in any order,
 *     repeats allowed. out may be NULL (only counts); info may be NULL when
 *     out is not; both NULL with n > 0, NULL tickets with n > 0 or n > 2^31 is
 *     RAFT_EINVAL. local >= G is RAFT_ERANGE; group != group_base + local is
 *     RAFT_EINVAL (another shard's ticket); nothing is written in either case.
 *   The call reads as raft_group_scan does: no group leaves its shared form,
 *     the steady tick's forms stay, the feed is left alone, frozen groups are
 *     read like any other. The same state and tickets give the same bytes. A
 *     poisoned engine answers RAFT_EINTERNAL. */
enum raft_ticket_state { RAFT_TICKET_COMMITTED = 0, RAFT_TICKET_SUPERSEDED = 1, RAFT_TICKET_PENDING = 2,
                         RAFT_TICKET_EVICTED = 3, RAFT_TICKET_DROPPED = 4, RAFT_TICKET_INVALID = 5 };
typedef struct raft_ticket_result {   /* 8 B */
  uint8_t state;      /* enum raft_ticket_state */
  uint8_t replica;    /* witness, 0xFF where the state names none */
  uint8_t fault;      /* the group's fault code now */
  uint8_t holders;    /* mask: replicas whose live entry at index equals (term, value) */
  uint8_t committed;  /* mask: holders with index <= min(CommitIndex, LastApplied) */
  uint8_t reserved[3];/* 0 */
} raft_ticket_result;
typedef struct raft_ticket_info { uint64_t per_state[8]; } raft_ticket_info;  /* [6], [7] are 0 */
int raft_ticket_status(raft_engine* e, const raft_ticket* tickets, uint64_t n, raft_ticket_result* out,
                       raft_ticket_info* info);

/* ---- group directory ------------------------------------------------------
 * The way out of the fault codes, and the way back in: find groups by what is
 * wrong with them, read the canonical view of a list of groups, and restart
 * single groups (what an operator of the Go program does to a process that
 * panicked). The scan and the store read the state on the device as
 * raft_state_digest does: they take no group out of its shared form, keep the
 * steady tick's forms and leave an open feed alone.
 *
 * raft_group_scan: a group g in [first_group, G) (local ids) is a hit when
 *   select & RAFT_SELECT_FAULTED    and its fault code is not 0, or
 *   select & RAFT_SELECT_LEADERLESS and its fault code is 0 and no replica's
 *                                   State is Leader (a live group waiting for
 *                                   an election; a frozen group is never
 *                                   reported as leaderless).
 * Hits come in ascending group order; the first `cap` are written to `out`
 * (cap = 0 only counts, out may then be NULL). info->matched = every hit in
 * the range, info->written = min(cap, matched), info->next_group = the local
 * id after the last hit written, G when nothing is left (written == matched),
 * first_group when nothing was written and hits are left (cap = 0): a caller
 * pages with first_group = next_group. The same state gives the same bytes.
 * RAFT_EINVAL: select 0 or with unknown bits, cap > 0 without out;
 * RAFT_ERANGE: first_group > G (first_group == G is an empty scan). */
enum raft_group_select { RAFT_SELECT_FAULTED = 1u, RAFT_SELECT_LEADERLESS = 2u };
typedef struct raft_group_hit {   /* 16 B */
  uint64_t group;     /* global id: config.group_base + local */
  uint32_t local;     /* what every batch call and the two calls below take */
  uint8_t  fault;     /* enum raft_fault */
  uint8_t  leader;    /* lowest-id replica whose State is Leader, 0xFF: none */
  uint16_t reserved;  /* 0 */
} raft_group_hit;
typedef struct raft_scan_info { uint64_t matched, written, next_group; } raft_scan_info;
int raft_group_scan(raft_engine* e, uint32_t select, uint64_t first_group, raft_group_hit* out, uint64_t cap,
                    raft_scan_info* info);
/* The canonical view of groups[0..n) (local ids, in any order, repeats
 * allowed), indexed by the list position i with the per-group shapes of
 * raft_store_state_range and byte-identical to the rows raft_store_state
 * returns for those groups; NULL fields are skipped. n = 0 is a no-op; an id
 * >= G is RAFT_ERANGE with nothing written. */
int raft_store_groups(raft_engine* e, const uint64_t* groups, uint64_t n, raft_state_view* v);
/* NewNode (main.go:59-76) for every replica of each listed group followed by
 * the FollowerRun entry at virtual tick `tick0` (main.go:113-115): exactly what
 * raft_init_new_nodes(tick0) writes for that group (the Go node keeps nothing
 * on disk: term 0, no vote, empty logs, timers drawn from the trace RNG by the
 * global id and tick0, fault and isolation record 0). Every other group is
 * untouched, bit for bit. Ids must be distinct (RAFT_EINVAL) and < G
 * (RAFT_ERANGE); any error leaves the state as it was, n = 0 changes nothing.
 * Like a handler batch, a restart ends the steady tick's list skip and steady
 * form until the next raft_init_steady. An open feed stays open: every fed
 * cursor of a restarted group becomes 0, the others do not move. */
int raft_restart_groups(raft_engine* e, const uint64_t* groups, uint64_t n, int64_t tick0);
/* The inverse of raft_store_groups: *v is the canonical view of groups[0..n)
 * (local ids), indexed by the list position i with the per-group shapes of
 * raft_store_groups, so what raft_store_groups(ids, n, &v) wrote can be passed
 * back as it is (the rows of a checkpoint, a repaired row, a hand-made state).
 * Fields: exactly raft_load_state's. role, voted, term, last, commit,
 *   deadline, timeout, match, fault, log_term and log_value are required (no
 *   partial patching: a missing one is RAFT_EINVAL); log_crc, next, hwm and
 *   iso_victim are optional with the same derivations: an absent log_crc on a
 *   payload_crc engine is stamped from (term, value), an absent or 0 next is
 *   match + 1, an absent hwm or hwm < last is last, an absent iso_victim is 0.
 * Validation: every listed row passes raft_load_state's range checks (fault
 *   code; iso_victim nibbles 0 or 8 | replica < R; role <= Leader; voted <= 1
 *   in REF, <= R in RAFT; last >= 0; timeout in 0..1023; RAFT: no derived
 *   NextIndex of MatchIndex 2^31-1, last entry inside (hwm - K, hwm]); the
 *   message names the list element and the group. Ids must be distinct
 *   (RAFT_EINVAL) and < G (RAFT_ERANGE).
 * Every argument error is found before anything is written: an error leaves
 *   the state, the steady tick's forms and the feed as they were. n = 0
 *   changes nothing. A poisoned engine answers RAFT_EINTERNAL.
 * A listed group then holds exactly the state raft_load_state would give it
 *   from the same rows: its canonical view and digest equal those of an
 *   engine that loaded the whole view with these rows spliced in (it continues
 *   on its own global id's trace). Every other group is untouched, bit for
 *   bit, view and digest. The rows' timers are on the engine's own virtual
 *   clock (as for raft_load_state): a timer start, deadline - timeout, after
 *   the time of the engine's next tick outlives later heartbeats, since the
 *   engine keeps the later of the two.
 * Like a restart or a handler batch, the call ends the steady tick's list
 *   skip and steady form until the next raft_init_steady. An open feed stays
 *   open: every fed cursor of a loaded group becomes min(CommitIndex,
 *   LastApplied) of that replica's loaded row (the restart's rule and
 *   RAFT_FEED_FROM_COMMIT's, so the pair is never left stalled); the others
 *   do not move.
 * raft_load_state and raft_checkpoint_load write the state through the same
 * device scatter, over every group (and, replacing the state, close the feed). */
int raft_load_groups(raft_engine* e, const uint64_t* groups, uint64_t n, const raft_state_view* v);

/* ---- group audit ----------------------------------------------------------
 * Is the state the engine holds a correct Raft state? A read-only device pass
 * that evaluates six safety invariants per group on the canonical view and
 * reports the violating groups, each with a witness: the operator's look at a
 * whole cluster (main.go:399-401 nodelog prints one node), and the one place
 * where a CRC32C is recomputed from the entry bytes that sit in device memory.
 * It reads the state as raft_group_scan does: no group leaves its shared
 * form, the steady tick's forms stay, an open feed is left alone. Frozen
 * groups are audited like any other.
 *
 * For replica r of a group (K = ring_depth):
 *   top_r = max(hwm_r, last_r)           (REF: last_r)
 *   lo_r  = max(1, top_r - K + 1)
 *   the live indices of r are lo_r .. last_r (none when last_r < lo_r);
 *   the common window of a pair a < b is max(lo_a, lo_b) .. min(last_a, last_b);
 *   two entries are equal when Term and Value are equal (stamps are not compared);
 *   "smallest pair" is the lexicographically smallest (a, b).
 * The checks (witness: a, b, index of the record):
 *   RAFT_AUDIT_TWO_LEADERS        replicas a < b are both Leader with equal Term
 *       (election safety). Witness: the smallest pair, index = that Term.
 *   RAFT_AUDIT_LOG_MATCHING       a pair has i <= j in its common window with
 *       log_term_a[j] == log_term_b[j] and the entries at i unequal: its smallest
 *       unequal index is <= its largest index with equal terms (log matching).
 *       Witness: the smallest violating pair, index = its smallest unequal index.
 *   RAFT_AUDIT_COMMIT_DIVERGED    a pair's smallest unequal index in the common
 *       window is <= min(commit_a, commit_b) (committed prefixes agree).
 *       Witness: the smallest violating pair and that index.
 *   RAFT_AUDIT_TERM_ORDER         a replica has a live i > lo_r with
 *       log_term[i] < log_term[i-1], or log_term[last_r] > term_r with a
 *       non-empty window. Witness: the smallest such replica, b = 0xFF, index =
 *       the smallest such i, last_r where there is none.
 *   RAFT_AUDIT_STAMP              payload_crc engines: a live entry's stamp
 *       differs from CRC32C(Term 4 B LE || Value 8 B LE), recomputed from the
 *       stored term and value. Witness: the smallest such replica, b = 0xFF, the
 *       smallest index. Without payload_crc the check is accepted and never violated.
 *   RAFT_AUDIT_COMMIT_BEYOND_LOG  commit_r > last_r. REF follows the reference
 *       here: a follower sets CommitIndex = min(LeaderCommit, LastApplied + 1)
 *       (main.go:152), so last + 1 is a legal REF state the audit makes visible
 *       (the commit feed waits for that entry); in RAFT it is a violation.
 *       Witness: the smallest such replica, b = 0xFF, index = commit_r.
 * Only the requested checks are evaluated. A group with at least one violated
 * check is a hit; hits come in ascending group order and `cap`, info->matched,
 * written and next_group follow raft_group_scan's contract (cap = 0 only
 * counts, out may then be NULL; next_group = the local id after the last hit
 * written, G when nothing is left, first_group when nothing was written and
 * hits are left). info->per_check[k] = groups of the range that violate check
 * bit k. The same state gives the same bytes.
 * RAFT_EINVAL: checks 0 or with unknown bits, cap > 0 without out;
 * RAFT_ERANGE: first_group > G (first_group == G is an empty audit). A
 * poisoned engine answers RAFT_EINTERNAL. The first audit allocates 8 B per
 * group on the device (counted by raft_engine_info), freed with the engine. */
enum raft_audit_check {
  RAFT_AUDIT_TWO_LEADERS       = 1u,
  RAFT_AUDIT_LOG_MATCHING      = 2u,
  RAFT_AUDIT_COMMIT_DIVERGED   = 4u,
  RAFT_AUDIT_TERM_ORDER        = 8u,
  RAFT_AUDIT_STAMP             = 16u,
  RAFT_AUDIT_COMMIT_BEYOND_LOG = 32u
};
#define RAFT_AUDIT_ALL 63u
typedef struct raft_audit_hit {   /* 24 B */
  uint64_t group;      /* global id: config.group_base + local */
  uint32_t local;
  uint8_t  violated;   /* mask of the requested checks this group violates */
  uint8_t  fault;      /* enum raft_fault (frozen groups are audited like any other) */
  uint8_t  a, b;       /* witness replicas of the lowest violated check; b = 0xFF where the check names one replica */
  int32_t  index;      /* witness index (TWO_LEADERS: the shared term) */
  uint32_t check;      /* the lowest violated check's bit */
} raft_audit_hit;
typedef struct raft_audit_info {  /* 88 B */
  uint64_t matched, written, next_group;
  uint64_t per_check[8];          /* groups in range violating check bit k; [6], [7] are 0 */
} raft_audit_info;
int raft_group_audit(raft_engine* e, uint32_t checks, uint64_t first_group, raft_audit_hit* out, uint64_t cap,
                     raft_audit_info* info);

/* ---- applied state --------------------------------------------------------
 * The last step of the client loop, on the device: every committed entry is
 * applied (folded) where the logs sit, and the replicas of a group are
 * compared wherever their applied prefixes meet: state-machine safety, checked
 * as the entries commit, with no entry leaving the device. The device keeps
 * one 32-B record per fed (group, replica of the mask) from raft_apply_open to
 * raft_apply_close / raft_engine_destroy (counted by raft_engine_info while
 * open); an engine that never opens one allocates nothing for it.
 *
 * The chain. All arithmetic is 64-bit and wrapping; sm is the splitmix64 step
 * of the trace RNG and the digest (x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30)
 * * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31);
 * gid = config.group_base + local group.
 *   seed(gid, base) = sm(sm(gid) ^ uint64(uint32(base)))
 *   folding entry i with Term T and Value V:
 *     chain' = sm(sm(chain ^ (uint64(uint32(T)) << 32 | uint32(i))) ^ uint64(V))
 *     sum'   = sum + V
 * Stamps are not folded: entry equality is the audit's, Term and Value.
 *
 * raft_apply_step treats one fed pair with applied = c, CommitIndex cm,
 * LastApplied l and high-water mark h (REF: h = l; ring depth K) by the commit
 * feed's rule for a cursor c:
 *   hi = min(cm, l)
 *   hi < c:  the pair is counted in `stalled` and left alone (applied, base,
 *            chain, sum, gaps); its trajectory is {c: chain}.
 *   else     lo = min(max(c, h - K), hi).
 *            lo > c: the lo - c entries that have left the ring are counted in
 *              `lost`, the pair in `gapped`; gaps += 1 (saturating at 65535),
 *              base = lo, chain = seed(gid, lo), sum = 0 (a re-seed).
 *            Entries lo+1 .. hi are then folded in order (`folded` counts
 *            them) and applied = hi: at most K entries per pair and step.
 *            The trajectory is the chain value at lo and the chain value after
 *            each folded index: {lo, lo+1, .., hi}.
 * Divergence, per group, from the trajectories of this step:
 *   two fed replicas a != b are comparable when their `base` after this step
 *   is equal (chains of replicas with different bases are never compared);
 *   a comparable pair diverges at i when i is the smallest index present in
 *   both trajectories with different chain values;
 *   a replica whose div_index is 0 and that belongs to a diverging pair (a
 *   stalled one included) gets div_index = the smallest such i over its pairs
 *   and div_peer = the lowest-id peer that attains that smallest index. Both
 *   are sticky: a later step never changes them.
 *   info->diverged counts the groups in which some replica was newly marked.
 * The same state and records give the same bytes. The step reads the state as
 * raft_feed_poll does: no group leaves its shared form, the steady tick's
 * forms and an open feed stay, frozen groups are read like any other. */
typedef struct raft_apply_record {   /* 32 B; one per fed (group, replica) */
  int32_t  applied;    /* entries 1..applied have been looked at; -1: replica outside the mask */
  int32_t  base;       /* the chain and the sum cover base+1..applied */
  uint64_t chain;
  int64_t  sum;        /* wrapping sum of Log.Value over base+1..applied */
  int32_t  div_index;  /* 0: never diverged; else the first index at which this replica's chain
                          differed from a comparable replica's (sticky) */
  uint16_t gaps;       /* re-seeds so far, saturating at 65535 */
  uint8_t  div_peer;   /* that replica, 0xFF: none */
  uint8_t  reserved;   /* 0 */
} raft_apply_record;
/* Where the records start. FROM_START: applied = base = 0. FROM_COMMIT:
 * applied = base = min(CommitIndex, LastApplied) (only what commits from now
 * on). In both chain = seed(gid, base), div_peer = 0xFF (none) and everything
 * else is 0. FROM_RECORDS: the caller's array, [G][R] records read for the
 * replicas of the mask only; every record read must have 0 <= base <= applied
 * and reserved == 0, otherwise the call is RAFT_EINVAL, found before anything
 * changes (an open apply stays open and unchanged); what raft_apply_read
 * returned resumes exactly. */
enum raft_apply_start { RAFT_APPLY_FROM_START = 0, RAFT_APPLY_FROM_COMMIT = 1, RAFT_APPLY_FROM_RECORDS = 2 };
typedef struct raft_apply_info { uint64_t folded, lost, stalled, gapped, diverged, reserved[3]; } raft_apply_info; /* 64 B */
enum raft_apply_select { RAFT_APPLY_DIVERGED = 1u, RAFT_APPLY_GAPPED = 2u };
typedef struct raft_apply_hit {      /* 24 B */
  uint64_t group; uint32_t local;
  uint8_t a, b, flags, fault;        /* flags: the select bits this group matches (all of them, asked for or not) */
  int32_t index; uint32_t gaps;      /* gaps: summed over the fed replicas */
} raft_apply_hit;
/* replica_mask: the feed's rules (RAFT_EINVAL when 0 or with bits at or above
 * R); start: enum raft_apply_start (anything else, or FROM_RECORDS without
 * records, is RAFT_EINVAL). Opening an open apply replaces it. */
int raft_apply_open(raft_engine* e, uint32_t replica_mask, uint32_t start, const raft_apply_record* records);
/* One step over every fed pair (the rules above); info may not be NULL
 * (RAFT_EINVAL); info->reserved is 0. */
int raft_apply_step(raft_engine* e, raft_apply_info* info);
/* out[i * R + r] = the record of replica r of groups[i] (local ids, in any
 * order, repeats allowed), i < n; replicas outside the mask read as all zero
 * with applied = -1. groups == NULL means groups 0..n-1. An id >= G, or n > G
 * with a NULL `groups`, is RAFT_ERANGE with nothing written. */
int raft_apply_read(raft_engine* e, const uint64_t* groups, uint64_t n, raft_apply_record* out);
/* Read-only; looks at the records and at the groups' fault codes only. A group
 * in [first_group, G) is a hit when
 *   select & RAFT_APPLY_DIVERGED and some fed replica has div_index != 0, or
 *   select & RAFT_APPLY_GAPPED   and some fed replica has gaps != 0.
 * Witness of a diverged group: a = the lowest-id fed replica with div_index !=
 * 0, b = its div_peer, index = its div_index. Of a group that is gapped but
 * not diverged: a = the lowest-id fed replica with gaps != 0, b = 0xFF, index
 * = its base. fault: enum raft_fault. Hits come in ascending group order; cap,
 * info->matched, written and next_group follow raft_group_scan's contract
 * (cap = 0 only counts, out may then be NULL; next_group = the local id after
 * the last hit written, G when nothing is left, first_group when nothing was
 * written and hits are left). The same records give the same bytes.
 * RAFT_EINVAL: select 0 or with unknown bits, cap > 0 without out;
 * RAFT_ERANGE: first_group > G (first_group == G is an empty scan). */
int raft_apply_scan(raft_engine* e, uint32_t select, uint64_t first_group, raft_apply_hit* out, uint64_t cap,
                    raft_scan_info* info);
/* Step, read and scan without an open apply are RAFT_EINVAL; close then does
 * nothing. A poisoned engine answers
 * RAFT_EINTERNAL. Handler batches, raft_tick and raft_propose leave the apply
 * open; whatever replaces the state (raft_init_*, raft_load_state,
 * raft_checkpoint_load) closes it, like the feed. raft_restart_groups and
 * raft_load_groups keep it open and reset the fed records of the listed
 * groups, to the FROM_START state after a restart and to the FROM_COMMIT state
 * of the loaded rows after a load; the others do not move. No collective: each
 * engine applies its own shard. */
int raft_apply_close(raft_engine* e);

/* ---- multi-GPU statistics (RCCL over xGMI) -------------------------------
 * Groups shard by id (config.group_base); the only collective is the sum of
 * tick statistics. raft_tick reduces per-tick records on the device (NSTAT
 * int64 = 64 B per tick) and all-reduces them: in a call that runs list or
 * general kernels, once per general-kernel window on a second HIP stream
 * (ordered by an event, overlapping the following ticks); the call's last sum,
 * and the only one of a steady call (list skipped), on the engine stream at
 * the end of the call. Rank 0 creates the id and distributes it out of band.
 * raft_comm_init and every wait on a call with a communicator are bounded by
 * RAFTSTEP_COMM_TIMEOUT_S seconds (default 300): a missing rank or ranks that
 * disagree end in RAFT_ETIMEDOUT with a message (an all-reduce timeout also
 * aborts the communicator and poisons the engine), never in a hang. */
int raft_comm_unique_id(uint8_t id_out[128]);
int raft_comm_init(raft_engine* e, int nranks, int rank, const uint8_t id[128]);
/* All-reduce `stats` (in/out) over the communicator (sum); no-op without one. */
int raft_comm_allreduce_stats(raft_engine* e, raft_tick_stats* stats);
/* Ranks of the attached communicator as RCCL reports them (ncclCommCount /
 * ncclCommUserRank; 1 / 0 without one) and the number of per-window stats
 * all-reduces raft_tick has issued on the engine's comm stream so far. */
int raft_comm_info(raft_engine* e, int32_t* nranks, int32_t* rank, uint64_t* allreduces);

/* ---- instrumentation -----------------------------------------------------
 * mode 1: the steady-state tick kernel is timed by events attached to its
 *         dispatches (hipExtLaunchKernel): in a call that runs the lean (or
 *         fused) kernel alone, one pair spanning the call's back-to-back
 *         launches (start on the first, stop on the last: the kernels run as
 *         in an unprofiled call); otherwise a pair on every dispatch
 *         (kernel-exact, ~5-9 us of wall time between launches);
 * mode 2: one event pair on the engine stream around all launches of each
 *         raft_tick call (no per-launch cost; includes the general kernel and
 *         launch gaps, so it upper-bounds the tick kernel's duration);
 * mode 3: as mode 1 for the second pass of the two-pass tick (the list
 *         kernel over the groups the lean steady-state kernel passed on);
 * mode 0: off. raft_profile_read() syncs and returns the summed milliseconds
 * and the number of tick launches covered. */
int raft_profile_enable(raft_engine* e, int mode);
int raft_profile_read(raft_engine* e, double* total_ms, uint64_t* launches);

/* ---- diagnostics: tick-class coverage ------------------------------------
 * raft_diag_enable(e, 1) zeroes and starts the device lane-class counters:
 * for every tick, the lanes (groups) of the steady-state (lean) kernel and of
 * the full fast-path body (the list kernel, or the one-pass kernel) that took
 * each class of tick. raft_diag_read copies out n <= RAFT_DIAG_COUNTERS
 * counters (indices below) and zeroes them. Counting costs one ballot and
 * atomic per wave and class; off by default. */
#define RAFT_DIAG_DEVICE_COUNTERS 64u
#define RAFT_DIAG_COUNTERS 72u
enum raft_diag_counter {
  /* lean kernel (first pass of the two-pass tick) */
  RAFT_DIAG_LEAN_LANES = 10,          /* groups looked at */
  RAFT_DIAG_LEAN_SKIPPED = 0,         /* deferred to the general kernel or frozen by a fault */
  RAFT_DIAG_LEAN_SSYNC = 18,          /* compressed steady ticks taken */
  RAFT_DIAG_LEAN_LXS = 19,            /* cut-off leader appending alone (LXS) taken */
  RAFT_DIAG_LEAN_THREE_SEG = 20,      /* ring segment switch while the previous segment stays live */
  RAFT_DIAG_LEAN_LXS_WHOLE_ROW = 21,  /* LXS ticks written as whole ring rows */
  RAFT_DIAG_LEAN_HWX = 22,            /* steady ticks of a group with a truncated log in step (HWX) */
  RAFT_DIAG_LEAN_PASSED = 23,         /* groups passed on to the list kernel */
  RAFT_DIAG_LEAN_FORCED = 24,         /* groups passed by raft_debug_force_pass */
  RAFT_DIAG_LEAN_SXS = 25,            /* new leader replicating while the stale one is cut off (SXS) taken */
  RAFT_DIAG_LEAN_SXS_STALE_IN_ROW = 26,/* ... with the stale leader's entry inside the common ring row */
  RAFT_DIAG_LEAN_SXS_VX = 27,         /* SXS ticks whose stale leader holds a virtual suffix (whole rows) */
  RAFT_DIAG_LIST_RETURN_VX = 28,      /* stale leaders' returns with a virtual suffix (no entry copy) */
  RAFT_DIAG_LIST_LXS_VX = 29,         /* LXS entered with a virtual suffix */
  RAFT_DIAG_LEAN_SH = 30,             /* steady ticks whose entries went to the shared ring (SH) */
  RAFT_DIAG_LIST_SH_COPIED = 31,      /* groups in shared form whose entries the list kernel copied back */
  RAFT_DIAG_LIST_SH_ENTRIES = 1,      /* ... the shared entries it copied */
  RAFT_DIAG_LIST_LAG_CATCHUP = 6,     /* REF + CRC: a follower that rejected a corrupted copy caught up (list kernel) */
  RAFT_DIAG_LIST_SH_KEPT = 7,         /* REF + CRC: listed groups that kept their shared form (no copy-back) */
  RAFT_DIAG_LEAN_SWITCH = 5,          /* ring segment switches */
  /* full fast-path body (list kernel / one-pass kernel): 32 + bit */
  RAFT_DIAG_LIST_LANES = 42,          /* groups looked at */
  RAFT_DIAG_LIST_DEFERRED = 33,       /* deferred to the general kernel this tick */
  RAFT_DIAG_LIST_ISOLATION = 34,      /* an isolation window over the group */
  RAFT_DIAG_LIST_SWITCH = 37,         /* ring segment switches */
  RAFT_DIAG_LIST_QUIET = 48,          /* quiet leaderless ticks */
  RAFT_DIAG_LIST_ISOLATED_LEADER = 49,/* cut-off leader appending alone */
  RAFT_DIAG_LIST_SSYNC = 50,          /* ticks ending in the compressed steady state */
  RAFT_DIAG_LIST_ELECTION = 51,       /* a follower's election while the leader is cut off */
  RAFT_DIAG_LIST_FIRST_ROUND = 52,    /* a new leader's first round (fresh rows) */
  RAFT_DIAG_LIST_RETURN = 53,         /* the stale leader's return (step-down + catch-up) */
  RAFT_DIAG_LIST_RETURN_TRUNC = 54,   /* ... with its log truncated */
  RAFT_DIAG_LIST_STALE = 55,          /* new leader replicating while the stale one is cut off */
  RAFT_DIAG_LIST_HWX = 56,            /* truncated logs in step */
  RAFT_DIAG_LIST_THREE_SEG = 57,      /* ring segment switch while the previous segment stays live */
  RAFT_DIAG_LIST_ISOLATED_REPLICA = 58,/* one isolated follower / candidate */
  RAFT_DIAG_LIST_TIMER_FIRE = 59,     /* the isolated replica's election timer fired */
  RAFT_DIAG_LIST_WINDOW_START = 60,   /* a leader-isolation window decided on the fast path */
  RAFT_DIAG_LIST_SXS_MATERIALISED = 61,/* SXS groups taken by the full body (explicit form rebuilt) */
  RAFT_DIAG_LIST_SXS_ENTERED = 62,    /* ticks ending in the SXS compressed form */
  RAFT_DIAG_LIST_STALE_MOVED = 63,    /* segment switch that moved a stale leader's entries (placement only) */
  /* host counters since the last read */
  RAFT_DIAG_TICKS = 64,
  RAFT_DIAG_TICKS_LIST_SKIPPED = 65,  /* ticks run by the lean kernel alone (steady-state list skip) */
  RAFT_DIAG_GENERAL_LAUNCHES = 66,
  RAFT_DIAG_TICKS_STEADY_FORM = 67,   /* ... of those, ticks the lean kernel ran in its steady form (every live group
                                         proven in the global ring phase; RAFTSTEP_STEADY_FORM=0: never) */
  RAFT_DIAG_LAUNCHES_STEADY_ONE = 68, /* steady-form launches that ran the one-entry instantiation (a split tick: two) */
  RAFT_DIAG_TICKS_SPLIT = 69          /* list-skipping ticks issued as two halves on two streams */
};
int raft_diag_enable(raft_engine* e, int on);
int raft_diag_read(raft_engine* e, uint64_t* counters, uint32_t n);
/* Test knob: the lean kernel passes `group` (< 0: none) to the list kernel at
 * every tick instead of taking it. Results are unchanged while the list kernel
 * runs; in a list-skipping call the group's tick is lost, which the engine
 * detects (RAFT_EINTERNAL, engine poisoned until its state is replaced). */
int raft_debug_force_pass(raft_engine* e, int64_t group);
/* Debugging: the raw per-group words of one group (gmeta, giso, hb, the
 * compressed record gss[4], glx[2], grot, grota, gsb, grotb, gsb2). */
#define RAFT_DEBUG_GROUP_WORDS 14u
int raft_debug_group_words(raft_engine* e, uint64_t group, int32_t* out, uint32_t n);
/* Timing diagnostics (results WRONG while non-zero): replaces the engine's
 * kernel diagnostic mode (RAFTSTEP_DIAG_LEAN's bits) from the next call on,
 * e.g. after a settle; RAFT_EINVAL unless the engine was created with
 * debug_flags RAFT_DEBUG_ALLOW_WRONG_RESULTS. 0 restores exact ticks (the
 * state is then whatever the diagnostic ticks left). */
int raft_debug_diag_mode(raft_engine* e, uint32_t mode);
/* Measurement: the steady lean kernel's byte mix and access shape (per
 * element 20 B read in one round trip, 20 B of record + heartbeat and R ring
 * entries of 12 B written as whole rows; 20 + 20 + 12 R bytes) over `elems`
 * fresh elements on `device`, no Raft state: one untimed pass, then `reps`
 * back-to-back passes between HIP events. Returns the mean pass time and the
 * bytes per pass (bench.py: the device's sustained rate for that pattern). */
#define RAFT_PROBE_PLAIN_RING 1u    /* plain (write-back) ring stores instead of non-temporal ones */
#define RAFT_PROBE_NT_RECORD 2u     /* non-temporal record / heartbeat stores */
#define RAFT_PROBE_NO_HEARTBEAT 4u  /* no heartbeat store (a group in shared form): 16 B written + ring */
int raft_stream_probe(int device, uint32_t replicas, uint64_t elems, uint32_t reps, uint32_t flags,
                      double* us_per_pass, double* bytes_per_pass);

#ifdef __cplusplus
}
#endif
#endif /* RAFTSTEP_H */
