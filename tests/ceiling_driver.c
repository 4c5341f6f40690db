/* Stand-alone driver of oracle/raft_oracle.c near index 2^31, built by
 * tests/test_oracle_ceiling.py with -fsanitize=address,undefined and run as a
 * child process: the windowed log's offset arithmetic (o_node.base) under the
 * sanitizers. It loads states whose logs end at I = 2^31-1 or just below,
 * runs the handlers and ticks that read, grow, truncate and resend those
 * logs, stores and digests the result, and checks a few known answers. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/raft_oracle.h"

#define I 2147483647
enum { G = 6, R = 3, K = 8 };

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

typedef struct {
  uint8_t role[G * R], voted[G * R], fault[G], iso[G];
  int32_t term[G * R], last[G * R], commit[G * R], deadline[G * R], timeout[G * R];
  int32_t match[G * R * R], next[G * R * R], hwm[G * R], log_term[G * R * K];
  int64_t log_value[G * R * K];
  uint32_t log_crc[G * R * K];
} planes;

static raft_state_view view_of(planes* p) {
  raft_state_view v;
  memset(&v, 0, sizeof v);
  v.role = p->role; v.voted = p->voted; v.term = p->term; v.last = p->last; v.commit = p->commit;
  v.deadline = p->deadline; v.timeout = p->timeout; v.match = p->match; v.fault = p->fault;
  v.log_term = p->log_term; v.log_value = p->log_value; v.log_crc = p->log_crc;
  v.next = p->next; v.hwm = p->hwm; v.iso_victim = p->iso;
  return v;
}

/* group g: replica 0 leads at `last`, the followers lag by lag1 / lag2 entries */
static void fill(planes* p, int raft, int g, int32_t last, int32_t term, int lag1, int lag2) {
  const int lag[R] = {0, lag1, lag2};
  for (int r = 0; r < R; ++r) {
    const int i = g * R + r;
    p->role[i] = r ? RAFT_FOLLOWER : RAFT_LEADER;
    p->voted[i] = 1;
    p->term[i] = term;
    p->last[i] = p->hwm[i] = last - lag[r];
    p->commit[i] = last - lag[r] - 1;
    p->timeout[i] = 20 + r;
    p->deadline[i] = 1000;
    for (int s = 0; s < K; ++s) { p->log_term[i * K + s] = term; p->log_value[i * K + s] = 1000 * g + s; }
    if (r) {
      p->match[(g * R) * R + r] = last - lag[r];
      p->next[(g * R) * R + r] = raft ? last - lag[r] + 1 : 0;
    }
  }
}

static void run(int raft, int crc) {
  raft_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.abi_version = RAFT_ABI_VERSION; cfg.replicas = R; cfg.groups = G; cfg.ring_depth = K;
  cfg.entries_per_tick = 3; cfg.client_period = 1; cfg.semantics = raft ? RAFT_SEM_RAFT : RAFT_SEM_REF;
  cfg.seed = 0xCE11; cfg.tick_seconds = 2;
  cfg.follower_timeout_min = 10; cfg.follower_timeout_span = 20;
  cfg.candidate_timeout_min = 10; cfg.candidate_timeout_span = 4;
  cfg.isolate_min_ticks = 8; cfg.isolate_max_ticks = 32; cfg.payload_crc = (uint32_t)crc;
  static planes a, b;
  memset(&a, 0, sizeof a);
  const int top = raft ? I - 1 : I;                 /* RAFT: NextIndex = match + 1 must fit */
  fill(&a, raft, 0, top, I, 0, 0);                  /* at the ceiling, in step, term I */
  fill(&a, raft, 1, top, 7, 2, 0);                  /* follower 1 lags by two */
  fill(&a, raft, 2, I - 1, 7, 0, 0);                /* room 1 of E = 3 */
  fill(&a, raft, 3, I - 20, 7, K - 1, 3);           /* lagging K-1: the oldest window entry is resent */
  fill(&a, raft, 4, I - 40, I - 1, 0, 0);           /* lives through the ticks */
  fill(&a, raft, 5, I - 9, 7, 0, 0);
  a.role[5 * R] = RAFT_FOLLOWER;                    /* leaderless: the first timeout elects */
  a.deadline[5 * R + 1] = 4;
  for (int p = 0; p < R; ++p) a.match[(5 * R) * R + p] = a.next[(5 * R) * R + p] = 0;
  if (crc)
    for (int i = 0; i < G * R * K; ++i) a.log_crc[i] = oracle_entry_crc(a.log_term[i], a.log_value[i]);
  raft_state_view va = view_of(&a), vb = view_of(&b);
  oracle* o = oracle_create(&cfg);
  CHECK(o != NULL);
  CHECK(oracle_load_state(o, &va) == RAFT_OK);
  oracle_store_state(o, &vb);
  CHECK(!memcmp(a.last, b.last, sizeof a.last) && !memcmp(a.log_term, b.log_term, sizeof a.log_term));
  CHECK(!memcmp(a.log_value, b.log_value, sizeof a.log_value) && !memcmp(a.log_crc, b.log_crc, sizeof a.log_crc));
  uint64_t d1[G], d2[G], t1, t2;
  oracle_state_digest(o, d1, &t1);

  /* handlers: an append to the ceiling, one past it, a leader round, a vote */
  raft_log_entry ents[3] = {{I, 1}, {I, 2}, {I, 3}};
  raft_ae_req q;
  raft_ae_resp qs;
  memset(&q, 0, sizeof q);
  q.group = 4; q.to = 1; q.term = I - 1; q.prev_log_index = I - 40; q.prev_log_term = I - 1;
  q.leader_commit = I; q.n_entries = 3;
  CHECK(oracle_append_entries(o, 2, &q, 1, ents, &qs) == RAFT_OK);
  CHECK(qs.success == 1 && qs.match_index == (int64_t)I - 37 && qs.fault == 0);
  raft_group_op op[2] = {{0, 0, RAFT_OP_LEADER_ROUND, 0}, {3, 0, RAFT_OP_LEADER_ROUND, 0}};
  raft_op_result ors[2];
  CHECK(oracle_group_ops(o, 2, op, 2, ors) == RAFT_OK);
  CHECK(ors[0].fault == (raft ? 0 : 0) && ors[1].fault == 0);
  raft_vote_req vq;
  raft_vote_resp vs;
  memset(&vq, 0, sizeof vq);
  vq.group = 1; vq.to = 2; vq.candidate_id = 1; vq.term = I; vq.last_log_index = I; vq.last_log_term = I;
  CHECK(oracle_request_vote(o, 2, &vq, 1, &vs) == RAFT_OK);

  raft_tick_stats st;
  for (int t = 3; t < 23; ++t) oracle_tick(o, t, 1, 1, &st);
  oracle_store_state(o, &vb);
  CHECK(b.fault[2] == RAFT_F_OVERFLOW);
  CHECK(b.last[2 * R] == I);                        /* REF: one of three appended; RAFT: the entry I, then the rule */
  CHECK(b.fault[0] == RAFT_F_OVERFLOW);             /* REF: client append at I; RAFT: NextIndex 2^31 */
  for (int i = 0; i < G * R; ++i) CHECK(b.last[i] >= 0 && b.commit[i] >= 0 && b.term[i] >= 0);
  char buf[512];
  CHECK(oracle_nodelog(o, 0, buf, sizeof buf) > 0);

  /* a second load of what was stored digests the same */
  oracle_state_digest(o, d1, &t1);
  oracle* o2 = oracle_create(&cfg);
  CHECK(oracle_load_state(o2, &vb) == RAFT_OK);
  oracle_state_digest(o2, d2, &t2);
  CHECK(t1 == t2 && !memcmp(d1, d2, sizeof d1));
  oracle_destroy(o2);
  oracle_destroy(o);
}

int main(void) {
  for (int raft = 0; raft < 2; ++raft)
    for (int crc = 0; crc < 2; ++crc) run(raft, crc);
  printf(failures ? "ceiling driver: %d checks failed\n" : "ceiling driver: ok\n", failures);
  return failures ? 1 : 0;
}
