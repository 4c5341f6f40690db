"""A host-side model of when a raft_tick call skips the list kernel, runs the
lean kernel's steady form and splits the tick in two halves, and a generator
of host call schedules. Plain Python: nothing of the engine is imported here.

The model restates the documented contract (include/raftstep.h; the comment
blocks on raft_engine::steady_origin / steady_ok, steady_form and split_steady
in engine.cpp), not the engine's call plan:

  origin  every log was empty at init_steady and only ticks appended since.
          Set by init_steady; cleared by init_new_nodes, load_state,
          load_checkpoint and any handler batch.
  ok      a call with statistics has proven the list empty. Cleared with
          origin and by init_steady; set at the end of a call with statistics
          while origin holds (a schedule issues that call itself: 6 ticks with
          statistics straight after every init_steady); a call without
          statistics leaves it as it is.
  phase   every live group appends in the global ring phase. Set by
          init_steady(.., tick0) for a call at tick0 + 1; dropped for good by a
          call that starts at any other tick than the one after the last call,
          and by everything that clears origin. A call of no ticks changes
          nothing.

  skip    = origin and ok and E < K and E * (first + k + 2) < 2e9
            (no isolation, no corruption in the configs modelled here)
  steady  = skip and one tick per launch and phase and device counters off
            and RAFTSTEP_STEADY_FORM != 0
  split   = skip and one tick per launch and RAFTSTEP_SPLIT_STEADY != 0 and
            both halves (of whole 256-group blocks) hold >= 65536 groups
  one tick per launch: ticks_per_launch <= 1, or payload_crc, or profile mode 3.

Host reads (store_state, store_state_range, state_digest, nodelog,
debug_group_words, save_checkpoint, sync) keep all three records.

An operation is a tuple whose first element is its kind (OPS below); ticks are
relative: apply() in the GPU test, and walk() here, keep the running tick.
"""
from collections import namedtuple

import numpy as np

Prediction = namedtuple("Prediction", "ticks skip steady split")

READS = ("store_state", "store_state_range", "state_digest", "nodelog", "debug_group_words", "sync")
BATCHES = ("append_entries", "request_vote", "group_ops")
# kinds that leave the records alone, and kinds after which only init_steady brings the steady form back
KEEPING = READS + ("tick0", "diag_enable", "profile")
DESTROYING = ("gap", "load_state", "checkpoint") + BATCHES
OPS = ("tick", "init_steady") + KEEPING + DESTROYING
PROVING = ("tick", 6, True)
TICK0S = (0, 4, 5, 1000003)


class Model:
    def __init__(self, cfg, env=None):
        """cfg: the engine's keyword arguments; env: the RAFTSTEP_* variables it is created under."""
        env = env or {}
        self.E = int(cfg.get("entries_per_tick", 1))
        self.K = int(cfg.get("ring_depth", 32))
        self.G = int(cfg["groups"])
        self.tpl = max(1, int(cfg.get("ticks_per_launch", 1)))
        self.crc = bool(cfg.get("payload_crc", 0))
        self.steady_form = int(env.get("RAFTSTEP_STEADY_FORM", "1")) != 0
        self.split_steady = int(env.get("RAFTSTEP_SPLIT_STEADY", "1")) != 0
        self.origin = self.ok = self.phase = False
        self.next = 0
        self.counters = False
        self.prof = 0

    # -- calls that replace or change the state ------------------------------
    def _mutated(self):
        self.origin = self.ok = self.phase = False

    def init_steady(self, leader, tick0):
        self._mutated()
        self.origin = self.phase = True
        self.next = tick0 + 1

    init_new_nodes = load_state = load_checkpoint = handler_batch = lambda self, *a: self._mutated()

    # -- calls that keep it ----------------------------------------------------
    def read(self):
        pass

    def diag_enable(self, on=True):
        self.counters = bool(on)

    def profile(self, mode):
        self.prof = int(mode)

    def tick(self, first, k, stats=True):
        if k == 0:
            return Prediction(0, False, False, False)
        if first != self.next:
            self.phase = False
        self.next = first + k
        skip = self.origin and self.ok and self.E < self.K and self.E * (first + k + 2) < 2_000_000_000
        one = self.tpl == 1 or self.crc or self.prof == 3
        steady = skip and one and self.phase and not self.counters and self.steady_form
        half = (self.G // 2) & ~255
        split = skip and one and self.split_steady and half >= 65536 and self.G - half >= 65536
        if stats and self.origin:
            self.ok = True
        return Prediction(k, skip, steady, split)


def batch_items(kind, sub_seed, cfg):
    """The items of one handler batch (plain dicts, as tests/harness.py's
    ae_reqs / vote_reqs / ops take them), over a third of the groups. A
    function of (kind, sub_seed, cfg): drawn once, both sides get the same."""
    G, R = int(cfg["groups"]), int(cfg.get("replicas", 3))
    rng = np.random.default_rng([0xBA7C4, BATCHES.index(kind), sub_seed])
    groups = rng.permutation(G)[: max(1, G // 3)]
    if kind == "append_entries":
        return [dict(group=int(g), to=int(rng.integers(0, R)), term=int(rng.integers(0, 6)),
                     prev_log_index=int(rng.integers(0, 8)), prev_log_term=int(rng.integers(0, 6)),
                     leader_commit=int(rng.integers(0, 10)),
                     logs=[(int(rng.integers(0, 6)), int(rng.integers(0, 1 << 62)))
                           for _ in range(int(rng.integers(0, 5)))]) for g in groups]
    if kind == "request_vote":
        return [dict(group=int(g), to=int(rng.integers(0, R)), term=int(rng.integers(0, 8)),
                     candidate_id=int(rng.integers(0, R))) for g in groups]
    return [dict(group=int(g), replica=int(rng.integers(0, R)), kind=int(rng.integers(1, 6)),
                 arg=int(rng.integers(0, 1 << 62))) for g in groups]


# the fixed mix: (kind, weight)
MIX = (("tick", 36), ("tick0", 3), ("gap", 2),
       ("store_state", 3), ("store_state_range", 4), ("state_digest", 3), ("nodelog", 4), ("debug_group_words", 4),
       ("sync", 3), ("checkpoint", 2), ("load_state", 2),
       ("append_entries", 1), ("request_vote", 1), ("group_ops", 1),
       ("diag_enable", 4), ("profile", 5), ("init_steady", 10))


def schedule(seed, n_ops, cfg):
    """n_ops operations, a function of (seed, n_ops, cfg). The first is an
    init_steady, and every init_steady is followed by the proving call. No
    operation is meant to fail."""
    G, R = int(cfg["groups"]), int(cfg.get("replicas", 3))
    rng = np.random.default_rng([0x5C4ED, seed])
    kinds = [k for k, _ in MIX]
    p = np.array([w for _, w in MIX], float)
    p /= p.sum()
    ops = []
    while len(ops) < n_ops:
        kind = "init_steady" if not ops else kinds[int(rng.choice(len(kinds), p=p))]
        if kind == "init_steady":
            if len(ops) + 2 > n_ops:
                continue                   # (no room for its proving call)
            ops.append((kind, (0, -1, R + 1)[int(rng.integers(0, 3))], TICK0S[int(rng.integers(0, 4))]))
            ops.append(PROVING)
        elif kind == "tick":
            ops.append((kind, int(rng.integers(1, 21)), bool(rng.integers(0, 2))))
        elif kind == "tick0":
            ops.append((kind, bool(rng.integers(0, 2))))
        elif kind == "gap":
            ops.append((kind, int(rng.integers(1, 10))))
        elif kind == "store_state_range":
            g0 = int(rng.integers(0, G))
            ops.append((kind, g0, int(rng.integers(1, G - g0 + 1))))
        elif kind in ("nodelog", "debug_group_words"):
            ops.append((kind, int(rng.integers(0, G))))
        elif kind in BATCHES:
            ops.append((kind, int(rng.integers(0, 1 << 31))))
        elif kind == "diag_enable":
            ops.append((kind, bool(rng.integers(0, 2))))
        elif kind == "profile":
            ops.append((kind, int(rng.integers(0, 4))))
        else:
            ops.append((kind,))
    return ops


# The schedules of tests/test_gpu_steady_schedule.py (and the conditions
# tests/test_steady_model.py holds them to): name -> (engine keywords,
# environment, seeds). Plain integers: semantics 1 = RAFT, client_source 1 =
# staged values (include/raftstep.h). The seeds were chosen, by coverage()
# alone, so that each schedule and each config's six together meet those
# conditions; fused16 runs the steady form only under profile mode 3.
N_OPS = 40
BASE = dict(replicas=5, groups=3000, ring_depth=16, client_period=1, seed=0x5EED0002)
SEEDS = (2208, 4269, 5141, 10666, 29067, 29270)
CONFIGS = {
    "default": (dict(BASE), {}, SEEDS),
    "nosh_R7_raft_E3_crc": (dict(BASE, replicas=7, semantics=1, entries_per_tick=3, payload_crc=1),
                            {"RAFTSTEP_SH": "0"}, SEEDS),
    "staged_E3": (dict(BASE, client_source=1, entries_per_tick=3), {}, SEEDS),
    "fused16": (dict(BASE, ticks_per_launch=16), {}, (3251, 3717, 5848, 21187, 24702, 27105)),
}


def walk(ops, cfg, env=None):
    """The model over a schedule: [(index, op, first tick or None, Prediction or None)]."""
    m = Model(cfg, env)
    t, out = 0, []
    for i, op in enumerate(ops):
        kind, first, pred = op[0], None, None
        if kind == "tick":
            first, pred = t, m.tick(t, op[1], op[2])
            t += op[1]
        elif kind == "tick0":
            first, pred = t, m.tick(t, 0, op[1])
        elif kind == "gap":
            t += op[1]
        elif kind == "init_steady":
            m.init_steady(op[1], op[2])
            t = op[2] + 1
        elif kind == "load_state":
            m.load_state()
        elif kind == "checkpoint":
            m.read()
            m.load_checkpoint()
        elif kind in BATCHES:
            m.handler_batch()
        elif kind == "diag_enable":
            m.diag_enable(op[1])
        elif kind == "profile":
            m.profile(op[1])
        else:
            assert kind in READS, kind
            m.read()
        out.append((i, op, first, pred))
    return out


def coverage(ops, cfg, env=None):
    """What a schedule covers: (ticks, steady ticks, the keeping kinds seen
    directly between two steady-form calls, the destroying kinds seen and later
    followed by an init_steady after which the steady form runs again)."""
    w = walk(ops, cfg, env)
    ticks = sum(p.ticks for _, _, _, p in w if p)
    steady = sum(p.ticks for _, _, _, p in w if p and p.steady)
    calls = [(i, p.steady) for i, op, _, p in w if op[0] == "tick"]
    between = set()
    for (a, sa), (b, sb) in zip(calls, calls[1:]):
        if sa and sb:
            between.update(ops[j][0] for j in range(a + 1, b))
    recovered = set()
    for i, op in enumerate(ops):
        if op[0] in DESTROYING:
            init = next((j for j in range(i + 1, len(ops)) if ops[j][0] == "init_steady"), None)
            if init is not None and any(p and p.steady for j, _, _, p in w[init:]):
                # (steady after that init_steady, or after a later one: the form rose again either way)
                recovered.add(op[0])
    return ticks, steady, between & set(KEEPING), recovered
