"""Clock and election-timer configurations away from the defaults (2 s ticks,
follower timers 10 + rand % 20, candidate timers 10 + rand % 4), shared by
tests/test_oracle_timers.py (CPU: the reference pinned by hand, and the
conditions on these inputs, on the oracle alone) and tests/test_gpu_timers.py
(GPU: engine against oracle).

A timing case is the five raft_config fields; an isolation variant is combined
with it. REF runs at a low isolation rate and ring depth 16; RAFT at a high
rate and ring depth 64 (at depth 16 nearly half of its groups would freeze
with RING_EVICTED, which tests nothing)."""
import numpy as np

import harness as H
from raftstep import abi


def _timing(secs, f_min, f_span, c_min, c_span):
    return dict(tick_seconds=secs, follower_timeout_min=f_min, follower_timeout_span=f_span,
                candidate_timeout_min=c_min, candidate_timeout_span=c_span)


TIMINGS = {
    "unit": _timing(1, 3, 1, 2, 1),             # span 1: `% 1`, every draw equal
    "sub_tick": _timing(7, 1, 5, 1, 3),         # every timer shorter than one tick
    "odd": _timing(3, 5, 13, 4, 7),             # odd spans, span > min, `now` not a multiple of 2
    "long": _timing(1, 40, 3, 40, 3),           # timers longer than any isolation window
    "top": _timing(37, 511, 513, 1000, 24),     # durations 511..1023: the whole 10-bit field, min + span = 1024
}
TIMING_FIELDS = tuple(TIMINGS["unit"])

ISOLATIONS = {
    "hashed": dict(isolate_min_ticks=3, isolate_max_ticks=9),                      # span 7
    "leader": dict(isolate_min_ticks=5, isolate_max_ticks=5, isolate_leader=1),   # span 1
    "full": dict(isolate_min_ticks=1, isolate_max_ticks=32),
}

REF, RAFT = abi.SEM_REF, abi.SEM_RAFT
SEMANTICS = {
    REF: dict(semantics=REF, isolate_per_65536=2500, ring_depth=16),
    RAFT: dict(semantics=RAFT, isolate_per_65536=16384, ring_depth=64),
}
BASE = dict(replicas=5, groups=600, client_period=1, seed=0x71AE)

# the isolation variants a tick trace runs at each timing case: `hashed` everywhere; `leader` and `full`
# where the timers are shorter than a tick or longer than a window (the cut-off leader's forms differ there)
TRACE_ISOLATIONS = {name: ("hashed", "leader", "full") if name in ("sub_tick", "long", "top") else ("hashed",)
                    for name in TIMINGS}


def config(timing, iso, sem, **kw):
    """Engine / oracle keywords of timing case `timing` with isolation variant
    `iso` (None: no isolation) under semantics `sem`."""
    c = dict(BASE, **SEMANTICS[sem])
    c.update(TIMINGS[timing])
    if iso is None:
        c["isolate_per_65536"] = 0
    else:
        c.update(ISOLATIONS[iso])
    c.update(kw)
    return c


TIMEOUT_EDGES = (0, 1, 2, 511, 512, 1022, 1023)


def timer_state(rng, G, R, K, secs):
    """harness.random_state over the whole range a load accepts for the timer
    rows: `timeout` from TIMEOUT_EDGES for half of the replicas and uniform in
    0..1023 for the rest, `deadline` in [-2000, 60 * secs + 2000] (well inside
    2^30: deadline - timeout stays far from the int32 edge). A timeout of 0 is
    a timer that fires in the very tick that resets it."""
    st = H.random_state(rng, G, R, K)
    edges = np.array(TIMEOUT_EDGES)
    pick = rng.integers(0, 2, (G, R)).astype(bool)
    st["timeout"][:] = np.where(pick, edges[rng.integers(0, len(edges), (G, R))], rng.integers(0, 1024, (G, R)))
    st["deadline"][:] = rng.integers(-2000, 60 * secs + 2000 + 1, (G, R))
    assert np.abs(st["deadline"]).max() < 2**30
    return st


PLANT_TERM, PLANT_LAST = 3, 5


def plant_zero_timeout_followers(st, sem, n=32):
    """Groups 0..n-1 of `st` become in-step groups (one leader, g mod R, every
    other replica a follower holding its log and term, MatchIndex = LastApplied:
    what the fast tick kernels take) in which one follower (even g) or every
    follower (odd g) has timeout 0 and a deadline far ahead. Under the oracle's
    rules the leader's heartbeat resets such a timer to now and the same tick's
    timer step fires it."""
    G, R = st["role"].shape
    K = st["log_term"].shape[2]
    assert n <= G and R >= 2 and PLANT_LAST <= K
    for g in range(n):
        c = g % R
        st["role"][g] = abi.FOLLOWER
        st["role"][g, c] = abi.LEADER
        st["voted"][g] = c + 1 if sem == RAFT else 1
        st["term"][g] = PLANT_TERM
        st["last"][g] = PLANT_LAST
        st["commit"][g] = PLANT_LAST - 1
        st["commit"][g, c] = PLANT_LAST
        st["log_term"][g] = 0
        st["log_value"][g] = 0
        st["log_term"][g, :, :PLANT_LAST] = PLANT_TERM
        st["log_value"][g, :, :PLANT_LAST] = 1000 * g + np.arange(PLANT_LAST)
        st["match"][g] = 0
        st["match"][g, c] = PLANT_LAST
        st["match"][g, c, c] = 0
        st["fault"][g] = 0
        st["deadline"][g] = 1 << 20
        st["timeout"][g] = 17
        zero = [r for r in range(R) if r != c]
        st["timeout"][g, zero if g % 2 else zero[:1]] = 0
    return st
