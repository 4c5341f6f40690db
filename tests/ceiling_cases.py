"""Tick traces that cross the int32 ceiling (I = 2^31-1), shared by
tests/test_oracle_ceiling.py (CPU: the coverage conditions, on the oracle
alone) and tests/test_gpu_ceiling.py (GPU: engine against oracle).

Start state: in-step groups, one leader with every follower's log equal to its
own and CommitIndex one behind. Group g's leader has last = I - HEADROOM[g % 20]
and every replica has term = I - ((g // 20) % 4). The headrooms are spread so
that, at one client tick per tick or every other tick and 40 ticks, both E = 1 and E = 3 leave at
least a quarter of the groups frozen by RAFT_F_OVERFLOW and at least a quarter
still live, and so that an E = 3 leader meets its last tick with room 0, 1 and
2. RAFT stores NextIndex = match + 1, and 2^31 is not a NextIndex
(include/raftstep.h), so a RAFT start state is one entry lower."""
import numpy as np

import harness as H
from raftstep import abi

I = H.I32
G, R, K, T0, NTICKS, EVERY = 600, 5, 16, 1, 40, 2
HEADROOM = (0, 1, 2, 4, 5, 10, 20, 30, 130, 160, 200, 250, 300, 400, 500, 600, 700, 800, 900, 1000)

CONFIGS = {
    # the compressed steady form walks into the ceiling
    "plain": dict(),
    # leader isolation: cut-off leaders, elections and term bumps at the ceiling
    "leader_iso": dict(isolate_per_65536=30000, isolate_leader=1),
    # hashed isolation with CRC and corruption on
    "hashed_crc": dict(isolate_per_65536=20000, payload_crc=1, corrupt_per_65536=4000),
    # a client tick every other tick, hashed isolation: with one every tick a leader whose log is at I
    # freezes on its next request before it runs a round, so only here does a leader round meet
    # MatchIndex == I (REF: NextIndex 2^31, a heartbeat) on the general and the list kernel
    "every_other": dict(isolate_per_65536=20000, client_period=2),
}


def config(name, sem, E, **kw):
    c = dict(replicas=R, groups=G, ring_depth=K, client_period=1, entries_per_tick=E, semantics=sem,
             seed=0xCE11 + 16 * sem + E)
    c.update(CONFIGS[name], **kw)
    return c


def start_state(sem, crc):
    rng = np.random.default_rng(0xCE11)
    st = abi.empty_state(G, R, K)
    g = np.arange(G)
    lead = g % R
    last = I - np.array(HEADROOM)[g % 20] - (1 if sem == abi.SEM_RAFT else 0)
    term = I - ((g // 20) % 4)
    st["role"][:] = abi.FOLLOWER
    st["role"][g, lead] = abi.LEADER
    st["voted"][:] = (lead + 1)[:, None] if sem == abi.SEM_RAFT else 1
    st["term"][:] = term[:, None]
    st["last"][:] = last[:, None]
    st["hwm"][:] = last[:, None]
    st["commit"][:] = (last - 1)[:, None]
    st["commit"][g, lead] = last
    st["timeout"][:] = rng.integers(10, 30, (G, R))
    st["timeout"][g, lead] = rng.integers(10, 14, G)
    st["deadline"][:] = 2 * (T0 - 1) + st["timeout"]
    peers = np.ones((G, R), bool)
    peers[g, lead] = False
    st["match"][g, lead] = np.where(peers, last[:, None], 0)
    st["next"][g, lead] = np.where(peers, last[:, None] + 1, 0) if sem == abi.SEM_RAFT else 0
    st["log_term"][:] = term[:, None, None]
    st["log_value"][:] = rng.integers(0, 1 << 62, (G, 1, K))      # the same log on every replica
    if crc:
        H.stamp_crcs(st)
    return st


def coverage(o, st0, E, t0=T0, n=NTICKS):
    """Run the trace on the oracle `o` one tick at a time; what it covered."""
    o.load_state(st0)
    prev = o.store_state()
    rooms, by_timeout = set(), 0
    for t in range(t0, t0 + n):
        o.tick(t, 1)
        s = o.store_state()
        new = np.nonzero((s["fault"] == abi.F_OVERFLOW) & (prev["fault"] == 0))[0]
        for g in new:
            lead = prev["role"][g] == abi.LEADER
            room = int(I - prev["last"][g][np.argmax(lead)]) if lead.any() else E
            if room < E:
                rooms.add(room)                    # frozen by the first leader's client appends
            elif (s["last"][g] < I).all() and (prev["term"][g] == I).any():
                by_timeout += 1                    # no log reached I: Term++ at I
        prev = s
    return dict(overflow=int((prev["fault"] == abi.F_OVERFLOW).sum()), live=int((prev["fault"] == 0).sum()),
                rooms=rooms, by_timeout=by_timeout)
