"""GPU: the steady form of the one-tick lean kernel (tick_steady.hpp; engine.cpp
raft_engine::steady_form) against the CPU oracle. A list-skipping call runs it
while the engine can prove every live group in the global ring phase (calls
consecutive since init_steady), with no device counters enabled — so none of
these tests calls diag_enable before the calls it checks, and each asserts by
the host counter ticks_steady_form that the form ran (or did not). Per-tick
records, digests after every call, then the whole state."""
import numpy as np
import pytest

import harness as H
import oracle
from raftstep import Engine, RaftError, abi

pytestmark = pytest.mark.gpu
G = 3000           # a partial last block, with a wave of dead lanes
CALLS = (6, 1, 13, 20)   # the proving call, then the steady form


def _values(seed, t, n, E, groups):
    """Staged client values of ticks [t, t+n): any int64 >= 0, a function of the tick."""
    return np.random.default_rng([seed, t]).integers(0, 1 << 62, size=(n, E, groups), dtype=np.int64)


def _call(e, o, t, k, stats=True, threads=1):
    """One call on both; the oracle tick by tick, for the per-tick records."""
    if e.cfg.client_source == abi.CLIENT_STAGED:
        v = _values(int(e.cfg.seed), t, k, e.cfg.entries_per_tick, e.cfg.groups)
        e.stage_values(t, v)
        o.stage_values(t, v)
    se = e.tick(t, k, stats=stats)
    recs = np.array([o.tick(t + i, 1, threads=threads) for i in range(k)], np.int64)
    if stats:
        assert list(se) == list(recs.sum(0)), f"sums of ticks [{t}, {t + k})"
        assert np.array_equal(e.tick_records(k), recs), f"per-tick records of ticks [{t}, {t + k})"
    de, do = e.state_digest(), o.state_digest()
    bad = np.nonzero(de[0] != do[0])[0]
    assert not bad.size and de[1] == do[1], f"after tick {t + k - 1}: {bad.size} digests differ, first {bad[:4]}"
    return t + k


def _pair(**kw):
    e, o = Engine(**kw), oracle.Oracle(**kw)
    e.init_steady(0, 0)
    o.init_steady(0, 0)
    return e, o


def _pair_at(leader, tick0, **kw):
    e, o = Engine(**kw), oracle.Oracle(**kw)
    e.init_steady(leader, tick0)
    o.init_steady(leader, tick0)
    return e, o


def _steady(e):
    return e.diag_read()["ticks_steady_form"]


def _setenv(monkeypatch, c):
    """The engine keywords of a case, its env entry applied."""
    c = dict(c)
    for k, v in c.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    return c


REF, RAFT = abi.SEM_REF, abi.SEM_RAFT
CASES = {
    # REF with R = 2 is the commit rule's other branch (2(R-1) > R fails: nothing commits)
    **{f"R{R}_{'raft' if s else 'ref'}": dict(replicas=R, semantics=s) for R in (2, 3, 5, 7) for s in (REF, RAFT)},
    "E3": dict(entries_per_tick=3),
    "E3_raft_crc": dict(entries_per_tick=3, semantics=RAFT, payload_crc=1),
    "crc": dict(payload_crc=1),
    "E16_K64_crc": dict(entries_per_tick=16, ring_depth=64, payload_crc=1),
    "period3": dict(client_period=3),                      # ticks with n == 0: no record stored
    "period3_R3_raft_E3": dict(client_period=3, replicas=3, semantics=RAFT, entries_per_tick=3),
    "staged": dict(client_source=abi.CLIENT_STAGED),
    "staged_E3_crc": dict(client_source=abi.CLIENT_STAGED, entries_per_tick=3, payload_crc=1),
    "nosh": dict(env={"RAFTSTEP_SH": "0"}),
    "nosh_R7_raft_E3_crc": dict(env={"RAFTSTEP_SH": "0"}, replicas=7, semantics=RAFT, entries_per_tick=3, payload_crc=1),
    "nosh_staged_E3": dict(env={"RAFTSTEP_SH": "0"}, client_source=abi.CLIENT_STAGED, entries_per_tick=3),
    "nosh_R2_period3": dict(env={"RAFTSTEP_SH": "0"}, replicas=2, client_period=3),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_the_oracle(monkeypatch, case):
    """3,000 groups, ring depth 16 (the ring wraps several times), calls of 6
    (the proving call), 1, 13 and 20 ticks."""
    c = dict(CASES[case])
    for k, v in c.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    kw = dict(dict(replicas=5, groups=G, ring_depth=16, client_period=1, seed=0x5EED0002), **c)
    e, o = _pair(**kw)
    t = 1
    for i, k in enumerate(CALLS):
        t = _call(e, o, t, k)
        assert _steady(e) == (0 if i == 0 else k), f"call {i}"   # (the first call proves the list empty)
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")
    # the host read copied the shared entries back: the next call re-enters the shared form
    t = _call(e, o, t, 5)
    assert _steady(e) == 5
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")


@pytest.mark.parametrize("split", ["1", "0"])
def test_split_steady_form_matches_oracle(monkeypatch, split):
    """tests/test_gpu_engine_checks.py test_split_steady_tick_matches_oracle
    without diag_enable, so the steady form is what runs: both halves of the
    split tick, a partial last block, calls with and without statistics."""
    monkeypatch.setenv("RAFTSTEP_SPLIT_STEADY", split)
    kw = dict(replicas=5, groups=(1 << 17) + 300, ring_depth=16, client_period=1, seed=0x5EED0002)
    e, o = _pair(**kw)
    t = 1
    for k, st in ((6, True), (20, True), (7, False), (1, True), (13, False), (9, True)):
        se = e.tick(t, k, stats=st)
        so = o.tick(t, k, threads=16)
        if st:
            assert list(se) == list(so), f"stats of ticks [{t}, {t + k})"
        t += k
    e.sync()
    assert e.state_digest()[1] == o.state_digest()[1]
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")
    assert _steady(e) == 50


@pytest.mark.parametrize("extra", [dict(), dict(entries_per_tick=3, payload_crc=1, semantics=abi.SEM_RAFT)],
                         ids=["c2_shape", "raft_E3_crc"])
def test_knob_off_equals_the_default(monkeypatch, extra):
    """RAFTSTEP_STEADY_FORM=0 (the general body everywhere) and the default:
    equal sums, per-tick records and digests after every call."""
    kw = dict(replicas=5, groups=G, ring_depth=16, client_period=1, seed=0x5EED0002, **extra)
    monkeypatch.setenv("RAFTSTEP_STEADY_FORM", "0")
    a = Engine(**kw)
    monkeypatch.delenv("RAFTSTEP_STEADY_FORM")
    b = Engine(**kw)
    a.init_steady(0, 0)
    b.init_steady(0, 0)
    t = 1
    for k, st in ((6, True), (1, True), (13, False), (20, True), (4, False), (3, True)):
        sa, sb = a.tick(t, k, stats=st), b.tick(t, k, stats=st)
        if st:
            assert list(sa) == list(sb), f"sums of ticks [{t}, {t + k})"
            assert np.array_equal(a.tick_records(k), b.tick_records(k)), f"records of ticks [{t}, {t + k})"
        da, db = a.state_digest(), b.state_digest()
        assert np.array_equal(da[0], db[0]) and da[1] == db[1], f"digests after tick {t + k - 1}"
        t += k
    H.assert_same_state(a.store_state(), b.store_state(), f"after tick {t - 1}")
    ca, cb = a.diag_read(), b.diag_read()
    assert ca["ticks_steady_form"] == 0 and ca["ticks_list_skipped"] == 41, ca
    assert cb["ticks_steady_form"] == 41 and cb["ticks_list_skipped"] == 41, cb


def test_gate_a_tick_gap_ends_the_steady_form_until_init_steady():
    kw = dict(replicas=5, groups=G, ring_depth=16, client_period=1, seed=0x5EED0002)
    e, o = _pair(**kw)
    t = _call(e, o, 1, 6)
    t = _call(e, o, t, 9)
    assert _steady(e) == 9
    t += 7                                  # a gap: the groups drift out of the global ring phase
    t = _call(e, o, t, 5)
    t = _call(e, o, t, 11)
    c = e.diag_read()
    assert c["ticks_steady_form"] == 0 and c["ticks"] == 16, c   # the general body, still exact:
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")
    t = _call(e, o, t, 4)                   # consecutive again, but drifted: off until the next init_steady
    assert _steady(e) == 0
    e.init_steady(0, 0)
    o.init_steady(0, 0)
    t = _call(e, o, 1, 6)
    t = _call(e, o, t, 8)
    assert _steady(e) == 8                  # it rises again
    e.diag_enable()                         # device counters keep the general body
    t = _call(e, o, t, 3)
    c = e.diag_read()
    assert c["ticks_steady_form"] == 0 and c["ticks_list_skipped"] == 3 and c["lean_ssync"] == 3 * G, c
    e.diag_enable(False)
    t = _call(e, o, t, 2)
    assert _steady(e) == 2
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")


def test_safety_net_in_the_call_with_statistics():
    """A lane that does not fit (debug_force_pass) during a steady-form call:
    an error return (RAFT_EINTERNAL), the engine poisoned until a reload."""
    kw = dict(replicas=5, groups=G, ring_depth=16, client_period=1, seed=0x5EED0002)
    e, o = _pair(**kw)
    t = _call(e, o, 1, 6)
    t = _call(e, o, t, 5)
    assert _steady(e) == 5
    e.debug_force_pass(42)
    with pytest.raises(RaftError, match="list kernel that did not run") as ei:
        e.tick(t, 4)
    assert ei.value.code == abi.RAFT_EINTERNAL
    assert _steady(e) == 4                  # (the steady form is what ran)
    for call in (lambda: e.tick(t + 4, 1), e.store_state, e.state_digest, e.sync):
        with pytest.raises(RaftError, match="engine state is invalid"):
            call()
    e.debug_force_pass(-1)
    e.load_state(o.store_state())
    t = _call(e, o, t, 4)
    t = _call(e, o, t, 3)
    assert _steady(e) == 0                  # (a loaded state carries no phase proof)
    H.assert_same_state(e.store_state(), o.store_state(), "after the reload")


def test_safety_net_at_the_call_after_a_stats_less_call():
    kw = dict(replicas=5, groups=G, ring_depth=16, client_period=1, seed=0x5EED0002)
    e, o = _pair(**kw)
    t = _call(e, o, 1, 6)
    e.tick(t, 5, stats=False)               # steady form, checked at the next call: clean
    e.tick(t + 5, 3, stats=False)
    e.debug_force_pass(99)
    e.tick(t + 8, 3, stats=False)           # the violation happens here (asynchronously)
    with pytest.raises(RaftError, match="ticks lost") as ei:
        e.tick(t + 11, 1, stats=False)      # ... and is reported by the next call
    assert ei.value.code == abi.RAFT_EINTERNAL
    assert _steady(e) == 11
    with pytest.raises(RaftError, match="engine state is invalid"):
        e.sync()
    e.debug_force_pass(-1)
    e.init_steady(0, 0)                     # state replaced: usable again, and exact
    o.init_steady(0, 0)
    t = _call(e, o, 1, 6)
    t = _call(e, o, t, 7)
    assert _steady(e) == 7
    H.assert_same_state(e.store_state(), o.store_state(), "after init_steady")


# ---- off the origin: per-group leaders, nonzero tick0, a shard base -------------

NOSH = {"RAFTSTEP_SH": "0"}
STAGED = abi.CLIENT_STAGED
KW0 = dict(replicas=5, groups=G, ring_depth=16, client_period=1, seed=0x5EED0002)


def _run_calls(e, o, tick0, what=""):
    """The proving call, then 1, 13 and 20 ticks from tick0 + 1: the steady form
    runs every tick of the later calls; the whole state once in the middle,
    followed by a further call, and at the end."""
    t = tick0 + 1
    for i, k in enumerate(CALLS):
        t = _call(e, o, t, k)
        assert _steady(e) == (0 if i == 0 else k), f"{what}call {i}"
        if i == 2:
            H.assert_same_state(e.store_state(), o.store_state(), f"{what}after tick {t - 1}")
    H.assert_same_state(e.store_state(), o.store_state(), f"{what}after tick {t - 1}")
    return t


# (leader as given or R + its offset, tick0, client_period, further keywords): a
# covering subset of leader {-1, 3, R-1, R+2} x tick0 {0, 4, 5, 1000003} (every
# pair) with client_period {1, 3}, REF / RAFT, the shared ring on / off and
# staged values spread over it. 1000003 = 1 mod 3 and 4 = 1, 5 = 2 mod 3: calls
# that start between two client ticks; 1000003 * E is far past the ring depth.
ORIGINS = [
    (-1, 0, 1, dict(semantics=REF)),
    (3, 4, 1, dict(semantics=RAFT)),
    ("R-1", 5, 3, dict(semantics=REF)),
    ("R+2", 1000003, 3, dict(semantics=RAFT)),
    (-1, 4, 3, dict(semantics=RAFT, env=NOSH)),
    (3, 5, 1, dict(semantics=REF, env=NOSH)),
    ("R-1", 1000003, 1, dict(semantics=RAFT, env=NOSH)),
    ("R+2", 0, 3, dict(semantics=REF, env=NOSH)),
    (-1, 5, 1, dict(semantics=RAFT, entries_per_tick=3)),
    (3, 1000003, 3, dict(semantics=REF, replicas=3)),
    ("R-1", 0, 1, dict(semantics=RAFT, payload_crc=1)),
    ("R+2", 4, 1, dict(semantics=REF, replicas=7, entries_per_tick=3, payload_crc=1, env=NOSH)),
    (-1, 1000003, 1, dict(semantics=REF, client_source=STAGED)),
    ("R+2", 5, 3, dict(semantics=RAFT, client_source=STAGED, entries_per_tick=3, env=NOSH)),
    (-1, 1000003, 3, dict(semantics=RAFT, replicas=7, entries_per_tick=3, payload_crc=1, env=NOSH)),
    (3, 0, 3, dict(semantics=RAFT, replicas=3, entries_per_tick=3)),
]


def _origin_id(c):
    leader, tick0, period, kw = c
    tags = [f"leader{leader}", f"tick{tick0}", f"period{period}", "raft" if kw["semantics"] == RAFT else "ref"]
    tags += ["nosh"] if "env" in kw else []
    tags += ["staged"] if "client_source" in kw else []
    tags += [f"{k[0].upper()}{v}" for k, v in kw.items() if k in ("replicas", "entries_per_tick")]
    tags += ["crc"] if "payload_crc" in kw else []
    return "_".join(tags)


@pytest.mark.parametrize("case", ORIGINS, ids=_origin_id)
def test_parity_off_the_origin(monkeypatch, case):
    """init_steady(leader, tick0) away from (0, 0): the ring rotation
    init_steady leaves is entries_before(tick0 + 1), the leader differs group
    by group (-1) or is taken mod R, and with it the value stream's key."""
    leader, tick0, period, c = case
    kw = dict(KW0, client_period=period, **_setenv(monkeypatch, c))
    R = kw["replicas"]
    leader = {"R-1": R - 1, "R+2": R + 2}.get(leader, leader)
    e, o = _pair_at(leader, tick0, **kw)
    if leader < 0:
        lead = np.argmax(o.store_state()["role"] == abi.LEADER, axis=1)
        assert len(set(lead.tolist())) == R, "the hashed leaders cover every replica"
    _run_calls(e, o, tick0)


@pytest.mark.parametrize("case", ["default", "nosh_R7_E3_crc"])
def test_parity_at_a_64_bit_shard_base(monkeypatch, case):
    """group_base = 2^33 + 77: the trace RNG's key is the global group id, past 32 bits."""
    c = {"default": {}, "nosh_R7_E3_crc": dict(env=NOSH, replicas=7, entries_per_tick=3, payload_crc=1)}[case]
    kw = dict(KW0, group_base=2**33 + 77, **_setenv(monkeypatch, c))
    e, o = _pair_at(-1, 0, **kw)
    assert e.cfg.group_base == o.cfg.group_base == 2**33 + 77
    _run_calls(e, o, 0)
    # (the base matters: the same groups at base 77 hold other values)
    o2 = oracle.Oracle(**dict(kw, group_base=77))
    o2.init_steady(-1, 0)
    o2.tick(1, 6)
    o3 = oracle.Oracle(**kw)
    o3.init_steady(-1, 0)
    o3.tick(1, 6)
    assert o2.state_digest()[1] != o3.state_digest()[1]


# ---- block and wave edges -----------------------------------------------------------

EDGE_FORMS = {
    "default": {},
    # R = 7 does not divide 64: a group's R copies straddle the lanes of a ring row
    "nosh_R7_E3": dict(env=NOSH, replicas=7, entries_per_tick=3),
    "staged": dict(client_source=STAGED),
}


@pytest.mark.parametrize("form", sorted(EDGE_FORMS))
@pytest.mark.parametrize("groups", [1, 63, 64, 65, 255, 256, 257, 512])
def test_parity_at_block_and_wave_edges(monkeypatch, groups, form):
    """Fewer groups than a wave and than a block, whole waves and blocks (no
    dead lane at all), one live lane in the last wave / block."""
    kw = dict(KW0, groups=groups, **_setenv(monkeypatch, EDGE_FORMS[form]))
    e, o = _pair_at(-1, 0, **kw)
    _run_calls(e, o, 0)


# ---- fused config: the steady form needs one tick per launch ------------------------------

@pytest.mark.parametrize("crc", [1, 0])
def test_ticks_per_launch_16_with_and_without_crc(crc):
    """ticks_per_launch = 16: with payload CRC the lean kernel runs tick by tick
    (the steady form), without it the fused launches do; exact either way."""
    kw = dict(KW0, ticks_per_launch=16, payload_crc=crc)
    e, o = _pair(**kw)
    t = 1
    for i, k in enumerate(CALLS + (17,)):
        t = _call(e, o, t, k)
        c = e.diag_read()
        assert c["ticks"] == k and c["ticks_list_skipped"] == (0 if i == 0 else k), (i, c)
        assert c["ticks_steady_form"] == (k if crc and i else 0), (i, c)
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")
    t = _call(e, o, t, 5)
    assert _steady(e) == (5 if crc else 0)
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")


# ---- the list skip's bound --------------------------------------------------------------

def test_list_skip_ends_at_its_bound():
    """The list skip holds while E * (first + k + 2) < 2e9 (LastApplied + E then
    stays inside int32 whatever the log holds). tick0 is derived from that
    formula so that the proving call (6 ticks) and one more call (5 ticks) are
    below the bound and the call after it is the first past it; virtual time,
    tick * tick_seconds + the longest timeout, stays far inside int32 seconds
    (check_ticks: 125e6 * 2 + 30 < 2^31)."""
    E = 16
    kw = dict(KW0, entries_per_tick=E, ring_depth=64)
    limit = (2_000_000_000 - 1) // E - 2          # the largest first + k with E * (first + k + 2) < 2e9
    assert E * (limit + 2) < 2_000_000_000 <= E * (limit + 3)
    tick0 = limit - 6 - 5 - 1                     # first = tick0 + 1; 6 + 5 ticks end exactly at the limit
    e, o = _pair_at(0, tick0, **kw)
    assert (tick0 + 40) * e.cfg.tick_seconds + 64 < 2**31
    t = tick0 + 1
    for k, skipped in ((6, 0), (5, 5), (4, 0), (1, 0), (7, 0)):   # below, at, and three calls past the bound
        assert (E * (t + k + 2) < 2_000_000_000) == (skipped > 0 or k == 6)
        t = _call(e, o, t, k)
        c = e.diag_read()
        assert c["ticks"] == k and c["ticks_list_skipped"] == skipped and c["ticks_steady_form"] == skipped, (t, c)
        if k == 4:
            H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")


# ---- the split tick's second half, every instantiation -------------------------------------

SPLIT_FORMS = {
    "R7_raft_E3_crc": dict(replicas=7, semantics=RAFT, entries_per_tick=3, payload_crc=1),
    "staged_E3_crc": dict(client_source=STAGED, entries_per_tick=3, payload_crc=1),
    "nosh_R3": dict(env=NOSH, replicas=3),
    "nosh_staged_E3": dict(env=NOSH, client_source=STAGED, entries_per_tick=3),
    "period3_R3_raft": dict(client_period=3, replicas=3, semantics=RAFT),
}
# (few and short calls: at this size the oracle's ticks and digests are what an
# item takes; with E = 3 the 16-slot ring still wraps, and the ring's wrap under
# the steady form is what the 3,000-group cases above run at length)
SPLIT_CALLS = ((6, True), (2, False), (1, True))


class _OracleInParts:
    """One oracle over every group, held as four oracles over consecutive
    quarters (group_base apart: groups never address each other and the trace
    RNG is keyed by the global group id, so the parts evolve exactly as one
    oracle over all of them does) — so that the digests and the state views,
    which one oracle computes on one thread, run four at a time like its ticks."""

    def __init__(self, **kw):
        from concurrent.futures import ThreadPoolExecutor
        self.cfg = abi.default_config(**kw)
        n = kw["groups"]
        self.cut = [n * i // 4 for i in range(5)]
        self.parts = [oracle.Oracle(**dict(kw, groups=b - a, group_base=kw.get("group_base", 0) + a))
                      for a, b in zip(self.cut, self.cut[1:])]
        self.pool = ThreadPoolExecutor(5)   # (one more: the engine's state view is copied out alongside)

    def _each(self, f):
        return list(self.pool.map(f, range(4)))

    def init_steady(self, leader, tick0):
        self._each(lambda i: self.parts[i].init_steady(leader, tick0))

    def stage_values(self, t, v):
        self._each(lambda i: self.parts[i].stage_values(t, v[:, :, self.cut[i]:self.cut[i + 1]]))

    def tick(self, t, k, threads=16):
        return np.sum(self._each(lambda i: self.parts[i].tick(t, k, threads=max(1, threads // 4))), axis=0)

    def state_digest(self):
        d = self._each(lambda i: self.parts[i].state_digest())
        return np.concatenate([x[0] for x in d]), sum(x[1] for x in d) % (1 << 64)

    def store_parts(self):
        """The state views of the four parts, and of groups [off, off + n) out of them."""
        s = self._each(lambda i: self.parts[i].store_state())

        def groups(off, n):
            return {f: np.concatenate([x[f][max(off - a, 0):max(off + n - a, 0)] for x, a in zip(s, self.cut)])
                    for f in s[0]}
        return s, groups

    def store_state(self):
        s, _ = self.store_parts()
        return {f: np.concatenate([x[f] for x in s]) for f in s[0]}


def _run_split(monkeypatch, groups, split, form):
    """In the middle the state of three slices (the first and last groups, and
    700 across the boundary between the halves) instead of the whole state: the
    same host read (it copies every group's shared entries back), and the next
    call re-enters the shared form; the whole state at the end."""
    monkeypatch.setenv("RAFTSTEP_SPLIT_STEADY", split)
    kw = dict(KW0, groups=groups, **_setenv(monkeypatch, SPLIT_FORMS[form]))
    e, o = Engine(**kw), _OracleInParts(**kw)
    e.init_steady(-1, 0)
    o.init_steady(-1, 0)
    half = (groups // 2) & ~255
    t = 1
    for i, (k, st) in enumerate(SPLIT_CALLS):
        t = _call(e, o, t, k, stats=st, threads=16)
        assert _steady(e) == (0 if i == 0 else k), f"call {i}"
        if i == 1:
            _, of = o.store_parts()
            for off in (0, half - 350, groups - 700):
                H.assert_same_state(e.store_state_range(off, 700), of(off, 700), f"after tick {t - 1}, slice at {off}")
    fe = o.pool.submit(e.store_state)
    (parts, _), se = o.store_parts(), fe.result()
    ranges = list(zip(o.cut, o.cut[1:]))
    diffs = o._each(lambda i: H.diff_states({f: v[ranges[i][0]:ranges[i][1]] for f, v in se.items()}, parts[i]))
    for (a, b), d in zip(ranges, diffs):
        assert not d, f"state mismatch after tick {t - 1}, groups [{a}, {b}) (indices from {a}):\n" + "\n".join(d)


@pytest.mark.parametrize("form", sorted(SPLIT_FORMS))
@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("groups", [131072, 131072 + 257])
def test_split_second_half_every_form(monkeypatch, groups, split, form):
    """131072 groups is the smallest count that splits (two halves of 65536,
    whole blocks); + 257 leaves one live lane in the second half's last block.
    The second half runs at a group offset on its own stream: staged values,
    the CRC table, ring tiles and the per-group records are all addressed
    through it. Calls alternate with and without statistics."""
    _run_split(monkeypatch, groups, split, form)


def test_one_group_below_the_split(monkeypatch):
    """131071 groups: the second half would hold 65535, so one launch per tick."""
    _run_split(monkeypatch, 131071, "1", "nosh_staged_E3")


# ---- streaming record stores (rec_nt) ---------------------------------------------------

SLICE = 700


@pytest.mark.parametrize("steady_form", ["1", "0"])
def test_streaming_record_stores(monkeypatch, steady_form):
    """Both lean bodies store the 16-byte group records with streaming stores
    once the engine's records outgrow the cache: padded groups * 40 B > 256 MiB
    (engine.cpp, where DevPlanes::rec_nt is set). The engine pads its groups to
    whole 256-group blocks, Gp = (G + 255) & ~255, so the smallest such count
    is the first G whose Gp exceeds 256 MiB / 40: Gp = 6,711,040 (26,215
    blocks; 26,214 blocks * 256 * 40 = 268,431,360 <= 268,435,456), G = Gp - 255
    = 6,710,785, computed below by the same expressions. R = 3 (REF commits:
    2(R-1) > R), ring depth 2 and E = 1 are the smallest the config check admits
    (E < K for the list skip). Ten oracle slices of 700 groups: group 0, the
    last groups, one across the split boundary (G/2) & ~255, seven in between."""
    monkeypatch.setenv("RAFTSTEP_STEADY_FORM", steady_form)
    padded = lambda g: (g + 255) & ~255
    first_gp = padded((256 << 20) // 40 + 1)          # the smallest padded count with Gp * 40 > 256 MiB
    groups = first_gp - 255                           # ... and the smallest G padded to it
    assert padded(groups) * 40 > 256 << 20 >= padded(groups - 1) * 40 and groups == 6710785
    kw = dict(replicas=3, groups=groups, ring_depth=2, entries_per_tick=1, client_period=1, seed=0x5EED0002)
    half = (groups // 2) & ~255
    rng = np.random.default_rng(7)
    offs = [0] + sorted(int(x) for x in rng.integers(1, groups - 2 * SLICE, 7)) + [half - SLICE // 2, groups - SLICE]
    e = Engine(**kw)
    slices = [oracle.Oracle(**dict(kw, groups=SLICE, group_base=off)) for off in offs]
    for x in [e] + slices:
        x.init_steady(-1, 0)
    t = 1
    for i, (k, st) in enumerate(((6, True), (1, True), (13, False), (20, True))):
        se = e.tick(t, k, stats=st)
        for o in slices:
            o.tick(t, k)
        t += k
        if st:                                        # no fault, and every group keeps its leader every tick
            assert se[6] == 0 and se[7] == groups * k, list(se)
        d, _ = e.state_digest()
        for o, off in zip(slices, offs):
            bad = np.nonzero(d[off:off + SLICE] != o.state_digest()[0])[0]
            assert not bad.size, (f"after tick {t - 1}: slice at {off}: {bad.size} digests differ, first group "
                                  f"{off + int(bad[0])}\nengine:\n{e.nodelog(off + int(bad[0]))}oracle:\n"
                                  f"{o.nodelog(int(bad[0]))}")
        c = e.diag_read()
        assert c["ticks_list_skipped"] == (k if i else 0), (i, c)
        assert c["ticks_steady_form"] == (k if i and steady_form == "1" else 0), (i, c)
    for o, off in zip(slices, offs):
        H.assert_same_state(e.store_state_range(off, SLICE), o.store_state(), f"slice at {off}")
