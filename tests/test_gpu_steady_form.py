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


def _steady(e):
    return e.diag_read()["ticks_steady_form"]


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
