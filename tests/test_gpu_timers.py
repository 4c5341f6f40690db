"""GPU: the engine against the oracle at the clock and election-timer
configurations of tests/timer_cases.py, bit-exact. Every other GPU test runs
at 2 s ticks, follower timers 10 + rand % 20 and candidate timers 10 +
rand % 4; here tick_seconds is 1, 3, 7, 37 and 1000, the spans are 1, odd and
larger than the minimum, the timers are shorter than a tick and longer than
any isolation window, the 10-bit duration field is full (511..1023), and
loaded rows carry every timeout the load accepts, 0 included. Tick traces on
every device path, the steady form and its implied heartbeat time, handler
batches and ticks from loaded states, round trips through every loader,
checkpoint mismatches, the end of virtual time and the checks at creation.
tests/test_oracle_timers.py pins the reference at these configurations."""
import os

import numpy as np
import pytest

import groups_model as GM
import harness as H
import load_model as LM
import oracle
import timer_cases as TC
from raftstep import Engine, RaftError, abi
from test_gpu_parity import compare, pair
from test_gpu_steady_form import CALLS, _call, _steady

pytestmark = pytest.mark.gpu
I = H.I32
SEMS = [TC.REF, TC.RAFT]
SEM_ID = {TC.REF: "ref", TC.RAFT: "raft"}.get


def _digests(e, o, what):
    de, do = e.state_digest(), o.state_digest()
    bad = np.nonzero(de[0] != do[0])[0]
    assert not bad.size and de[1] == do[1], f"{what}: {bad.size} digests differ, first {bad[:4]}"


def _refused(code, call, *a):
    with pytest.raises(RaftError) as ei:
        call(*a)
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


# ---- a. tick traces on every device path --------------------------------------------------

TRACES = [(name, iso, path) for name in sorted(TC.TIMINGS) for iso in TC.TRACE_ISOLATIONS[name]
          for path in (("auto", "single", "general") if iso == "hashed" else ("auto",))]


@pytest.mark.parametrize("sem", SEMS, ids=SEM_ID)
@pytest.mark.parametrize("name,iso,path", TRACES, ids=["-".join(c) for c in TRACES])
def test_tick_trace(name, iso, path, sem):
    """New nodes, then 120 ticks: the first elections come from the follower
    draws, everything after from both ranges. State and statistics every 8."""
    kw = TC.config(name, iso, sem)
    e, o = pair(general=(path == "general"), single=(path == "single"), **kw)
    e.init_new_nodes(0)
    o.init_new_nodes(0)
    compare(e, o, "init")
    tot_e, tot_o = np.zeros(8, np.int64), np.zeros(8, np.int64)
    for t in range(0, 120, 8):
        tot_e += e.tick(t, 8)
        tot_o += o.tick(t, 8, threads=4)
        compare(e, o, f"after tick {t + 7}")
        assert list(tot_e) == list(tot_o), f"stats differ after tick {t + 7}: {tot_e} vs {tot_o}"
    _digests(e, o, "at the end")


# ---- b. the steady form and the implied heartbeat time ------------------------------------

FORMS = {
    "default": dict(),
    # fused launches configured, CRC stamps, every entry in the replica rings, the split tick asked for
    "tpl16_crc_nosh_split": dict(ticks_per_launch=16, payload_crc=1,
                                 env={"RAFTSTEP_SH": "0", "RAFTSTEP_SPLIT_STEADY": "1"}),
}
STEADY = [(name, form) for name in sorted(TC.TIMINGS) for form in sorted(FORMS)
          if form == "default" or name in ("odd", "top")]


@pytest.mark.parametrize("leave", ["read_then_gap", "votes"])
@pytest.mark.parametrize("sem", SEMS, ids=SEM_ID)
@pytest.mark.parametrize("name,form", STEADY, ids=["-".join(c) for c in STEADY])
def test_steady_form_and_implied_heartbeat(monkeypatch, name, form, sem, leave):
    """3,000 in-step groups, ring depth 16, calls of 6 (the proving call), 1,
    13 and 20 ticks: the steady form runs the later ones. A group in shared
    form stores no heartbeat time: every follower's deadline is the last
    tick's now, last_tick * tick_seconds, plus its timeout. Then the form is
    left: by a host read (and re-entered) and a gap in ticks, or by a batch of
    vote requests."""
    c = dict(FORMS[form])
    for k, v in c.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    kw = TC.config(name, None, sem, groups=3000, ring_depth=16, **c)
    secs = kw["tick_seconds"]
    e, o = Engine(**kw), oracle.Oracle(**kw)
    e.init_steady(0, 0)
    o.init_steady(0, 0)
    t = 1
    for i, k in enumerate(CALLS):
        t = _call(e, o, t, k)
        assert _steady(e) == (0 if i == 0 else k), f"call {i}"
    st = e.store_state()
    H.assert_same_state(st, o.store_state(), f"after tick {t - 1}")
    fol = st["role"] == abi.FOLLOWER
    assert fol.sum() == 3000 * 4 and (st["fault"] == 0).all()
    assert (st["deadline"][fol] == (t - 1) * secs + st["timeout"][fol]).all()
    lo, hi = kw["follower_timeout_min"], kw["follower_timeout_min"] + kw["follower_timeout_span"]
    assert lo <= st["timeout"][fol].min() and st["timeout"][fol].max() < hi
    if leave == "read_then_gap":
        t = _call(e, o, t, 5)                  # the host read copied the shared entries back: re-entered
        assert _steady(e) == 5
        H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")
        t = _call(e, o, t, 3)                  # (in the form again when the gap comes)
        assert _steady(e) == 3
        t +=-(-(kw["follower_timeout_min"] + kw["follower_timeout_span"]) // secs) + 1
        t = _call(e, o, t, 10)
        assert _steady(e) == 0
    else:
        rng = np.random.default_rng(0xB0 + sem)
        groups = rng.permutation(3000)[:1000]
        reqs = H.vote_reqs([dict(group=int(g), to=int(rng.integers(0, 5)), term=int(rng.integers(2, 5)),
                                 candidate_id=int(rng.integers(0, 5))) for g in groups])
        reqs["last_log_index"] = t - 1
        reqs["last_log_term"] = 1
        a, b = e.request_vote(t, reqs), o.request_vote(t, reqs)
        assert a.tobytes() == b.tobytes(), "vote responses differ"
        H.assert_same_state(e.store_state(), o.store_state(), "after the vote requests")
        t = _call(e, o, t, 10)
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")


# ---- c. handler batches on loaded timer rows ----------------------------------------------

@pytest.mark.parametrize("sem", SEMS, ids=SEM_ID)
@pytest.mark.parametrize("name", ["odd", "top"])
@pytest.mark.parametrize("R", [3, 5, 8])
def test_handler_batches_timer_states(R, name, sem):
    """test_gpu_parity.py test_handler_batches_random_states on
    timer_cases.timer_state: every timeout a load accepts, deadlines on both
    sides of the batches' now (0..60 ticks). As there, prev_log_index starts
    at -1, under RAFT too: an entry to be checked at index 0 is GetLog(0),
    which panics (RAFT_F_PANIC_GETLOG)."""
    rng = np.random.default_rng(5000 + R + 7 * sem + (50 if name == "top" else 0))
    G, K = 192, 8
    kw = dict(TC.TIMINGS[name], replicas=R, groups=G, ring_depth=K, seed=0x71C + R, semantics=sem)
    e, o = pair(**kw)
    st = TC.timer_state(rng, G, R, K, kw["tick_seconds"])
    e.load_state(st)
    o.load_state(st)
    compare(e, o, "after load")
    _digests(e, o, "after load")
    for rnd in range(12):
        now = int(rng.integers(0, 61))
        kind = rnd % 3
        groups = rng.permutation(G)[: G // 2]
        if kind == 0:
            items = [dict(group=int(g), to=int(rng.integers(0, R)), term=int(rng.integers(0, 7)),
                          prev_log_index=int(rng.integers(-1, 14)), prev_log_term=int(rng.integers(0, 7)),
                          leader_commit=int(rng.integers(0, 16)),
                          logs=[(int(rng.integers(0, 7)), int(rng.integers(0, 1 << 62)))
                                for _ in range(int(rng.integers(0, 12)))]) for g in groups]
            reqs, ents = H.ae_reqs(items)
            a, b = e.append_entries(now, reqs, ents), o.append_entries(now, reqs, ents)
        elif kind == 1:
            reqs = H.vote_reqs([dict(group=int(g), to=int(rng.integers(0, R)), term=int(rng.integers(0, 8)),
                                     candidate_id=int(rng.integers(0, R))) for g in groups])
            reqs["last_log_index"] = rng.integers(0, 14, len(reqs))
            reqs["last_log_term"] = rng.integers(0, 7, len(reqs))
            a, b = e.request_vote(now, reqs), o.request_vote(now, reqs)
        else:
            ops = H.ops([dict(group=int(g), replica=int(rng.integers(0, R)), kind=int(rng.integers(1, 6)),
                              arg=int(rng.integers(0, 1 << 62))) for g in groups])
            a, b = e.group_ops(now, ops), o.group_ops(now, ops)
        assert a.tobytes() == b.tobytes(), f"round {rnd} kind {kind}: responses differ"
        compare(e, o, f"round {rnd} kind {kind}")
        _digests(e, o, f"round {rnd}")


# ---- d. ticks from loaded timer rows --------------------------------------------------------

PLANTED = 32


@pytest.mark.parametrize("sem", SEMS, ids=SEM_ID)
@pytest.mark.parametrize("name", ["odd", "top"])
@pytest.mark.parametrize("R", [3, 5])
def test_tick_from_timer_states(R, name, sem):
    """test_gpu_parity.py test_tick_from_random_states on timer_state: 30
    single ticks from tick 30. A row with timeout 0 is a timer that a reset at
    `now` leaves at deadline == now, which the same tick's timer step fires:
    a follower of a healthy leader stands for election at its heartbeat. The
    random rows hold few in-step groups, the only ones the fast kernels take,
    so 32 are planted (timer_cases.plant_zero_timeout_followers)."""
    rng = np.random.default_rng(277 + R + sem + (50 if name == "top" else 0))
    G, K = 512, 16
    kw = dict(TC.TIMINGS[name], replicas=R, groups=G, ring_depth=K, client_period=2, seed=0x71D + R,
              isolate_per_65536=8000, semantics=sem)
    e, o = pair(**kw)
    st = TC.plant_zero_timeout_followers(TC.timer_state(rng, G, R, K, kw["tick_seconds"]), sem, PLANTED)
    e.load_state(st)
    o.load_state(st)
    compare(e, o, "after load")
    for t in range(30, 60):
        se, so = e.tick(t, 1), o.tick(t, 1)
        assert list(se) == list(so), (R, t)
        compare(e, o, f"R={R} tick {t}")
        if t == 30:   # the planted in-step groups: the heartbeat fired the zero timers (but for a few cut-off replicas)
            moved = (o.store_state(logs=False)["term"][:PLANTED] > TC.PLANT_TERM).any(axis=1)
            assert moved.sum() >= PLANTED * 3 // 4, int(moved.sum())
    _digests(e, o, "at the end")


# ---- e. round trips at the edges of the duration field -------------------------------------

def test_round_trips_at_the_top_of_the_duration_field(tmp_path):
    """40 ticks of `top` (RAFT, hashed isolation): the stored durations are
    511..1023. load_state of the stored view into a fresh engine, a checkpoint
    into another, then rows of 100 groups into other groups of a twin that has
    run on: equal states and per-group digests, and again 10 ticks later."""
    kw = TC.config("top", "hashed", TC.RAFT)
    e, o = pair(**kw)
    e.init_new_nodes(0)
    o.init_new_nodes(0)
    assert list(e.tick(0, 40)) == list(o.tick(0, 40, threads=4))
    st = e.store_state()
    H.assert_same_state(st, o.store_state(), "after 40 ticks")
    assert st["timeout"].max() == 1023 and (st["timeout"] >= 512).sum() > kw["groups"]
    dig = e.state_digest()
    e2, o2 = pair(**kw)
    e2.load_state(st)
    o2.load_state(st)
    path = os.path.join(tmp_path, "top.ckpt")
    e.save_checkpoint(path)
    e3, _ = pair(**kw)
    e3.load_checkpoint(path)
    for x, what in ((e2, "load_state"), (e3, "the checkpoint")):
        H.assert_same_state(x.store_state(), st, f"after {what}")
        d = x.state_digest()
        assert np.array_equal(d[0], dig[0]) and d[1] == dig[1] == o.state_digest()[1], f"digests after {what}"
    so = o.tick(40, 10, threads=4)
    o2.tick(40, 10, threads=4)
    for x, what in ((e, "the source"), (e2, "load_state"), (e3, "the checkpoint")):
        assert list(x.tick(40, 10)) == list(so), f"stats of 10 more ticks: {what}"
        compare(x, o, f"10 ticks later: {what}")
        _digests(x, o, f"10 ticks later: {what}")
    # rows of the tick-40 state, the ones with the longest timers first, into other groups of the twin at tick 50
    G = kw["groups"]
    idx = np.argsort(-st["timeout"].max(axis=1), kind="stable")[:100]
    ids = (idx + G // 2 + 7) % G
    assert len(set(ids.tolist())) == 100 and not (ids == idx).any()
    rows = LM.take(st, idx)
    assert (rows["timeout"] >= 512).all(axis=1).any() and rows["timeout"].max() == 1023
    before = e2.state_digest()[0]
    e2.load_groups(ids, rows)
    LM.load(o2, ids, rows)
    compare(e2, o2, "after load_groups")
    _digests(e2, o2, "after load_groups")
    others = np.setdiff1d(np.arange(G), ids)
    assert np.array_equal(e2.state_digest()[0][others], before[others]), "an unlisted group changed"
    assert list(e2.tick(50, 10)) == list(o2.tick(50, 10, threads=4))
    compare(e2, o2, "10 ticks after load_groups")
    _digests(e2, o2, "10 ticks after load_groups")


def test_restart_draws_from_the_configured_range():
    """REF `unit` with hashed isolation: the groups frozen by tick 100 are
    restarted there. NewNode's follower timer is 3 + rand % 1 at 1 s per
    tick, not the default 10 + rand % 20 at 2 s."""
    kw = TC.config("unit", "hashed", TC.REF)
    e, o = pair(**kw)
    e.init_new_nodes(0)
    o.init_new_nodes(0)
    assert list(e.tick(0, 100)) == list(o.tick(0, 100, threads=4))
    compare(e, o, "after 100 ticks")
    ids = np.nonzero(o.store_state(logs=False)["fault"] != 0)[0]
    assert len(ids) >= 10, "the run froze too few groups to restart"
    hits, _ = e.group_scan(abi.SELECT_FAULTED)
    assert np.array_equal(hits["local"], ids)
    e.restart_groups(ids, 100)
    GM.restart(o, ids, 100)
    st = e.store_state()
    H.assert_same_state(st, o.store_state(), "right after the restart")
    assert (st["timeout"][ids] == 3).all() and (st["deadline"][ids] == 100 * 1 + 3).all()
    assert (st["role"][ids] == abi.FOLLOWER).all() and (st["fault"][ids] == 0).all()
    assert list(e.tick(100, 10)) == list(o.tick(100, 10, threads=4))
    compare(e, o, "10 ticks after the restart")
    _digests(e, o, "10 ticks after the restart")


# ---- f. a checkpoint of another timing configuration ---------------------------------------

ONE_FIELD_OFF = [("tick_seconds", 4, "tick_seconds"),
                 ("follower_timeout_min", 6, "follower timeout range"),
                 ("follower_timeout_span", 12, "follower timeout range"),
                 ("candidate_timeout_min", 5, "candidate timeout range"),
                 ("candidate_timeout_span", 8, "candidate timeout range")]


def test_checkpoint_of_another_timing_is_refused(tmp_path):
    """A checkpoint saved at `odd` is refused by an engine that differs in
    exactly one of the five timing fields, by name, and that engine, in the
    steady form with shared entries when the call comes, keeps its state."""
    kw = dict(TC.TIMINGS["odd"], replicas=3, groups=300, ring_depth=16, client_period=1, seed=0x71F)
    path = os.path.join(tmp_path, "odd.ckpt")
    src = Engine(**kw)
    src.init_steady(0, 0)
    src.tick(1, 11)
    src.save_checkpoint(path)
    for field, value, named in ONE_FIELD_OFF:
        assert kw[field] != value
        kw2 = dict(kw, **{field: value})
        e, o = pair(**kw2)
        e.init_steady(0, 0)
        o.init_steady(0, 0)
        e.tick(1, 6)
        e.tick(7, 5)
        o.tick(1, 11)
        assert _steady(e) == 5
        msg =_refused(abi.RAFT_EINVAL, e.load_checkpoint, path)
        assert named in msg, msg
        _digests(e, o, f"after the refused checkpoint ({field})")
        compare(e, o, f"after the refused checkpoint ({field})")
    same = Engine(**kw)
    same.load_checkpoint(path)
    d, s = same.state_digest(), src.state_digest()
    assert np.array_equal(d[0], s[0]) and d[1] == s[1]


# ---- g. the end of virtual time off the defaults --------------------------------------------

END = dict(tick_seconds=1000, follower_timeout_min=1, follower_timeout_span=1023, candidate_timeout_min=1000,
           candidate_timeout_span=24)
LONGEST = 1024                                # the longer timer range's end, min + span
FIRST = (I - LONGEST) // 1000 - 30            # the largest FIRST with (FIRST + 30) * 1000 + 1024 <= 2^31 - 1
LAST_TICK = (I - LONGEST) // 1000             # the largest tick with tick * 1000 + 1024 <= 2^31 - 1


def test_virtual_time_ends_where_check_ticks_says():
    assert (FIRST + 30) * 1000 + LONGEST <= I < (FIRST + 31) * 1000 + LONGEST
    kw = dict(END, replicas=3, groups=300, client_period=1, seed=0x71CE)
    e, o = pair(**kw)
    e.init_new_nodes(FIRST - 1)
    o.init_new_nodes(FIRST - 1)
    assert list(e.tick(FIRST, 30)) == list(o.tick(FIRST, 30))
    compare(e, o, "after the last 30 ticks of virtual time")
    so = o.store_state(logs=False)
    assert (so["role"] == abi.LEADER).any() and so["deadline"].max() > I - 2000
    before = e.state_digest()
    _refused(abi.RAFT_ERANGE, e.tick, FIRST + 1, 30)
    after = e.state_digest()
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]


def test_every_tick_taking_call_refuses_a_tick_past_the_end():
    """init_steady, init_new_nodes, restart_groups, propose and a handler
    batch at LAST_TICK + 1, the first tick whose now + the longest timer
    leaves int32: RAFT_ERANGE, and the state, in the steady form with shared
    entries when each call comes, stays what the oracle holds."""
    assert LAST_TICK * 1000 + LONGEST <= I < (LAST_TICK + 1) * 1000 + LONGEST
    kw = dict(END, replicas=3, groups=300, ring_depth=16, client_period=1, seed=0x71CF)
    bad = LAST_TICK + 1
    e, o = pair(**kw)
    t0 = LAST_TICK - 60
    e.init_steady(0, t0)
    o.init_steady(0, t0)
    t = _call(e, o, t0 + 1, 6)
    calls = [("init_steady", lambda: e.init_steady(0, bad)),
             ("init_new_nodes", lambda: e.init_new_nodes(bad)),
             ("restart_groups", lambda: e.restart_groups([0, 7], bad)),
             ("propose", lambda: e.propose(bad, [0, 7], [1, 2])),
             ("request_vote", lambda: e.request_vote(bad, H.vote_reqs([dict(group=3, to=1, term=9)]))),
             ("group_ops", lambda: e.group_ops(bad, H.ops([dict(group=3, replica=0, kind=abi.OP_TIMEOUT)])))]
    for what, call in calls:
        t = _call(e, o, t, 3)
        # (no host read between these ticks and the call: shared entries and their implied heartbeat time are live)
        assert list(e.tick(t, 2)) == list(o.tick(t, 2))
        t += 2
        _refused(abi.RAFT_ERANGE, call)
        _digests(e, o, f"after the refused {what}")
        compare(e, o, f"after the refused {what}")
    t = _call(e, o, t, 4)
    compare(e, o, "at the end")


# ---- h. the checks at creation ---------------------------------------------------------------

def test_creation_checks_the_timing_fields():
    base = dict(replicas=3, groups=4)
    for field in TC.TIMING_FIELDS:
        for v in (0, -1):
            _refused(abi.RAFT_EINVAL, lambda: Engine(**dict(base, **{field: v})))
    for rng in ("follower", "candidate"):
        mn, sp = f"{rng}_timeout_min", f"{rng}_timeout_span"
        for a, b in ((1, 1023), (1023, 1), (511, 513)):
            Engine(**dict(base, **{mn: a, sp: b})).close()                  # min + span == 1024: the field's top
        for a, b in ((1, 1024), (1024, 1), (512, 513)):
            _refused(abi.RAFT_EINVAL, lambda: Engine(**dict(base, **{mn: a, sp: b})))
        # the sum leaves int32: it must not wrap back into range
        for a, b in ((I, 1), (1, I), (I, I), (I - 1023, 1025 + 1023)):
            _refused(abi.RAFT_EINVAL, lambda: Engine(**dict(base, **{mn: a, sp: b})))
    # tick_seconds = 2^31-1 is a valid configuration; check_ticks refuses a call when (first + n) * tick_seconds +
    # the longest timer reaches 2^31 - 1: (0 + 1) * (2^31 - 1) + 30 does, so not even tick 0 can run
    e = Engine(**dict(base, tick_seconds=I))
    _refused(abi.RAFT_ERANGE, e.tick, 0, 1)
    _refused(abi.RAFT_ERANGE, e.init_new_nodes, 0)
