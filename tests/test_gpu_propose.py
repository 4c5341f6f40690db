"""GPU: client proposals (raft_propose / raft_ticket_status; propose_kernel in
k_slow.inc, ticket_status_kernel in k_propose.hip). Every case drives an engine
and the oracle alike; the tickets are compared with tests/propose_model.py's
(CLIENT_APPEND batches on the oracle), the results with its numpy model of the
header's rules over a canonical view. Anchors: main.go:87-93 (the client sends
LogReq to every Leader), 327-329 (LogReq), 330 (answer once CommitIndex has
advanced)."""
import ctypes as C

import numpy as np
import pytest

import bench
import harness as H
import oracle
import propose_model as PM
from raftstep import Engine, RaftError, abi

pytestmark = pytest.mark.gpu
THREADS = 16
G = 577   # two full blocks and a partial one
I = H.I32
STEADY = dict(replicas=5, groups=G, ring_depth=16, entries_per_tick=1, client_period=1, seed=0x5EED0002, group_base=4000)
NAMES = abi.TICKET_STATE_NAMES


def _pair(kw):
    return Engine(**kw), oracle.Oracle(**kw)


def _same_state(e, o, what):
    H.assert_same_state(e.store_state(), o.store_state(), what)
    de, do = e.state_digest(), o.state_digest()
    assert np.array_equal(de[0], do[0]) and de[1] == do[1], f"{what}: digests differ"


def _same_records(got, want, what):
    assert got.dtype == want.dtype and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {bad.size} of {len(got)} records differ, first at {int(bad[0])}: "
                             f"engine {got[bad[0]]}, model {want[bad[0]]}")


def _propose_both(e, o, t, ids, vals, what):
    got = e.propose(t, ids, vals)
    want = PM.propose(o, t, ids, vals)
    _same_records(got, want, what)
    return got


def _tick_both(e, o, t, k):
    se, so = e.tick(t, k), o.tick(t, k, threads=THREADS)
    assert list(se) == list(so), f"stats of ticks [{t}, {t + k}): engine {list(se)}, oracle {list(so)}"
    return t + k


def _status_both(e, view, tickets, what):
    """Engine results and counts against the model over `view`; count-only gives the same counts."""
    want, per = PM.ticket_status(view, e.cfg, tickets)
    got, gper = e.ticket_status(tickets)
    _same_records(got, want, what)
    assert gper == per, f"{what}: per_state {gper}, model {per}"
    none, cper = e.ticket_status(tickets, results=False)
    assert none is None and cper == per, f"{what}: count-only {cper}, model {per}"
    return want, per


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("period", [0, 1])
@pytest.mark.parametrize("R", [3, 5])
@pytest.mark.parametrize("sem", [abi.SEM_REF, abi.SEM_RAFT], ids=["ref", "raft"])
def test_propose_against_the_oracle(sem, R, period):
    K = 8
    rng = np.random.default_rng(100 + 10 * sem + R)
    e, o = _pair(dict(replicas=R, groups=G, ring_depth=K, semantics=sem, client_period=period, seed=0xC11E + R,
                      group_base=1 << 33))
    st = H.random_state(rng, G, R, K)
    st["fault"][:] = np.where(rng.integers(0, 10, G) == 0, rng.integers(1, 6, G), 0)
    nlead = (st["role"] == abi.LEADER).sum(axis=1)
    live = st["fault"] == 0
    assert (live & (nlead >= 2)).sum() > 20 and (live & (nlead == 0)).sum() > 20 and (~live).sum() > 20
    e.load_state(st)
    o.load_state(st)
    hot = int(np.flatnonzero(live & (nlead >= 1))[3])
    ids = np.concatenate([rng.permutation(G), rng.integers(0, G, 2000 - G - (K + 3)), np.full(K + 3, hot)])
    ids = ids[rng.permutation(len(ids))]
    vals = rng.integers(-(1 << 62), 1 << 62, len(ids))
    tk = _propose_both(e, o, 5, ids, vals, "tickets")
    counts = {k: int((tk["status"] == s).sum()) for s, k in enumerate(("none", "accepted", "no_leader", "frozen"))}
    print("propose:", counts, "two or more leaders:", int((tk["leaders"] & (tk["leaders"] - 1) != 0).sum()))
    assert counts["none"] == 0 and min(counts["accepted"], counts["no_leader"], counts["frozen"]) > 50
    hot_idx = tk["index"][ids == hot]
    assert len(hot_idx) >= K + 3 and (np.diff(hot_idx) == 1).all()     # list order, past the ring's depth
    _same_state(e, o, "after the propose")
    _tick_both(e, o, 5, 12)
    _same_state(e, o, "12 ticks after the propose")


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("raft", [False, True], ids=["ref", "raft"])
def test_status_against_the_model(raft):
    st, cfg, tickets = PM.coverage_inputs(raft)
    e = Engine(cfg)
    e.load_state(st)
    view = e.store_state()
    assert np.array_equal(view["hwm"], st["hwm"]) and np.array_equal(view["last"], st["last"])
    for n in (1, 255, 256, 257, len(tickets)):
        _, per = _status_both(e, view, tickets[:n], f"first {n} tickets")
    print("per state:", per)
    assert all(per[k] >= 10 for k in NAMES)
    # any order, repeats allowed
    pick = np.random.default_rng(5).integers(0, len(tickets), 700)
    _status_both(e, view, tickets[pick], "shuffled with repeats")


# 3 ------------------------------------------------------------------------
def _forms_case(kw, how, first_ticks, feature):
    e, o = _pair(kw)
    getattr(e, how[0])(*how[1:])
    getattr(o, how[0])(*how[1:])
    assert e.features()[feature]
    t = how[-1] + (1 if how[0] == "init_steady" else 0)
    for k in first_ticks:
        t = _tick_both(e, o, t, k)
    rng = np.random.default_rng(31)
    ids = rng.permutation(G)[:300]
    rows = e.store_groups(ids)                 # (the directory's read: nothing is flushed)
    tickets = PM.tickets_near_last(rng, rows, e.cfg, ids)
    got, gper = e.ticket_status(tickets)       # ... so this reads the forms the ticks left
    want, per = PM.ticket_status(o.store_state(), e.cfg, tickets)
    print(feature, "per state:", per)
    _same_records(got, want, f"{feature}: results")
    assert gper == per
    assert min(per["committed"], per["superseded"], per["evicted"], per["dropped"]) >= 20   # (of 1800, not empty)
    pids = np.concatenate([ids[:200], ids[:50], rng.integers(0, G, 100)])
    _propose_both(e, o, t, pids, rng.integers(0, 1 << 62, len(pids)), f"{feature}: tickets")
    _same_state(e, o, f"{feature}: after the propose")
    t = _tick_both(e, o, t, 6)
    _same_state(e, o, f"{feature}: 6 ticks after the propose")


def test_every_storage_form_steady_shared():
    _forms_case(STEADY, ("init_steady", -1, 0), (1, 7, 13), "shared_entries")


def test_every_storage_form_raft_leader_isolation():
    wl = bench.WORKLOADS["C4"]
    kw = bench.engine_kwargs(wl, 7, G, 0, 16, 1, 0)    # (K = 16: entries leave the rings within the 58 ticks)
    kw["isolate_per_65536"] = 4 * wl["iso"][0]
    _forms_case(kw, ("init_new_nodes", 0), (48, 5, 5), "virtual_suffixes")


# 4 ------------------------------------------------------------------------
def test_status_does_not_disturb():
    a, b = Engine(**STEADY), Engine(**STEADY)
    for x in (a, b):
        x.init_steady(-1, 0)
        x.feed_open(start="commit")
        x.diag_read()
    rng = np.random.default_rng(41)
    t, calls = 1, 0
    for k in (1, 7, 5, 6):
        a.tick(t, k)
        b.tick(t, k)
        t += k
        if calls < 3:
            cur = a.feed_cursors()
            ids = rng.permutation(G)[:200]
            tickets = PM.tickets_near_last(rng, a.store_groups(ids), a.cfg, ids)
            first = a.ticket_status(tickets)
            again = a.ticket_status(tickets)
            assert first[0].tobytes() == again[0].tobytes() and first[1] == again[1]   # same state, same bytes
            assert np.array_equal(a.feed_cursors(), cur)
            b.feed_cursors(), b.store_groups(ids), b.feed_cursors()   # (the twin makes every other call too)
            calls += 1
    assert calls == 3
    ca, cb = a.diag_read(), b.diag_read()
    print("status twin:", {k: ca[k] for k in ("ticks", "ticks_steady_form", "ticks_list_skipped")})
    assert ca["ticks_steady_form"] == cb["ticks_steady_form"] > 0
    assert ca["ticks_list_skipped"] == cb["ticks_list_skipped"]
    assert np.array_equal(a.feed_cursors(), b.feed_cursors())
    assert np.array_equal(a.state_digest()[0], b.state_digest()[0])
    for g in (0, 63, 64, 255, 256, G - 1):
        assert a.debug_group_words(g) == b.debug_group_words(g), g


# 5 ------------------------------------------------------------------------
def test_propose_ends_the_steady_form_and_keeps_the_feed():
    a, b = Engine(**STEADY), Engine(**STEADY)
    for x in (a, b):
        x.init_steady(-1, 0)
        x.feed_open(start="commit")
        x.tick(1, 1)
        x.tick(2, 6)
        x.diag_read()
    t = 8
    assert len(a.propose(t, [], [])) == 0           # n = 0: nothing changes, the proofs included
    for x in (a, b):
        x.tick(t, 5)
    t += 5
    ca, cb = a.diag_read(), b.diag_read()
    assert ca["ticks_steady_form"] == cb["ticks_steady_form"] > 0 and ca["ticks_list_skipped"] == 5
    cur = a.feed_cursors()
    assert np.array_equal(cur, b.feed_cursors())
    ids = np.random.default_rng(51).permutation(G)[:100]
    tk = a.propose(t, ids, np.arange(100))
    assert (tk["status"] == abi.PROPOSE_ACCEPTED).all() and len(set(tk["index"].tolist())) == 1   # (in step)
    assert np.array_equal(a.feed_cursors(), cur)    # the feed stays open, no cursor moves
    rest = np.setdiff1d(np.arange(G), ids)
    ra, rb = a.store_groups(rest), b.store_groups(rest)
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), f"untouched groups: {k}"
    for x in (a, b):
        x.tick(t, 5)
    ca, cb = a.diag_read(), b.diag_read()
    assert ca["ticks_steady_form"] == 0 and ca["ticks_list_skipped"] == 0
    assert cb["ticks_steady_form"] > 0 and cb["ticks_list_skipped"] == 5
    ra, rb = a.store_groups(rest), b.store_groups(rest)
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), f"untouched groups after 5 more ticks: {k}"


# 6 ------------------------------------------------------------------------
def test_the_loop_closes():
    """RAFT under leader isolation (committed entries are never rewritten), the
    feed open from the start on every replica: at the end bit r of a ticket's
    `committed` is set exactly when the feed delivered (group, r, index) with
    the ticket's term and value."""
    kw = dict(replicas=5, groups=G, ring_depth=64, seed=0x47, semantics=1, client_period=1, isolate_leader=1,
              isolate_per_65536=20000, isolate_min_ticks=4, isolate_max_ticks=16, group_base=70000)
    e, o = _pair(kw)
    e.init_new_nodes(0)
    o.init_new_nodes(0)
    e.feed_open(start="start")
    fed = {}

    def poll():
        ents, info = e.feed_poll()
        assert info["lost"] == 0
        for x in ents:
            fed[(int(x["group"]), int(x["replica"]), int(x["index"]))] = (int(x["term"]), int(x["value"]))

    t = _tick_both(e, o, 0, 40)
    poll()
    rng = np.random.default_rng(61)
    ids = np.concatenate([rng.permutation(G), rng.integers(0, G, 123)])
    tickets = _propose_both(e, o, t, ids, rng.integers(0, 1 << 62, len(ids)), "tickets")
    seen = dict.fromkeys(NAMES, 0)
    for _ in range(10):
        want, per = PM.ticket_status(o.store_state(), e.cfg, tickets)
        for k in NAMES:
            seen[k] += per[k]
        t = _tick_both(e, o, t, 1)
        poll()
    want, per = PM.ticket_status(o.store_state(), e.cfg, tickets)
    print("tickets over 10 ticks:", seen, "at the end:", per)
    assert seen["committed"] > 0 and seen["pending"] > 0 and per["committed"] > 100
    got, gper = e.ticket_status(tickets)
    _same_records(got, want, "results at the end")
    assert gper == per
    for tk, res in zip(tickets, got):
        for r in range(kw["replicas"]):
            have = fed.get((int(tk["group"]), r, int(tk["index"]))) == (int(tk["term"]), int(tk["value"]))
            assert have == bool(res["committed"] >> r & 1), (tk, res, r)


# 7 ------------------------------------------------------------------------
def test_proposed_entries_carry_their_stamp():
    kw = dict(STEADY, replicas=3, entries_per_tick=4, payload_crc=1)
    e, o = _pair(kw)
    e.init_steady(-1, 0)
    o.init_steady(-1, 0)
    t = _tick_both(e, o, 1, 6)
    before = set(e.group_audit(abi.AUDIT_STAMP)[0]["local"].tolist())
    rng = np.random.default_rng(71)
    ids = np.concatenate([rng.permutation(G)[:400], np.full(20, 9)])     # group 9 wraps its ring (K = 16)
    tk = _propose_both(e, o, t, ids, rng.integers(-(1 << 63), 1 << 63, len(ids)), "tickets")
    assert (tk["status"] == abi.PROPOSE_ACCEPTED).all()
    hits, info = e.group_audit(abi.AUDIT_STAMP)
    assert not (set(hits["local"].tolist()) - before) & set(ids.tolist()), info
    assert np.array_equal(e.store_state()["log_crc"], o.store_state()["log_crc"])


# 8 ------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [abi.SEM_REF, abi.SEM_RAFT], ids=["ref", "raft"])
def test_the_ceiling(sem):
    R, K, n = 3, 8, 300
    rng = np.random.default_rng(80 + sem)
    e, o = _pair(dict(replicas=R, groups=n, ring_depth=K, semantics=sem, seed=0xCE1))
    st = H.ceiling_state(rng, n, R, K, raft=sem == abi.SEM_RAFT)
    st["last"][:] = rng.choice([I - 1, I], (n, R))
    e.load_state(st)
    o.load_state(st)
    ids = np.concatenate([np.arange(n), rng.permutation(n)])        # two proposals each
    tk = _propose_both(e, o, 3, ids, rng.integers(0, 1 << 62, len(ids)), "tickets at the ceiling")
    assert ((tk["status"] == abi.PROPOSE_FROZEN) & (tk["fault"] == abi.F_OVERFLOW)).sum() > 50
    assert ((tk["status"] == abi.PROPOSE_ACCEPTED) & (tk["index"] == I)).sum() > 50
    assert ((tk["status"] == abi.PROPOSE_ACCEPTED) & (tk["fault"] == abi.F_OVERFLOW)).sum() > 5
    _same_state(e, o, "after the proposals at the ceiling")
    _status_both(e, e.store_state(), tk, "status at the ceiling")


# 9 ------------------------------------------------------------------------
def _steady_engine():
    e = Engine(**STEADY)
    e.init_steady(-1, 0)
    e.tick(1, 6)
    e.tick(7, 5)
    return e


def test_errors_leave_the_state_alone():
    e = _steady_engine()
    before = e.state_digest()[0]
    good = e.propose(12, [3, 4], [1, 2])
    after_good = e.state_digest()[0]
    assert (good["status"] == abi.PROPOSE_ACCEPTED).all() and not np.array_equal(before, after_good)

    def code(call):
        with pytest.raises(RaftError) as ei:
            call()
        return ei.value.code

    assert code(lambda: e.propose(12, [3, G], [1, 2])) == abi.RAFT_ERANGE
    assert code(lambda: e.propose(12, [1 << 63], [1])) == abi.RAFT_ERANGE
    assert code(lambda: e.propose(-1, [3], [1])) == abi.RAFT_ERANGE
    assert code(lambda: e.propose(1 << 40, [3], [1])) == abi.RAFT_ERANGE
    props, out = np.zeros(2, abi.PROPOSAL), np.zeros(2, abi.TICKET)
    lib, h = e.lib, e.h
    assert lib.raft_propose(h, 12, None, 2, out.ctypes.data) == abi.RAFT_EINVAL
    assert lib.raft_propose(h, 12, props.ctypes.data, 2, None) == abi.RAFT_EINVAL
    assert lib.raft_propose(None, 12, props.ctypes.data, 2, out.ctypes.data) == abi.RAFT_EINVAL
    assert lib.raft_propose(h, 12, props.ctypes.data, (1 << 31) + 1, out.ctypes.data) == abi.RAFT_EINVAL
    assert not out.view(np.uint8).any()
    # tickets: a local id outside the engine, another shard's ticket, null arguments, both outputs null
    res, info = np.zeros(2, abi.TICKET_RESULT), abi.TicketInfo()
    bad = good.copy()
    bad["local"][1] = G
    assert code(lambda: e.ticket_status(bad)) == abi.RAFT_ERANGE
    bad = good.copy()
    bad["group"][1] += 1
    assert code(lambda: e.ticket_status(bad)) == abi.RAFT_EINVAL
    tk = good.ctypes.data
    assert lib.raft_ticket_status(h, None, 2, res.ctypes.data, C.byref(info)) == abi.RAFT_EINVAL
    assert lib.raft_ticket_status(h, tk, 2, None, None) == abi.RAFT_EINVAL
    assert lib.raft_ticket_status(None, tk, 2, res.ctypes.data, C.byref(info)) == abi.RAFT_EINVAL
    assert lib.raft_ticket_status(h, tk, (1 << 31) + 1, res.ctypes.data, C.byref(info)) == abi.RAFT_EINVAL
    assert not res.view(np.uint8).any() and not any(info.per_state)
    # either output alone is enough; n = 0 is an empty answer
    assert lib.raft_ticket_status(h, tk, 2, res.ctypes.data, None) == 0
    assert lib.raft_ticket_status(h, tk, 2, None, C.byref(info)) == 0
    assert list(res["state"]) == [abi.TICKET_PENDING] * 2 and list(info.per_state) == [0, 0, 2, 0, 0, 0, 0, 0]
    assert e.ticket_status(good[:0])[1] == dict.fromkeys(NAMES, 0)
    assert np.array_equal(e.state_digest()[0], after_good)


def test_a_poisoned_engine_answers_einternal():
    e = _steady_engine()
    tickets = e.propose(12, [1], [5])
    e.init_steady(-1, 0)
    e.tick(1, 6)
    e.tick(7, 5)
    e.debug_force_pass(42)     # a group passed to a list kernel that does not run: ticks lost, the engine says so
    with pytest.raises(RaftError, match="list kernel that did not run"):
        e.tick(12, 4)
    for call in (lambda: e.propose(16, [1], [5]), lambda: e.ticket_status(tickets)):
        with pytest.raises(RaftError, match="engine state is invalid") as ei:
            call()
        assert ei.value.code == abi.RAFT_EINTERNAL
