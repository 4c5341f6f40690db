"""GPU: the group audit (raft_group_audit; k_audit.hip). The checker is the
numpy model (tests/audit_model.py) over the loaded state, over the oracle's
state next to the engine, and over Engine.store_state(). G = 1101 unless a
case says otherwise: four blocks plus a ragged 77-lane tail. The hand-derived
states and their expected records are tests/test_audit_model.py's. (The file
name: tests/test_gpu_audit.py is taken by the digest / nodelog / checkpoint
surface.) Anchors: nodelog (main.go:399-401), a follower's CommitIndex =
min(LeaderCommit, LastApplied + 1) (main.go:152)."""
import ctypes as C

import numpy as np
import pytest

import audit_model as AM
import feed_model as FM
import groups_model as GM
import harness as H
import oracle
import test_audit_model as TM
from raftstep import Engine, RaftError, abi

pytestmark = pytest.mark.gpu
THREADS = 16
G = 1101
BASE = 70000
CHECKS = (1, 2, 4, 8, 16, 32, abi.AUDIT_ALL)
LOG_BITS = abi.AUDIT_LOG_MATCHING | abi.AUDIT_COMMIT_DIVERGED | abi.AUDIT_TERM_ORDER | abi.AUDIT_STAMP

# tests/test_gpu_groups.py's configurations
REF = dict(replicas=3, groups=G, ring_depth=64, entries_per_tick=1, client_period=1, seed=0x5EED0001,
           isolate_per_65536=8000, isolate_min_ticks=4, isolate_max_ticks=16, group_base=5000)
STEADY_A = dict(replicas=5, groups=G, ring_depth=16, entries_per_tick=1, client_period=1, seed=0x5EED0002)
STEADY_B = dict(STEADY_A, replicas=3, entries_per_tick=4, payload_crc=1)
STEADY_C = dict(replicas=5, groups=G, entries_per_tick=16, ring_depth=64, payload_crc=1, corrupt_per_65536=3000,
                client_period=1, seed=0x5EED0005)
STEADY_CALLS = (1, 7, 1, 13, 19)   # 40 ticks in all (K = 16: the ring wraps twice)


def _pair(kw, how, *a):
    e, o = Engine(**kw), oracle.Oracle(**kw)
    getattr(e, how)(*a)
    getattr(o, how)(*a)
    return e, o


def _tick(e, o, t, k):
    se, so = e.tick(t, k), o.tick(t, k, threads=THREADS)
    assert list(se) == list(so), f"stats of ticks [{t}, {t + k}): engine {list(se)}, oracle {list(so)}"
    return t + k


def _same(got, want, what):
    (gh, gi), (wh, wi) = got, want
    assert gi == wi, f"{what}: info {gi}, model {wi}"
    if gh.tobytes() != wh.tobytes():
        bad = [i for i in range(len(gh)) if gh[i] != wh[i]][:3]
        raise AssertionError(f"{what}: hits differ, first {[(gh[i], wh[i]) for i in bad]}")
    assert gh.dtype == abi.AUDIT_HIT


def _crc(e):
    return bool(e.cfg.payload_crc)


def _all_equal_model(e, st, what):
    """ALL and every single check, uncapped, against the model over st; returns the model's info for ALL."""
    table = AM.evaluate(st, _crc(e))
    base = int(e.cfg.group_base)
    for checks in CHECKS:
        _same(e.group_audit(checks), AM.audit(st, checks, 0, None, base, table=table), f"{what}: checks {checks}")
    return AM.audit(st, abi.AUDIT_ALL, 0, None, base, table=table)[1]


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("R,K,raft", [(3, 8, 0), (5, 16, 0), (8, 8, 0), (1, 8, 0), (3, 8, 1)],
                         ids=["r3k8", "r5k16", "r8k8", "r1", "raft_r3k8"])
def test_dense_loaded_states(R, K, raft):
    rng = np.random.default_rng(11)
    st = H.random_state(rng, G, R, K, max_log=12 if K == 8 else 40)   # (logs past the ring's wrap)
    e = Engine(replicas=R, groups=G, ring_depth=K, group_base=BASE, semantics=raft)
    e.load_state(st)
    before = e.state_digest()[0]
    table = AM.evaluate(st)
    for checks in CHECKS:
        for first in (0, 200, 256, G - 1, G):
            _, winfo = AM.audit(st, checks, first, None, BASE, table=table)
            m = winfo["matched"]
            for cap in (0, 1, 70, m, m + 5):
                what = f"checks {checks} first_group {first} cap {cap}"
                _same(e.group_audit(checks, first, cap), AM.audit(st, checks, first, cap, BASE, table=table), what)
            _same(e.group_audit(checks, first), AM.audit(st, checks, first, None, BASE, table=table),
                  f"checks {checks} first_group {first}, counted")
        whole, winfo = AM.audit(st, checks, 0, None, BASE, table=table)   # paging with cap 33 reassembles the list
        pages, first = [], 0
        while first < G:
            hits, info = e.group_audit(checks, first, 33)
            assert info["written"] == min(33, info["matched"])
            pages.append(hits)
            first = info["next_group"]
        assert np.concatenate(pages).tobytes() == whole.tobytes(), f"checks {checks}: paging"
    print(f"R={R} K={K} raft={raft}: ALL hits", winfo["matched"], winfo["per_check"])
    assert winfo["matched"] > (0.9 * G if R > 1 else 0.5 * G)
    assert np.array_equal(e.state_digest()[0], before)


# 2 ------------------------------------------------------------------------
def _stamped_rows():
    """random_state rows with right stamps, then flipped ones in a seeded tenth of the groups: at the low end
    of a replica's window, at its last entry and at the entry in slot 0 (where the ring wraps)."""
    K = 8
    rng = np.random.default_rng(21)
    st = H.stamp_crcs(H.random_state(rng, G, 3, K))
    flipped = 0
    for g in np.nonzero(rng.random(G) < 0.10)[0]:
        r = int(rng.integers(0, 3))
        last = int(st["last"][g, r])
        if last == 0:
            continue
        lo = max(1, last - K + 1)
        wrap = [i for i in range(lo, last + 1) if (i - 1) % K == 0]
        where = {lo, last} if g % 3 == 0 else {wrap[0] if wrap else last} if g % 3 == 1 else {last}
        for i in sorted(where):
            st["log_crc"][g, r, (i - 1) % K] ^= np.uint32(1 << int(rng.integers(0, 32)))
            flipped += 1
    return st, flipped


def test_stamps():
    st, flipped = _stamped_rows()
    e = Engine(replicas=3, groups=G, ring_depth=8, group_base=BASE, payload_crc=1)
    e.load_state(st)
    table = AM.evaluate(st, True)
    want = AM.audit(st, abi.AUDIT_STAMP, 0, None, BASE, table=table)
    print("flipped stamps:", flipped, "STAMP hits:", want[1]["matched"])
    assert 0.05 * G <= want[1]["matched"] <= 0.15 * G
    _same(e.group_audit(abi.AUDIT_STAMP), want, "STAMP")
    _same(e.group_audit(), AM.audit(st, abi.AUDIT_ALL, 0, None, BASE, table=table), "ALL with stamps")
    plain = Engine(replicas=3, groups=G, ring_depth=8, group_base=BASE)
    plain.load_state(st)
    hits, info = plain.group_audit(abi.AUDIT_STAMP)
    assert len(hits) == 0 and info["matched"] == 0 and info["per_check"]["stamp"] == 0
    _same(plain.group_audit(), AM.audit(st, abi.AUDIT_ALL, 0, None, BASE), "ALL without payload_crc")


# 3 ------------------------------------------------------------------------
def _inject_and_check(e, seed, what):
    """A seeded tenth of the groups replaced by random_state rows through load_groups."""
    R, K = e.cfg.replicas, e.cfg.ring_depth
    rng = np.random.default_rng(seed)
    sick = np.nonzero(rng.random(G) < 0.10)[0]
    rows = H.random_state(rng, len(sick), R, K, max_log=12 if K == 8 else 2 * K + 8)
    e.load_groups(sick, rows)
    info = _all_equal_model(e, e.store_state(), f"{what}: after the injection")
    print(what, ": injected", len(sick), "rows,", info["matched"], "hits", info["per_check"])
    assert 0.05 * G <= info["matched"] <= 0.15 * G


@pytest.mark.parametrize("kw", [STEADY_A, STEADY_B, STEADY_C], ids=["a", "b", "c"])
def test_real_ticks_steady_shared(kw):
    e, o = _pair(kw, "init_steady", -1, 0)
    assert e.features()["shared_entries"]
    e.diag_read()
    t = 1
    for k in STEADY_CALLS:
        t = _tick(e, o, t, k)
    info = _all_equal_model(e, o.store_state(), "steady, tick 40 (entries in the shared ring)")
    c = e.diag_read()
    print("steady E =", kw["entries_per_tick"], ": hits", info["matched"], "ticks_steady_form", c["ticks_steady_form"],
          "ticks_list_skipped", c["ticks_list_skipped"])
    if kw is not STEADY_C:
        assert c["ticks_steady_form"] > 0 and c["ticks_list_skipped"] > 0
    assert info["matched"] == 0
    H.assert_same_state(e.store_state(), o.store_state(), "after the audits")
    _inject_and_check(e, 31, "steady")


def test_real_ticks_ref_churn():
    e, o = _pair(REF, "init_new_nodes", 0)
    _tick(e, o, 0, 60)
    info = _all_equal_model(e, o.store_state(), "REF churn, tick 60")
    print("REF churn, tick 60: hits", info["matched"], info["per_check"])
    _inject_and_check(e, 32, "REF churn")


def test_real_ticks_raft_churn():
    kw = dict(REF, semantics=1)
    e, o = _pair(kw, "init_new_nodes", 0)
    t = 0
    for upto in (20, 40):
        t = _tick(e, o, t, upto - t)
        info = _all_equal_model(e, o.store_state(), f"RAFT churn, tick {upto}")
        print("RAFT churn, tick", upto, ": hits", info["matched"], info["per_check"])
        assert info["matched"] == 0
    _inject_and_check(e, 33, "RAFT churn")


# 4 ------------------------------------------------------------------------
def test_looking_changes_nothing():
    """Two engines on STEADY_A run the same calls; one audits between them
    (ALL, the scalar checks alone, a capped page). Same digests, same steady
    form and list skips; the oracle runs the same ticks."""
    a, b, o = Engine(**STEADY_A), Engine(**STEADY_A), oracle.Oracle(**STEADY_A)
    o.init_steady(-1, 0)
    for x in (a, b):
        x.init_steady(-1, 0)
        x.diag_read()
    bytes_before = a.device_bytes()
    t = 1
    for k in STEADY_CALLS:
        a.tick(t, k)
        b.tick(t, k)
        o.tick(t, k, threads=THREADS)
        t += k
        for checks, cap in ((abi.AUDIT_ALL, None), (abi.AUDIT_TWO_LEADERS | abi.AUDIT_COMMIT_BEYOND_LOG, None),
                            (LOG_BITS, 5)):
            hits, info = a.group_audit(checks, cap=cap)
            assert info["matched"] == 0 and len(hits) == 0
        assert np.array_equal(a.state_digest()[0], o.state_digest()[0])
    ca, cb = a.diag_read(), b.diag_read()
    print("looking:", {k: ca[k] for k in ("ticks", "ticks_steady_form", "ticks_list_skipped")})
    for k in ("ticks", "ticks_steady_form", "ticks_list_skipped", "general_launches"):
        assert ca[k] == cb[k], (k, ca[k], cb[k])
    assert ca["ticks_list_skipped"] > 0 and ca["ticks_steady_form"] > 0
    assert a.device_bytes() == bytes_before + 8 * G and b.device_bytes() == bytes_before   # the scratch, once
    assert np.array_equal(a.state_digest()[0], b.state_digest()[0])
    H.assert_same_state(a.store_state(), o.store_state(), "the auditing engine vs the oracle")


def test_looking_changes_nothing_shared_tick_counters_and_feed():
    """The same with the device lane counters on (the shared-tick count) and a feed open on both engines:
    equal cursors and equal next polls."""
    a, b, o = Engine(**STEADY_A), Engine(**STEADY_A), oracle.Oracle(**STEADY_A)
    o.init_steady(-1, 0)
    fed = [0, 2]
    for x in (a, b):
        x.init_steady(-1, 0)
        x.diag_read()
        x.diag_enable()
        x.feed_open(fed, "start")
    cur = FM.start_cursors(o.store_state(), fed, "start")
    t = 1
    for k in STEADY_CALLS:
        a.tick(t, k)
        b.tick(t, k)
        o.tick(t, k, threads=THREADS)
        t += k
        assert a.group_audit()[1]["matched"] == 0
        assert np.array_equal(a.feed_cursors(), b.feed_cursors())
        if k == 13:
            want, winfo, cur = FM.poll(o.store_state(), cur, None, 0)
            for x in (a, b):
                got, ginfo = x.feed_poll()
                assert ginfo == winfo and got.tobytes() == want.tobytes()
            assert a.group_audit(LOG_BITS)[1]["matched"] == 0
    ca, cb = a.diag_read(), b.diag_read()
    for k in ("ticks", "ticks_list_skipped", "lean_sh", "list_sh_copied"):
        assert ca[k] == cb[k], (k, ca[k], cb[k])
    assert ca["lean_sh"] > 0
    want, winfo, cur = FM.poll(o.store_state(), cur, None, 0)
    for x in (a, b):
        got, ginfo = x.feed_poll()
        assert ginfo == winfo and got.tobytes() == want.tobytes() and winfo["delivered"] > 0
    assert np.array_equal(a.feed_cursors(), b.feed_cursors()) and np.array_equal(a.feed_cursors(), cur)


# 5 ------------------------------------------------------------------------
def _witnesses(kw, how, rows, want, what):
    """The hand-derived rows loaded into spaced groups of a ticked engine; the records there are the CPU
    file's, and the whole audit is the model's over store_state()."""
    e = Engine(**kw)
    if how == "steady":
        e.init_steady(-1, 0)
        e.tick(1, 12)
    else:
        e.init_new_nodes(0)
        e.tick(0, 12)
    n = len(want)
    ids = np.array([0, 255, 256, 700, G - 1, 63, 64, 511, 1000, 300, 301, 77][:n])
    assert len(ids) == n
    e.load_groups(ids, rows)
    st = e.store_state()
    _all_equal_model(e, st, what)
    hits, _ = e.group_audit()
    got = TM.records(hits[np.isin(hits["local"], ids)])
    assert got == {int(ids[i]): w for i, w in enumerate(want) if w is not None}, what
    assert (hits["group"] == hits["local"] + int(e.cfg.group_base)).all()


def test_witnesses_ref():
    want = [w for _, w in TM.REF_CASES.values()]
    _witnesses(dict(replicas=3, groups=G, ring_depth=TM.K, client_period=1, group_base=BASE), "steady",
               TM.hand_state(TM.REF_CASES, 3), want, "hand cases, REF")


def test_witnesses_raft_hwm_above_last():
    rows, want = TM.raft_hand_state()
    _witnesses(dict(replicas=3, groups=G, ring_depth=TM.K, client_period=1, semantics=1, isolate_per_65536=8000),
               "new", rows, want, "hand cases, RAFT with hwm > last")


def test_witnesses_stamps():
    rows, want = TM.crc_hand_state()
    _witnesses(dict(replicas=3, groups=G, ring_depth=TM.K, client_period=1, payload_crc=1), "steady", rows, want,
               "hand cases, stamps")


def test_witnesses_single_replica():
    want = [w for _, w in TM.R1_CASES.values()]
    _witnesses(dict(replicas=1, groups=G, ring_depth=TM.K, client_period=1), "steady", TM.hand_state(TM.R1_CASES, 1),
               want, "hand cases, R = 1")


# 6 ------------------------------------------------------------------------
@pytest.mark.parametrize("raft", [0, 1], ids=["ref", "raft"])
def test_ceiling(raft):
    st = H.ceiling_state(np.random.default_rng(41 + raft), G, 3, 8, raft=bool(raft))
    e = Engine(replicas=3, groups=G, ring_depth=8, group_base=BASE, semantics=raft)
    e.load_state(st)
    info = _all_equal_model(e, st, "ceiling state")
    print("ceiling, raft =", raft, ": hits", info["matched"], info["per_check"])
    assert info["matched"] > 0.9 * G
    # witnesses sit in the top of the range (the hand-derived ceiling case has LOG_MATCHING at 2^31-1 itself)
    hits, _ = e.group_audit(abi.AUDIT_LOG_MATCHING)
    assert len(hits) and (hits["index"] > H.I32 - 24).all()
    assert e.group_audit(abi.AUDIT_COMMIT_BEYOND_LOG)[0]["index"].max() == H.I32


# 7 ------------------------------------------------------------------------
def test_errors():
    e = Engine(**STEADY_A)
    e.init_steady(-1, 0)
    e.tick(1, 6)
    e.diag_read()
    before = e.state_digest()[0]

    def untouched():
        assert np.array_equal(e.state_digest()[0], before)

    for checks in (0, 64, 128 | 1, 1 << 31):
        with pytest.raises(RaftError) as ei:
            e.group_audit(checks)
        assert ei.value.code == abi.RAFT_EINVAL and "checks" in str(ei.value)
        untouched()
    info = abi.AuditInfo()
    info.matched = 77
    assert e.lib.raft_group_audit(e.h, 1, 0, None, 4, C.byref(info)) == abi.RAFT_EINVAL   # cap without a buffer
    assert info.matched == 77
    untouched()
    assert e.lib.raft_group_audit(e.h, 1, 0, None, 0, None) == abi.RAFT_EINVAL            # no info
    untouched()
    with pytest.raises(RaftError) as ei:
        e.group_audit(abi.AUDIT_ALL, G + 1)
    assert ei.value.code == abi.RAFT_ERANGE
    untouched()
    empty = dict(matched=0, written=0, next_group=G, per_check={k: 0 for k in abi.AUDIT_NAMES})
    assert e.group_audit(abi.AUDIT_ALL, G)[1] == empty
    untouched()
    assert e.device_bytes() == Engine(**STEADY_A).device_bytes()   # (none of these allocated the scratch)
    e.tick(7, 5)
    assert e.diag_read()["ticks_list_skipped"] == 5    # (the proofs stand after the errors)
    # a poisoned engine answers as the scan does
    e.debug_force_pass(42)
    with pytest.raises(RaftError, match="list kernel that did not run"):
        e.tick(12, 4)
    with pytest.raises(RaftError, match="engine state is invalid") as ei:
        e.group_audit()
    assert ei.value.code == abi.RAFT_EINTERNAL
