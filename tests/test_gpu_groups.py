"""GPU: the group directory (raft_group_scan / raft_store_groups /
raft_restart_groups; k_groups.hip). The checkers are the numpy model
(tests/groups_model.py) over Engine.store_state() and over the oracle.
G = 1101 unless a case says otherwise: four blocks plus a ragged 77-lane tail.
Anchors: NewNode (main.go:59-76), FollowerRun entry (main.go:113-115), the
panics and deadlocks behind the fault codes (main.go:142, 242, 308-332)."""
import ctypes as C

import numpy as np
import pytest

import bench
import feed_model as FM
import groups_model as GM
import harness as H
import oracle
from raftstep import Engine, RaftError, abi

pytestmark = pytest.mark.gpu
THREADS = 16
G = 1101
FAULTED, LEADERLESS = abi.SELECT_FAULTED, abi.SELECT_LEADERLESS

# REF new-node churn (the oracle alone: 102 of the 1101 groups frozen at tick 60, 29 with code 2, 73 with code 3)
REF = dict(replicas=3, groups=G, ring_depth=64, entries_per_tick=1, client_period=1, seed=0x5EED0001,
           isolate_per_65536=8000, isolate_min_ticks=4, isolate_max_ticks=16, group_base=5000)
STEADY_A = dict(replicas=5, groups=G, ring_depth=16, entries_per_tick=1, client_period=1, seed=0x5EED0002)
STEADY_B = dict(STEADY_A, replicas=3, entries_per_tick=4, payload_crc=1)
STEADY_C = dict(replicas=5, groups=G, entries_per_tick=16, ring_depth=64, payload_crc=1, corrupt_per_65536=3000,
                client_period=1, seed=0x5EED0005)
STEADY_CALLS = (1, 7, 1, 13, 19)   # one tick, then consecutive calls of 40 ticks in all (K = 16: the ring wraps twice)


def _pair(kw, how, *a):
    e, o = Engine(**kw), oracle.Oracle(**kw)
    getattr(e, how)(*a)
    getattr(o, how)(*a)
    return e, o


def _tick(e, o, t, k):
    se, so = e.tick(t, k), o.tick(t, k, threads=THREADS)
    assert list(se) == list(so), f"stats of ticks [{t}, {t + k}): engine {list(se)}, oracle {list(so)}"
    return t + k


def _same_scan(got, want, what):
    (gh, gi), (wh, wi) = got, want
    assert gi == wi, f"{what}: info {gi}, model {wi}"
    assert gh.dtype == abi.GROUP_HIT and gh.tobytes() == wh.tobytes(), f"{what}: hits differ"


# 1 ------------------------------------------------------------------------
def test_scan_against_the_model_on_loaded_faults():
    rng = np.random.default_rng(11)
    st = H.random_state(rng, G, 3, 8)
    sick = rng.random(G) < 0.10
    st["fault"][sick] = rng.integers(0, 6, int(sick.sum()))
    st["fault"][[0, 255, 256, G - 1]] = [3, 1, 2, 5]
    e = Engine(replicas=3, groups=G, ring_depth=8, group_base=70000)
    e.load_state(st)
    before = e.state_digest()[0]
    for select in (FAULTED, LEADERLESS, FAULTED | LEADERLESS):
        for first in (0, 200, 256, G - 1, G):
            _, winfo = GM.scan(st, select, first, None, 70000)
            m = winfo["matched"]
            assert first >= G - 1 or m > 5
            for cap in (0, 1, 70, m, m + 5):
                what = f"select {select} first_group {first} cap {cap}"
                _same_scan(e.group_scan(select, first, cap), GM.scan(st, select, first, cap, 70000), what)
            _same_scan(e.group_scan(select, first), GM.scan(st, select, first, None, 70000), f"select {select}, counted")
        whole, _ = GM.scan(st, select, 0, None, 70000)     # paging with cap 33 reassembles the uncapped list
        pages, first = [], 0
        while first < G:
            hits, info = e.group_scan(select, first, 33)
            assert info["written"] == min(33, info["matched"])
            pages.append(hits)
            first = info["next_group"]
        assert np.concatenate(pages).tobytes() == whole.tobytes()
    assert np.array_equal(e.state_digest()[0], before)


# 2 ------------------------------------------------------------------------
def test_scan_after_real_ticks():
    e, o = _pair(REF, "init_new_nodes", 0)
    _tick(e, o, 0, 60)
    so = o.store_state()
    want = GM.scan(so, FAULTED, 0, None, REF["group_base"])
    print("REF tick 60: FAULTED hits", want[1]["matched"], "codes", np.bincount(want[0]["fault"], minlength=6).tolist())
    assert want[1]["matched"] >= 0.05 * G
    _same_scan(e.group_scan(FAULTED), want, "REF new nodes at tick 60")
    _same_scan(e.group_scan(FAULTED | LEADERLESS, 300, 40), GM.scan(so, FAULTED | LEADERLESS, 300, 40, REF["group_base"]),
               "both kinds, capped")
    kw = dict(REF, semantics=1)
    e, o = _pair(kw, "init_new_nodes", 0)
    t = 0
    for upto in (2, 20, 40):
        t = _tick(e, o, t, upto - t)
        want = GM.scan(o.store_state(), LEADERLESS, 0, None, kw["group_base"])
        print("RAFT tick", upto, ": LEADERLESS hits", want[1]["matched"])
        assert want[1]["matched"] > 0
        _same_scan(e.group_scan(LEADERLESS), want, f"RAFT new nodes at tick {upto}")


# 3 ------------------------------------------------------------------------
def _id_lists(seed):
    rng = np.random.default_rng(seed)
    fixed = [0, G - 1, 63, 64, 127, 128, 0]                # both ends, both sides of two tile boundaries, a repeat
    lists = [rng.permutation(G), np.array([G - 1])]
    for n in (63, 64, 65):
        lists.append(np.concatenate([fixed, rng.integers(0, G, n - len(fixed))]))
    return lists


def _check_store_groups(e, what, seed=5):
    """store_groups first (the device view, shared entries still shared), then
    store_state (which materialises): byte-identical rows. Returns the full state."""
    lists = _id_lists(seed)
    got = [e.store_groups(ids) for ids in lists]
    nolog = e.store_groups(lists[2], logs=False)
    full = e.store_state()
    for ids, st in zip(lists, got):
        assert set(st) == set(full)
        for k in abi.STATE_FIELDS:
            assert st[k].dtype == full[k].dtype and st[k].shape == (len(ids),) + full[k].shape[1:], (what, k)
            if st[k].tobytes() != full[k][ids].tobytes():
                bad = np.argwhere(st[k] != full[k][ids])
                raise AssertionError(f"{what}: {k} differs at {len(bad)} places, first (list position, ...) "
                                     f"{bad[0].tolist()} of group {int(ids[bad[0][0]])}, list of {len(ids)}")
    assert set(nolog) == set(full) - {"log_term", "log_value", "log_crc"}
    for k in nolog:
        assert nolog[k].tobytes() == full[k][lists[2]].tobytes(), (what, k, "logs=False")
    return full


# both sides of a 64-group ring tile and of a 256-group block, the ragged tail, the last group
RANGES = ((0, 1), (63, 2), (255, 258), (1037, 64), (G - 1, 1))


def _same_rows(got, want, rows, what):
    for k in got:
        w = want[k][rows]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, k)
        if got[k].tobytes() != w.tobytes():
            bad = np.argwhere(got[k] != w)
            raise AssertionError(f"{what}: {k} differs from the oracle at {len(bad)} places, first (row, ...) "
                                 f"{bad[0].tolist()}")


def _check_ranges(e, so, what):
    """store_state_range against the oracle's rows, with and without logs."""
    for first, n in RANGES:
        for logs in (True, False):
            got = e.store_state_range(first, n, logs=logs)
            assert set(got) == (set(so) if logs else set(so) - {"log_term", "log_value", "log_crc"})
            _same_rows(got, so, slice(first, first + n), f"{what}: range ({first}, {n}) logs={logs}")


def _run_steady(kw, e, o, calls=STEADY_CALLS):
    t = 1
    for k in calls:
        t = _tick(e, o, t, k)
    return t


@pytest.mark.parametrize("kw", [STEADY_A, STEADY_B, STEADY_C], ids=["a", "b", "c"])
def test_store_groups_equals_store_state_rows_steady_shared(kw):
    """(a) R=5 K=16 E=1, (b) R=3 E=4 with CRC, (c) the chunked shared ring with
    2K slots and corrupted copies: entries in the shared ring at the read."""
    e, o = _pair(kw, "init_steady", -1, 0)
    assert e.features()["shared_entries"]
    e.diag_read()
    if kw is STEADY_C:
        e.diag_enable()   # (corrupted copies keep the list kernel running: no steady form to lose to the counters)
    _run_steady(kw, e, o)
    c = e.diag_read()
    print("steady", kw["entries_per_tick"], ": ticks_steady_form", c["ticks_steady_form"], "ticks_list_skipped",
          c["ticks_list_skipped"], "lean_sh", c["lean_sh"], "list_sh_kept", c["list_sh_kept"])
    if kw is STEADY_C:
        assert c["lean_sh"] > 0 and c["list_sh_kept"] > 0   # shared entries written, and kept through rejections
    else:
        assert c["ticks_steady_form"] > 0 and c["ticks_list_skipped"] > 0
    full = _check_store_groups(e, "steady shared")
    so = o.store_state()
    H.assert_same_state(full, so, "steady shared vs the oracle")
    _check_ranges(e, so, "steady shared")


def _forms(e, need, limit):
    """Forms of the groups' words (raft_device.hpp gmeta bits), read until every one of `need` was seen."""
    seen = {}
    for g in range(limit):
        m = e.debug_group_words(g)["meta"]
        ssync = bool(m & (1 << 13)) and (m & 0xF) < e.cfg.replicas
        form = "explicit" if not ssync else "LXS" if m & (1 << 15) else "SXS" if m & (1 << 12) else "SSYNC"
        seen[form] = seen.get(form, 0) + 1
        if m & (1 << 14):
            seen["HWX"] = seen.get("HWX", 0) + 1
        if all(k in seen for k in need):
            break
    return seen


def test_store_groups_equals_store_state_rows_raft_leader_isolation_churn():
    """(d) RAFT under leader isolation (the small C4 configuration of
    tests/test_gpu_vx.py): compressed records, LXS, SXS, truncated logs in
    step, explicit groups, three ring segments, virtual suffixes."""
    wl = bench.WORKLOADS["C4"]
    kw = bench.engine_kwargs(wl, 7, G, 0, wl["ring_depth"], 1, 0)
    kw["isolate_per_65536"] = 4 * wl["iso"][0]
    e, o = _pair(kw, "init_new_nodes", 0)
    t = _tick(e, o, 0, 48)
    e.diag_enable()
    need = ("lean_ssync", "lean_lxs", "lean_sxs", "lean_hwx", "lean_passed")
    for _ in range(12):   # until one call's ticks have taken every form
        t = _tick(e, o, t, 5)
        c = e.diag_read()
        if all(c[k] > 0 for k in need):
            break
    e.diag_enable(False)
    full = _check_store_groups(e, f"C4 churn after tick {t - 1}")
    # (read after the stores: a flush only materialises suffixes and shared entries, the forms stay)
    seen = _forms(e, ("SSYNC", "LXS", "SXS", "HWX", "explicit"), G)
    print("forms at the read:", seen)
    assert all(seen.get(k, 0) > 0 for k in ("SSYNC", "LXS", "SXS", "HWX", "explicit")), seen
    so = o.store_state()
    H.assert_same_state(full, so, "C4 churn vs the oracle")
    _check_ranges(e, so, "C4 churn")
    for g in range(G):   # nodelog on every form
        assert e.nodelog(g) == o.nodelog(g), f"nodelog of group {g}"


def test_store_groups_equals_store_state_rows_ref_new_nodes_with_frozen_groups():
    """(e) REF new nodes at tick 60, frozen groups included."""
    e, o = _pair(REF, "init_new_nodes", 0)
    _tick(e, o, 0, 60)
    full = _check_store_groups(e, "REF new nodes at tick 60")
    assert (full["fault"] != 0).sum() >= 0.05 * G
    so = o.store_state()
    H.assert_same_state(full, so, "REF new nodes vs the oracle")
    _check_ranges(e, so, "REF new nodes")


# 4 ------------------------------------------------------------------------
@pytest.mark.parametrize("counters", [False, True], ids=["steady_form", "device_counters"])
def test_looking_changes_nothing(counters):
    """Two engines on case 3(a) run the same calls; one scans, stores 300
    groups, takes the digest and reads node logs between them. counters: with
    the device lane counters on (the shared-tick count; the steady form is then
    off by definition). The oracle runs the same ticks: both engines end in its state."""
    a, b, o = Engine(**STEADY_A), Engine(**STEADY_A), oracle.Oracle(**STEADY_A)
    o.init_steady(-1, 0)
    ids = np.random.default_rng(3).permutation(G)[:300]
    for x in (a, b):
        x.init_steady(-1, 0)
        x.diag_read()
        if counters:
            x.diag_enable()
    t = 1
    for k in STEADY_CALLS:
        a.tick(t, k)
        b.tick(t, k)
        o.tick(t, k, threads=THREADS)
        t += k
        hits, info = a.group_scan(FAULTED | LEADERLESS)
        assert info["matched"] == 0 and len(hits) == 0
        _same_rows(a.store_groups(ids), o.store_state(), ids, f"store_groups after tick {t - 1}")
        assert np.array_equal(a.state_digest()[0], o.state_digest()[0])
        for g in (0, 63, 64, 700, G - 1):
            assert a.nodelog(g) == o.nodelog(g), f"nodelog of group {g} after tick {t - 1}"
    ca, cb = a.diag_read(), b.diag_read()
    print("looking:", {k: ca[k] for k in ("ticks", "ticks_steady_form", "ticks_list_skipped", "lean_sh")})
    for k in ("ticks", "ticks_steady_form", "ticks_list_skipped", "lean_sh"):
        assert ca[k] == cb[k], (k, ca[k], cb[k])
    assert ca["ticks_list_skipped"] > 0
    assert ca["lean_sh"] > 0 if counters else ca["ticks_steady_form"] > 0
    want = o.state_digest()[0]
    assert np.array_equal(a.state_digest()[0], want) and np.array_equal(b.state_digest()[0], want)
    H.assert_same_state(a.store_state(), o.store_state(), "the looking engine vs the oracle")


# 5 ------------------------------------------------------------------------
def _restart_both(e, o, ids, tick0):
    e.restart_groups(ids, tick0)
    GM.restart(o, ids, tick0)
    H.assert_same_state(e.store_state(), o.store_state(), f"right after the restart at tick {tick0}")


@pytest.mark.parametrize("isolate_leader", [0, 1])
def test_restart_every_frozen_group_ref(isolate_leader):
    kw = dict(REF, isolate_leader=isolate_leader)
    e, o = _pair(kw, "init_new_nodes", 0)
    t = _tick(e, o, 0, 60)
    hits, info = e.group_scan(FAULTED)
    _same_scan((hits, info), GM.scan(o.store_state(), FAULTED, 0, None, kw["group_base"]), "the frozen groups")
    assert info["matched"] >= 0.05 * G
    _restart_both(e, o, hits["local"], 60)
    assert e.group_scan(FAULTED, cap=0)[1]["matched"] == 0
    t = _tick(e, o, t, 13)
    H.assert_same_state(e.store_state(), o.store_state(), "13 ticks after the restart")
    for k in (5, 1, 21):
        t = _tick(e, o, t, k)
    assert t == 100
    H.assert_same_state(e.store_state(), o.store_state(), "40 ticks after the restart")
    end = o.store_state(logs=False)
    print("isolate_leader", isolate_leader, ": restarted", len(hits), "with a Leader at tick 100:",
          int((end["role"][hits["local"]] == abi.LEADER).any(axis=1).sum()))


def test_restart_healthy_groups_raft():
    kw = dict(REF, semantics=1)
    e, o = _pair(kw, "init_new_nodes", 0)
    t = _tick(e, o, 0, 37)
    healthy = np.nonzero(o.store_state(logs=False)["fault"] == 0)[0]
    ids = np.random.default_rng(9).permutation(healthy)[:50]
    _restart_both(e, o, ids, 37)
    t = _tick(e, o, t, 13)
    H.assert_same_state(e.store_state(), o.store_state(), "13 ticks after the restart")
    for k in (2, 24, 1):
        t = _tick(e, o, t, k)
    H.assert_same_state(e.store_state(), o.store_state(), "40 ticks after the restart")


# 6 ------------------------------------------------------------------------
def test_restart_inside_a_shared_steady_engine():
    e, o = _pair(STEADY_A, "init_steady", -1, 0)
    t = _run_steady(STEADY_A, e, o, (1, 20))
    ids = np.array([G - 1, 64, 700])
    before = e.state_digest()[0]
    _restart_both(e, o, ids, t)
    after = e.state_digest()[0]
    others = np.setdiff1d(np.arange(G), ids)
    assert np.array_equal(after[others], before[others])
    assert (after[ids] != before[ids]).all()
    for k in (1, 9, 20):
        t = _tick(e, o, t, k)    # (a poisoned engine would fail here)
    H.assert_same_state(e.store_state(), o.store_state(), "30 ticks after the restart")
    assert np.array_equal(e.state_digest()[0], o.state_digest()[0])


# 7 ------------------------------------------------------------------------
def test_restart_keeps_the_feed_open():
    e, o = _pair(STEADY_A, "init_steady", -1, 0)
    fed = [1, 3]
    e.feed_open(fed, "start")
    cur = FM.start_cursors(o.store_state(), fed, "start")
    t = _tick(e, o, 1, 10)

    def poll(what):
        nonlocal cur
        want, winfo, cur = FM.poll(o.store_state(), cur, None, 0)
        got, ginfo = e.feed_poll()
        assert ginfo == winfo and got.tobytes() == want.tobytes(), what
        assert np.array_equal(e.feed_cursors(), cur), f"{what}: cursors"
        return winfo

    assert poll("before the restart")["delivered"] > 0
    ids = np.array([0, 300, 301, G - 1])
    prev = e.feed_cursors()
    _restart_both(e, o, ids, t)
    now = e.feed_cursors()
    cur = GM.restart_cursors(cur, ids)
    assert np.array_equal(now, cur)
    assert (now[ids][:, fed] == 0).all() and (now[ids][:, [0, 2, 4]] == -1).all()
    others = np.setdiff1d(np.arange(G), ids)
    assert np.array_equal(now[others], prev[others]) and (prev[ids][:, fed] > 0).all()
    for k in (1, 14, 25):
        t = _tick(e, o, t, k)
        info = poll(f"poll after tick {t - 1}")
        assert info["stalled"] == 0
    H.assert_same_state(e.store_state(), o.store_state(), "after the feed")


# 8 ------------------------------------------------------------------------
def test_errors_and_the_empty_list():
    e, o = _pair(STEADY_A, "init_steady", -1, 0)
    t = _run_steady(STEADY_A, e, o, (1, 5))
    before = e.state_digest()[0]
    for call in (lambda: e.store_groups([3, G]), lambda: e.restart_groups([3, G], t)):
        with pytest.raises(RaftError) as ei:
            call()
        assert ei.value.code == abi.RAFT_ERANGE
    with pytest.raises(RaftError) as ei:
        e.restart_groups([5, 9, 5], t)
    assert ei.value.code == abi.RAFT_EINVAL and "twice" in str(ei.value)
    with pytest.raises(RaftError) as ei:
        e.restart_groups([5], 1 << 40)
    assert ei.value.code == abi.RAFT_ERANGE
    for select in (0, 4, 7):
        with pytest.raises(RaftError) as ei:
            e.group_scan(select)
        assert ei.value.code == abi.RAFT_EINVAL and "select" in str(ei.value)
    info = abi.ScanInfo()
    assert e.lib.raft_group_scan(e.h, 1, 0, None, 4, C.byref(info)) == abi.RAFT_EINVAL
    with pytest.raises(RaftError) as ei:
        e.group_scan(FAULTED, G + 1)
    assert ei.value.code == abi.RAFT_ERANGE
    assert e.group_scan(FAULTED, G)[1] == dict(matched=0, written=0, next_group=G)
    assert np.array_equal(e.state_digest()[0], before)
    # n = 0: nothing changes, the proofs included: the next call still skips the list
    e.diag_read()
    e.restart_groups([], t)
    st = e.store_groups([])
    assert st["role"].shape == (0, 5)
    t = _tick(e, o, t, 5)
    assert e.diag_read()["ticks_list_skipped"] == 5
    # ... while a restart ends the skip, as a handler batch does
    e.restart_groups([7], t)
    GM.restart(o, [7], t)
    t = _tick(e, o, t, 5)
    assert e.diag_read()["ticks_list_skipped"] == 0
    H.assert_same_state(e.store_state(), o.store_state(), "after the errors")


def test_a_poisoned_engine_answers_einternal():
    e = Engine(**STEADY_A)
    e.init_steady(-1, 0)
    e.tick(1, 6)
    e.tick(7, 5)
    e.debug_force_pass(42)     # a group passed to a list kernel that does not run: ticks lost, the engine says so
    with pytest.raises(RaftError, match="list kernel that did not run"):
        e.tick(12, 4)
    for call in (lambda: e.group_scan(FAULTED), lambda: e.store_groups([1]), lambda: e.restart_groups([1], 16)):
        with pytest.raises(RaftError, match="engine state is invalid") as ei:
            call()
        assert ei.value.code == abi.RAFT_EINTERNAL


# 9 ------------------------------------------------------------------------
@pytest.mark.parametrize("payload_crc", [1, 0], ids=["crc", "nocrc"])
def test_gather_chunk_edges(payload_crc):
    """K = 4096: a group's view is 196,760 B with log_crc rows and 147,608 B
    without, so a chunk of the gather is its 256-group floor either way and 600
    groups go as 256 + 256 + 88; the range starts inside the full call's first
    chunk and takes two of its own."""
    kw = dict(replicas=3, groups=600, ring_depth=4096, entries_per_tick=1, client_period=1, payload_crc=payload_crc)
    e, o = _pair(kw, "init_steady", -1, 0)
    _tick(e, o, 1, 70)
    so = o.store_state()
    assert (so["last"] == 70).all() and (so["fault"] == 0).all()
    H.assert_same_state(e.store_state(), so, "600 groups in three chunks vs the oracle")
    _same_rows(e.store_state_range(250, 300), so, slice(250, 550), "range (250, 300)")
    ids = np.random.default_rng(17).permutation(600)
    _same_rows(e.store_groups(ids), so, ids, "store_groups of a permutation of every id")
