"""GPU: raft_load_groups (the device scatter of k_groups.hip, scatter_view.hpp)
and the whole-state loads that go through it (raft_load_state,
raft_checkpoint_load). The checkers are the oracle through tests/load_model.py
(splice, then load_state) and per-group digests. G = 1101 unless a case says
otherwise: four blocks plus a ragged 77-lane tail. The rows come from the donor
states of load_model.py; a case picks them so that they hold every class of
rows of its semantics (load_model.classes)."""
import ctypes as C

import numpy as np
import pytest

import feed_model as FM
import groups_model as GM
import harness as H
import load_model as LM
import oracle
from raftstep import Engine, RaftError, abi

pytestmark = pytest.mark.gpu
THREADS = 16
G = LM.G
K = 16
# the churn target: test_gpu_groups.py's REF configuration with K = 16 (isolation on: 2K physical slots)
REF = dict(replicas=3, groups=G, ring_depth=K, entries_per_tick=1, client_period=1, seed=0x5EED0001,
           isolate_per_65536=8000, isolate_min_ticks=4, isolate_max_ticks=16, group_base=5000)
RAFT = dict(REF, semantics=1)
# the shared steady engines of test_gpu_groups.py (no isolation: K physical slots)
STEADY_A = dict(replicas=5, groups=G, ring_depth=K, entries_per_tick=1, client_period=1, seed=0x5EED0002)
STEADY_B = dict(STEADY_A, replicas=3, entries_per_tick=4, payload_crc=1)
OPTIONAL = ("log_crc", "next", "hwm", "iso_victim")


def _pair(kw, how, *a):
    e, o = Engine(**kw), oracle.Oracle(**kw)
    getattr(e, how)(*a)
    getattr(o, how)(*a)
    return e, o


def _tick(e, o, t, k):
    se, so = e.tick(t, k), o.tick(t, k, threads=THREADS)
    assert list(se) == list(so), f"stats of ticks [{t}, {t + k}): engine {list(se)}, oracle {list(so)}"
    return t + k


def _same(e, o, what):
    H.assert_same_state(e.store_state(), o.store_state(), what)
    assert np.array_equal(e.state_digest()[0], o.state_digest()[0]), f"{what}: digests"


def _targets(rows_idx, seed):
    """A random target id per row, none the id the row had."""
    ids = np.random.default_rng(seed).permutation(G)[:len(rows_idx)]
    while (ids == rows_idx).any():
        ids = np.roll(ids, 1)
    return ids


def _load_both(e, o, ids, rows, what):
    """Loads rows into ids on both; checks the states, and the digests of the others against before."""
    before = e.state_digest()[0]
    e.load_groups(ids, rows)
    LM.load(o, ids, rows)
    _same(e, o, what)
    others = np.setdiff1d(np.arange(e.cfg.groups), ids)
    assert np.array_equal(e.state_digest()[0][others], before[others]), f"{what}: an unlisted group changed"


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("raft", [0, 1], ids=["ref", "raft"])
def test_load_into_a_churned_engine(raft):
    kw = RAFT if raft else REF
    donor = LM.donor(LM.DONOR_RAFT if raft else LM.DONOR_REF)
    idx = LM.pick(donor, raft, K, 100, 21 + raft)
    rows = LM.take(donor, idx)
    print("rows:", len(idx), {k: int(m[idx].sum()) for k, m in LM.classes(donor, raft, K).items()})
    e, o = _pair(kw, "init_new_nodes", 0)
    t = _tick(e, o, 0, 60)
    _load_both(e, o, _targets(idx, 31), rows, "right after the load")
    for k in (13, 5, 1, 21):
        t = _tick(e, o, t, k)
    assert t == 100
    _same(e, o, "40 ticks after the load")


# 2 ------------------------------------------------------------------------
def test_round_trips_leave_every_digest():
    e = Engine(**RAFT)
    e.init_new_nodes(0)
    e.tick(0, 60)
    before = e.state_digest()[0]
    rng = np.random.default_rng(5)
    ids = rng.permutation(G)[:300]
    e.load_groups(ids, e.store_groups(ids))
    assert np.array_equal(e.state_digest()[0], before)
    a, b = ids[:150], ids[150:]
    ra, rb = e.store_groups(a), e.store_groups(b)
    e.load_groups(b, ra)
    got = e.store_groups(b)
    for k in ra:
        assert got[k].tobytes() == ra[k].tobytes(), k
    others = np.setdiff1d(np.arange(G), b)
    assert np.array_equal(e.state_digest()[0][others], before[others])
    e.load_groups(b, rb)
    assert np.array_equal(e.state_digest()[0], before)
    e.tick(60, 3)   # (and the engine runs on)


# 3 ------------------------------------------------------------------------
def test_optional_fields_absent_with_payload_crc():
    kw = dict(RAFT, payload_crc=1)
    donor = LM.donor(LM.DONOR_RAFT)
    idx = LM.pick(donor, True, K, 100, 23)
    rows = {k: v for k, v in LM.take(donor, idx).items() if k not in OPTIONAL}
    e, o = _pair(kw, "init_new_nodes", 0)
    t = _tick(e, o, 0, 60)
    ids = _targets(idx, 33)
    _load_both(e, o, ids, rows, "rows without the optional fields")
    got = e.store_groups(ids)
    live = got["log_term"] != 0
    assert live.any() and (got["log_crc"][live] != 0).all()   # stamped on the device
    assert np.array_equal(got["hwm"], rows["last"]) and not got["iso_victim"].any()
    for k in (13, 5, 1, 21):
        t = _tick(e, o, t, k)
    _same(e, o, "40 ticks after the load")


# 4 ------------------------------------------------------------------------
# The rows' timers are on the engine's own virtual clock: a row taken at donor
# tick 60 holds timer starts (deadline - timeout) of second 118, and in an
# engine that stands at tick 27 every later heartbeat would lie before them
# (the engine keeps max(timer start, last heartbeat), the oracle the last write:
# measured, deadlines 6 s apart 30 ticks on). So the steady cases, which load
# around tick 25, take their rows from the donor run at tick 20.
STEADY_DONOR_TICKS = 20


def _three_rows(kw):
    """A frozen, a candidate and a healthy donor group of the target's R, K and CRC setting."""
    dkw = dict(LM.DONOR_REF, replicas=kw["replicas"], payload_crc=kw.get("payload_crc", 0))
    donor = LM.donor(dkw, "new", STEADY_DONOR_TICKS)
    cl = LM.classes(donor, False, K)
    frozen = np.nonzero(donor["fault"] != 0)[0]
    idx = [int(frozen[0]), int(np.nonzero(cl["candidate"] & (donor["fault"] == 0))[0][0]),
           int(np.nonzero(cl["healthy_leader"])[0][0])]
    return donor, idx


@pytest.mark.parametrize("kw", [STEADY_A, STEADY_B], ids=["a", "b"])
def test_load_inside_a_shared_steady_engine(kw):
    e, o = _pair(kw, "init_steady", -1, 0)
    assert e.features()["shared_entries"]
    t = 1
    for k in (1, 20):
        t = _tick(e, o, t, k)
    # n = 0: nothing changes, the proofs included: the next call still skips the list
    e.diag_read()
    e.load_groups([], e.store_groups([]))
    t = _tick(e, o, t, 5)
    assert e.diag_read()["ticks_list_skipped"] == 5
    donor, idx = _three_rows(kw)
    ids = np.array([G - 1, 64, 700])
    before = e.state_digest()[0]
    _load_both(e, o, ids, LM.take(donor, idx), "right after the load")
    assert (e.state_digest()[0][ids] != before[ids]).all()
    for k in (1, 9, 20):
        t = _tick(e, o, t, k)    # (a poisoned engine would fail here)
    assert e.diag_read()["ticks_list_skipped"] == 0   # a load ends the skip, as a restart does
    _same(e, o, "30 ticks after the load")


# 5 ------------------------------------------------------------------------
def test_load_keeps_the_feed_open():
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

    assert poll("before the load")["delivered"] > 0
    t = _tick(e, o, t, 12)
    poll("at tick 22")
    donor = LM.donor(dict(LM.DONOR_REF, replicas=5), "new", STEADY_DONOR_TICKS)
    cl = LM.classes(donor, False, K)
    healthy = np.nonzero(cl["healthy_leader"])[0]
    rows = LM.take(donor, [int(healthy[0]), int(healthy[1]), int(np.nonzero(donor["fault"] != 0)[0][0]), int(healthy[2])])
    ids = np.array([0, 300, 301, G - 1])
    prev = e.feed_cursors()
    _load_both(e, o, ids, rows, "the load under an open feed")
    now = e.feed_cursors()
    cur = LM.load_cursors(cur, ids, rows)
    assert np.array_equal(now, cur)
    assert (now[ids][:, [0, 2, 4]] == -1).all() and (now[ids][:, fed] != prev[ids][:, fed]).any()
    others = np.setdiff1d(np.arange(G), ids)
    assert np.array_equal(now[others], prev[others])
    for k in (1, 14, 25):
        t = _tick(e, o, t, k)
        info = poll(f"poll after tick {t - 1}")
        assert info["stalled"] == 0
    _same(e, o, "after the feed")


# 6 ------------------------------------------------------------------------
def _raw_load(e, ids, rows):
    """raft_load_groups without Engine.load_groups' own checks (a view with a NULL field)."""
    ids = np.ascontiguousarray(ids, np.uint64)
    v = abi.make_view(rows)
    return e.lib.raft_load_groups(e.h, ids.ctypes.data, len(ids), C.byref(v))


@pytest.mark.parametrize("raft", [0, 1], ids=["ref", "raft"])
def test_errors_change_nothing(raft):
    kw = RAFT if raft else REF
    R = kw["replicas"]
    e, o = _pair(kw, "init_new_nodes", 0)
    t = _tick(e, o, 0, 40)
    st = o.store_state()
    lead = np.nonzero((st["fault"] == 0) & ((st["role"] == abi.LEADER).sum(axis=1) == 1) & (st["last"].min(axis=1) > 0))[0]
    ids = np.array([3, int(lead[0]), 1000])
    good = e.store_groups(ids)
    e.feed_open([0], "commit")
    cursors, before = e.feed_cursors(), e.state_digest()[0]

    def refused(code, rows, text=None, ids=ids):
        with pytest.raises(RaftError) as ei:
            e.load_groups(ids, rows)
        assert ei.value.code == code, str(ei.value)
        if text:
            assert text in str(ei.value), str(ei.value)

    def bad(field, pos, value):
        rows = {k: v.copy() for k, v in good.items()}
        rows[field][pos] = value
        return rows

    refused(abi.RAFT_ERANGE, good, "element 2: group 1101", ids=np.array([3, 5, G]))
    refused(abi.RAFT_EINVAL, good, "twice", ids=np.array([3, 5, 3]))
    for k in ("role", "match", "fault", "log_value"):   # a missing required field: no partial patching
        assert _raw_load(e, ids, {f: v for f, v in good.items() if f != k}) == abi.RAFT_EINVAL, k
    where = f"element 1: group {ids[1]}"
    refused(abi.RAFT_EINVAL, bad("fault", 1, 6), where)
    refused(abi.RAFT_EINVAL, bad("role", (1, 2), 3), where)
    refused(abi.RAFT_EINVAL, bad("voted", (1, 0), R + 1 if raft else 2), where)
    refused(abi.RAFT_EINVAL, bad("last", (1, 1), -1), where)
    refused(abi.RAFT_EINVAL, bad("timeout", (1, 0), 1024), where)
    refused(abi.RAFT_EINVAL, bad("iso_victim", 1, 0x04), where)
    refused(abi.RAFT_EINVAL, bad("iso_victim", 1, 0x80 | (8 | R) << 0), where)   # victim replica R
    if raft:
        r = int(good["last"][1].argmax())
        refused(abi.RAFT_EINVAL, bad("hwm", (1, r), int(good["last"][1, r]) + K), "ring window")
        ld = int((good["role"][1] == abi.LEADER).argmax())
        rows = bad("match", (1, ld, (ld + 1) % R), H.I32)
        rows["next"][1, ld, (ld + 1) % R] = 0
        refused(abi.RAFT_EINVAL, rows, "does not fit")
    assert np.array_equal(e.state_digest()[0], before)
    assert np.array_equal(e.feed_cursors(), cursors)   # (the feed is still open and did not move)
    e.load_groups(ids, good)                           # what was refused in part loads whole
    assert np.array_equal(e.state_digest()[0], before)
    t = _tick(e, o, t, 1)
    _same(e, o, "the tick after the errors")


def test_a_poisoned_engine_answers_einternal():
    e = Engine(**STEADY_A)
    e.init_steady(-1, 0)
    e.tick(1, 6)
    e.tick(7, 5)
    rows = e.store_groups([1])
    e.debug_force_pass(42)     # a group passed to a list kernel that does not run: ticks lost, the engine says so
    with pytest.raises(RaftError, match="list kernel that did not run"):
        e.tick(12, 4)
    with pytest.raises(RaftError, match="engine state is invalid") as ei:
        e.load_groups([1], rows)
    assert ei.value.code == abi.RAFT_EINTERNAL


# 7 ------------------------------------------------------------------------
@pytest.mark.parametrize("payload_crc", [1, 0], ids=["crc", "nocrc"])
def test_scatter_chunk_edges(payload_crc):
    """K = 4096: a group's view is 196,760 B with log_crc rows and 147,608 B
    without, so a chunk of the scatter is its 256-group floor either way and the
    300 groups go as 256 + 44. load_groups of a permutation of every id, and
    load_state of the same view on a twin engine."""
    kw = dict(replicas=3, groups=300, ring_depth=4096, entries_per_tick=1, client_period=1, payload_crc=payload_crc)
    donor = LM.donor(kw, "steady", 70)
    assert (donor["last"] == 70).all()
    perm = np.random.default_rng(17).permutation(300)
    a, b, o = Engine(**kw), Engine(**kw), oracle.Oracle(**kw)
    for x in (a, b, o):
        x.init_steady(-1, 0)
    a.load_groups(perm, donor)
    st = GM.splice(donor, perm, donor)   # group perm[i] holds row i
    b.load_state(st)
    o.load_state(st)
    _same(a, o, "load_groups of every id")
    _same(b, o, "load_state of the same view")
    so = o.tick(71, 5, threads=THREADS)
    for x in (a, b):
        assert list(x.tick(71, 5)) == list(so)
    _same(a, o, "5 ticks on, load_groups")
    _same(b, o, "5 ticks on, load_state")


# 9 ------------------------------------------------------------------------
@pytest.mark.parametrize("raft", [0, 1], ids=["ref", "raft"])
def test_whole_state_load_and_checkpoint(raft, tmp_path):
    kw = LM.DONOR_RAFT if raft else LM.DONOR_REF
    donor = LM.donor(kw)
    a, b, o = Engine(**kw), Engine(**kw), oracle.Oracle(**kw)
    a.load_state(donor)
    o.load_state(donor)
    _same(a, o, "load_state of the donor view")
    path = tmp_path / "donor.ckpt"
    a.save_checkpoint(path)
    b.load_checkpoint(path)
    _same(b, o, "the checkpoint on a fresh engine")
    so = o.tick(LM.DONOR_TICKS, 7, threads=THREADS)
    for x in (a, b):
        assert list(x.tick(LM.DONOR_TICKS, 7)) == list(so)
        _same(x, o, "7 ticks on")
