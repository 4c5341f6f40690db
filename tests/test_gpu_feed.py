"""GPU: the commit feed (raft_feed_open / _poll / _cursors / _close; k_feed.hip).
Every case drives an engine and the oracle alike, polls the engine, runs the
numpy model (tests/feed_model.py) over the oracle's canonical view with its own
cursor array, and asserts that the records, the info and the cursors are equal.
The figures quoted per case are the model's over the oracle at that shape.
Anchors: main.go:330 (the leader should answer the client once CommitIndex has
advanced), 151-153 (a follower's CommitIndex = min(LeaderCommit, len+1)),
387-390 (the leader's commit rule)."""
import numpy as np
import pytest

import feed_model as FM
import harness as H
import oracle
from raftstep import Engine, RaftError, abi

pytestmark = pytest.mark.gpu
THREADS = 16

STEADY = dict(replicas=5, groups=256 * 3 + 77, ring_depth=16, entries_per_tick=1, client_period=1, seed=0x5EED0002)


def _same(got, want, what):
    ge, gi = got
    we, wi = want
    assert gi == wi, f"{what}: info {gi}, model {wi}"
    assert ge.dtype == abi.FEED_ENTRY and len(ge) == len(we), what
    if ge.tobytes() != we.tobytes():
        bad = np.nonzero(ge != we)[0]
        raise AssertionError(f"{what}: {bad.size} records differ, first at {int(bad[0])}: "
                             f"engine {ge[bad[0]]}, model {we[bad[0]]}")


class Pair:
    """An engine (None: the model alone) and the oracle, driven alike, with a
    feed on the engine and the model's cursors beside it."""

    def __init__(self, kw, engine=True):
        self.kw = kw
        self.e = Engine(**kw) if engine else None
        self.o = oracle.Oracle(**kw)
        self.cur = None
        self.delivered = self.lost = self.stalled_polls = 0
        self.out = []

    def both(self):
        return [x for x in (self.e, self.o) if x is not None]

    def init(self, how, *a):
        for x in self.both():
            getattr(x, how)(*a)

    def open(self, replicas=None, start="start"):
        self.cur = FM.start_cursors(self.o.store_state(), replicas, start)
        if self.e is not None:
            self.e.feed_open(replicas, start)

    def tick(self, t, k, stats=True):
        so = self.o.tick(t, k, threads=THREADS)
        if self.e is not None:
            se = self.e.tick(t, k, stats=stats)
            if stats:
                assert list(se) == list(so), f"stats of ticks [{t}, {t + k})"
        return t + k

    def poll(self, cap=None, what=""):
        want, info, self.cur = FM.poll(self.o.store_state(), self.cur, cap, int(self.kw.get("group_base", 0)))
        if self.e is not None:
            _same(self.e.feed_poll(cap), (want, info), what)
            assert np.array_equal(self.e.feed_cursors(), self.cur), f"{what}: cursors"
        self.delivered += info["delivered"]
        self.lost += info["lost"]
        self.stalled_polls += info["stalled"]
        self.out.append(want)
        return want, info

    def run(self, t, nticks, every, stats=True):
        """nticks ticks from t, polled after every `every` of them (and at the end)."""
        end = t + nticks
        while t < end:
            k = min(every, end - t)
            t = self.tick(t, k, stats)
            self.poll(what=f"poll after tick {t - 1}")
        return t

    def entries(self):
        return np.concatenate(self.out) if self.out else np.zeros(0, abi.FEED_ENTRY)


def case_steady(engine=True, groups=STEADY["groups"], nticks=40, every=1, **kw):
    p = Pair(dict(STEADY, groups=groups, **kw), engine)
    p.init("init_steady", -1, 0)
    p.open()
    p.run(1, nticks, every)
    return p


def case_newnode(engine=True):
    p = Pair(dict(replicas=3, groups=700, client_period=3, isolate_per_65536=8000), engine)
    p.init("init_new_nodes", 0)
    p.open()
    p.run(0, 160, 5)
    return p


CHURN = {
    "A": (dict(replicas=7, groups=1024, ring_depth=64, seed=0x45, semantics=1, client_period=1, isolate_leader=1,
               isolate_per_65536=20000, isolate_min_ticks=4, isolate_max_ticks=32), 200, 7, 1289531, 0),
    "B": (dict(replicas=5, groups=1024, ring_depth=16, seed=0x46, semantics=1, client_period=1, isolate_leader=1,
               isolate_per_65536=30000, isolate_min_ticks=4, isolate_max_ticks=16), 300, 3, 994808, 12),
}


def case_churn(shape, engine=True):
    kw, nticks, every, _, _ = CHURN[shape]
    p = Pair(kw, engine)
    p.init("init_new_nodes", 0)
    p.open()
    p.run(0, nticks, every)
    return p


CRC = dict(replicas=5, groups=512, entries_per_tick=16, ring_depth=64, payload_crc=1, corrupt_per_65536=3000,
           client_period=1, seed=0x5EED0005)


def case_crc(engine=True):
    p = Pair(CRC, engine)
    p.init("init_steady", -1, 0)
    p.open()
    p.run(1, 20, 2)
    return p


# 1 ------------------------------------------------------------------------
def test_steady_shared_ring_past_the_wrap():
    """REF steady state, entries in the shared ring, polled after every tick
    for 40 ticks (K=16: the ring wraps twice); G has a partial block and a
    partial wave. A twin engine runs the same calls without a feed: polling
    between steady calls keeps the steady tick's forms. Model: 165,620 entries,
    0 lost."""
    p = Pair(STEADY)
    twin = Engine(**STEADY)
    assert p.e.features()["shared_entries"]
    p.init("init_steady", -1, 0)
    twin.init_steady(-1, 0)
    p.open()
    for x in (p.e, twin):
        x.diag_read()
    t = 1
    for _ in range(40):
        twin.tick(t, 1)
        t = p.tick(t, 1)
        p.poll(what=f"poll after tick {t - 1}")
    a, b = p.e.diag_read(), twin.diag_read()
    print("steady:", p.delivered, "entries,", p.lost, "lost; ticks_steady_form", a["ticks_steady_form"],
          "ticks_list_skipped", a["ticks_list_skipped"])
    for k in ("ticks", "ticks_steady_form", "ticks_list_skipped"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["ticks_steady_form"] > 0
    assert (p.delivered, p.lost, p.stalled_polls) == (165620, 0, 0)
    assert FM.disagreements(p.entries()) == 0
    H.assert_same_state(p.e.store_state(), p.o.store_state(), "after the feed")
    assert np.array_equal(twin.state_digest()[0], p.o.state_digest()[0])


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [1, 0])
def test_consumer_that_falls_behind(monkeypatch, paired):
    """Polled every 25 ticks with K=16: what left the ring is counted as lost
    and skipped. Model: 67,266 delivered, 31,302 lost. (paired = 0: the emit
    pass's other store form, RAFTSTEP_FEED_PAIRED; the same bytes.)"""
    monkeypatch.setenv("RAFTSTEP_FEED_PAIRED", str(paired))
    p = case_steady(groups=333, nticks=60, every=25)
    print("behind:", p.delivered, "delivered,", p.lost, "lost")
    assert (p.delivered, p.lost, p.stalled_polls) == (67266, 31302, 0)


# 3 ------------------------------------------------------------------------
def test_cap_cuts_and_resumes():
    """10 unpolled ticks, then drained under caps 1000, 1, G*R - 3 in turn: the
    concatenation equals one uncapped poll of a twin engine byte for byte, and
    pending is right at every step (the model is polled with the same caps)."""
    G, R = STEADY["groups"], STEADY["replicas"]
    p = Pair(STEADY)
    twin = Engine(**STEADY)
    p.init("init_steady", -1, 0)
    twin.init_steady(-1, 0)
    p.open()
    twin.feed_open(start="start")
    p.tick(1, 10)
    twin.tick(1, 10)
    whole, winfo = twin.feed_poll()
    assert winfo["delivered"] == G * (10 + 9 * (R - 1)) and winfo["pending"] == 0   # (followers commit a tick later)
    caps = [1000, 1, G * R - 3]
    left, i = winfo["delivered"], 0
    while True:
        cap = caps[i % 3]
        _, info = p.poll(cap, what=f"capped poll {i} (cap {cap})")
        left -= min(cap, left)
        assert info["pending"] == left
        i += 1
        if info["pending"] == 0:
            break
    assert p.entries().tobytes() == whole.tobytes()
    assert np.array_equal(p.e.feed_cursors(), twin.feed_cursors())


def test_cap_zero_only_skips_lost_entries():
    p = Pair(dict(STEADY, groups=333))
    p.init("init_steady", -1, 0)
    p.open()
    p.tick(1, 25)
    before = p.cur.copy()
    e, info = p.poll(0, what="counting poll")
    # every log holds 25 entries, of which the ring keeps 16: 9 lost per pair; the leader has
    # committed 25 and the four followers 24
    assert len(e) == 0 and info == dict(delivered=0, pending=333 * (16 + 4 * 15), lost=333 * 5 * 9, stalled=0)
    assert np.array_equal(p.cur, before + 9)            # past the lost entries, no further
    e, info = p.poll(what="full poll after the counting one")
    assert info["lost"] == 0 and info["delivered"] == 333 * (16 + 4 * 15)


# 4 ------------------------------------------------------------------------
def test_ref_from_newnode_with_isolation_and_faults():
    """REF from NewNode: elections, isolated replicas, followers whose
    CommitIndex runs ahead of their log, groups frozen by a fault (read like
    any other). Model: 77,875 entries, 292 frozen groups."""
    p = case_newnode()
    frozen = int((p.o.store_state()["fault"] != 0).sum())
    print("newnode:", p.delivered, "entries,", p.lost, "lost,", frozen, "frozen groups")
    assert (p.delivered, p.lost, p.stalled_polls, frozen) == (77875, 0, 0, 292)
    H.assert_same_state(p.e.store_state(), p.o.store_state(), "after the feed")


# 5 ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["A", "B"])
def test_raft_churn(shape):
    """RAFT semantics under leader isolation: LXS, SXS, virtual suffixes,
    truncated logs and three ring segments. Committed entries agree across
    replicas in the engine's output too."""
    p = case_churn(shape)
    print("churn", shape, ":", p.delivered, "entries,", p.lost, "lost")
    assert (p.delivered, p.lost) == CHURN[shape][3:]
    assert FM.disagreements(p.entries()) == 0
    H.assert_same_state(p.e.store_state(), p.o.store_state(), "after the feed")


# 6 ------------------------------------------------------------------------
def _entry_crcs(term, value):
    """harness.entry_crc over arrays: bitwise CRC32C of Term (4 B LE) || Value (8 B LE)."""
    c = np.full(len(term), 0xFFFFFFFF, np.uint64)
    words = (term.astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF), value.astype(np.uint64))
    for w, nbytes in zip(words, (4, 8)):
        for b in range(nbytes):
            c ^= (w >> np.uint64(8 * b)) & np.uint64(0xFF)
            for _ in range(8):
                c = (c >> np.uint64(1)) ^ (np.uint64(0x82F63B78) * (c & np.uint64(1)))
    return (c ^ np.uint64(0xFFFFFFFF)).astype(np.uint32)


@pytest.mark.parametrize("paired", [1, 0])
def test_crc_and_batches(monkeypatch, paired):
    """16 entries per tick with CRC stamps and corrupted copies (the chunked
    shared ring): every record carries its entry's stamp. Model: 783,088
    entries, 752 lost."""
    monkeypatch.setenv("RAFTSTEP_FEED_PAIRED", str(paired))
    p = case_crc()
    print("crc:", p.delivered, "entries,", p.lost, "lost")
    assert (p.delivered, p.lost) == (783088, 752)
    e = p.entries()
    for x in e[:: len(e) // 50]:                            # (the bitwise form below is harness.entry_crc's)
        assert _entry_crcs(x["term"][None], x["value"][None])[0] == H.entry_crc(int(x["term"]), int(x["value"]))
    assert np.array_equal(e["crc"], _entry_crcs(e["term"], e["value"]))


# 7 ------------------------------------------------------------------------
def test_staged_values_come_back_out():
    kw = dict(STEADY, client_source=abi.CLIENT_STAGED)
    p = Pair(kw)
    vals = H.staged_values(kw["seed"], 1, 40, 1, kw["groups"])
    p.init("init_steady", -1, 0)
    for x in p.both():
        x.stage_values(1, vals)
    p.open()
    p.run(1, 40, 4)
    e = p.entries()
    assert len(e) == 165620
    # entry i of every log is the client request of tick i (one per tick from tick 1)
    assert np.array_equal(e["value"], vals[e["index"] - 1, 0, e["group"].astype(np.int64)])


# 8 ------------------------------------------------------------------------
def test_follower_commit_one_past_its_log():
    """A REF follower with CommitIndex = LastApplied + 1 (main.go:152): the
    feed stops at its last entry; the missing entry arrives once an
    AppendEntries brings it."""
    R, K, G = 3, 16, 3
    groups = []
    for g in range(G):
        log = [(1, 10 * g + 1), (1, 10 * g + 2)]
        groups.append([H.node(H.L, 1, 1, log, commit=2, match=[0, 1, 2], deadline=1000),
                       H.node(H.F, 1, 1, log[:1], commit=2, deadline=1000),
                       H.node(H.F, 1, 1, log, commit=2, deadline=1000)])
    st = H.build_state(groups, R, K)
    p = Pair(dict(replicas=R, groups=G, ring_depth=K, client_period=0))
    for x in p.both():
        x.load_state(st)
    p.open()
    e, info = p.poll(what="first poll")
    assert info["delivered"] == G * 5 and info["stalled"] == 0
    assert e[e["replica"] == 1]["index"].tolist() == [1] * G
    reqs, ents = H.ae_reqs([dict(group=g, to=1, term=1, prev_log_index=1, prev_log_term=1, leader_commit=2,
                                 logs=[(1, 10 * g + 2)]) for g in range(G)])
    for x in p.both():
        x.append_entries(5, reqs, ents)
    e, info = p.poll(what="after the AppendEntries batch")
    assert [(int(x["group"]), int(x["replica"]), int(x["index"]), int(x["value"])) for x in e] == \
        [(g, 1, 2, 10 * g + 2) for g in range(G)]


# 9 ------------------------------------------------------------------------
def test_shards_merge_by_global_id():
    G = STEADY["groups"]
    G0 = G // 2
    whole = Pair(STEADY)
    a = Pair(dict(STEADY, groups=G0, group_base=0))
    b = Pair(dict(STEADY, groups=G - G0, group_base=G0))
    for p in (whole, a, b):
        p.init("init_steady", -1, 0)
        p.open()
        p.run(1, 12, 5)
    merged = np.concatenate([np.concatenate([x, y]) for x, y in zip(a.out, b.out)])
    assert merged.tobytes() == whole.entries().tobytes()
    assert int(merged["group"].max()) == G - 1


# 10 -----------------------------------------------------------------------
def test_lifecycle(tmp_path):
    kw = dict(STEADY, groups=300)
    p = Pair(kw)
    e = p.e
    p.init("init_steady", -1, 0)
    with pytest.raises(RaftError) as ei:
        e.feed_poll()
    assert ei.value.code == abi.RAFT_EINVAL and "no feed is open" in str(ei.value)
    with pytest.raises(RaftError) as ei:
        e.feed_cursors()
    assert ei.value.code == abi.RAFT_EINVAL
    for mask in (0, 1 << 5, 0xFF):
        with pytest.raises(RaftError) as ei:
            e.feed_open(mask)
        assert ei.value.code == abi.RAFT_EINVAL and "replica_mask" in str(ei.value)
    for bad in (dict(start=3), dict(start="cursors"), dict(start="cursors", cursors=np.full((300, 5), -1))):
        with pytest.raises(RaftError) as ei:
            e.feed_open(None, **bad)
        assert ei.value.code == abi.RAFT_EINVAL
    base = e.device_bytes()
    p.open()
    assert e.device_bytes() == base + 300 * 5 * 4
    t = p.run(1, 6, 3)
    # FROM_CURSORS with what feed_cursors() returned resumes exactly
    cur = e.feed_cursors()
    e.feed_close()
    assert e.device_bytes() == base
    with pytest.raises(RaftError):
        e.feed_poll()
    t = p.tick(t, 3)
    e.feed_open(None, "cursors", cur)
    p.poll(what="resumed from cursors")
    # closed and reopened FROM_COMMIT: nothing until the next commit
    e.feed_close()
    p.open(start="commit")
    _, info = p.poll(what="reopened from commit")
    assert info == dict(delivered=0, pending=0, lost=0, stalled=0)
    t = p.tick(t, 1)
    _, info = p.poll(what="first commit after reopening")
    assert info["delivered"] == 300 * 5
    # a single-replica mask delivers only that replica
    p.open([3], "start")
    assert (e.feed_cursors()[:, [0, 1, 2, 4]] == -1).all()
    t = p.tick(t, 2)
    got, info = p.poll(what="replica 3 alone")
    assert info["delivered"] > 0 and set(got["replica"].tolist()) == {3}
    # whatever replaces the state closes the feed
    ck = str(tmp_path / "feed.ckpt")
    e.save_checkpoint(ck)
    st = p.o.store_state()
    for replace in (lambda: e.load_state(st), lambda: e.init_steady(-1, 0), lambda: e.load_checkpoint(ck),
                    lambda: e.init_new_nodes(0)):
        e.feed_open()
        e.feed_poll()
        replace()
        with pytest.raises(RaftError) as ei:
            e.feed_poll()
        assert ei.value.code == abi.RAFT_EINVAL
