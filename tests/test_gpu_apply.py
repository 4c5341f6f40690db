"""GPU: the applied state (raft_apply_open / _step / _read / _scan / _close;
k_apply.hip). Every case drives an engine and the oracle alike, steps the
engine, runs the model (tests/apply_model.py) over the oracle's canonical view
with its own records, and asserts that the step's info, apply_read() of all
groups as bytes and apply_scan for both selects equal the model's."""
import ctypes as C

import numpy as np
import pytest

import apply_model as AM
import ceiling_cases as CC
import feed_model as FM
import groups_model as GM
import harness as H
import load_model as LM
import oracle
from raftstep import Engine, RaftError, abi
from test_gpu_feed import CHURN, CRC, STEADY

pytestmark = pytest.mark.gpu
THREADS = 16
BOTH = abi.APPLY_DIVERGED | abi.APPLY_GAPPED


def _same_records(got, want, what):
    assert got.dtype == abi.APPLY_RECORD and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        g, r = (int(x) for x in bad[0])
        raise AssertionError(f"{what}: {len(bad)} records differ, first at group {g} replica {r}: "
                             f"engine {got[g, r]}, model {want[g, r]}")


def check(e, rec, fault, group_base, what):
    """apply_read() of all groups and apply_scan for both selects against the model's records."""
    _same_records(e.apply_read(), rec, what)
    for select in (abi.APPLY_DIVERGED, abi.APPLY_GAPPED):
        hits, info = e.apply_scan(select)
        want, winfo = AM.scan(rec, fault, select, group_base=group_base)
        assert info == winfo, f"{what}: scan {select}: info {info}, model {winfo}"
        assert hits.tobytes() == want.tobytes(), f"{what}: scan {select}: hits differ"


class Pair:
    """An engine and the oracle, driven alike, with an apply on the engine and
    the model's records beside it."""

    def __init__(self, kw):
        self.kw = kw
        self.gb = int(kw.get("group_base", 0))
        self.e = Engine(**kw)
        self.o = oracle.Oracle(**kw)
        self.rec = None
        self.tot = dict(folded=0, lost=0, stalled=0, gapped=0, diverged=0)

    def init(self, how, *a):
        for x in (self.e, self.o):
            getattr(x, how)(*a)

    def open(self, replicas=None, start="start"):
        self.rec = AM.start_records(self.o.store_state(), replicas, start, self.gb)
        self.e.apply_open(replicas, start)

    def tick(self, t, k):
        so = self.o.tick(t, k, threads=THREADS)
        se = self.e.tick(t, k)
        assert list(se) == list(so), f"stats of ticks [{t}, {t + k})"
        return t + k

    def step(self, what):
        st = self.o.store_state()
        info, self.rec = AM.step(st, self.rec, self.gb)
        got = self.e.apply_step()
        assert got == info, f"{what}: info {got}, model {info}"
        check(self.e, self.rec, st["fault"], self.gb, what)
        for k in self.tot:
            self.tot[k] += info[k]
        return info

    def run(self, t, nticks, every):
        end = t + nticks
        while t < end:
            t = self.tick(t, min(every, end - t))
            self.step(f"step after tick {t - 1}")
        return t


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("feed", [False, True], ids=["alone", "beside_a_feed"])
def test_steady_shared_ring_past_the_wrap(feed):
    """REF steady state, entries in the shared ring, stepped after every tick
    for 40 ticks (K=16: the ring wraps twice); G has a partial block and a
    partial wave. A twin engine makes the same calls without an apply: stepping
    keeps the steady tick's forms. With a feed open beside the apply neither
    moves the other: the polls equal the feed model's."""
    p = Pair(STEADY)
    twin = Engine(**STEADY)
    assert p.e.features()["shared_entries"]
    p.init("init_steady", -1, 0)
    twin.init_steady(-1, 0)
    p.open()
    cur = None
    if feed:
        cur = FM.start_cursors(p.o.store_state(), None, "start")
        p.e.feed_open(None, "start")
    for x in (p.e, twin):
        x.diag_read()
    t = 1
    for _ in range(40):
        twin.tick(t, 1)
        t = p.tick(t, 1)
        p.step(f"step after tick {t - 1}")
        if feed:
            want, winfo, cur = FM.poll(p.o.store_state(), cur, None)
            got, info = p.e.feed_poll()
            assert info == winfo and got.tobytes() == want.tobytes(), f"poll after tick {t - 1}"
            assert np.array_equal(p.e.feed_cursors(), cur)
    a, b = p.e.diag_read(), twin.diag_read()
    print("steady:", p.tot, "ticks_steady_form", a["ticks_steady_form"], "ticks_list_skipped", a["ticks_list_skipped"])
    for k in ("ticks", "ticks_steady_form", "ticks_list_skipped"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["ticks_steady_form"] > 0
    # the feed's figure for this shape (tests/test_gpu_feed.py): every entry it delivers is folded here
    assert (p.tot["folded"], p.tot["lost"], p.tot["stalled"], p.tot["diverged"]) == (165620, 0, 0, 0)
    H.assert_same_state(p.e.store_state(), p.o.store_state(), "after the steps")
    assert np.array_equal(twin.state_digest()[0], p.o.state_digest()[0])
    assert np.array_equal(p.e.state_digest()[0], p.o.state_digest()[0])


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [1, 0], ids=["raft", "ref"])
def test_churn_b(sem):
    """CHURN["B"] (leader isolation: LXS, SXS, virtual suffixes, truncated logs,
    three ring segments) and its REF variant: gaps and lost entries on every
    storage form. Model over the oracle: RAFT 994,808 folded, 12 lost, 4 gapped;
    REF 441,848, 21, 3."""
    kw, nticks, every, _, _ = CHURN["B"]
    p = Pair(dict(kw, semantics=sem))
    p.init("init_new_nodes", 0)
    p.open()
    p.run(0, nticks, every)
    print("churn B sem", sem, ":", p.tot)
    assert p.tot["lost"] > 0 and p.tot["gapped"] > 0
    assert (p.tot["folded"], p.tot["lost"], p.tot["gapped"]) == ((994808, 12, 4) if sem else (441848, 21, 3))
    assert p.tot["diverged"] == 0 and p.tot["stalled"] == 0
    H.assert_same_state(p.e.store_state(), p.o.store_state(), "after the steps")


# 3 ------------------------------------------------------------------------
def test_crc_shape_many_entries_per_step():
    """E=16, a step every 2 ticks: up to 32 entries per pair and step in the
    chunked shared ring. Model: 783,088 folded, 752 lost, 47 gapped."""
    p = Pair(CRC)
    p.init("init_steady", -1, 0)
    p.open()
    p.run(1, 20, 2)
    print("crc:", p.tot)
    assert (p.tot["folded"], p.tot["lost"], p.tot["gapped"]) == (783088, 752, 47)


# 4 ------------------------------------------------------------------------
@pytest.mark.parametrize("R,replicas", [(1, None), (8, None), (5, [0, 2])], ids=["r1", "r8", "holes"])
def test_edges_of_r_and_the_mask(R, replicas):
    kw = dict(STEADY, replicas=R, groups=300, isolate_per_65536=6000)
    p = Pair(kw)
    if R == 1:
        # (a lone REF leader never commits: a hand-made state with ten committed entries, then ticks on top)
        st = _handmade(300, 1, STEADY["ring_depth"], 10)
        for x in (p.e, p.o):
            x.load_state(st)
    else:
        p.init("init_steady", -1, 0)
    p.open(replicas)
    p.run(1, 24, 5)
    print("R", R, replicas, p.tot)
    assert p.tot["folded"] > 0
    got = p.e.apply_read()
    if replicas is not None:
        unfed = [r for r in range(R) if r not in replicas]
        assert (got["applied"][:, unfed] == -1).all()
        z = got[:, unfed].copy()
        z["applied"] = 0
        assert not z.tobytes().strip(b"\0")
    # listed reads: any order, repeats
    ids = [299, 0, 7, 299]
    assert p.e.apply_read(ids).tobytes() == p.rec[ids].tobytes()


# 5 ------------------------------------------------------------------------
def _handmade(G, R, K, n):
    """G in-step groups: one leader, every log the same n entries, all committed."""
    rng = np.random.default_rng(77)
    groups = []
    for g in range(G):
        log = [(1 + i // 3, int(rng.integers(0, 1 << 62))) for i in range(n)]
        groups.append([H.node(H.L if r == 0 else H.F, 2, 1, log, commit=n, match=[0] + [n] * (R - 1), deadline=1000)
                       for r in range(R)])
    return H.build_state(groups, R, K)


@pytest.mark.parametrize("what", ["value", "term"])
def test_injected_divergence(what):
    """One committed entry of one replica altered in the first, a middle and
    the last group of a block (and in the ragged last block): the model's
    witness, lowest index and lowest peer. A twin without the alteration
    reports none."""
    G, R, K, n = 256 + 9, 3, 8, 6
    kw = dict(replicas=R, groups=G, ring_depth=K, client_period=0, group_base=1000)
    clean = _handmade(G, R, K, n)
    st = {k: v.copy() for k, v in clean.items()}
    cases = {0: (1, 2), 100: (2, 6), 255: (0, 1), 264: (1, 4)}      # group: (replica, index)
    for g, (r, i) in cases.items():
        if what == "value":
            st["log_value"][g, r, (i - 1) % K] ^= 1 << 40
        else:
            st["log_term"][g, r, (i - 1) % K] += 1
    e, twin = Engine(**kw), Engine(**kw)
    e.load_state(st)
    twin.load_state(clean)
    for x in (e, twin):
        x.apply_open(None, "start")
    rec = AM.start_records(st, None, "start", 1000)
    info, rec = AM.step(st, rec, 1000)
    assert info["diverged"] == len(cases) and info["folded"] == G * R * n
    assert e.apply_step() == info
    check(e, rec, st["fault"], 1000, "after the step")
    hits, sinfo = e.apply_scan(abi.APPLY_DIVERGED)
    assert [int(x) for x in hits["local"]] == sorted(cases) and sinfo["matched"] == len(cases)
    for h in hits:
        r, i = cases[int(h["local"])]
        # the altered replica differs from both others at i; the lowest diverged replica is the witness
        a = 0
        b = r if r != 0 else 1
        assert (int(h["a"]), int(h["b"]), int(h["index"]), int(h["flags"])) == (a, b, i, abi.APPLY_DIVERGED)
    # a second step changes nothing: sticky, and nothing new to fold
    info2, rec2 = AM.step(st, rec, 1000)
    assert e.apply_step() == info2 == dict(folded=0, lost=0, stalled=0, gapped=0, diverged=0)
    check(e, rec2, st["fault"], 1000, "after the second step")
    t = twin.apply_step()
    assert t["diverged"] == 0 and t["folded"] == G * R * n
    assert twin.apply_scan(BOTH)[1]["matched"] == 0 and not twin.apply_read()["div_index"].any()


# 6 ------------------------------------------------------------------------
def test_from_records():
    kw = dict(STEADY, groups=300, isolate_per_65536=6000)
    p = Pair(kw)
    other = Engine(**kw)
    p.init("init_steady", -1, 0)
    other.init_steady(-1, 0)
    p.open()
    other.apply_open(None, "start")
    t = p.run(1, 9, 3)
    other.tick(1, 3), other.apply_step(), other.tick(4, 3), other.apply_step(), other.tick(7, 3), other.apply_step()
    # read, close, reopen from the records: continues as the engine that never closed
    saved = other.apply_read()
    _same_records(saved, p.rec, "before closing")
    other.apply_close()
    other.apply_open(None, "records", saved)
    for _ in range(3):
        other.tick(t, 3)
        t = p.tick(t, 3)
        p.step(f"step after tick {t - 1}")
        other.apply_step()
    _same_records(other.apply_read(), p.rec, "resumed from records")
    # invalid records are refused, the open apply stays as it is
    before = p.e.apply_read()
    for field, value in (("base", -1), ("reserved", 1), ("base", 1 << 30)):
        bad = before.copy()
        bad[299, 4][field] = value
        with pytest.raises(RaftError) as ei:
            p.e.apply_open(None, "records", bad)
        assert ei.value.code == abi.RAFT_EINVAL and "group 299 replica 4" in str(ei.value)
        assert p.e.apply_read().tobytes() == before.tobytes()
    with pytest.raises(RaftError) as ei:
        p.e.apply_open(None, "records")
    assert ei.value.code == abi.RAFT_EINVAL
    bad = before.copy()
    bad[5, 1]["reserved"] = 3                       # (outside the mask: not read)
    p.e.apply_open([0, 2, 3, 4], "records", bad)
    assert (p.e.apply_read()["applied"][:, 1] == -1).all()
    # records placed above min(commit, last) stall and stay bit for bit
    high = before.copy()
    high["applied"][10:20] += 1000
    high["base"][10:20] += 1000
    p.e.apply_open(None, "records", high)
    p.rec = high.copy()
    t = p.tick(t, 2)
    info = p.step("placed above the commit index")
    assert info["stalled"] == 10 * 5
    assert p.e.apply_read()[10:20].tobytes() == high[10:20].tobytes()


# 7 ------------------------------------------------------------------------
def test_restart_and_load_groups_with_an_apply_open():
    kw = dict(replicas=3, groups=LM.G, ring_depth=16, entries_per_tick=1, client_period=1, seed=0x5EED0001,
              isolate_per_65536=8000, isolate_min_ticks=4, isolate_max_ticks=16, group_base=5000)
    p = Pair(kw)
    p.init("init_new_nodes", 0)
    p.open([0, 2], "start")
    t = p.run(0, 60, 20)
    ids = np.array([0, 255, 256, 700, LM.G - 1])
    p.e.restart_groups(ids, t)
    GM.restart(p.o, ids, t)
    want = AM.reset_records(p.rec, p.o.store_state(), ids, "start", p.gb)
    others = np.setdiff1d(np.arange(LM.G), ids)
    assert want[others].tobytes() == p.rec[others].tobytes() and (want["applied"][ids][:, [0, 2]] == 0).all()
    p.rec = want
    check(p.e, p.rec, p.o.store_state()["fault"], p.gb, "after the restart")
    t = p.run(t, 12, 4)
    donor = LM.donor(LM.DONOR_REF)
    idx = LM.pick(donor, 0, 16, 40, 23)
    rows = LM.take(donor, idx)
    ids = np.random.default_rng(9).permutation(LM.G)[:len(idx)]
    p.e.load_groups(ids, rows)
    LM.load(p.o, ids, rows)
    want = AM.reset_records(p.rec, p.o.store_state(), ids, "commit", p.gb)
    others = np.setdiff1d(np.arange(LM.G), ids)
    assert want[others].tobytes() == p.rec[others].tobytes()
    assert np.array_equal(want["applied"][ids][:, 0], np.minimum(rows["commit"], rows["last"])[:, 0])
    p.rec = want
    check(p.e, p.rec, p.o.store_state()["fault"], p.gb, "after the load")
    p.run(t, 12, 4)
    H.assert_same_state(p.e.store_state(), p.o.store_state(), "at the end")


# 8 ------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [0, 1], ids=["ref", "raft"])
def test_int32_ceiling(sem):
    """In-step groups a few entries below 2^31-1 (tests/ceiling_cases.py), opened
    FROM_COMMIT and ticked into the ceiling: the step ends, and records reach
    applied = 2^31-1 (REF; RAFT: 2^31-2, where its logs stop)."""
    kw = CC.config("plain", sem, 1)
    st0 = CC.start_state(sem, False)
    p = Pair(kw)
    for x in (p.e, p.o):
        x.load_state(st0)
    p.open(None, "commit")
    top = H.I32 - sem                                 # (a RAFT log stops one entry lower: 2^31 is no NextIndex)
    at_top = int((p.rec["applied"] == top).sum())
    p.run(CC.T0, 12, 2)
    print("ceiling sem", sem, ":", p.tot, "records at the top:", at_top, "->", int((p.rec["applied"] == top).sum()))
    # (conditions on the model's result: records arrive at the top by folding, not only by being opened there)
    assert int(p.rec["applied"].max()) == top and int((p.rec["applied"] == top).sum()) > at_top
    assert p.tot["folded"] > 0 and p.tot["diverged"] == 0
    # from the start, far behind: one gap per pair, then the K entries below the ceiling
    p.open(None, "start")
    info = p.step("from index 0 at the ceiling")
    assert info["gapped"] == CC.G * CC.R and info["folded"] > 0


# 9 ------------------------------------------------------------------------
def test_errors_and_lifecycle(tmp_path):
    kw = dict(STEADY, groups=300)
    p = Pair(kw)
    e = p.e
    p.init("init_steady", -1, 0)
    for call in (e.apply_step, e.apply_read, lambda: e.apply_read([0]), lambda: e.apply_scan(BOTH)):
        with pytest.raises(RaftError) as ei:
            call()
        assert ei.value.code == abi.RAFT_EINVAL and "no apply is open" in str(ei.value)
    e.apply_close()                                   # (nothing open: nothing to do)
    for mask in (0, 1 << 5, 0xFF):
        with pytest.raises(RaftError) as ei:
            e.apply_open(mask)
        assert ei.value.code == abi.RAFT_EINVAL and "replica_mask" in str(ei.value)
    with pytest.raises(RaftError) as ei:
        e.apply_open(None, 3)
    assert ei.value.code == abi.RAFT_EINVAL
    base = e.device_bytes()
    p.open()
    assert e.device_bytes() == base + 300 * 5 * 32
    p.open([1, 3])                                    # opening an open apply replaces it
    assert e.device_bytes() == base + 300 * 2 * 32
    t = p.run(1, 4, 2)
    assert e.lib.raft_apply_step(e.h, None) == abi.RAFT_EINVAL
    for ids in ([300], [0, 1 << 40]):
        with pytest.raises(RaftError) as ei:
            e.apply_read(ids)
        assert ei.value.code == abi.RAFT_ERANGE
    buf = np.zeros((301, 5), abi.APPLY_RECORD)
    assert e.lib.raft_apply_read(e.h, None, 301, buf.ctypes.data) == abi.RAFT_ERANGE and not buf.tobytes().strip(b"\0")
    for select in (0, 4, 7):
        with pytest.raises(RaftError) as ei:
            e.apply_scan(select)
        assert ei.value.code == abi.RAFT_EINVAL
    with pytest.raises(RaftError) as ei:
        e.apply_scan(BOTH, first_group=301)
    assert ei.value.code == abi.RAFT_ERANGE
    sinfo = abi.ScanInfo()
    assert e.lib.raft_apply_scan(e.h, BOTH, 0, None, 5, C.byref(sinfo)) == abi.RAFT_EINVAL   # cap without a buffer
    assert e.apply_scan(BOTH, first_group=300)[1] == dict(matched=0, written=0, next_group=300)
    # handler batches, ticks and proposals leave it open
    e.propose(t, [0, 1], [5, 6])
    p.o.load_state(e.store_state())
    p.step("after a proposal")
    e.apply_close()
    e.apply_close()
    assert e.device_bytes() == base
    with pytest.raises(RaftError):
        e.apply_step()
    # whatever replaces the state closes it
    ck = str(tmp_path / "apply.ckpt")
    e.save_checkpoint(ck)
    st = p.o.store_state()
    for replace in (lambda: e.init_steady(-1, 0), lambda: e.load_state(st), lambda: e.load_checkpoint(ck),
                    lambda: e.init_new_nodes(0)):
        e.apply_open()
        e.apply_step()
        replace()
        with pytest.raises(RaftError) as ei:
            e.apply_step()
        assert ei.value.code == abi.RAFT_EINVAL
        assert e.device_bytes() == base


def test_scan_pages_like_the_directory():
    """Gapped groups of a consumer that falls behind, paged with small caps:
    the pages' concatenation equals the whole scan, next_group as the model's."""
    kw = dict(STEADY, groups=700)
    p = Pair(kw)
    p.init("init_steady", -1, 0)
    p.open([0, 4], "start")
    t = p.tick(1, 25)
    info = p.step("25 ticks behind a ring of 16")
    assert info["gapped"] == 700 * 2 and info["lost"] == 700 * 2 * 9
    fault = p.o.store_state()["fault"]
    whole, winfo = p.e.apply_scan(abi.APPLY_GAPPED)
    assert winfo == dict(matched=700, written=700, next_group=700)
    first, pages = 0, []
    for cap in (1, 255, 2, 300, 1000):
        hits, hinfo = p.e.apply_scan(abi.APPLY_GAPPED, first, cap)
        want, minfo = AM.scan(p.rec, fault, abi.APPLY_GAPPED, first, cap)
        assert hinfo == minfo and hits.tobytes() == want.tobytes()
        pages.append(hits)
        first = hinfo["next_group"]
    assert first == 700 and np.concatenate(pages).tobytes() == whole.tobytes()
    assert p.e.apply_scan(abi.APPLY_GAPPED, 300, 0)[1] == dict(matched=400, written=0, next_group=300)
    assert p.e.apply_scan(abi.APPLY_DIVERGED)[1]["matched"] == 0
