"""GPU: the engine against the oracle at the top of the int32 range (I =
2^31-1), bit-exact: handler batches and single ticks from random near-ceiling
states, tick traces that walk in-step groups into the ceiling on every device
path, the readers of such a trace, and the end of virtual time. The oracle
holds these logs as a window (oracle/raft_oracle.c, o_node.base), which
tests/test_oracle_ceiling.py ties to the dense storage of the older tests."""
import os

import numpy as np
import pytest

import ceiling_cases as CC
import feed_model as FM
import groups_model as GM
import harness as H
from raftstep import RaftError, abi
from test_gpu_parity import compare, pair

pytestmark = pytest.mark.gpu
I = H.I32
SEMS = [abi.SEM_REF, abi.SEM_RAFT]


def _digests(e, o, what):
    de, do = e.state_digest(), o.state_digest()
    assert np.array_equal(de[0], do[0]) and de[1] == do[1], f"{what}: digests differ"


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("R,crc", [(1, 0), (3, 0), (5, 0), (8, 0), (5, 1)])
def test_handler_batches_ceiling_states(R, crc, sem):
    """test_handler_batches_random_states with every term in I-5..I, every index
    in I-12..I and 0..11 entries per request."""
    rng = np.random.default_rng(3000 + R + 50 * crc + 7 * sem)
    G, K = 192, 8
    e, o = pair(replicas=R, groups=G, ring_depth=K, seed=0xCE1 + R, payload_crc=crc, semantics=sem)
    st = H.ceiling_state(rng, G, R, K, raft=sem == abi.SEM_RAFT)
    if crc:
        H.stamp_crcs(st)
    e.load_state(st)
    o.load_state(st)
    compare(e, o, "after load")
    _digests(e, o, "after load")
    for rnd in range(12):
        now = int(rng.integers(0, 40))
        kind = rnd % 3
        groups = rng.permutation(G)[: G // 2]
        tm = lambda: int(rng.integers(I - 5, I + 1))      # noqa: E731
        ix = lambda: int(rng.integers(I - 12, I + 1))     # noqa: E731
        if kind == 0:
            items = [dict(group=int(g), to=int(rng.integers(0, R)), term=tm(), prev_log_index=ix(),
                          prev_log_term=tm(), leader_commit=ix(),
                          logs=[(tm(), int(rng.integers(0, 1 << 62))) for _ in range(int(rng.integers(0, 12)))])
                     for g in groups]
            reqs, ents = H.ae_reqs(items)
            a, b = e.append_entries(now, reqs, ents), o.append_entries(now, reqs, ents)
        elif kind == 1:
            reqs = H.vote_reqs([dict(group=int(g), to=int(rng.integers(0, R)), term=tm(),
                                     candidate_id=int(rng.integers(0, R))) for g in groups])
            reqs["last_log_index"] = rng.integers(I - 12, I + 1, len(reqs))
            reqs["last_log_term"] = rng.integers(I - 5, I + 1, len(reqs))
            a, b = e.request_vote(now, reqs), o.request_vote(now, reqs)
        else:
            ops = H.ops([dict(group=int(g), replica=int(rng.integers(0, R)), kind=int(rng.integers(1, 6)),
                              arg=int(rng.integers(0, 1 << 62))) for g in groups])
            a, b = e.group_ops(now, ops), o.group_ops(now, ops)
        assert a.tobytes() == b.tobytes(), f"round {rnd} kind {kind}: responses differ"
        compare(e, o, f"round {rnd} kind {kind}")
        _digests(e, o, f"round {rnd}")
    assert (o.store_state()["fault"] == abi.F_OVERFLOW).any()    # the guards were met at all


def _run_trace(e, o, kw, st0, staged=False, diag=False):
    e.load_state(st0)
    o.load_state(st0)
    compare(e, o, "after load")
    if diag:
        e.diag_enable(True)
    tot_e, tot_o = np.zeros(8, np.int64), np.zeros(8, np.int64)
    for t in range(CC.T0, CC.T0 + CC.NTICKS, CC.EVERY):
        if staged:
            v = H.staged_values(kw["seed"], t, CC.EVERY, kw["entries_per_tick"], CC.G)
            e.stage_values(t, v)
            o.stage_values(t, v)
        se, so = e.tick(t, CC.EVERY), o.tick(t, CC.EVERY)
        assert list(se) == list(so), f"stats of ticks [{t}, {t + CC.EVERY}): engine {list(se)}, oracle {list(so)}"
        tot_e += se
        tot_o += so
        compare(e, o, f"after tick {t + CC.EVERY - 1}")
        _digests(e, o, f"after tick {t + CC.EVERY - 1}")
    s = o.store_state()
    assert (s["fault"] == abi.F_OVERFLOW).sum() >= CC.G // 4 and (s["fault"] == 0).sum() >= CC.G // 4


@pytest.mark.parametrize("path", ["auto", "single", "general"])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name", sorted(CC.CONFIGS))
def test_tick_trace_crosses_the_ceiling(name, sem, E, path):
    kw = CC.config(name, sem, E)
    e, o = pair(general=(path == "general"), single=(path == "single"), **kw)
    diag = path == "auto" and name == "leader_iso"
    _run_trace(e, o, kw, CC.start_state(sem, kw.get("payload_crc", 0)), diag=diag)
    if diag:
        # the lean kernel's own bail / take terms were the ones deciding. LXS and
        # SXS (a cut-off leader appending alone, beside its successor) are forms
        # of RAFT groups only (k_fast.hip lean_tick: `RAFT && lxs`, `RAFT && !CRC
        # && sxs`): REF has no such classes (its groups freeze at a new leader's first
        # contact, KAT-11), so the two are asserted on the RAFT traces.
        d = e.diag_read()
        print(name, sem, E, {k: v for k, v in d.items() if v})
        need = ("lean_ssync", "lean_passed", "list_lanes") + (("lean_lxs", "lean_sxs") if sem == abi.SEM_RAFT else ())
        for k in need:
            assert d[k] > 0, (k, d)


@pytest.mark.parametrize("sem", SEMS)
def test_staged_trace_crosses_the_ceiling(sem):
    kw = CC.config("plain", sem, 3, client_source=abi.CLIENT_STAGED)
    e, o = pair(**kw)
    _run_trace(e, o, kw, CC.start_state(sem, 0), staged=True)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("R", [3, 5, 7])
def test_tick_from_ceiling_states(R, sem):
    """test_tick_from_random_states at the ceiling: 30 single ticks."""
    rng = np.random.default_rng(177 + R + sem)
    G, K = 512, 16
    e, o = pair(replicas=R, groups=G, ring_depth=K, client_period=2, seed=1900 + R, isolate_per_65536=8000,
                semantics=sem)
    st = H.ceiling_state(rng, G, R, K, raft=sem == abi.SEM_RAFT)
    e.load_state(st)
    o.load_state(st)
    for t in range(30, 60):
        se, so = e.tick(t, 1), o.tick(t, 1)
        assert list(se) == list(so), (R, t)
        compare(e, o, f"R={R} tick {t}")
    _digests(e, o, "at the end")


def test_readers_at_the_ceiling(tmp_path):
    """The commit feed, the group directory and a checkpoint over one crossing
    trace (REF, leader isolation, E = 3)."""
    kw = CC.config("leader_iso", abi.SEM_REF, 3)
    e, o = pair(**kw)
    st0 = CC.start_state(abi.SEM_REF, 0)
    e.load_state(st0)
    o.load_state(st0)
    cur = FM.start_cursors(o.store_state(), None, "start")
    e.feed_open(None, "start")
    for t in range(CC.T0, CC.T0 + CC.NTICKS, 4):
        assert list(e.tick(t, 4)) == list(o.tick(t, 4))
        want, info, cur = FM.poll(o.store_state(), cur, None, 0)
        got, ginfo = e.feed_poll(None)
        assert ginfo == info and got.tobytes() == want.tobytes(), f"feed after tick {t + 3}"
        assert np.array_equal(e.feed_cursors(), cur)
    e.feed_close()
    so = o.store_state()
    hits, info = e.group_scan(abi.SELECT_FAULTED)
    whits, winfo = GM.scan(so, abi.SELECT_FAULTED, 0, None, 0)
    assert info == winfo and hits.tobytes() == whits.tobytes() and winfo["matched"] >= CC.G // 4
    got = e.store_groups(hits["group"])
    for k, v in got.items():
        assert np.array_equal(v, so[k][hits["local"]]), k
    path = os.path.join(tmp_path, "ceiling.ckpt")
    e.save_checkpoint(path)
    dig = e.state_digest()
    e2, _ = pair(**kw)
    e2.load_checkpoint(path)
    d2 = e2.state_digest()
    assert np.array_equal(dig[0], d2[0]) and dig[1] == d2[1] == o.state_digest()[1]
    H.assert_same_state(e2.store_state(), so, "after the checkpoint")


def test_virtual_time_ends_where_check_ticks_says():
    """Virtual seconds are int32: a call is refused when (first + n) *
    tick_seconds + the longest timer reaches 2^31. With the default config
    (2 s per tick, timers below 30 s) the last 30-tick call starts at FIRST."""
    FIRST, n = (2**31 - 1 - 30) // 2 - 30, 30
    e, o = pair(replicas=3, groups=300, client_period=1, seed=0x71CE)
    e.init_new_nodes(FIRST - 1)
    o.init_new_nodes(FIRST - 1)
    assert list(e.tick(FIRST, n)) == list(o.tick(FIRST, n))
    compare(e, o, "after the last 30 ticks of virtual time")
    assert (o.store_state()["role"] == abi.LEADER).any()
    before = e.state_digest()
    with pytest.raises(RaftError) as err:
        e.tick(FIRST + 1, n)
    assert err.value.code == abi.RAFT_ERANGE
    after = e.state_digest()
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
