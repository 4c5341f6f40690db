"""CPU: the model of raft_load_groups (tests/load_model.py) against rows
derived by hand from the header's rules, and the coverage of the donor states
every load test takes its rows from."""
import numpy as np
import pytest

import harness as H
import load_model as LM
import oracle
from raftstep import abi

F, C, L = H.F, H.C, H.L
OPTIONAL = ("log_crc", "next", "hwm", "iso_victim")


def _cfg(**kw):
    return abi.default_config(**kw)


def _without(rows, *fields):
    return {k: v for k, v in rows.items() if k not in fields}


def _hand_rows(R, K):
    """Three groups: a Leader over two Followers (one lagging), new nodes with
    empty logs, and a log past the ring wrap."""
    e = [(1, 100 + i) for i in range(1, 6)]
    long_log = [(2, 1000 + i) for i in range(1, 22)]            # 21 entries, K = 8: indices 14..21 in the ring
    groups = [
        [H.node(L, 1, 1, e, commit=4, deadline=50, timeout=0, match=[0, 5, 3]),
         H.node(F, 1, 1, e, commit=4, deadline=80, timeout=25),
         H.node(F, 1, 1, e[:3], commit=3, deadline=75, timeout=20)],
        [H.node(F, 0, 0, (), deadline=30, timeout=12), H.node(F, 0, 0, (), deadline=31, timeout=13),
         H.node(C, 1, 1, (), deadline=29, timeout=11)],
        [H.node(F, 2, 1, long_log[-K:], commit=20, deadline=90, timeout=22, last=21),
         H.node(F, 2, 1, long_log[-K - 1:-1], commit=20, deadline=91, timeout=23, last=20),
         H.node(C, 3, 1, long_log[-K - 2:-2], commit=19, deadline=92, timeout=12, last=19)],
    ]
    return H.build_state(groups, R, K)


@pytest.mark.parametrize("semantics", [0, 1], ids=["ref", "raft"])
@pytest.mark.parametrize("payload_crc", [0, 1], ids=["nocrc", "crc"])
def test_complete_derives_the_optional_fields(semantics, payload_crc):
    R, K = 3, 8
    cfg = _cfg(replicas=R, groups=3, ring_depth=K, semantics=semantics, payload_crc=payload_crc)
    rows = _without(_hand_rows(R, K), *OPTIONAL)
    assert set(rows) == set(abi.STATE_FIELDS) - set(OPTIONAL)
    got = LM.complete(cfg, rows)
    assert set(got) == set(abi.STATE_FIELDS)
    for k in rows:   # what was given reads back as given
        assert np.array_equal(got[k], rows[k]), k
    # a Leader row with next absent: match + 1 for the peers, 0 for itself and for rows of non-leaders
    assert got["next"][0, 0].tolist() == [0, 6, 4]
    assert not got["next"][0, 1:].any() and not got["next"][1:].any()
    # hwm absent: last (the empty logs: 0)
    assert np.array_equal(got["hwm"], rows["last"]) and got["hwm"][1].tolist() == [0, 0, 0]
    assert not got["iso_victim"].any()
    # stamps: CRC32C of (term, value) of every live entry, 0 elsewhere and without payload_crc
    want = np.zeros((3, R, K), np.uint32)
    if payload_crc:
        for g in range(3):
            for r in range(R):
                last = int(rows["last"][g, r])
                for i in range(max(1, last - K + 1), last + 1):
                    s = (i - 1) % K
                    want[g, r, s] = oracle.entry_crc(int(rows["log_term"][g, r, s]), int(rows["log_value"][g, r, s]))
        assert want[0, 0, :5].all() and not want[1].any() and want[2].all()
    assert np.array_equal(got["log_crc"], want)


def test_complete_keeps_given_optional_fields_and_lifts_a_low_hwm():
    R, K = 3, 8
    cfg = _cfg(replicas=R, groups=3, ring_depth=K, semantics=1, payload_crc=1)
    rows = _hand_rows(R, K)
    rows["next"][0, 0] = [0, 4, 0]            # a stored NextIndex below match + 1; 0 still derives
    rows["hwm"][:] = rows["last"]
    rows["hwm"][0, 2] = 5                     # truncated from 5 to 3 entries: inside (hwm - K, hwm]
    rows["hwm"][2, 0] = 7                     # below last = 21: means last
    rows["iso_victim"][1] = 0x9A              # parities: 8 | 2 and 8 | 1
    rows["log_crc"][0, 0, :5] = [11, 12, 13, 14, 15]
    got = LM.complete(cfg, rows)
    assert got["next"][0, 0].tolist() == [0, 4, 4]
    assert got["hwm"][0].tolist() == [5, 5, 5] and got["hwm"][2].tolist() == [21, 20, 19]
    assert got["iso_victim"].tolist() == [0, 0x9A, 0]
    assert got["log_crc"][0, 0, :5].tolist() == [11, 12, 13, 14, 15]   # given stamps are kept, not recomputed


def test_load_splices_and_leaves_the_others():
    kw = dict(LM.DONOR_REF, groups=40)
    st = LM.donor(kw)
    with oracle.Oracle(**kw) as o:
        o.init_new_nodes(0)
        o.tick(0, 20, threads=4)
        before = o.store_state()
        dig = o.state_digest()[0]
        ids = np.array([39, 0, 17])
        rows = LM.take(st, [5, 6, 7])
        LM.load(o, ids, _without(rows, *OPTIONAL[1:]))
        after = o.store_state()
        others = np.setdiff1d(np.arange(40), ids)
        for k in after:
            assert np.array_equal(after[k][others], before[k][others]), k
            if k != "iso_victim":
                assert np.array_equal(after[k][ids], rows[k]), k
        assert np.array_equal(o.state_digest()[0][others], dig[others])


def test_load_cursors_on_a_mask_with_unfed_replicas():
    cur = np.array([[3, -1, 4], [9, -1, 9], [0, -1, 0], [7, -1, 2]], np.int32)
    rows = dict(commit=np.array([[5, 5, 2], [0, 0, 0]], np.int32), last=np.array([[4, 6, 6], [0, 0, 0]], np.int32))
    got = LM.load_cursors(cur, [3, 1], rows)
    assert got.tolist() == [[3, -1, 4], [0, -1, 0], [0, -1, 0], [4, -1, 2]]
    assert got.dtype == np.int32 and cur[3, 0] == 7   # (a copy)


def _counts(st, raft, K):
    return {k: int(m.sum()) for k, m in LM.classes(st, raft, K).items()}


def test_the_donors_hold_every_class():
    K = LM.DONOR["ring_depth"]
    ref = LM.donor(LM.DONOR_REF)
    n = _counts(ref, False, K)
    print("REF donor:", n)
    assert all(v >= 1 for v in n.values()), n
    assert n["wrapped"] > LM.G // 2   # logs past the ring wrap are the rule (groups frozen early stay short)
    raft = LM.donor(LM.DONOR_RAFT)
    n = _counts(raft, True, K)
    print("RAFT donor:", n)
    assert all(v >= 1 for v in n.values()), n
    ref0 = LM.donor(dict(LM.DONOR_REF, isolate_leader=0))
    n4 = int((ref0["fault"] == abi.F_RING_EVICTED).sum())
    print("REF donor with isolate_leader = 0: code 4 in", n4)
    assert n4 >= 1
    for st, is_raft, seed in ((ref, False, 1), (raft, True, 2)):
        rows = LM.pick(st, is_raft, K, 100, seed)
        assert 90 <= len(rows) <= 110 and len(set(rows.tolist())) == len(rows)
