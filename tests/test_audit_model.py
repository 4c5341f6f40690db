"""CPU: the group audit's numpy model (tests/audit_model.py) on hand-derived
cases (one minimal state per check with the expected record written out by
hand; tests/test_gpu_group_audit.py loads the same states into engines), the
record layouts against the header, the model over oracle traces and over
injected violations. The properties are test_oracle_raft.py's (election
safety, log matching, committed-prefix agreement), here per group with a
witness; COMMIT_BEYOND_LOG is a REF follower's CommitIndex = LastApplied + 1
(main.go:152) made visible."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import audit_model as AM
import groups_model as GM
import harness as H
import oracle
from raftstep import abi

THREADS = 16
F, L = H.F, H.L
I = H.I32
X = abi.NO_REPLICA
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raftstep.h")
K = 8


def _same3(log, **kw):
    return [H.node(log=log, **kw) for _ in range(3)]


def _wrapped():
    """13 entries in a ring of 8: indices 6..13 live, index 9 in slot 0; replica 1 differs at 6."""
    log = [(1 if i <= 9 else 2, 100 + i) for i in range(1, 14)]
    other = list(log)
    other[5] = (1, 999)     # index 6, the low end of the window
    other[2] = (7, 7)       # index 3 has left the ring: not looked at
    return [H.node(term=2, log=log, commit=5), H.node(term=2, log=other, commit=5), H.node(term=2, log=log, commit=5)]


def _ceiling():
    """last = 2^31-1: replica 1's last value differs (terms equal there: LOG_MATCHING at 2^31-1, and both
    have committed it); replica 2's last entry carries a term above its own."""
    log = [(I - 1, 50 + j) for j in range(K)]
    return [H.node(term=I, log=log, last=I, commit=I),
            H.node(term=I, log=log[:-1] + [(I - 1, 4242)], last=I, commit=I),
            H.node(term=I - 1, log=log[:-1] + [(I, 50 + K - 1)], last=I, commit=I - 3)]


# name -> (nodes, expected (violated, a, b, index, check) or None for a group that is no hit)
REF_CASES = {
    "clean": (_same3([(1, 10), (1, 11), (2, 12)], term=2, commit=3), None),
    "two_leaders": ([H.node(role=L, term=3), H.node(role=L, term=3), H.node(term=3)], (1, 0, 1, 3, 1)),
    "leaders_of_two_terms": ([H.node(role=L, term=3), H.node(role=L, term=4), H.node(term=4)], None),
    "log_matching": ([H.node(term=2, log=[(1, 10), (1, 11), (2, 12)]), H.node(term=2, log=[(1, 10), (1, 99), (2, 12)]),
                      H.node(term=2, log=[(1, 10), (1, 11), (2, 12)])], (2, 0, 1, 2, 2)),
    # the terms agree only below the unequal index: a committed divergence, no log-matching violation
    "commit_diverged_only": ([H.node(term=3, log=[(1, 10), (1, 11), (2, 12)], commit=3),
                              H.node(term=3, log=[(1, 10), (1, 11), (3, 13)], commit=3),
                              H.node(term=3, log=[(1, 10), (1, 11), (2, 12)], commit=0)], (4, 0, 1, 3, 4)),
    "term_descends": (_same3([(2, 1), (1, 2), (3, 3)], term=3), (8, 0, X, 2, 8)),
    "term_above_own": ([H.node(term=2, log=[(1, 1), (2, 2)]), H.node(term=1, log=[(1, 1), (2, 2)]),
                        H.node(term=2, log=[(1, 1), (2, 2)])], (8, 1, X, 2, 8)),
    "commit_beyond_log": ([H.node(term=1, log=[(1, 5)], commit=1), H.node(term=1, log=[(1, 5)], commit=1),
                           H.node(term=1, log=[(1, 5)], commit=2)], (32, 2, X, 2, 32)),
    # three checks at once: the record carries the lowest one's witness
    "several": ([H.node(role=L, term=2, log=[(1, 10), (2, 11)]), H.node(role=L, term=2, log=[(1, 77), (2, 11)]),
                 H.node(term=2, log=[(1, 10), (2, 11)], commit=3)], (1 | 2 | 32, 0, 1, 2, 1)),
    "wrapped": (_wrapped(), (2, 0, 1, 6, 2)),
    "ceiling": (_ceiling(), (2 | 4 | 8, 0, 1, I, 2)),
}
R1_CASES = {
    "clean": ([H.node(role=L, term=2, log=[(1, 1), (2, 2)], commit=2)], None),
    "r1": ([H.node(role=L, term=2, log=[(1, 1), (3, 2)], commit=3)], (8 | 32, 0, X, 2, 8)),
}


def hand_state(cases, R):
    return H.build_state([nodes for nodes, _ in cases.values()], R, K)


def raft_hand_state():
    """RAFT rows with hwm > last: replica 1 was truncated from 12 to 6, so its ring holds 5..6 only; what sits
    in the slots of 1..4 is not its log. Group 0: it agrees with the others at 5 and 6. Group 1: it differs at 6."""
    a = [(1, 10 + i) for i in range(1, 11)]
    groups = []
    for v6 in (16, 666):
        b = [(9, 900 + i) for i in range(1, 5)] + [(1, 15), (1, v6)]
        groups.append([H.node(term=1, log=a, commit=2), H.node(term=1, log=b, commit=2), H.node(term=1, log=a, commit=2)])
    st = H.build_state(groups, 3, K)
    st["hwm"][:] = st["last"]
    st["hwm"][:, 1] = 12
    return st, [None, (2, 0, 1, 6, 2)]


def crc_hand_state():
    """payload_crc rows, 10 entries in a ring of 8 (3..10 live, 9 in slot 0). Group 0: every stamp right.
    Group 1: replica 1's stamps of 3 and 10 (both ends of its window) and replica 2's of 9 (the slot that
    wraps) flipped."""
    log = [(1 + i // 6, 1000 + i) for i in range(1, 11)]
    st = H.stamp_crcs(H.build_state([_same3(log, term=2, commit=4), _same3(log, term=2, commit=4)], 3, K))
    for r, i in ((1, 3), (1, 10), (2, 9)):
        st["log_crc"][1, r, (i - 1) % K] ^= 1 << (i % 32)
    return st, [None, (16, 1, X, 3, 16)]


def records(hits):
    return {int(h["local"]): (int(h["violated"]), int(h["a"]), int(h["b"]), int(h["index"]), int(h["check"]))
            for h in hits}


def expected(want):
    return {g: w for g, w in enumerate(want) if w is not None}


# hand-derived cases ---------------------------------------------------------
def test_hand_cases_one_per_check():
    st = hand_state(REF_CASES, 3)
    hits, info = AM.audit(st, group_base=100)
    want = expected([w for _, w in REF_CASES.values()])
    assert records(hits) == want
    assert [int(h["group"]) for h in hits] == [100 + g for g in want] and not hits["fault"].any()
    names = list(REF_CASES)
    per = {k: 0 for k in abi.AUDIT_NAMES}
    for w in want.values():
        for k, name in enumerate(abi.AUDIT_NAMES):
            per[name] += (w[0] >> k) & 1
    assert info == dict(matched=len(want), written=len(want), next_group=len(names), per_check=per)
    assert per["stamp"] == 0    # (no payload_crc: accepted and never violated)


def test_only_the_requested_checks_and_the_lowest_ones_witness():
    st = hand_state(REF_CASES, 3)
    g = list(REF_CASES).index("several")
    hits, _ = AM.audit(st, AM.LOG_MATCHING | AM.COMMIT_BEYOND_LOG)
    assert records(hits)[g] == (2 | 32, 0, 1, 1, 2)           # the first entries differ, the second have equal terms
    hits, _ = AM.audit(st, AM.COMMIT_BEYOND_LOG)
    assert records(hits)[g] == (32, 2, X, 3, 32)
    hits, info = AM.audit(st, AM.COMMIT_DIVERGED)
    assert records(hits) == {list(REF_CASES).index("commit_diverged_only"): (4, 0, 1, 3, 4),
                             list(REF_CASES).index("ceiling"): (4, 0, 1, I, 4)}
    c = list(REF_CASES).index("ceiling")
    assert records(AM.audit(st, AM.TERM_ORDER)[0])[c] == (8, 2, X, I, 8)


def test_paging_follows_the_scan():
    st = hand_state(REF_CASES, 3)
    whole, winfo = AM.audit(st)
    n, G = winfo["matched"], len(REF_CASES)
    out, info = AM.audit(st, cap=0)
    assert len(out) == 0 and (info["matched"], info["written"], info["next_group"]) == (n, 0, 0)
    out, info = AM.audit(st, cap=3)
    assert out.tobytes() == whole[:3].tobytes() and info["next_group"] == int(whole["local"][2]) + 1
    out, info = AM.audit(st, first_group=info["next_group"])
    assert out.tobytes() == whole[3:].tobytes() and info["next_group"] == G and info["per_check"] != winfo["per_check"]
    out, info = AM.audit(st, first_group=G)
    assert len(out) == 0 and (info["matched"], info["next_group"]) == (0, G)


def test_hwm_above_last_shortens_the_window():
    st, want = raft_hand_state()
    assert records(AM.audit(st)[0]) == expected(want)
    # (read as a REF row, hwm = last, slots 1..4 would be replica 1's log: they differ from the others' 3 and
    # 4, and replica 1's terms would descend from 4 to 5)
    ref = dict(st, hwm=st["last"])
    assert records(AM.audit(ref)[0])[0] == (2 | 8, 0, 1, 3, 2)


def test_stamps():
    st, want = crc_hand_state()
    assert records(AM.audit(st, payload_crc=True)[0]) == expected(want)
    assert AM.audit(st, payload_crc=False)[1]["matched"] == 0
    # the vectorised CRC against the bitwise one of the harness
    t, v = np.array([0, 1, I, 7]), np.array([0, 1 << 62, 12345, -1], np.int64)
    assert AM.entry_crcs(t, v).tolist() == [H.entry_crc(int(a), int(b)) for a, b in zip(t, v)]


def test_single_replica():
    st = hand_state(R1_CASES, 1)
    assert records(AM.audit(st)[0]) == expected([w for _, w in R1_CASES.values()])


# layout -----------------------------------------------------------------------
def test_record_layouts_match_header(tmp_path):
    fields = [("raft_audit_hit", f) for f in abi.AUDIT_HIT.names] + \
             [("raft_audit_info", f) for f, _ in abi.AuditInfo._fields_]
    body = "".join(f'printf("%zu ", offsetof({s}, {f}));' for s, f in fields)
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%u ", '
                    'sizeof(raft_audit_hit), sizeof(raft_audit_info), RAFT_AUDIT_ALL);%s'
                    'printf("%%d %%d %%d %%d %%d %%d\\n", RAFT_AUDIT_TWO_LEADERS, RAFT_AUDIT_LOG_MATCHING, '
                    'RAFT_AUDIT_COMMIT_DIVERGED, RAFT_AUDIT_TERM_ORDER, RAFT_AUDIT_STAMP, RAFT_AUDIT_COMMIT_BEYOND_LOG);'
                    'return 0;}\n' % (HEADER, body))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [abi.AUDIT_HIT.itemsize, C.sizeof(abi.AuditInfo), abi.AUDIT_ALL]
    want += [abi.AUDIT_HIT.fields[f][1] for f in abi.AUDIT_HIT.names]
    want += [getattr(abi.AuditInfo, f).offset for f, _ in abi.AuditInfo._fields_]
    want += [abi.AUDIT_TWO_LEADERS, abi.AUDIT_LOG_MATCHING, abi.AUDIT_COMMIT_DIVERGED, abi.AUDIT_TERM_ORDER,
             abi.AUDIT_STAMP, abi.AUDIT_COMMIT_BEYOND_LOG]
    assert got == want and got[:2] == [24, 88]
    assert "raft_group_audit" in abi.SIGNATURES and "raft_group_audit" in abi.OPTIONAL
    assert [getattr(AM, n.upper()) for n in abi.AUDIT_NAMES] == [1, 2, 4, 8, 16, 32]


# the model over oracle traces -------------------------------------------------
# tests/test_gpu_groups.py's REF configuration (new-node churn) and its steady engines
REF = dict(replicas=3, groups=1101, ring_depth=64, entries_per_tick=1, client_period=1, seed=0x5EED0001,
           isolate_per_65536=8000, isolate_min_ticks=4, isolate_max_ticks=16, group_base=5000)
STEADY_A = dict(replicas=5, groups=1101, ring_depth=16, entries_per_tick=1, client_period=1, seed=0x5EED0002)
STEADY_B = dict(STEADY_A, replicas=3, entries_per_tick=4, payload_crc=1)


def _churn(kw, upto):
    with oracle.Oracle(**kw) as o:
        o.init_new_nodes(0)
        t = 0
        for u in upto:
            o.tick(t, u - t, threads=THREADS)
            t = u
            yield u, o.store_state()


@pytest.mark.parametrize("sem", [0, 1], ids=["ref", "raft"])
def test_churn_traces(sem):
    kw = dict(REF, semantics=sem)
    for t, st in _churn(kw, (30, 60, 120)):
        _, info = AM.audit(st, group_base=kw["group_base"])
        print("REF" if not sem else "RAFT", "churn, tick", t, ": violating groups", info["matched"], info["per_check"])
        if sem:   # test_raft_safety_under_churn's property, per group
            assert info["matched"] == 0, info


def test_raft_leader_isolation_trace():
    kw = dict(replicas=5, groups=512, ring_depth=16, client_period=1, semantics=1, seed=0x46, isolate_per_65536=30000,
              isolate_min_ticks=4, isolate_max_ticks=16, isolate_leader=1)
    for t, st in _churn(kw, (100, 200)):
        _, info = AM.audit(st)
        print("RAFT leader isolation, tick", t, ": violating groups", info["matched"], info["per_check"])
        assert info["matched"] == 0, info


@pytest.mark.parametrize("kw", [STEADY_A, STEADY_B], ids=["a", "b"])
def test_steady_traces_past_the_ring_wrap(kw):
    with oracle.Oracle(**kw) as o:
        o.init_steady(-1, 0)
        o.tick(1, 40, threads=THREADS)
        st = o.store_state()
    assert (st["last"] > kw["ring_depth"]).all()
    _, info = AM.audit(st, payload_crc=bool(kw.get("payload_crc")))
    print("steady, tick 40: violating groups", info["matched"], info["per_check"])
    assert info["matched"] == 0, info


# injection ----------------------------------------------------------------------
def test_random_rows_violate_densely_and_a_tenth_of_them_sparsely():
    G = 1101
    rows = H.random_state(np.random.default_rng(11), G, 3, K)
    _, info = AM.audit(rows)
    print("random_state rows: violating groups", info["matched"], "of", G, info["per_check"])
    assert info["matched"] > 0.9 * G and info["per_check"]["stamp"] == 0
    assert all(info["per_check"][k] > 0 for k in abi.AUDIT_NAMES if k != "stamp")
    kw = dict(REF, semantics=1, ring_depth=K)
    for _, st in _churn(kw, (60,)):
        pass
    assert AM.audit(st)[1]["matched"] == 0
    sick = np.nonzero(np.random.default_rng(12).random(G) < 0.10)[0]
    mixed = GM.splice(st, sick, {k: v[sick] for k, v in rows.items()})
    hits, info = AM.audit(mixed, group_base=kw["group_base"])
    print("a tenth replaced:", len(sick), "rows,", info["matched"], "hits")
    assert 0.05 * G <= info["matched"] <= 0.15 * G
    assert set(hits["local"].tolist()) <= set(sick.tolist())
