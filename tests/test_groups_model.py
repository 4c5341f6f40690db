"""CPU: the group directory's numpy model (tests/groups_model.py) on
hand-derived cases, the restart recipe on the oracle, and the oracle property
the GPU tests (tests/test_gpu_groups.py) rely on. Anchors: NewNode
(main.go:59-76), FollowerRun entry (main.go:113-115), the fault codes of
include/raftstep.h (main.go:242, 308-332)."""
import numpy as np
import pytest

import groups_model as GM
import harness as H
import oracle
from raftstep import abi

THREADS = 16
F, C, L = H.F, H.C, H.L

# REF new-node churn: 102 of the 1101 groups are frozen at tick 60 (29 with code 2, 73 with code 3)
REF = dict(replicas=3, groups=1101, ring_depth=64, entries_per_tick=1, client_period=1, seed=0x5EED0001,
           isolate_per_65536=8000, isolate_min_ticks=4, isolate_max_ticks=16, group_base=5000)


def _hand_state():
    """Seven groups of three replicas:
    0 healthy with a leader          1 faulted (code 3) with a leader (replica 2)
    2 faulted (code 2), no leader    3 healthy, no leader
    4 two leaders (replicas 1, 2)    5 healthy, no leader (all candidates)
    6 faulted (code 1) with leader 0"""
    roles = [[L, F, F], [F, F, L], [C, F, F], [F, F, F], [F, L, L], [C, C, C], [L, F, F]]
    st = H.build_state([[H.node(role=r, term=1) for r in g] for g in roles], 3, 8, faults=[0, 3, 2, 0, 0, 0, 1])
    return st


def _hits(out):
    return [(int(x["group"]), int(x["local"]), int(x["fault"]), int(x["leader"]), int(x["reserved"])) for x in out]


def test_scan_hand_cases():
    st = _hand_state()
    out, info = GM.scan(st, GM.FAULTED, group_base=100)
    # the faulted group with a Leader reports it; the one without reports 0xFF
    assert _hits(out) == [(101, 1, 3, 2, 0), (102, 2, 2, 0xFF, 0), (106, 6, 1, 0, 0)]
    assert info == dict(matched=3, written=3, next_group=7)
    out, info = GM.scan(st, GM.LEADERLESS)
    # group 2 has no Leader but is frozen: not a LEADERLESS hit
    assert _hits(out) == [(3, 3, 0, 0xFF, 0), (5, 5, 0, 0xFF, 0)]
    out, info = GM.scan(st, GM.FAULTED | GM.LEADERLESS)
    assert [h[1] for h in _hits(out)] == [1, 2, 3, 5, 6] and info["matched"] == 5
    # two leaders: the lower id (group 4 is no hit of either kind; read through leaders())
    assert GM.leaders(st).tolist() == [0, 2, 0xFF, 0xFF, 1, 0xFF, 0]


def test_scan_cap_and_paging():
    st = _hand_state()
    both = GM.FAULTED | GM.LEADERLESS
    whole, _ = GM.scan(st, both)
    out, info = GM.scan(st, both, cap=0)
    assert len(out) == 0 and info == dict(matched=5, written=0, next_group=0)
    out, info = GM.scan(st, both, cap=3)               # a cut in the middle
    assert [h[1] for h in _hits(out)] == [1, 2, 3] and info == dict(matched=5, written=3, next_group=4)
    out, info = GM.scan(st, both, cap=5)
    assert info == dict(matched=5, written=5, next_group=7)
    out, info = GM.scan(st, both, first_group=2, cap=9)
    assert [h[1] for h in _hits(out)] == [2, 3, 5, 6] and info == dict(matched=4, written=4, next_group=7)
    pages, first = [], 0                                # paging reassembles the list
    while first < 7:
        out, info = GM.scan(st, both, first_group=first, cap=2)
        pages.append(out)
        first = info["next_group"]
    assert np.concatenate(pages).tobytes() == whole.tobytes() and len(pages) == 3
    out, info = GM.scan(st, both, first_group=7)        # first_group = G: an empty scan
    assert len(out) == 0 and info == dict(matched=0, written=0, next_group=7)


def test_restart_cursor_rule():
    cur = np.array([[3, -1, 5], [2, -1, 2], [7, -1, 0]], np.int32)
    assert GM.restart_cursors(cur, [2, 0]).tolist() == [[0, -1, 0], [2, -1, 2], [0, -1, 0]]


@pytest.fixture(scope="module")
def ref_at_60():
    o = oracle.Oracle(**REF)
    o.init_new_nodes(0)
    o.tick(0, 60, threads=THREADS)
    return o, o.store_state()


def test_restart_recipe_on_the_oracle(ref_at_60):
    """Restart every frozen group at tick 60 and run 40 more ticks: every
    restarted group elects a Leader again (some freeze again later)."""
    _, st = ref_at_60
    G = REF["groups"]
    hits, info = GM.scan(st, GM.FAULTED, group_base=REF["group_base"])
    codes = np.bincount(hits["fault"], minlength=6)
    print("frozen at tick 60:", info["matched"], "of", G, "codes", codes.tolist())
    assert info["matched"] >= 0.05 * G
    assert codes[abi.F_DEADLOCK_VRES] > 0 and codes[abi.F_DEADLOCK_LEADER_VREQ] > 0
    ids = hits["local"]
    rows = GM.restart_rows(abi.default_config(**REF), ids, 60)
    assert not rows["fault"].any() and not rows["term"].any() and not rows["last"].any()
    assert (rows["role"] == F).all() and (rows["deadline"] == 120 + rows["timeout"]).all()
    new = GM.splice(st, ids, rows)
    others = np.setdiff1d(np.arange(G), ids)
    for k in st:
        assert np.array_equal(new[k][others], st[k][others]), k
    o = oracle.Oracle(**REF)
    o.load_state(new)
    o.tick(60, 40, threads=THREADS)
    end = o.store_state(logs=False)
    led = (end["role"][ids] == L).any(axis=1)
    again = int((end["fault"][ids] != 0).sum())
    print("restarted groups with a Leader after 40 ticks:", int(led.sum()), "of", len(ids), "; frozen again:", again)
    assert led.all()


@pytest.mark.parametrize("sem", [0, 1])
def test_stored_and_loaded_state_runs_like_the_uninterrupted_twin(sem):
    """What the GPU restart tests rely on: the canonical view is the whole
    state, so store + load into a fresh oracle changes nothing that follows."""
    kw = dict(REF, semantics=sem)
    a, b = oracle.Oracle(**kw), oracle.Oracle(**kw)
    a.init_new_nodes(0)
    a.tick(0, 60, threads=THREADS)
    b.load_state(a.store_state())
    assert np.array_equal(a.state_digest()[0], b.state_digest()[0])
    for t, k in ((60, 13), (73, 27)):
        sa, sb = a.tick(t, k, threads=THREADS), b.tick(t, k, threads=THREADS)
        assert list(sa) == list(sb)
        assert np.array_equal(a.state_digest()[0], b.state_digest()[0]), f"after tick {t + k - 1}"
