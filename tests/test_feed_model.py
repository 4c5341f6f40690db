"""CPU checks of the commit feed: the numpy model (tests/feed_model.py, the
expected feed of tests/test_gpu_feed.py) against cases derived by hand, the
record sizes of the header, and the NULL-engine returns of raft_feed_*."""
import ctypes as C
import os
import subprocess

import numpy as np

import feed_model as FM
import harness as H
from raftstep import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raftstep.h")
R, K = 3, 4


def _log(n, base):
    return [(1, base + i) for i in range(n)]


def _state():
    """Group 0: replica 1 is a follower with CommitIndex = LastApplied + 1
    (main.go:152). Group 1: replica 0's log (7 entries) has outgrown the ring
    of 4, replica 2 has 2 entries."""
    g0 = [H.node(H.L, 1, 1, _log(3, 100), commit=3, match=[0, 2, 3]),
          H.node(H.F, 1, 1, _log(2, 100), commit=3),
          H.node(H.F, 1, 1, _log(3, 100), commit=2)]
    g1 = [H.node(H.L, 1, 1, _log(7, 200), commit=6, match=[0, 7, 2]),
          H.node(H.F, 1, 1, _log(7, 200), commit=7),
          H.node(H.F, 1, 1, _log(2, 200), commit=2)]
    st = H.build_state([g0, g1], R, K)
    st["hwm"][:] = st["last"]
    return st


def _rec(e):
    return [(int(x["group"]), int(x["replica"]), int(x["index"]), int(x["term"]), int(x["value"])) for x in e]


CURSORS = np.array([[0, 0, 0], [1, 5, 4]], np.int32)
# group 0: replica 1 delivers up to its LastApplied 2 although it has committed 3.
# group 1: replica 0's cursor 1 is behind hwm - K = 3: entries 2, 3 are lost, 4..6 delivered;
#          replica 2's cursor 4 is ahead of min(commit, last) = 2: stalled, untouched.
WANT = [(0, 0, 1, 1, 100), (0, 0, 2, 1, 101), (0, 0, 3, 1, 102),
        (0, 1, 1, 1, 100), (0, 1, 2, 1, 101),
        (0, 2, 1, 1, 100), (0, 2, 2, 1, 101),
        (1, 0, 4, 1, 203), (1, 0, 5, 1, 204), (1, 0, 6, 1, 205),
        (1, 1, 6, 1, 205), (1, 1, 7, 1, 206)]


def test_model_follower_commit_past_last_lost_and_stalled():
    e, info, cur = FM.poll(_state(), CURSORS)
    assert _rec(e) == WANT
    assert info == dict(delivered=12, pending=0, lost=2, stalled=1)
    assert cur.tolist() == [[3, 2, 2], [6, 7, 4]]
    assert FM.disagreements(e) == 0
    # the entry replica 1 of group 0 had committed arrives once it exists
    st = _state()
    st["last"][0, 1] = st["hwm"][0, 1] = 3
    st["log_term"][0, 1, 2], st["log_value"][0, 1, 2] = 1, 102
    e, info, cur2 = FM.poll(st, cur)
    assert _rec(e) == [(0, 1, 3, 1, 102)] and info == dict(delivered=1, pending=0, lost=0, stalled=1)
    assert cur2.tolist() == [[3, 3, 2], [6, 7, 4]]


def test_model_cap_cuts_a_pair_and_cap_zero_only_skips_lost():
    st = _state()
    e, info, cur = FM.poll(st, CURSORS, cap=4)
    assert _rec(e) == WANT[:4]
    assert info == dict(delivered=4, pending=8, lost=2, stalled=1)
    assert cur.tolist() == [[3, 1, 0], [3, 5, 4]]           # (the lost entries are skipped whatever the cap)
    e2, info2, cur2 = FM.poll(st, cur, cap=100, group_base=10)
    assert _rec(e2) == [(g + 10, r, i, t, v) for g, r, i, t, v in WANT[4:]]
    assert info2 == dict(delivered=8, pending=0, lost=0, stalled=1)
    assert cur2.tolist() == [[3, 2, 2], [6, 7, 4]]
    e0, info0, cur0 = FM.poll(st, CURSORS, cap=0)
    assert len(e0) == 0 and info0 == dict(delivered=0, pending=12, lost=2, stalled=1)
    assert cur0.tolist() == [[0, 0, 0], [3, 5, 4]]


def test_model_mask_and_start_modes():
    st = _state()
    c = FM.start_cursors(st, [1], "start")
    assert c.tolist() == [[-1, 0, -1], [-1, 0, -1]]
    e, info, cur = FM.poll(st, c)
    assert set(e["replica"].tolist()) == {1} and info["delivered"] == 2 + 4 and info["lost"] == 3
    assert cur.tolist() == [[-1, 2, -1], [-1, 7, -1]]
    c = FM.start_cursors(st, None, "commit")
    assert c.tolist() == [[3, 2, 2], [6, 7, 2]]
    assert FM.poll(st, c)[1] == dict(delivered=0, pending=0, lost=0, stalled=0)
    assert FM.mask_of(0b101, 3).tolist() == [True, False, True]


def test_feed_record_sizes_match_header_and_numpy(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include "%s"\nint main(void){printf("%%zu %%zu\\n", '
                    'sizeof(raft_feed_entry), sizeof(raft_feed_info));return 0;}\n' % HEADER)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(prog), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert sizes == [32, 32]
    assert sizes == [abi.FEED_ENTRY.itemsize, C.sizeof(abi.FeedInfo)]


def test_feed_calls_refuse_a_null_engine():
    lib = engine.load_library()
    info = abi.FeedInfo()
    buf = (C.c_int32 * 4)()
    assert lib.raft_feed_open(None, 1, abi.FEED_FROM_START, None) == abi.RAFT_EINVAL
    assert lib.raft_feed_poll(None, None, 0, C.byref(info)) == abi.RAFT_EINVAL
    assert lib.raft_feed_cursors(None, buf) == abi.RAFT_EINVAL
    assert lib.raft_feed_close(None) == abi.RAFT_EINVAL
    assert b"null" in lib.raft_last_error()
