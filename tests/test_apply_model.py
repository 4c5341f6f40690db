"""CPU checks of the applied state: the model (tests/apply_model.py, the
expected records of tests/test_gpu_apply.py) against known answers and one
hand-derived case per rule of include/raftstep.h ("applied state"), the record
layouts of the header, the feed cross-check over oracle traces, the host-side
check of FROM_RECORDS under the sanitizers and the NULL-engine returns."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import apply_model as AM
import feed_model as FM
import harness as H
import oracle
from raftstep import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "raftstep.h")
R, K = 3, 4
M = (1 << 64) - 1


# the test's own few lines of integer arithmetic ------------------------------
def _sm(x):
    x = (x + 0x9E3779B97F4A7C15) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def _seed(gid, base):
    return _sm(_sm(gid) ^ base)


def _fold(ch, i, t, v):
    return _sm(_sm(ch ^ ((t << 32) | i)) ^ (v & M))


def _chain(gid, base, entries):
    """entries: (index, term, value) in order."""
    ch = _seed(gid, base)
    for i, t, v in entries:
        ch = _fold(ch, i, t, v)
    return ch


def test_sm_is_the_engines_splitmix64():
    """rng_vectors.json pins rng = sm(sm(sm(seed ^ sm(gid)) ^ (stream << 32 | replica)) ^ tick)."""
    for v in json.load(open(os.path.join(ROOT, "tests", "golden", "rng_vectors.json"))):
        for f in (_sm, AM.sm):
            k = f(v["seed"] ^ f(v["gid"]))
            assert f(f(k ^ ((v["stream"] << 32) | v["replica"])) ^ v["tick"]) == v["rng"]


def _one(logs, commits, group_base=0):
    """One group of R replicas: follower logs as lists of (term, value)."""
    nodes = [H.node(H.F, 1, 1, lg, commit=cm) for lg, cm in zip(logs, commits)]
    return H.build_state([nodes], R, K)


def _rec(x):
    return tuple(int(x[k]) for k in ("applied", "base", "chain", "sum", "div_index", "gaps", "div_peer", "reserved"))


def test_chain_known_answers():
    """A three-entry log with a negative value and a term above 2^31-1's half:
    seed, each fold and the wrapping sum, at group_base 7."""
    log = [(1, 100), (2, -5), (0x7FFFFFFF, (1 << 62) + 3)]
    st = _one([log, log[:2], []], [3, 2, 0])
    rec = AM.start_records(st, None, "start", group_base=7)
    assert _rec(rec[0, 0]) == (0, 0, _seed(7, 0), 0, 0, 0, 0xFF, 0)
    info, rec = AM.step(st, rec, group_base=7)
    c1 = _fold(_seed(7, 0), 1, 1, 100)
    c2 = _fold(c1, 2, 2, -5)
    c3 = _fold(c2, 3, 0x7FFFFFFF, (1 << 62) + 3)
    assert c2 == _sm(_sm(c1 ^ ((2 << 32) | 2)) ^ ((-5) & M))
    assert _rec(rec[0, 0]) == (3, 0, c3, 100 - 5 + (1 << 62) + 3, 0, 0, 0xFF, 0)
    assert _rec(rec[0, 1]) == (2, 0, c2, 95, 0, 0, 0xFF, 0)
    assert _rec(rec[0, 2]) == (0, 0, _seed(7, 0), 0, 0, 0, 0xFF, 0)
    assert info == dict(folded=5, lost=0, stalled=0, gapped=0, diverged=0)
    assert AM.seed(7, 0) == _seed(7, 0) and AM.fold(c1, 2, 2, -5) == c2


def test_sum_wraps():
    log = [(1, (1 << 63) - 1), (1, (1 << 63) - 1)]
    st = _one([log, [], []], [2, 0, 0])
    _, rec = AM.step(st, AM.start_records(st, [0], "start"))
    assert int(rec[0, 0]["sum"]) == -2 and int(rec[0, 1]["applied"]) == -1


def test_commit_start_and_mask():
    log = [(1, 10), (1, 11), (1, 12)]
    st = _one([log, log[:2], log], [3, 3, 1])
    rec = AM.start_records(st, [0, 2], "commit", group_base=5)
    assert _rec(rec[0, 0]) == (3, 3, _seed(5, 3), 0, 0, 0, 0xFF, 0)
    assert _rec(rec[0, 1]) == (-1, 0, 0, 0, 0, 0, 0, 0)          # outside the mask: all zero, applied -1
    assert _rec(rec[0, 2]) == (1, 1, _seed(5, 1), 0, 0, 0, 0xFF, 0)
    info, out = AM.step(st, rec, group_base=5)
    assert info == dict(folded=0, lost=0, stalled=0, gapped=0, diverged=0) and out.tobytes() == rec.tobytes()


def test_stall_leaves_the_record_alone():
    log = [(1, 10), (1, 11)]
    st = _one([log, log, log], [2, 2, 2])
    rec = AM.start_records(st, None, "start")
    rec[0, 1]["applied"], rec[0, 1]["base"], rec[0, 1]["chain"], rec[0, 1]["sum"] = 5, 5, 77, 9
    info, out = AM.step(st, rec)
    assert info == dict(folded=4, lost=0, stalled=1, gapped=0, diverged=0)
    assert out[0, 1].tobytes() == rec[0, 1].tobytes()


def test_gap_reseeds():
    """Replica 0's log (7 entries) has outgrown the ring of 4 and it has applied
    1: entries 2, 3 are lost, the chain starts again at 3, entries 4..6 fold."""
    log = [(1, 200 + i) for i in range(7)]
    st = _one([log, log[:1], []], [6, 1, 0])
    rec = AM.start_records(st, None, "start", group_base=2)
    rec[0, 0]["applied"], rec[0, 0]["chain"], rec[0, 0]["sum"] = 1, _chain(2, 0, [(1, 1, 200)]), 200
    info, out = AM.step(st, rec, group_base=2)
    assert info == dict(folded=4, lost=2, stalled=0, gapped=1, diverged=0)
    want = _chain(2, 3, [(4, 1, 203), (5, 1, 204), (6, 1, 205)])
    assert _rec(out[0, 0]) == (6, 3, want, 203 + 204 + 205, 0, 1, 0xFF, 0)
    # replica 1 (base 0) and replica 0 (base 3) are not comparable: no divergence although the chains differ
    assert int(out[0, 1]["div_index"]) == 0


def test_ref_follower_commit_one_past_its_log():
    log = [(1, 10), (1, 11), (1, 12)]
    st = _one([log, log[:2], log], [3, 3, 3])
    info, out = AM.step(st, AM.start_records(st, None, "start"))
    assert [int(x) for x in out[0]["applied"]] == [3, 2, 3] and info["stalled"] == 0 and info["folded"] == 8
    st = _one([log, log, log], [3, 3, 3])
    info, out = AM.step(st, out)
    assert info == dict(folded=1, lost=0, stalled=0, gapped=0, diverged=0)
    assert len({int(x) for x in out[0]["chain"]}) == 1


A, B, Cc, X, Y = (1, 1), (1, 2), (1, 3), (1, 99), (2, 3)


def _diverged_state():
    """r0 = [A B C], r1 = [A X C] (a value differs at 2), r2 = [A B Y] (a term differs at 3)."""
    return _one([[A, B, Cc], [A, X, Cc], [A, B, Y]], [3, 3, 3])


def test_divergence_smallest_index_and_lowest_peer():
    st = _diverged_state()
    info, out = AM.step(st, AM.start_records(st, None, "start"))
    # r0 differs from r1 at 2 and from r2 at 3: (2, r1). r1 from r0 and r2 at 2: (2, r0). r2 from r0 at 3, r1 at 2: (2, r1)
    assert [(int(x["div_index"]), int(x["div_peer"])) for x in out[0]] == [(2, 1), (2, 0), (2, 1)]
    assert info == dict(folded=9, lost=0, stalled=0, gapped=0, diverged=1)
    # the same with replica 1 unfed: r0 and r2 meet their first difference at 3
    info, out = AM.step(st, AM.start_records(st, [0, 2], "start"))
    assert [(int(x["div_index"]), int(x["div_peer"])) for x in out[0]] == [(3, 2), (0, 0), (3, 0)]
    assert info["diverged"] == 1


def test_divergence_is_sticky():
    st = _diverged_state()
    _, rec = AM.step(st, AM.start_records(st, None, "start"))
    st2 = _one([[A, B, Cc, (3, 1)], [A, X, Cc, (3, 2)], [A, B, Y, (3, 3)]], [4, 4, 4])
    info, out = AM.step(st2, rec)
    assert info == dict(folded=3, lost=0, stalled=0, gapped=0, diverged=0)
    assert [(int(x["div_index"]), int(x["div_peer"])) for x in out[0]] == [(2, 1), (2, 0), (2, 1)]


def test_divergence_met_at_the_start_of_a_trajectory():
    """r1 has applied 3 and stalls at nothing new; r0 arrives at 3 in this step:
    their trajectories share index 3 only, and that is where they differ."""
    st = _one([[A, B, Cc], [A, X, Cc], []], [3, 3, 0])
    rec = AM.start_records(st, [0, 1], "start")
    rec[0, 1]["applied"] = 3
    rec[0, 1]["chain"] = _chain(0, 0, [(1, 1, 1), (2, 1, 99), (3, 1, 3)])
    info, out = AM.step(st, rec)
    assert [(int(x["div_index"]), int(x["div_peer"])) for x in out[0][:2]] == [(3, 1), (3, 0)]
    assert info == dict(folded=3, lost=0, stalled=0, gapped=0, diverged=1)


def test_different_bases_are_never_compared():
    st = _diverged_state()
    rec = AM.start_records(st, None, "start")
    rec[0, 1]["applied"] = rec[0, 1]["base"] = 1
    rec[0, 1]["chain"] = _seed(0, 1)
    info, out = AM.step(st, rec)
    assert [(int(x["div_index"]), int(x["div_peer"])) for x in out[0]] == [(3, 2), (0, 0xFF), (3, 0)]
    assert info["diverged"] == 1 and info["folded"] == 8


def test_gaps_saturate():
    log = [(1, 200 + i) for i in range(7)]
    st = _one([log, log, log], [7, 7, 7])
    rec = AM.start_records(st, None, "start")
    rec["gaps"][0] = [65534, 65535, 0]
    info, out = AM.step(st, rec)
    assert [int(x) for x in out[0]["gaps"]] == [65535, 65535, 1] and info["gapped"] == 3 and info["lost"] == 9


def test_from_records_validation():
    st = _diverged_state()
    rec = AM.start_records(st, None, "commit")
    assert AM.records_valid(rec)
    for field, value in (("base", -1), ("base", 4), ("reserved", 1)):
        bad = rec.copy()
        bad[0, 1][field] = value
        assert not AM.records_valid(bad)
        assert AM.records_valid(bad, [0, 2])            # (read for the masked replicas only)


def test_scan_witnesses_and_paging():
    G = 6
    rec = np.zeros((G, R), abi.APPLY_RECORD)
    rec["div_peer"] = 0xFF
    rec["applied"][:, 1] = -1                            # replica 1 is not fed
    rec[1, 2]["div_index"], rec[1, 2]["div_peer"] = 9, 0
    rec[1, 0]["gaps"] = 2
    rec[3, 2]["gaps"], rec[3, 2]["base"] = 5, 40
    rec[3, 0]["gaps"] = 0
    rec[4, 1]["div_index"] = 3                           # unfed: no hit
    rec[5, 0]["div_index"], rec[5, 0]["div_peer"] = 7, 2
    rec[5, 2]["div_index"], rec[5, 2]["div_peer"] = 7, 0
    fault = np.array([0, 2, 0, 0, 0, 1], np.uint8)

    def rows(h):
        return [tuple(int(x[k]) for k in ("group", "local", "a", "b", "flags", "fault", "index", "gaps")) for x in h]

    h, info = AM.scan(rec, fault, abi.APPLY_DIVERGED, group_base=100)
    assert rows(h) == [(101, 1, 2, 0, 3, 2, 9, 2), (105, 5, 0, 2, 1, 1, 7, 0)]
    assert info == dict(matched=2, written=2, next_group=G)
    h, info = AM.scan(rec, fault, abi.APPLY_GAPPED)
    assert rows(h) == [(1, 1, 2, 0, 3, 2, 9, 2), (3, 3, 2, 0xFF, 2, 0, 40, 5)]
    h, info = AM.scan(rec, fault, abi.APPLY_GAPPED | abi.APPLY_DIVERGED, cap=2)
    assert [int(x) for x in h["local"]] == [1, 3] and info == dict(matched=3, written=2, next_group=4)
    h, info = AM.scan(rec, fault, 3, first_group=4, cap=5)
    assert [int(x) for x in h["local"]] == [5] and info == dict(matched=1, written=1, next_group=G)
    h, info = AM.scan(rec, fault, 3, first_group=2, cap=0)
    assert len(h) == 0 and info == dict(matched=2, written=0, next_group=2)


def test_reset_records():
    st = _diverged_state()
    st = {k: np.concatenate([v, v]) for k, v in st.items()}
    rec = AM.start_records(st, [0, 2], "start")
    _, rec = AM.step(st, rec)
    out = AM.reset_records(rec, st, [1], "commit", group_base=0)
    assert out[0].tobytes() == rec[0].tobytes()
    assert _rec(out[1, 0]) == (3, 3, _seed(1, 3), 0, 0, 0, 0xFF, 0) and int(out[1, 1]["applied"]) == -1
    out = AM.reset_records(rec, st, [0], "start")
    assert _rec(out[0, 2]) == (0, 0, _seed(0, 0), 0, 0, 0, 0xFF, 0) and out[1].tobytes() == rec[1].tobytes()


# layouts -------------------------------------------------------------------
def test_record_layouts_match_header_and_numpy(tmp_path):
    fields = {
        "raft_apply_record": (abi.APPLY_RECORD, ("applied", "base", "chain", "sum", "div_index", "gaps", "div_peer",
                                                 "reserved")),
        "raft_apply_hit": (abi.APPLY_HIT, ("group", "local", "a", "b", "flags", "fault", "index", "gaps")),
    }
    body = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void){"]
    for name, (_, names) in fields.items():
        body.append('printf("%%zu ", sizeof(%s));' % name)
        body += ['printf("%%zu ", offsetof(%s, %s));' % (name, f) for f in names]
    body.append('printf("%zu %zu %zu %d %d %d %d %d\\n", sizeof(raft_apply_info), offsetof(raft_apply_info, diverged), '
                'offsetof(raft_apply_info, reserved), (int)RAFT_APPLY_FROM_START, (int)RAFT_APPLY_FROM_COMMIT, '
                '(int)RAFT_APPLY_FROM_RECORDS, (int)RAFT_APPLY_DIVERGED, (int)RAFT_APPLY_GAPPED);return 0;}')
    prog = tmp_path / "sz.c"
    prog.write_text("\n".join(body) + "\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = []
    for dt, names in fields.values():
        want.append(dt.itemsize)
        want += [dt.fields[f][1] for f in names]
    want += [C.sizeof(abi.ApplyInfo), abi.ApplyInfo.diverged.offset, abi.ApplyInfo.reserved.offset,
             abi.APPLY_FROM_START, abi.APPLY_FROM_COMMIT, abi.APPLY_FROM_RECORDS, abi.APPLY_DIVERGED, abi.APPLY_GAPPED]
    assert got == want
    assert (abi.APPLY_RECORD.itemsize, abi.APPLY_HIT.itemsize, C.sizeof(abi.ApplyInfo)) == (32, 24, 64)
    names = {"raft_apply_open", "raft_apply_step", "raft_apply_read", "raft_apply_scan", "raft_apply_close"}
    assert names <= set(abi.SIGNATURES) and names <= set(abi.OPTIONAL)


def test_apply_calls_refuse_a_null_engine():
    lib = engine.load_library()
    info, sinfo = abi.ApplyInfo(), abi.ScanInfo()
    buf = np.zeros(4, abi.APPLY_RECORD)
    assert lib.raft_apply_open(None, 1, abi.APPLY_FROM_START, None) == abi.RAFT_EINVAL
    assert lib.raft_apply_step(None, C.byref(info)) == abi.RAFT_EINVAL
    assert lib.raft_apply_read(None, None, 1, buf.ctypes.data) == abi.RAFT_EINVAL
    assert lib.raft_apply_scan(None, 1, 0, None, 0, C.byref(sinfo)) == abi.RAFT_EINVAL
    assert lib.raft_apply_close(None) == abi.RAFT_EINVAL
    assert b"null" in lib.raft_last_error()


def test_records_driver_under_sanitizers(tmp_path):
    """tests/apply_records_driver.cpp over raft-sample_amd/csrc/apply_records.hpp, built with
    the host compiler and -fsanitize=address,undefined, run as a child process."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = os.path.join(tmp_path, "apply_records_driver")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "apply_records_driver.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "apply records driver: ok" in r.stdout


# feed cross-check over oracle traces ----------------------------------------
CHURN_A = dict(replicas=7, groups=1024, ring_depth=64, seed=0x45, semantics=1, client_period=1, isolate_leader=1,
               isolate_per_65536=20000, isolate_min_ticks=4, isolate_max_ticks=32)
CHURN_B = dict(replicas=5, groups=1024, ring_depth=16, seed=0x46, semantics=1, client_period=1, isolate_leader=1,
               isolate_per_65536=30000, isolate_min_ticks=4, isolate_max_ticks=16)
CRC = dict(replicas=5, groups=512, entries_per_tick=16, ring_depth=64, payload_crc=1, corrupt_per_65536=3000,
           client_period=1, seed=0x5EED0005)
# (config, init, first tick, ticks, a look every, the model's folded, lost, gapped pairs); the first row's 994,808
# and 12 are the feed test's own figures (tests/test_gpu_feed.py CHURN["B"])
TRACES = {
    "churn_b": (CHURN_B, ("init_new_nodes", 0), 0, 300, 3, 994808, 12, 4),
    "churn_b_ref": (dict(CHURN_B, semantics=0), ("init_new_nodes", 0), 0, 300, 3, 441848, 21, 3),
    "crc": (CRC, ("init_steady", -1, 0), 1, 20, 2, 783088, 752, 47),
    # (29 whole looks of 7 ticks, the first at tick 6: 203 ticks; 624,118 is that schedule's figure, 200 ticks with
    # a short last look give 620,947)
    "churn_a_ref": (dict(CHURN_A, semantics=0), ("init_new_nodes", 0), 0, 203, 7, 624118, 0, 0),
}


def run_trace(name, look=None):
    """The oracle over trace `name`, looked at on the feed test's schedule by the
    feed model (cap=None) and the apply model alike; look(o, st, info, rec) after each."""
    kw, init, t, nticks, every, *_ = TRACES[name]
    o = oracle.Oracle(**kw)
    getattr(o, init[0])(*init[1:])
    st = o.store_state()
    cur = FM.start_cursors(st, None, "start")
    rec = AM.start_records(st, None, "start")
    feed = dict(delivered=0, lost=0, stalled=0)
    tot = dict(folded=0, lost=0, stalled=0, gapped=0, diverged=0)
    end = t + nticks
    while t < end:
        k = min(every, end - t)
        o.tick(t, k, threads=16)
        t += k
        st = o.store_state()
        _, fi, cur = FM.poll(st, cur, None)
        info, rec = AM.step(st, rec)
        for key in feed:
            feed[key] += fi[key]
        for key in tot:
            tot[key] += info[key]
        if look:
            look(o, st, info, rec)
    assert np.array_equal(rec["applied"], cur)
    return feed, tot, rec


@pytest.mark.parametrize("name", list(TRACES))
def test_feed_cross_check_over_oracle_traces(name):
    """With the same schedule of looks, folded, lost and stalled equal the sums
    of the feed model's delivered, lost and stalled: both derive (lo, hi] alike.
    No trace stalls or diverges (committed prefixes agree)."""
    feed, tot, rec = run_trace(name)
    print(name, tot)
    assert (tot["folded"], tot["lost"], tot["stalled"]) == (feed["delivered"], feed["lost"], feed["stalled"])
    assert (tot["folded"], tot["lost"], tot["gapped"]) == TRACES[name][5:]
    assert tot["stalled"] == 0 and tot["diverged"] == 0 and not rec["div_index"].any()
    assert int((rec["gaps"] != 0).sum()) <= tot["gapped"]
