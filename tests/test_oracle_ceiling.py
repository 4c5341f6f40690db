"""CPU: the oracle's windowed log storage (oracle/raft_oracle.c, o_node.base)
and the traces of tests/test_gpu_ceiling.py, on the oracle alone.

A loaded log keeps only the entries its own ring-depth rule lets anyone read,
so a log near index 2^31 costs K entries. The shift-invariance test ties that
storage to the dense one which the KATs and golden files pin: a run from a
state lifted towards the ceiling must equal the lift of the dense run."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ceiling_cases as CC
import harness as H
from raftstep import abi

I = H.I32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _base_state(oracle_mod, kw, rng):
    """Election-free in-step groups grown from empty (dense), followers lagging
    0..K-1 entries behind their leader, every match >= 1."""
    K, R, G = kw["ring_depth"], kw["replicas"], kw["groups"]
    o = oracle_mod.Oracle(**kw)
    o.init_steady(-1, 0)
    t = 2 * K + 3
    o.tick(1, t)
    st = o.store_state()
    for g in range(G):
        lead = int(np.argmax(st["role"][g] == abi.LEADER))
        for r in range(R):
            # even groups stay inside the leader's ring after the client tick (lag <= K-1-E) and live on
            lag = int(rng.integers(0, K if g % 2 else K - kw["entries_per_tick"]))
            if r == lead or not lag:
                continue
            last = int(st["last"][g, r])
            for i in range(last - lag + 1, last + 1):          # drop the newest `lag` entries
                for k in ("log_term", "log_value", "log_crc"):
                    st[k][g, r, (i - 1) % K] = 0
            st["last"][g, r] = st["hwm"][g, r] = last - lag
            st["commit"][g, r] = min(int(st["commit"][g, r]), last - lag)
            st["match"][g, lead, r] = last - lag
            st["next"][g, lead, r] = last - lag + 1
    return st, t + 1


@pytest.mark.parametrize("mult", [True, False], ids=["dmultK", "dany"])
@pytest.mark.parametrize("crc", [0, 1])
@pytest.mark.parametrize("sem", [abi.SEM_REF, abi.SEM_RAFT])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("K", [8, 16])
@pytest.mark.parametrize("R", [3, 5])
def test_index_shift_invariance(oracle_mod, R, K, E, sem, crc, mult):
    G, N = 64, 20
    kw = dict(replicas=R, groups=G, ring_depth=K, entries_per_tick=E, client_period=1, semantics=sem,
              payload_crc=crc, seed=0x51F7 + R + K)
    rng = np.random.default_rng(R * 1000 + K * 10 + E)
    S, t = _base_state(oracle_mod, kw, rng)
    grown = int(S["last"].max()) + N * E
    d_index = (I - grown - 40) // K * K + (0 if mult else 5)      # no index reaches I
    d_term = I - 9
    assert grown + d_index < I and (d_index % K == 0) == mult
    dense, lifted = oracle_mod.Oracle(**kw), oracle_mod.Oracle(**kw)
    dense.load_state(S)
    lifted.load_state(H.lift_state(S, d_index, d_term, K))
    sd, sl = dense.tick(t, N), lifted.tick(t, N)
    assert list(sd) == list(sl)
    out = dense.store_state()
    # (a follower lagging more than K-1-E entries is out of the leader's ring after the client
    #  tick: RAFT_F_RING_EVICTED, on both sides alike)
    assert set(out["fault"]) <= {0, abi.F_RING_EVICTED} and (out["fault"] == 0).sum() >= G // 4
    assert int(sd[abi.STAT_NAMES.index("elections_won")]) == 0
    H.assert_same_state(lifted.store_state(), H.lift_state(out, d_index, d_term, K), "lifted run vs lift of the dense run")


@pytest.mark.parametrize("sem", [abi.SEM_REF, abi.SEM_RAFT])
def test_round_trip_near_the_ceiling(oracle_mod, sem):
    rng = np.random.default_rng(5 + sem)
    G, R, K = 128, 5, 8
    kw = dict(replicas=R, groups=G, ring_depth=K, semantics=sem, payload_crc=1)
    st = H.stamp_crcs(H.ceiling_state(rng, G, R, K, raft=sem == abi.SEM_RAFT))
    a, b = oracle_mod.Oracle(**kw), oracle_mod.Oracle(**kw)
    a.load_state(st)
    back = a.store_state()
    for k in ("role", "voted", "term", "last", "commit", "deadline", "timeout", "match", "fault", "log_term",
              "log_value", "log_crc"):
        assert np.array_equal(back[k], st[k]), k
    assert np.array_equal(back["hwm"], st["last"])
    b.load_state(back)
    H.assert_same_state(b.store_state(), back, "second load")
    da, db = a.state_digest(), b.state_digest()
    assert np.array_equal(da[0], db[0]) and da[1] == db[1]


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("sem", [abi.SEM_REF, abi.SEM_RAFT])
@pytest.mark.parametrize("name", sorted(CC.CONFIGS))
def test_gpu_traces_cover_the_ceiling(oracle_mod, name, sem, E):
    """What makes the traces of test_gpu_ceiling.py worth running, asserted on
    the oracle: a quarter of the groups end frozen by RAFT_F_OVERFLOW, a
    quarter end live; REF with E = 3 freezes leaders with room 0, 1 and 2; with
    isolation some group's fault is a timeout at term I."""
    kw = CC.config(name, sem, E)
    c = CC.coverage(oracle_mod.Oracle(**kw), CC.start_state(sem, kw.get("payload_crc", 0)), E)
    print(name, sem, E, c)
    assert c["overflow"] >= CC.G // 4 and c["live"] >= CC.G // 4
    if sem == abi.SEM_REF and E == 3:
        assert {0, 1, 2} <= c["rooms"]
    if name != "plain":
        assert c["by_timeout"] >= 1


def test_virtual_time_oracle_half(oracle_mod):
    """The oracle has no end of virtual time of its own; at the last ticks the
    engine accepts its deadlines still fit int32 (test_gpu_ceiling.py compares)."""
    FIRST = (2**31 - 1 - 30) // 2 - 30
    o = oracle_mod.Oracle(replicas=3, groups=300, client_period=1, seed=0x71CE)
    o.init_new_nodes(FIRST - 1)
    o.tick(FIRST, 30)
    s = o.store_state()
    assert (s["deadline"] > 0).all() and (s["role"] == abi.LEADER).any()
    assert (FIRST + 30) * 2 + 30 < 2**31 <= (FIRST + 31) * 2 + 30


def test_standalone_driver_under_sanitizers(tmp_path):
    """tests/ceiling_driver.c with raft_oracle.c, built with the host compiler
    and -fsanitize=address,undefined, run as a child process."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler found")
    exe = os.path.join(tmp_path, "ceiling_driver")
    subprocess.run([cc, "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "ceiling_driver.c"),
                    os.path.join(ROOT, "oracle", "raft_oracle.c"), "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ceiling driver: ok" in r.stdout
