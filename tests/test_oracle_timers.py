"""CPU: the oracle at the clock and timer configurations of
tests/timer_cases.py, on the oracle alone. The draws stay inside the
configured ranges and reach both ends; one election per case is derived by
hand from the draws and the firing rule; the regimes the cases are meant to
reach (no election while a leader is cut off, an election at every missed
heartbeat) exist; and the inputs of tests/test_gpu_timers.py leave at most a
quarter of the groups frozen, so that a pass there is not a pass on groups
that stopped moving."""
import numpy as np
import pytest

import timer_cases as TC
from raftstep import abi

F, C, L = abi.FOLLOWER, abi.CANDIDATE, abi.LEADER
STAT = {k: i for i, k in enumerate(abi.STAT_NAMES)}
NTICKS = 160


@pytest.mark.parametrize("name", sorted(TC.TIMINGS))
def test_timer_draw_ranges(oracle_mod, name):
    """min + rand % span over a few thousand (group, replica, tick): inside
    [min, min + span), both ends drawn; with span 1 every draw is min."""
    t = TC.TIMINGS[name]
    o = oracle_mod.Oracle(seed=7, **t)
    keys = [(g, r, k) for g in range(100) for r in range(5) for k in range(8)]
    for role, mn, span in ((F, t["follower_timeout_min"], t["follower_timeout_span"]),
                           (C, t["candidate_timeout_min"], t["candidate_timeout_span"])):
        d = {o.timer_draw(g, r, role, k) for g, r, k in keys}
        assert min(d) == mn and max(d) == mn + span - 1, (name, role, min(d), max(d))
        assert d <= set(range(mn, mn + span))
        if span <= 24:
            assert d == set(range(mn, mn + span))      # 4000 draws over at most 24 values: each one occurs
    if name == "unit":
        assert {o.timer_draw(g, r, F, k) for g, r, k in keys} == {3}
        assert {o.timer_draw(g, r, C, k) for g, r, k in keys} == {2}


@pytest.mark.parametrize("name", sorted(TC.TIMINGS))
def test_first_election_by_hand(oracle_mod, name):
    """One group of three new nodes, no client, no isolation (REF). Node r
    starts at tick 0 (now = 0) with timeout = deadline = its follower draw d_r.
    Nothing happens until the first tick T with T * tick_seconds >= min d,
    T = ceil(min d / tick_seconds). There the replica with the least (d, r)
    fires first: Term 1, a candidate timer drawn at tick T from now = T *
    tick_seconds. Its vote round runs at once: both others are followers of
    term 0 that have not voted, so they grant (Term 1, Voted, timer reset to
    now + their own timeout, which is past now: they do not fire) and the
    candidate becomes Leader with three votes."""
    t = TC.TIMINGS[name]
    secs = t["tick_seconds"]
    o = oracle_mod.Oracle(replicas=3, groups=1, client_period=0, seed=0x71AE, **t)
    o.init_new_nodes(0)
    d = [o.timer_draw(0, r, F, 0) for r in range(3)]
    first = min(range(3), key=lambda r: (d[r], r))
    T = -(-d[first] // secs)
    assert (T - 1) * secs < d[first] <= T * secs and T >= 1
    o.tick(0, T)                                   # ticks 0 .. T-1
    st = o.store_state()
    assert st["role"][0].tolist() == [F] * 3 and st["term"][0].tolist() == [0] * 3
    assert st["voted"][0].tolist() == [0] * 3 and st["fault"][0] == 0
    assert st["deadline"][0].tolist() == d and st["timeout"][0].tolist() == d
    stats = o.tick(T, 1)
    cd = o.timer_draw(0, first, C, T)
    assert t["candidate_timeout_min"] <= cd < t["candidate_timeout_min"] + t["candidate_timeout_span"]
    st = o.store_state()
    now = T * secs
    assert st["role"][0].tolist() == [L if r == first else F for r in range(3)]
    assert st["term"][0].tolist() == [1] * 3 and st["voted"][0].tolist() == [1] * 3
    assert st["timeout"][0].tolist() == [cd if r == first else d[r] for r in range(3)]
    assert st["deadline"][0].tolist() == [now + (cd if r == first else d[r]) for r in range(3)]
    assert st["fault"][0] == 0 and (st["last"] == 0).all() and (st["commit"] == 0).all()
    want = dict(term_bumps=1, elections_won=1, votes_granted=2, leader_groups=1)
    assert stats.tolist() == [want.get(k, 0) for k in abi.STAT_NAMES]


def _run(oracle_mod, kw, init, n=NTICKS):
    o = oracle_mod.Oracle(**kw)
    if init == "new":
        o.init_new_nodes(0)
        first = 0
    else:
        o.init_steady(*init)
        first = init[1] + 1
    return o, o.tick(first, n, threads=4)


@pytest.mark.parametrize("sem", [TC.REF, TC.RAFT])
def test_the_regimes_exist(oracle_mod, sem):
    """160 ticks from init_steady(-1, 0). Timers longer than a 5-tick window
    (`long`: at least 40 ticks; `top`: at least 511 s / 37 s = 13 ticks): a
    cut-off leader comes back before any follower's timer fires, so requests
    fail and no term moves. Timers of at most 3 ticks (`unit`) or below one
    tick (`sub_tick`): elections."""
    for name in ("long", "top"):
        _, s = _run(oracle_mod, TC.config(name, "leader", sem), (-1, 0))
        assert s[STAT["term_bumps"]] == 0 and s[STAT["ae_fail"]] > 0, (name, s.tolist())
    for name in ("unit", "sub_tick"):
        _, s = _run(oracle_mod, TC.config(name, "hashed", sem), (-1, 0))
        assert s[STAT["term_bumps"]] > 0, (name, s.tolist())


@pytest.mark.parametrize("init", ["new", "steady"])
@pytest.mark.parametrize("sem", [TC.REF, TC.RAFT])
@pytest.mark.parametrize("iso", sorted(TC.ISOLATIONS))
@pytest.mark.parametrize("name", sorted(TC.TIMINGS))
def test_at_most_a_quarter_frozen(oracle_mod, name, iso, sem, init):
    """The cap on frozen groups for every (case, isolation, semantics, init)
    the table offers; `top` stores timeouts up to 1023 (the 10-bit field's top
    bit set); and from new nodes every run elects at least one leader per
    group."""
    kw = TC.config(name, iso, sem)
    o, s = _run(oracle_mod, kw, "new" if init == "new" else (-1, 0))
    if init == "new":
        assert s[STAT["elections_won"]] >= kw["groups"], s.tolist()
    st = o.store_state(logs=False)
    frozen = int((st["fault"] != 0).sum())
    assert 4 * frozen <= kw["groups"], f"{frozen} of {kw['groups']} groups frozen"
    t = TC.TIMINGS[name]
    lo = min(t["follower_timeout_min"], t["candidate_timeout_min"])
    hi = max(t["follower_timeout_min"] + t["follower_timeout_span"],
             t["candidate_timeout_min"] + t["candidate_timeout_span"]) - 1
    assert lo <= st["timeout"].min() and st["timeout"].max() <= hi
    if name == "top":
        assert st["timeout"].max() == 1023 and (st["timeout"] >= 512).any()


@pytest.mark.parametrize("sem", [TC.REF, TC.RAFT])
@pytest.mark.parametrize("R", [3, 5])
def test_a_zero_timeout_fires_at_the_heartbeat(oracle_mod, R, sem):
    """The planted in-step groups of test_gpu_timers.py
    test_tick_from_timer_states, without isolation:
    the leader's heartbeat resets a follower's timer of 0 to now, and the
    timer step of the same tick fires it, in every such group. A follower with
    a timeout of 17 in the same groups stays a follower of term 3 unless a
    candidate's request reaches it."""
    n, K = 32, 16
    kw = dict(TC.TIMINGS["odd"], replicas=R, groups=64, ring_depth=K, client_period=2, seed=0x71D + R, semantics=sem)
    st = TC.plant_zero_timeout_followers(TC.timer_state(np.random.default_rng(3), 64, R, K, 3), sem, n)
    o = oracle_mod.Oracle(**kw)
    o.load_state(st)
    before = o.store_state()
    assert (before["term"][:n] == TC.PLANT_TERM).all() and (before["deadline"][:n] == 1 << 20).all()
    s = o.tick(30, 1)
    after = o.store_state()
    assert s[STAT["term_bumps"]] >= n
    assert ((after["term"][:n] > TC.PLANT_TERM).any(axis=1)).all()
    if sem == TC.REF:   # the candidate's request reaches the Leader, which has no case for it (main.go:308)
        assert (after["fault"][:n] != 0).all()
    # the same groups with every timeout 17: one heartbeat, nothing else
    st["timeout"][:n] = 17
    o.load_state(st)
    o.tick(30, 1)
    quiet = o.store_state()
    assert (quiet["term"][:n] == TC.PLANT_TERM).all() and (quiet["fault"][:n] == 0).all()
    fol = quiet["role"][:n] == F
    assert (quiet["deadline"][:n][fol] == 30 * 3 + 17).all()


def test_timer_state_covers_the_loadable_range():
    """timer_state draws every edge of the 10-bit field, and deadlines on both
    sides of the window it is ticked in."""
    st = TC.timer_state(np.random.default_rng(1), 192, 3, 8, 37)
    assert set(TC.TIMEOUT_EDGES) <= set(st["timeout"].ravel().tolist())
    assert st["timeout"].min() == 0 and st["timeout"].max() == 1023
    assert st["deadline"].min() < 0 and st["deadline"].max() > 60 * 37
    assert -2000 <= st["deadline"].min() and st["deadline"].max() <= 60 * 37 + 2000
