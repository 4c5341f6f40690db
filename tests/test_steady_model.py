"""CPU: the schedule generator and host-side model of tests/steady_model.py,
and the conditions that keep tests/test_gpu_steady_schedule.py from passing
vacuously: for its committed configs and seeds, by the model alone, the steady
form is predicted for at least half of all ticks of each schedule; over a
config's schedules every operation kind that keeps the continuity records
occurs directly between two steady-form calls, and every kind that destroys
them occurs and is later followed by an init_steady after which the steady
form is predicted again. Each schedule also runs through the oracle alone: no
operation in it fails."""
import numpy as np
import pytest

import harness as H
import oracle
import steady_model as M


@pytest.mark.parametrize("name", sorted(M.CONFIGS))
def test_schedules_are_deterministic_and_well_formed(name):
    cfg, env, seeds = M.CONFIGS[name]
    assert len(seeds) == 6 and len(set(seeds)) == 6
    for seed in seeds:
        a, b = M.schedule(seed, M.N_OPS, cfg), M.schedule(seed, M.N_OPS, cfg)
        assert a == b and len(a) == M.N_OPS
        assert a != M.schedule(seed + 1, M.N_OPS, cfg)
        assert a[0][0] == "init_steady" and all(op[0] in M.OPS for op in a)
        for i, op in enumerate(a):
            if op[0] == "init_steady":   # every init_steady is followed by the proving call
                assert a[i + 1] == M.PROVING, (seed, i)
                assert op[1] in (0, -1, cfg["replicas"] + 1) and op[2] in M.TICK0S


def test_model_follows_the_contract():
    cfg = dict(M.BASE)
    m = M.Model(cfg)
    assert m.tick(0, 5) == (5, False, False, False)            # nothing proven
    m.init_steady(-1, 4)
    assert m.tick(5, 6, True) == (6, False, False, False)      # the proving call itself runs the list kernel
    assert m.tick(11, 3, False) == (3, True, True, False)
    m.read()
    assert m.tick(14, 0, True).ticks == 0                      # a call of no ticks changes nothing
    assert m.tick(14, 2, True).steady
    m.diag_enable(True)
    assert m.tick(16, 2, True) == (2, True, False, False)      # device counters: the general body
    m.diag_enable(False)
    assert m.tick(18, 2, True).steady
    assert m.tick(21, 2, True) == (2, True, False, False)      # a gap: the phase is gone for good,
    assert m.tick(23, 2, True) == (2, True, False, False)      # the list skip is not
    m.init_steady(0, 0)
    assert m.tick(1, 6, False) == (6, False, False, False)     # without statistics nothing is proven
    assert m.tick(7, 6, True) == (6, False, False, False)
    assert m.tick(13, 1, True).steady
    for destroy in (m.load_state, m.load_checkpoint, m.handler_batch, m.init_new_nodes):
        m.init_steady(0, 0)
        m.tick(1, 6, True)
        assert m.tick(7, 1, True).steady
        destroy()
        assert m.tick(8, 1, True) == (1, False, False, False)
        assert m.tick(9, 1, True) == (1, False, False, False)  # (no origin: a call with statistics proves nothing)
    # one tick per launch
    f = M.Model(dict(cfg, ticks_per_launch=16))
    f.init_steady(0, 0)
    f.tick(1, 6, True)
    assert f.tick(7, 4, True) == (4, True, False, False)       # fused launches
    f.profile(3)
    assert f.tick(11, 4, True) == (4, True, True, False)
    f.profile(1)
    assert f.tick(15, 4, True) == (4, True, False, False)
    c = M.Model(dict(cfg, ticks_per_launch=16, payload_crc=1))
    c.init_steady(0, 0)
    c.tick(1, 6, True)
    assert c.tick(7, 4, True).steady
    # the knob, E < K, the bound, the split
    k = M.Model(cfg, {"RAFTSTEP_STEADY_FORM": "0"})
    k.init_steady(0, 0)
    k.tick(1, 6, True)
    assert k.tick(7, 4, True) == (4, True, False, False)
    e = M.Model(dict(cfg, entries_per_tick=16))
    e.init_steady(0, 0)
    e.tick(1, 6, True)
    assert e.tick(7, 4, True) == (4, False, False, False)
    b = M.Model(dict(cfg, entries_per_tick=16, ring_depth=64))
    b.init_steady(0, 124999985)
    b.tick(124999986, 6, True)
    assert b.tick(124999992, 5, True).steady                   # 16 * (124999992 + 5 + 2) = 2e9 - 16
    assert not b.tick(124999997, 1, True).skip                 # 16 * (124999997 + 1 + 2) = 2e9
    for G, split in ((131071, False), (131072, True), (131072 + 257, True), (3000, False)):
        s = M.Model(dict(cfg, groups=G))
        s.init_steady(0, 0)
        s.tick(1, 6, True)
        assert s.tick(7, 1, True) == (1, True, True, split), G
    s = M.Model(dict(cfg, groups=131072), {"RAFTSTEP_SPLIT_STEADY": "0"})
    s.init_steady(0, 0)
    s.tick(1, 6, True)
    assert s.tick(7, 1, True) == (1, True, True, False)


@pytest.mark.parametrize("name", sorted(M.CONFIGS))
def test_committed_schedules_cover_the_contract(name):
    cfg, env, seeds = M.CONFIGS[name]
    between, recovered, kinds = set(), set(), set()
    for seed in seeds:
        ops = M.schedule(seed, M.N_OPS, cfg)
        ticks, steady, b, r = M.coverage(ops, cfg, env)
        assert ticks > 0 and 2 * steady >= ticks, f"seed {seed}: steady form for {steady} of {ticks} ticks"
        between |= b
        recovered |= r
        kinds |= {op[0] for op in ops}
    assert between == set(M.KEEPING), f"never directly between two steady-form calls: {set(M.KEEPING) - between}"
    assert kinds >= set(M.OPS), f"never drawn: {set(M.OPS) - kinds}"
    for kind in ("gap", "load_state", "checkpoint"):
        assert kind in recovered, f"{kind}: never followed by an init_steady and the steady form again"
    assert recovered & set(M.BATCHES), "no handler batch is followed by an init_steady and the steady form again"


@pytest.mark.parametrize("name", sorted(M.CONFIGS))
def test_committed_schedules_run_on_the_oracle(name):
    """Every state-changing operation goes through the oracle alone (the reads,
    profile and diag operations go to the engine alone on the GPU): none
    fails, ticks run where the model says, and the steady-state stretches
    commit every entry appended (no fault, a leader in every group)."""
    cfg, env, seeds = M.CONFIGS[name]
    G, E = cfg["groups"], cfg.get("entries_per_tick", 1)
    for seed in seeds:
        ops = M.schedule(seed, M.N_OPS, cfg)
        o = oracle.Oracle(**cfg)
        t = 0
        for i, op, first, pred in M.walk(ops, cfg, env):
            if op[0] not in ("tick", "tick0", "gap", "init_steady") + M.BATCHES:
                continue
            if first is not None:
                assert first == t, (seed, i)
            t, res = H.apply_op(o, op, t, cfg, threads=8)
            if op[0] == "tick" and op[2] and pred.skip:
                # the compressed steady state: every group's leader commits this call's entries
                assert res[6] == 0 and res[7] == G * op[1] and res[0] == G * E * op[1], (seed, i, op, list(res))
        st = o.store_state()
        assert st["last"].shape == (G, cfg["replicas"]) and np.all(st["last"] >= 0)
        o.close()
