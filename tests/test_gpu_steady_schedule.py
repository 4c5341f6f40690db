"""GPU: generated host call schedules (tests/steady_model.py) on the engine and
the CPU oracle. The engine decides call by call, from its continuity records,
whether the list kernel is skipped and whether the lean kernel's steady form
may run; the model predicts both from the documented contract, and the host
counters (raft_diag_read: ticks, ticks_list_skipped, ticks_steady_form) must
equal its prediction after every call — while sums, per-tick records, digests,
every host read and the final state equal the oracle's.

Reads, profile and diag operations go to the engine alone; client values are
staged for each call on both sides. raft_debug_group_words has no oracle
equivalent (raw device words): it is called for what it does to the shared
entries, and only its shape is checked. tests/test_steady_model.py holds the
committed seeds to the conditions that keep this from passing vacuously."""
import numpy as np
import pytest

import harness as H
import oracle
import steady_model as M
from raftstep import Engine

pytestmark = pytest.mark.gpu
THREADS = 8


def _same_digests(e, o, what):
    de, do = e.state_digest(), o.state_digest()
    bad = np.nonzero(de[0] != do[0])[0]
    if bad.size or de[1] != do[1]:
        g = int(bad[0]) if bad.size else 0
        raise AssertionError(f"{what}: {bad.size} digests differ, first {bad[:4].tolist()}\nengine:\n{e.nodelog(g)}"
                             f"oracle:\n{o.nodelog(g)}engine words: {e.debug_group_words(g)}")


def _apply(e, o, op, t, pred, cfg, tmp_path):
    """One operation on both sides, checked; returns the next tick."""
    kind = op[0]
    if kind in ("tick", "tick0"):
        k, stats = (op[1], op[2]) if kind == "tick" else (0, op[1])
        t1, se = H.apply_op(e, op, t, cfg)
        if k and o.cfg.client_source:
            o.stage_values(t, H.staged_values(int(o.cfg.seed), t, k, o.cfg.entries_per_tick, o.cfg.groups))
        recs = np.array([o.tick(t + i, 1, threads=THREADS) for i in range(k)], np.int64).reshape(k, 8)
        if not k:
            o.tick(t, 0)
        if stats:
            assert list(se) == list(recs.sum(0)), f"sums of ticks [{t}, {t + k})"
            if k:
                assert np.array_equal(e.tick_records(k), recs), f"per-tick records of ticks [{t}, {t + k})"
        _same_digests(e, o, f"after ticks [{t}, {t + k})")
        c = e.diag_read()
        got = (c["ticks"], c["ticks_list_skipped"], c["ticks_steady_form"])
        want = (k, k if pred.skip else 0, k if pred.steady else 0)
        assert got == want, f"ticks [{t}, {t + k}): (ticks, list skipped, steady form) {got}, the model predicts {want}"
        return t1
    if kind in ("gap", "init_steady"):
        H.apply_op(e, op, t, cfg)
        return H.apply_op(o, op, t, cfg)[0]
    if kind in M.BATCHES:
        re, ro = H.apply_op(e, op, t, cfg)[1], H.apply_op(o, op, t, cfg)[1]
        assert np.array_equal(re, ro), f"{kind}: responses differ"
        _same_digests(e, o, f"after {kind}")
    elif kind == "store_state":
        H.assert_same_state(e.store_state(), o.store_state(), "store_state")
    elif kind == "store_state_range":
        g0, n = op[1], op[2]
        whole = o.store_state()
        H.assert_same_state(e.store_state_range(g0, n), {k: v[g0:g0 + n] for k, v in whole.items()},
                            f"store_state_range({g0}, {n})")
    elif kind == "state_digest":
        _same_digests(e, o, "state_digest")
    elif kind == "nodelog":
        assert e.nodelog(op[1]) == o.nodelog(op[1]), f"nodelog({op[1]})"
    elif kind == "debug_group_words":
        w = e.debug_group_words(op[1])
        assert len(w) == 14 and all(isinstance(x, int) for x in w.values())
    elif kind == "sync":
        e.sync()
    elif kind == "checkpoint":
        path = tmp_path / "schedule.ckpt"
        e.save_checkpoint(path)
        e.load_checkpoint(path)
        _same_digests(e, o, "after the checkpoint load")
    elif kind == "load_state":
        e.load_state(o.store_state())
        _same_digests(e, o, "after load_state")
    elif kind == "diag_enable":
        e.diag_enable(op[1])
    else:
        assert kind == "profile", kind
        e.profile(op[1])
    return t


CASES = [(name, seed) for name in sorted(M.CONFIGS) for seed in M.CONFIGS[name][2]]


@pytest.mark.parametrize("name,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_schedule_matches_oracle_and_model(monkeypatch, tmp_path, name, seed):
    cfg, env, _ = M.CONFIGS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ops = M.schedule(seed, M.N_OPS, cfg)
    e, o = Engine(**cfg), oracle.Oracle(**cfg)
    t = 0
    for i, op, first, pred in M.walk(ops, cfg, env):
        try:
            assert first is None or first == t
            t = _apply(e, o, op, t, pred, cfg, tmp_path)
        except Exception as x:
            shown = "\n".join(f"  {j}: {p}" for j, p in enumerate(ops[:i + 1]))
            raise AssertionError(f"config {name}, seed {seed}, operation {i} {op} at tick {t}: {x}\n"
                                 f"M.schedule({seed}, {M.N_OPS}, cfg)[:{i + 1}] =\n{shown}") from x
    H.assert_same_state(e.store_state(), o.store_state(), f"config {name}, seed {seed}: at the end")
