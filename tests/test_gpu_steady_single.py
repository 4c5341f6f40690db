"""GPU: the straight-line steady body (tick_steady.hpp) and its two
instantiations against the CPU oracle: the one-entry one (trace-RNG values,
one client entry per tick, plain record stores, the shared ring — the headline
shape's whole tick) and the generic one (everything else: E > 1, ticks without
client entries, staged values, RAFTSTEP_SH=0, streaming record stores), each
launched once per tick or as two halves. Every case checks the per-tick
records and the digests after every call, the whole state at its end, and by
the host counters (raft_diag_read) that the steady form is what ran, that the
one-entry instantiation ran exactly the launches it is for, and in which launch
form."""
import os

import numpy as np
import pytest

import harness as H
import oracle
from raftstep import Engine, RaftError, abi

pytestmark = pytest.mark.gpu
REF, RAFT = abi.SEM_REF, abi.SEM_RAFT
STAGED = abi.CLIENT_STAGED
NOSH = {"RAFTSTEP_SH": "0"}
KW0 = dict(replicas=5, groups=513, ring_depth=16, client_period=1, seed=0x5EED0002)
CALLS = (6, 1, 9, 4)   # the proving call, then the steady form (the 16-slot ring wraps with E = 3)

# the launch-uniform cases: which instantiation a tick runs is decided by the
# shared ring, the value source, the tick's client entries and the record stores
FORMS = {
    "c2": dict(),                                                       # one-entry
    "R3_raft": dict(replicas=3, semantics=RAFT),                        # one-entry
    "R7_ref": dict(replicas=7, semantics=REF),                          # one-entry
    "R3_crc": dict(replicas=3, payload_crc=1),                          # one-entry with the CRC stamp
    "R7_raft_crc": dict(replicas=7, semantics=RAFT, payload_crc=1),
    "E3": dict(entries_per_tick=3),                                     # generic: the entry loop
    "R7_raft_E3_crc": dict(replicas=7, semantics=RAFT, entries_per_tick=3, payload_crc=1),
    "period2": dict(client_period=2),                                   # one-entry and, n == 0, generic ticks alternate
    "period2_R3_raft_E3_crc": dict(client_period=2, replicas=3, semantics=RAFT, entries_per_tick=3, payload_crc=1),
    "staged": dict(client_source=STAGED),                               # generic: staged values
    "staged_raft_E3_crc": dict(client_source=STAGED, semantics=RAFT, entries_per_tick=3, payload_crc=1),
    "staged_period2_R3": dict(client_source=STAGED, client_period=2, replicas=3),
    "nosh": dict(env=NOSH),                                             # generic: whole ring rows
    "nosh_R7_raft_E3_crc": dict(env=NOSH, replicas=7, semantics=RAFT, entries_per_tick=3, payload_crc=1),
    "nosh_R3_period2": dict(env=NOSH, replicas=3, client_period=2),
    "nosh_staged_E3": dict(env=NOSH, client_source=STAGED, entries_per_tick=3),
}
SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513]
# every size in the one-entry body, the generic body with the shared ring
# (entry loop, empty ticks, CRC) and the generic body with whole ring rows
SIZE_FORMS = ["c2", "period2_R3_raft_E3_crc", "nosh_R7_raft_E3_crc"]


def _values(seed, t, n, E, groups):
    return np.random.default_rng([seed, t]).integers(0, 1 << 62, size=(n, E, groups), dtype=np.int64)


def _engine_kw(monkeypatch, form, **over):
    c = dict(FORMS[form])
    for k, v in c.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    return dict(KW0, **c, **over)


def _pair(leader=-1, **kw):
    e, o = Engine(**kw), oracle.Oracle(**kw)
    e.init_steady(leader, 0)
    o.init_steady(leader, 0)
    return e, o


def _one_ticks(e, t, k):
    """Ticks of [t, t + k) that the one-entry instantiation runs when the steady
    form does: the shared ring, trace-RNG values, exactly one client entry in
    the tick (client_entries: E at every client_period-th tick) and plain
    record stores (every engine here but the streaming-store one)."""
    c = e.cfg
    if os.environ.get("RAFTSTEP_SH") == "0" or c.client_source == STAGED or c.entries_per_tick != 1:
        return 0
    return sum(1 for x in range(t, t + k) if x % c.client_period == 0)


def _form(e, t, k, steady=True, split=None, one=None):
    """The host counters of the call of ticks [t, t + k) just made: the steady
    form ran all of it (or none), the one-entry instantiation exactly the
    launches it is for (two per tick of a split call), and, where the caller
    knows it, whether the call was issued as two halves."""
    c = e.diag_read()
    assert c["ticks"] == k and c["ticks_steady_form"] == (k if steady else 0), (t, k, c)
    halves = 2 if c["ticks_split"] else 1
    assert c["ticks_split"] in (0, k), c
    want = (_one_ticks(e, t, k) if one is None else one) * halves if steady else 0
    assert c["launches_steady_one"] == want, (t, k, want, c)
    if split is not None:
        assert c["ticks_split"] == (k if split else 0), (t, k, c)


def _call(e, o, t, k, stats=True, threads=1, records=True):
    if e.cfg.client_source == STAGED:
        v = _values(int(e.cfg.seed), t, k, e.cfg.entries_per_tick, e.cfg.groups)
        e.stage_values(t, v)
        o.stage_values(t, v)
    se = e.tick(t, k, stats=stats)
    if records:
        recs = np.array([o.tick(t + i, 1, threads=threads) for i in range(k)], np.int64)
    else:
        recs = np.array([o.tick(t, k, threads=threads)], np.int64)
    if stats:
        assert list(se) == list(recs.sum(0)), f"sums of ticks [{t}, {t + k})"
        if records:
            assert np.array_equal(e.tick_records(k), recs), f"per-tick records of ticks [{t}, {t + k})"
    de, do = e.state_digest(), o.state_digest()
    bad = np.nonzero(de[0] != do[0])[0]
    assert not bad.size and de[1] == do[1], f"after tick {t + k - 1}: {bad.size} digests differ, first {bad[:4]}"
    return t + k


def _run(e, o, calls=CALLS, **kw):
    t = 1
    for i, k in enumerate(calls):
        t = _call(e, o, t, k, **kw)
        _form(e, t - k, k, steady=i > 0, split=False)   # (the first call proves the list empty; too few groups to split)
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")
    return t


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_form_against_the_oracle(monkeypatch, form):
    """513 groups: two whole blocks and one live lane in the third."""
    e, o = _pair(**_engine_kw(monkeypatch, form))
    t = _run(e, o)
    # the host read copied the shared entries back: the next call re-enters the shared form
    t = _call(e, o, t, 5)
    _form(e, t - 5, 5, split=False)
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")


@pytest.mark.parametrize("form", SIZE_FORMS)
@pytest.mark.parametrize("groups", SIZES)
def test_block_and_wave_edges(monkeypatch, groups, form):
    """A lane past the last group reads the last group's words and stores
    nothing: fewer groups than a wave, than a block and than two, whole waves
    and blocks, one live lane in the last wave / block."""
    e, o = _pair(**_engine_kw(monkeypatch, form, groups=groups))
    _run(e, o)


@pytest.mark.parametrize("form", ["c2", "period2_R3_raft_E3_crc"])
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("groups", [131072, 131329])
def test_one_launch_and_two_halves(monkeypatch, groups, split, form):
    """131072 groups is the smallest count that splits, 131329 leaves one live
    lane in the second half's last block: RAFTSTEP_SPLIT_STEADY forces one
    launch per tick or the two halves, whichever the default is."""
    monkeypatch.setenv("RAFTSTEP_SPLIT_STEADY", split)
    e, o = _pair(**_engine_kw(monkeypatch, form, groups=groups))
    t = 1
    for i, (k, st) in enumerate(((6, True), (3, False), (2, True), (5, True))):
        t = _call(e, o, t, k, stats=st, threads=16, records=(k == 2))
        _form(e, t - k, k, steady=i > 0, split=i > 0 and split == "1")   # (ticks_split counts list-skipping ticks)
    H.assert_same_state(e.store_state(), o.store_state(), f"after tick {t - 1}")


def test_default_split_by_call_length_and_shape(monkeypatch):
    """RAFTSTEP_SPLIT_STEADY unset, 131329 groups (enough to split): the
    one-entry shape runs a call of fewer than 48 ticks as one launch per tick
    and one of 48 ticks as two halves; a shape with longer waves (three
    entries per tick) keeps the halves at any length; exact either way."""
    monkeypatch.delenv("RAFTSTEP_SPLIT_STEADY", raising=False)
    for form, plan in (("c2", ((6, None), (47, False), (48, True))), ("E3", ((6, None), (5, True)))):
        e, o = _pair(**_engine_kw(monkeypatch, form, groups=131072))
        t = 1
        for i, (k, split) in enumerate(plan):
            t = _call(e, o, t, k, threads=16, records=False)
            _form(e, t - k, k, steady=i > 0, split=bool(split))
        H.assert_same_state(e.store_state(), o.store_state(), f"{form}: after tick {t - 1}")
        e.close()


def test_streaming_record_stores():
    """The generic body's streaming record stores (DevPlanes::rec_nt: padded
    groups * 40 B > 256 MiB; the size tests/test_gpu_steady_form.py derives),
    which the one-entry body leaves to it: three oracle slices of 700 groups —
    group 0, across the boundary between the halves, the last groups."""
    groups, slice_n = 6710785, 700
    assert ((groups + 255) & ~255) * 40 > 256 << 20 >= ((groups - 1 + 255) & ~255) * 40
    kw = dict(replicas=3, groups=groups, ring_depth=2, entries_per_tick=1, client_period=1, seed=0x5EED0002)
    offs = [0, ((groups // 2) & ~255) - slice_n // 2, groups - slice_n]
    e = Engine(**kw)
    slices = [oracle.Oracle(**dict(kw, groups=slice_n, group_base=off)) for off in offs]
    for x in [e] + slices:
        x.init_steady(-1, 0)
    t = 1
    for i, (k, st) in enumerate(((6, True), (1, True), (5, False), (3, True))):
        se = e.tick(t, k, stats=st)
        for o in slices:
            o.tick(t, k)
        t += k
        if st:
            assert se[6] == 0 and se[7] == groups * k, list(se)
        d, _ = e.state_digest()
        for o, off in zip(slices, offs):
            bad = np.nonzero(d[off:off + slice_n] != o.state_digest()[0])[0]
            assert not bad.size, f"after tick {t - 1}: slice at {off}: {bad.size} digests differ, first {bad[:4]}"
        _form(e, t - k, k, steady=i > 0, split=False, one=0)   # (short calls of one-entry ticks: one launch)
    for o, off in zip(slices, offs):
        H.assert_same_state(e.store_state_range(off, slice_n), o.store_state(), f"slice at {off}")


@pytest.mark.parametrize("form", ["c2", "E3"])
def test_a_lane_that_does_not_fit_ends_in_einternal(monkeypatch, form):
    """debug_force_pass during a steady-form call: the lane leaves its group
    alone and appends its id to the list; the end-of-call check turns that
    into RAFT_EINTERNAL and poisons the engine until its state is replaced."""
    e, o = _pair(**_engine_kw(monkeypatch, form, groups=3000))
    t = _call(e, o, 1, 6)
    _form(e, 1, 6, steady=False, split=False)
    t = _call(e, o, t, 5)
    _form(e, t - 5, 5, split=False)
    e.debug_force_pass(42)
    with pytest.raises(RaftError, match="list kernel that did not run") as ei:
        e.tick(t, 4)
    assert ei.value.code == abi.RAFT_EINTERNAL
    _form(e, t, 4, split=False)             # (the steady form is what ran)
    with pytest.raises(RaftError, match="engine state is invalid"):
        e.tick(t + 4, 1)
    e.debug_force_pass(-1)
    e.init_steady(-1, 0)
    o.init_steady(-1, 0)
    t = _call(e, o, 1, 6)
    t = _call(e, o, t, 7)
    assert e.diag_read()["ticks_steady_form"] == 7
    H.assert_same_state(e.store_state(), o.store_state(), "after init_steady")
