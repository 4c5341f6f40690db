"""raft_load_groups restated over the oracle and numpy.

Written from the rules of include/raftstep.h ("group directory",
raft_load_groups), not from the kernels:
  complete  the rows a listed group reads back after the load: the oracle's
            own raft_load_state derivations of the optional fields (log_crc
            stamped from (term, value) with payload_crc, next = match + 1 when
            absent or 0, hwm = last when absent or below it, iso_victim 0), by
            loading the rows into a scratch oracle of len(rows) groups and
            storing them back;
  load      a listed group holds what raft_load_state would give it from the
            same rows, every other group is untouched: splice, then load_state;
  cursors   every fed cursor of a loaded group becomes min(CommitIndex,
            LastApplied) of that replica's loaded row.
Also the donor states the CPU and GPU tests take their rows from, and the
classes of rows a test has to cover.
"""
import functools

import numpy as np

import groups_model as GM
import oracle
from raftstep import abi

G = 1101
# the donors: new-node churn under leader isolation, every log past the ring wrap at tick 60
DONOR = dict(replicas=3, groups=G, ring_depth=16, entries_per_tick=1, client_period=1, isolate_per_65536=8000,
             isolate_min_ticks=4, isolate_max_ticks=16, isolate_leader=1, group_base=900000)
DONOR_REF = dict(DONOR, seed=0xD0D0)
DONOR_RAFT = dict(DONOR, semantics=1, seed=0xD0D1)
DONOR_TICKS = 60


def complete(cfg, rows):
    """The (possibly partial) rows as a scratch oracle of len(rows) groups
    reads them back after load_state: every field of the view."""
    n = len(rows["fault"])
    kw = dict(GM.cfg_kw(cfg), groups=n)
    with oracle.Oracle(**kw) as o:
        o.load_state(rows)
        return o.store_state()


def load(impl, ids, rows):
    """raft_load_groups on the oracle (or on an engine, as raft_load_state of
    the spliced view): returns the state loaded."""
    st = GM.splice(impl.store_state(), ids, complete(impl.cfg, rows))
    impl.load_state(st)
    return st


def load_cursors(cursors, ids, rows):
    """Feed cursors after a load of `rows` into `ids`: the fed ones (>= 0) of
    those groups become min(commit, last) of the loaded rows."""
    c = np.array(cursors, copy=True)
    ids = np.asarray(ids, np.int64)
    new = np.minimum(np.asarray(rows["commit"]), np.asarray(rows["last"])).astype(c.dtype)
    c[ids] = np.where(c[ids] >= 0, new, c[ids])
    return c


def take(state, rows):
    """Rows `rows` of a canonical view, indexed by list position."""
    rows = np.asarray(rows, np.int64)
    return {k: np.ascontiguousarray(v[rows]) for k, v in state.items()}


@functools.lru_cache(maxsize=None)
def _donor(items, how, ticks):
    kw = dict(items)
    with oracle.Oracle(**kw) as o:
        if how == "new":
            o.init_new_nodes(0)
            o.tick(0, ticks, threads=16)
        else:
            o.init_steady(-1, 0)
            o.tick(1, ticks, threads=16)
        st = o.store_state()
    for v in st.values():
        v.setflags(write=False)   # shared among the tests: left unchanged
    return st


def donor(kw, how="new", ticks=DONOR_TICKS):
    """The donor state of configuration kw (computed once per process)."""
    return _donor(tuple(sorted(kw.items())), how, ticks)


def classes(st, raft, K):
    """Per class of rows the loader has to get right: a bool[G] of the groups in it."""
    role, last = st["role"], st["last"]
    leaders = (role == abi.LEADER).sum(axis=1)
    c = {
        "code2": st["fault"] == abi.F_DEADLOCK_VRES,
        "code3": st["fault"] == abi.F_DEADLOCK_LEADER_VREQ,
        "candidate": (role == abi.CANDIDATE).any(axis=1),
        "iso_victim": st["iso_victim"] != 0,
        "wrapped": (last > K).any(axis=1),
        "healthy_leader": (st["fault"] == 0) & (leaders == 1),
    }
    if raft:
        is_l = role == abi.LEADER
        peer = ~np.eye(role.shape[1], dtype=bool)[None]
        stored = is_l[:, :, None] & peer & (st["next"] != st["match"] + 1)
        c.update({
            "two_leaders": leaders >= 2,
            "hwm_above_last": (st["hwm"] > last).any(axis=1),
            "stored_next": stored.any(axis=(1, 2)),
            "code4": st["fault"] == abi.F_RING_EVICTED,
        })
        for k in ("code2", "code3", "candidate"):   # (REF's classes: the RAFT donor at tick 60 holds none)
            c.pop(k)
    else:
        c["empty_log"] = (last == 0).any(axis=1)
    return c


def pick(st, raft, K, n, seed):
    """About n donor groups holding every class of the semantics: up to 6 of
    each class, filled up with random others. Asserts the coverage."""
    rng = np.random.default_rng(seed)
    cl = classes(st, raft, K)
    rows = []
    for name, m in cl.items():
        g = np.nonzero(m)[0]
        assert len(g), f"the donor holds no group of class {name}"
        rows.extend(rng.permutation(g)[:6].tolist())
    rows = list(dict.fromkeys(rows))
    rest = np.setdiff1d(np.arange(len(st["fault"])), rows)
    rows.extend(rng.permutation(rest)[:max(0, n - len(rows))].tolist())
    rows = np.array(rows)
    for name, m in cl.items():
        assert m[rows].any(), name
    return rows
