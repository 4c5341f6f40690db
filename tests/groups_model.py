"""The group directory (raft_group_scan / raft_store_groups /
raft_restart_groups) restated in numpy over a canonical view.

Written from the rules of include/raftstep.h ("group directory"), not from
the kernels:
  scan     a group g in [first_group, G) is a hit when
             select & FAULTED    and fault[g] != 0, or
             select & LEADERLESS and fault[g] == 0 and no role[g, r] is Leader;
           hits in ascending group order, the first `cap` written;
           next_group = G when every hit was written, the id after the last
           hit written otherwise (first_group when none was written);
  restart  the rows of a fresh oracle after init_new_nodes(tick0): NewNode x R
           (main.go:59-76) + the FollowerRun entry (main.go:113-115), keyed by
           the global group id, spliced over the listed groups;
  cursors  every fed cursor of a restarted group becomes
           min(CommitIndex, LastApplied) of the new state, that is 0.
"""
import numpy as np

import oracle
from raftstep import abi

FAULTED, LEADERLESS = abi.SELECT_FAULTED, abi.SELECT_LEADERLESS


def leaders(state):
    """Per group the lowest-id replica whose role is Leader, 0xFF: none."""
    is_l = np.asarray(state["role"]) == abi.LEADER
    return np.where(is_l.any(axis=1), is_l.argmax(axis=1), abi.NO_LEADER).astype(np.uint8)


def scan(state, select, first_group=0, cap=None, group_base=0):
    """(hits as abi.GROUP_HIT, info dict) of one raft_group_scan call."""
    fault = np.asarray(state["fault"])
    G = len(fault)
    assert select and not select & ~(FAULTED | LEADERLESS) and 0 <= first_group <= G
    ld = leaders(state)
    hit = np.zeros(G, bool)
    if select & FAULTED:
        hit |= fault != 0
    if select & LEADERLESS:
        hit |= (fault == 0) & (ld == abi.NO_LEADER)
    hit[:first_group] = False
    g = np.nonzero(hit)[0]
    matched = len(g)
    written = matched if cap is None else min(int(cap), matched)
    g = g[:written]
    out = np.zeros(written, abi.GROUP_HIT)
    out["group"] = group_base + g
    out["local"] = g
    out["fault"] = fault[g]
    out["leader"] = ld[g]
    nxt = G if written == matched else (int(g[-1]) + 1 if written else first_group)
    return out, dict(matched=matched, written=written, next_group=nxt)


def cfg_kw(cfg):
    """The keyword arguments that rebuild an abi.Config."""
    return {k: getattr(cfg, k) for k, _ in abi.Config._fields_ if k not in ("abi_version", "reserved")}


def restart_rows(cfg, ids, tick0):
    """The canonical rows of groups `ids` (local) of a fresh oracle with this
    configuration after init_new_nodes(tick0), indexed by list position."""
    with oracle.Oracle(**cfg_kw(cfg)) as o:
        o.init_new_nodes(tick0)
        st = o.store_state()
    ids = np.asarray(ids, np.int64)
    return {k: v[ids].copy() for k, v in st.items()}


def splice(state, ids, rows):
    """A copy of `state` with rows[i] in place of group ids[i]."""
    ids = np.asarray(ids, np.int64)
    out = {k: np.array(v, copy=True) for k, v in state.items()}
    for k in out:
        out[k][ids] = rows[k]
    return out


def restart(impl, ids, tick0):
    """raft_restart_groups on the oracle: store, splice the fresh rows, load."""
    st = splice(impl.store_state(), ids, restart_rows(impl.cfg, ids, tick0))
    impl.load_state(st)
    return st


def restart_cursors(cursors, ids):
    """Feed cursors after a restart of `ids`: the fed ones (>= 0) of those groups become 0."""
    c = np.array(cursors, copy=True)
    ids = np.asarray(ids, np.int64)
    c[ids] = np.where(c[ids] >= 0, 0, c[ids])
    return c
