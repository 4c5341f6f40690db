"""The commit feed (raft_feed_poll) restated in numpy over a canonical view.

Written from the rules of include/raftstep.h ("commit feed"), not from the
kernels: for a pair with cursor c, CommitIndex cm, LastApplied l and
high-water mark h,
  1. hi = min(cm, l);
  2. hi < c: the pair is stalled and left alone;
  3. lo = min(max(c, h - K), hi); the lo - c entries that left the ring are
     lost and skipped whatever the cap is;
  4. entries lo+1 .. hi are deliverable.
All pairs' deliverable entries in (group, replica, index) order are cut at
`cap`; the cursors advance by exactly what was delivered. Entry i of a log is
read at slot (i-1) mod K of the view's log_* arrays.
"""
import numpy as np

from raftstep import abi


def mask_of(replicas, R):
    """Replica mask of an iterable of ids, a mask or None (all), as a bool[R]."""
    if replicas is None:
        m = (1 << R) - 1
    elif isinstance(replicas, (int, np.integer)):
        m = int(replicas)
    else:
        m = sum(1 << int(r) for r in set(replicas))
    return np.array([(m >> r) & 1 for r in range(R)], bool)


def start_cursors(st, replicas=None, start="commit"):
    """The cursors raft_feed_open leaves: [G][R] int32, -1 outside the mask."""
    G, R = st["last"].shape
    m = mask_of(replicas, R)
    c = np.zeros((G, R), np.int32) if start == "start" else np.minimum(st["commit"], st["last"]).astype(np.int32)
    c[:, ~m] = -1
    return c


def poll(st, cursors, cap=None, group_base=0):
    """One poll over the view `st` with cursors [G][R] (-1: replica outside the
    mask). Returns (entries as abi.FEED_ENTRY, info dict, the new cursors)."""
    G, R, K = st["log_term"].shape
    c = np.asarray(cursors).astype(np.int64)
    fed = c >= 0
    cm, l = st["commit"].astype(np.int64), st["last"].astype(np.int64)
    h = np.maximum(st["hwm"].astype(np.int64), l)   # (a view without hwm: REF, h = l)
    hi = np.minimum(cm, l)
    stalled = fed & (hi < c)
    live = fed & ~stalled
    lo = np.where(live, np.minimum(np.maximum(c, h - K), hi), c)
    n = np.where(live, hi - lo, 0)
    total = int(n.sum())
    delivered = total if cap is None else min(int(cap), total)
    off = np.cumsum(n.ravel()) - n.ravel()                     # (group, replica) order
    take = np.clip(delivered - off, 0, n.ravel())
    new = np.where(live, lo + take.reshape(G, R), c).astype(np.int32)
    pair = np.repeat(np.arange(G * R), take)                   # the pair of every delivered entry
    first = np.cumsum(take) - take
    idx = lo.ravel()[pair] + 1 + (np.arange(delivered) - first[pair])
    g, r = pair // R, pair % R
    slot = (idx - 1) % K
    out = np.zeros(delivered, abi.FEED_ENTRY)
    out["group"] = group_base + g
    out["replica"] = r
    out["index"] = idx
    out["term"] = st["log_term"][g, r, slot]
    out["value"] = st["log_value"][g, r, slot]
    out["crc"] = st["log_crc"][g, r, slot]
    info = dict(delivered=delivered, pending=total - delivered, lost=int((lo - c)[live].sum()),
                stalled=int(stalled.sum()))
    return out, info, new


def disagreements(entries):
    """Delivered (group, index) pairs on which two replicas' records differ in
    term, value or crc (committed entries agree across replicas)."""
    if not len(entries):
        return 0
    o = np.lexsort((entries["replica"], entries["index"], entries["group"]))
    e = entries[o]
    same = (e["group"][1:] == e["group"][:-1]) & (e["index"][1:] == e["index"][:-1])
    diff = (e["term"][1:] != e["term"][:-1]) | (e["value"][1:] != e["value"][:-1]) | (e["crc"][1:] != e["crc"][:-1])
    return int((same & diff).sum())
