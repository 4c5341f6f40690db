"""The applied state (raft_apply_*) restated in numpy and plain Python ints
over a canonical view.

Written from the rules of include/raftstep.h ("applied state"), not from the
kernel. The model holds its own [G][R] records (abi.APPLY_RECORD; applied = -1
for a replica outside the mask). All chain arithmetic is 64-bit and wrapping:
  seed(gid, base) = sm(sm(gid) ^ uint64(uint32(base)))
  fold of entry i (Term T, Value V):
      chain' = sm(sm(chain ^ (uint64(uint32(T)) << 32 | uint32(i))) ^ uint64(V))
A step treats a fed pair with applied c, CommitIndex cm, LastApplied l and
high-water mark h:
  1. hi = min(cm, l); hi < c: stalled, left alone, trajectory {c: chain};
  2. lo = min(max(c, h - K), hi); lo > c: lost += lo - c, gapped += 1, gaps += 1
     (saturating), base = lo, chain = seed(gid, lo), sum = 0;
  3. entries lo+1 .. hi are folded in order, applied = hi; the trajectory is
     the chain at lo and after every folded index.
Two fed replicas are comparable when their bases after the step are equal; a
comparable pair diverges at the smallest index both trajectories hold with
different chains; a replica with div_index 0 in a diverging pair gets the
smallest such index over its pairs and the lowest-id peer attaining it. Entry
i of a log is read at slot (i-1) mod K of the view's log_* arrays.
"""
import numpy as np

from feed_model import mask_of
from raftstep import abi

M64 = (1 << 64) - 1
NO_PEER = 0xFF
_BIG = np.int64(1) << np.int64(40)   # above every log index


def sm(x):
    """The engine's splitmix64 step on a Python int."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def seed(gid, base):
    return sm(sm(gid) ^ (base & 0xFFFFFFFF))


def fold(chain, i, term, value):
    return sm(sm(chain ^ (((term & 0xFFFFFFFF) << 32) | (i & 0xFFFFFFFF))) ^ (value & M64))


def _sm_np(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _u32(a):
    return (np.asarray(a).astype(np.int64) & np.int64(0xFFFFFFFF)).astype(np.uint64)


def _seed_np(gid, base):
    return _sm_np(_sm_np(gid) ^ _u32(base))


def _fold_np(chain, i, term, value):
    return _sm_np(_sm_np(chain ^ ((_u32(term) << np.uint64(32)) | _u32(i))) ^ value.astype(np.int64).view(np.uint64))


def _gids(G, R, group_base):
    return np.repeat((np.arange(G, dtype=np.uint64) + np.uint64(group_base))[:, None], R, axis=1)


def start_records(st, replicas=None, start="commit", group_base=0):
    """The records raft_apply_open leaves for start = "start" or "commit"."""
    G, R = st["last"].shape
    m = mask_of(replicas, R)
    rec = np.zeros((G, R), abi.APPLY_RECORD)
    b = np.zeros((G, R), np.int64) if start == "start" else np.minimum(st["commit"], st["last"]).astype(np.int64)
    rec["applied"] = rec["base"] = b
    rec["chain"] = _seed_np(_gids(G, R, group_base), b)
    rec["div_peer"] = NO_PEER
    rec[:, ~m] = np.zeros((), abi.APPLY_RECORD)
    rec["applied"][:, ~m] = -1
    return rec


def reset_records(rec, st, ids, start, group_base=0):
    """raft_restart_groups (start = "start") / raft_load_groups ("commit", st
    the view after the load): the fed records of the listed groups reset."""
    fresh = start_records(st, None, start, group_base)
    out = rec.copy()
    ids = np.asarray(ids, np.int64)
    fed = rec["applied"][ids] >= 0
    sub = out[ids]
    sub[fed] = fresh[ids][fed]
    out[ids] = sub
    return out


def records_valid(rec, replicas=None):
    """raft_apply_open(FROM_RECORDS)'s check of the masked replicas' records."""
    m = mask_of(replicas, rec.shape[1])
    x = rec[:, m]
    return bool(((x["base"] >= 0) & (x["base"] <= x["applied"]) & (x["reserved"] == 0)).all())


def step(st, rec, group_base=0):
    """One raft_apply_step over the view `st`: (info dict, the new records)."""
    G, R, K = st["log_term"].shape
    c = rec["applied"].astype(np.int64)
    fed = c >= 0
    cm, l = st["commit"].astype(np.int64), st["last"].astype(np.int64)
    h = np.maximum(st["hwm"].astype(np.int64), l)   # (REF: h = l)
    hi = np.minimum(cm, l)
    stalled = fed & (hi < c)
    live = fed & ~stalled
    lo = np.where(live, np.minimum(np.maximum(c, h - K), hi), c)
    n = np.where(live, hi - lo, 0)
    gap = live & (lo > c)
    base = np.where(gap, lo, rec["base"].astype(np.int64))
    chain = np.where(gap, _seed_np(_gids(G, R, group_base), lo), rec["chain"])
    total = np.where(gap, 0, rec["sum"]).astype(np.int64)
    gaps = np.where(gap, np.minimum(rec["gaps"].astype(np.int64) + 1, 65535), rec["gaps"])
    nmax = int(n.max()) if n.size else 0
    traj = np.zeros((G, R, nmax + 1), np.uint64)    # [.., j]: the chain at index lo + j (j <= n)
    traj[:, :, 0] = chain
    gi, ri = np.meshgrid(np.arange(G), np.arange(R), indexing="ij")
    for j in range(1, nmax + 1):
        act = n >= j
        idx = lo + j
        slot = (idx - 1) % K
        t, v = st["log_term"][gi, ri, slot], st["log_value"][gi, ri, slot]
        chain = np.where(act, _fold_np(chain, idx, t, v), chain)
        with np.errstate(over="ignore"):
            total = np.where(act, total + v, total)
        traj[:, :, j] = chain
    # divergence: per replica a the smallest first-differing index over its comparable peers, lowest peer first
    first = np.full((G, R), _BIG, np.int64)
    peer = np.full((G, R), NO_PEER, np.int64)
    rows = np.arange(G)
    for a in range(R):
        for b in range(R):
            comp = fed[:, a] & fed[:, b] & (base[:, a] == base[:, b])
            if a == b or not comp.any():
                continue
            fd = np.full(G, _BIG, np.int64)
            for j in range(int(n[:, a].max()) + 1):
                i = lo[:, a] + j
                pos = i - lo[:, b]
                ok = comp & (j <= n[:, a]) & (pos >= 0) & (pos <= n[:, b])
                vb = traj[rows, b, np.clip(pos, 0, nmax)]
                fd = np.where(ok & (traj[:, a, j] != vb) & (i < fd), i, fd)
            better = fd < first[:, a]
            first[:, a] = np.where(better, fd, first[:, a])
            peer[:, a] = np.where(better, b, peer[:, a])
    newly = fed & (rec["div_index"] == 0) & (first < _BIG)
    out = rec.copy()
    out["applied"] = np.where(live, hi, rec["applied"])
    out["base"] = base
    out["chain"] = chain
    out["sum"] = total
    out["gaps"] = gaps
    out["div_index"] = np.where(newly, first, rec["div_index"])
    out["div_peer"] = np.where(newly, peer, rec["div_peer"])
    info = dict(folded=int(n.sum()), lost=int((lo - c)[gap].sum()), stalled=int(stalled.sum()),
                gapped=int(gap.sum()), diverged=int(newly.any(axis=1).sum()))
    return info, out


def scan(rec, fault, select, first_group=0, cap=None, group_base=0):
    """raft_apply_scan over the records: (abi.APPLY_HIT array, info dict)."""
    G, R = rec.shape
    fed = rec["applied"] >= 0
    div = fed & (rec["div_index"] != 0)
    gp = fed & (rec["gaps"] != 0)
    flags = div.any(axis=1) * abi.APPLY_DIVERGED | gp.any(axis=1) * abi.APPLY_GAPPED
    g = np.nonzero(((flags & select) != 0) & (np.arange(G) >= first_group))[0]
    hits = np.zeros(len(g), abi.APPLY_HIT)
    d = div[g].any(axis=1)
    a = np.where(d, div[g].argmax(axis=1), gp[g].argmax(axis=1))
    w = rec[g, a]
    hits["group"] = group_base + g
    hits["local"] = g
    hits["a"] = a
    hits["b"] = np.where(d, w["div_peer"], NO_PEER)
    hits["flags"] = flags[g]
    hits["fault"] = np.asarray(fault)[g]
    hits["index"] = np.where(d, w["div_index"], w["base"])
    hits["gaps"] = np.where(fed[g], rec["gaps"][g].astype(np.int64), 0).sum(axis=1)
    matched = len(hits)
    written = matched if cap is None else min(int(cap), matched)
    nxt = G if written == matched else (first_group if written == 0 else int(hits["local"][written - 1]) + 1)
    return hits[:written], dict(matched=matched, written=written, next_group=int(nxt))
