"""Model of the client proposals (raft_propose / raft_ticket_status), written
from the rules in include/raftstep.h ("client proposals"), not from the
kernels.

propose(oracle, ...) drives the CPU oracle through RAFT_OP_CLIENT_APPEND
batches (one per rank of a proposal within its group and leader ordinal, so
that every batch has distinct groups, as the oracle requires) and builds the
tickets from the results. ticket_status(view, cfg, tickets) is plain numpy /
Python over a canonical view (store_state's dict).
"""
import numpy as np

from raftstep import abi

NAMES = abi.TICKET_STATE_NAMES
NONE = 0xFF


def propose(oracle, now_tick, groups, values):
    cfg = oracle.cfg
    groups = np.asarray(groups, dtype=np.uint64)
    values = np.asarray(values).astype(np.int64)
    assert groups.shape == values.shape and groups.ndim == 1
    assert not len(groups) or int(groups.max()) < cfg.groups
    st = oracle.store_state(logs=False)
    role, term = st["role"], st["term"]
    fault = st["fault"].astype(np.int64).copy()
    n = len(groups)
    out = np.zeros(n, abi.TICKET)
    out["group"] = groups + np.uint64(cfg.group_base)
    out["value"] = values
    out["local"] = groups
    out["leader"] = NONE
    # rank of each proposal within its group, in list order
    rank = np.zeros(n, np.int64)
    seen = {}
    for i, g in enumerate(groups.tolist()):
        rank[i] = seen.get(g, 0)
        seen[g] = rank[i] + 1
    leaders_of = {g: [r for r in range(cfg.replicas) if role[g, r] == abi.LEADER] for g in seen}
    for k in range(int(rank.max()) + 1 if n else 0):
        idx = np.flatnonzero(rank == k)
        for j in range(cfg.replicas):   # leader ordinal
            batch = [i for i in idx.tolist() if fault[int(groups[i])] == 0 and len(leaders_of[int(groups[i])]) > j]
            if not batch:
                break
            ops = np.zeros(len(batch), abi.GROUP_OP)
            ops["group"] = groups[batch]
            ops["replica"] = [leaders_of[int(groups[i])][j] for i in batch]
            ops["kind"] = abi.OP_CLIENT_APPEND
            ops["arg"] = values[batch]
            res = oracle.group_ops(now_tick, ops)
            for i, o, rs in zip(batch, ops, res):
                g, r = int(o["group"]), int(o["replica"])
                assert rs["status"] == 0, (i, g, r, rs)
                if rs["fault"]:          # frozen at this append (it was not before): nothing appended
                    fault[g] = int(rs["fault"])
                    continue
                out["leaders"][i] |= 1 << r
                if out["leader"][i] == NONE:
                    out["leader"][i] = r
                    out["index"][i] = int(rs["value"])
                    out["term"][i] = int(term[g, r])
        for i in idx.tolist():
            g = int(groups[i])
            out["fault"][i] = fault[g]
            out["status"][i] = (abi.PROPOSE_ACCEPTED if out["leaders"][i] else
                                abi.PROPOSE_FROZEN if fault[g] else abi.PROPOSE_NO_LEADER)
    return out


def ticket_status(view, cfg, tickets):
    """(TICKET_RESULT array, {state name: count}) of `tickets` over the canonical view `view`."""
    R, K = cfg.replicas, cfg.ring_depth
    raft = cfg.semantics == abi.SEM_RAFT
    tickets = np.asarray(tickets, dtype=abi.TICKET)
    out = np.zeros(len(tickets), abi.TICKET_RESULT)
    for i, t in enumerate(tickets):
        g, index, term, value = int(t["local"]), int(t["index"]), int(t["term"]), int(t["value"])
        assert g < cfg.groups and int(t["group"]) == cfg.group_base + g
        o = out[i]
        o["fault"] = view["fault"][g]
        o["replica"] = NONE
        if t["status"] != abi.PROPOSE_ACCEPTED or index <= 0:
            o["state"] = abi.TICKET_INVALID
            continue
        decided_live, decided_gone, same_r, gone_r = [], [], [], []
        for r in range(R):
            l, cm = int(view["last"][g, r]), int(view["commit"][g, r])
            if index > l:
                continue   # absent
            top = max(int(view["hwm"][g, r]), l) if raft else l
            lo = max(1, top - K + 1)
            decided = index <= min(cm, l)
            if index < lo:
                gone_r.append(r)
                if decided:
                    decided_gone.append(r)
                continue
            s = (index - 1) % K
            same = int(view["log_term"][g, r, s]) == term and int(view["log_value"][g, r, s]) == value
            if same:
                same_r.append(r)
                o["holders"] |= 1 << r
                if decided:
                    o["committed"] |= 1 << r
            if decided:
                decided_live.append((r, same))
        if decided_live:
            r, same = decided_live[0]
            o["state"], o["replica"] = (abi.TICKET_COMMITTED if same else abi.TICKET_SUPERSEDED), r
        elif decided_gone:
            o["state"] = abi.TICKET_EVICTED
        elif same_r:
            o["state"], o["replica"] = abi.TICKET_PENDING, same_r[0]
        elif gone_r:
            o["state"] = abi.TICKET_EVICTED
        else:
            o["state"] = abi.TICKET_DROPPED
    per = {k: int((out["state"] == s).sum()) for s, k in enumerate(NAMES)}
    return out, per


def synthetic_tickets(rng, view, cfg, index=None, ids=None):
    """Tickets that raft_propose could have handed out: for row i of `view`
    (group ids[i], default i) one ticket per index of index[i] ([rows][m]
    int; default 0..14 for every row), (term, value) copied from a random
    replica's slot of that index, the value's low bit flipped for one ticket
    in four. An index <= 0 is the INVALID case."""
    R, K = cfg.replicas, cfg.ring_depth
    rows = view["last"].shape[0]
    ids = np.arange(rows) if ids is None else np.asarray(ids)
    index = np.tile(np.arange(15), (rows, 1)) if index is None else np.asarray(index)
    m = index.shape[1]
    n = rows * m
    t = np.zeros(n, abi.TICKET)
    row = np.repeat(np.arange(rows), m)
    idx = index.reshape(-1).astype(np.int64)
    r = rng.integers(0, R, n)
    s = (idx - 1) % K
    t["local"] = ids[row]
    t["group"] = ids[row] + cfg.group_base
    t["index"] = idx
    t["term"] = view["log_term"][row, r, s]
    t["value"] = view["log_value"][row, r, s] ^ (rng.integers(0, 4, n) == 0)
    t["status"] = abi.PROPOSE_ACCEPTED
    t["leader"] = r
    t["leaders"] = 1 << r
    return t


def tickets_near_last(rng, view, cfg, ids=None, m=6):
    """synthetic_tickets at m random indices per row in last - K - 2 .. last + 2
    of a random replica: live, evicted and absent entries of a ticked state."""
    rows, R = view["last"].shape
    last = view["last"][np.arange(rows), rng.integers(0, R, rows)].astype(np.int64)
    index = last[:, None] + rng.integers(-cfg.ring_depth - 2, 3, (rows, m))
    return synthetic_tickets(rng, view, cfg, np.clip(index, 0, 2**31 - 1), ids)


def coverage_inputs(raft, base=9000):
    """The state and tickets of the status tests (CPU coverage and GPU):
    harness.random_state(default_rng(11), 64, 3, 8), RAFT with hwm = last +
    0..3, and one synthetic ticket per group and index 0..14."""
    import harness as H
    rng = np.random.default_rng(11)
    st = H.random_state(rng, 64, 3, 8)
    st["hwm"][:] = st["last"] + (rng.integers(0, 4, st["last"].shape) if raft else 0)
    cfg = abi.default_config(replicas=3, groups=64, ring_depth=8, semantics=int(raft), group_base=base)
    return st, cfg, synthetic_tickets(np.random.default_rng(12), st, cfg)
