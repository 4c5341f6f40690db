"""The group audit (raft_group_audit) restated in numpy over a canonical view.

Written from the rules of include/raftstep.h ("group audit"), not from the
kernels. For replica r of a group, K = ring depth:
  top_r = max(hwm_r, last_r), lo_r = max(1, top_r - K + 1); the live indices
  are lo_r .. last_r; index i sits in slot (i - 1) mod K of the view's log
  rows; the common window of a pair a < b is max(lo) .. min(last); entries are
  equal when term and value are (stamps are not compared).
  TWO_LEADERS        a < b both Leader with equal Term        (a, b, that Term)
  LOG_MATCHING       a pair's smallest unequal index <= its largest index with
                     equal terms                              (a, b, smallest unequal index)
  COMMIT_DIVERGED    a pair's smallest unequal index <= min(commit_a, commit_b)
                                                              (a, b, that index)
  TERM_ORDER         a live i > lo_r with log_term[i] < log_term[i-1], or
                     log_term[last_r] > term_r, window not empty
                                                              (r, 0xFF, smallest such i, else last_r)
  STAMP              payload_crc: a live entry's stamp != CRC32C(term 4 B LE ||
                     value 8 B LE)                            (r, 0xFF, smallest index)
  COMMIT_BEYOND_LOG  commit_r > last_r                        (r, 0xFF, commit_r)
Pairs and replicas: the lexicographically smallest that violates. A hit's
witness is that of its lowest violated check among those asked for. Paging
(cap, matched, written, next_group) is the scan's (tests/groups_model.py).
"""
import numpy as np

from raftstep import abi

TWO_LEADERS, LOG_MATCHING, COMMIT_DIVERGED, TERM_ORDER, STAMP, COMMIT_BEYOND_LOG = (1 << k for k in range(6))
ALL = 63
NONE = abi.NO_REPLICA
BIG = np.int64(1) << 40   # above every index


def _crc_table():
    t = np.zeros(256, np.uint32)
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 & -(c & 1))
        t[n] = c
    return t


_T = _crc_table()


def entry_crcs(term, value):
    """CRC32C(term as 4 B LE || value as 8 B LE) of arrays of entries (bytewise, reflected 0x82F63B78)."""
    term = np.ascontiguousarray(term, np.int64).view(np.uint64) & np.uint64(0xFFFFFFFF)
    value = np.ascontiguousarray(value, np.int64).view(np.uint64)
    c = np.full(term.shape, 0xFFFFFFFF, np.uint32)
    for word, n in ((term, 4), (value, 8)):
        for k in range(n):
            byte = ((word >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(np.uint32)
            c = _T[(c ^ byte) & np.uint32(0xFF)] ^ (c >> np.uint32(8))
    return c ^ np.uint32(0xFFFFFFFF)


def evaluate(state, payload_crc=False):
    """Per group and check k (bit 1 << k): viol[G, 6] bool and the witness
    wit[G, 6, 3] = (a, b, index) where violated."""
    role, term = np.asarray(state["role"]), np.asarray(state["term"]).astype(np.int64)
    last, commit = np.asarray(state["last"]).astype(np.int64), np.asarray(state["commit"]).astype(np.int64)
    lt, lv = np.asarray(state["log_term"]).astype(np.int64), np.asarray(state["log_value"])
    G, R, K = lt.shape
    hwm = np.asarray(state["hwm"]).astype(np.int64) if state.get("hwm") is not None else last
    top = np.maximum(hwm, last)
    lo = np.maximum(1, top - K + 1)
    s = np.arange(K, dtype=np.int64)[None, None, :]
    idx = last[:, :, None] - ((last[:, :, None] - 1 - s) % K)      # the index slot s holds (the largest <= last)
    live = (idx >= lo[:, :, None]) & (idx >= 1) & (last[:, :, None] >= 1)
    viol = np.zeros((G, 6), bool)
    wit = np.zeros((G, 6, 3), np.int64)

    def put(k, m, a, b, index):
        """Groups m not yet violating check k get the witness (a, b, index)."""
        m = m & ~viol[:, k]
        viol[m, k] = True
        wit[m, k, 0], wit[m, k, 1] = a, b
        wit[m, k, 2] = index[m]

    for a in range(R):
        for b in range(a + 1, R):
            put(0, (role[:, a] == abi.LEADER) & (role[:, b] == abi.LEADER) & (term[:, a] == term[:, b]), a, b, term[:, a])
            common = live[:, a] & live[:, b] & (idx[:, a] == idx[:, b])
            uneq = common & ((lt[:, a] != lt[:, b]) | (lv[:, a] != lv[:, b]))
            eqt = common & (lt[:, a] == lt[:, b])
            u = np.where(uneq, idx[:, a], BIG).min(axis=1)          # smallest unequal index (BIG: none)
            e = np.where(eqt, idx[:, a], -1).max(axis=1)            # largest index with equal terms (-1: none)
            put(1, (u < BIG) & (u <= e), a, b, u)
            put(2, (u < BIG) & (u <= np.minimum(commit[:, a], commit[:, b])), a, b, u)
    crc = entry_crcs(lt, lv) if payload_crc else None
    for r in range(R):
        prev_t, prev_i = np.roll(lt[:, r], 1, axis=1), np.roll(idx[:, r], 1, axis=1)
        desc = live[:, r] & (idx[:, r] > lo[:, r, None]) & (lt[:, r] < prev_t)
        assert (prev_i[desc] == idx[:, r][desc] - 1).all()
        d = np.where(desc, idx[:, r], BIG).min(axis=1)
        nonempty = last[:, r] >= lo[:, r]
        t_last = lt[np.arange(G), r, (np.maximum(last[:, r], 1) - 1) % K]
        above = nonempty & (t_last > term[:, r])
        put(3, (d < BIG) | above, r, NONE, np.where(d < BIG, d, last[:, r]))
        if payload_crc:
            bad = live[:, r] & (crc[:, r] != np.asarray(state["log_crc"])[:, r])
            i = np.where(bad, idx[:, r], BIG).min(axis=1)
            put(4, i < BIG, r, NONE, i)
        put(5, commit[:, r] > last[:, r], r, NONE, commit[:, r])
    return viol, wit


def audit(state, checks=ALL, first_group=0, cap=None, group_base=0, payload_crc=False, table=None):
    """(hits as abi.AUDIT_HIT, info dict) of one raft_group_audit call.
    table: evaluate()'s result for this state (computed once, shared)."""
    fault = np.asarray(state["fault"])
    G = len(fault)
    assert checks and not checks & ~ALL and 0 <= first_group <= G
    viol, wit = table if table is not None else evaluate(state, payload_crc)
    asked = np.array([(checks >> k) & 1 for k in range(6)], bool)
    v = viol & asked[None, :]
    v[:first_group] = False
    mask = (v * (1 << np.arange(6))[None, :]).sum(axis=1)
    g = np.nonzero(mask)[0]
    matched = len(g)
    written = matched if cap is None else min(int(cap), matched)
    g = g[:written]
    low = v[g].argmax(axis=1)
    out = np.zeros(written, abi.AUDIT_HIT)
    out["group"] = group_base + g
    out["local"] = g
    out["violated"] = mask[g]
    out["fault"] = fault[g]
    out["a"], out["b"] = wit[g, low, 0], wit[g, low, 1]
    out["index"] = wit[g, low, 2]
    out["check"] = 1 << low
    nxt = G if written == matched else (int(g[-1]) + 1 if written else first_group)
    per = {name: int(v[:, k].sum()) for k, name in enumerate(abi.AUDIT_NAMES)}
    return out, dict(matched=matched, written=written, next_group=nxt, per_check=per)
