"""Group-audit measurement on the directory probe's state (tools/groups_probe.py:
bench.WORKLOADS["C4REF"] at 2^20 groups, R=7, K=128, run from init_new_nodes
until a tenth of the groups are frozen, tick 48). Medians with the spread of
  - the wall time of raft_group_audit(ALL), every hit into a buffer touched
    before, and of the scalar-only audit (TWO_LEADERS | COMMIT_BEYOND_LOG)
    beside the count-only raft_group_scan of the same session,
  - in a run of its own (RAFTSTEP_AUDIT_TIME=1, RAFTSTEP_GROUPS_TIME=1: the
    events cost a synchronise) the spans of the audit's launches between HIP
    events, raft_store_state's wall time (the only other way to the same
    answer, before any host check) with the event time of its gather kernels,
    and the gather's log kernel alone (a store of the log rows only),
  - the bytes the rules make the audit read: the record words plus 12 B per
    live entry (16 B with stamps), and the rate the log kernel reaches on them.
Every GPU step is a child process under its own time limit; one JSON line.
    python tools/audit_probe.py [--reps 10] [--full-stores 2] [--groups N]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raft-sample_amd"), os.path.join(ROOT, "tools")]
import groups_probe as GP  # noqa: E402  (the engine, timed, spread)


def step(args, env=None):
    """One GPU step in a child process of its own, under a time limit."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                       timeout=GP.STEP_LIMIT_S, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise SystemExit(f"step {args} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def child_wall(groups, reps):
    import numpy as np
    from raftstep import abi
    e, t, frozen = GP.engine(groups)
    info, sinfo = abi.AuditInfo(), abi.ScanInfo()
    scalar = abi.AUDIT_TWO_LEADERS | abi.AUDIT_COMMIT_BEYOND_LOG
    assert e.lib.raft_group_audit(e.h, abi.AUDIT_ALL, 0, None, 0, C.byref(info)) == 0
    matched = int(info.matched)
    out = np.zeros(max(matched, 1), abi.AUDIT_HIT)
    out["local"] = 1   # (touched: no page faults inside the timed calls)
    res = dict(all_wall_us=[], all_count_only_wall_us=[], scalar_wall_us=[], scan_count_only_wall_us=[])
    for i in range(reps + 2):   # (the first calls grow the staging buffer)
        for key, f in (
                ("all_wall_us", lambda: e.lib.raft_group_audit(e.h, abi.AUDIT_ALL, 0, out.ctypes.data, matched, C.byref(info))),
                ("all_count_only_wall_us", lambda: e.lib.raft_group_audit(e.h, abi.AUDIT_ALL, 0, None, 0, C.byref(info))),
                ("scalar_wall_us", lambda: e.lib.raft_group_audit(e.h, scalar, 0, None, 0, C.byref(info))),
                ("scan_count_only_wall_us", lambda: e.lib.raft_group_scan(e.h, abi.SELECT_FAULTED, 0, None, 0, C.byref(sinfo)))):
            ms = GP.timed(f)
            if i >= 2:
                res[key].append(ms * 1e3)
    hits, ainfo = e.group_audit()
    st = e.store_state(logs=False)
    R, K = e.cfg.replicas, e.cfg.ring_depth
    top = np.maximum(st["hwm"], st["last"]).astype(np.int64)
    live = np.clip(st["last"] - np.maximum(1, top - K + 1) + 1, 0, None).sum()
    per_entry = 16 if e.cfg.payload_crc else 12
    words = 4 * (2 + 4 * R) + 20   # gmeta, the fault's word, R x (rs, term, last, commit) and the ring form's five words
    print(json.dumps(dict(groups=groups, ticks=t, frozen=frozen, matched=matched, per_check=ainfo["per_check"],
                          hit_faults=np.bincount(hits["fault"], minlength=6).tolist(), live_entries=int(live),
                          bytes_per_group_rules=round(words + per_entry * live / groups, 1),
                          bytes_rules=int(words * groups + per_entry * live), **res)))


def child_events(groups, reps, full_stores):
    import numpy as np
    from raftstep import abi
    e, t, frozen = GP.engine(groups)
    info = abi.AuditInfo()
    scalar = abi.AUDIT_TWO_LEADERS | abi.AUDIT_COMMIT_BEYOND_LOG
    for i in range(reps + 2):
        assert e.lib.raft_group_audit(e.h, abi.AUDIT_ALL, 0, None, 0, C.byref(info)) == 0
        assert e.lib.raft_group_audit(e.h, scalar, 0, None, 0, C.byref(info)) == 0
    R, K = e.cfg.replicas, e.cfg.ring_depth
    logs = dict(log_term=np.zeros((groups, R, K), np.int32), log_value=np.zeros((groups, R, K), np.int64))
    v = abi.make_view(logs)
    log_store = [GP.timed(lambda: e.lib.raft_store_state(e.h, C.byref(v))) for _ in range(full_stores + 1)][1:]
    del logs, v
    store = [GP.timed(lambda: e.store_state()) for _ in range(full_stores)]
    print(json.dumps(dict(groups=groups, ticks=t, store_state_ms=store, store_state_log_rows_only_ms=log_store)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--full-stores", type=int, default=2, help="raft_store_state calls (seconds each at 2^20 groups)")
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "wall":
        return child_wall(a.groups, a.reps)
    if a.child == "events":
        return child_events(a.groups, a.reps, a.full_stores)
    common = ["--reps", str(a.reps), "--groups", str(a.groups), "--full-stores", str(a.full_stores)]
    w, _ = step(common + ["--child", "wall"])
    res = {k: (GP.spread(v) if k.endswith("_us") else v) for k, v in w.items()}
    ev, err = step(common + ["--child", "events"], env={"RAFTSTEP_AUDIT_TIME": "1", "RAFTSTEP_GROUPS_TIME": "1"})
    spans = {}
    for m in re.finditer(r"raft_group_audit: checks (\d+) matched \d+ written \d+ scalar_us ([\d.]+) log_us ([\d.]+) "
                         r"count_scan_us ([\d.]+)", err):
        spans.setdefault(int(m.group(1)), []).append(tuple(float(x) for x in m.groups()[1:]))
    for checks, name in ((63, "all"), (33, "scalar")):
        s = spans.get(checks, [])[-a.reps:]
        for k, key in enumerate(("scalar_kernel_us", "log_kernel_us", "count_scan_us")):
            res[f"{name}_{key}"] = GP.spread([x[k] for x in s])
    gk = [(int(m.group(1)), float(m.group(2))) for m in re.finditer(
        r"gather_view: groups \d+ chunks \d+ logs (\d) kernels_us ([\d.]+)", err)]
    n = a.full_stores
    res.update(store_state_ms=GP.spread(ev["store_state_ms"]),
               store_state_log_rows_only_ms=GP.spread(ev["store_state_log_rows_only_ms"]),
               gather_log_kernel_us=GP.spread([us for _, us in gk[1:n + 1]]),
               gather_kernels_us=GP.spread([us for _, us in gk[n + 1:2 * n + 1]]))
    res["log_kernel_gb_per_s"] = round(res["bytes_rules"] / res["all_log_kernel_us"]["median"] / 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
