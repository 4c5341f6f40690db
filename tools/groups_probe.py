"""Group-directory measurement under REF new-node churn (bench.WORKLOADS["C4REF"]
at 2^20 groups, R=7, K=128): the engine runs from init_new_nodes until about a
tenth of its groups are frozen, then, as medians with the spread,
  - the wall time of raft_group_scan (FAULTED, every hit into a buffer touched
    before) and, in a run of its own (RAFTSTEP_GROUPS_TIME=1: the events cost a
    synchronise), the spans of its three launches between HIP events,
  - raft_store_groups of every hit with logs, alternating with raft_store_state
    (the only other way to see scattered groups),
  - raft_store_groups of 4096 random ids, alternating with
    raft_store_state_range(0, 4096) (the cheapest other way to that many groups),
  - raft_state_digest with the per-group digests (the third reader of the
    canonical view, csrc/canon_view.hpp),
  - raft_restart_groups of every hit and the first raft_tick call after it
    (repeats restart the same groups again: the same work),
  - raft_load_groups of every hit (the rows raft_store_groups just returned,
    back into their groups) and of 4096 random distinct ids, each beside
    raft_store_groups of the same ids (the C calls, arrays reused), and raft_load_state
    of the full view with the child's peak resident set beside it (--full-view
    c2: that line on a C2 engine, R=5 K=32, where host memory does not hold the
    R=7 K=128 view; a library without raft_load_groups gives the last line only).
Every GPU step is a child process under its own time limit; one JSON line.
    python tools/groups_probe.py [--reps 10] [--full-stores 3] [--groups N] [--only load] [--full-view c2]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raft-sample_amd")]
STEP_LIMIT_S = 420
TICK_LIMIT = 480


def spread(xs, nd=1):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], nd), min=round(xs[0], nd), max=round(xs[-1], nd), n=len(xs))


def engine(groups):
    """A C4REF engine run until a tenth of its groups are frozen: (engine, next tick, frozen groups)."""
    import bench
    from raftstep import Engine, abi
    wl = bench.WORKLOADS["C4REF"]
    e = Engine(**bench.engine_kwargs(wl, 7, groups, 0, 128, wl["entries"], wl["crc"]))
    e.init_new_nodes(0)
    t, info = 0, abi.ScanInfo()
    while t < TICK_LIMIT:
        e.tick(t, 8, stats=False)
        t += 8
        assert e.lib.raft_group_scan(e.h, abi.SELECT_FAULTED, 0, None, 0, C.byref(info)) == 0
        if info.matched * 10 >= groups:
            break
    return e, t, int(info.matched)


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def child_scan(groups, reps):
    import numpy as np
    from raftstep import abi
    e, t, frozen = engine(groups)
    out = np.zeros(frozen, abi.GROUP_HIT)
    out["local"] = 1   # (touched: no page faults inside the timed calls)
    info = abi.ScanInfo()
    wall, count = [], []
    for i in range(reps + 2):   # (the first call grows the staging buffer)
        for cap, ts in ((frozen, wall), (0, count)):
            ms = timed(lambda: e.lib.raft_group_scan(e.h, abi.SELECT_FAULTED, 0, out.ctypes.data if cap else None, cap,
                                                     C.byref(info)))
            assert info.matched == frozen and info.written == cap
            if i >= 2:
                ts.append(ms * 1e3)
    print(json.dumps(dict(groups=groups, ticks=t, matched=frozen, scan_wall_us=wall, scan_count_only_wall_us=count,
                          fault_codes=np.bincount(out["fault"], minlength=6).tolist())))


def child_store(groups, reps, full_stores):
    import numpy as np
    e, t, frozen = engine(groups)
    hits, _ = e.group_scan(1)
    ids = hits["local"].astype(np.uint64)
    rnd = np.random.default_rng(1).integers(0, groups, 4096).astype(np.uint64)
    res = dict(groups=groups, ticks=t, matched=frozen, store_groups_hits_ms=[], store_state_ms=[],
               store_groups_4096_ms=[], store_state_range_4096_ms=[])
    e.store_groups(ids[:4096])   # (grows the staging buffer)
    res["state_digest_ms"] = [timed(lambda: e.state_digest()) for _ in range(reps + 1)][1:]
    for i in range(reps):
        res["store_groups_hits_ms"].append(timed(lambda: e.store_groups(ids)))
        if i < full_stores:
            res["store_state_ms"].append(timed(lambda: e.store_state()))
    for i in range(reps):
        res["store_groups_4096_ms"].append(timed(lambda: e.store_groups(rnd)))
        res["store_state_range_4096_ms"].append(timed(lambda: e.store_state_range(0, 4096)))
    R, K = e.cfg.replicas, e.cfg.ring_depth
    res["view_bytes_per_group"] = R * (2 + 4 * 6) + 8 * R * R + 2 + 16 * R * K
    print(json.dumps(res))


def child_restart(groups, reps):
    import numpy as np
    e, t, frozen = engine(groups)
    hits, _ = e.group_scan(1)
    ids = hits["local"].astype(np.uint64)
    tick_before = [timed(lambda: e.tick(t + i, 1, stats=False) or e.sync()) for i in range(3)]
    t += 3
    restart, first_tick = [], []
    for i in range(reps):
        restart.append(timed(lambda: e.restart_groups(ids, t)))
        first_tick.append(timed(lambda: e.tick(t, 1, stats=False) or e.sync()))
        t += 1
    left = e.group_scan(1, cap=0)[1]["matched"]
    print(json.dumps(dict(groups=groups, matched=frozen, restart_ms=restart, first_tick_after_ms=first_tick,
                          tick_before_ms=tick_before, frozen_after=left)))


def child_load(groups, reps):
    """Both directions as wall times of the C calls over arrays made and touched
    before (no allocation, coercion or page fault inside a timed call)."""
    import numpy as np
    from raftstep import abi
    e, t, frozen = engine(groups)
    res = dict(groups=groups, ticks=t, matched=frozen, has_load_groups=hasattr(e.lib, "raft_load_groups"))
    if res["has_load_groups"]:
        hits, _ = e.group_scan(1)
        ids = hits["local"].astype(np.uint64)
        rnd = np.random.default_rng(1).permutation(groups)[:4096].astype(np.uint64)
        before = e.state_digest()[1]
        for key, x in (("hits", ids), ("4096", rnd)):
            rows, back = e.store_groups(x), e.store_groups(x)   # (what is loaded, and where the stores go)
            vr, vb = abi.make_view(rows), abi.make_view(back)
            load = lambda: e.lib.raft_load_groups(e.h, x.ctypes.data, len(x), C.byref(vr))
            store = lambda: e.lib.raft_store_groups(e.h, x.ctypes.data, len(x), C.byref(vb))
            assert load() == 0 and store() == 0   # (grows the staging buffer)
            res[f"load_groups_{key}_ms"] = [timed(load) for _ in range(reps)]
            res[f"store_groups_{key}_ms"] = [timed(store) for _ in range(reps)]
            assert all(back[k].tobytes() == rows[k].tobytes() for k in rows)
        res["digest_kept"] = bool(e.state_digest()[1] == before)   # (the same rows back: the state is as it was)
        R, K = e.cfg.replicas, e.cfg.ring_depth
        res["view_bytes_per_group"] = R * (2 + 4 * 6) + 8 * R * R + 2 + 16 * R * K
    print(json.dumps(res))


def child_loadfull(groups, full_stores, shape):
    import resource
    import bench
    from raftstep import Engine
    if shape == "c2":
        wl = bench.WORKLOADS["C2"]
        e = Engine(**bench.engine_kwargs(wl, 5, groups, 0, wl["ring_depth"], wl["entries"], wl["crc"]))
        e.init_steady(-1, 0)
        e.tick(1, 48, stats=False)
    else:
        e, _, _ = engine(groups)
    want = e.state_digest()[1]
    st = e.store_state()
    view = sum(a.nbytes for a in st.values())
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    ms = [timed(lambda: e.load_state(st)) for _ in range(full_stores)]
    rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    print(json.dumps(dict(groups=groups, shape=shape, replicas=e.cfg.replicas, ring_depth=e.cfg.ring_depth,
                          view_bytes=view, load_state_ms=ms, peak_rss_before_mb=rss0 // 1024,
                          peak_rss_after_mb=rss1 // 1024, digest_kept=bool(e.state_digest()[1] == want))))


def load_lines(common, full_view):
    """The load lines of the result (the keys the earlier lines do not use)."""
    ld, _ = step(common + ["--child", "load"])
    res = dict(has_load_groups=ld["has_load_groups"])
    if ld["has_load_groups"]:
        res.update(load_groups_hits_ms=spread(ld["load_groups_hits_ms"]),
                   load_groups_4096_ms=spread(ld["load_groups_4096_ms"], 2),
                   load_store_groups_hits_ms=spread(ld["store_groups_hits_ms"]),
                   load_store_groups_4096_ms=spread(ld["store_groups_4096_ms"], 2), load_digest_kept=ld["digest_kept"],
                   load_groups_hits=ld["matched"], load_groups_hits_bytes=ld["matched"] * ld["view_bytes_per_group"])
    lf, _ = step(common + ["--child", "loadfull", "--full-view", full_view])
    res.update(load_state_ms=spread(lf["load_state_ms"]), load_state_shape=lf["shape"], load_state_replicas=lf["replicas"],
               load_state_ring_depth=lf["ring_depth"], load_state_view_bytes=lf["view_bytes"],
               load_state_peak_rss_before_mb=lf["peak_rss_before_mb"],
               load_state_peak_rss_after_mb=lf["peak_rss_after_mb"], load_state_digest_kept=lf["digest_kept"])
    return res


def step(args, env=None):
    """One GPU step in a child process of its own, under a time limit."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                       timeout=STEP_LIMIT_S, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise SystemExit(f"step {args} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--full-stores", type=int, default=3, help="raft_store_state calls (seconds each at 2^20 groups)")
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--child", default=None)
    ap.add_argument("--only", default=None, choices=["load"], help="the load lines alone")
    ap.add_argument("--full-view", default="c4ref", choices=["c4ref", "c2"],
                    help="engine of the raft_load_state line: the probe's own, or C2 (R=5, K=32)")
    a = ap.parse_args()
    if a.child == "scan":
        return child_scan(a.groups, a.reps)
    if a.child == "store":
        return child_store(a.groups, a.reps, a.full_stores)
    if a.child == "restart":
        return child_restart(a.groups, a.reps)
    if a.child == "load":
        return child_load(a.groups, a.reps)
    if a.child == "loadfull":
        return child_loadfull(a.groups, a.full_stores, a.full_view)
    common = ["--reps", str(a.reps), "--groups", str(a.groups), "--full-stores", str(a.full_stores)]
    if a.only == "load":
        print(json.dumps(dict(groups=a.groups, **load_lines(common, a.full_view))))
        return
    sc, _ = step(common + ["--child", "scan"])
    _, err = step(common + ["--child", "scan"], env={"RAFTSTEP_GROUPS_TIME": "1"})
    spans = [tuple(float(x) for x in m.groups()) for m in re.finditer(
        r"raft_group_scan: matched \d+ written [1-9]\d* count_us ([\d.]+) scan_us ([\d.]+) emit_us ([\d.]+)", err)][-a.reps:]
    res = dict(groups=sc["groups"], ticks=sc["ticks"], matched=sc["matched"], fault_codes=sc["fault_codes"],
               scan_wall_us=spread(sc["scan_wall_us"]), scan_count_only_wall_us=spread(sc["scan_count_only_wall_us"]),
               count_us=spread([s[0] for s in spans]), scan_us=spread([s[1] for s in spans]),
               emit_us=spread([s[2] for s in spans]))
    st, _ = step(common + ["--child", "store"])
    n, per = st["matched"], st["view_bytes_per_group"]
    res.update(view_bytes_per_group=per, store_groups_hits_bytes=n * per, store_state_bytes=st["groups"] * per,
               store_groups_hits_ms=spread(st["store_groups_hits_ms"]), store_state_ms=spread(st["store_state_ms"]),
               store_groups_4096_ms=spread(st["store_groups_4096_ms"], 2),
               store_state_range_4096_ms=spread(st["store_state_range_4096_ms"], 2),
               state_digest_ms=spread(st["state_digest_ms"], 2))
    rs, _ = step(common + ["--child", "restart"])
    res.update(restart_ms=spread(rs["restart_ms"], 3), first_tick_after_ms=spread(rs["first_tick_after_ms"], 3),
               tick_before_ms=spread(rs["tick_before_ms"], 3), frozen_after_restarts=rs["frozen_after"])
    res.update(load_lines(common, a.full_view))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
