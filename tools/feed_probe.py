"""Commit-feed measurement at the C2 shape (bench.WORKLOADS["C2"]: 2^20 groups,
R=5, E=1, init_steady and a warm-up): per poll after one tick, for a mask of
replica 0 and of all replicas,
  - the wall time of raft_feed_poll (into a buffer allocated and touched before),
  - the spans between HIP events around its launches (RAFTSTEP_FEED_TIME=1:
    count + scan + totals, the emit kernel alone, the copy out), in a run of
    their own (the events cost a synchronise),
  - the device bytes of the two kernel passes and their rate, against
    raft_stream_probe's sustained rate on the same GPU,
and the comparison: raft_store_state_range over all groups with logs, the only
way to these entries without the feed.
Every GPU step is a child process under its own time limit; one JSON line.
    python tools/feed_probe.py [--polls 20] [--groups N]
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
STEP_LIMIT_S = 240


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if xs else None


def engine(groups):
    import bench
    from raftstep import Engine
    wl = bench.WORKLOADS["C2"]
    e = Engine(**bench.engine_kwargs(wl, 5, groups or wl["groups"], 0, wl["ring_depth"], wl["entries"], wl["crc"]))
    e.init_steady(0, 0)
    e.tick(1, 20)
    return e, 21


def child_feed(mask, polls, groups):
    import numpy as np
    from raftstep import abi
    e, t = engine(groups)
    G, nm = e.cfg.groups, bin(mask).count("1")
    e.feed_open(mask, "commit")
    out = np.zeros(2 * G * nm, abi.FEED_ENTRY)
    out["value"] = 1   # (touched: no page faults inside the timed calls)
    info = abi.FeedInfo()
    wall, delivered = [], []
    for i in range(polls + 2):
        e.tick(t, 1)
        t += 1
        t0 = time.perf_counter()
        rc = e.lib.raft_feed_poll(e.h, out.ctypes.data, len(out), C.byref(info))
        dt = time.perf_counter() - t0
        assert rc == 0 and info.pending == 0 and info.lost == 0, (rc, info.pending, info.lost)
        if i >= 2:   # (the first polls grow the staging buffer)
            wall.append(dt * 1e6)
            delivered.append(int(info.delivered))
    print(json.dumps(dict(wall_us=wall, delivered=delivered, groups=G)))


def child_store(groups):
    e, t = engine(groups)
    ts = []
    for _ in range(3):
        e.tick(t, 1)
        t += 1
        t0 = time.perf_counter()
        e.store_state_range(0, e.cfg.groups, logs=True)
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(store_state_range_ms=ts, groups=e.cfg.groups)))


def child_stream(groups):
    from raftstep import engine as eng
    us, by = eng.stream_probe(0, 5, groups or 1 << 20, 20)
    print(json.dumps(dict(stream_probe_us=us, stream_probe_bytes=by, stream_probe_gbs=by / us / 1e3)))


def step(args, env=None):
    """One GPU step in a child process of its own, under a time limit."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                       timeout=STEP_LIMIT_S, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise SystemExit(f"step {args} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--polls", type=int, default=20)
    ap.add_argument("--groups", type=int, default=0, help="0: the C2 workload's")
    ap.add_argument("--child", default=None)
    ap.add_argument("--mask", type=int, default=1)
    a = ap.parse_args()
    if a.child == "feed":
        return child_feed(a.mask, a.polls, a.groups)
    if a.child == "store":
        return child_store(a.groups)
    if a.child == "stream":
        return child_stream(a.groups)
    common = ["--polls", str(a.polls), "--groups", str(a.groups)]
    res = {}
    res.update(step(common + ["--child", "stream"])[0])
    for name, mask in (("replica0", 1), ("all", 31)):
        plain, _ = step(common + ["--child", "feed", "--mask", str(mask)])
        _, err = step(common + ["--child", "feed", "--mask", str(mask)], env={"RAFTSTEP_FEED_TIME": "1"})
        spans = [tuple(float(x) for x in m.groups()) for m in re.finditer(
            r"raft_feed_poll: delivered \d+ count_scan_us ([\d.]+) emit_us ([\d.]+) copy_us ([\d.]+)", err)][-a.polls:]
        G, n = plain["groups"], med(plain["delivered"])
        cs, em, cp = (med([s[i] for s in spans]) for i in range(3))
        dev_bytes = 26 * G + (12 + 32) * n      # gmeta, the gss record, the cursor read and written; per entry 12 + 32
        res[name] = dict(entries_per_poll=n, wall_us_median=round(med(plain["wall_us"]), 1),
                         wall_us_min=round(min(plain["wall_us"]), 1), wall_us_max=round(max(plain["wall_us"]), 1),
                         count_scan_us=cs, emit_us=em, copy_us=cp, copy_gbs=round(32 * n / cp / 1e3, 1),
                         device_bytes=dev_bytes, kernels_gbs=round(dev_bytes / (cs + em) / 1e3, 1),
                         emit_gbs=round(44 * n / em / 1e3, 1))
    st, _ = step(common + ["--child", "store"])
    res["store_state_range_ms_median"] = round(med(st["store_state_range_ms"]), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
