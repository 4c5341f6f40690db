"""Idle time between consecutive tick_lean_kernel dispatches of one queue in a
rocprofv3 --kernel-trace CSV, over the last N ticks' dispatches (the bench's
timed call), set against the span of those dispatches.

    python tools/stream_gaps.py TRACE.csv --ticks N [--launches-per-tick L] [--out F]

Per queue: dispatches, kernel time (median, mean), idle between a dispatch's
end and the next one's start on that queue (median, mean, p90; negative when
they overlap), start-to-start period. Over all queues: the window's span per
tick and the sum of kernel times per tick. A queue whose idle time is about
the period minus the kernel time is waiting for its next launch to arrive
(the host, or the packet processor), not for the kernel before it."""
import argparse
import csv
import json
import statistics
from collections import defaultdict


def stats(v):
    v = sorted(v)
    return {"median": statistics.median(v), "mean": sum(v) / len(v), "p90": v[int(0.9 * (len(v) - 1))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--ticks", type=int, required=True)
    ap.add_argument("--launches-per-tick", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [r for r in csv.DictReader(open(a.trace)) if "tick_lean_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    win = rows[-a.ticks * a.launches_per_tick:]
    t0 = min(int(r["Start_Timestamp"]) for r in win)
    t1 = max(int(r["End_Timestamp"]) for r in win)
    per = defaultdict(list)
    for r in win:
        per[r.get("Queue_Id", "0")].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {"ticks": a.ticks, "launches_per_tick": a.launches_per_tick,
           "kernel": win[-1]["Kernel_Name"].split("(")[0],
           "span_us_per_tick": (t1 - t0) / 1e3 / a.ticks,
           "kernel_us_per_tick": sum(e - s for v in per.values() for s, e in v) / 1e3 / a.ticks, "queues": {}}
    for q, v in sorted(per.items()):
        if len(v) < 3:
            continue
        out["queues"][q] = {
            "dispatches": len(v),
            "kernel_us": stats([(e - s) / 1e3 for s, e in v]),
            "idle_us": stats([(b[0] - x[1]) / 1e3 for x, b in zip(v, v[1:])]),
            "period_us": stats([(b[0] - x[0]) / 1e3 for x, b in zip(v, v[1:])]),
        }
    s = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(s + "\n")
    print(s)


if __name__ == "__main__":
    main()
