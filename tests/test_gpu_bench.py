"""GPU: bench.py's own command line. A plain run prints the headline only
(nothing that --full adds), times exactly --steps ticks, and --dump-outputs
writes what the last timed call returned and left in the engine: the dumped
statistics equal the line's, and the dumped state slice and digests equal an
oracle run over the same groups through the same ticks (init_steady, then
warm-up + steps ticks from tick 1, as bench.measure drives the engine)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle
from raftstep import STAT_NAMES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, STEPS, WARMUP = 5000, 7, 3   # no multiple of the 256-group blocks; more than one block


def _whole(halves):
    return (halves[..., 0].astype(np.uint64) << np.uint64(32)) | halves[..., 1].astype(np.uint64)


def test_plain_run_is_the_headline_only_and_dumps_its_last_step(tmp_path):
    d = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--groups-per-gpu", str(G), "--dump-outputs", d],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == STEPS and line["full"] is False and line["stats_check"] is True
    assert line["timing"]["repeats"] == 1
    assert line["value"] == pytest.approx(G * 1e3 / line["ms_per_step"])
    # exactly STEPS timed ticks: one entry committed per group and tick
    assert line["stats"]["committed"] == G * STEPS
    for k in ("fused", "extra_workloads", "list_kernel", "oracle_slice_check", "roofline_frac", "cpu_baseline_value"):
        assert k not in line
    assert line["cpu_baseline"] is None
    assert "avg_kernel_us" not in line["roofline"] and "stream_probe" not in line["roofline"]

    out = {os.path.basename(p)[:-4]: np.load(p) for p in glob.glob(os.path.join(d, "*.npy"))}
    assert all(a.dtype == np.float64 for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert [int(x) for x in out["stats"]] == [line["stats"][k] for k in STAT_NAMES]
    assert out["last_step_stats"][STAT_NAMES.index("committed")] == G

    wl = bench.WORKLOADS["C2"]
    first, n = (int(x) for x in out["slice_groups"])
    assert 0 <= first and first + n <= G and n >= 1
    o = oracle.Oracle(**bench.engine_kwargs(wl, bench.R_DEFAULT, G, 0, wl["ring_depth"], wl["entries"], wl["crc"]))
    o.init_steady(0, 0)
    o.tick(1, WARMUP + STEPS)
    dig, _ = o.state_digest()
    st = o.store_state()
    o.close()
    ids = out["digest_groups"].astype(np.int64)
    assert np.array_equal(ids, np.arange(G))
    assert np.array_equal(_whole(out["state_digest"]), dig[ids])
    assert set(out) == {"stats", "last_step_stats", "digest_groups", "state_digest", "slice_groups"} | \
        {"state_" + k for k in st}
    for k, a in st.items():
        got = out["state_" + k]
        want = a[first:first + n]
        if a.dtype.itemsize == 8:
            assert np.array_equal(_whole(got), want.astype(np.uint64)), k
        else:
            assert np.array_equal(got, want.astype(np.float64)), k
