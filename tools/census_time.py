#!/usr/bin/env python3
"""Wall time of the view census (swim_view_census) on the C3 workload as bench.py builds it: 100 000 members, full views,
preconverged, default ClusterConfig, after 5 periods. Per line one warm-up call, then 7 repeats timed between swim_sync
barriers; min and median, and bytes_read / time in TB/s beside the streaming ceiling DESIGN.md uses for k_sync_diff.

  (a) full census, 8-bit shadow plane            (b) counts only (key_min / key_max null)
  (c) the same two on the u32 key plane (SWIM_NO_K8=1, a fresh child process)
  (d) the older route: row() of 512 evenly spaced observers on the same handle, as measured, and x N/512 (an
      extrapolation to every observer, labelled as such)

Writes one JSON line to profiles/census_c3_100k.json (--out) and prints it. No pass / fail threshold.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scalecube-cluster_amd"))

STREAM_TBPS = 6.29  # the measured streaming ceiling DESIGN.md quotes for k_sync_diff
REPEATS = 7


def timed(c, fn):
    fn()  # warm-up
    ts = []
    for _ in range(REPEATS):
        c.sync()
        t0 = time.perf_counter()
        out = fn()
        c.sync()
        ts.append(time.perf_counter() - t0)
    return out, ts


def census_lines(c):
    lines = {}
    for name, kw in (("full", {}), ("counts_only", {"keys": False})):
        got, ts = timed(c, lambda: c.census(**kw))
        tmin, tmed = min(ts), statistics.median(ts)
        lines[name] = {"path": got.path, "n_observers": got.n_observers, "bytes_read": got.bytes_read,
                       "ms_min": tmin * 1e3, "ms_median": tmed * 1e3, "tbps_at_min": got.bytes_read / tmin / 1e12,
                       "tbps_at_median": got.bytes_read / tmed / 1e12,
                       "frac_of_stream_ceiling_at_median": got.bytes_read / tmed / 1e12 / STREAM_TBPS,
                       "records": [int(x) for x in got.records]}
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=100_000)
    ap.add_argument("--periods", type=int, default=5)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "census_c3_100k.json"))
    ap.add_argument("--leg", choices=["all", "key32"], default="all")
    a = ap.parse_args()
    import swimhip
    from swimhip import SimConfig

    c = swimhip.cluster(SimConfig(n_members=a.members, device=0, profile=True))
    c.run_periods(a.periods)
    c.sync()
    lines = census_lines(c)
    if a.leg == "key32":  # the child: its lines on stdout for the parent
        print(json.dumps(lines))
        return
    n = a.members
    obs = [i * n // a.rows for i in range(a.rows)]
    _, ts = timed(c, lambda: [c.row(o) for o in obs])
    tmed = statistics.median(ts)
    rows = {"observers": a.rows, "ms_min": min(ts) * 1e3, "ms_median": tmed * 1e3,
            "extrapolated_all_observers_s": tmed * n / a.rows,
            "extrapolation": f"median x {n}/{a.rows}: not measured"}
    c.close()
    env = dict(os.environ, SWIM_NO_K8="1")
    child = subprocess.run([sys.executable, __file__, "--leg", "key32", "--members", str(n), "--periods", str(a.periods)],
                           env=env, check=True, capture_output=True, text=True)
    key32 = json.loads(child.stdout.strip().splitlines()[-1])
    line = {"tool": "tools/census_time.py", "workload": f"C3: {n} members, full views, preconverged, {a.periods} periods",
            "repeats": REPEATS, "stream_ceiling_tbps": STREAM_TBPS, "key8": lines, "key32": key32, "read_row": rows}
    text = json.dumps(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
