#!/usr/bin/env python3
"""Wall time of the subject watch (swim_watch_sample, swim_run_until) on the C3 workload as bench.py builds it: 100 000
members, full views, preconverged, default ClusterConfig, after 5 periods. Per line one warm-up call, then 7 repeats
timed between swim_sync barriers; min and median. One session (one process):

  (a) one sample of K = 1, 16 and 256 evenly spaced subjects (no two share a cache line: the traffic model's worst case),
      with and without stamps, beside a counts-only swim_view_census on the same handle
  (b) after one swim_kill: run_until(GONE, check_every = 1) on the killed member: the ticks it ran and its wall time,
      beside the wall time of a plain swim_step of that many ticks on a twin handle (created after the first is closed)

Writes one JSON line to profiles/watch_c3_100k.json (--out) and prints it. The one fixed requirement: a K = 16 sample
takes less wall time than the counts-only census measured beside it (exit status 1 otherwise); the ratios are reported.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scalecube-cluster_amd"))

REPEATS = 7
KS = (1, 16, 256)


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


def ms(ts):
    return {"ms_min": min(ts) * 1e3, "ms_median": statistics.median(ts) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=100_000)
    ap.add_argument("--periods", type=int, default=5)
    ap.add_argument("--max-ticks", type=int, default=4000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "watch_c3_100k.json"))
    a = ap.parse_args()
    import swimhip
    from swimhip import SimConfig, _abi

    n = a.members
    cfg = SimConfig(n_members=n, device=0)
    c = swimhip.cluster(cfg)
    c.run_periods(a.periods)
    c.sync()
    cen, ts = timed(c, lambda: c.census(keys=False, by_observer=False))
    census = dict(ms(ts), path=cen.path, n_observers=cen.n_observers, bytes_read=cen.bytes_read)
    samples = {}
    for k in KS:
        subjects = [i * n // k + n // (2 * k) for i in range(k)]
        for stamps in (False, True):
            w = c.watch(subjects, stamps=stamps)
            got, ts = timed(c, w.sample)
            w.close()
            line = dict(ms(ts), k=k, stamps=stamps, n_observers=got.n_observers, path=got.path,
                        lines_requested_model=n * k)
            line["census_over_sample_at_median"] = census["ms_median"] / line["ms_median"]
            samples[f"k{k}_{'stamps' if stamps else 'plain'}"] = line
    # (b)
    victim = n // 3
    c.kill(victim)
    w = c.watch([victim])
    c.sync()
    t0 = time.perf_counter()
    met, ticks = c.run_until(w, _abi.UNTIL_GONE, a.max_ticks, 1)
    c.sync()
    t_until = time.perf_counter() - t0
    last = w.sample()
    gone = w.stamps()["gone"][0]
    seen = gone[gone != _abi.WATCH_NEVER]
    until = {"cond": "GONE", "check_every": 1, "max_ticks": a.max_ticks, "met": met, "ticks_run": ticks,
             "wall_ms": t_until * 1e3, "ms_per_tick": t_until * 1e3 / max(ticks, 1), "tick": last.tick,
             "counts": [int(x) for x in last.counts[0]],
             "first_gone_tick": int(seen.min()) if len(seen) else None,
             "last_gone_tick": int(seen.max()) if len(seen) else None}
    c.close()
    twin = swimhip.cluster(cfg)
    twin.run_periods(a.periods)
    twin.kill(victim)
    twin.sync()
    t0 = time.perf_counter()
    twin.step(ticks)
    twin.sync()
    t_plain = time.perf_counter() - t0
    twin.close()
    until["plain_step_wall_ms"] = t_plain * 1e3
    until["plain_ms_per_tick"] = t_plain * 1e3 / max(ticks, 1)
    until["until_over_plain"] = t_until / t_plain if t_plain else None
    line = {"tool": "tools/watch_time.py", "workload": f"C3: {n} members, full views, preconverged, {a.periods} periods",
            "repeats": REPEATS, "block_rows": _abi.WATCH_BLOCK_ROWS, "census_counts_only": census, "sample": samples,
            "run_until": until}
    text = json.dumps(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
    print(text)
    k16 = max(samples["k16_plain"]["ms_median"], samples["k16_stamps"]["ms_median"])
    if not k16 < census["ms_median"]:
        print(f"FAIL: a K = 16 sample ({k16:.3f} ms) is not faster than the counts-only census "
              f"({census['ms_median']:.3f} ms)", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
