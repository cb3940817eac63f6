#!/usr/bin/env python3
"""Wall time of a recording on a subject watch (swim_watch_record: a sample queued behind every tick inside swim_step,
speculative batches included) on the C3 workload as bench.py builds it: 100 000 members, full views, preconverged,
default ClusterConfig.

(a) The steady cluster, after 5 periods and one untimed call: the state in which swim_step runs elided, lister-free
speculative batches (each timed call's lister_free_ticks and diff_elided deltas are in the output, so the regime is on
record). A handle of this size takes about 206 GB, so two cannot live side by side on one GPU; in a steady cluster
every tick costs the same, so the pair is the same handle in alternating calls. Each repeat is a pair of
swim_step(2000) calls, one bare and one with the configuration under test, the order swapped from repeat to repeat,
five repeats per configuration; a repeat's cost is the recording call's wall time minus the bare call's, per tick.

  none          no watch in either call (what two calls differ by on their own)
  k1_every1     K = 1, a sample every tick
  k16_every1    K = 16 evenly spaced subjects, every tick
  k16_every10   K = 16, every tenth tick
  k256_every10  K = 256, every tenth tick
  run_until     for comparison the host loop: swim_run_until(check_every = 1) over as many ticks, on a condition that
                is never met (a sample and a host wait after every tick)

Every recorded series is read back after its repeat (outside the timed part) and must be complete.

(b) The curve: one swim_kill, a K = 1 recording of every tick, swim_run_until_recorded(GONE) in calls of 64 ticks
(each call's wall time and gossip creations are kept). Once the
killed member is detected the gossip plane runs and the host looks after every tick (no batches): this part says what
the answer costs there, beside DESIGN.md §3.7's figures for the swim_run_until host loop over the same stretch. It stops
at --curve-ticks, before every member's suspicion timeout spreads a gossip of its own.

Writes one JSON line to profiles/watch_series_c3_100k.json (--out) and prints it; progress goes to stderr."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scalecube-cluster_amd"))


def wall(c, fn):
    c.sync()
    t0 = time.perf_counter()
    fn()
    c.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=100_000)
    ap.add_argument("--periods", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--curve-ticks", type=int, default=1200)
    ap.add_argument("--configs", default="", help="(a): only these, comma-separated (for a kernel trace of one)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "watch_series_c3_100k.json"))
    a = ap.parse_args()
    import swimhip
    from swimhip import SimConfig, _abi

    n, ticks = a.members, a.ticks
    victim = n // 3
    cfg = SimConfig(n_members=n, device=0)
    t00 = time.perf_counter()

    def note(what):  # progress on stderr: a run of this size is quiet for minutes otherwise
        print(f"[{time.perf_counter() - t00:7.1f} s] {what}", file=sys.stderr, flush=True)

    c = swimhip.cluster(cfg)
    note("created")
    for _ in range(a.periods):  # (a call each: the lister-free mode is entered between two batches)
        c.run_periods(1)
    c.step(ticks)
    c.sync()
    note(f"{a.periods} periods and {ticks} untimed ticks")

    def regime():
        d = _abi.debug_diff_dirty(c.lib, c._h)
        return {k: d[k] for k in ("lister_free_ticks", "diff_elided", "diff_halts")}

    def spaced(k):
        return [i * n // k + n // (2 * k) for i in range(k)]

    configs = [("none", None, 0), ("k1_every1", [victim], 1), ("k16_every1", spaced(16), 1),
               ("k16_every10", spaced(16), 10), ("k256_every10", spaced(256), 10), ("run_until", [n // 2], 0)]
    if a.configs:
        configs = [x for x in configs if x[0] in a.configs.split(",")]
    out = {}
    for name, subjects, every in configs:
        w = c.watch(subjects) if subjects else None
        tb, tw, entries = [], [], 0
        r0 = regime()
        for r in range(a.repeats):
            def run():
                if every:
                    w.record(every=every, cap=ticks // every + 1)  # (takes the first sample and waits: not timed)
                if name == "run_until":
                    t = wall(c, lambda: c.run_until(w, _abi.UNTIL_GONE, ticks, 1))
                else:
                    t = wall(c, lambda: c.step(ticks))
                if every:
                    s = w.series()
                    assert len(s) == ticks // every + 1 and s.ticks[-1] == c.tick, (len(s), s.ticks[-1:], c.tick)
                    w.stop()
                    return t, len(s)
                return t, 0

            first = c.tick
            for which in ("bw" if r % 2 == 0 else "wb"):
                if which == "b":
                    tb.append(wall(c, lambda: c.step(ticks)))
                else:
                    t, got = run()
                    tw.append(t)
                    entries += got
            assert c.tick == first + 2 * ticks, (c.tick, first)
            note(f"{name} repeat {r}: bare {tb[-1] * 1e6 / ticks:.2f} watched {tw[-1] * 1e6 / ticks:.2f} us/tick")
        if w is not None:
            w.close()
        over = [(x - y) * 1e6 / ticks for x, y in zip(tw, tb)]
        r1 = regime()
        out[name] = {"k": len(subjects) if subjects else 0, "every": every, "entries_read": entries,
                     "ticks_run": 2 * a.repeats * ticks, "regime_delta": {k: r1[k] - r0[k] for k in r1},
                     "bare_us_per_tick": [t * 1e6 / ticks for t in tb],
                     "watched_us_per_tick": [t * 1e6 / ticks for t in tw],
                     "over_bare_us_per_tick_min": min(over), "over_bare_us_per_tick_median": statistics.median(over),
                     "over_bare_us_per_sample_median": statistics.median(over) * (every or 1)}
        print(f"{name}: bare {statistics.median(tb) * 1e6 / ticks:.2f} us/tick, watched "
              f"{statistics.median(tw) * 1e6 / ticks:.2f} us/tick, over {statistics.median(over):+.2f} us/tick", flush=True)
    # (b)
    c.kill(victim)
    w = c.watch([victim])
    w.record(every=1, cap=a.curve_ticks + 1)
    start, g0 = c.tick, c.counters()["gossips_created"]
    # a call per chunk, so that each chunk's wall time and gossip creations are on record
    met, met_tick, ran, t, chunks = False, 0, 0, 0.0, []
    while not met and ran < a.curve_ticks:
        res, g1 = [], c.counters()["gossips_created"]
        dt = wall(c, lambda: res.append(c.run_until_recorded(w, _abi.UNTIL_GONE, min(64, a.curve_ticks - ran), 64)))
        met, met_tick, did = res[0]
        chunks.append({"ticks": did, "ms_per_tick": dt * 1e3 / max(did, 1),
                       "gossips_created": c.counters()["gossips_created"] - g1})
        ran += did
        t += dt
    s = w.series()
    gone = w.stamps()["gone"][0]
    seen = gone[gone != _abi.WATCH_NEVER]
    curve = {"cond": "GONE", "chunk": 64, "max_ticks": a.curve_ticks, "met": met, "met_after_ticks": met_tick - start if met else None,
             "ticks_run": ran, "wall_ms": t * 1e3, "ms_per_tick": t * 1e3 / max(ran, 1), "entries": len(s),
             "first_not_alive_after_ticks": int(np.argmax(s.counts[:, 0, 1] < s.n_observers)) if len(s) else None,
             "first_gone_tick_after": int(seen.min()) - start if len(seen) else None,
             "last_gone_tick_after": int(seen.max()) - start if len(seen) else None,
             "gossips_created": c.counters()["gossips_created"] - g0, "chunks": chunks}
    note(f"curve: {dict(curve, chunks=[(x['ticks'], round(x['ms_per_tick'], 2), x['gossips_created']) for x in chunks])}")
    tick = c.tick
    c.close()
    line = {"tool": "tools/watch_series_time.py",
            "workload": f"C3: {n} members, full views, preconverged, {a.periods} periods and {ticks} untimed ticks", "ticks_per_call": ticks,
            "repeats": a.repeats, "final_tick": tick, "configs": out, "curve": curve}
    text = json.dumps(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
