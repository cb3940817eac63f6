"""Ticks without a lister launch on one GPU ("Lister-free batches"): in a cluster whose rows all equal
the baseline, whose write logs are empty and whose payloads are all undelayed live rows, k_ack_resolve's verdict is a
constant (ncand = 0 for every message), so the untimed ticks of a speculative batch queue the member kernel alone and
the receivers count their messages in the lister's place. A member kernel that writes stops the batch (the wrote word),
and the host goes on from the next tick's lister. Every variant must be bit-identical (state hashes after every phase,
full event streams, the deterministic counters and the lister's own counters) to the run with a lister on every tick
(SWIM_NO_LISTERFREE=1), to the run with a diff on every tick as well (SWIM_NO_ELIDE=1) and to the CPU oracle.

Sizes as in test_gpu_diff_dirty.py: 2 100 members are 2 chunks, 4 200 are 3 (the last one partial), 9 000 are 5."""
import pytest

from swimhip import SimConfig, SimulatedCluster, _abi

from parity_util import run_lockstep
from test_gpu_diff_dirty import FAST_SYNC, FAULT_CAPS, create, dirty, fault_run, same_runs

pytestmark = pytest.mark.gpu

NO_LF = {"SWIM_NO_LISTERFREE": "1"}
NO_ELIDE = {"SWIM_NO_ELIDE": "1"}
VARIANTS = (("default", None), ("SWIM_NO_LISTERFREE", NO_LF), ("SWIM_NO_ELIDE", NO_ELIDE))
# What the lister counts, the same in every variant whoever counted: the messages resolved from the write logs and the
# others (swim_counters) in every run; in a clean cluster also what swim_debug_diff_dirty derives from its counters. (Once
# rows are dirty those depend on the masks, and the masks on the ticks at which the host looked at the rebase counters:
# between batches, which the variants cut differently. The results do not.)
LISTER = ("ack_resolved_total", "diff_msgs_total")
LISTER_CLEAN = ("diff_key_bytes_total",)
LISTER_DD = ("skipped", "streamed", "msg_skipped", "pin_decided", "rebases", "dirty_rows")


def lister_counts(engine, c, clean=True):
    ctr, dd = c.counters(), dirty(engine, c)
    lc = {k: ctr[k] for k in LISTER}
    if clean:
        lc.update({k: ctr[k] for k in LISTER_CLEAN})
        lc.update({k: dd[k] for k in LISTER_DD})
    return ctr, dd, lc


def same_lister_counts(runs):
    """runs: (name, the third value of lister_counts)."""
    name0, c0 = runs[0]
    for name, c in runs[1:]:
        assert c == c0, f"{name} vs {name0}: {c} != {c0}"


def periods(c, n):
    """n periods, a call each (a speculative batch ends with its call, and the mode is entered between two batches)."""
    for _ in range(n):
        c.run_periods(1)


def mode_off(dd):
    assert dd["lister_free_ticks"] == 0 and dd["lister_free_stops"] == 0, dd


@pytest.mark.parametrize("n", [2100, 9000])
def test_clean_steady_state(engine, n):
    """9 000 members: ~1 800 payloads per tick, well over a hundred receivers with several (pinned) payloads per tick."""
    cfg = SimConfig(n_members=n, cluster=FAST_SYNC)
    runs, cnts = [], []
    for name, env in VARIANTS:
        c = create(engine, cfg, env)
        periods(c, 4)
        ctr, dd, lc = lister_counts(engine, c)
        print(f"steady {n} {name}: {dd} {lc} sync_merges={ctr['sync_merges']}", flush=True)
        assert _abi.debug_dirty_check(engine, c._h) == 0
        assert ctr["ack_resolved_total"] + ctr["diff_msgs_total"] == ctr["sync_merges"]
        assert dd["skipped"] == -(-n // 2048) * dd["msg_skipped"] and dd["streamed"] == 0, dd
        assert dd["pin_decided"] > 0, dd
        if name == "default":
            assert dd["lister_free_ticks"] > 0 and dd["lister_free_stops"] == 0, dd
            assert dd["diff_halts"] == 0, dd
        else:
            mode_off(dd)
        runs.append((name, [c.state_hash()], c.events(), ctr))
        cnts.append((name, lc))
        c.close()
    same_runs(runs)
    same_lister_counts(cnts)


def test_clean_against_the_oracle(oracle, engine):
    """Two steps of eight ticks: the first batch runs with its listers, the second without."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC)
    o, e = SimulatedCluster(oracle, cfg), create(engine, cfg)
    run_lockstep(o, e, 16, 8, "clean", events=False)
    assert o.events() == e.events()
    dd = dirty(engine, e)
    print(f"clean oracle lockstep: {dd}", flush=True)
    assert dd["lister_free_ticks"] > 0 and dd["lister_free_stops"] == 0 and dd["streamed"] == 0, dd
    e.close()
    o.close()


def test_timed_ticks_interleaved(engine):
    """profile=True times every tenth tick: its lister and diff are queued between two lister-free ticks, and its member
    kernel must not count what that lister counted."""
    runs, cnts = [], []
    for profile in (False, True):
        c = create(engine, SimConfig(n_members=2100, cluster=FAST_SYNC, profile=profile))
        periods(c, 4)
        ctr, dd, lc = lister_counts(engine, c)
        print(f"timed profile={profile}: {dd} {lc} diff_launches={ctr['diff_launches']}", flush=True)
        assert dd["lister_free_ticks"] > 0 and dd["lister_free_stops"] == 0, dd
        assert ctr["ack_resolved_total"] + ctr["diff_msgs_total"] == ctr["sync_merges"]
        assert (ctr["diff_launches"] > 0) == profile
        runs.append((f"profile={profile}", [c.state_hash()], c.events(), ctr))
        cnts.append((f"profile={profile}", lc))
        c.close()
    same_runs(runs)
    same_lister_counts(cnts)


def set_incarnation(engine, c, m, inc):
    """swim_debug_set_incarnation between steps; refused while m has a live-row payload in flight: a tick later then
    (the runs compared are equal up to here, so they all wait the same ticks)."""
    for _ in range(12):
        if _abi.debug_set_incarnation(engine, c._h, m, inc) == 0:
            return
        c.step(1)
    raise AssertionError(f"member {m} had a live-row payload in flight 12 ticks in a row")


def test_dirt_from_the_host(engine):
    """Rows dirtied between steps by the host (no gossip, no device write): the call itself leaves the mode, and the
    new incarnations spread for longer than the 30 ticks that follow, so it is not entered again."""
    cfg = SimConfig(n_members=4200, cluster=FAST_SYNC)
    runs, cnts = [], []
    for name, env in VARIANTS:
        c = create(engine, cfg, env)
        periods(c, 2)
        hs = [c.state_hash()]
        if name == "default":
            assert dirty(engine, c)["lister_free_ticks"] > 0
        for m in (0, 2048, 4199):
            set_incarnation(engine, c, m, 7)
        before = dirty(engine, c)
        for _ in range(3):
            c.step(10)
            hs.append(c.state_hash())
        assert _abi.debug_dirty_check(engine, c._h) == 0
        ctr, dd, lc = lister_counts(engine, c, clean=False)
        print(f"host dirt {name}: {dd} {lc} tick {c.tick}", flush=True)
        assert dd["streamed"] > 0, dd
        if name == "default":  # off since the host call: not one more tick without a lister
            assert dd["lister_free_ticks"] == before["lister_free_ticks"] and dd["lister_free_stops"] == 0, dd
        else:
            mode_off(dd)
        runs.append((name, hs, c.events(), ctr))
        cnts.append((name, lc))
        c.close()
    same_runs(runs)
    same_lister_counts(cnts)


def test_dirt_inside_a_batch_against_the_oracle(oracle, engine):
    """update_incarnation queued while the mode is on: P0 of the next tick changes a key (and takes a gossip slot in the
    same launch) inside a lister-free batch. Three steps of eight ticks in lockstep, the bump before the third."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC)
    o, e = SimulatedCluster(oracle, cfg), create(engine, cfg)
    run_lockstep(o, e, 16, 8, "clean", events=False)
    before = dirty(engine, e)
    assert before["lister_free_ticks"] > 0, before
    for c in (o, e):
        c.update_incarnation(77)
    run_lockstep(o, e, 8, 8, "bump", events=False)
    assert o.events() == e.events()
    dd = dirty(engine, e)
    print(f"bump oracle lockstep: before {before} after {dd}", flush=True)
    # the first tick of the third batch ran without a lister and wrote: nothing after it did
    assert dd["lister_free_ticks"] <= before["lister_free_ticks"] + 1, (before, dd)
    e.close()
    o.close()


# periods after an incarnation bump within which the mode must be on again: the gossip of the bump is spread for
# 3 x ceil(log2 N) = 36 gossip periods of 2 ticks and swept after twice that (~22 periods of 10 ticks in all), then
# every row's chunk 0 is dirty though the rows agree, ~210 SYNC payloads per tick stream it, and N = 2 100 wasted
# compares rebase it at the next look (every 16 ticks)
SETTLE = 40


def test_dirt_inside_a_batch(engine):
    """The same bump queued before one multi-period call, then periods one by one until the gossip is swept and the
    chunk rebased (the default run says how many; the references run as many): the mode leaves, and is on again."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC)
    runs, cnts, settle = [], [], None
    for name, env in VARIANTS:
        c = create(engine, cfg, env)
        periods(c, 2)
        hs = [c.state_hash()]
        first = dirty(engine, c)
        c.update_incarnation(77)
        c.run_periods(3)
        hs.append(c.state_hash())
        mid = dirty(engine, c)
        if name == "default":
            # (the tick of the bump itself ran without a lister, and wrote)
            assert 0 < first["lister_free_ticks"] and mid["lister_free_ticks"] <= first["lister_free_ticks"] + 1, (first, mid)
            for q in range(SETTLE):
                c.run_periods(1)
                if dirty(engine, c)["lister_free_ticks"] > mid["lister_free_ticks"]:
                    settle = q + 1
                    break
            assert settle is not None, dirty(engine, c)
        else:
            periods(c, settle)
        hs.append(c.state_hash())
        assert _abi.debug_dirty_check(engine, c._h) == 0
        ctr, dd, lc = lister_counts(engine, c, clean=False)
        print(f"batch dirt {name}: {settle} periods to settle; after the bump {mid} at the end {dd} {lc}", flush=True)
        if name == "default":
            assert dd["rebases"] > 0 and dd["dirty_rows"] == 0, dd
        else:
            mode_off(dd)
        runs.append((name, hs, c.events(), ctr))
        cnts.append((name, lc))
        c.close()
    same_runs(runs)
    same_lister_counts(cnts)


def test_device_write_ends_the_mode(engine):
    """A write that starts on the device while the mode is on: a member killed between steps is suspected by whoever
    pings it next (a key change at the ping's timeout). That writer spreads its gossip in the same launch, so the gossip
    halt ends the batch and the wrote word only switches the mode off (lister_free_stops stays 0: DESIGN.md §3.2, no
    writer of a clean cluster comes without a gossip). The results are those of the reference paths."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC)
    runs, cnts = [], []
    for name, env in VARIANTS:
        c = create(engine, cfg, env)
        periods(c, 2)
        hs = [c.state_hash()]
        c.kill(1234)
        for _ in range(3):
            c.run_periods(1)
            hs.append(c.state_hash())
        ctr, dd, lc = lister_counts(engine, c, clean=False)
        print(f"device write {name}: {dd} {lc}", flush=True)
        if name != "default":
            mode_off(dd)
        runs.append((name, hs, c.events(), ctr))
        cnts.append((name, lc))
        c.close()
    same_runs(runs)
    same_lister_counts(cnts)


# killed between steps: with a SYNC every 10 ticks from each of 2 100 members, eight dead members are sent about one
# payload in every tick until they are suspected
VICTIMS = (3, 300, 777, 1024, 1500, 1999, 2047, 2048)


def test_dead_receivers(engine):
    """Payloads to members killed between steps are dropped by the triage, which counts them in the lister's place while
    the mode is on (a kill changes no row, mask or message: the mode stays on across it)."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC)
    runs, cnts = [], []
    for name, env in VARIANTS:
        c = create(engine, cfg, env)
        periods(c, 2)
        hs = [c.state_hash()]
        before = dirty(engine, c)
        for m in VICTIMS:
            c.kill(m)
        for _ in range(4):
            c.step(5)
            hs.append(c.state_hash())
        ctr, dd, lc = lister_counts(engine, c, clean=False)
        print(f"dead receivers {name}: before {before} after {dd} {lc}", flush=True)
        if name == "default":
            assert dd["lister_free_ticks"] > before["lister_free_ticks"], (before, dd)
        else:
            mode_off(dd)
        runs.append((name, hs, c.events(), ctr))
        cnts.append((name, lc))
        c.close()
    same_runs(runs)
    same_lister_counts(cnts)


def test_link_delays(engine):
    """Every link 200 ms late: delayed payloads are stored and redelivered as snapshots, the mode never enters."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC, delay_cap_ms=500)
    runs, cnts = [], []
    for name, env in (("default", None), ("SWIM_NO_LISTERFREE", NO_LF)):
        c = create(engine, cfg, env)
        c.set_default_link_settings(0, 200)
        hs = []
        for _ in range(3):
            c.run_periods(1)
            hs.append(c.state_hash())
        ctr, dd, lc = lister_counts(engine, c, clean=False)
        print(f"delays {name}: {dd} {lc}", flush=True)
        mode_off(dd)
        runs.append((name, hs, c.events(), ctr))
        cnts.append((name, lc))
        c.close()
    same_runs(runs)
    same_lister_counts(cnts)


def test_fault_script(engine):
    """The fault script of test_gpu_diff_dirty.py (loss, a kill, a leave, metadata and incarnation bumps)."""
    cfg = SimConfig(n_members=4200, cluster=FAST_SYNC, **FAULT_CAPS)
    a, dda, _ = fault_run(engine, cfg, None, "default")
    b, ddb, _ = fault_run(engine, cfg, NO_LF, "SWIM_NO_LISTERFREE")
    mode_off(ddb)
    same_runs([b, a])
    for k in LISTER:
        assert a[3][k] == b[3][k], k
