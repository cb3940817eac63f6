"""Ticks without a k_sync_diff launch on one GPU: the lister decides a pinned live-row payload (one of
several payloads of its receiver in a tick) when every row involved is clean, and a speculative batch queues no diff on
its untimed ticks; a lister that lists work after all raises a diff-halt, the host runs that diff and the handle stops
eliding until a whole batch has listed nothing. Every variant must be bit-identical (state hashes after every phase,
full event streams, the deterministic counters) to the run with a diff launch on every tick (SWIM_NO_ELIDE=1), to the
run that consults no mask (SWIM_NO_DIRTY=1: no pinned decision either) and to the CPU oracle.

Sizes as in test_gpu_diff_dirty.py: 2 100 members are 2 chunks, 4 200 are 3 (the last one partial), 9 000 are 5 (two
items, the second with one partial chunk)."""
import pytest

from swimhip import SimConfig, SimulatedCluster, _abi

from parity_util import run_lockstep
from test_gpu_diff_dirty import FAST_SYNC, FAULT_CAPS, create, dirty, fault_phase, fault_run, same_runs

pytestmark = pytest.mark.gpu

NO_ELIDE = {"SWIM_NO_ELIDE": "1"}
NO_DIRTY = {"SWIM_NO_DIRTY": "1"}


def test_clean_steady_state(engine):
    """~1 800 payloads per tick over 9 000 receivers: well over a hundred receivers with several payloads per tick."""
    cfg = SimConfig(n_members=9000, cluster=FAST_SYNC)
    runs = []
    for name, env in (("default", None), ("SWIM_NO_ELIDE", NO_ELIDE), ("SWIM_NO_DIRTY", NO_DIRTY)):
        c = create(engine, cfg, env)
        c.run_periods(4)
        ctr, dd = c.counters(), dirty(engine, c)
        print(f"steady {name}: {dd} diff_msgs_total={ctr['diff_msgs_total']} ack_resolved_total="
              f"{ctr['ack_resolved_total']} sync_merges={ctr['sync_merges']} diff_key_bytes_total="
              f"{ctr['diff_key_bytes_total']}", flush=True)
        assert _abi.debug_dirty_check(engine, c._h) == 0
        assert ctr["ack_resolved_total"] + ctr["diff_msgs_total"] == ctr["sync_merges"]
        if name == "default":
            assert dd["pin_decided"] > 0 and dd["diff_elided"] > 0 and dd["diff_halts"] == 0, dd
            assert dd["streamed"] == 0 and ctr["diff_key_bytes_total"] == 0, (dd, ctr)
            assert dd["skipped"] == 5 * dd["msg_skipped"], dd
        elif name == "SWIM_NO_ELIDE":
            assert dd["diff_elided"] == 0 and dd["diff_halts"] == 0, dd
        else:
            assert dd["pin_decided"] == 0 and dd["diff_elided"] == 0 and dd["diff_halts"] == 0, dd
        runs.append((name, [c.state_hash()], c.events(), ctr))
        c.close()
    same_runs(runs)


def set_incarnation(engine, c, m, inc):
    """swim_debug_set_incarnation between steps; refused while m has a live-row payload in flight: a tick later then
    (the runs compared are equal up to here, so they all wait the same ticks)."""
    for _ in range(12):
        if _abi.debug_set_incarnation(engine, c._h, m, inc) == 0:
            return
        c.step(1)
    raise AssertionError(f"member {m} had a live-row payload in flight 12 ticks in a row")


def test_halt_and_resume(engine):
    """Rows dirtied between steps without a gossip (swim_debug_set_incarnation): the handle is still in speculative
    batches and eliding when the lister first lists one of those rows' chunks."""
    cfg = SimConfig(n_members=4200, cluster=FAST_SYNC)
    runs = []
    for name, env in (("default", None), ("SWIM_NO_ELIDE", NO_ELIDE), ("SWIM_NO_DIRTY", NO_DIRTY)):
        c = create(engine, cfg, env)
        c.run_periods(2)
        hs = [c.state_hash()]
        for m in (0, 2048, 4199):
            set_incarnation(engine, c, m, 7)
        for _ in range(3):
            c.step(10)
            hs.append(c.state_hash())
        assert _abi.debug_dirty_check(engine, c._h) == 0
        dd = dirty(engine, c)
        print(f"halt {name}: {dd} tick {c.tick}", flush=True)
        if name == "default":
            assert dd["diff_halts"] >= 1 and dd["streamed"] > 0, dd
        else:
            assert dd["diff_halts"] == 0 and dd["diff_elided"] == 0, dd
        runs.append((name, hs, c.events(), c.counters()))
        c.close()
    same_runs(runs)


def test_mixed_siblings_under_faults(engine):
    """The fault script of test_equality_under_faults: snapshot and live-row siblings, dirty and clean rows, receivers
    of several payloads whose later payloads are re-checked (trk=1: by the bitmap walk; mq=1: selected by list walks).
    A decided payload that was read after all would raise E_PIN and fail the step."""
    cfg = SimConfig(n_members=4200, cluster=FAST_SYNC, **FAULT_CAPS)
    runs = []
    for name, env in (("default", None), ("SWIM_NO_ELIDE", NO_ELIDE), ("SWIM_NO_DIRTY", NO_DIRTY),
                      ("trk=1,mq=1", {"SWIM_CAPS": "trk=1,mq=1"})):
        run, dd, _ = fault_run(engine, cfg, env, name)
        if name == "SWIM_NO_DIRTY":
            assert dd["pin_decided"] == 0 and dd["diff_elided"] == 0, dd
        runs.append(run)
    same_runs(runs)


def test_against_the_oracle(oracle, engine):
    """The fault operations up front, 16 ticks in steps of eight (speculative batches where no gossip is in flight)."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC, **FAULT_CAPS)
    o, e = SimulatedCluster(oracle, cfg), create(engine, cfg)
    for c in (o, e):
        for phase in range(3):
            fault_phase(c, phase, cfg.n_members)
    run_lockstep(o, e, 16, 8, "faults", events=False)
    assert _abi.debug_dirty_check(engine, e._h) == 0
    assert o.events() == e.events()
    print(f"oracle lockstep: {dirty(engine, e)}", flush=True)
    e.close()
    o.close()


def test_clean_against_the_oracle(oracle, engine):
    """A clean preconverged cluster, where every tick but the first elides its diff: two steps of eight ticks."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC)
    o, e = SimulatedCluster(oracle, cfg), create(engine, cfg)
    run_lockstep(o, e, 16, 8, "clean", events=False)
    assert o.events() == e.events()
    dd = dirty(engine, e)
    print(f"clean oracle lockstep: {dd}", flush=True)
    assert dd["diff_elided"] > 0 and dd["diff_halts"] == 0 and dd["streamed"] == 0, dd
    e.close()
    o.close()


def delayed(engine, cfg, env, setup):
    c = create(engine, cfg, env)
    setup(c)
    hs = []
    for _ in range(2):
        c.run_periods(1)
        hs.append(c.state_hash())
    run = (str(env), hs, c.events(), c.counters())
    dd = dirty(engine, c)
    c.close()
    return run, dd


def late_ack_links(c):
    for h in range(2, 6):
        c.block(1, h)
    c.set_link_settings(1, 0, 0, 500)


def test_link_delays(engine):
    """k_sync_redeliver and k_sync_defer run after every member kernel once a delay is set, in speculative batches too:
    the smallest delayed one-GPU configuration of test_gpu_delay.py (test_late_direct_ack), preconverged, two periods."""
    cfg = SimConfig(n_members=6, record_events=True, emulator_counters=True, delay_cap_ms=500)
    a, _ = delayed(engine, cfg, None, late_ack_links)
    b, _ = delayed(engine, cfg, NO_ELIDE, late_ack_links)
    same_runs([b, a])


def test_link_delays_with_syncs(engine):
    """The same with delayed SYNC / SYNC_ACK payloads in flight (a SYNC every 10 ticks, every link 200 ms late): their
    redelivered snapshots are siblings that the pinned decision must leave to the diff."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC, delay_cap_ms=500)
    a, dd = delayed(engine, cfg, None, lambda c: c.set_default_link_settings(0, 200))
    b, _ = delayed(engine, cfg, NO_ELIDE, lambda c: c.set_default_link_settings(0, 200))
    print(f"delays with syncs: {dd}", flush=True)
    same_runs([b, a])
