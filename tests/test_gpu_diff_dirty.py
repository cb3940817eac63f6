"""Dirty-chunk skipping of the SYNC diff on one GPU: a 2048-subject chunk of a live-row payload that
neither the sender's nor the receiver's row ever changed against the baseline row equals it in both, so its compares
are decided without a load, and the baseline follows the cluster by rebasing (k_rebase). The skipping run must be
bit-identical to the run that streams every chunk (SWIM_NO_DIRTY=1, masks kept but never consulted) and to the CPU
oracle, and the masks' invariant (a clean chunk equals the baseline's) must hold at every look (swim_debug_dirty_check).

Sizes sit just past the chunk (2048 subjects) and item (4 chunks) boundaries: 2 100 members are 2 chunks, 4 200 are 3
(the last one partial), 9 000 are 5: one full item and a second one with a single partial chunk. A second mask word
needs more than 131 072 members, which no cluster here has: the lister's and k_sync_diff's MW > 1 loops run on rows of
131 080 and 262 152 subjects (two and three mask words) in test_gpu_sync_diff.py, the helpers they call (dirty_mark,
dirty_mark_wave and payload_key_at's rank) on 2- and 3-word masks in test_gpu_primitives.py."""
import os

import numpy as np
import pytest

from swimhip import ClusterConfig, SimConfig, SimulatedCluster, _abi

from parity_util import run_lockstep

pytestmark = pytest.mark.gpu

FAST_SYNC = ClusterConfig(syncInterval=1000)  # SYNC every 10 ticks: many SYNC / SYNC_ACK pairs per tick
# (the fault scripts' repeated incarnation bumps under loss hold more than the default 256 metadata fetches open per member)
FAULT_CAPS = dict(gossip_slot_cap=1 << 16, pending_fetch_cap=2048)
DET = ("record_compares", "row_writes", "messages", "events", "sync_merges", "messages_lost")


def create(engine, cfg, env=None):
    """A one-GPU cluster created with the environment settings env (read at create only)."""
    env = env or {}
    os.environ.update(env)
    try:
        return SimulatedCluster(engine, cfg)
    finally:
        for k in env:
            os.environ.pop(k, None)


def dirty(engine, c):
    return _abi.debug_diff_dirty(engine, c._h)


def same_runs(runs):
    """Every run: (name, hashes per phase, events, counters); all equal to the first."""
    name0, h0, e0, c0 = runs[0]
    for name, hs, ev, ctr in runs[1:]:
        assert len(hs) == len(h0)
        for i, (x, y) in enumerate(zip(h0, hs)):
            assert np.array_equal(x, y), f"{name} vs {name0}: state hash differs after phase {i}"
        assert ev == e0, f"{name} vs {name0}: event streams differ"
        for k in DET:
            assert ctr[k] == c0[k], (name, k)


def test_steady_state_skips_everything(engine):
    cfg = SimConfig(n_members=9000, cluster=FAST_SYNC)
    runs = []
    for env in (None, {"SWIM_NO_DIRTY": "1"}):
        c = create(engine, cfg, env)
        c.run_periods(4)
        ctr, dd = c.counters(), dirty(engine, c)
        print(f"steady {env}: {dd} diff_msgs_total={ctr['diff_msgs_total']} ack_resolved_total={ctr['ack_resolved_total']}"
              f" sync_merges={ctr['sync_merges']} diff_key_bytes_total={ctr['diff_key_bytes_total']}", flush=True)
        assert _abi.debug_dirty_check(engine, c._h) == 0
        assert ctr["ack_resolved_total"] + ctr["diff_msgs_total"] == ctr["sync_merges"]
        if env is None:
            assert dd["streamed"] == 0 and dd["msg_skipped"] > 0 and dd["skipped"] == 5 * dd["msg_skipped"]
            assert dd["dirty_rows"] == 0
        else:
            assert dd["skipped"] == 0 and dd["msg_skipped"] == 0 and dd["streamed"] > 0
        runs.append((str(env), [c.state_hash()], c.events(), ctr))
        c.close()
    same_runs(runs)


# members of chunk 0, chunk 1, the last partial chunk and both sides of a chunk boundary (4 200 members)
BUMP = (5, 2047, 2048, 2100, 4150)
PRESET = (7, 2047, 4150)  # start at incarnation 60: three bumps take them past the 8-bit shadow's escape


def fault_phase(c, phase, n):
    if phase == 0:
        c.set_default_loss(10)
    elif phase == 1:
        c.kill(n - 100)
        c.update_metadata(11)
    elif phase == 2:
        c.leave(90)
    for m in BUMP:
        if m < n:
            c.update_incarnation(m)


def fault_run(engine, cfg, env, name, ticks=15, quiet=0):
    """The fault script on a fresh cluster: hashes after every phase, 0 invariant violations at every look."""
    c = create(engine, cfg, env)
    for m in PRESET:
        if m < cfg.n_members:
            assert _abi.debug_set_incarnation(engine, c._h, m, 60) == 0
    assert _abi.debug_dirty_check(engine, c._h) == 0
    hs = []
    for phase in range(3):
        fault_phase(c, phase, cfg.n_members)
        c.step(ticks)
        hs.append(c.state_hash())
        assert _abi.debug_dirty_check(engine, c._h) == 0, (name, phase)
    last, per = None, []
    if quiet:  # no loss and no further change: the rows agree again
        c.set_default_loss(0)
        for q in range(quiet):
            before = _abi.debug_diff_dirty(engine, c._h, 4)
            c.run_periods(1)
            if q % 5 == 4:
                hs.append(c.state_hash())
            last = {k: v - before[k] for k, v in _abi.debug_diff_dirty(engine, c._h, 4).items()}
            per.append(last["streamed"])
        assert _abi.debug_dirty_check(engine, c._h) == 0, (name, "quiet")
    dd = dirty(engine, c)
    print(f"{name}: {dd} streamed per quiet period {per}", flush=True)
    run = (name, hs, c.events(), c.counters())
    c.close()
    return run, dd, last


def test_equality_under_faults(engine):
    cfg = SimConfig(n_members=4200, cluster=FAST_SYNC, **FAULT_CAPS)
    runs = []
    for name, env in (("default", None), ("SWIM_NO_DIRTY", {"SWIM_NO_DIRTY": "1"}), ("hv=1", {"SWIM_CAPS": "hv=1"})):
        run, dd, _ = fault_run(engine, cfg, env, name)
        if name != "SWIM_NO_DIRTY":
            assert dd["skipped"] > 0 and dd["streamed"] > 0, (name, dd)
        else:
            assert dd["skipped"] == 0 and dd["rebases"] == 0, dd
        runs.append(run)
    same_runs(runs)


def test_against_the_oracle(oracle, engine):
    """Independent of the engine's own reference path: the fault script's operations, all at the start and for 16
    ticks only (the CPU oracle takes seconds per tick at this size once the gossips of the faults spread)."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC, **FAULT_CAPS)
    o, e = SimulatedCluster(oracle, cfg), create(engine, cfg)
    for c in (o, e):
        for phase in range(3):
            fault_phase(c, phase, cfg.n_members)
    run_lockstep(o, e, 16, 8, "faults", events=False)
    assert _abi.debug_dirty_check(engine, e._h) == 0
    assert o.events() == e.events()
    dd = dirty(engine, e)
    print(f"oracle lockstep: {dd}", flush=True)
    assert dd["skipped"] > 0 and dd["streamed"] > 0
    e.close()
    o.close()


def test_cold_join(engine):
    """A start that is not preconverged: an empty baseline, every member's own chunk dirty, rows filling up. 300 members
    start at once and the others join in waves, the second chunk's first (2 100 joining in one tick would need more
    candidate-pool entries than the engine sizes by default)."""
    n = 2100
    cfg = SimConfig(n_members=n, cluster=ClusterConfig(seedMembers=[0], syncInterval=1000),
                    init_mode=_abi.INIT_COLD_JOIN, n_dormant=n - 300, pending_fetch_cap=4096)
    waves = [range(2040, 2100), range(300, 500), range(1900, 2040)]
    runs = []
    for name, env in (("default", None), ("SWIM_NO_DIRTY", {"SWIM_NO_DIRTY": "1"})):
        c = create(engine, cfg, env)
        assert _abi.debug_dirty_check(engine, c._h) == 0
        assert dirty(engine, c)["dirty_rows"] == n  # the own record's chunk of every row
        hs = []
        for wave in [()] + waves:
            for m in wave:
                c.join(m)
            c.step(10)
            hs.append(c.state_hash())
            assert _abi.debug_dirty_check(engine, c._h) == 0, name
        print(f"cold join {name}: {dirty(engine, c)}", flush=True)
        runs.append((name, hs, c.events(), c.counters()))
        c.close()
    same_runs(runs)


# periods without loss or changes after the fault script. With suspicionMult = 1 a suspicion lasts 13 periods at this
# size, so the killed member is declared DEAD, the record of that spreads and the rows agree again within the stretch
QUIET = 26


def test_rebase_follows_the_cluster(engine):
    """Rebases made frequent (threshold 8 wasted compares, looked at every tick): they fire while the rows disagree,
    and once the cluster is quiet the baseline catches up: nothing is streamed any more."""
    cfg = SimConfig(n_members=4200, cluster=ClusterConfig(syncInterval=1000, suspicionMult=1), **FAULT_CAPS)
    ref, _, _ = fault_run(engine, cfg, {"SWIM_NO_DIRTY": "1"}, "SWIM_NO_DIRTY", quiet=QUIET)
    run, dd, last = fault_run(engine, cfg, {"SWIM_CAPS": "rbt=8,rbi=1"}, "rebase", quiet=QUIET)
    same_runs([ref, run])
    assert dd["rebases"] > 0, dd
    assert last["streamed"] == 0 and last["skipped"] > 0, last


def test_debug_set_incarnation_marks_the_chunk(engine):
    cfg = SimConfig(n_members=4200, cluster=FAST_SYNC)
    c = create(engine, cfg)
    assert dirty(engine, c)["dirty_rows"] == 0
    for i, m in enumerate((2048, 4199, 0)):
        assert _abi.debug_set_incarnation(engine, c._h, m, 7) == 0
        assert dirty(engine, c)["dirty_rows"] == i + 1  # one row, the member's own chunk
        assert _abi.debug_dirty_check(engine, c._h) == 0
    c.step(20)
    assert _abi.debug_dirty_check(engine, c._h) == 0
    c.close()
