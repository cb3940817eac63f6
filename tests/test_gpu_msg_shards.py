"""The message buffers' slot shards (csrc/msg_slots.h, DESIGN.md §3.2 "Round 14") against the unsharded buffer.

SWIM_MSG_SHARDS=n (read at create) sets the shards of a one-GPU handle's SYNC message buffers; 1 is the buffer as it was
before the shards: one counter, slots 0, 1, 2, ... Twin handles, 8 shards against 1, go through the same calls one tick
per step, and after every tick their state hashes (which fold every member's event digest) and swim_counters must be
equal; at the end the full event streams, the emulator counters, every member's request counters, the capacity
fallbacks, swim_debug_diff_dirty's counters and swim_debug_light. Nothing a caller can observe depends on which slot a
message took.

Sizes: 66 members (two waves, the second partial: shards 0 and 1), 96, and 300 (two blocks, eight waves: all 8 shards).
The scenarios cover every reader of a buffer: the light path's and the general body's sends, the lister (k_ack_resolve)
on every tick and on none, the diff without lists (SWIM_NO_ACKRES), the delayed-message store (k_sync_redeliver,
k_sync_defer), and a cold join whose seed answers every member from one lane, which overflows its shard's Q fast slots
into the overflow region. One sharded run of the delay scenario and of the lossy one is also held against the CPU oracle."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

from swimhip import ClusterConfig, SimConfig, SimulatedCluster, _abi

from parity_util import run_lockstep
from test_gpu_diff_dirty import FAST_SYNC, FAULT_CAPS, create, dirty
from test_gpu_light_path import COUNTED, COUNTS, COUNTS_NO_DELAY, DD_HOST, all_events, scalars

pytestmark = pytest.mark.gpu

SIZES = (66, 96, 300)
SHARDED = {"SWIM_MSG_SHARDS": "8", **COUNTED}
PLAIN = {"SWIM_MSG_SHARDS": "1", **COUNTED}


def msg_slots(c):
    """The message buffer of the latest tick as the host readers walk it (a debugging aid of the library, outside the
    ABI headers): shards, Q, R, messages in fast slots, in overflow slots, the highest slot in use, all records sane."""
    fn = c.lib.swimdbg_msg_slots
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 7)()
    assert fn(c._h, out) == 0
    return dict(zip(("shards", "q", "r", "fast", "over", "top", "sane"), (int(v) for v in out)))


def twins(engine, cfg, ticks, script=None, before=None, name="", env=None, dd_all=True, shards="8", chunk=1):
    """`shards` shards and the unsharded reference through the same calls: `before(c)` once, `script(c, t)` before the
    step that starts at tick t, `chunk` ticks per step (1: compared after every tick). Returns swim_debug_light and
    swim_counters of the sharded twin, and the largest fast and overflow message counts any of its steps left.

    After every step the two buffers are read back: the sharded twin must have been created with `shards` shards and
    hold its messages in fast slots (and overflow slots) that the walk finds, the reference must hold the same number
    of messages in slots 0, 1, 2, ... of an unsharded buffer."""
    cfg = replace(cfg, record_events=True, emulator_counters=True)
    new = create(engine, cfg, {**SHARDED, "SWIM_MSG_SHARDS": shards, **(env or {})})
    ref = create(engine, cfg, {**PLAIN, **(env or {})})
    peak = {"fast": 0, "over": 0}
    try:
        for c in (new, ref):
            if before:
                before(c)
        for t in range(0, ticks, chunk):
            for c in (new, ref):
                if script:
                    script(c, t)
                c.step(chunk)
            sn, sr = msg_slots(new), msg_slots(ref)
            assert sn["shards"] == int(shards) and sn["q"] == sn["r"] // int(shards) and sn["sane"] == 1, (name, t, sn)
            assert sr["shards"] == 1 and sr["r"] == 0 and sr["fast"] == 0 and sr["sane"] == 1, (name, t, sr)
            assert sn["fast"] + sn["over"] == sr["over"], (name, t, sn, sr)  # the same messages, whatever their slots
            assert sr["over"] == 0 or sr["top"] == sr["over"] - 1, (name, t, sr)
            assert sn["fast"] <= sn["r"] and (sn["over"] == 0 or sn["top"] == sn["r"] + sn["over"] - 1), (name, t, sn)
            peak["fast"], peak["over"] = max(peak["fast"], sn["fast"]), max(peak["over"], sn["over"])
            hn, hr = new.state_hash(), ref.state_hash()
            if not np.array_equal(hn, hr):
                m, w = np.argwhere(hn != hr)[0]
                raise AssertionError(f"{name}: state hash differs after tick {t} at member {m} word {w}")
            cn, cr = new.counters(), ref.counters()
            for k in COUNTS + (COUNTS_NO_DELAY if dd_all else ()):
                assert cn[k] == cr[k], (name, t, k, cn[k], cr[k])
        en, er = all_events(new), all_events(ref)
        assert en == er, f"{name}: event streams differ ({len(en)} vs {len(er)})"
        assert np.array_equal(new.emulator_counters(), ref.emulator_counters()), name
        assert np.array_equal(scalars(new), scalars(ref)), name
        assert _abi.debug_fallbacks(engine, new._h) == _abi.debug_fallbacks(engine, ref._h), name
        dn, dr = dirty(engine, new), dirty(engine, ref)
        for k in (dn if dd_all else DD_HOST):
            assert dn[k] == dr[k], (name, k, dn, dr)
        ln, lr = _abi.debug_light(engine, new._h), _abi.debug_light(engine, ref._h)
        assert ln == lr, (name, ln, lr)  # the same member-ticks on the same path
        print(f"{name}: light {ln}; messages {cn['messages']}, sync merges {cn['sync_merges']}", flush=True)
        assert peak["fast"] > 0, (name, peak)  # the sharded twin did take sharded slots
        return ln, {**cn, "peak_fast": peak["fast"], "peak_over": peak["over"], "q": sn["q"]}
    finally:
        new.close()
        ref.close()


@pytest.mark.parametrize("n", SIZES)
def test_clean_fast_sync(engine, n):
    """(a) 60 clean ticks with a SYNC every period: every tick carries n / 10 SYNCs and their SYNC_ACKs, and the light
    path finishes the steady state's member-ticks on both twins."""
    ln, cn = twins(engine, SimConfig(n_members=n, cluster=FAST_SYNC), 60, name=f"clean {n}")
    assert ln["on"] == 1 and ln["p1"] > 0 and ln["sync"] > 0, ln
    assert cn["sync_merges"] >= 2 * 5 * n - 2 * n, cn  # a SYNC and its SYNC_ACK per member and period, less the ends
    assert ln["ticks"] >= 2 * ln["general"], ln


@pytest.mark.parametrize("n", SIZES)
def test_loss(engine, n):
    """(b) 15 % loss throughout: lost SYNCs and SYNC_ACKs, suspicions, merges with candidates, snapshots (cow)."""
    twins(engine, SimConfig(n_members=n, cluster=FAST_SYNC, **FAULT_CAPS), 60,
          before=lambda c: c.set_default_loss(15), name=f"loss {n}")


@pytest.mark.parametrize("n", SIZES)
def test_partition_heals(engine, n):
    """(c) a partition of the two halves that heals: the general body sends (the SYNC an ALIVE verdict on a SUSPECT row
    sends, merges of rows that differ)."""
    half = (np.arange(n) % 2).astype(np.uint32)

    def script(c, t):
        if t == 5:
            c.partition(half)
        elif t == 45:
            c.unblock_all()

    ln, _ = twins(engine, SimConfig(n_members=n, cluster=FAST_SYNC, **FAULT_CAPS), 80, script=script,
                  name=f"partition {n}")
    assert ln["general"] > 0, ln


@pytest.mark.parametrize("n", SIZES)
def test_lister_on_every_tick(engine, n):
    """(d) SWIM_NO_ELIDE=1: k_ack_resolve walks the buffer on every tick."""
    ln, _ = twins(engine, SimConfig(n_members=n, cluster=FAST_SYNC), 40, name=f"no elide {n}", env={"SWIM_NO_ELIDE": "1"})
    assert ln["p1"] > 0, ln


@pytest.mark.parametrize("n", SIZES)
def test_diff_without_lists(engine, n):
    """(e) SWIM_NO_ACKRES=1: k_sync_diff walks every message of the buffer itself, holes included."""
    def script(c, t):
        if t == 10:
            c.set_default_loss(10)
        elif t == 25:
            c.set_default_loss(0)

    twins(engine, SimConfig(n_members=n, cluster=FAST_SYNC, **FAULT_CAPS), 40, script=script, name=f"no ackres {n}",
          env={"SWIM_NO_ACKRES": "1"})


DELAYS = dict(cluster=FAST_SYNC, delay_cap_ms=300)


@pytest.mark.parametrize("n", SIZES)
def test_link_delays(engine, n):
    """(f) link delays: delayed SYNC / SYNC_ACK messages leave the buffer for the store (k_sync_defer) and come back
    into it (k_sync_redeliver)."""
    twins(engine, SimConfig(n_members=n, **DELAYS), 60, before=lambda c: c.set_default_link_settings(0, 200),
          name=f"delays {n}", dd_all=False)


def test_cold_join_overflows_its_shard(engine):
    """(g) a cold join of 300 members at seed 0 with the override on: the seed's lane answers ~300 SYNCs in a tick from
    one shard, more than its Q = MSGCAP / 32 fast slots, and the rest go to the overflow region. No error (a step that
    raised E_MSGS would fail), and the run equals the twin's."""
    # (the seed fetches 299 members' metadata at once: more than the default 256 pending fetches per member)
    cfg = SimConfig(n_members=300, cluster=ClusterConfig(seedMembers=[0]), init_mode=_abi.INIT_COLD_JOIN, **FAULT_CAPS)
    _, cn = twins(engine, cfg, 40, name="cold join 300")
    assert cn["sync_merges"] >= 2 * 299, cn
    # the seed's answers of one tick: its shard's Q fast slots, the rest in the overflow region
    assert cn["peak_over"] >= 299 - cn["q"] - 8 and cn["peak_fast"] >= cn["q"], cn


def test_default_shard_count(engine):
    """(h) 2 304 members (nine blocks, 36 waves) with 32 shards, 20 clean ticks."""
    ln, _ = twins(engine, SimConfig(n_members=2304, cluster=FAST_SYNC), 20, name="32 shards 2304", shards="32")
    assert ln["p1"] > 0 and ln["sync"] > 0, ln


@pytest.mark.parametrize("n,shards", [(300, "8"), (2304, "32")])
def test_whole_periods_per_step(engine, n, shards):
    """Ten ticks per step: the speculative batches, whose launches reset the next buffer's counters at their start
    (tick_reset), and after a clean one the lister-free batches, where no kernel but the member kernel reads a buffer."""
    ln, _ = twins(engine, SimConfig(n_members=n, cluster=FAST_SYNC), 80, name=f"periods {n}", shards=shards, chunk=10)
    assert ln["p1"] > 0 and ln["sync"] > 0, ln


def sharded_against_oracle(oracle, engine, cfg, before, ticks, name):
    cfg = replace(cfg, record_events=True, emulator_counters=True)
    o, e = SimulatedCluster(oracle, cfg), create(engine, cfg, SHARDED)
    try:
        for c in (o, e):
            before(c)
        run_lockstep(o, e, ticks, 10, name)
        assert np.array_equal(o.emulator_counters(), e.emulator_counters()), name
    finally:
        o.close()
        e.close()


def test_sharded_link_delays_against_the_oracle(oracle, engine):
    sharded_against_oracle(oracle, engine, SimConfig(n_members=66, **DELAYS),
                           lambda c: c.set_default_link_settings(0, 200), 60, "oracle, delays 66, 8 shards")


def test_sharded_loss_against_the_oracle(oracle, engine):
    sharded_against_oracle(oracle, engine, SimConfig(n_members=66, cluster=FAST_SYNC, **FAULT_CAPS),
                           lambda c: c.set_default_loss(15), 60, "oracle, loss 66, 8 shards")


def test_override_is_checked(engine):
    with pytest.raises(Exception):
        create(engine, SimConfig(n_members=66), {"SWIM_MSG_SHARDS": "3"})
