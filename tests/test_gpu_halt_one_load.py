"""The halt words of a speculative batch, read at once (csrc/spec.h halt_load), and the member kernel's front, which
issues its triage loads beside them and decides when both have arrived (csrc/member.hip, DESIGN.md §3.2 "Round 15").

A launch of a batch that halted at an earlier tick must leave no trace although its loads are already in flight when
it learns that it is void, and the combined read must decide as the three single loads did. Each scenario runs twins
through the same calls: one handle is stepped a tick per call (every call is a batch of one tick: no launch is ever
queued behind a halt), the other in whole batches, where the halt stops the launches queued behind it and the host
resumes. Tick, state hashes and counters are compared at every call boundary of the batched handle, the event streams
at the end. One scenario per way a batch stops (step.hip spec_batch): the gossip halt, the wrote word of a lister-free
batch, the diff-halt of an eliding one. The handle's own counters say that the stop happened.

Sizes: 65 and 66 members (two waves, the second with one or two members: the lanes past the last member load a clamped
index), 257 (a second block with one member) and 300."""
from dataclasses import replace

import numpy as np
import pytest

from swimhip import SimConfig, _abi

from test_gpu_diff_dirty import FAST_SYNC, create, dirty

pytestmark = pytest.mark.gpu

COUNTS = ("record_compares", "row_writes", "messages", "gossip_messages", "events", "messages_lost", "gossips_created",
          "sync_merges", "ack_resolved_total", "diff_msgs_total")


def all_events(c):
    out = []
    while True:
        ev = c.events()
        if not ev:
            return out
        out += ev


def same_at_boundary(name, one, bat):
    assert one.tick == bat.tick, (name, one.tick, bat.tick)
    ho, hb = one.state_hash(), bat.state_hash()
    if not np.array_equal(ho, hb):
        m, w = np.argwhere(ho != hb)[0]
        raise AssertionError(f"{name}: state hash differs at tick {bat.tick}, member {m} word {w}")
    co, cb = one.counters(), bat.counters()
    for k in COUNTS:
        assert co[k] == cb[k], (name, bat.tick, k, co[k], cb[k])


def twins(engine, cfg):
    cfg = replace(cfg, record_events=True)
    return create(engine, cfg), create(engine, cfg)


def batched(name, one, bat, calls, ticks):
    """`calls` calls of `ticks` ticks on the batched handle, a tick per call on the other; compared after each."""
    for _ in range(calls):
        bat.step(ticks)
        for _ in range(ticks):
            one.step(1)
        same_at_boundary(name, one, bat)


def finish(name, one, bat):
    eo, eb = all_events(one), all_events(bat)
    assert eo == eb, f"{name}: event streams differ ({len(eo)} vs {len(eb)})"
    one.close()
    bat.close()


@pytest.mark.parametrize("n", [65, 66, 300])
def test_gossip_halt(engine, n):
    """update_incarnation before a step of several periods: P0 of the first tick takes a gossip slot, member(k) raises
    the gossip halt, and everything queued behind it returns at once; the host resumes with the gossip plane, and as
    long as the gossip spreads every further batch halts again."""
    name = f"gossip halt {n}"
    one, bat = twins(engine, SimConfig(n_members=n, cluster=FAST_SYNC))
    batched(name, one, bat, 2, 10)
    g0, d0 = bat.counters()["gossips_created"], dirty(engine, bat)
    for c in (one, bat):
        c.update_incarnation(n - 1)
    batched(name, one, bat, 1, 30)
    ctr, d1 = bat.counters(), dirty(engine, bat)
    print(f"{name}: gossips_created {g0} -> {ctr['gossips_created']}, gossip_messages {ctr['gossip_messages']}, "
          f"diff_elided {d0['diff_elided']} -> {d1['diff_elided']}", flush=True)
    # the gossip of the bump was created and sent inside the batched call: its member kernel halted the batch
    assert ctr["gossips_created"] > g0 and ctr["gossip_messages"] > 0, ctr
    # and the call did go through the halt's path: a batch of 30 ticks that runs whole counts 29 or 30 ticks without a
    # diff launch (spec_batch: every untimed tick behind the first front); one that halts counts the ticks up to the
    # halt only and stops eliding (a gossip plane ran)
    assert d0["diff_elided"] > 0 and d1["diff_elided"] - d0["diff_elided"] < 29, (d0, d1)
    batched(name, one, bat, 1, 30)
    finish(name, one, bat)


@pytest.mark.parametrize("n", [257, 300])
def test_write_inside_a_lister_free_batch(engine, n):
    """A member killed while the lister-free mode is on: the suspicion of whoever pings it next is a key change, written
    by a member kernel in the middle of a batch of launches that were queued without listers (MT_LF: they return on the
    wrote word)."""
    name = f"lister-free write {n}"
    one, bat = twins(engine, SimConfig(n_members=n, cluster=FAST_SYNC))
    for _ in range(6):  # (the mode is entered between two batches, after an elided batch that listed nothing)
        batched(name, one, bat, 1, 10)
        if dirty(engine, bat)["lister_free_ticks"] > 0:
            break
    before = dirty(engine, bat)
    assert before["lister_free_ticks"] > 0, before
    for c in (one, bat):
        c.kill(n // 2)
    batched(name, one, bat, 4, 10)
    dd = dirty(engine, bat)
    print(f"{name}: before {before} after {dd}", flush=True)
    # The batch of the write began in the mode and stopped inside it: some of its ticks ran without a lister, not all
    # ten, and none since. (lister_free_stops counts the batches that the wrote word alone stopped. It stays 0 here, as
    # in test_gpu_lister_free.test_device_write_ends_the_mode: a writer of a clean cluster spreads its gossip in the same
    # launch, so the gossip halt word carries the same tick and the host takes that path. Measured on
    # MI355X: lister_free_ticks 10 -> 17 (257 members) and 10 -> 16 (300), lister_free_stops 0.)
    assert before["lister_free_ticks"] < dd["lister_free_ticks"] < before["lister_free_ticks"] + 10, (before, dd)
    assert bat.counters()["gossips_created"] > 0
    finish(name, one, bat)


def set_incarnation(engine, c, m, inc):
    """swim_debug_set_incarnation between steps; refused while m has a live-row payload in flight: a tick later then
    (the twins are equal up to here, so they wait the same ticks)."""
    for _ in range(12):
        if _abi.debug_set_incarnation(engine, c._h, m, inc) == 0:
            return
        c.step(1)
    raise AssertionError(f"member {m} had a live-row payload in flight 12 ticks in a row")


@pytest.mark.parametrize("n", [66, 257])
def test_diff_halt_under_elision(engine, n):
    """Rows dirtied between steps without a gossip: the handle is still eliding its diffs when a lister first lists one
    of those rows' chunks and raises the diff-halt; member(kd) and everything behind it return at once, before the
    resets, and the host runs that diff over the lists as they stand."""
    name = f"diff-halt {n}"
    one, bat = twins(engine, SimConfig(n_members=n, cluster=FAST_SYNC))
    batched(name, one, bat, 2, 10)
    for c in (one, bat):
        for m in (0, n // 2, n - 1):
            set_incarnation(engine, c, m, 7)
    same_at_boundary(name, one, bat)
    batched(name, one, bat, 3, 10)
    dd = dirty(engine, bat)
    print(f"{name}: {dd}", flush=True)
    assert dd["diff_halts"] >= 1 and dd["streamed"] > 0, dd
    finish(name, one, bat)
