"""The light path while nobody is dead (csrc/member_light.h, DESIGN.md §3.2 "Round 13") against the general body.

One device word, first_dead, is at most every member's dead tick. A member kernel launched for a tick below it skips the
light path's dead-member lookups (the ping target's, a hop target's, the SYNC and SYNC_ACK destinations').
Each scenario runs through test_gpu_light_path.lockstep (the default build and SWIM_NO_LIGHT=1, every state hash after
every tick, then events, counters, emulator counters and request scalars), and after every tick reads
swim_debug_light_sure of both handles: first_dead <= min(dead_tick) always, and the counter says when the shortcut
was taken, so that no scenario passes by never taking it (or, where it must be off, by taking it).

Sizes as test_gpu_light_path: 66 members (two waves, the second partial), 96, 300 (two blocks), and one run of 2 100
members stepped whole periods at a time."""
import numpy as np
import pytest

from swimhip import ClusterConfig, SimConfig, _abi

from test_gpu_diff_dirty import FAST_SYNC, FAULT_CAPS, create, dirty
from test_gpu_light_path import COUNTED, COUNTS, HEAL, NO_LIGHT, SIZES, SYNC_MS, faults_then_partition, lockstep

pytestmark = pytest.mark.gpu

NEVER = 0xFFFFFFFF


def look(engine, c, name=""):
    s = _abi.debug_light_sure(engine, c._h)
    assert s["first_dead"] <= s["min_dead"], (name, s)
    return s


class Probe:
    """swim_debug_light_sure of each handle after every step: series(i)[t] is the reading after tick t (one tick per
    step). Handles are numbered in the order lockstep first shows them: 0 the default build, 1 the reference."""

    def __init__(self, engine, script=None):
        self.engine, self.script, self.handles, self.readings = engine, script, [], []

    def __call__(self, c, t):  # lockstep's `script`
        if c not in self.handles:
            self.handles.append(c)
            self.readings.append([])
            step, out = c.step, self.readings[-1]

            def stepped(ticks=1):
                step(ticks)
                r = look(self.engine, c, f"after tick {len(out)}")
                r["ticks"] = _abi.debug_light(self.engine, c._h)["ticks"]  # member-ticks the light path finished
                out.append(r)
            c.step = stepped
        if self.script:
            self.script(c, t)

    def series(self, i):
        return self.readings[i]


def reference_idle(probe):
    """The SWIM_NO_LIGHT=1 handle never counts; its word follows the same writers."""
    for a, b in zip(probe.series(0), probe.series(1)):
        assert b["skipped"] == 0, b
        assert (a["first_dead"], a["min_dead"]) == (b["first_dead"], b["min_dead"]), (a, b)


@pytest.mark.parametrize("n", SIZES)
def test_clean_cluster(engine, n):
    """(1) Nobody ever dies: every light member-tick skips its lookups, the pings, the hops and the SYNC / SYNC_ACK
    sends among them."""
    probe = Probe(engine)
    ln, _ = lockstep(engine, SimConfig(n_members=n, cluster=FAST_SYNC), 30, script=probe, name=f"sure clean {n}")
    s = probe.series(0)[-1]
    print(f"sure clean {n}: {s}", flush=True)
    assert s["first_dead"] == NEVER and s["min_dead"] == NEVER
    assert s["skipped"] == ln["ticks"] > 0, (s, ln)
    assert ln["fd"] > 0 and ln["p1"] > 0 and ln["sync"] > 0, ln
    reference_idle(probe)


@pytest.mark.parametrize("n", SIZES)
def test_kills(engine, n):
    """(2) test_gpu_light_path.test_kills' script: kills at ticks 83, 84 and 85 with pings, hops, acks and SYNCs in
    flight to the members that die. The first kill lowers the word to 83; from that tick on nothing is skipped."""
    faults = {83: [lambda c: c.kill(5)], 84: [lambda c: c.kill(n - 2)], 85: [lambda c: c.kill(n // 2)]}
    probe = Probe(engine, faults_then_partition(n, faults, 100))
    lockstep(engine, SimConfig(n_members=n, cluster=ClusterConfig(syncInterval=SYNC_MS[n]), **FAULT_CAPS),
             HEAL[n] // 10 + 4, script=probe, name=f"sure kills {n}")
    s = probe.series(0)
    assert s[82]["first_dead"] == NEVER and s[82]["skipped"] > 0, s[82]
    for r in s[83:]:
        assert r["first_dead"] == 83 and r["min_dead"] == 83, r
        assert r["skipped"] == s[82]["skipped"], (r, s[82])
    reference_idle(probe)


@pytest.mark.parametrize("n", SIZES)
def test_leave(engine, n):
    """(3) leaveCluster: the member is dead from the tick after it swept its own leave notification. That sweep lowers
    the word on the device, in the tick's gossip kernels; the next member kernel already sees it."""
    probe = Probe(engine, lambda c, t: c.leave(11) if t == 57 else None)
    lockstep(engine, SimConfig(n_members=n), 40, script=probe, name=f"sure leave {n}")
    s = probe.series(0)
    left = [t for t, r in enumerate(s) if r["min_dead"] != NEVER]
    assert left and left[0] > 57, left[:1]
    t0 = left[0]
    assert s[t0 - 1]["first_dead"] == NEVER and s[t0 - 1]["skipped"] > 0, s[t0 - 1]
    for r in s[t0:]:
        assert r["first_dead"] == r["min_dead"] == t0 + 1, (t0, r)
        assert r["skipped"] == s[t0]["skipped"], (r, s[t0])
    reference_idle(probe)


@pytest.mark.parametrize("n", SIZES)
def test_loss_and_partition(engine, n):
    """(4) 5 % loss over ticks 40-59, a partition of the halves over ticks 200-259. Sends fail, nobody dies: the word
    stays where it was, and after every tick, the ticks of both faults included, every member-tick the light path has
    finished has skipped its lookups: the counter grows through the faults exactly as the path's own count does. (How
    many it finishes under a fault is the path's own gate, not this shortcut's: the ticks behind a gossip plane run the
    split launches, and the suspicions of the loss may still be spreading when the partition starts. The first ticks of
    the loss do have light member-ticks: a suspicion's gossip starts only after a ping timeout.)"""
    half = (np.arange(n) % 2).astype(np.uint32)

    def script(c, t):
        if t == 40:
            c.set_default_loss(5)
        elif t == 60:
            c.set_default_loss(0)
        elif t == 200:
            c.partition(half)
        elif t == 260:
            c.unblock_all()

    probe = Probe(engine, script)
    ln, _ = lockstep(engine, SimConfig(n_members=n, cluster=FAST_SYNC, **FAULT_CAPS), 30, script=probe,
                     name=f"sure loss, partition {n}")
    s = probe.series(0)
    assert all(r["first_dead"] == NEVER and r["min_dead"] == NEVER for r in s)
    for t, r in enumerate(s):
        assert r["skipped"] == r["ticks"], (t, r)
    assert s[59]["skipped"] > s[39]["skipped"] > 0, (s[39], s[59])
    assert s[259]["skipped"] - s[199]["skipped"] == s[259]["ticks"] - s[199]["ticks"] >= 0, (s[199], s[259])
    assert s[-1]["skipped"] == ln["ticks"], (s[-1], ln)
    reference_idle(probe)


def test_dormant_members(engine):
    """(5) A dormant member refuses connections like a dead one (dead_tick 0), so the word is 0 from create and stays
    there after the join: nothing is ever skipped."""
    cfg = SimConfig(n_members=96, cluster=ClusterConfig(seedMembers=[0]), init_mode=_abi.INIT_COLD_JOIN, n_dormant=8)
    seen = {}

    def script(c, t):
        if t == 0:
            seen[c] = look(engine, c, "at create")
        elif t == 50:
            c.join(95, [0])

    probe = Probe(engine, script)
    ln, _ = lockstep(engine, cfg, 20, script=probe, name="sure dormant 96")
    assert ln["ticks"] > 0, ln  # the light path itself runs
    assert all(r["first_dead"] == 0 and r["min_dead"] == 0 for r in seen.values()), seen
    for r in probe.series(0):
        assert r["first_dead"] == 0 and r["skipped"] == 0, r
    reference_idle(probe)


def test_whole_periods_per_step(engine):
    """(6) Ten ticks per step (test_gpu_light_path.test_whole_periods_per_step's shape): the speculative and the
    lister-free batches take the shortcut too, and a kill between two steps ends it at once."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC)
    new = create(engine, cfg, COUNTED)
    ref = create(engine, cfg, NO_LIGHT)
    try:
        def period(i):
            for c in (new, ref):
                c.run_periods(1)
            assert np.array_equal(new.state_hash(), ref.state_hash()), i
            cn, cr = new.counters(), ref.counters()
            for k in COUNTS:
                assert cn[k] == cr[k], (i, k, cn[k], cr[k])
            sr = look(engine, ref, f"reference, call {i}")
            assert sr["skipped"] == 0, sr
            return look(engine, new, f"call {i}")

        for i in range(8):
            before = period(i)
        assert before["skipped"] > 0 and before["first_dead"] == NEVER, before
        assert before["skipped"] == _abi.debug_light(engine, new._h)["ticks"], before
        at = new.tick
        for c in (new, ref):
            c.kill(1000)
        for i in range(8, 12):
            after = period(i)
            assert after["first_dead"] == after["min_dead"] == at, (at, after)
            assert after["skipped"] == before["skipped"], (before, after)
        dn, dr = dirty(engine, new), dirty(engine, ref)
        assert dn == dr and dn["lister_free_ticks"] > 0, (dn, dr)
        ln = _abi.debug_light(engine, new._h)
        assert ln["p1"] > 0 and ln["sync"] > 0, ln
    finally:
        new.close()
        ref.close()
