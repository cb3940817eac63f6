"""The member kernel's light path (csrc/member_light.h, DESIGN.md §3.2 "Round 12") against the general body.

On one GPU the steady state's member-ticks (a ping, its hop, its ack, one or two SYNC / SYNC_ACK receipts with nothing
to merge, the periodic SYNC send) run on a path that loads in rounds, decides in registers and commits only then;
everything else falls back to member_tick_body before any store. SWIM_NO_LIGHT=1 (read at create) runs every
member-tick through the general body: the reference here. Each scenario drives the default build and the reference in
lockstep, one tick per step, and compares the state hashes of every component after every tick, then the full event
streams, swim_counters, the emulator counters, swim_debug_diff_dirty's lister counters and every member's request
counters (correlation ids, SYNC sequence, FD period, pending paths and subscriptions). A last scenario steps whole
periods at a time, so that the speculative and lister-free batches run through the path as well.

Sizes: 66 members (two waves, the second partial), 96, and 300 (two blocks). swim_debug_light says what ran where, so
that no scenario passes by never taking the path (or, where it must not be taken, by taking it)."""
from dataclasses import replace

import ctypes as C

import numpy as np
import pytest

from swimhip import ClusterConfig, SimConfig, _abi

from test_gpu_diff_dirty import FAST_SYNC, FAULT_CAPS, create, dirty

pytestmark = pytest.mark.gpu

# both handles count their fallbacks (SWIM_FALLBACKS): a handle without the light path counts the general body's
# member-ticks only then (swim_debug_light), and the capacity-fallback counters are compared as well
COUNTED = {"SWIM_FALLBACKS": "1"}
NO_LIGHT = {"SWIM_NO_LIGHT": "1", **COUNTED}
SIZES = (66, 96, 300)
LIGHT = ("ticks", "fd", "p1", "sync")
FALLBACKS = ("fb_reshuffle", "fb_send", "fb_payloads", "fb_candidates", "fb_busy", "fb_status", "fb_other")
# swim_counters that are counts (the others are times and sizes)
COUNTS = ("record_compares", "row_writes", "messages", "gossip_messages", "events", "messages_lost", "gossips_created",
          "sync_merges", "ack_resolved_total", "diff_msgs_total")
# (with link delays, which payloads are streamed depends on which sender's pin came first)
COUNTS_NO_DELAY = ("diff_key_bytes_total",)
# swim_debug_diff_dirty's entries that do not depend on which payloads raced for a pin (they do with link delays)
DD_HOST = ("rebases", "diff_elided", "diff_halts", "lister_free_ticks", "lister_free_stops")


def all_events(c):
    out = []
    while True:
        ev = c.events()
        if not ev:
            return out
        out += ev


def scalars(c):
    """[n][8] per member: cidCnt, syncSeq, gCounter, nextSync, fdPeriod, gossip period, npath, nsub (a debugging aid of
    the library, outside the ABI headers)."""
    fn = c.lib.swimdbg_scalars
    fn.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    out = np.zeros((c.n, 8), dtype=np.uint64)
    for m in range(c.n):
        assert fn(c._h, m, out[m].ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    return out


def lockstep(engine, cfg, periods, script=None, before=None, chunk=1, name="", dd_all=True, env=None):
    """The default build and the SWIM_NO_LIGHT=1 reference through the same calls: `before(c)` once, `script(c, t)`
    before the step that starts at tick t, `chunk` ticks per step. Returns swim_debug_light of both."""
    cfg = replace(cfg, record_events=True, emulator_counters=True)
    new, ref = create(engine, cfg, {**COUNTED, **(env or {})}), create(engine, cfg, {**NO_LIGHT, **(env or {})})
    try:
        for c in (new, ref):
            if before:
                before(c)
        for t in range(0, 10 * periods, chunk):
            for c in (new, ref):
                if script:
                    script(c, t)
                c.step(chunk)
            hn, hr = new.state_hash(), ref.state_hash()
            if not np.array_equal(hn, hr):
                m, w = np.argwhere(hn != hr)[0]
                raise AssertionError(f"{name}: state hash differs after tick {t + chunk - 1} at member {m} word {w}")
        en, er = all_events(new), all_events(ref)
        assert en == er, f"{name}: event streams differ ({len(en)} vs {len(er)})"
        cn, cr = new.counters(), ref.counters()
        for k in COUNTS + (COUNTS_NO_DELAY if dd_all else ()):
            assert cn[k] == cr[k], (name, k, cn[k], cr[k])
        assert np.array_equal(new.emulator_counters(), ref.emulator_counters()), name
        assert np.array_equal(scalars(new), scalars(ref)), name
        assert _abi.debug_fallbacks(engine, new._h) == _abi.debug_fallbacks(engine, ref._h), name
        dn, dr = dirty(engine, new), dirty(engine, ref)
        for k in (dn if dd_all else DD_HOST):
            assert dn[k] == dr[k], (name, k, dn, dr)
        ln, lr = _abi.debug_light(engine, new._h), _abi.debug_light(engine, ref._h)
        print(f"{name}: light {ln}; reference general {lr['general']}", flush=True)
        # the reference never takes the path
        assert lr["on"] == 0 and all(lr[k] == 0 for k in LIGHT + FALLBACKS), (name, lr)
        assert lr["general"] > 0
        # a fallback runs the general body; every member-tick ran on exactly one of the two
        assert ln["ticks"] + ln["general"] == lr["general"], (name, ln, lr)
        return ln, lr
    finally:
        new.close()
        ref.close()


@pytest.mark.parametrize("n,periods", [(96, 30), (300, 30), (66, 70)])
def test_clean_default_config(engine, n, periods):
    """(a) 70 periods at 66 members take pingIdx across fdLen = 65: the reshuffle fallback."""
    ln, _ = lockstep(engine, SimConfig(n_members=n), periods, name=f"clean {n}")
    assert ln["on"] == 1
    assert ln["fd"] > 0 and ln["p1"] > 0 and ln["sync"] > 0
    # per member and period three FD ticks are light; the general body is left with the gossip rounds of the start
    if n == 300:
        assert ln["ticks"] >= 9 * ln["general"], ln
    for k in FALLBACKS:
        if k not in ("fb_reshuffle", "fb_payloads"):
            assert ln[k] == 0, (k, ln)
    if n == 66:
        assert ln["fb_reshuffle"] > 0, ln


@pytest.mark.parametrize("n", SIZES)
def test_fast_sync(engine, n):
    """(b) a SYNC every period: SYNC and SYNC_ACK receipts in every tick, some receivers with two payloads in one."""
    ln, _ = lockstep(engine, SimConfig(n_members=n, cluster=FAST_SYNC), 30, name=f"fast sync {n}")
    assert ln["p1"] > 0 and ln["sync"] > 0 and ln["fb_payloads"] > 0, ln


# The member kernel takes the light path only in its single launch of a tick (BODY_FULL). A tick that follows a gossip
# plane runs the split launches, whose bodies are the general one. Under lasting loss some gossip is always in flight:
# measured on MI355X, 300 ticks at 15 % loss throughout leave 9 (66 members), 193 (96) and 48 (300) light member-ticks,
# all before the first suspicion spreads (test_lasting_loss keeps that run for identity). An ack can meet a SUSPECT row
# on a light tick only when the suspected member is alive and no gossip about it is left, and neither lasting loss nor
# a kill gives that: the refutation follows the suspicion at once, and a dead member sends no ack. So (c) and (d) each
# go on, after their own faults, with a partition of the two halves that lasts until the suspicions' gossip has
# drained (measured: the light path resumes ~210 ticks after the partition at 66 and 96 members, ~280 at 300, and the
# suspicion timeouts fire after 350 / 450) and then heals: the first acks across find the other half SUSPECT. With the
# default SYNC interval: at a SYNC every period the rows were repaired before an ack met one (0 hits measured).
# At 300 members with the default interval a periodic SYNC crosses the healed partition in nearly every tick, its
# receiver refutes its own SUSPECT record, and the tick the first acks arrive in is already a split one (0 hits measured
# at heals of 400, 440 and 480): there the SYNC interval is 120 s, which gives the SYNC rate per tick of the small sizes.
HEAL = {66: 320, 96: 320, 300: 400}  # the tick of unblockAll
SYNC_MS = {66: 30_000, 96: 30_000, 300: 120_000}


def faults_then_partition(n, faults, at):
    half = (np.arange(n) % 2).astype(np.uint32)

    def script(c, t):
        for f in faults.get(t, ()):
            f(c)
        if t == at:
            c.partition(half)
        elif t == HEAL[n]:
            c.unblock_all()
    return script


@pytest.mark.parametrize("n", SIZES)
def test_loss(engine, n):
    """(c) 15 % loss for five periods: lost pings, ping-reqs, timeouts, SUSPECT rows and the SYNC an ALIVE verdict on
    one sends (in split ticks, through the general body in both runs); then the partition that heals (above)."""
    faults = {0: [lambda c: c.set_default_loss(15)], 50: [lambda c: c.set_default_loss(0)]}
    ln, _ = lockstep(engine, SimConfig(n_members=n, cluster=ClusterConfig(syncInterval=SYNC_MS[n]), **FAULT_CAPS),
                     HEAL[n] // 10 + 4, script=faults_then_partition(n, faults, 60), name=f"loss {n}")
    assert ln["fd"] > 0 and ln["p1"] > 0 and ln["fb_send"] > 0 and ln["fb_status"] > 0, ln


@pytest.mark.parametrize("n", SIZES)
def test_kills(engine, n):
    """(d) three kills mid-run, on consecutive ticks, so that pings, hops, acks, SYNCs and SYNC_ACKs are in flight to
    and from the members that die: dead ping targets (the failed-send fallback, for as long as the lists hold them), a
    dead SYNC sender and receiver, a dead issuer with a hop in flight; then the partition that heals (above)."""
    faults = {83: [lambda c: c.kill(5)], 84: [lambda c: c.kill(n - 2)], 85: [lambda c: c.kill(n // 2)]}
    ln, _ = lockstep(engine, SimConfig(n_members=n, cluster=ClusterConfig(syncInterval=SYNC_MS[n]), **FAULT_CAPS),
                     HEAL[n] // 10 + 4, script=faults_then_partition(n, faults, 100), name=f"kills {n}")
    assert ln["fd"] > 0 and ln["p1"] > 0 and ln["fb_send"] > 0 and ln["fb_status"] > 0, ln


@pytest.mark.parametrize("n", SIZES)
def test_lasting_loss(engine, n):
    """(c) as the issue states it, 15 % loss throughout: few member-ticks are light (the ticks after a gossip plane run
    the split launches), and those run beside SUSPECT rows, live timers, ping-req subscriptions and gossip in flight.
    Identity must hold however few they are."""
    ln, _ = lockstep(engine, SimConfig(n_members=n, cluster=FAST_SYNC, **FAULT_CAPS), 30,
                     before=lambda c: c.set_default_loss(15), name=f"lasting loss {n}")
    assert ln["on"] == 1 and ln["ticks"] > 0, ln


@pytest.mark.parametrize("n", [96, 300])
def test_two_payloads_under_mq_cap_one(engine, n):
    """SWIM_CAPS mq=1: P1 sorts one message in registers and takes its list-walk path for two, counting FB_MQ; the
    light path must leave those receivers to it (the capacity-fallback counters are compared)."""
    ln, _ = lockstep(engine, SimConfig(n_members=n, cluster=FAST_SYNC), 12, name=f"mq=1 {n}", env={"SWIM_CAPS": "mq=1"})
    assert ln["p1"] > 0 and ln["fb_payloads"] > 0, ln


@pytest.mark.parametrize("n", SIZES)
def test_host_requests(engine, n):
    """(e) updateIncarnation and leave mid-run: the gossip plane runs, and the light path resumes afterwards."""
    seen = {}

    def script(c, t):
        if t == 42:
            c.update_incarnation(7)
            c.update_incarnation(n - 1)
        elif t == 57:
            c.leave(11)
        elif t == 300 and c not in seen:
            seen[c] = _abi.debug_light(engine, c._h)["ticks"]

    ln, _ = lockstep(engine, SimConfig(n_members=n), 40, script=script, name=f"requests {n}")
    resumed = ln["ticks"] - max(seen.values())
    assert resumed >= 2 * n * 10, (resumed, ln)  # ten more periods, two light ticks or more per member in each


@pytest.mark.parametrize("n", SIZES)
def test_per_member_config(engine, n):
    """(f) two ping intervals in one cluster (swim_set_member_config)."""
    slow = ClusterConfig(pingInterval=2000, pingTimeout=700)

    def before(c):
        for m in range(0, n, 3):
            c.set_member_config(m, slow)

    ln, _ = lockstep(engine, SimConfig(n_members=n), 20, before=before, name=f"per-member {n}")
    assert ln["fd"] > 0 and ln["fb_other"] == 0, ln


def test_cold_join(engine):
    """(g) a start that is not preconverged: initial syncs, full merges, fetches, then the steady state."""
    cfg = SimConfig(n_members=96, cluster=ClusterConfig(seedMembers=[0]), init_mode=_abi.INIT_COLD_JOIN)
    ln, _ = lockstep(engine, cfg, 20, name="cold join 96")
    assert ln["fd"] > 0 and ln["general"] > 0, ln


@pytest.mark.parametrize("n", SIZES)
def test_link_delays_turn_the_path_off(engine, n):
    """(h) with a link delay set the light path must be off, and the results equal."""
    cfg = SimConfig(n_members=n, cluster=FAST_SYNC, delay_cap_ms=300)
    ln, _ = lockstep(engine, cfg, 20, before=lambda c: c.set_default_link_settings(0, 200), name=f"delays {n}",
                     dd_all=False)
    assert ln["on"] == 0 and all(ln[k] == 0 for k in LIGHT + FALLBACKS), ln


def test_whole_periods_per_step(engine):
    """Ten ticks per step: the speculative batches, and after a clean one the lister-free batches, whose receivers
    count their messages in the lister's place, on the light path too."""
    cfg = SimConfig(n_members=2100, cluster=FAST_SYNC)
    new = create(engine, cfg, COUNTED)
    ref = create(engine, cfg, NO_LIGHT)
    try:
        for c in (new, ref):
            for _ in range(8):
                c.run_periods(1)
        assert np.array_equal(new.state_hash(), ref.state_hash())
        cn, cr = new.counters(), ref.counters()
        for k in COUNTS:
            assert cn[k] == cr[k], (k, cn[k], cr[k])
        dn, dr = dirty(engine, new), dirty(engine, ref)
        assert dn == dr and dn["lister_free_ticks"] > 0, (dn, dr)
        ln = _abi.debug_light(engine, new._h)
        assert ln["p1"] > 0 and ln["sync"] > 0, ln
    finally:
        new.close()
        ref.close()
