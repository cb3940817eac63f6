"""The gossip period (GossipProtocolImpl's `period`) is not stored by the engine: it is derived from the member's
nextGossip and firstGossip (gossip_period, dev_util.h), which only ever advance and are only ever set
together. The oracle keeps the counter itself (gPeriod++ in doSpreadGossip), so after every chunk of a lockstep run
every member's period (word 5 of swimdbg_scalars, which both libraries answer) and all six state-hash words must agree.

Each run steps in chunks of 1, 7, 13 and 30 ticks, over and over: single ticks and speculative batches both run, and
every chunk length crosses gossip boundaries (a round every 2 or 3 ticks)."""
import ctypes as C

import numpy as np
import pytest

from swimhip import ClusterConfig, SimConfig, _abi
from swimhip.cluster import SimulatedCluster
from swimhip.shard import ThreadShardGroup

from parity_util import explain, first_diff, step_both

CHUNKS = (1, 7, 13, 30)


def periods(c, members):
    """The gossip period of each of `members` from handle c (a SimulatedCluster or one shard)."""
    fn = c.lib.swimdbg_scalars
    if fn.argtypes is None:  # bound once per library
        fn.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
        fn.restype = C.c_int
    out = (C.c_uint64 * 8)()
    res = []
    for m in members:
        assert fn(c._h, m, out) == 0, f"swimdbg_scalars({m})"
        res.append(int(out[5]))
    return res


def engine_periods(e, n):
    if isinstance(e, ThreadShardGroup):  # each rank answers for its own members
        res = []
        for s in e.shards:
            res += periods(s, range(s.lo, s.hi))
        return res
    return periods(e, range(n))


def check(o, e, where):
    n = o.n
    po, pe = periods(o, range(n)), engine_periods(e, n)
    bad = [(m, a, b) for m, (a, b) in enumerate(zip(po, pe)) if a != b]
    assert not bad, f"{where}: gossip period (member, oracle, engine) differs: {bad[:8]} ({len(bad)} members)"
    ho, he = o.state_hash(), e.state_hash()
    d = first_diff(ho, he)
    if d is not None:
        m, w, cnt = d
        raise AssertionError(f"{where}: state hash differs at member {m} word {w} ({cnt} words differ); " + explain(o, e, m))
    return po


def run_chunks(o, e, ticks, where, actions=None):
    """`ticks` ticks in chunks of 1, 7, 13, 30, 1, ... (cut at the end and at an action's tick); actions: {tick: fn(c)},
    applied to both before that tick runs. The check after every chunk."""
    actions = dict(actions or {})
    end, i = o.tick + ticks, 0
    while o.tick < end:
        now = o.tick
        if now in actions:
            act = actions.pop(now)
            for c in (o, e):
                act(c)
        stop = min([end] + [t for t in actions if t > now])
        n = min(CHUNKS[i % len(CHUNKS)], stop - now)
        i += 1
        step_both(o, e, n)
        check(o, e, f"{where} tick {o.tick} (chunk of {n})")
    assert not actions, actions


# ---- case 1: N = 96 (more than one wave), COLD_JOIN, two dormant members joined at an odd and an even tick, a user
# gossip (rounds with and without gossips held), a kill and a leave part-way, 10 % loss ----
N1, TICKS1 = 96, 204
JOINS1 = {94: 1, 95: 8}  # member: the tick of its swim_join
KILL1, LEAVE1 = (7, 51), (11, 52)  # (member, tick)


def cfg1(gossip_ms):
    return SimConfig(n_members=N1, cluster=ClusterConfig(seedMembers=[0], gossipInterval=gossip_ms),
                     init_mode=_abi.INIT_COLD_JOIN, n_dormant=len(JOINS1))


def actions1():
    acts = {t: (lambda c, m=m: c.join(m, [0])) for m, t in JOINS1.items()}
    acts[21] = lambda c: c.spread_gossip(5, 0xC0FFEE)
    acts[KILL1[1]] = lambda c: c.kill(KILL1[0])
    acts[LEAVE1[1]] = lambda c: c.leave(LEAVE1[0])
    return acts


@pytest.mark.gpu
@pytest.mark.parametrize("gossip_ms", [200, 300])
def test_cold_join_joins_kill_leave(oracle, engine, gossip_ms):
    cfg = cfg1(gossip_ms)
    o, e = SimulatedCluster(oracle, cfg), SimulatedCluster(engine, cfg)
    for c in (o, e):
        c.set_default_loss(10)
    run_chunks(o, e, TICKS1, f"cold join, gossip every {gossip_ms} ms", actions1())
    p = periods(o, range(N1))
    gt, last = gossip_ms // cfg.tick_ms, TICKS1 - 1
    # a round every gt ticks after the start (tick 0, or the join's); none from the kill's tick on
    assert [p[0], p[94], p[95]] == [last // gt, (last - JOINS1[94]) // gt, (last - JOINS1[95]) // gt], p
    assert p[KILL1[0]] == (KILL1[1] - 1) // gt and 0 < p[LEAVE1[0]] < p[0], p
    e.close()
    o.close()


# ---- case 2: N = 300 (two blocks, the second partly filled), PRECONVERGED, no loss: 60 ticks in one call (the
# lister-free steady state), then an updateIncarnation and more ticks in chunks ----
@pytest.mark.gpu
def test_preconverged_steady_state(oracle, engine):
    cfg = SimConfig(n_members=300)
    o, e = SimulatedCluster(oracle, cfg), SimulatedCluster(engine, cfg)
    step_both(o, e, 60)
    p = check(o, e, "steady state, 60 ticks in one call")
    assert set(p) <= {29, 30}, sorted(set(p))  # a round every 2 ticks from tick 1 or 2
    for c in (o, e):
        c.update_incarnation(123)
    run_chunks(o, e, 20, "after updateIncarnation")
    run_chunks(o, e, 51, "after updateIncarnation, second pass")
    e.close()
    o.close()


# ---- case 3: N = 100 on two row shards over the host transport: each rank's own members ----
@pytest.mark.gpu
def test_two_row_shards(oracle, engine):
    cfg = SimConfig(n_members=100)
    o, e = SimulatedCluster(oracle, cfg), ThreadShardGroup(engine, cfg, 2)
    for c in (o, e):
        c.set_default_loss(10)
    acts = {1: lambda c: c.spread_gossip(60, 7), 8: lambda c: c.kill(20), 21: lambda c: c.update_incarnation(70)}
    run_chunks(o, e, 102, "two row shards", acts)
    e.close()
    o.close()


# ---- case 4: N = 200, RUMOR mode with churn, 40 ticks ----
@pytest.mark.gpu
def test_rumor_mode_churn(oracle, engine):
    cfg = SimConfig(n_members=200, mode=_abi.MODE_RUMOR, churn_per_period=3)
    o, e = SimulatedCluster(oracle, cfg), SimulatedCluster(engine, cfg)
    for c in (o, e):
        c.set_default_loss(5)
    run_chunks(o, e, 40, "rumor + churn", {8: lambda c: c.kill(40), 21: lambda c: c.spread_gossip(17, 99)})
    e.close()
    o.close()


# ---- CPU only: the invariant the derived value rests on, in the oracle alone over case 1's schedule ----
@pytest.mark.parametrize("gossip_ms", [200, 300])
def test_oracle_period_changes_only_with_next_gossip(oracle, gossip_ms):
    """A member's period only changes in a tick in which its nextGossip changes, and then by one. The oracle does not
    expose nextGossip; the ticks at which it changes follow from its schedule rule (Member::start: start + gossip_t,
    then + gossip_t at every tick that equals it, for as long as the member runs): tick k with k > start and
    (k - start) % gossip_t == 0, start = 0 for the initial COLD_JOIN members and the join tick for the others. A member
    that ran the whole time made a round at every one of those ticks."""
    cfg = cfg1(gossip_ms)
    gt = gossip_ms // cfg.tick_ms
    o = SimulatedCluster(oracle, cfg)
    o.set_default_loss(10)
    acts = actions1()
    start = {m: JOINS1.get(m, 0) for m in range(N1)}
    prev = periods(o, range(N1))
    assert prev == [0] * N1
    for k in range(TICKS1):
        if k in acts:
            acts[k](o)
        o.step(1)  # runs tick k
        cur = periods(o, range(N1))
        for m in range(N1):
            due = k > start[m] and (k - start[m]) % gt == 0 and (m not in JOINS1 or k > JOINS1[m])
            assert cur[m] - prev[m] in ((0, 1) if due else (0,)), (m, k, prev[m], cur[m], due)
            if m not in (KILL1[0], LEAVE1[0]) and k >= start[m] and (m not in JOINS1 or k >= JOINS1[m]):
                assert cur[m] == (k - start[m]) // gt, (m, k, cur[m])
        prev = cur
    assert prev[KILL1[0]] == (KILL1[1] - 1) // gt  # no round from the kill's tick on
    assert 0 < prev[LEAVE1[0]] < prev[0]  # the leaver stopped once its own leave gossip was swept
    o.close()
