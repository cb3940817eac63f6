"""The view census (include/swimhip_census.h, swim_view_census) against rows read one observer at a time.

The expected census is always computed in numpy from rows (census_from_rows): the CPU oracle's row(o) wherever the oracle
runs in lockstep, the engine's own row(o) (swim_read_row, the older readback) at the one size the oracle is too slow for.
Every comparison covers the four arrays and the totals. The tile sizes come from the header's SWIM_CENSUS_TILE_* (mirrored
in _abi): a workgroup counts 128 observers x 4096 subjects, a lane 16 subjects, a wave 1024."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from swimhip import ClusterConfig, SimConfig, SimulatedCluster, _abi
from swimhip.census import combine

from parity_util import run_lockstep

pytestmark = pytest.mark.gpu

KEY8, KEY32, IMPLICIT = _abi.CENSUS_PATH_KEY8, _abi.CENSUS_PATH_KEY32, _abi.CENSUS_PATH_IMPLICIT
ROW_BYTES = {KEY8: 1, KEY32: 4}  # key bytes per record of the plane a path streams


def census_from_rows(cluster, observers):
    """The census of `observers` (ids) computed from cluster.row(o): a dict of the four arrays, the totals and the
    number of held records whose key does not fit the 8-bit shadow (the escapes the KEY8 path re-reads as u32)."""
    n = cluster.n
    bs, bo = np.zeros((n, 4), np.uint32), np.zeros((n, 4), np.uint32)
    mn, mx = np.full(n, 0xFFFFFFFF, np.uint64), np.zeros(n, np.uint64)
    esc = 0
    for o in observers:
        row = cluster.row(o)
        st, inc = ((row >> np.uint64(32)) & np.uint64(3)).astype(np.int64), row & np.uint64(0xFFFFFFFF)
        key = (inc << np.uint64(2)) | st.astype(np.uint64)
        held = st != _abi.ST_ABSENT
        for k in range(4):
            bs[:, k] += st == k
            bo[o, k] = np.count_nonzero(st == k)
        mn = np.where(held, np.minimum(mn, key), mn)
        mx = np.where(held, np.maximum(mx, key), mx)
        esc += int(np.count_nonzero(held & (key >= 0xFF)))
    return dict(n_observers=len(observers), by_subject=bs, by_observer=bo, key_min=mn.astype(np.uint32),
                key_max=mx.astype(np.uint32), records=bo.sum(axis=0, dtype=np.uint64), escapes=esc,
                tick=cluster.tick)


def check(got, want, where, path=None):
    """Every array and total of a ViewCensus against census_from_rows' dict."""
    assert got.tick == want["tick"], where
    assert got.n_observers == want["n_observers"], (where, got.n_observers, want["n_observers"])
    for f in ("by_subject", "by_observer", "key_min", "key_max"):
        a, b = getattr(got, f), want[f]
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{where}: {f} differs at {bad[:6].tolist()}: got {a[tuple(bad[0])]} want {b[tuple(bad[0])]}"
    assert got.records.tolist() == want["records"].tolist(), where
    assert np.array_equal(got.records, got.by_observer.sum(axis=0)), where
    if path is not None:
        assert got.path == path, (where, got.path)
    n = len(want["key_min"])
    if got.path == IMPLICIT:
        assert got.bytes_read == 0, where
    else:
        esc = want["escapes"] if got.path == KEY8 else 0
        assert got.bytes_read == want["n_observers"] * n * ROW_BYTES[got.path] + 4 * esc, (where, got.bytes_read)


def mask_of(n, ids):
    m = np.zeros(n, np.uint8)
    m[list(ids)] = 1
    return m


def create(engine, cfg, env=None):
    """A cluster created with the environment settings env (read at create only)."""
    env = env or {}
    os.environ.update(env)
    try:
        return SimulatedCluster(engine, cfg)
    finally:
        for k in env:
            os.environ.pop(k, None)


# ---- the fault scenario of the small shapes and of the sharded handles ------------------------------------------

# A ping every 8 ticks and a suspicion of ceilLog2(n) pings (56 ticks at n = 100, 72 at 257): the killed members are
# removed within ~90 ticks of their kill. (The ping-req path takes four hops of one tick: a shorter interval than
# timeout + 4 ticks makes every lost ping a false suspicion, and the CPU oracle crawls under the gossip that follows.)
FAST = ClusterConfig(suspicionMult=1, pingInterval=800, pingTimeout=400, syncInterval=2000, gossipRepeatMult=1)
LOSS = 5  # per cent: enough for false suspicions and refutations, few enough of them for the oracle at 257 members


def scenario_cfg(n, **kw):
    return SimConfig(n_members=n, cluster=FAST, seed=0xCE5 + n, gossip_slot_cap=1 << 12, pending_fetch_cap=1024, **kw)


class Seen:
    """Which statuses the compared (counted) rows held over a run, from the reference rows."""

    def __init__(self):
        self.st = np.zeros(4, np.uint64)

    def add(self, want):
        self.st += want["records"]


def stopped(o, leaver):
    """Whether the leaver has stopped, from the oracle: a leaver holds its own leave gossip until the tick it sweeps it,
    and stops (its gossips are cleared) at the end of that tick."""
    return len(o.gossips(leaver)) == 0


def run_scenario(o, e, compare, chunk=10):
    """PRECONVERGED under loss: two kills, a partition set and healed, one leave. compare(running, where) is called
    after every chunk with the members that run (the test did the kills; the leaver's stop is read from the oracle), and
    with dead_in = the leaver on the tick after its leave, when its own record is DEAD. Returns (killed, leaver)."""
    n = o.n
    killed, leaver = (1, n - 2), 2
    running = set(range(n))
    both = (o, e)

    def chunks(ticks, where):
        for _ in range(ticks // chunk):
            run_lockstep(o, e, chunk, chunk, where, events=False)
            compare(sorted(running), where)

    for c in both:
        c.set_default_loss(LOSS)
    chunks(10, "loss")
    for c in both:
        for m in killed:
            c.kill(m)
    running -= set(killed)
    compare(sorted(running), "just killed")  # a killed member is not running from the kill call on
    chunks(20, "two kills")
    for c in both:
        c.partition([0 if m < n - 3 else 1 for m in range(n)])
    chunks(20, "partition")  # healed before the suspicions across it run out
    for c in both:
        c.unblock_all()
    chunks(20, "healed")
    for c in both:
        c.leave(leaver)
    run_lockstep(o, e, 1, 1, "leave", events=False)
    assert not stopped(o, leaver)
    compare(sorted(running), "the tick after leave", dead_in=leaver)
    done = False
    for _ in range(16):  # until the chunk after the one in which the leaver stopped
        run_lockstep(o, e, chunk, chunk, "leaving", events=False)
        was = done
        if not done and stopped(o, leaver):
            running.discard(leaver)
            done = True
        compare(sorted(running), "leaving")
        if was:
            break
    assert done, "the leaver never stopped"
    return killed, leaver


@pytest.mark.parametrize("n", [5, 63, 64, 65, 100, 257])
def test_small_shapes_against_the_oracle(oracle, engine, n):
    """n = 100: NS = 104 and NS8 = 112, both padded; 63 / 64 / 65 straddle a wave's lanes; 5 is less than one lane's 16
    subjects. At every chunk: observers = None (every running member) and a fixed pseudo-random mask with a killed one."""
    cfg = scenario_cfg(n)
    o, e = SimulatedCluster(oracle, cfg), SimulatedCluster(engine, cfg)
    rng = np.random.default_rng(n)
    fixed = rng.random(n) < 0.4
    fixed[1] = True  # member 1 is killed: an explicit mask is taken literally, its frozen row is counted
    fixed_ids = [int(m) for m in np.nonzero(fixed)[0]]
    seen, dead_seen = Seen(), []

    def compare(running, where, dead_in=None):
        want = census_from_rows(o, running)
        check(e.census(), want, f"n={n} {where}: None", KEY8)
        seen.add(want)
        ids = sorted(set(fixed_ids) | ({dead_in} if dead_in is not None else set()))
        want = census_from_rows(o, ids)
        check(e.census(mask_of(n, ids)), want, f"n={n} {where}: mask", KEY8)
        seen.add(want)
        if dead_in is not None:
            dead_seen.append(int(want["by_observer"][dead_in, _abi.ST_DEAD]))

    killed, leaver = run_scenario(o, e, compare)
    # not vacuous: the compared rows held every status (DEAD: the leaver's own record, through the explicit mask)
    assert seen.st[_abi.ST_ABSENT] and seen.st[_abi.ST_ALIVE] and seen.st[_abi.ST_SUSPECT], seen.st
    assert dead_seen == [1], dead_seen
    # after the leaver stopped: None counts the n - 3 others, exactly as their explicit mask does
    rest = sorted(set(range(n)) - set(killed) - {leaver})
    a, b = e.census(), e.census(mask_of(n, rest))
    assert a.n_observers == n - 3
    check(b, census_from_rows(o, rest), f"n={n} the end: mask of the rest", KEY8)
    for f in ("by_subject", "by_observer", "key_min", "key_max", "records"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert (a.n_observers, a.bytes_read, a.tick) == (b.n_observers, b.bytes_read, b.tick)
    o.close()
    e.close()


def test_dormant_members(oracle, engine):
    """COLD_JOIN with dormant members: None counts exactly the started ones, before and after a swim_join."""
    n = 40
    cfg = SimConfig(n_members=n, cluster=ClusterConfig(seedMembers=[0]), init_mode=_abi.INIT_COLD_JOIN, n_dormant=4)
    o, e = SimulatedCluster(oracle, cfg), SimulatedCluster(engine, cfg)
    running = list(range(n - 4))
    check(e.census(), census_from_rows(o, running), "dormant: tick 0", KEY8)
    run_lockstep(o, e, 30, 10, "dormant: before the join", events=False)
    want = census_from_rows(o, running)
    check(e.census(), want, "dormant: before the join", KEY8)
    assert want["records"][_abi.ST_ABSENT] > 0  # nobody holds the dormant members
    for c in (o, e):
        c.join(n - 2, [0])
    running.append(n - 2)
    check(e.census(), census_from_rows(o, running), "dormant: just joined", KEY8)
    run_lockstep(o, e, 40, 10, "dormant: after the join", events=False)
    got = e.census()
    check(got, census_from_rows(o, running), "dormant: after the join", KEY8)
    assert got.n_observers == n - 3
    check(e.census(np.ones(n, np.uint8)), census_from_rows(o, range(n)), "dormant: every row", KEY8)
    o.close()
    e.close()


@pytest.mark.parametrize("env,path", [(None, KEY8), ({"SWIM_NO_K8": "1"}, KEY32)], ids=["key8", "key32"])
def test_escape_boundary(oracle, engine, env, path):
    """The movers of test_key8_escape_boundary: incarnations 60-63 bumped across 62 / 63 / 64 under loss and SYNCs every
    tick. A shadow byte of 0xFF reads as DEAD in its low bits: the census must take those records from the u32 keys."""
    n = 96
    cfg = SimConfig(n_members=n, cluster=ClusterConfig(syncInterval=1000), seed=0x8B)
    o, e = SimulatedCluster(oracle, cfg), create(engine, cfg, env)
    lib = {id(o): oracle, id(e): engine}
    movers = (3, 31, 32, 63, 64, 95)
    for c in (o, e):
        c.set_default_loss(10)
        for j, m in enumerate(movers):
            assert _abi.debug_set_incarnation(lib[id(c)], c._h, m, 60 + j % 4) == 0
    everyone, some = list(range(n)), [m for m in range(n) if m % 3 != 1]
    escaped_alive = 0
    for step in range(5):
        if step:
            for c in (o, e):
                for m in movers[(step - 1) % 2::2]:
                    c.update_incarnation(m)
        run_lockstep(o, e, 30, 10, f"bump {step}", events=False)
        want = census_from_rows(o, everyone)
        check(e.census(), want, f"escape {path} bump {step}: None", path)
        check(e.census(mask_of(n, some)), census_from_rows(o, some), f"escape {path} bump {step}: mask", path)
        # ALIVE records at incarnation >= 64: escaped bytes whose low bits say DEAD
        escaped_alive += int(np.count_nonzero((want["key_max"] >= 0xFF) & ((want["key_max"] & 3) == _abi.ST_ALIVE)))
        if step == 4:
            assert want["escapes"] > 0 and want["records"][_abi.ST_DEAD] == 0
    assert escaped_alive > 0
    o.close()
    e.close()


TILE_ROWS, TILE_COLS = _abi.CENSUS_TILE_ROWS, _abi.CENSUS_TILE_COLS  # 128 observers x 4096 subjects per workgroup


@pytest.mark.parametrize("env,path", [(None, KEY8), ({"SWIM_NO_K8": "1"}, KEY32)], ids=["key8", "key32"])
def test_tile_boundaries(engine, env, path):
    """One column span + 37 subjects and 33 row tiles, engine only: the killed subjects sit at a tile's first lane, its
    last column and in the 37-subject tail, and are SUSPECT at some observers only, so the tiles' partial sums differ."""
    n = TILE_COLS + 37
    assert n <= 4200 and n > TILE_ROWS
    killed = (5, TILE_COLS - 1, TILE_COLS + 4)
    c = create(engine, SimConfig(n_members=n, seed=0x711E), env)
    c.set_default_loss(10)
    for m in killed:
        c.kill(m)
    probe = list(range(0, n, 61))
    c.step(6)
    for _ in range(40):  # until a sample of rows shows a killed subject SUSPECT at some but not all observers
        st = np.stack([(c.row(o)[list(killed)] >> np.uint64(32)) & np.uint64(3) for o in probe])
        frac = (st == _abi.ST_SUSPECT).mean(axis=0)
        if np.any((frac > 0.2) & (frac < 0.8)):
            break
        c.step(1)
    running = [m for m in range(n) if m not in killed]
    want = census_from_rows(c, running)
    sus = want["by_subject"][list(killed), _abi.ST_SUSPECT]
    assert np.any((sus > 0) & (sus < len(running))), sus
    check(c.census(), want, f"tiles {path}: None", path)
    half = [m for m in range(n) if (m * 7) % 5 < 2 or m in killed]
    check(c.census(mask_of(n, half)), census_from_rows(c, half), f"tiles {path}: mask", path)
    c.close()


@pytest.mark.parametrize("world", [2, 3, 0], ids=["W2", "W3", "n_gpus2"])
def test_sharded(oracle, engine, world):
    """Row shards (ThreadShardGroup, W = 2 and 3) and an n_gpus = 2 handle (world 0) under the scenario of the small
    shapes: each shard's partial is zero outside its range and the partials combine to the whole."""
    from swimhip.shard import ThreadShardGroup
    n = 100
    cfg = scenario_cfg(n)
    o = SimulatedCluster(oracle, cfg)
    e = ThreadShardGroup(engine, cfg, world) if world else SimulatedCluster(engine, dataclasses.replace(cfg, n_gpus=2))
    fixed_ids = [1] + [m for m in range(n) if (m * 11) % 7 < 3]
    seen = Seen()

    def compare(running, where, dead_in=None):
        for ids, mask in ((running, None), (sorted(set(fixed_ids) | ({dead_in} if dead_in is not None else set())), 1)):
            want = census_from_rows(o, ids)
            seen.add(want)
            mk = None if mask is None else mask_of(n, ids)
            check(e.census(mk), want, f"W={world} {where}", KEY8)
            if world:  # the partials themselves
                parts = [s.census(mk) for s in e.shards]
                for s, p in zip(e.shards, parts):
                    assert not p.by_observer[:s.lo].any() and not p.by_observer[s.hi:].any(), (world, where)
                    assert p.n_observers == len([m for m in ids if s.lo <= m < s.hi])
                check(combine(parts), want, f"W={world} {where}: combined", KEY8)

    run_scenario(o, e, compare)
    assert seen.st[_abi.ST_ABSENT] and seen.st[_abi.ST_SUSPECT] and seen.st[_abi.ST_DEAD], seen.st
    e.close()
    o.close()


def test_implicit_views(engine):
    """RUMOR mode with implicit views: every row is the PRECONVERGED row, the answer is closed form (no bytes read)."""
    n = 300
    c = SimulatedCluster(engine, SimConfig(n_members=n, mode=_abi.MODE_RUMOR, churn_per_period=3, implicit_views=True))
    c.run_periods(2)
    c.kill(17)
    c.run_periods(1)
    running = [m for m in range(n) if m != 17]
    got = c.census()
    check(got, census_from_rows(c, running), "implicit: None", IMPLICIT)
    assert got.n_observers == n - 1 and got.bytes_read == 0
    ids = [17] + list(range(4, n, 7))  # the killed member's frozen row and 43 others
    check(c.census(mask_of(n, ids)), census_from_rows(c, ids), "implicit: mask", IMPLICIT)
    assert c.census().converged().all()
    c.close()


def test_no_side_effects(engine):
    """Two handles with the same config, SYNC every tick (lister and dirty masks busy), loss and a kill: one takes a full
    census after every chunk, the other none; everything the simulation computes and counts is identical."""
    cfg = SimConfig(n_members=200, cluster=ClusterConfig(syncInterval=100), seed=0x51DE)
    keys = ["record_compares", "row_writes", "messages", "gossip_messages", "events", "messages_lost", "gossips_created",
            "sync_merges", "diff_msgs", "diff_msgs_total", "diff_key_bytes", "diff_key_bytes_total", "ack_resolved",
            "ack_resolved_total"]
    out = []
    for take in (True, False):
        c = SimulatedCluster(engine, cfg)
        c.set_default_loss(10)
        c.kill(7)
        for _ in range(8):
            c.step(10)
            if take:
                got = c.census()
                assert got.n_observers == 199
                c.census(mask_of(200, range(0, 200, 3)))
        if take:
            assert _abi.debug_dirty_check(engine, c._h) == 0
        ctr = c.counters()
        out.append((c.state_hash(), {k: ctr[k] for k in keys}, _abi.debug_diff_dirty(engine, c._h)))
        c.close()
    assert np.array_equal(out[0][0], out[1][0]), "state hashes differ"
    assert out[0][1] == out[1][1]
    assert out[0][2] == out[1][2]


def test_arguments(engine):
    n = 70
    c = SimulatedCluster(engine, scenario_cfg(n))
    c.set_default_loss(10)
    c.kill(3)
    c.step(40)
    _abi.bind_census(engine)
    assert engine.swim_view_census(c._h, None) == _abi.SWIM_EINVAL
    assert engine.swim_view_census(None, C.byref(_abi.SwimCensus())) == _abi.SWIM_EINVAL
    full = c.census()
    assert full.records[_abi.ST_SUSPECT] + full.records[_abi.ST_ABSENT] > 0
    P = C.POINTER(C.c_uint32)

    def call(**outs):
        s = _abi.SwimCensus()
        for k, a in outs.items():
            setattr(s, k, a.ctypes.data_as(P))
        assert engine.swim_view_census(c._h, C.byref(s)) == 0
        assert (int(s.tick), int(s.n_observers), list(s.records), int(s.bytes_read), int(s.path)) == \
            (full.tick, full.n_observers, full.records.tolist(), full.bytes_read, full.path), outs.keys()

    call()  # all outputs null: the totals only
    for name, shape in (("by_subject", (n, 4)), ("by_observer", (n, 4)), ("key_min", n), ("key_max", n)):
        a = np.full(shape, 0xABABABAB, np.uint32)
        call(**{name: a})
        assert np.array_equal(a, getattr(full, name)), name
    part = c.census(by_subject=False, keys=False)
    assert part.by_subject is None and part.key_min is None and np.array_equal(part.by_observer, full.by_observer)
    c.close()
