"""The subject watch (include/swimhip_watch.h: swim_watch_*, swim_run_until) against rows read one observer at a time.

The expected tallies, stamps and verdicts always come from rows through tests/watch_ref.py: the CPU oracle's rows after
every tick wherever the oracle runs (the engine follows the same script one tick per step), the engine's own row() at the
one larger size. A watch's block is SWIM_WATCH_BLOCK_ROWS observers (one per lane); the shapes straddle a wave's 64 lanes
and one block."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from swimhip import ClusterConfig, SimConfig, SimulatedCluster, _abi
from swimhip.cluster import SwimError

import watch_ref as ref

pytestmark = pytest.mark.gpu

KEY8, KEY32 = _abi.CENSUS_PATH_KEY8, _abi.CENSUS_PATH_KEY32
BLOCK = _abi.WATCH_BLOCK_ROWS
NEVER = _abi.WATCH_NEVER
P = C.POINTER(C.c_uint32)
# A ping every 8 ticks and a suspicion of ceilLog2(n) pings: a killed member is suspected everywhere within ~35 ticks
# and removed everywhere within ~90 (n <= 300), so 120 ticks after the kill cover both.
FAST = ClusterConfig(suspicionMult=1, pingInterval=800, pingTimeout=400, syncInterval=2000, gossipRepeatMult=1)
KILLED, LEAD, TICKS = 1, 10, 120
PARITY_KEYS = ["record_compares", "row_writes", "messages", "gossip_messages", "events", "messages_lost",
               "gossips_created", "sync_merges"]


def cfg_of(n, **kw):
    return SimConfig(n_members=n, cluster=FAST, seed=0xA7C + n, gossip_slot_cap=1 << 12, pending_fetch_cap=1024, **kw)


def create(engine, cfg, env=None):
    """A cluster created with the environment settings env (read at create only)."""
    env = env or {}
    os.environ.update(env)
    try:
        return SimulatedCluster(engine, cfg)
    finally:
        for k in env:
            os.environ.pop(k, None)


def all_rows(c):
    return np.stack([c.row(o) for o in range(c.n)])


def start(c, loss=0):
    """The script's head: LEAD ticks, then the kill."""
    if loss:
        c.set_default_loss(loss)
    c.step(LEAD)
    c.kill(KILLED)
    return c


_TRACES = {}


def oracle_trace(oracle, n, loss=0, keep=False):
    """[(tick, rows [n, n])] of the oracle after each of the TICKS ticks that follow the kill. Computed once per (n, loss)
    where several tests share it (keep), and never changed."""
    if (n, loss) in _TRACES:
        return _TRACES[(n, loss)]
    o = start(SimulatedCluster(oracle, cfg_of(n)), loss)
    out = []
    for _ in range(TICKS):
        o.step(1)
        rows = all_rows(o)
        rows.setflags(write=False)
        out.append((o.tick, rows))
    o.close()
    if keep:
        _TRACES[(n, loss)] = out
    return out


def first_met(trace, cond, ids, subjects, inc_target=None):
    """Ticks after the kill at which the oracle's rows first meet cond over observers ids (None: never in the trace)."""
    for i, (_, rows) in enumerate(trace):
        t = ref.tally(rows, ids, subjects)
        if ref.met(cond, t["counts"], t["key_min"], t["key_max"], inc_target):
            return i + 1
    return None


def mask_of(n, ids):
    m = np.zeros(n, np.uint8)
    m[list(ids)] = 1
    return m


def same_tally(got, want, tick, where):
    assert got.tick == tick, (where, got.tick, tick)
    assert got.n_observers == want["n_observers"], (where, got.n_observers, want["n_observers"])
    for f in ("counts", "key_min", "key_max"):
        a, b = getattr(got, f), want[f]
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{where}: {f} differs at {bad[:6].tolist()}: got {a[tuple(bad[0])]} want {b[tuple(bad[0])]}"


def same_as_census(c, got, mask, subjects, where, path=None):
    """On the same handle at the same tick: the sample equals census(mask) restricted to the subjects."""
    cen = c.census(mask, by_observer=False)
    assert (got.tick, got.n_observers) == (cen.tick, cen.n_observers), where
    assert np.array_equal(got.counts, cen.by_subject[subjects]), where
    assert np.array_equal(got.key_min, cen.key_min[subjects]), where
    assert np.array_equal(got.key_max, cen.key_max[subjects]), where
    assert got.path == cen.path and (path is None or got.path == path), (where, got.path)


def same_stamps(got, want, where):
    for name in ref.STAMPS:
        bad = np.argwhere(got[name] != want[name])
        assert len(bad) == 0, (f"{where}: stamps {name} differ at {bad[:6].tolist()}: got "
                               f"{got[name][tuple(bad[0])]} want {want[name][tuple(bad[0])]}")


class Watched:
    """One watch on e, its reference stamps, and which statuses its compared columns held."""

    def __init__(self, e, n, subjects, ids=None, inc_target=None):
        self.subjects, self.ids = list(subjects), ids
        self.mask = None if ids is None else mask_of(n, ids)
        self.inc = inc_target
        self.w = e.watch(self.subjects, inc_target=inc_target, observers=self.mask)
        self.ref = ref.StampRef(n, self.subjects, inc_target)
        self.seen = np.zeros(4, np.uint64)

    def compare(self, tick, rows, running, where):
        ids = self.ids if self.ids is not None else running
        want = ref.tally(rows, ids, self.subjects)
        got = self.w.sample()
        same_tally(got, want, tick, where)
        self.ref.feed(tick, rows, ids)
        self.seen += want["counts"].sum(axis=0, dtype=np.uint64)
        return got, want


def subject_sets(n):
    """{the killed member}; four subjects out of order (a neighbour of the killed one among them); as many as fit, up to
    256, in a scrambled order."""
    perm = np.random.default_rng(n).permutation(n)[:_abi.WATCH_MAX_SUBJECTS]
    if KILLED not in perm:
        perm[0] = KILLED
    return [[KILLED], [KILLED, 0, n - 1, 2], [int(s) for s in perm]]


# ---- 1, 2: small shapes against the oracle, and against the census on the same handle ----------------------------

@pytest.mark.parametrize("n,loss", [(5, 0), (63, 0), (64, 0), (65, 0), (100, 0), (100, 5), (BLOCK + 1, 0)])
def test_small_shapes_against_the_oracle(oracle, engine, n, loss):
    trace = oracle_trace(oracle, n, loss, keep=(n == 100 and loss == 0))
    e = start(SimulatedCluster(engine, cfg_of(n)), loss)
    fixed = np.random.default_rng(n + 1).random(n) < 0.4
    fixed[[KILLED, 0]] = True  # an explicit mask is taken literally: the killed member's frozen row is counted
    fixed_ids = [int(m) for m in np.nonzero(fixed)[0]]
    running = [m for m in range(n) if m != KILLED]
    ws = []
    for subjects in subject_sets(n):
        ws.append(Watched(e, n, subjects))
        ws.append(Watched(e, n, subjects, fixed_ids, inc_target=[0] * len(subjects)))
    for i, (tick, rows) in enumerate(trace):
        e.step(1)
        for x, w in enumerate(ws):
            where = f"n={n} loss={loss} tick {tick} watch {x}"
            got, _ = w.compare(tick, rows, running, where)
            if i % 10 == 0 or i == TICKS - 1:
                same_as_census(e, got, w.mask, w.subjects, where, KEY8)
    for x, w in enumerate(ws):
        same_stamps(w.w.stamps(), w.ref.planes, f"n={n} loss={loss} watch {x}")
        # not vacuous: the compared columns held ALIVE, SUSPECT and ABSENT
        assert w.seen[ref.ALIVE] and w.seen[ref.SUSPECT] and w.seen[ref.ABSENT], (x, w.seen)
    # ... and the observers learnt of the kill at different ticks; the killed member's own row never did
    na = ws[0].ref.planes["not_alive"][0]
    assert len(set(na[running].tolist())) > 1 and NEVER not in na[running] and na[KILLED] == NEVER
    assert ws[1].ref.planes["not_alive"][0][KILLED] == NEVER  # its frozen row holds itself ALIVE, counted or not
    assert (ws[1].ref.planes["inc_ge"][0][fixed_ids] == trace[0][0]).all()  # literal: true at the first sample
    e.close()


@pytest.mark.parametrize("env,path", [(None, KEY8), ({"SWIM_NO_K8": "1"}, KEY32)], ids=["key8", "key32"])
def test_against_the_census_past_a_tile(engine, env, path):
    """Engine only, n = one census column span + 37 (17 watch blocks): the subjects sit at the span's ends and in the
    tail, one of them killed and SUSPECT at some observers only, so the blocks' partial tallies differ."""
    cols = _abi.CENSUS_TILE_COLS
    n = cols + 37
    killed = (5, cols - 1, cols + 4)
    subjects = [0, cols - 1, cols, n - 1]
    c = create(engine, SimConfig(n_members=n, seed=0x711E), env)
    c.set_default_loss(10)
    for m in killed:
        c.kill(m)
    half = [m for m in range(n) if (m * 7) % 5 < 2 or m in killed]
    w0, w1 = c.watch(subjects), c.watch(subjects, observers=mask_of(n, half))
    c.step(6)
    partial = False
    for _ in range(40):  # until the killed subject is SUSPECT at some but not all observers
        a, b = w0.sample(), w1.sample()
        same_as_census(c, a, None, subjects, f"past a tile {path}: None", path)
        same_as_census(c, b, mask_of(n, half), subjects, f"past a tile {path}: mask", path)
        sus = int(a.counts[1, ref.SUSPECT])
        if 0.2 * a.n_observers < sus < 0.8 * a.n_observers:
            partial = True
            break
        c.step(1)
    assert partial, a.counts
    rows = all_rows(c)
    running = [m for m in range(n) if m not in killed]
    same_tally(a, ref.tally(rows, running, subjects), c.tick, "past a tile: rows, None")
    same_tally(b, ref.tally(rows, half, subjects), c.tick, "past a tile: rows, mask")
    st = w0.stamps()
    assert np.array_equal(st["not_alive"][1] != NEVER, st["not_alive"][1] <= c.tick)
    assert a.counts[1, ref.SUSPECT] <= np.count_nonzero(st["not_alive"][1] != NEVER) < n
    c.close()


# ---- 3: the escape ------------------------------------------------------------------------------------------------

ESC_N, ESC_MOVERS, ESC_STEPS, ESC_TICKS = 96, (3, 31, 32, 63, 64, 95), 9, 15


def escape_script(lib, c):
    """The movers at incarnations 60-63, bumped in alternating halves before every step but the first (four bumps each:
    all end at 64 or above); yields after every tick."""
    c.set_default_loss(10)
    for j, m in enumerate(ESC_MOVERS):
        assert _abi.debug_set_incarnation(lib, c._h, m, 60 + j % 4) == 0
    for step in range(ESC_STEPS):
        if step:
            for m in ESC_MOVERS[(step - 1) % 2::2]:
                c.update_incarnation(m)
        for _ in range(ESC_TICKS):
            c.step(1)
            yield step


def escape_cfg():
    return SimConfig(n_members=ESC_N, cluster=ClusterConfig(syncInterval=1000), seed=0x8B)


def escape_trace(oracle):
    """[(tick, rows)] of the oracle under escape_script: computed once for both planes, never changed."""
    if "escape" not in _TRACES:
        o = SimulatedCluster(oracle, escape_cfg())
        out = []
        for _ in escape_script(oracle, o):
            rows = all_rows(o)
            rows.setflags(write=False)
            out.append((o.tick, rows))
        o.close()
        _TRACES["escape"] = out
    return _TRACES["escape"]


@pytest.mark.parametrize("env,path", [(None, KEY8), ({"SWIM_NO_K8": "1"}, KEY32)], ids=["key8", "key32"])
def test_escape(oracle, engine, env, path):
    """Movers at incarnations 60-63 bumped across 64 under loss: a shadow byte of 0xFF is the escape and reads as DEAD
    in its low bits, so the watch must take those records from the u32 keys. inc_target = 64 for the movers."""
    n = ESC_N
    trace = escape_trace(oracle)
    e = create(engine, escape_cfg(), env)
    subjects = [95, 3, 64, 0, 31, 63, 32]  # the movers out of order, and a member that never moves
    target = [0 if s == 0 else 64 for s in subjects]
    everyone, some = list(range(n)), [m for m in range(n) if m % 3 != 1]
    ws = [Watched(e, n, subjects, None, target), Watched(e, n, subjects, some, target)]
    verdicts, escaped_alive = [], 0
    for (tick, rows), step in zip(trace, escape_script(engine, e)):
        for x, w in enumerate(ws):
            where = f"escape {path} bump {step} tick {tick} watch {x}"
            got, want = w.compare(tick, rows, everyone, where)
            assert got.path == path, where
            ok = ref.met(ref.INC_GE, want["counts"], want["key_min"], want["key_max"], target)
            assert w.w.met(_abi.UNTIL_INC_GE, got) == ok, where
            if x == 0:
                verdicts.append(ok)
                # ALIVE records at incarnation >= 64: escaped bytes whose low bits say DEAD
                escaped_alive += int(np.count_nonzero((want["key_max"] >= 0xFF) & ((want["key_max"] & 3) == ref.ALIVE)))
    assert len(verdicts) == len(trace) == ESC_STEPS * ESC_TICKS
    for x, w in enumerate(ws):
        same_stamps(w.w.stamps(), w.ref.planes, f"escape {path} watch {x}")
    assert escaped_alive > 0
    assert verdicts[0] is False and verdicts[-1] is True  # every mover reached 64 everywhere, and not at once
    inc = ws[0].ref.planes["inc_ge"]  # (member 0, target 0: literal, stamped by the first sample at tick 1)
    assert (inc[3] == 1).all() and len(set(inc[0].tolist())) > 1 and NEVER not in inc
    e.close()


# ---- 4: run_until -------------------------------------------------------------------------------------------------

def exact_gone(oracle, n=100):
    trace = oracle_trace(oracle, n, 0, keep=True)
    return first_met(trace, ref.GONE, [m for m in range(n) if m != KILLED], [KILLED])


def test_run_until_gone(oracle, engine):
    """(a) check_every = 1: ticks_run is the first tick at which the oracle's rows meet the condition, and the handle is
    where a twin plainly stepped that many ticks is. (d) the condition already holds: nothing runs."""
    n = 100
    exact = exact_gone(oracle, n)
    assert exact == 88
    e = start(SimulatedCluster(engine, cfg_of(n)))
    w = e.watch([KILLED])
    assert e.run_until(w, _abi.UNTIL_GONE, 200, 1) == (True, exact)
    assert e.tick == LEAD + exact
    twin = start(SimulatedCluster(engine, cfg_of(n)))
    twin.step(exact)
    assert np.array_equal(e.state_hash(), twin.state_hash()), "state hashes differ"
    ce, ct = e.counters(), twin.counters()
    assert {k: ce[k] for k in PARITY_KEYS} == {k: ct[k] for k in PARITY_KEYS}
    assert ce["device_bytes"] == ct["device_bytes"]  # the watch's memory is its own
    # the stamps of the run: every running observer saw it gone by the last tick, some earlier
    gone = w.stamps()["gone"][0]
    running = [m for m in range(n) if m != KILLED]
    assert gone[running].max() == LEAD + exact and gone[running].min() < LEAD + exact and gone[KILLED] == NEVER
    # (d)
    ok, ticks, last = w.run_until(e._h, _abi.UNTIL_GONE, 200, 1)
    assert (ok, ticks, e.tick, last.tick) == (True, 0, LEAD + exact, LEAD + exact)
    assert last.counts[0].tolist() == [n - 1, 0, 0, 0] and last.n_observers == n - 1
    assert e.run_until(w, _abi.UNTIL_NOT_ALIVE, 0, 5) == (True, 0)
    twin.close()
    e.close()


def test_run_until_resolution_and_limit(oracle, engine):
    """(b) check_every = 7: the answer is the first look at or after the exact tick. (c) max_ticks 25 with check_every 10:
    looks at 10, 20 and 25, not met, exactly 25 ticks run."""
    n = 100
    exact = exact_gone(oracle, n)
    e = start(SimulatedCluster(engine, cfg_of(n)))
    w = e.watch([KILLED], stamps=False)
    ok, ticks = e.run_until(w, _abi.UNTIL_GONE, 200, 7)
    assert ok and ticks % 7 == 0 and exact <= ticks < exact + 7, (ticks, exact)
    assert e.tick == LEAD + ticks
    e.close()
    e = start(SimulatedCluster(engine, cfg_of(n)))
    w = e.watch([KILLED])
    ok, ticks, last = w.run_until(e._h, _abi.UNTIL_GONE, 25, 10)
    assert (ok, ticks, e.tick, last.tick) == (False, 25, LEAD + 25, LEAD + 25)
    assert set(np.unique(w.stamps()["not_alive"][0]).tolist()) <= {LEAD, LEAD + 10, LEAD + 20, LEAD + 25, NEVER}
    assert e.run_until(w, _abi.UNTIL_GONE, 0, 1) == (False, 0) and e.tick == LEAD + 25
    e.close()


def test_run_until_join_converged(oracle, engine):
    """(e) COLD_JOIN with dormant members: the joiner's record has reached every running member, itself included."""
    n, joiner = 40, 38
    cfg = SimConfig(n_members=n, cluster=ClusterConfig(seedMembers=[0]), init_mode=_abi.INIT_COLD_JOIN, n_dormant=4)
    o, e = SimulatedCluster(oracle, cfg), SimulatedCluster(engine, cfg)
    for c in (o, e):
        c.step(30)
        c.join(joiner, [0])
    running = list(range(n - 4)) + [joiner]
    exact = None
    for i in range(60):
        t = ref.tally(all_rows(o), running, [joiner])
        if ref.met(ref.CONVERGED, t["counts"], t["key_min"], t["key_max"]):
            exact = i
            break
        o.step(1)
    assert exact == 12
    w = e.watch([joiner])
    first = w.sample()
    assert first.n_observers == len(running) and first.counts[0, ref.ABSENT] == len(running) - 1
    assert e.run_until(w, _abi.UNTIL_CONVERGED, 100, 1) == (True, exact)
    assert e.tick == 30 + exact
    o.close()
    e.close()


# ---- 5: sharded ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3, 0], ids=["W2", "W3", "n_gpus2"])
def test_sharded(oracle, engine, world):
    """Row shards (ThreadShardGroup, W = 2 and 3) and an n_gpus = 2 handle (world 0): each shard's partial covers its own
    observers only, the combined tallies and stamps are the oracle's, run_until gives the one-GPU answer."""
    from swimhip.shard import ThreadShardGroup
    n = 100
    trace = oracle_trace(oracle, n, 0, keep=True)
    cfg = cfg_of(n)

    def make():
        return start(ThreadShardGroup(engine, cfg, world) if world
                     else SimulatedCluster(engine, dataclasses.replace(cfg, n_gpus=2)))

    e = make()
    running = [m for m in range(n) if m != KILLED]
    fixed_ids = [KILLED] + [m for m in range(n) if (m * 11) % 7 < 3 and m != KILLED]
    subjects = [KILLED, 0, n - 1, 2]
    ws = [Watched(e, n, subjects), Watched(e, n, subjects, fixed_ids, [0] * 4)]
    for tick, rows in trace:
        e.step(1)
        for x, w in enumerate(ws):
            ids = w.ids if w.ids is not None else running
            w.compare(tick, rows, running, f"W={world} tick {tick} watch {x}")
            if world:  # the partials themselves
                for s, p in zip(e.shards, w.w.parts):
                    assert p.sample().n_observers == len([m for m in ids if s.lo <= m < s.hi])
    for x, w in enumerate(ws):
        same_stamps(w.w.stamps(), w.ref.planes, f"W={world} watch {x}")
        assert w.seen[ref.ALIVE] and w.seen[ref.SUSPECT] and w.seen[ref.ABSENT], w.seen
        if world:
            for s, p in zip(e.shards, w.w.parts):
                for name, plane in p.stamps().items():
                    assert (plane[:, :s.lo] == NEVER).all() and (plane[:, s.hi:] == NEVER).all(), (world, name)
                    if name != "inc_ge" or w.inc is not None:
                        assert (plane[:, s.lo:s.hi] != NEVER).any(), (world, name)
    e.close()
    e = make()
    w = e.watch([KILLED])
    assert e.run_until(w, _abi.UNTIL_GONE, 200, 1) == (True, exact_gone(oracle, n))
    if world:  # one shard cannot give the verdict
        t, m = C.c_uint32(), C.c_uint32()
        s, p = e.shards[0], w.parts[0]
        assert engine.swim_run_until(s._h, p._w, _abi.UNTIL_GONE, 5, 1, C.byref(t), C.byref(m), None) == \
            _abi.SWIM_EUNSUPPORTED
        assert s.tick == e.shards[1].tick
    e.close()


# ---- 6: no side effects -------------------------------------------------------------------------------------------

def test_no_side_effects(engine):
    """Two handles with the same config, SYNC every tick (lister and dirty masks busy), loss and a kill: one samples two
    watches after every tick, the other none; everything the simulation computes and counts is identical."""
    cfg = SimConfig(n_members=200, cluster=ClusterConfig(syncInterval=100), seed=0x51DE)
    keys = PARITY_KEYS + ["diff_msgs", "diff_msgs_total", "diff_key_bytes", "diff_key_bytes_total", "ack_resolved",
                          "ack_resolved_total", "device_bytes"]
    out = []
    for take in (True, False):
        c = SimulatedCluster(engine, cfg)
        c.set_default_loss(10)
        c.kill(7)
        if take:
            ws = [c.watch([7, 8, 199]), c.watch(list(range(0, 200, 3)), inc_target=[1] * 67,
                                                observers=mask_of(200, range(0, 200, 2)))]
        for _ in range(80):
            c.step(1)
            if take:
                assert ws[0].sample().n_observers == 199 and ws[1].sample().n_observers == 100
        if take:
            assert (ws[0].stamps()["not_alive"][0] != NEVER).any()
        assert _abi.debug_dirty_check(engine, c._h) == 0
        ctr = c.counters()
        out.append((c.state_hash(), {k: ctr[k] for k in keys}, _abi.debug_diff_dirty(engine, c._h)))
        c.close()
    assert np.array_equal(out[0][0], out[1][0]), "state hashes differ"
    assert out[0][1] == out[1][1]
    assert out[0][2] == out[1][2]


# ---- 7: arguments -------------------------------------------------------------------------------------------------

def test_arguments(engine):
    n = 70
    c = start(SimulatedCluster(engine, cfg_of(n)), loss=10)
    c.step(30)
    _abi.bind_watch(engine)
    EINVAL, EUNSUP = _abi.SWIM_EINVAL, _abi.SWIM_EUNSUPPORTED

    def make(subjects, inc=None, mask=None, flags=_abi.WATCH_STAMPS, handle=None, out=True, null_subjects=False):
        w = C.c_void_p()
        s = np.ascontiguousarray(subjects, dtype=np.uint32)
        i = None if inc is None else np.ascontiguousarray(inc, dtype=np.uint32)
        rc = engine.swim_watch_create(c._h if handle is None else handle, None if null_subjects else s.ctypes.data_as(P),
                                      len(subjects), None if i is None else i.ctypes.data_as(P),
                                      None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), flags,
                                      C.byref(w) if out else None)
        return rc, w

    assert make([])[0] == EINVAL                       # k = 0
    assert make(list(range(70)) * 4)[0] == EINVAL      # k > 256 (and duplicates)
    assert make([0, n])[0] == EINVAL                   # a subject >= N
    assert make([3, 5, 3])[0] == EINVAL                # a duplicate subject
    assert make([1], null_subjects=True)[0] == EINVAL  # null arguments
    assert make([1], out=False)[0] == EINVAL
    assert make([1], flags=2)[0] == EINVAL             # an unknown flag
    rumor = SimulatedCluster(engine, SimConfig(n_members=300, mode=_abi.MODE_RUMOR, churn_per_period=3))
    assert make([1], handle=rumor._h)[0] == EUNSUP
    with pytest.raises(SwimError):
        rumor.watch([1])
    rumor.close()
    rumor = SimulatedCluster(engine, SimConfig(n_members=300, mode=_abi.MODE_RUMOR, churn_per_period=3,
                                               implicit_views=True))
    assert make([1], handle=rumor._h)[0] == EUNSUP
    rumor.close()

    subjects = [KILLED, 69, 0]
    rc, w = make(subjects, inc=[0, 1, 2])
    assert rc == 0
    rc, bare = make(subjects, flags=0)
    assert rc == 0
    full = _abi.SwimWatchSample()
    counts, mn, mx = np.full((3, 4), 0xABABABAB, np.uint32), np.full(3, 0xABABABAB, np.uint32), \
        np.full(3, 0xABABABAB, np.uint32)
    full.counts, full.key_min, full.key_max = counts.ctypes.data_as(P), mn.ctypes.data_as(P), mx.ctypes.data_as(P)
    full.reserved[0] = 9
    assert engine.swim_watch_sample(w, C.byref(full)) == 0
    want = ref.tally(all_rows(c), [m for m in range(n) if m != KILLED], subjects)
    assert np.array_equal(counts, want["counts"]) and np.array_equal(mn, want["key_min"])  # sentinels overwritten
    assert np.array_equal(mx, want["key_max"]) and list(full.reserved) == [0, 0, 0]
    assert (int(full.tick), int(full.n_observers), int(full.path)) == (c.tick, n - 1, KEY8)
    assert counts[0, ref.ALIVE] < n - 1  # the killed member is suspected or gone somewhere
    tot = _abi.SwimWatchSample()  # null output pointers: the totals only
    tot.tick = tot.n_observers = 0xABAB
    assert engine.swim_watch_sample(bare, C.byref(tot)) == 0
    assert (int(tot.tick), int(tot.n_observers), int(tot.path)) == (c.tick, n - 1, KEY8)
    assert engine.swim_watch_sample(w, None) == EINVAL and engine.swim_watch_sample(None, C.byref(tot)) == EINVAL

    buf = np.full(3 * n, 0xABABABAB, np.uint32)
    assert engine.swim_watch_stamps(w, _abi.STAMP_NOT_ALIVE, buf.ctypes.data_as(P), buf.size) == 0
    assert not (buf == 0xABABABAB).any() and set(np.unique(buf).tolist()) == {c.tick, NEVER}
    assert engine.swim_watch_stamps(w, _abi.STAMP_INC_GE, buf.ctypes.data_as(P), buf.size) == 0
    assert (buf[:n][np.arange(n) != KILLED] == c.tick).all() and buf[KILLED] == NEVER  # target 0: held is enough
    assert engine.swim_watch_stamps(w, 3, buf.ctypes.data_as(P), buf.size) == EINVAL          # an unknown stamp
    assert engine.swim_watch_stamps(w, 0, buf.ctypes.data_as(P), buf.size - 1) == EINVAL      # a cap too small
    assert engine.swim_watch_stamps(w, 0, None, buf.size) == EINVAL
    assert engine.swim_watch_stamps(bare, 0, buf.ctypes.data_as(P), buf.size) == EINVAL       # made without the flag
    # sampling twice at one tick changes nothing
    before = np.zeros(3 * n, np.uint32)
    engine.swim_watch_stamps(w, 0, before.ctypes.data_as(P), before.size)
    assert engine.swim_watch_sample(w, C.byref(full)) == 0
    after = np.zeros(3 * n, np.uint32)
    engine.swim_watch_stamps(w, 0, after.ctypes.data_as(P), after.size)
    assert np.array_equal(before, after)

    t, m = C.c_uint32(7), C.c_uint32(7)
    run = lambda h, ww, cond, mx_, every, tt=t, mm=m: engine.swim_run_until(
        h, ww, cond, mx_, every, C.byref(tt) if tt is not None else None, C.byref(mm) if mm is not None else None, None)
    tick = c.tick
    assert run(c._h, w, _abi.UNTIL_GONE, 5, 0) == EINVAL       # check_every = 0
    assert run(c._h, w, 4, 5, 1) == EINVAL                     # an unknown condition
    assert run(None, w, 0, 5, 1) == EINVAL and run(c._h, None, 0, 5, 1) == EINVAL
    assert run(c._h, w, 0, 5, 1, None, m) == EINVAL and run(c._h, w, 0, 5, 1, t, None) == EINVAL
    assert run(c._h, bare, _abi.UNTIL_INC_GE, 5, 1) == EINVAL  # no inc_target
    other = SimulatedCluster(engine, cfg_of(n))
    assert run(other._h, w, _abi.UNTIL_GONE, 5, 1) == EINVAL   # a watch of another handle
    other.close()
    assert c.tick == tick
    assert run(c._h, bare, _abi.UNTIL_GONE, 3, 2) == 0 and (t.value, m.value, c.tick) == (3, 0, tick + 3)
    assert engine.swim_watch_destroy(bare) == 0 and engine.swim_watch_destroy(None) == EINVAL
    # swim_destroy with live watches (w, and one the wrapper knows) is clean; closing the wrapper's afterwards is a no-op
    pyw = c.watch([2, 3])
    pyw.sample()
    c.close()
    pyw.close()
