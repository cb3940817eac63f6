"""Recording on a subject watch (include/swimhip_watch_series.h): the per-tick series the engine takes inside swim_step,
speculative batches included, against rows read one observer at a time and against the host-sampled watch.

Expected tallies and stamps come from the CPU oracle's rows through tests/watch_ref.py at the small shapes, and from the
merged, oracle-checked path (one tick per call, swim_watch_sample after each) at the size where the batches elide their
diffs and run without a lister. Configurations and scripts are those of test_gpu_watch.py (FAST) and
test_gpu_lister_free.py / test_gpu_diff_dirty.py (FAST_SYNC, 2 100 members)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from swimhip import SimConfig, SimulatedCluster, _abi
from swimhip.watch import combine_series

import watch_ref as ref
from test_gpu_diff_dirty import FAST_SYNC, dirty
from test_gpu_watch import KILLED, LEAD, PARITY_KEYS, TICKS, all_rows, cfg_of, create, exact_gone, same_stamps, start

pytestmark = pytest.mark.gpu

NEVER = _abi.WATCH_NEVER
EINVAL, EUNSUP = _abi.SWIM_EINVAL, _abi.SWIM_EUNSUPPORTED
P, P64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_CACHE = {}


def same_series(a, b, where, fields=("ticks", "n_observers", "counts", "key_min", "key_max")):
    assert len(a) == len(b), (where, len(a), len(b))
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        bad = np.argwhere(x != y)
        assert len(bad) == 0, f"{where}: {f} differs at {bad[:6].tolist()}: {x[tuple(bad[0])]} != {y[tuple(bad[0])]}"


# ---- 1: the small shapes against the oracle ------------------------------------------------------------------------

def full_trace(oracle, n):
    """[rows [n, n]] of the oracle at every tick 0 .. LEAD + TICKS of the script (LEAD ticks, the kill, TICKS ticks).
    Computed once per n, never changed."""
    if ("trace", n) not in _CACHE:
        o = SimulatedCluster(oracle, cfg_of(n))
        out = []
        for t in range(LEAD + TICKS + 1):
            if t:
                o.step(1)
            assert o.tick == t
            rows = all_rows(o)
            rows.setflags(write=False)
            out.append(rows)
            if t == LEAD:
                o.kill(KILLED)  # (changes no row)
        o.close()
        _CACHE[("trace", n)] = out
    return _CACHE[("trace", n)]


@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("n", [65, 257])
def test_small_shapes_against_the_oracle(oracle, engine, n, k):
    """A wave plus one and a block plus one observers; the 8-wide unroll has a one-subject tail at K = 9. Armed at tick 0,
    then the script in two swim_step calls: the sample of tick LEAD is taken before the kill, as a host sample would be."""
    trace = full_trace(oracle, n)
    subjects = [KILLED, 0, n - 1, 2, 40, 63, 5, 33, 17][:k]
    inc = [0] * k
    e = SimulatedCluster(engine, cfg_of(n))
    w = e.watch(subjects, inc_target=inc)
    w.record(every=1, cap=LEAD + TICKS + 1)
    assert w.recorded() == 1
    e.step(LEAD)
    e.kill(KILLED)
    e.step(TICKS)
    s = w.series()
    assert len(s) == s.n_recorded == LEAD + TICKS + 1 and s.ticks.tolist() == list(range(LEAD + TICKS + 1))
    stamps = ref.StampRef(n, subjects, inc)
    seen = np.zeros(4, np.uint64)
    everyone, running = list(range(n)), [m for m in range(n) if m != KILLED]
    for t, rows in enumerate(trace):
        ids = everyone if t <= LEAD else running
        want = ref.tally(rows, ids, subjects)
        assert s.n_observers[t] == want["n_observers"], (n, k, t)
        for f in ("counts", "key_min", "key_max"):
            assert np.array_equal(getattr(s, f)[t], want[f]), (n, k, t, f, getattr(s, f)[t], want[f])
        stamps.feed(t, rows, ids)
        seen += want["counts"][0].astype(np.uint64)
    assert s.n_observers[LEAD] == n and s.n_observers[LEAD + 1] == n - 1  # drops by one at the kill
    same_stamps(w.stamps(), stamps.planes, f"n={n} K={k}")
    assert seen[ref.ALIVE] and seen[ref.SUSPECT] and seen[ref.ABSENT], seen  # not vacuous
    na = stamps.planes["not_alive"][0][running]
    assert len(set(na.tolist())) > 1 and NEVER not in na
    # the host sample at the last tick is the last entry; it leaves the series alone
    last = w.sample()
    assert last.tick == s.ticks[-1] and np.array_equal(last.counts, s.counts[-1])
    same_series(w.series(), s, "after a host sample")
    e.close()


# ---- 2, 3: through every halt, against the host-sampled twin and against a handle without a watch -----------------

BIG_N, BUMPED, VICTIM = 2100, 5, 1234
BIG_SUBJECTS, BIG_INC = [VICTIM, BUMPED, 0], [0, 7, 0]
CALL, SETTLE_CALLS, TAIL_CALLS = 40, 40, 40


def replay(engine, c, ops, after_tick=None):
    """The recorded script on another handle; after_tick(c) after every single tick if given (then one tick per call)."""
    for op in ops:
        if op[0] == "step":
            if after_tick is None:
                c.step(op[1])
            else:
                for _ in range(op[1]):
                    c.step(1)
                    after_tick(c)
        elif op[0] == "inc":
            assert _abi.debug_set_incarnation(engine, c._h, op[1], op[2]) == 0
        else:
            c.kill(op[1])


def recorded_run(engine):
    """Handle A: 2 100 members, SYNC every 10 ticks, a recording of every tick armed at tick 0 and long swim_step calls.
    A clean stretch (four calls of 10 ticks: the batches elide their diffs, then run lister-free), a key changed from the
    host (test_gpu_lister_free.py test_dirt_from_the_host's way), 40-tick calls until the new incarnation has spread, its
    chunk is rebased and lister-free ticks run again (test_dirt_inside_a_batch's settling), a kill while both modes are
    on (test_device_write_ends_the_mode), and a tail of 40-tick calls until the victim is gone everywhere and a whole
    call has elided its diffs again without a gossip. (Lister-free ticks cannot come back after the kill: the victim's
    frozen row keeps a dirty chunk for good, and the mode needs every mask zero; so the quiet stretch that re-enters both
    modes comes before the kill.) Returns the script as run, the per-call deltas of swim_debug_diff_dirty and
    gossips_created, and what the handle computed. Run once for the tests that share it."""
    if "A" in _CACHE:
        return _CACHE["A"]
    c = create(engine, SimConfig(n_members=BIG_N, cluster=FAST_SYNC))
    w = c.watch(BIG_SUBJECTS, inc_target=BIG_INC)
    w.record(every=1, cap=64 + CALL * (SETTLE_CALLS + TAIL_CALLS))
    ops, deltas = [], []

    def step(n):
        d0, g0 = dirty(engine, c), c.counters()["gossips_created"]
        c.step(n)
        d1 = dirty(engine, c)
        ops.append(("step", n))
        deltas.append(({k: d1[k] - d0[k] for k in d1}, c.counters()["gossips_created"] - g0))

    for _ in range(4):
        step(10)
    for _ in range(12):  # refused while the member has a live-row payload in flight: a tick later then
        if _abi.debug_set_incarnation(engine, c._h, BUMPED, 7) == 0:
            break
        step(1)
    else:
        raise AssertionError("member 5 had a live-row payload in flight 12 ticks in a row")
    ops.append(("inc", BUMPED, 7))
    settled = None
    for q in range(SETTLE_CALLS):
        step(CALL)
        if deltas[-1][0]["lister_free_ticks"] > 0:
            settled = q
            break
    c.kill(VICTIM)
    ops.append(("kill", VICTIM))
    gone_at = None
    for q in range(TAIL_CALLS):
        step(CALL)
        if gone_at is None:
            last = w.series(w.recorded() - 1).counts[0, 0]  # the victim's column at the latest tick
            if last[ref.ALIVE] == 0 and last[ref.SUSPECT] == 0:
                gone_at = q
        if gone_at is not None and q > gone_at and deltas[-1][0]["diff_elided"] == CALL and deltas[-1][1] == 0:
            break
    ctr = c.counters()
    out = dict(ops=ops, deltas=deltas, series=w.series(), stamps=w.stamps(), hash=c.state_hash(), tick=c.tick,
               counters={k: ctr[k] for k in PARITY_KEYS}, dd=dirty(engine, c), gone_at=gone_at, settled=settled)
    print(f"recorded run: {len(ops)} ops, tick {c.tick}, dd {out['dd']}, settled after call {settled}, gone after tail "
          f"call {gone_at}", flush=True)
    c.close()
    _CACHE["A"] = out
    return out


def test_against_the_host_sampled_twin_through_every_halt(engine):
    """Handle B follows A's script one tick per call with swim_watch_sample after each tick: entries, stamps, the final
    state hash and the parity counters are identical. A's own counters say that, inside recorded calls, ticks ran without a
    lister and without a diff, a batch stopped at a diff-halt, and a batch that elided diffs stopped at a gossip halt
    (conditions on the script). lister_free_stops is printed, not asserted: a member kernel that writes without taking a
    gossip slot in the same launch has never occurred in any run of this engine ("Who breaks the mode"),
    no existing test reaches that branch at any size, and the sample it would leave valid (tick kw + 1, queued behind
    member(kw)) is the one the gossip-halt path voids and queues again here."""
    a = recorded_run(engine)
    sums = {k: sum(d[k] for d, _ in a["deltas"]) for k in a["dd"]}
    print(f"inside recorded calls: {sums}", flush=True)
    assert sums["lister_free_ticks"] > 0 and sums["diff_elided"] > 0 and sums["diff_halts"] > 0, sums
    assert any(g > 0 and d["diff_elided"] > 0 for d, g in a["deltas"]), "no gossip halt inside an eliding call"
    assert a["settled"] is not None, "lister-free ticks did not come back after the host's key change"
    assert a["gone_at"] is not None and a["deltas"][-1][0]["diff_elided"] == CALL, "the tail did not elide again"
    b = create(engine, SimConfig(n_members=BIG_N, cluster=FAST_SYNC))
    wb = b.watch(BIG_SUBJECTS, inc_target=BIG_INC)
    samples = [wb.sample()]
    replay(engine, b, a["ops"], lambda c: samples.append(wb.sample()))
    s = a["series"]
    assert b.tick == a["tick"] and len(s) == s.n_recorded == len(samples) == a["tick"] + 1
    for i, x in enumerate(samples):
        assert (x.tick, x.n_observers) == (s.ticks[i], s.n_observers[i]), (i, x.tick, x.n_observers, s.n_observers[i])
        for f in ("counts", "key_min", "key_max"):
            assert np.array_equal(getattr(x, f), getattr(s, f)[i]), (i, f, getattr(x, f), getattr(s, f)[i])
    same_stamps(a["stamps"], wb.stamps(), "recorded vs host-sampled")
    assert (a["stamps"]["gone"][0] != NEVER).sum() == BIG_N - 1 and len(np.unique(a["stamps"]["gone"][0])) > 2
    assert (a["stamps"]["inc_ge"][1] != NEVER).sum() >= BIG_N - 1 and len(np.unique(a["stamps"]["inc_ge"][1])) > 2
    assert np.array_equal(a["hash"], b.state_hash()), "state hashes differ"
    cb = b.counters()
    assert a["counters"] == {k: cb[k] for k in PARITY_KEYS}
    b.close()


def test_no_side_effects_on_the_run_or_the_batching(engine):
    """A handle without any watch after the same calls: the state, the counters and all ten swim_debug_diff_dirty entries
    (the batches were cut at the same ticks and took the same paths) are A's."""
    a = recorded_run(engine)
    c = create(engine, SimConfig(n_members=BIG_N, cluster=FAST_SYNC))
    replay(engine, c, a["ops"])
    assert c.tick == a["tick"]
    assert np.array_equal(a["hash"], c.state_hash()), "state hashes differ"
    ctr = c.counters()
    assert a["counters"] == {k: ctr[k] for k in PARITY_KEYS}
    dd = dirty(engine, c)
    assert len(dd) == 10 and dd == a["dd"], (dd, a["dd"])
    c.close()


# ---- 4: every and cap ---------------------------------------------------------------------------------------------

def test_every_and_cap(engine):
    n = 100
    e = start(SimulatedCluster(engine, cfg_of(n)))
    t0 = e.tick
    w1, w7, w5 = e.watch([KILLED, 0]), e.watch([KILLED, 0]), e.watch([KILLED, 0])
    w1.record(every=1, cap=256)
    w7.record(every=7, cap=64)
    w5.record(every=1, cap=5)
    e.step(60)
    s1, s7, s5 = w1.series(), w7.series(), w5.series()
    assert len(s1) == 61 and len(s7) == 9 and s7.ticks.tolist() == [t0 + 7 * i for i in range(9)]
    for i in range(9):
        for f in ("n_observers", "counts", "key_min", "key_max"):
            assert np.array_equal(getattr(s7, f)[i], getattr(s1, f)[7 * i]), (i, f)
    assert len(np.unique(s7.counts[:, 0, ref.SUSPECT])) > 1  # the entries differ from one another
    # every = 7 stamps with its own samples' ticks
    assert set(np.unique(w7.stamps()["not_alive"][0]).tolist()) <= {t0 + 7 * i for i in range(9)} | {NEVER}
    # cap = 5: exactly five entries, the run goes on, the stamps stop changing after the fifth
    assert len(s5) == s5.n_recorded == 5 and s5.ticks.tolist() == list(range(t0, t0 + 5))
    same_series(s5, w1.series(0, 5), "cap 5 vs the first five")
    st5 = w5.stamps()
    assert set(np.unique(st5["not_alive"][0]).tolist()) <= set(range(t0, t0 + 5)) | {NEVER}
    assert (st5["not_alive"][0] == NEVER).any() and (w1.stamps()["not_alive"][0] != NEVER).sum() > \
        (st5["not_alive"][0] != NEVER).sum()
    got = C.c_uint32()
    assert engine.swim_watch_series(w5._w, 5, 1, None, None, None, None, None, C.byref(got)) == EINVAL and got.value == 5
    e.step(10)
    assert w5.recorded() == 5 and e.tick == t0 + 70
    same_stamps(w5.stamps(), st5, "after the series was full")
    # re-arming (a full series counts as stopped) starts a new one at the then-current tick
    w5.record(every=2, cap=10)
    assert w5.recorded() == 1 and w5.series().ticks.tolist() == [t0 + 70]
    w7.stop()
    e.step(9)
    assert w5.series().ticks.tolist() == [t0 + 70 + 2 * i for i in range(5)]
    s1, s7 = w1.series(), w7.series()  # stopped at tick t0 + 70: eleven entries, and no more
    assert s7.ticks.tolist() == [t0 + 7 * i for i in range(11)] and np.array_equal(s7.counts, s1.counts[0:71:7])
    w7.record(every=3, cap=4)  # after a stop: a new series
    assert w7.series().ticks.tolist() == [t0 + 79]
    s1 = w1.series()
    i = int(t0 + 78 - s1.ticks[0])
    assert np.array_equal(w5.series().counts[4], s1.counts[i])
    e.close()


def test_arming_leaves_other_recordings_alone(engine):
    """A second watch armed after a kill at the same tick: the first watch's entry of that tick, taken when the tick
    came to rest, still counts the victim as an observer; the second watch's first entry does not. Also on an n_gpus
    handle, whose shards each arm their own series."""
    for gpus in (1, 2):
        e = SimulatedCluster(engine, dataclasses.replace(cfg_of(100), n_gpus=gpus))
        a = e.watch([KILLED, 0])
        a.record(every=1, cap=64)
        e.step(LEAD)
        before, stamps = a.series(), a.stamps()
        e.kill(KILLED)
        b = e.watch([KILLED, 0])
        b.record(every=1, cap=64)
        same_series(a.series(), before, f"n_gpus={gpus}: after arming another watch")
        same_stamps(a.stamps(), stamps, f"n_gpus={gpus}")
        assert a.series().n_observers[-1] == 100 and b.series().n_observers.tolist() == [99]
        e.step(3)
        sa, sb = a.series(), b.series()
        assert sa.n_observers.tolist() == [100] * (LEAD + 1) + [99] * 3 and sb.n_observers.tolist() == [99] * 4
        assert np.array_equal(sa.counts[LEAD + 1:], sb.counts[1:])
        assert a.series(first=sa.n_recorded + 5).ticks.tolist() == []  # past the complete entries: an empty series
        e.close()


# ---- 5: run_until_recorded ----------------------------------------------------------------------------------------

def test_run_until_recorded(oracle, engine):
    n, chunk = 100, 16
    twin = start(SimulatedCluster(engine, cfg_of(n)))
    ok, ticks = twin.run_until(twin.watch([KILLED]), _abi.UNTIL_GONE, 200, 1)
    assert ok and ticks == exact_gone(oracle, n)
    stop_tick = twin.tick
    twin.close()
    e = start(SimulatedCluster(engine, cfg_of(n)))
    begin = e.tick
    w = e.watch([KILLED])
    w.record(every=1, cap=256)
    ok, met_tick, ran = e.run_until_recorded(w, _abi.UNTIL_GONE, 200, chunk)
    assert ok and met_tick == stop_tick, (ok, met_tick, stop_tick)
    assert e.tick == begin + ran and 0 <= ran - (met_tick - begin) < chunk and ran % chunk == 0, (ran, met_tick, begin)
    assert w.first_met(_abi.UNTIL_GONE)[0] == met_tick
    # already met: the entry of the current tick says so, nothing runs
    tick = e.tick
    assert e.run_until_recorded(w, _abi.UNTIL_GONE, 50, chunk) == (True, tick, 0) and e.tick == tick
    # max_ticks reached: member 0 is never gone
    w0 = e.watch([0])
    w0.record(every=1, cap=64)
    assert e.run_until_recorded(w0, _abi.UNTIL_GONE, 10, 4) == (False, 0, 10) and e.tick == tick + 10
    assert w0.recorded() == 11
    e.close()


# ---- 6, 7: sharded, and the KEY32 path ----------------------------------------------------------------------------

SH_SUBJECTS = [KILLED, 0, 99, 2]


def armed_run(c):
    """The script's head, a recording armed after the kill, TICKS ticks in one call: (series, stamps)."""
    start(c)
    w = c.watch(SH_SUBJECTS, inc_target=[0] * 4)
    w.record(every=1, cap=TICKS + 1)
    c.step(TICKS)
    return w, w.series(), w.stamps()


def one_gpu_series(engine):
    if "one" not in _CACHE:
        c = SimulatedCluster(engine, cfg_of(100))
        _, s, st = armed_run(c)
        assert len(s) == TICKS + 1 and len(np.unique(s.counts[:, 0, ref.SUSPECT])) > 2
        c.close()
        _CACHE["one"] = (s, st)
    return _CACHE["one"]


@pytest.mark.parametrize("world", [2, 3, 0], ids=["W2", "W3", "n_gpus2"])
def test_sharded(engine, world):
    from swimhip.shard import ThreadShardGroup
    want, want_stamps = one_gpu_series(engine)
    cfg = cfg_of(100)
    c = ThreadShardGroup(engine, cfg, world) if world else SimulatedCluster(engine, dataclasses.replace(cfg, n_gpus=2))
    w, s, st = armed_run(c)
    same_series(s, want, f"W={world}")
    same_stamps(st, want_stamps, f"W={world}")
    if world:
        parts = [p.series() for p in w.parts]
        assert [int(p.n_observers[1]) for p in parts] == [sh.hi - sh.lo - (sh.lo <= KILLED < sh.hi) for sh in c.shards]
        same_series(combine_series(parts), want, f"W={world} partials")
        t, m, r = C.c_uint64(), C.c_uint32(), C.c_uint32()
        sh, p = c.shards[0], w.parts[0]
        assert engine.swim_run_until_recorded(sh._h, p._w, _abi.UNTIL_GONE, 5, 1, C.byref(t), C.byref(m), C.byref(r)) \
            == EUNSUP
        assert sh.tick == c.shards[1].tick
    else:
        w0 = c.watch([0])
        w0.record(every=1, cap=16)
        tick = c.tick
        assert c.run_until_recorded(w0, _abi.UNTIL_GONE, 6, 3) == (False, 0, 6) and c.tick == tick + 6
        assert w0.series().ticks.tolist() == list(range(tick, tick + 7))
    c.close()


def test_key32_path(engine):
    want, want_stamps = one_gpu_series(engine)
    c = create(engine, cfg_of(100), {"SWIM_NO_K8": "1"})
    w, s, st = armed_run(c)
    assert w.sample().path == _abi.CENSUS_PATH_KEY32
    same_series(s, want, "KEY32")
    same_stamps(st, want_stamps, "KEY32")
    c.close()


# ---- 8: arguments -------------------------------------------------------------------------------------------------

def test_arguments(engine):
    c = start(SimulatedCluster(engine, cfg_of(70)))
    w, bare = c.watch([KILLED, 3]), c.watch([3])
    lib, tick = engine, c.tick
    got = C.c_uint32(77)
    t, m, r = C.c_uint64(), C.c_uint32(), C.c_uint32()
    until = lambda ww, chunk=4: lib.swim_run_until_recorded(c._h, ww._w, _abi.UNTIL_GONE, 8, chunk, C.byref(t), C.byref(m),
                                                            C.byref(r))
    # nothing armed yet
    assert lib.swim_watch_series(w._w, 0, 0, None, None, None, None, None, C.byref(got)) == EINVAL
    assert lib.swim_watch_record_stop(w._w) == EINVAL
    assert until(w) == EINVAL and c.tick == tick                    # run_until_recorded without a recording
    assert lib.swim_watch_record(w._w, 0, 8) == EINVAL              # every = 0
    assert lib.swim_watch_record(w._w, 1, 0) == EINVAL              # cap = 0
    assert lib.swim_watch_record(w._w, 1, _abi.WATCH_SERIES_MAX_WORDS // 14 + 1) == EINVAL  # 5 K + 4 = 14 words an entry
    assert lib.swim_watch_series(w._w, 0, 0, None, None, None, None, None, C.byref(got)) == EINVAL  # (still none)
    assert lib.swim_watch_record(w._w, 2, 8) == 0
    assert lib.swim_watch_record(w._w, 1, 8) == EINVAL              # arming twice
    assert w.recorded() == 1 and w.series().ticks.tolist() == [tick]  # ... left the first recording alone
    c.step(5)
    assert w.recorded() == 3
    ticks = np.zeros(4, np.uint64)
    assert lib.swim_watch_series(w._w, 0, 4, ticks.ctypes.data_as(P64), None, None, None, None, C.byref(got)) == EINVAL
    assert got.value == 3 and not ticks.any()                       # a range past n_recorded
    assert lib.swim_watch_series(w._w, 3, 1, None, None, None, None, None, None) == EINVAL
    assert lib.swim_watch_series(w._w, 1, 2, ticks.ctypes.data_as(P64), None, None, None, None, None) == 0
    assert ticks.tolist() == [tick + 2, tick + 4, 0, 0]             # every output is optional
    assert until(w, 0) == EINVAL                                    # chunk = 0
    assert lib.swim_run_until_recorded(c._h, w._w, 4, 8, 4, C.byref(t), C.byref(m), C.byref(r)) == EINVAL
    assert lib.swim_run_until_recorded(c._h, w._w, 0, 8, 4, None, C.byref(m), C.byref(r)) == EINVAL
    assert until(bare) == EINVAL                                    # this watch has no recording
    other = SimulatedCluster(engine, cfg_of(70))
    assert lib.swim_run_until_recorded(other._h, w._w, 0, 8, 4, C.byref(t), C.byref(m), C.byref(r)) == EINVAL
    other.close()
    assert lib.swim_watch_record_stop(w._w) == 0 and lib.swim_watch_record_stop(w._w) == 0
    assert until(w) == EINVAL and c.tick == tick + 5                # stopped: not armed
    c.step(4)
    assert w.recorded() == 3                                        # a stopped recording takes no more samples
    assert lib.swim_watch_record(w._w, 1, 4) == 0 and w.series().ticks.tolist() == [tick + 9]
    # swim_destroy with an armed recording is clean; closing the wrapper afterwards is a no-op
    c.close()
    w.close()
