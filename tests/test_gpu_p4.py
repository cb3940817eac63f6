"""P4, the gossip first-receipt phase, on caller-chosen receipts: the lane-serial fold (member.hip p4_receipts) and the
wave version (inbox.hip k_inbox_apply) against a plain reference and against each other.

swim_debug_receipts_set installs the routed receipts of a live handle's next tick (include/swimhip_debug.h), so the
batch sizes, repeated subjects, slow receipts, write-log fills and incarnation edges that whole-cluster runs only meet
by chance are forced here. The reference is tests/prim_ref.py p4_fold, a serial fold over dictionaries restating
onMembershipGossip -> updateMembership (MembershipProtocolImpl.java:401-408,475-541; SEMANTICS.md §7); pre-states other
than "ALIVE at incarnation 0" are made by the engine itself in a preparation tick that the reference folds too. The
engine takes a latency of one tick only, so the preparation tick's metadata requests are answered in the tick under
test, before P4 (prim_ref.p4_hops): P4 appends to a fetch list that already holds records.

Known answers compare, after the tick under test, every member's table, lists, scalars, write log, fetch records and
events with the reference by equality, on three launch paths (one BODY_FULL launch; the split triple with nobody parked;
the split triple with every member that has a receipt parked) and with the default threshold (parked and unparked members
in one block). What P4 does not decide (the pings of the same tick: correlation ids, messages) is taken out as the
difference to a twin handle that runs the same ticks with no receipt. The path-equality tests need no reference: the
same injection through the serial and the wave path, then 40 ticks of the engine's own gossip traffic, equal at every
tick."""
import re
from dataclasses import replace

import numpy as np
import pytest

import prim_ref as R
from swimhip import ClusterConfig, SimConfig, _abi
from swimhip.cluster import SimulatedCluster, SwimError

pytestmark = pytest.mark.gpu

# path -> (split launch, SWIM_CAPS): hv is the receipt count from which a member's P4 runs in k_inbox_apply
PATHS = {"full": (0, None), "split_nobody_parked": (1, "hv=1000000"), "split_all_parked": (1, "hv=1"),
         "split_hv24": (1, "hv=24")}
COUNTERS = ["record_compares", "row_writes", "messages", "events", "messages_lost", "gossips_created"]
HASH_COUNTERS = COUNTERS + ["gossip_messages", "sync_merges"]
FETCH_CAP = 64
E_FETCH, E_INC = 2, 1 << 20


def make(engine, monkeypatch, cfg, caps=None):
    if caps:
        monkeypatch.setenv("SWIM_CAPS", caps)
    try:
        return SimulatedCluster(engine, cfg)
    finally:
        if caps:
            monkeypatch.delenv("SWIM_CAPS")


def inject(c, tick, split):
    recs, lists = R.p4_pack(tick)
    rc = _abi.debug_receipts_set(c.lib, c._h, recs, lists, split)
    assert rc == 0, (rc, c.lib.swim_last_error(c._h))


def read_back(c, fetch_cap=FETCH_CAP):
    rc, out, msg = _abi.debug_receipts_read(c.lib, c._h, 0, c.n, c.n, fetch_cap, True)
    assert rc == 0, rc
    return out, msg


def restore(c):
    rc, _, _ = _abi.debug_receipts_read(c.lib, c._h, 0, 0, c.n)
    assert rc == 0, rc


def event_tuples(c):
    return [(e.tick, e.observer, e.seq, e.type, e.member, e.oldMetadata, e.newMetadata, e.gossipCounter)
            for e in c.events()]


def error_bits(c, n=1):
    """The device error bits of a step that must fail with a capacity error."""
    with pytest.raises(SwimError) as x:
        c.step(n)
    m = re.search(r"rc=(-?\d+).*error bits 0x([0-9a-f]+)", str(x.value))
    assert m, str(x.value)
    return int(m.group(1)), int(m.group(2), 16)


def ka_config(N, **kw):
    return SimConfig(n_members=N, cluster=ClusterConfig(), record_events=True, tick_ms=100, latency_ticks=1, **kw)


_KA = {}


def known_answer(engine, monkeypatch, N):
    """The case at N members, the reference's state after each of its ticks, and the twin handle's figures (the same
    kills and ticks, no receipt), computed once and left unchanged."""
    if N in _KA:
        return _KA[N]
    case = R.p4_case(N)
    c = make(engine, monkeypatch, ka_config(N))
    cfg = {"suspicion_mult": c.cfg.cluster.suspicionMult, "ping_t": c.cfg.cluster.pingInterval // c.cfg.tick_ms,
           "md_t": c.cfg.cluster.metadataTimeout // c.cfg.tick_ms, "lat": c.cfg.latency_ticks}
    members = []
    for m in range(N):
        fd, gl, _ = c.lists(m)
        members.append(R.p4_member(m, N, fd.tolist(), gl.tolist()))
    for m in case["killed"]:
        c.kill(m)
    twin, ref = [], []
    for k, tick in enumerate(case["ticks"]):
        inject(c, {}, 0)
        c.step(1)
        out, _ = read_back(c, 0)
        twin.append({"words": out.copy(), "counters": c.counters(), "cursors": [c.lists(m)[2] for m in range(N)]})
        # (the metadata requests of the tick before reach their subjects in this tick, ahead of P4)
        hops = sum(R.p4_hops(members[m], k, set(case["killed"]), cfg) for m in range(N))
        res = [R.p4_fold(members[m], k, *tick.get(m, (0, [])), set(case["killed"]), cfg) for m in range(N)]
        ref.append({"res": res, "events": [e for r in res for e in r["events"]],
                    "tot": {x: sum(r[x] for r in res) + (hops if x == "M" else 0) for x in ("R", "W", "M", "E", "LOST")},
                    "gossips": sum(len(r["gossips"]) for r in res),
                    "state": [{"row": R.p4_row_words(s, N), "fd": list(s["fd"]), "gl": list(s["gl"]), "tsize": s["tsize"],
                               "cid": s["cid"], "fetch": [list(f) for f in s["fetch"]], "fnext": s["fnext"],
                               "timerMin": s["timerMin"], "gcnt": s["gcnt"], "evseq": s["evseq"]} for s in members]})
    assert event_tuples(c) == [], "the twin emits no event in these ticks"
    assert ref[0]["gossips"] == 0 and ref[1]["gossips"] > 0
    c.close()
    # the same ticks with the receipts through the lane-serial path: what every path's read-back and list cursors are
    # compared with word for word, the words the reference does not restate included (held, the gossip cursor)
    c = make(engine, monkeypatch, ka_config(N))
    for m in case["killed"]:
        c.kill(m)
    for k, tick in enumerate(case["ticks"]):
        inject(c, tick, 0)
        c.step(1)
        out, _ = read_back(c)
        twin[k]["serial"] = out.copy()
        twin[k]["serial_cursors"] = [c.lists(m)[2] for m in range(N)]
    c.close()
    _KA[N] = (case, ref, twin)
    return _KA[N]


def compare_tick(c, N, case, ref, twin, k, out, msg, where):
    W = {n: i for i, n in enumerate(_abi.RD_NAMES)}
    tw = twin["words"]
    dead = set(case["killed"])
    # every receipt list was taken: by P4, or by the triage for a dead member (nothing applied, counts cleared). After
    # the preparation tick no list exists; after the tick under test its gossip plane has routed the next tick's
    # receipts of the live members (the refutations' first receipts), so only the dead members' counts are known
    left = msg[2 + N:].reshape(2, N)
    who = range(N) if k == 0 else sorted(dead)
    assert not left[:, who].any(), f"{where} tick {k}: rc_cnt / rc_fill left: {left[:, who].tolist()}"
    for m in range(N):
        s, r = ref["state"][m], ref["res"][m]
        at = f"{where} tick {k} member {m} ({case['who'].get(m, 'no receipts')})"
        row = c.row(m)
        bad = np.nonzero(row != s["row"])[0]
        assert len(bad) == 0, f"{at}: row differs at subjects {bad[:6].tolist()}: engine " \
                              f"{[hex(int(row[b])) for b in bad[:6]]} reference {[hex(int(s['row'][b])) for b in bad[:6]]}"
        fd, gl, cur = c.lists(m)
        assert fd.tolist() == s["fd"] and gl.tolist() == s["gl"], f"{at}: lists"
        # The ping cursor is P6's alone. The gossip cursor moves when a refutation of this tick is spread by the member's
        # gossip round in P6 of the same tick (selectGossipMembers); the reference restates P4 only, so for a refuting
        # member that cursor is compared with the lane-serial path's instead, like every other member's.
        assert cur[0] == twin["cursors"][m][0], f"{at}: ping cursor {cur} != {twin['cursors'][m]}"
        assert r["gossips"] or cur == twin["cursors"][m], f"{at}: list cursors {cur} != {twin['cursors'][m]}"
        assert cur == twin["serial_cursors"][m], f"{at}: list cursors {cur} != lane-serial {twin['serial_cursors'][m]}"
        o = out[m]
        got = {n: int(o[i]) for n, i in W.items()}
        # held, the member's gossip count: P4 adds one per refutation (spread). The gossip plane of the same tick then
        # delivers the refutations that their members' gossip rounds sent in P6, so other live members' counts rise by
        # first receipts that this reference does not restate: equality where no gossip exists (the preparation tick,
        # dead members), a lower bound elsewhere, and equality with the lane-serial path for every member
        dh = got["held"] - int(tw[m][W["held"]])
        if k == 0 or m in dead:
            assert dh == 0, f"{at}: held {got['held']} twin {tw[m][W['held']]}"
        assert dh >= len(r["gossips"]), f"{at}: held rose by {dh}, {len(r['gossips'])} refutations"
        assert o.tolist() == twin["serial"][m].tolist(), f"{at}: read-back differs from the lane-serial path's"
        assert got["tsize"] == s["tsize"] and got["nfetch"] == len(s["fetch"]), f"{at}: {got}"
        assert got["fnext"] == s["fnext"] and got["timerMin"] == s["timerMin"], f"{at}: {got} {s['fnext']} {s['timerMin']}"
        # P6's ping of this tick takes a correlation id after P4's: the twin's count is that part
        assert got["cidCnt"] - int(tw[m][W["cidCnt"]]) == s["cid"], f"{at}: cidCnt {got['cidCnt']} twin {tw[m][W['cidCnt']]}"
        assert got["gCounter"] - int(tw[m][W["gCounter"]]) == s["gcnt"], f"{at}: gCounter"
        assert got["evSeq"] - int(tw[m][W["evSeq"]]) == s["evseq"], f"{at}: evSeq"
        assert got["tl_n"] == r["tl_n"], f"{at}: write-log length {got['tl_n']} != {r['tl_n']}"
        assert o[9:9 + _abi.DEBUG_TL].tolist() == r["tl"] + [0] * (_abi.DEBUG_TL - len(r["tl"])), f"{at}: write log"
        # the fetch records carry P4's correlation ids themselves: the count before the tick plus i
        want = [w for f in s["fetch"] for w in f]
        assert len(s["fetch"]) <= FETCH_CAP
        assert o[_abi.DEBUG_RD_WORDS:_abi.DEBUG_RD_WORDS + len(want)].tolist() == want, f"{at}: fetch records"
    assert _abi.debug_dirty_check(c.lib, c._h) == 0


@pytest.mark.parametrize("path", list(PATHS))
# (66: the table holds 64 records after the preparation tick, so one removal in the tick under test changes the
# suspicion timeout's ceilLog2(size): a deadline computed from a stale size differs)
@pytest.mark.parametrize("N", [66, 96, 300])
def test_p4_known_answer(engine, monkeypatch, N, path):
    case, ref, twin = known_answer(engine, monkeypatch, N)
    split, caps = PATHS[path]
    c = make(engine, monkeypatch, ka_config(N), caps)
    for m in case["killed"]:
        c.kill(m)
    # the preparation tick, through the lane-serial path on every handle
    inject(c, case["ticks"][0], 0)
    c.step(1)
    out, msg = read_back(c)
    compare_tick(c, N, case, ref[0], twin[0], 0, out, msg, path)
    # the tick under test
    inject(c, case["ticks"][1], split)
    c.step(1)
    out, msg = read_back(c)
    compare_tick(c, N, case, ref[1], twin[1], 1, out, msg, path)
    got = event_tuples(c)
    want = sorted(ref[0]["events"] + ref[1]["events"], key=lambda e: e[:3])
    assert len(got) == len(want), (len(got), len(want))
    for a, b in zip(got, want):
        assert a == b, f"{path}: event {a} != reference {b}"
    cnt = c.counters()
    names = dict(zip(COUNTERS, ("R", "W", "M", "E", "LOST")))
    for key, x in names.items():
        delta = cnt[key] - twin[1]["counters"][key]
        assert delta == ref[0]["tot"][x] + ref[1]["tot"][x], (key, delta)
    assert cnt["gossips_created"] - twin[1]["counters"]["gossips_created"] == ref[1]["gossips"]
    c.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_p4_incarnation_limit_is_the_same_error_on_every_path(engine, monkeypatch, path):
    """One record at incarnation 2^30 (in a short list, and as receipt 64 of 71): the kernels' own E_INC."""
    N = 96
    case = R.p4_case_einc(N)
    split, caps = PATHS[path]
    c = make(engine, monkeypatch, ka_config(N), caps)
    inject(c, case["ticks"][0], split)
    rc, bits = error_bits(c)
    assert (rc, bits) == (_abi.SWIM_ECAPACITY, E_INC), (rc, hex(bits))
    restore(c)
    c.close()


# ------------------------------------------------------------------------------------------------------ path equality
def gossips_of(c, members):
    return [c.gossips(m, cap=1 << 15) for m in members]  # (no handle here has more slots)


def run_pair(engine, monkeypatch, cfg, setup, ticks, further=40, sample=None, before=0, split_all=False, between=None):
    """The same injections on a handle that takes the lane-serial path (one BODY_FULL launch) and on one whose parked
    members take the wave path (split, hv = 1; the last injected tick, or all of them), then `further` ticks of the
    engine's own traffic: equal at every tick, and equal in every read-back word after each injected tick.
    between(c, i): host calls before injected tick i. Returns both handles' message read-backs of the last injected tick."""
    full, wave = make(engine, monkeypatch, cfg), make(engine, monkeypatch, cfg, "hv=1")
    msgs, outs = [], []
    for c, split in ((full, 0), (wave, 1)):
        setup(c)
        if before:
            c.step(before)
        outs.append([])
        for i, tick in enumerate(ticks):
            if between:
                between(c, i)
            inject(c, tick, split if split_all or i == len(ticks) - 1 else 0)
            c.step(1)
            out, msg = read_back(c, 16)
            outs[-1].append(out)
        msgs.append(msg)
    for i, (a, b) in enumerate(zip(*outs)):  # tsize, ids, fetch list, timers, held, counters of the member, write log
        bad = np.nonzero((a != b).any(axis=1))[0]
        assert len(bad) == 0, f"injected tick {i}: read-back differs at members {bad[:6].tolist()}: " \
                              f"{a[bad[0]][:25].tolist()} != {b[bad[0]][:25].tolist()}"
    members = list(range(cfg.n_members)) if sample is None else sample
    for t in range(further + 1):
        where = f"{t} ticks after the injected one"
        hf, hw = full.state_hash(), wave.state_hash()
        bad = np.argwhere(hf != hw)
        assert len(bad) == 0, f"{where}: state hash differs at (member, word) {bad[:4].tolist()}"
        cf, cw = full.counters(), wave.counters()
        assert [cf[k] for k in HASH_COUNTERS] == [cw[k] for k in HASH_COUNTERS], f"{where}: counters {cf} {cw}"
        assert event_tuples(full) == event_tuples(wave), f"{where}: events"
        # (with a sample, the other members' gossips are compared through the state hash's gossips-held word alone)
        assert gossips_of(full, members) == gossips_of(wave, members), f"{where}: gossips held"
        if t < further:
            full.step(1)
            wave.step(1)
    assert full.counters()["gossips_created"] > 0
    full.close()
    wave.close()
    return msgs


def test_paths_agree_under_loss(engine, monkeypatch):
    """(a) default loss 15 %: the loss draws of the metadata requests are keyed by their correlation ids."""
    N = 120
    case = R.p4_case(N, top=1000)  # (the run goes on: see p4_case)

    def setup(c):
        c.set_default_loss(15)
        for m in case["killed"]:
            c.kill(m)

    run_pair(engine, monkeypatch, ka_config(N, pending_fetch_cap=1024, list_slack=1024), setup, case["ticks"])


def sync_case(N):
    """Case (b): two injected ticks. Members fall into four classes (m % 4) that are told different things about eight
    subjects, so that rows differ between classes and every SYNC / SYNC_ACK payload matters by value. Tick A: class c hears
    of its own two subjects. Tick B: everyone hears of all eight, at incarnations that rise with the class, on top of what
    P1 of that tick merged from the payloads sent after tick A (a write log that already has entries, and whose last
    entry may be the first receipt's subject, when the member is parked); a few members also refute, and a few got
    swim_update_incarnation before the tick (P0 writes the row and the log before the member parks)."""
    subj = list(range(8, 16))
    A, B = {}, {}
    for m in range(N):
        c = m % 4
        mine = [s for s in subj[2 * c:2 * c + 2] if s != m]
        A[m] = (1, [("M", mine[0], R.P4_SUSPECT, 0), ("M", mine[-1], R.P4_ALIVE, 1), ("M", mine[0], R.P4_ALIVE, 2)])
        lst = []
        for s in subj:
            if s != m:
                lst += [("M", s, R.P4_ALIVE, 3 + c), ("M", s, R.P4_SUSPECT, 3 + c)]
        B[m] = (m % 3, lst + ([("M", m, R.P4_SUSPECT, 0)] if m % 40 == 7 else []))
    return [A, B]


def test_paths_agree_with_sync_payloads_in_flight(engine, monkeypatch):
    """(b) a SYNC every second: at the injected ticks many members have answered a SYNC before P4, and the SYNC_ACK still
    carries their live row. An accepted receipt then needs the row's snapshot first: the serial path's copy-on-write,
    the wave's own copy. Rows differ between member classes (sync_case), so a snapshot taken after the row write would
    hand the receiver of class c' < c records it must not have yet. The read-back shows that parked senders did take
    arena rows. swim_read_gossips copies the whole slot table per call (12 800 slots here), so it is read for every
    fourth member at every tick and the others are compared through the state hash's gossips-held word."""
    N = 200
    cfg = replace(ka_config(N, pending_fetch_cap=1024, list_slack=1024), cluster=ClusterConfig(syncInterval=1000))

    def between(c, i):
        if i == 1:
            for m in range(3, N, 25):
                c.update_incarnation(m)

    full, wave = run_pair(engine, monkeypatch, cfg, lambda c: None, sync_case(N), before=3, sample=list(range(0, N, 4)),
                          split_all=True, between=between)
    senders = int((wave[2:2 + N] > 0).sum())
    assert wave[1] > 0 and senders >= 1, "no parked member's SYNC_ACK took a snapshot: nothing tested"
    assert full.tolist() == wave.tolist(), (full[:2], wave[:2], senders)


def test_paths_agree_past_8192_parked_members(engine, monkeypatch):
    """(c) 8320 members with one or two receipts each and hv = 1: k_inbox_apply's grid (2048 blocks of four waves) takes a
    second trip of its grid-stride loop. Every 500th member also refutes a SUSPECT record about itself, so the 40 ticks
    that follow carry gossip receipts to everyone; swim_read_gossips copies the slot table per call, so it is read for
    every 521st member and the rest is compared through the state hash."""
    N = 8320
    tick = {}
    for m in range(N):
        p = [s for s in range(4) if s != m]  # (the same few subjects for everyone: the later SYNCs merge nothing)
        tick[m] = (0, [("M", p[0], R.P4_SUSPECT, 0)] + ([("M", p[1 + m % 2], R.P4_ALIVE, 1)] if m % 3 else []) +
                   ([("M", m, R.P4_SUSPECT, 0)] if m % 500 == 0 else []))
    cfg = ka_config(N, gossip_slot_cap=32768, pending_fetch_cap=1024)
    run_pair(engine, monkeypatch, cfg, lambda c: None, [tick], sample=list(range(0, N, 521)))


def test_fetch_list_overflow_is_the_same_error_on_both_paths(engine, monkeypatch):
    """(d) a fetch list of four records and six accepted incarnation increases: E_FETCH from both paths."""
    N = 96
    tick = {5: (0, [("M", 10 + j, R.P4_ALIVE, 1) for j in range(6)]),
            70: (0, [("M", j % 7, R.P4_ALIVE, 1 + j // 7) for j in range(70)])}
    got = []
    for split, caps in ((0, None), (1, "hv=1")):
        c = make(engine, monkeypatch, ka_config(N, pending_fetch_cap=4), caps)
        inject(c, tick, split)
        got.append(error_bits(c))
        restore(c)
        c.close()
    assert got[0] == got[1] == (_abi.SWIM_ECAPACITY, E_FETCH), got


def test_injector_refuses_what_it_cannot_install(engine, monkeypatch):
    N = 64
    c = make(engine, monkeypatch, ka_config(N))
    ok = [(0, 1, 1, 1, 1, 0)]
    bad = [([(0, N, 1, 1, 1, 0)], {0: (0, [0])}), ([(0, 1, 0, 1, 1, 0)], {0: (0, [0])}), ([(0, 1, 4, 1, 1, 0)], {0: (0, [0])}),
           ([(1, N, 0, 0, 0, 0)], {0: (0, [0])}), ([(2, 1, 1, 1, 1, 0)], {0: (0, [0])}), (ok, {N: (0, [0])}),
           (ok, {0: (0, [1])}), (ok, [0, 0, 1, 0, 0, 0, 1, 0]), (ok, [0, 0, 2, 0])]
    cap = _abi.debug_caps(c.lib, c._h)
    bad.append((ok, {0: (0, [0] * (cap["receipts"] + 1))}))
    bad.append(([(0, 1, 1, i, 1, 0) for i in range(cap["slots"] + 1)], {}))
    before = c.state_hash()
    for recs, lists in bad:
        assert _abi.debug_receipts_set(c.lib, c._h, recs, lists, 0) == _abi.SWIM_EINVAL, (recs[:2], lists)
    assert _abi.debug_receipts_read(c.lib, c._h, 0, 1, N)[0] == _abi.SWIM_EINVAL  # nothing was installed
    c.step(3)
    assert np.array_equal(c.state_hash()[:, 0], before[:, 0]) and c.counters()["row_writes"] == 0
    # an incarnation of 2^30 is not the injector's to refuse; a second injection before the read-back is
    assert _abi.debug_receipts_set(c.lib, c._h, [(0, 1, 1, 1 << 30, 1, 0)], {}, 0) == 0
    assert _abi.debug_receipts_set(c.lib, c._h, ok, {}, 0) == _abi.SWIM_EINVAL
    restore(c)
    c.update_incarnation(3)
    c.step(2)  # a gossip in flight: real routed receipts would collide with injected ones
    assert _abi.debug_receipts_set(c.lib, c._h, ok, {0: (0, [0])}, 0) == _abi.SWIM_EINVAL
    c.close()
    r = make(engine, monkeypatch, SimConfig(n_members=N, mode=_abi.MODE_RUMOR, churn_per_period=4))
    assert _abi.debug_receipts_set(r.lib, r._h, ok, {0: (0, [0])}, 0) == _abi.SWIM_EINVAL
    r.close()
