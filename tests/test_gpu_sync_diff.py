"""Known answers for the SYNC diff (k_sync_diff) and its lister (k_ack_resolve), through SWIM_PRIM_SYNC_DIFF of
swim_debug_prim_eval (include/swimhip_debug.h): the two kernels run on a Dev that holds only what they read, queued by
launch_diff / launch_diff_listed as a step queues them, on chosen rows, messages, logs and masks, and every output is
compared bit for bit with the plain references of tests/prim_ref.py (validated without a GPU in tests/test_prim_ref.py).
Integer code: no tolerance appears anywhere. Engine only.

Whole clusters feed the diff rows that are equal almost everywhere, at the sizes a test can simulate, and one item per
block. Here the sizes sit at the segment, chunk, item and mask-word edges (up to three mask words, which no stored
table a test can build has), the differences at the lane, segment and chunk edges, with escaped keys (>= 0xFF) next to
them, and the grids 1, 2, 3 and 7 rotate the software pipeline of stream_narrow / stream_wide many times per block.
"""
import functools

import numpy as np
import pytest

import prim_ref as R
from swimhip import _abi

pytestmark = pytest.mark.gpu

NEVER, CH, MCH, TL = R.NEVER, R.CH, R.MCH, R.TL
GRIDS = [1, 2, 3, 7, 0]  # 0: the engine's own grid
SENT = R.SD_SENT


def run(engine, case):
    params, inp, out = R.sd_pack(case)
    _abi.prim_eval(engine, _abi.PRIM_SYNC_DIFF, params, inp, out)
    return R.sd_unpack(case, out)


def check(case, res, exp, absent_set, overflow=False, whole=()):
    """What the kernels left against exp (per message: {segment: words} it must have written; other segments untouched).
    With overflow a segment may instead report (NEVER, 0), written nothing; a message of `whole` (resolved by the
    lister, which reserves all its candidates at once) may instead have written nothing at all, ncand = 0."""
    z = R.sd_sizes(case["N"])
    cap, pool, used = case["POOLCAP"], res["pool"], res["pool_used"]
    owned = np.zeros(cap, bool)
    attempted = 0
    for i, (m, e) in enumerate(zip(case["msgs"], exp)):
        got = 0
        if overflow and i in whole and (res["meta"][i] == SENT).all():
            assert int(res["ncand"][i]) == 0 and int(res["kind"][i]) == m["kind"], (i, "no room: nothing written")
            attempted += sum(len(w) for w in e["segs"].values())
            continue
        for g in range(z["NMETA"]):
            off, cnt = int(res["meta"][i, g, 0]), int(res["meta"][i, g, 1])
            if g not in e["segs"]:
                assert (off, cnt) == (SENT, SENT), (i, g, "a segment nobody streams is not written")
                continue
            want = e["segs"][g]
            attempted += len(want)
            if overflow and len(want) and cnt == 0:
                assert off == NEVER, (i, g, "a segment without room reports (NEVER, 0)")
                continue
            assert cnt == len(want), (i, g, off, cnt, len(want))
            if cnt:
                assert off + cnt <= min(used, cap), (i, g, "inside the pool")
                assert not owned[off:off + cnt].any(), (i, g, "ranges are disjoint")
                owned[off:off + cnt] = True
                bad = np.flatnonzero(pool[off:off + cnt] != want)
                assert len(bad) == 0, (i, g, [(hex(int(pool[off + j])), hex(int(want[j]))) for j in bad[:4]])
            got += cnt
        assert int(res["ncand"][i]) == got, (i, "ncand counts what was written", int(res["ncand"][i]), got)
        assert int(res["kind"][i]) == m["kind"] | (R.KF_ABS if absent_set and e["absent"] else 0), (i, hex(int(res["kind"][i])))
    assert used == attempted, "pool_used is the total count (segments without room included)"
    assert overflow or used <= cap
    assert res["err"] == (R.E_POOL if used > cap else 0)
    assert (pool[:cap][~owned] == np.uint64(R.SD_SENT64)).all(), "pool words nobody owns keep the sentinel"
    assert (pool[cap:] == np.uint64(R.SD_SENT64)).all() and len(pool) == cap + 64, "guard words"


def check_pins(case, res, entries):
    """A pinned payload's arena row equals the sender's row; the other arena rows are unchanged."""
    lo, pinned = case.get("lo", 0), {}
    for i, src, dst, w in entries:
        if w not in (NEVER, R.DESC_DEFER) and w & R.DESC_PIN:
            pinned[w & ~R.DESC_PIN] = src - lo
    for a in range(len(case.get("arena", []))):
        want = case["rows"][pinned[a]] if a in pinned else case["arena"][a]
        assert np.array_equal(res["arena"][a], want), ("arena row", a, a in pinned)


# ------------------------------------------------------------------------------------------------------------ rows
def key(inc, st):
    return (np.asarray(inc, np.uint32) << np.uint32(2)) | np.asarray(st, np.uint32)


EDGE_SUBJECTS = [0, 31, 32, 1023, 1024, 2047, 2048, 8191, 8192]


@functools.lru_cache(maxsize=None)
def rows_for(N):
    """Eight rows over one baseline (rows are read-only: shared by every test of a size).
    0 the baseline; 1 one changed subject at each edge; 2 all ABSENT (a joiner), at subjects 0 and N - 1 with
    incarnation bits >= 64 under the ABSENT status (against row 7's absent records there, only the receiver's shadow
    escapes, and its status bits read 3: the lane must compare the 4-B keys); 3 / 4 1 % / 50 % changed, some to ABSENT; 5 / 6 escaped keys (>= 0xFF) at lanes' first and last subjects: in 5 only, in 6 only, equal in both, different
    in both, next to a lane that differs on small keys only, and status-only differences; 7 some subjects ABSENT."""
    z = R.sd_sizes(N)
    rng = np.random.default_rng(7000 + N)
    base = np.zeros(z["NS"], np.uint32)
    base[:N] = key(rng.integers(0, 40, N), rng.integers(1, 4, N))
    rows = np.tile(base, (8, 1))
    for s in EDGE_SUBJECTS + [N - 1]:
        if s < N:
            rows[1, s] += 4  # the next incarnation
    rows[2] = 0
    rows[2, [0, N - 1]] = key([64, 2**30 - 1], 0)
    for r, frac in ((3, 0.01), (4, 0.5)):
        ch = np.flatnonzero(rng.random(N) < frac)
        rows[r, ch] = key(rng.integers(0, 40, len(ch)), rng.integers(0, 4, len(ch)))
        rows[r, ch[::7]] = 0
    big = lambda n: key(rng.integers(64, 2**30, n), rng.integers(1, 4, n))
    for o in (0, 1024, 2048, 4096 + 1024, (z["NCHUNK"] - 1) * CH):
        if o + 11 * 32 > N:
            continue
        L = lambda lane, j: o + 32 * lane + j
        rows[5, [L(2, 0), L(3, 31)]] = big(2)                    # in the payload only (5 -> 6), the receiver only (6 -> 5)
        rows[6, [L(4, 31), L(4, 0)]] = big(2)
        rows[5, L(5, 7)] = rows[6, L(5, 7)] = big(1)[0]          # equal in both
        a, b = big(2), big(2)
        b[b == a] += 4
        rows[5, [L(6, 0), L(7, 31)]], rows[6, [L(6, 0), L(7, 31)]] = a, b  # >= 0xFF in both, different: equal shadows
        rows[5, L(8, 3)] += 4                                    # lane 8 differs on small keys only, lanes 7 and 9 escape
        rows[6, L(9, 0)] = big(1)[0]
        rows[5, L(10, 5)] = (rows[5, L(10, 5)] & ~np.uint32(3)) | (rows[5, L(10, 5)] % 3 + 1)
    rows[5, N - 1] = big(1)[0]
    st = np.flatnonzero(rng.random(N) < 0.002)                   # only the status bits differ
    rows[5, st] = (rows[5, st] & ~np.uint32(3)) | ((rows[5, st] & 3) % 3 + 1)
    ab = np.flatnonzero(rng.random(N) < 0.003)
    rows[7, ab] = 0
    rows[7, [0, N - 1]] = 0
    rows.setflags(write=False)
    return rows


PAIRS = [(0, 0), (1, 0), (0, 1), (0, 2), (2, 0), (2, 2), (3, 0), (0, 3), (4, 0), (0, 4), (4, 3), (5, 6), (6, 5), (5, 0),
         (0, 5), (7, 0), (7, 2), (0, 7), (5, 4), (1, 7)]


def poolcap_for(N):
    return 6 * N + 64  # above the total of PAIRS (two joiners' N each, four times about N / 2, small ones)


def all_items(z, i, src, dst):
    out = []
    for t in range(z["nit"]):
        nv = min(R.NPER, z["NCHUNK"] - R.NPER * t)
        out.append((i, src, dst, t << 4 | ((1 << nv) - 1)))
    return out


def expected_counters(**kw):
    c = dict.fromkeys(R.SD_CTR, 0)
    c.update(kw)
    return c


# ------------------------------------------------------------------------------------------------------------ mode A
@pytest.mark.parametrize("N", R.SD_NS)
def test_every_message_wide_without_lists(engine, N):
    """ackres = 0: k_sync_diff reads the messages themselves, all on 4-B keys: live rows, pinned live rows (copied into
    the arena as they stream), arena snapshots and delayed messages (zero counts)."""
    rows = rows_for(N)
    arena = np.zeros((6, rows.shape[1]), np.uint32)
    arena[4], arena[5] = rows[4], rows[5]  # snapshots: rows 0 .. 3 take pinned copies
    arena[4, :N:5] = rows[1, :N:5]
    msgs = []
    for j, (s, d) in enumerate(PAIRS):
        kind = j % 4
        msgs.append(R.sd_msg(s, d, kind=1 | (R.KF_DEFER if kind == 3 else 0), payload=4 + j % 2 if kind == 2 else NEVER,
                             pin=len([m for m in msgs if m["pin"] != NEVER]) if kind == 1 and j < 16 else NEVER))
    case = dict(N=N, rows=rows, arena=arena, msgs=msgs, flags=0, POOLCAP=poolcap_for(N), k=4)
    wide = [(i, m["src"], m["dst"], R.desc_pay(m)) for i, m in enumerate(msgs)]
    exp, _ = R.sd_expect(case, [], wide)
    for grid in GRIDS:
        res = run(engine, dict(case, grid=grid))
        check(case, res, exp, absent_set=False)  # KF_ABS is the lister's business: only set with ackres
        check_pins(case, res, wide)
        assert res["ctr"] == expected_counters(diffmsg_all=len(msgs), diffwide_all=len(msgs)), grid
        assert (res["cstat"] == 0).all() and (res["pin"] == [m["pin"] for m in msgs]).all()


def listed_case(N):
    """Messages of PAIRS split over the two lists: even ones narrow (every item, every chunk), odd ones wide as live row,
    pinned copy, snapshot or delayed message in turn."""
    rows = rows_for(N)
    z = R.sd_sizes(N)
    arena = np.zeros((4, rows.shape[1]), np.uint32)
    arena[3] = rows[3]
    arena[3, 1:N:3] = rows[4, 1:N:3]
    msgs, narrow, wide = [], [], []
    for j, (s, d) in enumerate(PAIRS):
        if j % 2 == 0:
            msgs.append(R.sd_msg(s, d))
            narrow += all_items(z, j, s, d)
            continue
        kind = (j // 2) % 4
        npin = len([m for m in msgs if m["pin"] != NEVER])
        m = R.sd_msg(s, d, kind=1 | (R.KF_DEFER if kind == 3 else 0), payload=3 if kind == 2 else NEVER,
                     pin=npin if kind == 1 and npin < 3 else NEVER)
        msgs.append(m)
        wide.append((j, s, d, R.desc_pay(m)))
    rng = np.random.default_rng(N)
    narrow = [narrow[i] for i in rng.permutation(len(narrow))]  # atomics decide a real list's order
    wide = [wide[i] for i in rng.permutation(len(wide))]
    return dict(N=N, rows=rows, arena=arena, msgs=msgs, narrow=narrow, wide=wide, flags=R.SD_LISTS | R.SD_K8,
                POOLCAP=poolcap_for(N), k=7)


@pytest.mark.parametrize("N", R.SD_NS)
def test_narrow_and_wide_lists(engine, N):
    case = listed_case(N)
    exp, differed = R.sd_expect(case, case["narrow"], case["wide"])
    for grid in GRIDS:
        res = run(engine, dict(case, grid=grid))
        check(case, res, exp, absent_set=True)
        check_pins(case, res, case["wide"])
        assert res["ctr"] == expected_counters(diffwide_all=len(case["wide"])), grid
        assert np.array_equal(res["cstat"][:, 1], differed), (grid, "narrow chunk compares that differed")
        assert (res["cstat"][:, [0, 2]] == 0).all()
        assert res["nnar"] == len(case["narrow"]) and res["nwide"] == len(case["wide"])


def test_item_chunk_bits(engine):
    """Entries with each of the 15 chunk-bit patterns: a chunk whose bit is clear gets zero counts although the rows
    differ (that is the lister's promise); N = 8200 has a full item and a second one with one partial chunk."""
    N = 8200
    rows, z = rows_for(N), R.sd_sizes(N)
    msgs, narrow = [], []
    for m4 in range(1, 16):
        s, d = [(4, 0), (0, 2), (5, 6), (7, 0)][m4 % 4]
        msgs.append(R.sd_msg(s, d))
        narrow.append((m4 - 1, s, d, 0 << 4 | m4))
        if m4 % 2:
            narrow.append((m4 - 1, s, d, 1 << 4 | 1))  # the item of the last, partial chunk (odd ones: the item not listed)
    case = dict(N=N, rows=rows, msgs=msgs, narrow=narrow, wide=[], flags=R.SD_LISTS | R.SD_K8, POOLCAP=poolcap_for(N), k=2)
    exp, differed = R.sd_expect(case, narrow, [])
    assert any(len(e["segs"]) == z["NMETA"] for e in exp) and any(len(e["segs"]) < z["NMETA"] for e in exp)
    for grid in GRIDS:
        res = run(engine, dict(case, grid=grid))
        check(case, res, exp, absent_set=True)
        assert np.array_equal(res["cstat"][:, 1], differed), grid


@pytest.mark.parametrize("N", [2056, 8200])
def test_pool_overflow_is_a_capacity_error(engine, N):
    """POOLCAP below the total: E_POOL, every segment either complete inside the pool or (NEVER, 0) with nothing written,
    ncand counts what was written, the guard words keep the sentinel."""
    case = listed_case(N)
    exp, _ = R.sd_expect(case, case["narrow"], case["wide"])
    total = sum(len(w) for e in exp for w in e["segs"].values())
    for cap in (total // 2, total - 1, 3):
        for grid in (1, 3, 0):
            c = dict(case, POOLCAP=cap, grid=grid)
            res = run(engine, c)
            assert res["err"] == R.E_POOL and res["pool_used"] == total
            check(c, res, exp, absent_set=True, overflow=True)
    c = dict(case, POOLCAP=total)  # exactly enough room is no error
    check(c, run(engine, c), exp, absent_set=True)


# ---------------------------------------------------------------------------------------------------- mode A, W = 2
def sharded_case(N, seed):
    """A row shard (W = 2, lo = 3, four rows): payloads received from the other shard as baseline + shipped chunks by
    mask (random masks and their complements, so every chunk is met shipped and unshipped, with shipped chunks in
    earlier mask words), on the narrow and on the wide list, next to local live rows and a pinned one."""
    z = R.sd_sizes(N)
    rng = np.random.default_rng(seed)
    all8 = rows_for(N)
    lo, rows = 3, all8[[0, 1, 5, 6]]
    base = all8[0]
    full = (1 << z["NCHUNK"]) - 1
    m0 = int.from_bytes(rng.bytes(8 * z["MW"]), "little") & full
    m0 |= 1 | 1 << (z["NCHUNK"] - 1)  # the first and the last (partial) chunk shipped in one payload, not in the other
    masks = [m0, full & ~m0, full, 0]
    content = [all8[5], all8[6], all8[4], all8[0]]  # escapes inside shipped chunks; 50 % changed; nothing shipped
    rx, chunks_all = [], []
    for mask, src_row in zip(masks, content):
        ch = [np.zeros(CH, np.uint32) for c in range(z["NCHUNK"]) if (mask >> c) & 1]
        for j, c in enumerate(c for c in range(z["NCHUNK"]) if (mask >> c) & 1):
            n = min(CH, z["NS"] - c * CH)
            ch[j][:n] = src_row[c * CH:c * CH + n]
        rx.append(dict(mask=mask, chunks=ch))
        chunks_all.append(ch)
    order = [2, 0, 3, 1]  # the receive buffer holds the payloads in another order than their indices
    off, recv = 0, []
    for ri in order:
        rx[ri]["off"] = off
        recv += chunks_all[ri]
        off += 4 * CH * len(chunks_all[ri])
    recv = np.array(recv, np.uint32).reshape(-1, CH) if recv else np.zeros((0, CH), np.uint32)
    arena = np.zeros((1, z["NS"]), np.uint32)
    msgs, narrow, wide = [], [], []
    for ri in range(4):
        for dst in (lo + 0, lo + 2, lo + 3):
            i = len(msgs)
            msgs.append(R.sd_msg(ri * 1000 % N if ri else N - 1, dst, payload=R.PAY_RX | ri))
            (narrow if (ri + dst) % 2 else wide).append((i, msgs[i]["src"], dst, R.PAY_RX | ri))
    for s, d, pin in ((lo + 2, lo + 3, NEVER), (lo + 1, lo + 0, NEVER), (lo + 3, lo + 2, 0), (lo + 3, lo + 1, NEVER)):
        i = len(msgs)
        msgs.append(R.sd_msg(s, d, pin=pin))
        if pin != NEVER or i % 2:
            wide.append((i, s, d, R.desc_pay(msgs[i])))
        else:
            narrow.append((i, s, d, NEVER))
    return dict(N=N, rows=rows, arena=arena, msgs=msgs, narrow=narrow, wide=wide, lo=lo, rx=rx, base=base, recv=recv,
                flags=R.SD_LISTS | R.SD_K8 | R.SD_SHARDED, POOLCAP=8 * N + 64, k=5)


@pytest.mark.parametrize("N", [8200, 131080, 262152])  # MW = 1, 2, 3
def test_sharded_received_payloads(engine, N):
    case = sharded_case(N, 90 + N)
    exp, _ = R.sd_expect(case, case["narrow"], case["wide"])
    assert sum(len(w) for e in exp for w in e["segs"].values()) > 0
    for grid in GRIDS:
        res = run(engine, dict(case, grid=grid))
        check(case, res, exp, absent_set=True)
        check_pins(case, res, case["wide"])
        assert res["ctr"] == expected_counters(), "on a row shard the lister counts"
        assert (res["cstat"] == 0).all()
    # without lists (ackres = 0) every message streams wide through pay_keys
    c2 = dict(case, flags=R.SD_K8 | R.SD_SHARDED, narrow=[], wide=[], grid=3)
    wide = [(i, m["src"], m["dst"], R.desc_pay(m)) for i, m in enumerate(case["msgs"])]
    res = run(engine, c2)
    check(c2, res, R.sd_expect(c2, [], wide)[0], absent_set=False)
    assert res["ctr"] == expected_counters(diffmsg_all=len(wide), diffwide_all=len(wide))


# ------------------------------------------------------------------------------------------------------------ mode B
def inbound(case):
    """m_head / m_next as the member kernel links them: each receiver's messages in index order."""
    n, R_ = len(case["msgs"]), len(case["rows"])
    head, nxt, last = np.full(R_, NEVER, np.uint32), np.full(n, NEVER, np.uint32), {}
    for i, m in enumerate(case["msgs"]):
        if m["dst"] in last:
            nxt[last[m["dst"]]] = i
        else:
            head[m["dst"]] = i
        last[m["dst"]] = i
    case["m_head"], case["m_next"] = head, nxt
    return case


def lister_expect(case, ref, diff_runs):
    """exp / the two lists / the counters that follow from ack_resolve_ref's verdicts."""
    z = R.sd_sizes(case["N"])
    narrow, wide = [], []
    ctr = expected_counters()
    exp_res = {}
    cstat0 = np.zeros(z["NCHUNK"], np.int64)
    senders = [set() for _ in range(z["NCHUNK"])]
    for i, (m, v) in enumerate(zip(case["msgs"], ref)):
        if v["how"] == "resolved":
            ctr["ackres_all"] += 1
            w = np.array(v["cand"], np.uint64)
            cut = np.searchsorted(w >> np.uint64(34), np.arange(z["NMETA"] + 1) * MCH)
            exp_res[i] = {g: w[cut[g]:cut[g + 1]] for g in range(z["NMETA"])} if len(w) else {}
            continue
        ctr["diffmsg_all"] += 1
        if v["how"] == "wide":
            wide.append((i, m["src"], m["dst"], v["place"]))
            continue
        if v["how"] in ("pin", "decided"):
            ctr["dmsgskip"] += 1
            ctr["pindec"] += v["how"] == "pin"
            continue
        for t, m4 in v["items"].items():
            narrow.append((i, m["src"], m["dst"], t << 4 | m4))
            for j in range(R.NPER):
                if (m4 >> j) & 1:
                    cstat0[R.NPER * t + j] += 1
                    senders[R.NPER * t + j].add(m["src"])
        nch = sum(bin(m4).count("1") for m4 in v["items"].values())
        last = z["NCHUNK"] - 1
        ctr["dstream"] += nch
        ctr["dsubj_all"] += nch * CH - ((z["NCHUNK"] * CH - case["N"]) if (v["items"].get(last // R.NPER, 0) >> last % R.NPER) & 1 else 0)
    if diff_runs:
        ctr["diffwide_all"] = len(wide)
    exp, differed = R.sd_expect(case, narrow if diff_runs else [], wide if diff_runs else [])
    for i, v in enumerate(ref):
        if v["how"] == "resolved":
            exp[i]["segs"] = exp_res[i]
        elif v["how"] == "narrow":  # the items without a chunk to stream get their zero counts from the lister
            for t in range(z["nit"]):
                if t not in v["items"]:
                    for g in range(2 * R.NPER * t, min(2 * R.NPER * (t + 1), z["NMETA"])):
                        exp[i]["segs"][g] = np.zeros(0, np.uint64)
    return exp, narrow, wide, ctr, cstat0, senders, differed


def check_lister(engine, case, grids=(0,)):
    ref = R.ack_resolve_ref(case)
    masks = bool(case["flags"] & R.SD_DIRTY)
    elidable = masks and bool(case["flags"] & R.SD_K8)
    diff_runs = not (elidable and case.get("ls", 0) & R.LS_NODIFF)
    exp, narrow, wide, ctr, cstat0, senders, differed = lister_expect(case, ref, diff_runs)
    for grid in grids:
        res = run(engine, dict(case, grid=grid))
        assert res["nnar"] == len(narrow) and res["nwide"] == len(wide), (res["nnar"], len(narrow), res["nwide"], len(wide))
        assert set(map(tuple, res["narrow"][:res["nnar"]].tolist())) == set(narrow), "the narrow list, as a set"
        assert set(map(tuple, res["wide"][:res["nwide"]].tolist())) == set(wide), "the wide list, as a set"
        assert (res["narrow"][res["nnar"]:] == SENT).all() and (res["wide"][res["nwide"]:] == SENT).all()
        check(case, res, exp, absent_set=True)
        if diff_runs:
            check_pins(case, res, wide)
        for i, v in enumerate(ref):
            want_pin = NEVER if v["how"] == "pin" else case["msgs"][i]["pin"]
            assert int(res["pin"][i]) == want_pin, (i, v["how"])
        assert res["ctr"] == ctr, (res["ctr"], ctr)
        assert np.array_equal(res["cstat"][:, 0], cstat0 if masks else 0 * cstat0)
        assert np.array_equal(res["cstat"][:, 1], differed)
        for c, s in enumerate(senders):
            assert int(res["cstat"][c, 2]) in (s if masks and s else {0}), (c, "a sender of the streamed chunk")
        listed = len(narrow) + len(wide) if elidable else 0
        assert res["halt"] == [0, case["k"] + 1 if listed and not diff_runs else 0, listed], res["halt"]
        assert res["streamed"] == (1 if masks and narrow else 0)
    return ref, res


def log_case(N, k, specs, seed, flags=R.SD_K8 | R.SD_LISTER):
    """SYNC_ACKs between disjoint row pairs (2 j + 1 answers 2 j). spec: tln, n0, n1 (log lengths as stored: TL + 1 is
    an overflowed log), and optionally kind, pin, defer, stale (which of the requester's two logs carries another tick),
    where ("one": every log subject in one segment, "ends": in the first and the last). Rows differ only in subjects of
    the logs that count, so a resolvable message's log-derived diff must equal the diff of the full rows."""
    z = R.sd_sizes(N)
    rng = np.random.default_rng(seed)
    rows = np.tile(rows_for(N)[0], (2 * len(specs), 1))
    p0, p1 = k & 1, (k - 1) & 1
    tl_tick = np.zeros((2, len(rows)), np.uint32)
    tl_n = np.zeros((2, len(rows)), np.uint32)
    tlog = np.zeros((2, len(rows), TL), np.uint32)
    tl_tick[p0], tl_tick[p1] = k - 2 if k >= 2 else 77, k - 1
    msgs = []
    arena = np.zeros((len(specs), z["NS"]), np.uint32)
    for j, sp in enumerate(specs):
        req, rsp = 2 * j, 2 * j + 1
        if sp.get("where") == "one":
            dom = np.arange(MCH, min(2 * MCH, N)) if N > MCH + 64 else np.arange(N)
        else:
            dom = np.concatenate([np.arange(0, 40), np.arange(N - 40, N)])
        pick = lambda n: rng.choice(dom, min(n, TL), replace=False).astype(np.uint32)
        a, b0, b1 = pick(sp["tln"]), pick(sp["n0"]), pick(sp["n1"])
        if len(a) and len(b0):
            b0[0] = a[-1]  # duplicates across the logs
        if len(b0) > 1 and len(b1) > 1:
            b1[1] = b0[1]
            b1[0] = b1[1] if len(a) == 0 else b1[0]  # and inside one
        tlog[p1, rsp, :len(a)], tlog[p0, req, :len(b0)], tlog[p1, req, :len(b1)] = a, b0, b1
        tl_n[p0, req], tl_n[p1, req] = sp["n0"], sp["n1"]
        if sp.get("stale") is not None:
            tl_tick[p0 if sp["stale"] == 0 else p1, req] = k - 4 if k >= 4 else 99
        m = R.sd_msg(rsp, req, kind=sp.get("kind", 2 | R.KF_RES) | (R.KF_DEFER if sp.get("defer") else 0),
                     pin=j if sp.get("pin") else NEVER, tln=sp["tln"])
        msgs.append(m)
        case = dict(N=N, k=k, tl_tick=tl_tick, tl_n=tl_n, tlog=tlog)
        subs = R.sd_log_subjects(case, m)
        if subs is None:  # streamed: the rows may differ anywhere
            subs = rng.choice(N, 30, replace=False).tolist()
        for s in subs:
            how = rng.integers(0, 5)
            if how == 0:
                rows[rsp, s] += 4            # the responder's record is newer: a candidate
            elif how == 1:
                rows[req, s] += 8            # the requester's is: a candidate too (the diff only compares)
            elif how == 2:
                rows[rsp, s] = 0             # absent in the payload: no candidate
            elif how == 3:
                rows[rsp, s] = key(rng.integers(64, 2**30), 1)  # an escaped key
    case = dict(N=N, rows=rows, arena=arena, msgs=msgs, flags=flags, POOLCAP=4096, k=k, tl_tick=tl_tick, tl_n=tl_n, tlog=tlog)
    return inbound(case)


LOG_LENGTHS = [(a, b, c) for a in (0, 1, TL) for b in (0, 1, TL) for c in (0, 1, TL)]


@pytest.mark.parametrize("N", [2049, 8200])
def test_lister_resolves_from_the_logs(engine, N):
    """tln, n0, n1 in {0, 1, TL} (all at TL: 48 lanes), duplicates across the logs, candidates in one segment or in the
    first and the last; for every resolved message the log-derived candidates equal the diff of the full rows."""
    nres = 0
    for q in range(0, len(LOG_LENGTHS), 4):
        specs = [dict(tln=a, n0=b, n1=c, where=("one", "ends")[(q + j) % 2]) for j, (a, b, c) in enumerate(LOG_LENGTHS[q:q + 4])]
        case = log_case(N, 6 + q % 3, specs, 300 + q + N)
        ref, res = check_lister(engine, case, grids=(0, 1))
        assert all(v["how"] == "resolved" for v in ref)
        for i, (m, v) in enumerate(zip(case["msgs"], ref)):  # the cross-check against the streamed diff's reference
            segs, _ = R.sync_diff_ref(R.sd_payload(case, m), case["rows"][m["dst"]])
            assert sum(len(w) for w in segs) == len(v["cand"]) == int(res["ncand"][i])
            for g, w in enumerate(segs):
                if len(v["cand"]):
                    off, cnt = res["meta"][i, g]
                    assert np.array_equal(res["pool"][off:off + cnt], w), (i, g)
            nres += len(v["cand"]) > 0
    assert nres >= 10


def test_lister_pool_overflow_is_a_capacity_error(engine):
    """The lister reserves a resolved message's candidates with one add: without room it writes nothing of the message
    (no candidate, no chunk_meta, ncand = 0) and raises E_POOL; the other messages are complete."""
    specs = [dict(tln=TL, n0=TL, n1=TL, where=("one", "ends")[j % 2]) for j in range(4)]
    case = log_case(8200, 8, specs, 77)
    ref = R.ack_resolve_ref(case)
    exp = lister_expect(case, ref, True)[0]
    counts = [len(v["cand"]) for v in ref]
    assert all(v["how"] == "resolved" for v in ref) and min(counts) >= 4
    for cap in (sum(counts) - 1, max(counts), min(counts) - 1, 0):
        c = dict(case, POOLCAP=cap)
        res = run(engine, c)
        assert res["err"] == R.E_POOL and res["pool_used"] == sum(counts)
        check(c, res, exp, absent_set=True, overflow=True, whole=range(4))
        fit = [i for i in range(4) if int(res["ncand"][i])]
        assert sum(counts[i] for i in fit) <= cap and (cap < min(counts) or fit), "what fits is written"
        assert res["ctr"]["ackres_all"] == 4
    c = dict(case, POOLCAP=sum(counts))
    check(c, run(engine, c), exp, absent_set=True)


def test_lister_leaves_unresolvable_acks_to_the_diff(engine):
    """tln = TL + 1, a requester log past TL, a stale tl_tick (that log counts as empty), KF_RES missing, a delayed and a
    pinned message, and k = 1: streamed (or resolved from fewer logs), and the diff that follows gives the reference."""
    N = 8200
    specs = [dict(tln=TL + 1, n0=1, n1=1), dict(tln=3, n0=TL + 1, n1=0), dict(tln=3, n0=2, n1=TL + 1),
             dict(tln=4, n0=5, n1=6, stale=0), dict(tln=4, n0=5, n1=6, stale=1), dict(tln=2, n0=2, n1=2, kind=2),
             dict(tln=2, n0=2, n1=2, defer=True), dict(tln=2, n0=2, n1=2, pin=True)]
    for half, want in ((specs[:4], ["narrow", "narrow", "narrow", "resolved"]), (specs[4:], ["resolved", "narrow", "wide", "wide"])):
        case = log_case(N, 9, half, 17 + len(want[0]))
        ref, _ = check_lister(engine, case, grids=(0, 2))
        assert [v["how"] for v in ref] == want
        # without the 8-bit plane the unresolved ones all go to the wide list
        c2 = inbound(dict(case, flags=R.SD_LISTER))
        ref, _ = check_lister(engine, c2, grids=(3,))
        assert [v["how"] for v in ref] == [w if w == "resolved" else "wide" for w in want]
    case = log_case(N, 1, [dict(tln=1, n0=0, n1=1), dict(tln=0, n0=0, n1=0)], 5)
    ref, _ = check_lister(engine, case)
    assert [v["how"] for v in ref] == ["narrow", "narrow"], "k < 2: no log of tick k - 2"


def mask_case(N, seed, ls=0, flags=R.SD_K8 | R.SD_LISTER | R.SD_DIRTY):
    """Rows that differ from the baseline only in the chunks their mask marks; SYNCs between them: needed because of the
    sender only, the receiver only, both, and with no dirty chunk (decided in the lister); dirty bits in every mask
    word the size has."""
    z = R.sd_sizes(N)
    rng = np.random.default_rng(seed)
    all8 = rows_for(N)
    rows = np.tile(all8[0], (8, 1))
    dirty = np.zeros((8, 3), np.uint64)
    words = list(range(z["MW"]))
    marks = {1: [0], 2: [z["NCHUNK"] - 1], 3: [min(5, z["NCHUNK"] - 1), z["NCHUNK"] - 1], 4: [64 * w + 1 for w in words if 64 * w + 1 < z["NCHUNK"]],
             5: [c for c in (63, 64, 127, 128) if c < z["NCHUNK"]] or [1]}
    for r, chunks in marks.items():
        for c in chunks:
            dirty[r, c >> 6] |= np.uint64(1 << (c & 63))
            a, b = c * CH, min((c + 1) * CH, N)
            ch = a + np.flatnonzero(rng.random(b - a) < 0.05)
            rows[r, ch] = all8[[4, 5, 6, 7, 1][r - 1], ch]
            rows[r, [a, b - 1]] = all8[2 + r % 2 * 3, [a, b - 1]]  # (row 2: absent; row 5: escapes)
    pairs = [(1, 0), (0, 1), (0, 6), (6, 7), (2, 0), (0, 2), (3, 4), (4, 3), (5, 0), (0, 5), (5, 5), (7, 6), (2, 3)]
    msgs = [R.sd_msg(s, d) for s, d in pairs]
    case = dict(N=N, rows=rows, msgs=msgs, dirty=dirty, flags=flags, POOLCAP=4 * N, k=3, ls=ls)
    case.update(tl_tick=np.zeros((2, 8), np.uint32), tl_n=np.zeros((2, 8), np.uint32), tlog=np.zeros((2, 8, TL), np.uint32))
    return inbound(case)


@pytest.mark.parametrize("N", [2049, 8200, 131080, 262152])
def test_lister_consults_the_dirty_masks(engine, N):
    case = mask_case(N, 40 + N)
    ref, res = check_lister(engine, case, grids=(0, 1, 7))
    hows = [v["how"] for v in ref]
    assert hows.count("decided") >= 3 and hows.count("narrow") >= 8
    for i, v in enumerate(ref):
        if v["how"] == "decided":
            assert int(res["ncand"][i]) == 0 and (res["meta"][i] == SENT).all(), "no entry, its chunk_meta not written"
    # the lists alone (no diff queued: LS_NODIFF raises the diff-halt), and the masks kept but not consulted
    check_lister(engine, mask_case(N, 40 + N, ls=R.LS_SPEC | R.LS_NODIFF))
    ref2, _ = check_lister(engine, mask_case(N, 40 + N, flags=R.SD_K8 | R.SD_LISTER), grids=(3,))
    assert all(v["how"] == "narrow" and len(v["items"]) == R.sd_sizes(N)["nit"] for v in ref2)


PIN_VARIANTS = ["clean", "snapshot-sibling", "deferred-sibling", "dirty-sender", "dirty-receiver", "not-on-the-list"]


def pin_case(N, L, variant):
    """Receiver 0 with L pinned live-row payloads from clean senders; the variants break one condition each."""
    z = R.sd_sizes(N)
    rows = np.tile(rows_for(N)[0], (8, 1))
    dirty = np.zeros((8, 3), np.uint64)
    arena = np.zeros((L + 1, z["NS"]), np.uint32)
    arena[L] = rows_for(N)[1]
    msgs = [R.sd_msg(1 + j % 7, 0, pin=j) for j in range(L)]
    if variant == "snapshot-sibling":
        msgs[L // 2] = R.sd_msg(3, 0, payload=L)
    elif variant == "deferred-sibling":
        msgs[L - 1]["kind"] |= R.KF_DEFER
    elif variant in ("dirty-sender", "dirty-receiver"):
        r, c = (msgs[L - 1]["src"] if variant == "dirty-sender" else 0), z["NCHUNK"] - 1  # a bit in word MW - 1 only
        dirty[r, c >> 6] = np.uint64(1 << (c & 63))
        rows[r, N - 1] += 4
    case = dict(N=N, rows=rows, arena=arena, msgs=msgs, dirty=dirty, flags=R.SD_K8 | R.SD_LISTER | R.SD_DIRTY, POOLCAP=4096, k=3)
    case.update(tl_tick=np.zeros((2, 8), np.uint32), tl_n=np.zeros((2, 8), np.uint32), tlog=np.zeros((2, 8, TL), np.uint32))
    inbound(case)
    if variant == "not-on-the-list":  # the last message is linked nowhere (found = false for it)
        if L == 1:
            case["m_head"][0] = NEVER
        else:
            case["m_next"][L - 2] = NEVER
    return case


@pytest.mark.parametrize("N", [8200, 131080, 262152])
@pytest.mark.parametrize("variant", PIN_VARIANTS)
def test_lister_decides_pinned_payloads_of_clean_rows(engine, N, variant):
    for L in (1, 2, 8, 9):
        case = pin_case(N, L, variant)
        ref, res = check_lister(engine, case)
        hows = [v["how"] for v in ref]
        if variant == "clean" and L <= 8:
            assert hows == ["pin"] * L and (res["pin"] == NEVER).all() and res["nwide"] == 0
        elif variant == "not-on-the-list":  # (the list then has L - 1 <= 8 entries)
            assert hows == ["pin"] * (L - 1) + ["wide"]
        elif variant == "deferred-sibling":
            assert "pin" not in hows and hows[-1] == "wide" and res["wide"][:L, 3].tolist().count(R.DESC_DEFER) == 1
        else:
            assert "pin" not in hows, (variant, L, hows)


# ------------------------------------------------------------------------------------------------------ validation
def test_invalid_sync_diff_arguments_are_refused_before_any_launch(engine):
    E = _abi.SWIM_EINVAL

    def rc(case, params_patch=None, in_patch=None, extra_in=0):
        params, inp, out = R.sd_pack(case)
        for i, v in (params_patch or {}).items():
            params[i] = v
        if in_patch:
            inp = inp.copy()
            inp[in_patch[0]] = in_patch[1]
        if extra_in:
            inp = np.concatenate([inp, np.zeros(extra_in, np.uint32)])
        return _abi.prim_eval_rc(engine, _abi.PRIM_SYNC_DIFF, params, inp, out)

    N = 2049  # NS = 2056: seven padding keys
    z = R.sd_sizes(N)
    rows = np.tile(rows_for(N)[0], (2, 1))
    arena = np.zeros((1, z["NS"]), np.uint32)
    base = dict(N=N, rows=rows, arena=arena, msgs=[R.sd_msg(0, 1), R.sd_msg(1, 0, payload=0, pin=0)], flags=R.SD_K8 | R.SD_LISTS,
                narrow=[(0, 0, 1, 0 << 4 | 3)], wide=[(1, 1, 0, 0)], POOLCAP=64, k=1)
    assert rc(base) == 0
    msg = lambda **kw: dict(base, msgs=[R.sd_msg(0, 1), dict(R.sd_msg(1, 0, payload=0, pin=0), **kw)])
    assert rc(msg(src=2)) == E and rc(msg(dst=2)) == E and rc(msg(payload=1)) == E and rc(msg(pin=1)) == E
    assert rc(msg(payload=R.PAY_RX)) == E, "a received payload on one GPU"
    nar = lambda *e: dict(base, narrow=[e])
    assert rc(nar(2, 0, 1, 3)) == E and rc(nar(0, 2, 1, 3)) == E and rc(nar(0, 0, 2, 3)) == E
    assert rc(nar(0, 0, 1, 1 << 4 | 1)) == E, "an item past the last"
    assert rc(nar(0, 0, 1, 4)) == E, "a chunk bit past NCHUNK = 2"
    assert rc(dict(base, flags=R.SD_LISTS)) == E, "a narrow entry without the 8-bit plane"
    wid = lambda w: dict(base, wide=[(1, 1, 0, w)])
    assert rc(wid(R.DESC_PIN | 0)) == 0 and rc(wid(R.DESC_DEFER)) == 0 and rc(wid(NEVER)) == 0
    assert rc(wid(1)) == E and rc(wid(R.DESC_PIN | 1)) == E and rc(wid(R.PAY_RX | 0)) == E
    pad = dict(base, rows=rows.copy())
    pad["rows"][1, N] = 5
    assert rc(pad) == E, "a padding key between N and NS"
    pad = dict(base, arena=arena.copy())
    pad["arena"][0, z["NS"] - 1] = 5
    assert rc(pad) == E
    # sizes, the tick, flags that do not go together, a list longer than its capacity, trailing input
    for i, v in [(0, 0), (0, 3 * 64 * CH + 1), (1, 0), (1, 65), (2, 32), (3, 3), (4, 4097), (5, 65), (6, 2**22 + 1), (7, 0),
                 (8, 4097), (12, 1), (13, 1), (14, 1)]:
        assert rc(base, {i: v}) == E, (i, v)
    assert rc(base, {2: R.SD_K8 | R.SD_LISTS | R.SD_LISTER}) == E and rc(base, {2: R.SD_K8 | R.SD_LISTS | R.SD_DIRTY}) == E
    assert rc(base, {10: 0}) == E and rc(base, extra_in=2) == E and rc(base, extra_in=CH) == E
    assert _abi.prim_eval_rc(engine, _abi.PRIM_SYNC_DIFF, R.sd_pack(base)[0], R.sd_pack(base)[1], np.zeros(8, np.uint32)) == E
    # mode B: a log subject >= N, links past nmsg, a list that does not end
    lst = inbound(dict(base, flags=R.SD_K8 | R.SD_LISTER, narrow=[], wide=[], k=2, tl_tick=np.zeros((2, 2), np.uint32),
                       tl_n=np.zeros((2, 2), np.uint32), tlog=np.zeros((2, 2, TL), np.uint32)))
    assert rc(lst) == 0
    bad = dict(lst, tlog=lst["tlog"].copy())
    bad["tlog"][1, 1, 15] = N
    assert rc(bad) == E
    assert rc(dict(lst, m_head=R.u32([2, NEVER]))) == E and rc(dict(lst, m_next=R.u32([NEVER, 2]))) == E
    assert rc(dict(lst, m_head=R.u32([0, NEVER]), m_next=R.u32([1, 0]))) == E, "a cycle"
    assert rc(lst, {7: 0}) == E and rc(lst, {14: 4}) == E
    # W = 2: ri and rx_off against the receive buffer, the shipped chunks against popcount(mask), mask bits past NCHUNK
    sh = sharded_case(8200, 1)
    assert rc(sh) == 0
    rx = lambda ri, **kw: dict(sh, rx=[dict(r, **kw) if j == ri else r for j, r in enumerate(sh["rx"])])
    assert rc(rx(1, off=sh["rx"][1]["off"] + 2)) == E and rc(rx(2, off=sh["rx"][2]["off"] + 4)) == E
    assert rc(rx(1, off=4 * CH * len(sh["recv"]) + 16)) == E
    assert rc(rx(1, off=sh["rx"][1]["off"] + 4 * CH)) == E, "the last payload's chunks would pass the buffer"
    assert rc(rx(3, mask=1 << R.sd_sizes(8200)["NCHUNK"])) == E, "a mask bit past NCHUNK"
    assert rc(dict(sh, wide=sh["wide"] + [(0, 0, sh["lo"], R.PAY_RX | 4)])) == E, "ri past nrx"
    assert rc(dict(sh, msgs=sh["msgs"][:-1] + [R.sd_msg(0, sh["lo"])])) == E, "a local sender below lo"
    assert rc(sh, {12: 8200 - 3}) == E, "lo + R past N"
