"""Known answers for the row-shard exchange codec of shard.hip, through SWIM_PRIM_XPACK, XUNPACK, PACK_B and
INLINE_IN of swim_debug_prim_eval (include/swimhip_debug.h): k_pack_all, k_unpack_a with msgs_commit, k_pack_b,
k_inline_out and k_inline_in run in the engine's own grids on a Dev that holds only what they read, every output buffer
preset to a sentinel, and what they leave is compared with the plain references of tests/prim_ref.py (validated without a
GPU in tests/test_prim_ref.py). Integer code: every comparison is equality; where atomics assign the indices it is
equality of multisets, with the reason written next to it. Engine only.

Whole-cluster parity runs reach this code with one mask word, one chunk per row and a handful of messages per tick. Here
the shapes sit where a hand-laid byte format goes wrong: a second and third batch of the block scans, a second mask word,
eight ranks, a region at and one step past the inline block, a partial last chunk, and every capacity overflow.
"""
import functools

import numpy as np
import pytest

import prim_ref as R
from swimhip import _abi

pytestmark = pytest.mark.gpu

NEVER, CH, TL, SMW = R.NEVER, R.CH, R.TL, R.SMW
CASES = R.xpack_cases()
SENT = R.XP_BYTE


@functools.lru_cache(maxsize=None)
def packed(engine, name):
    """(case, reference, what k_pack_all and k_inline_out left): one launch per case, shared by the tests."""
    c = CASES[name]
    params, inp, out = R.xp_pack(c)
    _abi.prim_eval(engine, _abi.PRIM_XPACK, params, inp, out)
    return c, R.xpack_ref(c), R.xp_unpack(c, out)


def words(b):
    return np.frombuffer(np.ascontiguousarray(b).tobytes(), np.uint32)


def first_diff(got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return None if len(bad) == 0 else (int(bad[0]), int(np.asarray(got).reshape(-1)[bad[0]]), int(np.asarray(want).reshape(-1)[bad[0]]))


def peers(c):
    return [q for q in range(c["W"]) if q != c["rank"]]


# ---------------------------------------------------------------------------------------------------------- k_pack_all
@pytest.mark.parametrize("name", list(CASES))
def test_pack_header_and_records(engine, name):
    c, ref, got = packed(engine, name)
    for q in peers(c):
        reg = ref["regions"][q]
        if reg is None:  # a halted speculative launch
            continue
        H, Hw = words(got["xa_send"][q][:32]), words(ref["xa_send"][q][:32])
        for k, f in enumerate(("nslot", "nround", "nsync", "nchunk", "data_off", "H[5]", "H[6]", "H[7]")):
            assert H[k] == Hw[k], (name, "peer", q, "header field", f, int(H[k]), int(Hw[k]))
        o = 32 + 4 * R.NSW * reg["nslot"]
        assert first_diff(got["xa_send"][q][32:o], ref["xa_send"][q][32:o]) is None, (name, "peer", q, "slot records")
        assert first_diff(got["xa_send"][q][o:reg["off_sync"]], ref["xa_send"][q][o:reg["off_sync"]]) is None, \
            (name, "peer", q, "round records")
        assert int(got["xa_scnt"][q]) == int(ref["xa_scnt"][q]), \
            (name, "peer", q, "xa_scnt: bytes | XFLAG_GOSSIP", hex(int(got["xa_scnt"][q])), hex(int(ref["xa_scnt"][q])))


@pytest.mark.parametrize("name", list(CASES))
def test_pack_sync_entries(engine, name):
    """Entries go in message order (every block of a column walks the same list), so the bytes are determined."""
    c, ref, got = packed(engine, name)
    MW, SE = R.sd_sizes(c["N"])["MW"], R.sync_entry_size(R.sd_sizes(c["N"])["MW"])
    for q in peers(c):
        reg = ref["regions"][q]
        if reg is None or not reg["fits"]:
            continue
        for j, (i, base, mask, nlog) in enumerate(reg["entries"]):
            o = reg["off_sync"] + SE * j
            g, w = words(got["xa_send"][q][o:o + SE]), words(ref["xa_send"][q][o:o + SE])
            at = (name, "peer", q, "entry", j, "message", i)
            assert first_diff(g[:SMW], w[:SMW]) is None, at + ("SyncMsg bytes", first_diff(g[:SMW], w[:SMW]))
            assert g[SMW] == base, at + ("chunk base", int(g[SMW]), base)
            assert g[SMW + 1] == 0, at + ("pad", int(g[SMW + 1]))
            for k in range(MW):
                gm = int(g[SMW + 2 + 2 * k]) | int(g[SMW + 3 + 2 * k]) << 32
                assert gm == (mask >> (64 * k)) & R.M64, at + ("mask word", k, hex(gm), hex((mask >> (64 * k)) & R.M64))
            lg, lw = g[SMW + 2 + 2 * MW:], w[SMW + 2 + 2 * MW:]
            assert first_diff(lg[:nlog], lw[:nlog]) is None, at + ("log prefix", nlog)
            assert (lg[nlog:] == R.XP_WORD).all(), at + ("log words past the prefix keep the sentinel", nlog)
        o = reg["off_sync"] + SE * reg["nsync"]
        assert (got["xa_send"][q][o:reg["data_off"]] == SENT).all(), (name, "peer", q, "gap between the entries and data_off")


@pytest.mark.parametrize("name", list(CASES))
def test_pack_chunks(engine, name):
    """Chunk base + i of an entry is the payload row's i-th dirty chunk; a partial last chunk leaves the words of the
    subjects >= NS alone."""
    c, ref, got = packed(engine, name)
    NS = R.sd_sizes(c["N"])["NS"]
    for q in peers(c):
        reg = ref["regions"][q]
        if reg is None or not reg["fits"]:
            continue
        for j, (i, base, mask, _) in enumerate(reg["entries"]):
            keys = R.xp_payload(c, c["msgs"][i])[0]
            for n, ch in enumerate(R.mask_chunks(mask)):
                o = reg["data_off"] + (base + n) * CH * 4
                g = words(got["xa_send"][q][o:o + CH * 4])
                live = min(CH, NS - ch * CH)
                at = (name, "peer", q, "entry", j, "message", i, "shipped chunk", base + n, "row chunk", ch)
                assert first_diff(g[:live], keys[ch * CH:ch * CH + live]) is None, at + ("keys", first_diff(g[:live], keys[ch * CH:ch * CH + live]))
                assert (g[live:] == R.XP_WORD).all(), at + ("words of the subjects >= NS keep the sentinel", live)


@pytest.mark.parametrize("name", list(CASES))
def test_pack_writes_nothing_out_of_place(engine, name):
    c, ref, got = packed(engine, name)
    for q in range(c["W"]):
        reg = ref["regions"][q]
        if q == c["rank"] or reg is None:
            assert (got["xa_send"][q] == SENT).all(), (name, "region", q, "the own column / a halted launch writes no byte")
            assert int(got["xa_scnt"][q]) == R.XP_WORD64, (name, "xa_scnt", q)
            continue
        assert (got["xa_send"][q][reg["bytes"]:] == SENT).all(), (name, "peer", q, "bytes at and past the region's byte count")
        d = first_diff(got["xa_send"][q], ref["xa_send"][q])
        assert d is None, (name, "peer", q, "region byte", d)
    assert first_diff(got["xn"][[0, 1, 2, 3, 5, 6, 7]], ref["xn"][[0, 1, 2, 3, 5, 6, 7]]) is None, (name, "xn words it does not own")


@pytest.mark.parametrize("name", list(CASES))
def test_pack_local_column(engine, name):
    """mtmp[xn4 .. xn[4]) holds the messages to the rank's own members in message order (one block, a block scan per
    batch: determined), mlog alongside; everything else keeps the sentinel."""
    c, ref, got = packed(engine, name)
    assert int(got["xn"][4]) == int(ref["xn"][4]), (name, "xn[4]", int(got["xn"][4]), int(ref["xn"][4]))
    for j in range(c["MSGCAP"]):
        assert first_diff(got["mtmp"][j], ref["mtmp"][j]) is None, (name, "mtmp", j, first_diff(got["mtmp"][j], ref["mtmp"][j]))
        assert first_diff(got["mlog"][j], ref["mlog"][j]) is None, (name, "mlog", j, first_diff(got["mlog"][j], ref["mlog"][j]))
    assert got["err"] & R.E_MSGS == ref["err"] & R.E_MSGS, (name, "E_MSGS", hex(got["err"]))


@pytest.mark.parametrize("name", list(CASES))
def test_pack_inline_blocks(engine, name):
    """The count word, then the region's first min(bytes, XI - 8) bytes; XFLAG_OVER on every peer's word iff some region
    of this rank is past XI - 8; the own block is the single zero count word; with inline off nothing is written."""
    c, ref, got = packed(engine, name)
    XI = c["XI"]
    over = any(reg and reg["bytes"] > XI - 8 for reg in ref["regions"])
    for q in range(c["W"]):
        g, w = got["xi_send"][q], ref["xi_send"][q]
        if not c["flags"] & R.XP_INLINE or c["flags"] & R.XP_HALTED:
            assert (g == SENT).all(), (name, "inline block", q, "untouched")
            continue
        gw, ww = int(g[:8].view(np.uint64)[0]), int(w[:8].view(np.uint64)[0])
        if q == c["rank"]:
            assert gw == 0 and (g[8:] == SENT).all(), (name, "own inline block: a zero count word and nothing else", hex(gw))
            continue
        assert bool(gw & R.XFLAG_OVER) == over, (name, "peer", q, "XFLAG_OVER", hex(gw), over)
        assert gw == ww, (name, "peer", q, "count word", hex(gw), hex(ww))
        n = min(ref["regions"][q]["bytes"], XI - 8)
        d = first_diff(g[8:8 + n], got["xa_send"][q][:n])
        assert d is None, (name, "peer", q, "inline bytes", d)
        assert (g[8 + n:] == SENT).all(), (name, "peer", q, "nothing past the region's head", n)
        assert first_diff(g, w) is None, (name, "peer", q, "inline block", first_diff(g, w))


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("ovf-")])
def test_pack_overflow(engine, name):
    c, ref, got = packed(engine, name)
    assert got["err"] == ref["err"] != 0, (name, "err", hex(got["err"]), hex(ref["err"]))
    for q in peers(c):
        reg = ref["regions"][q]
        if reg["fits"]:
            continue
        H = words(got["xa_send"][q][:32])
        assert H[:5].tolist() == [0, 0, 0, 0, 256], (name, "peer", q, "header counts of a region that does not fit", H[:5].tolist())
        assert int(got["xa_scnt"][q]) & R.XCNT_MASK == 32, (name, "peer", q, "byte count 32")
        assert (got["xa_send"][q][32:] == SENT).all(), (name, "peer", q, "no entry or chunk byte is written")


@pytest.mark.parametrize("name", list(CASES))
def test_pack_err(engine, name):
    c, ref, got = packed(engine, name)
    assert got["err"] == ref["err"], (name, "err", hex(got["err"]), hex(ref["err"]))
    assert got["halt"] == (1 if c["flags"] & R.XP_HALTED else 0), (name, "halt word")


def test_pack_halted_spec_launch_writes_nothing(engine):
    c, ref, got = packed(engine, "spec-halted")
    for f in ("xa_send", "xi_send", "mtmp", "mlog"):
        assert (got[f].view(np.uint8) == SENT).all(), f
    assert (got["xa_scnt"] == R.XP_WORD64).all() and got["err"] == 0
    assert got["xn"].tolist() == ref["xn"].tolist() == [3, 3, R.XP_WORD, R.XP_WORD, 0, R.XP_WORD, R.XP_WORD, R.XP_WORD]


@pytest.mark.parametrize("name", list(CASES))
def test_inline_out_matches_pack_tail(engine, name):
    """k_inline_out on the regions and count words k_pack_all left writes the blocks its inline tail wrote; only the tail
    adds the OVER mark."""
    c, ref, got = packed(engine, name)
    assert first_diff(got["xi_out"], ref["xi_out"]) is None, (name, "k_inline_out block byte", first_diff(got["xi_out"], ref["xi_out"]))
    if c["flags"] & R.XP_INLINE and not c["flags"] & R.XP_HALTED:
        for q in peers(c):
            a, b = got["xi_out"][q].copy(), got["xi_send"][q].copy()
            b[:8] = np.array([int(b[:8].view(np.uint64)[0]) & ~R.XFLAG_OVER], np.uint64).view(np.uint8)
            assert first_diff(a, b) is None, (name, "peer", q, "the two inline writers differ at byte", first_diff(a, b))


def test_pack_refuses_what_the_layout_does_not_allow(engine):
    """SWIM_EINVAL before any launch; the output keeps the sentinel."""
    base = CASES["n2049-w3-r1"]

    def rc(**kw):
        c = dict(base, **kw)
        params, inp, out = R.xp_pack(c)
        code = _abi.prim_eval_rc(engine, _abi.PRIM_XPACK, params, inp, out)
        assert code == 0 or (out == SENT).all()
        return code

    def with_msg(i, **kw):
        msgs = [dict(m) for m in base["msgs"]]
        msgs[i].update(kw)
        return msgs

    EINVAL = _abi.SWIM_EINVAL
    assert rc() == 0
    assert rc(msgs=with_msg(0, src=682)) == EINVAL and rc(msgs=with_msg(0, src=689)) == EINVAL, "src outside the rows"
    assert rc(msgs=with_msg(0, dst=2049)) == EINVAL, "dst >= N"
    assert rc(msgs=with_msg(0, payload=2)) == EINVAL, "a payload that is no arena row"
    assert rc(rdirty=[4] + base["rdirty"][1:]) == EINVAL and rc(arena_dirty=[1 << 63, 0]) == EINVAL, "mask bits past NCHUNK"
    assert rc(xn0=4) == EINVAL and rc(xn1=4) == EINVAL, "records the caller did not supply"
    assert rc(XA_PEER=base["XA_PEER"] + 8) == EINVAL and rc(XI=16380) == EINVAL and rc(XI=56) == EINVAL
    assert rc(flags=R.XP_ACKRES, tlog=None, msgs=with_msg(0, kind=R.KF_RES, tln=1)) == EINVAL, "a log nobody supplied"
    assert rc(flags=R.XP_ACKRES, tlog=None, msgs=with_msg(0, kind=R.KF_RES, tln=17)) == 0
    assert rc(rank=3) == EINVAL and rc(flags=R.XP_HALTED) == EINVAL


# ------------------------------------------------------------------------------------------------------------ k_pack_b
@pytest.mark.parametrize("nd", R.PACKB_NDS)
@pytest.mark.parametrize("W,rank", [(2, 1), (8, 3)])
def test_pack_b(engine, nd, W, rank):
    xd = (np.arange(nd, dtype=np.uint64) << np.uint64(32)) | np.uint64(0x80000000) | np.arange(nd, dtype=np.uint64)[::-1]
    run_pack_b(engine, W, rank, 32768, nd, 16 + 8 * 16385, xd, 0)


def run_pack_b(engine, W, rank, DCAP, xd_n, XB, xd, err):
    out = np.full((W * XB + 8 * W + 8) // 8, R.XP_WORD64, np.uint64).view(np.uint8)
    _abi.prim_eval(engine, _abi.PRIM_PACK_B, [W, rank, DCAP, xd_n, XB], np.ascontiguousarray(xd[:min(xd_n, DCAP)]), out)
    send, scnt, e = R.pack_b_ref(W, rank, DCAP, xd_n, XB, xd)
    assert e == err
    gs, gc = out[:W * XB].reshape(W, XB), out[W * XB:W * XB + 8 * W].view(np.uint64)
    for q in range(W):
        assert int(gc[q]) == int(scnt[q]), ("xb_scnt", q, hex(int(gc[q])), hex(int(scnt[q])))
        assert words(gs[q][:16]).tolist() == words(send[q][:16]).tolist(), ("header", q, words(gs[q][:16]).tolist())
        assert first_diff(gs[q], send[q]) is None, ("region byte", q, first_diff(gs[q], send[q]))
    assert int(out[W * XB + 8 * W:].view(np.uint32)[0]) == err, "err"


def test_pack_b_clamps_and_overflows(engine):
    xd = np.arange(1, 41, dtype=np.uint64) * np.uint64(0x100000001)
    run_pack_b(engine, 3, 0, 16, 40, 16 + 8 * 16, xd, 0)                  # nd > DCAP clamps; the region is exactly full
    run_pack_b(engine, 3, 2, 16, 16, 16 + 8 * 15, xd, R.E_XCAP)           # one record short: E_XCAP and a header only
    assert _abi.prim_eval_rc(engine, _abi.PRIM_PACK_B, [3, 3, 16, 0, 64], None, np.zeros(3 * 64 + 32, np.uint8)) != 0


# --------------------------------------------------------------------------------------------------------- k_inline_in
@pytest.mark.parametrize("halt", [0, 1, 3])
def test_inline_in(engine, halt):
    """min(bytes, XI - 8) bytes per peer behind the count word and nothing past them; rcnt[p], host[p] = scnt[p] and
    host[W + p]; with a raised halt nothing. Byte counts around the block: 0, 8, XI - 16, XI - 8, XI, far past, flagged."""
    W, XI, cap = 8, 256, 512
    rng = np.random.default_rng(71)
    irecv = rng.integers(0, 256, (W, XI), dtype=np.uint8)
    counts = [0, 8, XI - 16, XI - 8, XI, 1 << 20, (XI - 8) | R.XFLAG_GOSSIP, 40 | R.XFLAG_OVER | R.XFLAG_GOSSIP]
    for p, n in enumerate(counts):
        irecv[p][:8] = np.array([n], np.uint64).view(np.uint8)
    scnt = rng.integers(0, 2**63, W, dtype=np.uint64)
    inp = np.concatenate([irecv.reshape(-1), scnt.view(np.uint8)])
    out = np.full((W * cap + 24 * W) // 8, R.XP_WORD64, np.uint64).view(np.uint8)
    _abi.prim_eval(engine, _abi.PRIM_INLINE_IN, [W, XI, cap, halt], np.frombuffer(inp.tobytes(), np.uint64).copy().view(np.uint8), out)
    recv, rcnt, host = R.inline_in_ref(W, XI, cap, irecv, scnt, halt == 3)
    g = out[:W * cap].reshape(W, cap)
    for p in range(W):
        assert first_diff(g[p], recv[p]) is None, ("receive region", p, "byte", first_diff(g[p], recv[p]))
    assert out[W * cap:W * cap + 8 * W].view(np.uint64).tolist() == rcnt.tolist(), "rcnt"
    assert out[W * cap + 8 * W:].view(np.uint64).tolist() == host.tolist(), "host words"


# ---------------------------------------------------------------------------------------------------------- k_unpack_a
UCASES = R.xunpack_cases()
ORDER_FREE = ("msgs", "m_head", "m_next", "rx_mask", "rx_off", "mlog", "rg")  # compared by xu_props / as sets
HOLES = {"ovf-rxcap": 100}


@functools.lru_cache(maxsize=None)
def unpacked(engine, name):
    c = UCASES[name]
    params, inp, out = R.xu_pack(c)
    _abi.prim_eval(engine, _abi.PRIM_XUNPACK, params, inp, out)
    return c, R.xunpack_ref(c), R.xu_unpack(c, out)


def gated(c):
    return bool(c["flags"] & R.XU_SPEC and (c["flags"] & R.XU_HALTED or R.xu_gate(c)))


@pytest.mark.parametrize("name", [n for n in UCASES if not gated(UCASES[n])])
def test_unpack_messages_lists_pins_and_payloads(engine, name):
    """Properties 1-4 and 9 (prim_ref.xu_props). k_unpack_a hands out message and rx indices with atomicAdd from 32 x W
    blocks, so which entry gets which index is not determined; that every entry gets one of each, once, and what is
    stored under them, is."""
    c, ref, got = unpacked(engine, name)
    R.xu_props(c, got, holes=HOLES.get(name, 0))
    nloc = len(c["local"])
    assert (got["mlog"][:nloc] == R.XP_WORD).all(), "the local messages' log rows are k_pack_all's, not touched here"
    n = got["sc"][f"nmsg{c['k'] & 1}"]
    assert (got["msgs"][n:] == R.XP_WORD).all() and (got["m_next"][n:] == R.XP_WORD).all(), "nothing past nmsg is written"


@pytest.mark.parametrize("name", list(UCASES))
def test_unpack_counters_and_resets(engine, name):
    """Every scalar the launch owns, and tick_end's resets with end = 1 (none of them with end = 0); a gated or halted
    speculative launch changes nothing but the gate's halt word."""
    c, ref, got = unpacked(engine, name)
    for f in R.XU_SC:
        if name in ("ovf-msgcap", "ovf-rxcap") and f == f"arena{c['k'] & 1}":
            continue  # which entries an overflow drops is not determined, so neither is how many pins the rest need (xu_props)
        assert got["sc"][f] == ref["sc"][f], (name, f, hex(got["sc"][f]), hex(ref["sc"][f]))
    for f in ("xa_scnt", "xb_scnt", "xdone", "xa_rcnt", "host"):
        assert got[f].tolist() == ref[f].tolist(), (name, f, got[f].tolist(), ref[f].tolist())
    if gated(c):
        for f in ORDER_FREE:
            if f in got:
                assert np.array_equal(got[f], ref[f]), (name, f, "a launch that stops at the gate writes nothing")


@pytest.mark.parametrize("name", [n for n in UCASES if UCASES[n]["gossip"] is not None])
def test_unpack_gossip_records(engine, name):
    """Every slot record yields slot_create's writes and every round record the round replay's; members and slots named
    in no record keep the sentinel. Ring positions are reserved with atomicAdd: the creations of one origin fill
    [old tail, new tail) in any order, so those entries are compared as a set."""
    c, ref, got = unpacked(engine, name)
    g = c["gossip"]
    for f in ("slot_gid", "slot_key", "slot4", "gudm", "S", "HB", "mem8", "T", "log3", "log_tg"):
        bad = np.argwhere(got[f] != ref[f])
        assert len(bad) == 0, (name, f, "first difference at", bad[0].tolist(), int(got[f][tuple(bad[0])]), int(ref[f][tuple(bad[0])]))
    for m in range(c["N"]):
        t0, t1 = int(g["rtail"][m]), int(ref["mem8"][0][m])
        pos = [(t0 + i) & (g["BCAP"] - 1) for i in range((t1 - t0) & R.M32)]
        assert sorted(got["rg"][m][pos].tolist()) == sorted(ref["rg"][m][pos].tolist()), (name, "ring entries of", m)
        rest = np.delete(got["rg"][m], pos)
        assert (rest == R.XP_WORD).all(), (name, "ring of", m, "outside [old tail, new tail)")


def test_unpack_refuses_what_the_layout_does_not_allow(engine):
    E = _abi.SWIM_EINVAL
    base = UCASES["n2049>0"]

    def rc(c):
        params, inp, out = R.xu_pack(c)
        code = _abi.prim_eval_rc(engine, _abi.PRIM_XUNPACK, params, inp, out)
        assert code == 0 or (out == SENT).all()
        return code

    def region_with(off, words):
        c = dict(base, recv=base["recv"].copy())
        c["recv"][1][off:off + 4 * len(words)] = np.array(words, np.uint32).view(np.uint8)
        return c

    assert rc(base) == 0
    reg = R.xpack_ref(base["senders"][1])["regions"][0]
    assert rc(region_with(0, [1000])) == E, "records past the region"
    assert rc(region_with(8, [10**6])) == E, "entries past data_off"
    assert rc(region_with(12, [reg["nchunk"] + 1])) == E, "chunks past the byte count"
    assert rc(region_with(16, [reg["data_off"] - 256])) == E and rc(region_with(16, [reg["data_off"] + 8])) == E, "data_off"
    assert rc(region_with(32, [128])) == E, "slot id >= SLOTS"
    assert rc(region_with(32 + 28, [2049])) == E, "origin >= N"
    o = 32 + 4 * R.NSW * 3
    assert rc(region_with(o, [2049])) == E and rc(region_with(o + 4 * R.RRW * 2 + 4, [9])) == E, "round member, cnt > F"
    assert rc(region_with(o + 4 * R.RRW * 2 + 16, [2049])) == E, "target >= N"
    e0 = reg["off_sync"]
    assert rc(region_with(e0 + 4, [2049])) == E, "dst >= N"
    assert rc(region_with(e0 + 4 * SMW, [reg["nchunk"] + 1])) == E, "base + popcount(mask) chunks past nchunk"
    assert rc(region_with(e0 + 4 * SMW + 8, [4])) == E, "mask bits past NCHUNK"
    assert rc(dict(base, gossip=dict(base["gossip"], BCAP=3))) == E and rc(dict(base, gossip=dict(base["gossip"], LOGW=0))) == E
    assert rc(dict(base, local=[R.xp_msg(0, 5, 2049)], MSGCAP=8)) == E, "an initial mtmp entry with dst out of range"
    assert rc(dict(base, rcnt=np.array([0, base["XA_PEER"] + 8, 0], np.uint64))) == E, "a count past XA_PEER"
    assert rc(dict(base, flags=base["flags"] | R.XU_INLINE_IN)) == E, "an inline block shorter than its region, no gate"
    assert rc(dict(base, flags=base["flags"] & ~R.XU_GOSSIP, gossip=None)) == E, "records without a gossip plane"
