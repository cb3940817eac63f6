"""Known answers for the gossip data plane's per-tick kernels (gossip_round.hip to gossip_apply.hip) through SWIM_PRIM_GOSSIP of
swim_debug_prim_eval (include/swimhip_debug.h): launch_gossip_send and launch_gossip_apply run unchanged, in their own
grids, for one tick on a holder state built by tests/prim_ref.py, every output preset to a sentinel, and what they leave is
compared with the plain references there (gs_ref: Python sets of slot ids per member; validated without a GPU in
tests/test_prim_ref.py). Integer code: every comparison is equality. Where an atomic assigns the positions (ring segments,
a target's senders, the target and round lists, the recycled slots, the raw receipts) it is equality of multisets, with
the reason next to it. One launch per case, shared by the tests of that case. Engine only.

Whole-cluster parity reaches these kernels with small slot tables. The shapes here are the ones it never reaches: rows
above 1024 words (k_round_apply_b), rows staged in two and three LDS chunks with a partial last one, a second and third
batch of the group scan, a second batch of k_gossip_apply_big, (target, group) runs that straddle a wavefront, ring
positions that cross 2^32 and period tags that wrap at 1024.

The contact cases pin the look-back cut, the cached records, the RX rows and the lists of diverted sends on gossips their
targets never held (the replay's answer is then known without history: sent). The replay cases come from a tiny forward
simulation with explicit infectedFrom sets (prim_ref.GsSim: four members, scripted rounds, lossless links) that emits logs,
rings, S and the incarnation history as it goes, so each carries the device encoding and the explicit answer: (a) the target
delivered the gossip inside the sender's current incarnation, (b) only before it, (c) never held it, (d) the situation of
(a) through k_gossip_send_slow, (e) a window split by the RX row, (f) the situation of (a) after a rebirth. The general
correctness of replay_pair over long histories stays with the oracle parity, tape and fallback tests; no second oracle is
grown here.
"""
import functools

import numpy as np
import pytest

import prim_ref as R
from swimhip import _abi

pytestmark = pytest.mark.gpu

CASES = R.gs_cases()
ALL = list(CASES)
APPLIED = [n for n in ALL if CASES[n]["flags"] & R.GS_APPLY]
SENT, NEVER = R.GS_SENT, R.NEVER
DROPPED = {}  # case -> the replay-list entries that found no place (E_CONTACTS)


@functools.lru_cache(maxsize=None)
def ran(engine, name):
    """(state, reference, what the launchers left)."""
    c = CASES[name]
    params, inp, out = R.gs_pack(c)
    _abi.prim_eval(engine, _abi.PRIM_GOSSIP, params, inp, out)
    got, ref = R.gs_unpack(c, out), R.gs_ref(c)
    if ref["nrx"] > c["CRCAP"]:  # which pairs got the RX rows is an atomic's order: the reference is told, and checks
        ref = R.gs_ref(c, rows={ms for ms in ref["cev"] if got["crow"][ms] != R.NEVER})  # that they are pairs that wanted one
    if len(ref["rp"]) > c["RPCAP"]:  # E_CONTACTS: which sends found no place in the list, likewise
        kept = got["rp"][:c["RPCAP"]].tolist()
        assert len(set(kept)) == len(kept) and set(kept) <= set(ref["rp"]), (name, "rp under E_CONTACTS")
        DROPPED[name] = set(ref["rp"]) - set(kept)
        ref = R.gs_ref(c, dropped=DROPPED[name])
    return c, ref, got


def rows(plane):
    return [R.gs_bits(r) for r in plane]


def same(got, want, *at):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert len(bad) == 0, at + ("first difference at", int(bad[0]), "got", int(got.reshape(-1)[bad[0]]), "want",
                                int(want.reshape(-1)[bad[0]]), "differences", len(bad))


def listed(got_list, n, want, *at):
    """A list filled through an atomic counter: its first n entries are `want` in some order, the rest is untouched."""
    assert n == len(want), at + ("length", n, len(want))
    assert sorted(got_list[:n].tolist()) == sorted(want), at
    assert (got_list[n:] == SENT).all(), at + ("written past its end",)


# --------------------------------------------------------------------------------------------------- k_gossip_groups
@pytest.mark.parametrize("name", ALL)
def test_groups(engine, name):
    """The active groups in ascending order (a block scan: the positions are determined), their count and span."""
    c, ref, got = ran(engine, name)
    assert (got["nag"], got["span"]) == (ref["nag"], ref["span"]), name
    same(got["agroup"][:ref["nag"]], ref["agroup"], name, "agroup")
    assert (got["agroup"][ref["nag"]:] == SENT).all(), (name, "agroup past the count")
    assert got["xd_n"] == 0, (name, "per-tick counters reset")


# ---------------------------------------------------------------------------------- k_round_plan, k_round_apply_w / _b
@pytest.mark.parametrize("name", ALL)
def test_rounds(engine, name):
    c, ref, got = ran(engine, name)
    # block_reserve hands out rwl's places in the order the workgroups reach the counter
    listed(got["rwl"], got["nrwl"], sorted(ref["rwl"]), name, "rwl")
    for m in range(c["N"]):
        for f in ("rsend", "rwnew"):
            assert got[f][m] == ref[f].get(m, SENT), (name, f, m, int(got[f][m]), ref[f].get(m))
    for f in ("rhead", "rwin", "rseen", "dead_tick"):
        same(got[f], ref[f], name, f)
    for m, (g, w) in enumerate(zip(rows(got["WB"]), ref["WB"])):
        assert g == w, (name, "WB of member", m, "extra", sorted(g - w)[:8], "missing", sorted(w - g)[:8])


@pytest.mark.parametrize("name", ALL)
def test_holder_rows_table_and_counts(engine, name):
    """HB after the sweeps and the first receipts, the holder table S and the gossip counts."""
    c, ref, got = ran(engine, name)
    for m, (g, w) in enumerate(zip(rows(got["HB"]), ref["HB"])):
        assert g == w, (name, "HB of member", m, "extra", sorted(g - w)[:8], "missing", sorted(w - g)[:8])
    same(got["S"], ref["S"], name, "S")
    same(got["held"], ref["held"], name, "held")


ROUND_BASES = sorted({n.rsplit("_", 1)[0] for n in ALL if n.startswith("rounds_")})


@pytest.mark.parametrize("base", ROUND_BASES)
def test_round_paths_agree(engine, base):
    """Atomics, wave-staged and block-staged in one, two and three chunks leave the same words (rwl as a multiset)."""
    outs = {p: ran(engine, f"{base}_{p}")[2] for p in R.GS_PATHS}
    first = outs["atomic"]
    for p, o in outs.items():
        for f, a in first.items():
            if f == "rwl":
                assert sorted(a.tolist()) == sorted(o[f].tolist()), (base, p, f)
            elif isinstance(a, np.ndarray):
                same(o[f], a, base, p, f)
            else:
                assert o[f] == a, (base, p, f)


# ------------------------------------------------------------------------------------------ k_tin_scatter and the scan
@pytest.mark.parametrize("name", ALL)
def test_scatter(engine, name):
    c, ref, got = ran(engine, name)
    same(got["tin_cnt_send"], ref["tin_cnt_send"], name, "tin_cnt after the send launcher")
    same(got["tin_off"], ref["tin_off"], name, "tin_off")
    same(got["tin_cnt"], ref["tin_cnt"], name, "tin_cnt")
    same(got["tin_fill"], ref["tin_fill"], name, "tin_fill")
    for t, want in ref["tin"].items():  # a sender's place among its target's senders comes from an atomic on tin_fill
        o = int(ref["tin_off"][t])
        assert sorted(got["tin"][o:o + len(want)].tolist()) == want, (name, "senders of target", t)
    assert (got["tin"][int(ref["tin_cnt_send"].sum()):] == SENT).all(), (name, "tin past the pairs")
    listed(got["tlist"], got["ntl"], sorted(ref["tlist"]), name, "tlist")  # block_reserve order
    for t in range(c["N"]):
        assert got["rt0"][t] == ref["rt0"].get(t, SENT), (name, "rt0", t)


# ------------------------------------------------------------------------------------------------------ k_gossip_send
@pytest.mark.parametrize("name", ALL)
def test_first_receipts(engine, name):
    c, ref, got = ran(engine, name)
    same(got["rtail"], ref["rtail"], name, "rtail")
    mask = c["BCAP"] - 1
    for m in range(c["N"]):
        new = ref["new"].get(m, set())
        seg = [(ref["rt0"][m] + j) & R.M32 & mask for j in range(len(new))] if new else []
        # the lanes of a run take consecutive places, but which run of a target reserves first is an atomic's order
        assert sorted(got["rg"][m][seg].tolist()) == sorted(g | ref["tag"][m] << 22 for g in new), (name, "new ring entries of", m)
        keep = np.ones(c["BCAP"], bool)
        keep[seg] = False
        same(got["rg"][m][keep], c["rg"][m][keep], name, "ring entries outside the new segment of member", m)
    same(got["dead_rx"], ref["dead_rx"], name, "dead_rx")
    assert int(got["ctr_g"][0]) == ref["ctr_g"], (name, "gossip sends counted", int(got["ctr_g"][0]), ref["ctr_g"])
    same(got["em"], ref["em"], name, "emulator counters")
    assert int(got["err"][0]) == ref["err"], (name, "err", hex(int(got["err"][0])), hex(ref["err"]))


@pytest.mark.parametrize("name", [n for n in ALL if n.endswith("_em")])
def test_emulator_counters_change_no_receipt(engine, name):
    """The exact per-send path (GS_EM) delivers what the fast path delivers; only the ring order inside a segment may differ."""
    a, b = ran(engine, name)[2], ran(engine, name[:-3])[2]
    for f in ("HB", "WB", "rtail", "dead_rx", "ctr_g", "S", "held", "err"):
        same(a[f], b[f], name, f)
    same(np.sort(a["rg"], axis=1), np.sort(b["rg"], axis=1), name, "ring entries")


@pytest.mark.parametrize("name", ALL)
def test_contacts_and_replay_lists(engine, name):
    """k_gossip_contacts, k_contact_cache, k_rx_build and the sends k_gossip_send diverts. Without logged contacts every
    pair is looked at and none is flagged, cached, given an RX row or diverted."""
    c, ref, got = ran(engine, name)
    pairs = sorted(ref["tcontact"])
    rest = np.ones(c["N"] * c["F"], bool)
    rest[pairs] = False
    for f in ("tcontact", "cin"):
        same(got[f][pairs], [ref[f][ms] for ms in pairs], name, f)
        assert (got[f][rest] == SENT).all(), (name, f, "of a pair that does not exist")
    assert got["ncfl"] == ref["ncfl"] and got["nrx"] == ref["nrx"], (name, "ncfl, nrx", got["ncfl"], got["nrx"], ref["ncfl"], ref["nrx"])
    span, rows_used = ref["span"], set()
    for ms in range(c["N"] * c["F"]):
        rec = ref["cev"].get(ms)
        if rec is None:
            assert got["crow"][ms] == SENT and (got["cev"][ms] == SENT).all(), (name, "no record for pair", ms)
            continue
        same(got["cev"][ms][:len(rec)], rec, name, "cev record of pair", ms)
        assert (got["cev"][ms][len(rec):] == SENT).all(), (name, "cev words past the events of pair", ms)
        row = int(got["crow"][ms])
        if ms not in ref["rx"]:
            assert row == R.NEVER, (name, "RX_ALL for pair", ms, row)
            continue
        a, b, early = ref["rx"][ms]  # which row a pair gets is wave_append's order on nrx
        assert row < min(ref["nrx"], c["CRCAP"]) and row not in rows_used, (name, "RX row of pair", ms, row)
        rows_used.add(row)
        assert got["rxl"][row].tolist() == [ms, a, b], (name, "rxl of pair", ms, got["rxl"][row].tolist(), [ms, a, b])
        same(got["RX"][row][:span], R.gs_words(early, c["SLOTS"] // 64)[:span], name, "RX row of pair", ms)
        assert (got["RX"][row][span:] == np.uint64(R.GS_SENT64)).all(), (name, "RX row past the span")
    assert (got["RX"][len(rows_used):] == np.uint64(R.GS_SENT64)).all() and (got["rxl"][len(rows_used):] == SENT).all(), name
    for f, cap in (("rp", "RPCAP"), ("slow", "SLOWCAP")):  # wave_reserve hands out the places
        assert got[f + "_n"] == len(ref[f]), (name, f + "_n", got[f + "_n"], len(ref[f]))
        n = min(len(ref[f]), c[cap])
        kept = [v for v in ref[f] if v not in DROPPED.get(name, ())]
        assert sorted(got[f][:n].tolist()) == sorted(kept), (name, f)
        assert (got[f][n:] == np.uint64(R.GS_SENT64)).all(), (name, f, "past its end")
    same(got["fb"], ref["fb"], name, "fallback counters")


# ----------------------------------------------------------------- k_gossip_apply, k_gossip_apply_big, receipt routing
@pytest.mark.parametrize("name", APPLIED)
def test_apply(engine, name):
    c, ref, got = ran(engine, name)
    same(got["slot_exp"], ref["slot_exp"], name, "slot_exp")
    same(got["rc_ndrop"], ref["rc_ndrop"], name, "rc_ndrop")
    listed(got["ap_list"], got["nap"], sorted(ref["ap"]), name, "ap_list")  # wave_reserve order
    assert got["rc_n"] == len(ref["routed"]), (name, "rc_n", got["rc_n"], len(ref["routed"]))
    n = min(got["rc_n"], c["RCAP"])
    raw = got["rc_raw"][:n]
    if n == got["rc_n"]:  # every wave reserves its places with one atomic on rc_n
        assert sorted(raw.tolist()) == ref["routed"], (name, "rc_raw")
    else:  # E_RECEIPTS: the list keeps the RCAP receipts whose places came first
        assert len(set(raw.tolist())) == n and set(raw.tolist()) <= set(ref["routed"]), (name, "rc_raw under E_RECEIPTS")
    assert (got["rc_raw"][n:] == np.uint64(R.GS_SENT64)).all(), (name, "rc_raw past its end")
    # the routed lists: routing_ref of the receipts (gossip ids are distinct, so their order does not matter)
    cnt, off, per, sg = R.routing_ref(dict(N=c["N"], RCAP=c["RCAP"], rc_n=got["rc_n"], raw=raw, gid=c["slot_gid"]))
    same(got["rc_cnt"], cnt, name, "rc_cnt")
    same(got["rc_off"], off, name, "rc_off")
    for m, (slots, keys) in per.items():
        o = int(off[m])
        same(got["rc_slot"][o:o + len(slots)], slots, name, "rc_slot of member", m)
        assert np.array_equal(got["rc_key"][o:o + len(slots)], keys), (name, "rc_key of member", m)
    assert (got["rc_slot"][n:] == SENT).all(), (name, "rc_slot past its end")
    listed(got["sg_list"], got["nsg"], sorted(sg), name, "sg_list")
    hist = R.gs_hist_decode(got["hist"])
    assert hist == ref["hist"], (name, "incarnation history", len(hist), len(ref["hist"]))
    fresh = [kk for kk in hist if kk not in ref["hist_old"]]  # the sampled count of entries in use: one in 8 counts 8
    assert got["hist_n"] == 8 * sum(1 for gid, m in fresh if R.gs_hist_tag(gid, m) & 0x700 == 0), (name, "hist_n")


# --------------------------------------------------------------------------------------- k_gossip_expire, k_gossip_free
@pytest.mark.parametrize("name", ALL)
def test_expire_and_free(engine, name):
    c, ref, got = ran(engine, name)
    if not c["flags"] & R.GS_APPLY:
        for f in ("GU", "DM", "slot_used", "slot_exp", "free_list", "fexp", "hist", "rc_raw", "rc_slot", "rc_ndrop"):
            same(got[f], c.get(f, np.full(got[f].shape, SENT if got[f].dtype == np.uint32 else R.GS_SENT64, got[f].dtype)), name, f)
        assert got["free_top"] == c["free_top"] and got["nfexp"] == 0 and got["rc_n"] == 0, name
        return
    assert R.gs_bits(got["GU"]) == ref["GU"] and R.gs_bits(got["DM"]) == ref["DM"], (name, "GU / DM")
    same(got["slot_used"], ref["slot_used"], name, "slot_used")
    listed(got["fexp"], got["nfexp"], ref["fexp"], name, "fexp")  # wave_append order
    f0 = c["free_top"]
    assert got["free_top"] == f0 + len(ref["free"]), (name, "free_top")
    same(got["free_list"][:f0], c["free_list"][:f0], name, "free_list below the old top")
    listed(got["free_list"][f0:], len(ref["free"]), ref["free"], name, "free_list")  # an atomic on free_top


# ------------------------------------------------------------------------------------------- host validation (EINVAL)
def _bad(edit, **params):
    """The contact case with one value the kernels would index with (or a size) out of range."""
    c = R.gs_variant(CASES["contacts"], **params)
    for f in ("T", "tcnt", "log_cnt", "log_tg", "rg", "rhead", "rtail", "rwin", "rseen", "slot_subj"):
        c[f] = c[f].copy()
    edit(c)
    return c


def _set(f, idx, v):
    def edit(c):
        c[f][idx] = v
    return edit


REJECTED = {
    "target >= N": _bad(_set("T", (2, 1), 18)),
    "tcnt > F": _bad(_set("tcnt", 5, 9)),
    "log_cnt > F": _bad(_set("log_cnt", (3, 0), 9)),
    "log target >= N": _bad(_set("log_tg", (1, 0, 0), 18)),
    "ring slot >= SLOTS": _bad(_set("rg", (0, 1), 192 | 5 << 22)),
    "ring longer than BCAP": _bad(_set("rtail", 4, 65)),
    "rwin before rhead": _bad(_set("rwin", 0, 0xFFFFFFFF)),
    "rseen past rtail": _bad(_set("rseen", 0, 7)),
    "slot_subj == N": _bad(_set("slot_subj", 9, 18)),
    "k = 0": _bad(lambda c: None, k=0),
    "cev_cap > CEV": _bad(lambda c: None, cev_cap=7),
    "cw > 1024": _bad(lambda c: None, cw=1025),
    "cb > 4096": _bad(lambda c: None, cb=4097),
    "cx > 8192": _bad(lambda c: None, cx=8193),
    "HCAP no power of two": _bad(lambda c: None, HCAP=48, hist=np.zeros((48, R.HREC), np.uint64)),
    "sort_cap = 1": _bad(lambda c: None, sort_cap=1),
    "SPR = 0": _bad(lambda c: None, SPR=0),
    "ep_loss > 100": _bad(lambda c: None, ep_loss=101),
    "free_top < 0": _bad(lambda c: None, free_top=0xFFFFFFFF),
    "free list too short for the slots in use": _bad(lambda c: None, free_top=192),
}


@pytest.mark.parametrize("what", list(REJECTED))
def test_rejected_before_any_launch(engine, what):
    """What the kernels would index with is checked on the host: SWIM_EINVAL, and not a word of `out` changes."""
    params, inp, out = R.gs_pack(REJECTED[what])
    before = out.copy()
    assert _abi.prim_eval_rc(engine, _abi.PRIM_GOSSIP, params, inp, out) == _abi.SWIM_EINVAL, what
    assert np.array_equal(out, before), what


def test_rejected_lengths_and_counter(engine):
    params, inp, out = R.gs_pack(CASES["contacts"])
    ev = lambda i, o, p=params: _abi.prim_eval_rc(engine, _abi.PRIM_GOSSIP, p, i, o)
    assert ev(inp[:-1].copy(), out.copy()) == _abi.SWIM_EINVAL, "an in buffer 8 bytes short (no room for leaving[N])"
    assert ev(inp, out[:-1].copy()) == _abi.SWIM_EINVAL, "an out buffer 8 bytes short"
    assert ev(inp, out.copy(), params[:-1]) == _abi.SWIM_EINVAL, "26 params"
    o2 = out.copy()
    o2.view(np.uint32)[-8 - 16 + R.GS_SC.index("rc_n")] = 1
    assert ev(inp, o2) == _abi.SWIM_EINVAL, "rc_n starts a tick at 0"
    assert ev(inp, out) == _abi.SWIM_OK, "the unedited case runs"
