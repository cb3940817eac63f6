"""Known answers for the device primitives the per-tick kernels are built from, through swim_debug_prim_eval
(include/swimhip_debug.h): the engine's own launch_scan, k_seg_sort, launch_receipt_routing, launch_ring_move and the
inline helpers of dev_util.h / engine.h / swim_common.h run on chosen data and are compared bit for bit with the plain
references of tests/prim_ref.py (which tests/test_prim_ref.py validates without a GPU). All of it is integer code: no
tolerance appears anywhere. Engine only; the oracle has none of these structures.

The whole-engine parity tests reach these primitives only with whatever a simulated cluster produces; here the sizes,
lane masks and window positions are the ones where such code goes wrong.
"""
import numpy as np
import pytest

import prim_ref as R
from swimhip import _abi

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5


def ev(engine, op, params, inp, out):
    return _abi.prim_eval(engine, op, params, inp, out)


def words(*arrays):
    """The arrays' bytes one after the other, as 32-bit words (u64 arrays first keep everything 8-byte aligned)."""
    return np.frombuffer(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays), dtype=np.uint32).copy()


# ------------------------------------------------------------------------------------------------------------ scan
# launch_scan as the receipt routing (n = N members) and the target-major send (tin_cnt) call it: one block of 1024
# (n <= 1024), the block edges, several blocks, and the 2^20 ceiling k_scan_top's single block of 1024 sums assumes.
@pytest.mark.parametrize("n", R.SCAN_NS)
def test_scan(engine, n):
    for kind in R.SCAN_KINDS:
        v = R.scan_input(n, kind)
        out = np.full(n + 64, SENT, np.uint32)
        ev(engine, _abi.PRIM_SCAN, [n], v, out)
        assert np.array_equal(out[:n], R.scan_ref(v)), (n, kind)
        assert (out[n:] == SENT).all(), (n, kind, "words at and past n keep the sentinel")


# -------------------------------------------------------------------------------------------------------- seg sort
SEG_CASES = R.seg_cases()


def run_seg_sort(engine, c, fb):
    total = len(c["key"])
    inp = words(c["key"], c["val"], c["off"], c["cnt"], c["sg"])
    out = np.zeros(2 + 3 * total, np.uint32)
    ev(engine, _abi.PRIM_SEG_SORT, [total, len(c["off"]), len(c["sg"]), c["run"], fb], inp, out)
    return (int(out[0]) | int(out[1]) << 32, out[2:2 + 2 * total].view(np.uint64), out[2 + 2 * total:])


# run = 2 is SWIM_CAPS sort=2, run = 4096 the default; 64 lies between and is sorted nowhere else. Lengths around run,
# 2 run and an odd number of runs (the last run without a partner); the 1500-segment case reuses a block's LDS across the
# li += gridDim.x loop; "unlisted" has segments the kernel must not touch.
@pytest.mark.parametrize("name", list(SEG_CASES))
def test_seg_sort(engine, name):
    c = SEG_CASES[name]
    key, val, merges = R.seg_sort_ref(c)
    got_m, got_k, got_v = run_seg_sort(engine, c, 1)
    for s in c["sg"].tolist():
        o, n = int(c["off"][s]), int(c["cnt"][s])
        assert np.array_equal(got_k[o:o + n], key[o:o + n]), (name, "segment", s, "length", n, "keys")
        assert np.array_equal(got_v[o:o + n], val[o:o + n]), (name, "segment", s, "length", n, "values")
    assert np.array_equal(got_k, key) and np.array_equal(got_v, val), "nothing outside the listed segments changes"
    assert got_m == merges, "FB_SORT_MERGE counts the listed segments longer than run"
    nm, nk, nv = run_seg_sort(engine, c, 0)  # fb = nullptr (a handle without SWIM_CAPS / SWIM_FALLBACKS)
    assert nm == 0 and np.array_equal(nk, key) and np.array_equal(nv, val)


# --------------------------------------------------------------------------------------------------------- routing
# launch_receipt_routing as launch_gossip queues it: N = 5 (one scan block, fewer members than lanes) and 1025 (the
# hot member sits in the second scan block), sort_cap = 64 so the hot member's 150 receipts take the merge path.
@pytest.mark.parametrize("N,over", [(5, False), (1025, False), (1025, True)])
def test_receipt_routing(engine, N, over):
    c = R.routing_case(N, over, 50 + N)
    cnt, off, rows, sg = R.routing_ref(c)
    RCAP = c["RCAP"]
    out = words(np.full(RCAP, R.M64, np.uint64), np.zeros(1, np.uint64), np.full(RCAP + 3 * N + 2, SENT, np.uint32))
    ev(engine, _abi.PRIM_ROUTING, [N, RCAP, c["rc_n"], c["SLOTS"], R.ROUTE_SORT_CAP, 1], words(c["raw"], c["gid"]), out)
    rc_key = out[:2 * RCAP].view(np.uint64)
    merges = int(out[2 * RCAP]) | int(out[2 * RCAP + 1]) << 32
    rest = out[2 * RCAP + 2:]
    rc_slot, rc_off, rc_cnt, sg_list, nsg = (rest[:RCAP], rest[RCAP:RCAP + N], rest[RCAP + N:RCAP + 2 * N],
                                             rest[RCAP + 2 * N:RCAP + 3 * N], int(rest[RCAP + 3 * N]))
    assert np.array_equal(rc_cnt, cnt) and np.array_equal(rc_off, off), "rc_off is the exclusive scan of the counts"
    for m, (slots, keys) in rows.items():
        o = int(off[m])
        assert np.array_equal(rc_slot[o:o + len(slots)], slots), (m, "slots in ascending slot_gid")
        assert np.array_equal(rc_key[o:o + len(slots)], keys), (m, "rc_key alongside")
    used = int(cnt.sum())
    assert used == min(c["rc_n"], RCAP), "only the first RCAP receipts count"
    assert (rc_slot[used:] == SENT).all() and (rc_key[used:] == np.uint64(R.M64)).all()
    assert nsg == len(sg) and set(sg_list[:nsg].tolist()) == sg and (sg_list[nsg:] == SENT).all()
    assert merges == sum(1 for m in sg if cnt[m] > R.ROUTE_SORT_CAP) >= 1


# ----------------------------------------------------------------------------------------------------- collectives
BLOCKS = 8  # several blocks contend on one counter, 4 waves each as in every engine kernel that calls these
PATTERNS = R.lane_patterns(BLOCKS)


def halves(v):
    """A uint64 array as its (low, high) 32-bit halves."""
    return [(v & np.uint64(R.M32)).astype(np.uint32), (v >> np.uint64(32)).astype(np.uint32)]


def join64(lo, hi):
    return lo.astype(np.uint64) | hi.astype(np.uint64) << np.uint64(32)


def run_wave(engine, sub, a, ctr0=0):
    T = BLOCKS * 256
    arg = np.zeros((3, T), np.uint32)
    arg[:len(a)] = a
    out = np.full(3 * T + 4, SENT, np.uint32)
    out[3 * T:] = [ctr0, SENT, SENT, SENT]
    ev(engine, _abi.PRIM_WAVE, [sub, BLOCKS], arg, out)
    assert (out[3 * T + 1:] == SENT).all()
    return out[:3 * T].reshape(3, T), int(out[3 * T])


# wave_append inside a divergent branch (k_scatter_rc's `f == 1`, the list builders of the gossip plane)
@pytest.mark.parametrize("pat", list(PATTERNS))
def test_wave_append(engine, pat):
    act = PATTERNS[pat]
    r, ctr = run_wave(engine, _abi.WAVE_APPEND, [act.astype(np.uint32)], ctr0=3)
    assert R.append_ok(act, r[0], 3, ctr), pat
    assert (r[0][~act] == SENT).all() and ctr == 3 + int(act.sum())


def reserve_counts(pat, seed):
    """Per-thread n: zero outside the pattern, small inside, with one large request."""
    rng = np.random.default_rng(seed)
    n = np.where(PATTERNS[pat], rng.integers(0, 7, BLOCKS * 256), 0).astype(np.uint32)
    n[np.flatnonzero(PATTERNS[pat])[-1]] = 2**31
    return n


# wave_reserve / block_reserve: every lane calls (inactive work passes n = 0), as the list builders of the member and
# gossip kernels do; the patterns are the lanes with work
@pytest.mark.parametrize("pat", list(PATTERNS))
def test_wave_reserve(engine, pat):
    n = reserve_counts(pat, 60)
    r, ctr = run_wave(engine, _abi.WAVE_RESERVE, [n], ctr0=11)
    assert R.reserve_ok(n, r[0], 64, 11, ctr), pat
    assert ctr == (11 + int(n.astype(np.uint64).sum())) & R.M32


@pytest.mark.parametrize("pat", list(PATTERNS))
def test_block_reserve_three_calls(engine, pat):
    n = np.stack([reserve_counts(pat, 61), np.roll(reserve_counts(pat, 62), 64) & 0xFF, reserve_counts(pat, 63) & 0xFF])
    n[1, :256] = 0  # an all-zero block between two calls that reserve
    r, ctr = run_wave(engine, _abi.WAVE_BLOCK_RESERVE, n, ctr0=0)
    assert R.reserve_ok(n.reshape(-1), r.reshape(-1), 256, 0, ctr), pat
    assert ctr == int(n.astype(np.uint64).sum()) & R.M32


def test_reserve_nothing_leaves_the_counter(engine):
    z = np.zeros((3, BLOCKS * 256), np.uint32)
    for sub in (_abi.WAVE_RESERVE, _abi.WAVE_BLOCK_RESERVE, _abi.WAVE_APPEND):
        assert run_wave(engine, sub, z, ctr0=77)[1] == 77


# wave_sum / wave_min are called by every lane (ctr_wave_add, the triage): the lanes outside the pattern hold the
# operation's identity
@pytest.mark.parametrize("pat", list(PATTERNS))
def test_wave_sum_min(engine, pat):
    rng = np.random.default_rng(64)
    act = PATTERNS[pat]
    v = np.where(act, rng.integers(2**31, 2**32, len(act)), 0).astype(np.uint32)  # two lanes already wrap
    assert np.array_equal(run_wave(engine, _abi.WAVE_SUM32, [v])[0][0], R.wave_sum32_ref(v)), pat
    v = np.where(act, rng.integers(0, 2**32, len(act)), R.M32).astype(np.uint32)
    assert np.array_equal(run_wave(engine, _abi.WAVE_MIN32, [v])[0][0], R.wave_min_ref(v)), pat
    v64 = np.where(act, rng.integers(2**63 - 2**33, 2**63 + 2**33, len(act), dtype=np.uint64), 0).astype(np.uint64)
    v64[np.flatnonzero(act)[::3]] |= np.uint64(R.M32)  # low halves at 2^32 - 1: every add carries
    r = run_wave(engine, _abi.WAVE_SUM64, halves(v64))[0]
    assert np.array_equal(join64(r[0], r[1]), R.wave_sum64_ref(v64)), pat


def test_wave_sum64_carries(engine):
    v = np.zeros(BLOCKS * 256, np.uint64)
    v[:512] = R.sum64_values()
    r = run_wave(engine, _abi.WAVE_SUM64, halves(v))[0]
    assert np.array_equal(join64(r[0], r[1]), R.wave_sum64_ref(v))


# dirty_mark as key_put calls it (the row's owner lane) and dirty_mark_wave as the wave that owns a row calls it, on
# masks of MW words: MW > 1 (more than 131 072 members) is beyond any stored table one card holds
@pytest.mark.parametrize("MW", [1, 2, 3])
def test_dirty_mark(engine, MW):
    a, pre = R.dirty_thread_case(MW)
    out = pre.copy()
    ev(engine, _abi.PRIM_DIRTY, [0, 1, MW], a, out)
    want = R.dirty_ref(pre, [[int(s) for s in a[:, t] if s != R.NEVER] for t in range(256)])
    assert np.array_equal(out, want), "exactly the bits of the written chunks, pre-set bits kept"


@pytest.mark.parametrize("MW", [1, 2, 3])
def test_dirty_mark_wave(engine, MW):
    a, pre = R.dirty_wave_case(MW)
    out = pre.copy()
    ev(engine, _abi.PRIM_DIRTY, [1, 2, MW], a, out)
    s, wr = a[0].reshape(8, 64), a[1].reshape(8, 64) != 0
    want = R.dirty_ref(pre, [s[r][wr[r]].tolist() for r in range(8)])
    for r in range(8):
        assert out[r].tolist() == want[r].tolist(), ("row", r)


# ------------------------------------------------------------------------------------------------ window arithmetic
# div_gt over every gossip period a configuration can give it, far past the tick differences a run produces
@pytest.mark.parametrize("g", R.GOSSIP_TS)
def test_div_gt(engine, g):
    x = R.div_gt_inputs(g)
    out = np.zeros(len(x) + 1, np.uint32)
    ev(engine, _abi.PRIM_ARITH, [_abi.ARITH_DIV_GT, len(x), g], x, out)
    assert int(out[-1]) == (2**32 - 1 if g == 1 else 2**32 // g), "Dev::gt_mul as swim_create computes it"
    bad = np.flatnonzero(out[:-1] != R.div_gt_ref(x, g))
    assert len(bad) == 0, (g, [(int(x[i]), int(out[i])) for i in bad[:5]])


def test_s16_tick(engine):  # the 13-bit creation-tick window of the holder entries, up to the top of the tick range
    rows = R.s16_cases()
    out = np.zeros(len(rows), np.uint32)
    ev(engine, _abi.PRIM_ARITH, [_abi.ARITH_S16, len(rows)], R.u32(rows[:, :2]), out)
    assert np.array_equal(out, R.u32(rows[:, 2]))


def test_rg_entry_period(engine):  # the 10-bit infection-period window of the ring entries
    rows = R.rg_cases()
    out = np.zeros((len(rows), 3), np.uint32)
    ev(engine, _abi.PRIM_ARITH, [_abi.ARITH_RG, len(rows)], R.u32(rows), out)
    assert np.array_equal(join64(out[:, 0], out[:, 1]), rows[:, 1]), "rg_period returns the period the entry was written at"
    assert np.array_equal(out[:, 2], R.u32(rows[:, 0])), "the slot bits survive"


def test_key8(engine):
    k = R.u32(R.KEY8_KEYS)
    out = np.zeros(len(k), np.uint32)
    ev(engine, _abi.PRIM_ARITH, [_abi.ARITH_KEY8, len(k)], k, out)
    assert np.array_equal(out, R.key8_ref(k))
    lo = out[:0xFF]  # two keys below 0xFF are equal iff their shadows are
    assert np.array_equal(lo[:, None] == lo[None, :], k[:0xFF, None] == k[None, :0xFF])
    assert (lo != 0xFF).all() and (out[0xFF:] == 0xFF).all()


def test_delay_ticks(engine):
    for di, thr, x in R.delay_cases():
        out = np.zeros(len(x), np.uint32)
        ev(engine, _abi.PRIM_ARITH, [_abi.ARITH_DELAY, len(x), di, len(thr)], words(thr, x), out)
        assert np.array_equal(out, R.delay_ref(thr, x)), (di, len(thr))


def test_epoch_at(engine):
    for tab, k in R.epoch_cases():
        out = np.zeros(len(k), np.uint32)
        ev(engine, _abi.PRIM_ARITH, [_abi.ARITH_EPOCH, len(k)], words(tab, k), out)
        assert np.array_equal(out.view(np.int32).astype(np.int64), R.epoch_ref(tab, k)), tab.tolist()


# payload_key_at of a payload received from another shard: the rank of the subject's chunk among the shipped ones, over
# MW mask words. MW > 1 needs a stored table of more than 131 072 members, which no whole-engine test can build.
@pytest.mark.parametrize("i", range(len(R.paykey_cases())))
def test_payload_key_at_rx(engine, i):
    MW, mask, subs = R.paykey_cases()[i]
    NS, base, ship = R.paykey_input(MW, mask)
    out = np.zeros(len(subs), np.uint32)
    ev(engine, _abi.PRIM_ARITH, [_abi.ARITH_PAYKEY, len(subs), MW, NS, 2, 4, 64], words(mask, base, ship, subs), out)
    assert np.array_equal(out, R.paykey_ref(mask, subs)), (MW, [hex(int(w)) for w in mask])


# the PRECONVERGED list order behind list_at, at sizes next to a power of four (where make_perm's domain changes)
@pytest.mark.parametrize("n", R.FEISTEL_NS)
def test_feistel(engine, n):
    for keys in R.FEISTEL_KEYS:
        out = np.zeros(2 * n, np.uint32)
        ev(engine, _abi.PRIM_FEISTEL, [n, *keys], None, out)
        assert np.array_equal(np.sort(out[:n]), np.arange(n, dtype=np.uint32)), "a permutation of [0, n)"
        assert np.array_equal(out[:n], out[n:]), "device and host compile of the same SW_HD functions agree"
        assert np.array_equal(out[:n], R.feistel_ref(n, keys))


# launch_ring_move as grow_caps calls it (B -> 2 B), and B = B2; ring positions are absolute and wrap past 2^32
@pytest.mark.parametrize("B,B2", [(64, 128), (64, 64)])
def test_ring_move(engine, B, B2):
    rg, h, t = R.ring_case(B, B2)
    out = np.full((len(h), B2), R.RING_SENTINEL, np.uint32)
    ev(engine, _abi.PRIM_RING_MOVE, [len(h), B, B2], words(rg, h, t), out)
    assert np.array_equal(out, R.ring_ref(rg, h, t, B2))


# ------------------------------------------------------------------------------------------------------ validation
def test_invalid_arguments_are_refused_before_any_launch(engine):
    def rc(op, params, n_in, n_out):  # zero words of the given counts
        return _abi.prim_eval_rc(engine, op, params, np.zeros(n_in + 2, np.uint32)[:n_in],
                                 np.zeros(n_out + 2, np.uint32)[:n_out])

    E = _abi.SWIM_EINVAL
    assert rc(_abi.PRIM_SCAN, [0], 0, 64) == E and rc(_abi.PRIM_SCAN, [2**20 + 1], 2**20 + 1, 2**20 + 65) == E
    assert rc(_abi.PRIM_SCAN, [4], 4, 4) == E and rc(99, [4], 4, 68) == E
    # total = 4, one member, one listed: run not a power of two / above SORT_MAX; a segment past the arrays; sg past nmem
    ok = words(np.zeros(4, np.uint64), np.zeros(4, np.uint32), R.u32([0]), R.u32([4]), R.u32([0]))
    seg = lambda params, inp: _abi.prim_eval_rc(engine, _abi.PRIM_SEG_SORT, params, inp, np.zeros(14, np.uint32))
    assert seg([4, 1, 1, 4, 1], ok) == 0
    assert seg([4, 1, 1, 3, 1], ok) == E and seg([4, 1, 1, 8192, 1], ok) == E and seg([4, 1, 1, 1, 1], ok) == E
    bad = ok.copy()
    bad[13] = 5  # cnt
    assert seg([4, 1, 1, 4, 1], bad) == E
    bad = ok.copy()
    bad[14] = 1  # sg
    assert seg([4, 1, 1, 4, 1], bad) == E
    # a receipt for a member >= N, a slot >= SLOTS
    route = lambda raw: _abi.prim_eval_rc(engine, _abi.PRIM_ROUTING, [2, 4, 1, 8, 64, 0],
                                          words(np.array([raw], np.uint64), np.zeros(8, np.uint64)),
                                          np.zeros(8 + 2 + 4 + 6 + 2, np.uint32))
    assert route(1 << 32 | 7) == 0 and route(2 << 32 | 7) == E and route(1 << 32 | 8) == E
    assert rc(_abi.PRIM_WAVE, [_abi.WAVE_SUM64 + 1, 1], 768, 772) == E and rc(_abi.PRIM_WAVE, [0, 65], 768, 772) == E
    # a subject past the mask words
    a = np.zeros((3, 256), np.uint32)
    a[0, 5] = 64 * R.CH
    assert _abi.prim_eval_rc(engine, _abi.PRIM_DIRTY, [1, 1, 1], a, np.zeros(4, np.uint64)) == E
    assert _abi.prim_eval_rc(engine, _abi.PRIM_DIRTY, [0, 1, 1], a, np.zeros(256, np.uint64)) == E
    assert rc(_abi.PRIM_DIRTY, [0, 1, 4], 768, 2048) == E
    assert rc(_abi.PRIM_ARITH, [_abi.ARITH_DIV_GT, 4, 0], 4, 5) == E
    assert rc(_abi.PRIM_ARITH, [_abi.ARITH_DELAY, 4, 16, 0], 4, 4) == E
    assert rc(_abi.PRIM_ARITH, [_abi.ARITH_DELAY, 4, 0, 257], 261, 4) == E
    # payload_key_at: a subject >= NS, NS past the mask words, ri >= RXCAP
    pk = lambda params, s: _abi.prim_eval_rc(engine, _abi.PRIM_ARITH, [_abi.ARITH_PAYKEY, 1, *params],
                                             words(np.zeros(1, np.uint64), np.zeros(min(params[1], 8), np.uint32),
                                                   R.u32([s])), np.zeros(2, np.uint32)[:1])
    assert pk([1, 8, 0, 1, 0], 7) == 0 and pk([1, 8, 0, 1, 0], 8) == E and pk([1, 64 * R.CH + 1, 0, 1, 0], 0) == E
    assert pk([1, 8, 1, 1, 0], 0) == E and pk([1, 8, 0, 1, 2], 0) == E
    assert rc(_abi.PRIM_FEISTEL, [0, 1, 2, 3, 4], 0, 0) == E
    assert rc(_abi.PRIM_FEISTEL, [2**20 + 1, 1, 2, 3, 4], 0, 2**21 + 2) == E
    # ring sizes that are no power of two, B > B2, more held entries than the ring has
    ring = lambda B, B2, h, t: _abi.prim_eval_rc(engine, _abi.PRIM_RING_MOVE, [1, B, B2],
                                                 words(np.zeros(B, np.uint32), R.u32([h]), R.u32([t])),
                                                 np.zeros(B2 + 2, np.uint32)[:B2])
    assert ring(4, 8, 0, 4) == 0 and ring(4, 8, 0, 5) == E and ring(3, 8, 0, 1) == E and ring(8, 4, 0, 1) == E
    assert ring(4, 6, 0, 1) == E
