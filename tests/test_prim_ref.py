"""tests/prim_ref.py checked without a GPU: every reference against a second, naive formulation on small inputs, and
every generated input set against the conditions the primitives state, so that a red test in
tests/test_gpu_primitives.py points at the device code and not at its yardstick."""
import numpy as np
import pytest

import prim_ref as R

M32 = R.M32


def test_scan_ref_and_inputs():
    for n in (1, 2, 5, 300):
        for kind in R.SCAN_KINDS:
            v = R.scan_input(n, kind)
            acc, want = 0, []
            for x in v:
                want.append(acc & M32)
                acc += int(x)
            assert R.scan_ref(v).tolist() == want, (n, kind)
    for n in R.SCAN_NS:
        assert 1 <= n <= 2**20
        for kind in R.SCAN_KINDS:
            v = R.scan_input(n, kind)
            assert v.dtype == np.uint32 and len(v) == n
        assert int(R.scan_input(n, "zero").sum()) == 0 and int(R.scan_input(n, "one").sum()) == n
        assert int(R.scan_input(n, "random").max()) < 4096
        if n >= 2:  # the total passes 2^32, so the reference (and the scan) wraps
            assert int(R.scan_input(n, "wrap").astype(np.uint64).sum()) >= 2**32
    assert R.scan_ref(R.u32([2**32 - 1, 2, 5])).tolist() == [0, 2**32 - 1, 1]


def test_seg_sort_ref_and_inputs():
    cases = R.seg_cases()
    assert {f"run{r}-{o}" for r in (2, 64, 4096) for o in ("random", "sorted", "reversed")} <= set(cases)
    for name, c in cases.items():
        total, run = len(c["key"]), c["run"]
        assert run & (run - 1) == 0 and 2 <= run <= R.SORT_MAX
        assert len(set(c["sg"].tolist())) == len(c["sg"]) and (c["sg"] < len(c["off"])).all()
        covered = np.zeros(total, int)
        for o, n in zip(c["off"].tolist(), c["cnt"].tolist()):
            assert o + n <= total
            covered[o:o + n] += 1
            k = c["key"][o:o + n]
            assert len(set(k.tolist())) == n, "keys unique within a segment"
            assert not (k == np.uint64(R.M64)).any(), "~0 is the pad value"
            if n >= 3:
                assert 0 in k.tolist() and (k >= np.uint64(2**63)).any()
        assert covered.max() == 1 and (covered == 0).any(), "segments disjoint, with entries outside them"
        key, val, merges = R.seg_sort_ref(c)
        # second formulation: Python's sort on (key, val) pairs
        for s in c["sg"].tolist():
            o, n = int(c["off"][s]), int(c["cnt"][s])
            pairs = sorted(zip(c["key"][o:o + n].tolist(), c["val"][o:o + n].tolist()))
            assert [p[0] for p in pairs] == key[o:o + n].tolist() and [p[1] for p in pairs] == val[o:o + n].tolist()
        listed = np.zeros(total, bool)
        for s in c["sg"].tolist():
            listed[int(c["off"][s]):int(c["off"][s]) + int(c["cnt"][s])] = True
        assert np.array_equal(key[~listed], c["key"][~listed]) and np.array_equal(val[~listed], c["val"][~listed])
        assert merges == sum(1 for s in c["sg"].tolist() if c["cnt"][s] > run)
    for run in (2, 64):
        assert sorted(cases[f"run{run}-random"]["cnt"].tolist()) == sorted(
            [2, 3, run - 1, run, run + 1, 2 * run - 1, 2 * run, 2 * run + 1, 3 * run, 5 * run + 7])
    assert sorted(cases["run4096-random"]["cnt"].tolist()) == [4095, 4096, 4097, 3 * 4096 + 5]
    for o, keyfn in (("sorted", lambda k: k == sorted(k)), ("reversed", lambda k: k == sorted(k, reverse=True))):
        c = cases[f"run64-{o}"]
        assert all(keyfn(c["key"][a:a + n].tolist()) for a, n in zip(c["off"].tolist(), c["cnt"].tolist()))
    c = cases["1500-segments"]
    assert len(c["sg"]) == 1500 > 1024 and 2 <= c["cnt"].min() and c["cnt"].max() <= 5
    c = cases["unlisted"]
    ls = set(c["sg"].tolist())
    assert any(c["cnt"][s] > 1 for s in range(len(c["cnt"])) if s not in ls), "a segment with cnt > 1 not in sg"
    assert any(c["cnt"][s] > c["run"] for s in range(len(c["cnt"])) if s not in ls)
    assert {int(c["cnt"][s]) for s in ls} >= {0, 1}, "listed segments with cnt <= 1"


@pytest.mark.parametrize("N,over", [(5, False), (1025, False), (1025, True)])
def test_routing_ref_and_inputs(N, over):
    c = R.routing_case(N, over, 50 + N)
    raw = c["raw"]
    assert len(raw) == min(c["rc_n"], c["RCAP"]) and (c["rc_n"] == c["RCAP"] + 5) == over
    mem, slot = [int(x) >> 32 for x in raw], [int(x) & M32 for x in raw]
    assert max(mem) < N and max(slot) < c["SLOTS"] and len(set(zip(mem, slot))) == len(raw)
    assert len(set(c["gid"].tolist())) == c["SLOTS"] and R.M64 not in c["gid"].tolist()
    order = np.argsort(c["gid"], kind="stable")
    assert not np.array_equal(order, np.arange(c["SLOTS"])), "sorting by gid is not sorting by slot"
    cnt, off, rows, sg = R.routing_ref(c)
    assert int(cnt.sum()) == len(raw) and cnt.max() > R.ROUTE_SORT_CAP, "one member above sort_cap"
    assert (cnt == 1).sum() >= max(1, N // 4) and (cnt == 0).any(), "many with exactly one receipt, some with none"
    naive = {}
    for m, s in zip(mem, slot):
        naive.setdefault(m, []).append(s)
    o = 0
    for m in range(N):
        assert int(off[m]) == o and int(cnt[m]) == len(naive.get(m, []))
        o += int(cnt[m])
        if m in naive:
            want = sorted(naive[m], key=lambda s: int(c["gid"][s]))
            assert rows[m][0].tolist() == want and rows[m][1].tolist() == [int(c["gid"][s]) for s in want]
    assert sg == {m for m, v in naive.items() if len(v) >= 2}


def test_lane_patterns_and_collective_checks():
    pats = R.lane_patterns(8)
    assert set(pats) == {"full", "lane0", "lane63", "alternating", "sparse", "per-wave"}
    for name, a in pats.items():
        assert a.dtype == bool and len(a) == 8 * 256 and a.any()
    w = pats["per-wave"].reshape(-1, 4, 64)
    assert all(len({tuple(x.tolist()) for x in blk}) == 4 for blk in w), "four different masks in every block"
    assert pats["lane0"].reshape(-1, 64)[:, 0].all() and pats["lane0"].sum() == 32
    assert pats["lane63"].reshape(-1, 64)[:, 63].all() and pats["lane63"].sum() == 32
    assert 0 < pats["sparse"].sum() < 8 * 256 // 4
    # append_ok accepts what a serial model of wave_append produces, waves in any order, and rejects near misses
    rng = np.random.default_rng(0)
    for a in pats.values():
        res, ctr = np.full(len(a), 0xABABABAB, np.uint32), 0
        for wv in rng.permutation(len(a) // 64):
            for l in range(64):
                if a[64 * wv + l]:
                    res[64 * wv + l] = ctr
                    ctr += 1
        assert R.append_ok(a, res, 0, ctr)
        assert not R.append_ok(a, res, 0, ctr + 1)
        for wv in range(len(a) // 64):  # two lanes of one wave swapped: still a permutation, not in lane order
            i = 64 * wv + np.flatnonzero(a[64 * wv:64 * wv + 64])
            if len(i) >= 2:
                bad = res.copy()
                bad[i[0]], bad[i[-1]] = bad[i[-1]], bad[i[0]]
                assert not R.append_ok(a, bad, 0, ctr)
                break
    # reserve_ok the same way
    for group in (64, 256):
        n = rng.integers(0, 5, 1024).astype(np.uint32)
        n[0:256] = 0
        n[300] = 2**31
        res, ctr = np.zeros(1024, np.uint32), 7
        for g in rng.permutation(1024 // group):
            for t in range(group * g, group * g + group):
                res[t] = ctr & M32
                ctr += int(n[t])
        assert int(n.astype(np.uint64).sum()) < 2**32
        assert R.reserve_ok(n, res, group, 7, ctr & M32)
        bad = res.copy()
        bad[700] += 1
        assert not R.reserve_ok(n, bad, group, 7, ctr & M32)
        assert not R.reserve_ok(n, res, group, 8, ctr & M32)
    assert R.reserve_ok(np.zeros(256, np.uint32), np.zeros(256, np.uint32), 64, 5, 5)
    assert not R.reserve_ok(np.zeros(256, np.uint32), np.zeros(256, np.uint32), 64, 5, 6)


def test_wave_reduction_refs():
    rng = np.random.default_rng(1)
    v = rng.integers(0, 2**32, 256, dtype=np.uint32)
    for w in range(4):
        assert R.wave_sum32_ref(v)[64 * w + 9] == sum(int(x) for x in v[64 * w:64 * w + 64]) & M32
        assert R.wave_min_ref(v)[64 * w + 63] == min(int(x) for x in v[64 * w:64 * w + 64])
    assert R.wave_sum32_ref(np.full(64, 2**31, np.uint32)).tolist() == [0] * 64  # wraps
    v = R.sum64_values()
    got = R.wave_sum64_ref(v)
    fs = np.array([float(x) for x in v]).reshape(-1, 64).sum(axis=1)  # the high bits, independently, in floating point
    for w in range(len(v) // 64):
        want = 0
        for x in v[64 * w:64 * w + 64].tolist():
            want = (want + x) % 2**64
        assert int(got[64 * w]) == want == int(got[64 * w + 63])
        assert abs((fs[w] - want) / 2**64 - round((fs[w] - want) / 2**64)) < 1e-6
    assert int(got[0]) == 64 * (2**32 - 1) and int(got[64]) == 0 and int(got[192]) == 2**32
    assert int(got[128]) == (64 * (2**63 - 1)) % 2**64 and int(got[320]) == 2**64 - 64


@pytest.mark.parametrize("MW", [1, 2, 3])
def test_dirty_inputs_and_ref(MW):
    lim = MW * 64 * R.CH
    a, pre = R.dirty_thread_case(MW)
    assert pre.shape == (256, MW) and pre.any() and not pre[::2].any()
    used = a[a != R.NEVER]
    assert (used < lim).all() and (a == R.NEVER).any()
    assert {int(s) // R.CH for s in used} == {c for c in R.CHUNKS if c < 64 * MW}
    rows = [[int(s) for s in a[:, t] if s != R.NEVER] for t in range(256)]
    want = R.dirty_ref(pre, rows)
    for t in range(256):  # second formulation: bit by bit on the words
        w = pre[t].copy()
        for s in rows[t]:
            c = s // R.CH
            w[c // 64] |= np.uint64(1 << (c % 64))
        assert w.tolist() == want[t].tolist()
    a, pre = R.dirty_wave_case(MW)
    s, wr = a[0].reshape(8, 64), a[1].reshape(8, 64) != 0
    assert (s < lim).all() and pre.shape == (8, MW)
    assert len({int(x) // R.CH for x in s[0]}) == 3 and wr[0].all(), "a wave whose lanes span three chunks"
    assert not wr[1, 0] and wr[1, 1:].all(), "lane 0 has wr = false"
    assert int(s[1, 0]) // R.CH not in {int(x) // R.CH for x in s[1, 1:]}, "and its chunk is nobody else's"
    assert not wr[2].any() and len({int(x) // R.CH for x in s[3]}) == 1 and wr[5].tolist() == [False] * 63 + [True]
    assert len({int(x) // R.CH for x in s[4]}) == 64
    assert {int(x) // R.CH for x in s[wr]} >= {c for c in R.CHUNKS if c < 64 * MW}


def test_window_inputs_and_refs():
    for g in R.GOSSIP_TS:
        x = R.div_gt_inputs(g)
        assert {0, 1, g - 1, g, g + 1, 2**31 - 1, 2**31, 2**32 - g, 2**32 - 1} <= set(x.tolist()) and len(x) > 10000
        q = R.div_gt_ref(x, g).astype(np.uint64)
        r = x.astype(np.uint64) - q * np.uint64(g)
        assert (r < g).all() and (q * np.uint64(g) + r == x).all()
    rows = R.s16_cases()
    e, ref, c = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int64)
    assert ((c <= ref) & (ref < c + 8192) & (ref < 2**32)).all() and ((e & R.S16_TICK) == (c & R.S16_TICK)).all()
    assert (e >> 13).max() > 0 and {0, 1, 8191, 8192, 8193, 2**29, 2**32 - 8193} <= set(c.tolist())
    assert (ref - c).max() == 8191 and (ref - c).min() == 0
    for ee, rr, cc in rows[::97].tolist():  # naive: search downwards from ref for the stored low bits
        t = rr
        while t & R.S16_TICK != ee & R.S16_TICK:
            t -= 1
        assert t == cc
    rows = R.rg_cases()
    g, infp, P = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int64)
    assert ((infp <= P) & (infp >= P - 500) & (infp >= 0)).all() and (g <= R.RG_SLOT).all()
    assert {0, 1, 511, 512, 1023, 1024, 2**32 - 1} <= set(P.tolist()) and {0, R.RG_SLOT} <= set(g.tolist())
    for PP in set(P.tolist()):  # every infp of the window
        assert sorted(infp[P == PP].tolist()) == list(range(max(0, PP - 500), PP + 1))
    k = R.u32(R.KEY8_KEYS)
    assert set(range(0x200)) | {2**32 - 1} == set(k.tolist())
    s = R.key8_ref(k)
    assert s[:0xFF].tolist() == list(range(0xFF)) and set(s[0xFF:].tolist()) == {0xFF}


def test_table_inputs_and_refs():
    cases = R.delay_cases()
    assert [len(t) for _, t, _ in cases] == [0, 1, 2, 255, 256] and all(di < 16 for di, _, _ in cases)
    for di, thr, x in cases:
        assert (np.diff(thr.astype(np.int64)) >= 0).all()
        if len(thr) >= 2:
            assert (np.diff(thr.astype(np.int64)) == 0).any(), "repeated thresholds"
        for t in thr.tolist():
            assert {t - 1, t, t + 1} <= set(x.tolist())
        want = [sum(1 for t in thr.tolist() if t <= xx) for xx in x.tolist()]
        assert R.delay_ref(thr, x).tolist() == want
    cases = R.epoch_cases()
    assert any(len([f for f in t if f != R.NEVER]) != len(set(f for f in t.tolist() if f != R.NEVER)) for t, _ in cases)
    assert any(t[i] == R.NEVER and (t[:i] != R.NEVER).any() and (t[i + 1:] != R.NEVER).any()
               for t, _ in cases for i in range(8)), "unused entries in the middle"
    for tab, k in cases:
        assert len(tab) == R.MAX_EPOCHS and 2**32 - 2 in k.tolist()
        got = R.epoch_ref(tab, k)
        for kk, gg in zip(k.tolist(), got.tolist()):
            best, bf = -1, 0
            for e in range(8):  # a scan that keeps the latest start, a later index replacing an equal one
                f = int(tab[e])
                if f != R.NEVER and f <= kk and (best < 0 or f >= bf):
                    best, bf = e, f
            assert gg == best
        if (tab != R.NEVER).any() and int(tab.min()) > 0:
            assert -1 in got.tolist(), "k before every epoch"
    assert R.epoch_ref(R.u32([7, 7, 7] + [R.NEVER] * 5), [7]).tolist() == [2]


def test_paykey_inputs_and_ref():
    cases = R.paykey_cases()
    assert sorted({mw for mw, _, _ in cases}) == [1, 2, 3]
    seen = {}
    for MW, mask, subs in cases:
        NS, base, ship = R.paykey_input(MW, mask)
        m = R.mask_int(mask)
        assert len(mask) == MW and NS == MW * 64 * R.CH and (subs < NS).all()
        assert ship.shape == (bin(m).count("1"), R.CH) and len(base) == NS
        assert (ship >= 0x80000000).all() and (base < 0x80000000).all(), "base_row is distinct from any shipped word"
        assert len(np.unique(ship)) == ship.size
        want = R.paykey_ref(mask, subs)
        # second formulation: lay the shipped chunks out as a full row and index it
        row = base.copy()
        r = 0
        for c in range(64 * MW):
            if (int(mask[c // 64]) >> (c % 64)) & 1:
                row[c * R.CH:(c + 1) * R.CH] = ship[r]
                r += 1
        assert np.array_equal(want, row[subs])
        for s in subs.tolist():
            seen.setdefault((MW, s // R.CH), set()).add((m >> (s // R.CH)) & 1)
    for MW in (1, 2, 3):
        for c in R.CHUNKS:
            if c < 64 * MW:
                assert seen[(MW, c)] == {0, 1}, "every edge chunk both shipped and not"


def test_feistel_ref():
    def fmix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & M32
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & M32
        return h ^ (h >> 16)

    for n in (1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1000):
        for keys in R.FEISTEL_KEYS:
            got = R.feistel_ref(n, keys)
            assert sorted(got.tolist()) == list(range(n))
            b = 2
            while 2**b < n:
                b += 2
            h, mask = b // 2, 2**(b // 2) - 1
            for x in range(n):  # scalar Python
                y = x
                while True:
                    L, Rr = y >> h, y & mask
                    for k in keys:
                        L, Rr = Rr, L ^ (fmix(Rr ^ k) & mask)
                    y = (L << h) | Rr
                    if y < n:
                        break
                assert y == int(got[x])
    assert sorted(R.feistel_ref(65537, R.FEISTEL_KEYS[0]).tolist()) == list(range(65537))
    assert max(R.FEISTEL_NS) == 2**20 and {4**k + d for k in (1, 2, 4, 8) for d in (-1, 0, 1)} <= set(R.FEISTEL_NS)


@pytest.mark.parametrize("B,B2", [(64, 128), (64, 64)])
def test_ring_inputs_and_ref(B, B2):
    rg, h, t = R.ring_case(B, B2)
    d = (t.astype(np.int64) - h.astype(np.int64)) % 2**32
    assert sorted(set(d.tolist())) == [0, 1, 17, B] and sorted(set(h.tolist())) == [0, 5, 2**32 - 3]
    assert len(h) == 12 and (t < h).any(), "positions that wrap past 2^32"
    assert not (rg == R.RING_SENTINEL).any()
    want = R.ring_ref(rg, h, t, B2)
    for m in range(len(h)):
        held = [(int(h[m]) + i) % 2**32 for i in range(int(d[m]))]
        assert (want[m] != R.RING_SENTINEL).sum() == len(held)
        for p in held:
            assert want[m, p & (B2 - 1)] == rg[m, p & (B - 1)]


# ---------------------------------------------------------------------------------------------- SYNC diff and lister
def naive_diff(p, r):
    """Subject by subject, in Python integers."""
    segs, absent = [[] for _ in range(-(-len(p) // R.MCH))], False
    for s, (a, b) in enumerate(zip(p.tolist(), r.tolist())):
        if a & 3 == 0:
            absent |= b & 3 != 0
        elif a != b:
            segs[s // R.MCH].append((s << 34) | (a & 3) << 32 | a >> 2)
    return segs, absent


def test_sync_diff_sizes():
    want = {1000: (1000, 1008, 1, 1, 1, 1), 1025: (1032, 1040, 1, 2, 1, 1), 2048: (2048, 2048, 1, 2, 1, 1),
            2049: (2056, 2064, 2, 3, 1, 1), 2056: (2056, 2064, 2, 3, 1, 1), 8192: (8192, 8192, 4, 8, 1, 1),
            8200: (8200, 8208, 5, 9, 1, 2), 131080: (131080, 131088, 65, 129, 2, 17), 262152: (262152, 262160, 129, 257, 3, 33)}
    assert sorted(want) == R.SD_NS
    for N, w in want.items():
        z = R.sd_sizes(N)
        assert (z["NS"], z["NS8"], z["NCHUNK"], z["NMETA"], z["MW"], z["nit"]) == w, N
    assert R.sd_sizes(3 * 64 * R.CH)["MW"] == 3 and R.sd_sizes(3 * 64 * R.CH + 1)["MW"] == 4, "three mask words: 393 216"


def test_sync_diff_ref_against_a_subject_loop():
    rng = np.random.default_rng(1)
    for n in (1, 7, 1024, 1025, 2100):
        p = R.u32(rng.integers(0, 2**32, n))
        r = p.copy()
        ch = rng.random(n) < 0.3
        r[ch] = rng.integers(0, 2**32, int(ch.sum()))
        p[rng.random(n) < 0.1] &= ~np.uint32(3)  # absent in the payload: whatever the incarnation bits say
        r[rng.random(n) < 0.1] = 0
        for a, b in ((p, r), (r, p), (p, p)):
            segs, ab = R.sync_diff_ref(a, b)
            want, wab = naive_diff(a, b)
            assert [w.tolist() for w in segs] == want and ab == wab, n
    segs, ab = R.sync_diff_ref(R.u32([0x401, 0xFF, 0x3FC]), R.u32([0x402, 0x1FF, 0]))
    assert segs[0].tolist() == [1 << 32 | 0x100, 1 << 34 | 3 << 32 | 0x3F] and not ab, "the third is absent in both"
    assert int(R.key34(0xFFFFFFFF)) == 3 << 32 | 0x3FFFFFFF


def test_rx_payload_overlays_the_shipped_chunks_by_mask():
    for MW, mask, subs in R.paykey_cases():
        NS, base, ship = R.paykey_input(MW, mask)
        pay = R.rx_payload(base, R.mask_int(mask), ship)
        assert np.array_equal(pay[subs], R.paykey_ref(mask, subs)), "the same answers as payload_key_at's reference"
    base = np.arange(2 * R.CH + 8, dtype=np.uint32)  # a partial last chunk
    pay = R.rx_payload(base, 0b101, [np.full(R.CH, 7, np.uint32), np.full(R.CH, 9, np.uint32)])
    assert (pay[:R.CH] == 7).all() and np.array_equal(pay[R.CH:2 * R.CH], base[R.CH:2 * R.CH]) and (pay[2 * R.CH:] == 9).all()


def sd_cases():
    import test_gpu_sync_diff as G  # the GPU tests' case builders (importing it touches no GPU)
    return G


def test_sync_diff_cases_meet_their_preconditions():
    G = sd_cases()
    for N in R.SD_NS:
        z = R.sd_sizes(N)
        rows = G.rows_for(N)
        assert rows.shape == (8, z["NS"]) and (rows[:, N:] == 0).all(), "padding keys are absent"
        assert ((rows[0, :N] & 3) != 0).all() and (rows[0, :N] < 0xFF).all() and ((rows[2] & 3) == 0).all()
        d = np.flatnonzero(rows[1] != rows[0]).tolist()
        assert d == sorted({s for s in G.EDGE_SUBJECTS + [N - 1] if s < N})
        for r, lo, hi in ((3, 0.003, 0.02), (4, 0.4, 0.6)):
            assert lo < (rows[r, :N] != rows[0, :N]).mean() < hi
        big5, big6 = rows[5, :N] >= 0xFF, rows[6, :N] >= 0xFF
        if N >= 2048:
            assert (big5 & ~big6).any() and (big6 & ~big5).any(), "an escaped key in the payload only, the receiver only"
            assert (big5 & big6 & (rows[5, :N] == rows[6, :N])).any() and (big5 & big6 & (rows[5, :N] != rows[6, :N])).any()
            both = np.flatnonzero(big5 & big6 & (rows[5, :N] != rows[6, :N]))
            assert (both % 32 == 0).any() and (both % 32 == 31).any(), "at a lane's first and last subject"
            lanes5 = set((np.flatnonzero(big5 | big6) // 32).tolist())
            small = np.flatnonzero((rows[5, :N] != rows[6, :N]) & ~big5 & ~big6) // 32
            assert any(l not in lanes5 and (l - 1 in lanes5 or l + 1 in lanes5) for l in small.tolist()), \
                "a lane that differs on shadows only next to an escaped one"
        st = (rows[5, :N] != rows[0, :N]) & (rows[5, :N] >> 2 == rows[0, :N] >> 2)
        assert st.any() and ((rows[5, :N][st] & 3) != 0).all(), "only the status bits differ"
        assert ((rows[7, :N] == 0) & (rows[0, :N] != 0)).any()
        odd = np.flatnonzero((rows[2] >= 0xFF) & (rows[7] == 0))  # an escape in the receiver only, both records absent
        assert len(odd) == 2 and not (rows[7].reshape(-1, 8)[odd // 8] >= 0xFF).any() and not R.sync_diff_ref(rows[7], rows[2])[1]
        case = G.listed_case(N)
        exp, _ = R.sd_expect(case, case["narrow"], case["wide"])
        total = sum(len(w) for e in exp for w in e["segs"].values())
        assert 0 < total <= case["POOLCAP"] <= 2**22
        assert any(e["absent"] for e in exp) and not all(e["absent"] for e in exp)
        assert {w for *_, w in case["wide"]} >= {R.NEVER, R.DESC_DEFER, R.DESC_PIN | 0, 3}, "every kind of wide payload"
        assert len({(i, w >> 4) for i, _, _, w in case["narrow"]}) == len(case["narrow"]) == 10 * z["nit"]
        params, inp, out = R.sd_pack(case)
        assert len(params) == 15 and inp.dtype == out.dtype == np.uint32 and len(inp) % 2 == 0


def test_ack_resolve_ref_and_its_cases():
    G = sd_cases()
    seen = set()
    for N in (2049, 8200):
        for q in range(0, len(G.LOG_LENGTHS), 4):
            specs = [dict(tln=a, n0=b, n1=c, where=("one", "ends")[(q + j) % 2]) for j, (a, b, c) in enumerate(G.LOG_LENGTHS[q:q + 4])]
            case = G.log_case(N, 6 + q % 3, specs, 300 + q + N)
            for m, sp, v in zip(case["msgs"], specs, R.ack_resolve_ref(case)):
                subs = R.sd_log_subjects(case, m)
                p, r = R.sd_payload(case, m), case["rows"][m["dst"]]
                assert v["how"] == "resolved" and len(subs) <= sp["tln"] + sp["n0"] + sp["n1"] <= 3 * R.TL
                assert set(np.flatnonzero(p != r).tolist()) <= set(subs), "resolvable: the rows differ only in logged subjects"
                # second formulation: the full diff, which then holds only logged subjects
                segs, _ = R.sync_diff_ref(p, r)
                assert np.concatenate(segs).tolist() == v["cand"]
                seen.add((sp["tln"], sp["n0"], sp["n1"], len(subs) < sp["tln"] + sp["n0"] + sp["n1"]))
    assert {s[:3] for s in seen} == set(G.LOG_LENGTHS) and (R.TL, R.TL, R.TL, True) in seen, "with duplicates across the logs"
    # a stale tick empties that log; the conditions that leave a message to the diff
    case = G.log_case(8200, 9, [dict(tln=4, n0=5, n1=6, stale=0), dict(tln=4, n0=5, n1=6, stale=1)], 3)
    n = [len(R.sd_log_subjects(case, m)) for m in case["msgs"]]
    assert n[0] <= 4 + 6 and n[1] <= 4 + 5
    for sp in (dict(tln=R.TL + 1, n0=0, n1=0), dict(tln=0, n0=R.TL + 1, n1=0), dict(tln=0, n0=0, n1=R.TL + 1),
               dict(tln=1, n0=1, n1=1, kind=2), dict(tln=1, n0=1, n1=1, defer=True), dict(tln=1, n0=1, n1=1, pin=True)):
        case = G.log_case(8200, 9, [sp], 4)
        assert R.sd_log_subjects(case, case["msgs"][0]) is None, sp
    assert R.sd_log_subjects(G.log_case(8200, 1, [dict(tln=1, n0=0, n1=1)], 5), dict(R.sd_msg(1, 0, kind=R.KF_RES, tln=1))) is None


def test_mask_and_pin_cases():
    G = sd_cases()
    for N in (2049, 8200, 131080, 262152):
        z = R.sd_sizes(N)
        case = G.mask_case(N, 40 + N)
        base = G.rows_for(N)[0]
        words = set()
        for r in range(8):
            m = R.mask_int(case["dirty"][r])
            assert m < 1 << z["NCHUNK"]
            words |= {c >> 6 for c in range(z["NCHUNK"]) if (m >> c) & 1}
            for c in range(z["NCHUNK"]):
                same = np.array_equal(case["rows"][r, c * R.CH:(c + 1) * R.CH], base[c * R.CH:(c + 1) * R.CH])
                assert same or (m >> c) & 1, "a clean chunk equals the baseline's (a dirty one may, too)"
        assert words == set(range(z["MW"])), "dirty bits in every mask word"
        ref = R.ack_resolve_ref(case)
        only_src = only_dst = 0
        for m, v in zip(case["msgs"], ref):
            ms, md = R.mask_int(case["dirty"][m["src"]]), R.mask_int(case["dirty"][m["dst"]])
            assert (v["how"] == "decided") == (ms | md == 0)
            if v["how"] == "narrow":  # second formulation: the union mask cut into items
                assert v["items"] == {t: ((ms | md) >> (4 * t)) & 15 for t in range(z["nit"]) if ((ms | md) >> (4 * t)) & 15}
                only_src += md == 0
                only_dst += ms == 0
            p, r = R.sd_payload(case, m), case["rows"][m["dst"]]
            for c in np.unique(np.flatnonzero(p != r) // R.CH).tolist():
                assert ((ms | md) >> c) & 1, "the rows differ only in chunks the lister has streamed"
        assert only_src and only_dst
        for variant in G.PIN_VARIANTS:
            for L in (1, 2, 8, 9):
                case = G.pin_case(N, L, variant)
                hows = [v["how"] for v in R.ack_resolve_ref(case)]
                lst = R.inbound_list(case, 0)
                assert len(lst) == (L - 1 if variant == "not-on-the-list" else L)
                if variant == "clean":
                    assert hows == (["pin"] * L if L <= R.PINWALK else ["wide"] * L)
                elif variant == "not-on-the-list":
                    assert hows == ["pin"] * (L - 1) + ["wide"]
                else:
                    assert "pin" not in hows
                if variant.startswith("dirty"):
                    assert [w for r in range(8) for w in range(3) if case["dirty"][r][w]] == [z["MW"] - 1]


# ------------------------------------------------------------------------------------- row-shard exchange codec
import re
import struct
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "scalecube-cluster_amd" / "csrc"
XP = R.xpack_cases()
XU = R.xunpack_cases()


def test_sync_entry_size_against_engine_h():
    """The references' SyncMsg is engine.h's, field for field, and an entry is SyncMsg + 8 + 8 MW + 4 TL bytes: a change
    of the struct breaks this test, not the meaning of the others."""
    text = (CSRC / "engine.h").read_text()
    body = re.search(r"struct SyncMsg \{(.*?)\n\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    fields = [f.strip() for decl in re.findall(r"uint32_t ([^;]+);", body) for f in decl.split(",")]
    assert tuple(fields) == R.SM_FIELDS and 4 * R.SMW == 52
    assert re.search(r"sync_entry_size\(uint32_t MW\) \{ return sizeof\(SyncMsg\) \+ 8 \+ 8ull \* MW \+ 4ull \* TL; \}", text)
    assert re.search(r"constexpr uint32_t TL = 16;", text) and R.TL == 16
    assert re.search(r"RRW = 12;", text) and re.search(r"NSW = 8;", text) and (R.NSW, R.RRW) == (8, 12)
    assert [R.sync_entry_size(MW) for MW in (1, 2, 3)] == [132, 140, 148]
    for name, v in (("XFLAG_GOSSIP", 62), ("XFLAG_OVER", 61)):
        assert re.search(rf"{name} = 1ull << {v}", text) and getattr(R, name) == 1 << v
    assert re.search(r"E_MSGS = 32,", text) and re.search(r"E_XCAP = 1u << 17", text) and re.search(r"PAY_RX = 0x40000000u", text)


def test_shard_routing_refs_agree_with_shard_range():
    from swimhip.shard import shard_range
    for n, w in [(64, 2), (300, 3), (100_000, 8), (50, 7), (131073, 8), (5, 2), (5, 3), (2049, 3), (4100, 2)]:
        for r in range(w):
            lo, hi = shard_range(n, w, r)
            assert (R.shard_lo(n, w, r), R.shard_lo(n, w, r + 1)) == (lo, hi)
            for m in {lo, hi - 1, (lo + hi) // 2} if hi > lo else ():
                assert R.shard_of(n, w, m) == r, (n, w, m)


def naive_region(buf, MW):
    """A header walk with struct.unpack, nothing shared with xpack_ref: (header, slot records, round records, entries =
    [(13 message words, base, pad, mask words, 16 log words)], the byte where the entries end)."""
    H = struct.unpack_from("<8I", buf, 0)
    o = 32
    ns = [struct.unpack_from("<8I", buf, o + 32 * i) for i in range(H[0])]
    o += 32 * H[0]
    rr = [struct.unpack_from("<12I", buf, o + 48 * i) for i in range(H[1])]
    o += 48 * H[1]
    ent = []
    for _ in range(H[2]):
        msg = struct.unpack_from("<13I", buf, o)
        base, pad = struct.unpack_from("<2I", buf, o + 52)
        mask = struct.unpack_from(f"<{MW}Q", buf, o + 60)
        log = struct.unpack_from("<16I", buf, o + 60 + 8 * MW)
        ent.append((msg, base, pad, mask, log))
        o += 60 + 8 * MW + 64
    return H, ns, rr, ent, o


@pytest.mark.parametrize("name", list(XP))
def test_xpack_ref_parses_back(name):
    c = XP[name]
    ref, z = R.xpack_ref(c), R.sd_sizes(c["N"])
    N, W, rank, MW = c["N"], c["W"], c["rank"], z["MW"]
    lo = R.shard_lo(N, W, rank)
    if c["flags"] & R.XP_HALTED:
        assert all((ref[f].view(np.uint8) == R.XP_BYTE).all() for f in ("xa_send", "xa_scnt", "xi_send", "mtmp", "mlog"))
        return
    sent = [m for m in c["msgs"][:c["MSGCAP"]]]
    for q in range(W):
        if q == rank:
            assert (ref["xa_send"][q] == R.XP_BYTE).all()
            continue
        buf = ref["xa_send"][q].tobytes()
        H, ns, rr, ent, end = naive_region(buf, MW)
        bytes_ = int(ref["xa_scnt"][q]) & R.XCNT_MASK
        assert bool(int(ref["xa_scnt"][q]) & R.XFLAG_GOSSIP) == (c["used"] > 0)
        want = [m for m in sent if lo_hi(N, W, q)[0] <= m["dst"] < lo_hi(N, W, q)[1]]
        if not ref["regions"][q]["fits"]:
            assert H == (0, 0, 0, 0, 256, 0, 0, 0) and bytes_ == 32 and set(buf[32:]) == {R.XP_BYTE}
            continue
        assert H[5:] == (0, 0, 0) and H[4] % 256 == 0 and end <= H[4] < end + 256 and bytes_ == H[4] + H[3] * R.CH * 4 <= c["XA_PEER"]
        assert [list(r) for r in ns] == np.asarray(c["ns_rec"])[:H[0]].tolist() and H[0] == min(c["xn0"], c["NSCAP"])
        assert [list(r) for r in rr] == np.asarray(c["rr_rec"])[:H[1]].tolist() and H[1] == min(c["xn1"], c["RRCAP"])
        assert len(ent) == len(want)
        nxt = 0
        for (msg, base, pad, mask, log), m in zip(ent, want):
            assert list(msg) == [m[f] for f in R.SM_FIELDS] and pad == 0 and base == nxt
            row = c["rows"][m["src"] - lo] if m["payload"] == R.NEVER else c["arena"][m["payload"]]
            dirty = c["rdirty"][m["src"] - lo] if m["payload"] == R.NEVER else c["arena_dirty"][m["payload"]]
            assert R.mask_int(mask) == dirty
            nlog = m["tln"] if c["flags"] & R.XP_ACKRES and m["kind"] & R.KF_RES and m["tln"] <= R.TL else 0
            assert list(log[:nlog]) == c["tlog"][m["src"] - lo][:nlog].tolist() and set(log[nlog:]) <= {R.XP_WORD}
            for ch in range(z["NCHUNK"]):
                if (dirty >> ch) & 1:
                    n = min(R.CH, z["NS"] - ch * R.CH)
                    got = struct.unpack_from(f"<{R.CH}I", buf, H[4] + nxt * R.CH * 4)
                    assert list(got[:n]) == row[ch * R.CH:ch * R.CH + n].tolist() and set(got[n:]) <= {R.XP_WORD}
                    nxt += 1
        assert nxt == H[3] and set(buf[end:H[4]]) <= {R.XP_BYTE} and set(buf[bytes_:]) <= {R.XP_BYTE}


def lo_hi(N, W, q):
    return q * N // W, (q + 1) * N // W


def test_xpack_cases_reach_their_edges():
    sh = {n: R.xp_shape(c) for n, c in XP.items()}
    z = lambda n: R.sd_sizes(XP[n]["N"])
    assert z("n5-w2")["NS"] == 8 and z("n5-w2")["NCHUNK"] == 1 and sh["n5-w2"]["bytes"] == {1: 256 + 8192}
    assert [R.shard_of(5, 2, m["dst"]) for m in XP["n5-w2"]["msgs"]] == [0, 1, 0]
    assert z("n2049-w3-r1")["NS"] == 2056 and z("n2049-w3-r1")["NCHUNK"] == 2
    c = XP["n2049-w3-r1"]
    masks = {R.xp_payload(c, m)[1] for m in c["msgs"]}
    assert masks == {0, 1, 2, 3} and {m["payload"] for m in c["msgs"]} == {R.NEVER, 0, 1}
    assert [int(r[1]) for r in c["rr_rec"]] == [0, 1, 8] and len(c["ns_rec"]) == 3
    c = XP["n4100-batches"]
    dests = [R.shard_of(4100, 2, m["dst"]) for m in c["msgs"]]
    assert dests.count(1) == 600 and dests.count(0) == 300 and sh["n4100-batches"]["batches"] >= 3 and z("n4100-batches")["NCHUNK"] == 3
    assert all(dests[i] == 1 and R.xp_payload(c, c["msgs"][i])[1] for i in (255, 256, 257, 511, 512))
    assert sum(sh["n4100-batches"]["per_block"][1]) > 16 and min(sh["n4100-batches"]["per_block"][1]) >= 1
    c = XP["n131073-w8-r3"]
    assert sh["n131073-w8-r3"]["MW"] == 2 and z("n131073-w8-r3")["NCHUNK"] == 65 and len(c["rows"]) == 4
    assert {ch for m in c["msgs"] for ch in R.mask_chunks(R.xp_payload(c, m)[1])} == {0, 63, 64}
    assert sh["n131073-w8-r3"]["bytes"][5] == 256 and set(sh["n131073-w8-r3"]["bytes"]) == {0, 1, 2, 4, 5, 6, 7}
    assert all(v > 256 for q, v in sh["n131073-w8-r3"]["bytes"].items() if q != 5)
    for XI, rel in ((272, -16), (264, -8), (256, 0), (248, 8)):
        assert sh[f"inl-xi{XI}"]["bytes"] == {1: 256} and 256 - XI == rel
    assert XP["inl-xi64"]["XI"] == 64 and not XP["inl-off"]["flags"] & R.XP_INLINE
    c = XP["inl-one-over"]
    assert sh["inl-one-over"]["bytes"] == {1: c["XI"] - 8, 2: c["XI"] - 8 + 8192}
    for n, q in (("ovf-rqcap", 0), ("ovf-chcap", 0), ("ovf-xa-peer", 0)):
        assert sh[n]["fits"] == {0: False, 2: True} and sh[n]["err"] == R.E_XCAP, n
    c = XP["ovf-rqcap"]
    assert c["RQCAP"] == 2 and sum(R.shard_of(2049, 3, m["dst"]) == 0 for m in c["msgs"]) == 3
    c = XP["ovf-chcap"]
    assert c["CHCAP"] == 1 and bin(R.xp_payload(c, c["msgs"][0])[1]).count("1") == 2
    c = XP["ovf-xa-peer"]
    assert c["XA_PEER"] == 256 + 2 * 8192 - 8192 and sh["ovf-xa-peer"]["bytes"][2] == c["XA_PEER"]
    c = XP["ovf-msgcap"]
    assert c["MSGCAP"] == 4 and c["xn4"] + sum(R.shard_of(5, 2, m["dst"]) == 0 for m in c["msgs"]) == 6 and sh["ovf-msgcap"]["err"] == R.E_MSGS
    c = XP["ackres-on"]
    assert sorted({m["tln"] for m in c["msgs"] if m["kind"] & R.KF_RES}) == [0, 1, 16, 17]
    assert XP["ackres-off"]["msgs"] == c["msgs"] and not XP["ackres-off"]["flags"] & R.XP_ACKRES


def test_xpack_masks_are_consistent_with_the_rows():
    """A mask bit is set if the chunk differs from the baseline (and on some equal chunks, which is allowed); a clear bit
    means equal: what the payload closure rests on."""
    extra = 0
    for c in XP.values():
        z = R.sd_sizes(c["N"])
        assert not c["base"][c["N"]:].any()
        for row, mask in list(zip(c["rows"], c["rdirty"])) + list(zip(c["arena"], c["arena_dirty"])):
            for ch in range(z["NCHUNK"]):
                differs = not np.array_equal(row[ch * R.CH:(ch + 1) * R.CH], c["base"][ch * R.CH:(ch + 1) * R.CH])
                assert not differs or (mask >> ch) & 1
                extra += (mask >> ch) & 1 and not differs
            assert mask >> z["NCHUNK"] == 0
    assert extra > 0


@pytest.mark.parametrize("name", list(XU))
def test_xunpack_ref_round_trip(name):
    """xunpack_ref(xpack_ref(case)) satisfies the order-free properties (messages, lists, pins, payload closure)."""
    c = XU[name]
    r = R.xunpack_ref(c)
    b = c["k"] & 1
    if c["flags"] & R.XU_SPEC and (c["flags"] & R.XU_HALTED or R.xu_gate(c)):
        assert r["sc"][f"nmsg{b}"] == R.XP_WORD and (r["msgs"] == R.XP_WORD).all() and (r["m_head"] == R.NEVER).all()
        assert r["sc"]["halt"] == (1 if c["flags"] & R.XU_HALTED else c["k"] + 1)
        return
    R.xu_props(c, r, holes={"ovf-rxcap": 100}.get(name, 0))
    # the reference's own parse agrees with what the case expects, entry for entry
    ent = [e for p in range(c["W"]) for e in (R.xu_region(c, p) or ((), (), (), 0))[2]]
    assert len(ent) == len(c["entries"])
    for (mw, base, mask, logw), e in zip(ent, c["entries"]):
        assert mw.tolist() == R.msg_words(e["msg"]).tolist() and mask == e["mask"]


def test_xunpack_cases_reach_their_edges():
    assert {XU[n]["W"] for n in XU} == {2, 3, 8}
    c = XU["two-peers-300"]
    assert len(c["senders"]) == 2 and all(len(s["msgs"]) == 300 for s in c["senders"].values()) and len(c["local"]) == 20
    assert len(c["entries"]) == 600 and XU["ovf-msgcap"]["MSGCAP"] < 620 <= XU["ovf-msgcap"]["RXCAP"] + 20
    assert XU["ovf-rxcap"]["RXCAP"] < 600 and XU["ovf-rxcap"]["MSGCAP"] >= 620
    r = R.xunpack_ref(XU["pins"])
    F = {f: i for i, f in enumerate(R.SM_FIELDS)}
    pinned = {int(w[F["seq"]]) for w in r["msgs"][:r["sc"]["nmsg1"]] if int(w[F["pin"]]) != R.NEVER}
    assert pinned == {1000 + 6000, 1000 + 6003, 1000 + 6004} and r["sc"]["arena1"] == 3
    per_dst = {}
    for w in r["msgs"][:r["sc"]["nmsg1"]]:
        if int(w[F["payload"]]) == R.NEVER and not int(w[F["kind"]]) & R.KF_DEFER:
            per_dst[int(w[F["dst"]])] = per_dst.get(int(w[F["dst"]]), 0) + 1
    assert max(per_dst.values()) <= 2, "at most two live rows per receiver: no arena row is lost to a pin race"
    e = XU["edges"]
    assert int(e["rcnt"][2]) == 24 and int(e["rcnt"][0]) >= 32 and e["rank"] == 0
    g = XU["gossip-w8"]
    origins = [int(r_[7]) for s in g["senders"].values() for r_ in s["ns_rec"]]
    assert len(origins) == 14 and len(set(origins)) == 7, "two creations per origin"
    rr = XU["n2049>0"]["senders"][1]["rr_rec"]
    st = XU["n2049>0"]["gossip"]
    changed = [int(st["log_pos"][int(r_[0])]) > 0 and int(st["log_spread"][int(r_[0])][(int(st["log_pos"][int(r_[0])]) - 1) % 2]) != int(r_[2]) for r_ in rr]
    assert changed == [False, True, False] and [int(st["log_pos"][int(r_[0])]) for r_ in rr] == [3, 4, 0]
    assert R.xu_gate(XU["spec-sent-past-inline"]) and not R.xu_gate(XU["spec-sent-at-inline"]) and not R.xu_gate(XU["spec-runs"])
    assert XU["inline-in-256"]["XI"] - 8 == 256 == int(XU["inline-in-256"]["rcnt"][0]) & R.XCNT_MASK


def test_pack_b_and_inline_in_refs():
    xd = np.arange(100, dtype=np.uint64) + np.uint64(1 << 40)
    send, scnt, err = R.pack_b_ref(3, 1, 16, 40, 16 + 8 * 16, xd)
    assert err == 0 and scnt.tolist() == [144, R.XP_WORD64, 144] and struct.unpack_from("<4I", send[0].tobytes()) == (16, 0, 0, 0)
    assert struct.unpack_from("<16Q", send[2].tobytes(), 16) == tuple(int(v) for v in xd[:16]) and (send[1] == R.XP_BYTE).all()
    send, scnt, err = R.pack_b_ref(3, 1, 16, 16, 16 + 8 * 15, xd)
    assert err == R.E_XCAP and scnt[0] == 16 and (send[0][16:] == R.XP_BYTE).all()
    irecv = np.zeros((2, 64), np.uint8)
    irecv[:, 8:] = np.arange(56, dtype=np.uint8)
    irecv[0][:8] = np.array([24 | R.XFLAG_OVER], np.uint64).view(np.uint8)
    irecv[1][:8] = np.array([4096], np.uint64).view(np.uint8)
    recv, rcnt, host = R.inline_in_ref(2, 64, 128, irecv, np.array([7, 9], np.uint64), False)
    assert recv[0][:24].tolist() == list(range(24)) and (recv[0][24:] == R.XP_BYTE).all()
    assert recv[1][:56].tolist() == list(range(56)) and (recv[1][56:] == R.XP_BYTE).all()
    assert rcnt.tolist() == [24 | R.XFLAG_OVER, 4096] and host.tolist() == [7, 9, 24 | R.XFLAG_OVER, 4096]


def test_exchange_calls_are_well_formed():
    """The buffers handed to the library: 8-byte aligned, the output preset to the sentinel and of the size the parts add
    up to (xp_unpack / xu_unpack consume it exactly)."""
    for c in XP.values():
        params, inp, out = R.xp_pack(c)
        assert len(params) == 22 and inp.ctypes.data % 8 == 0 and out.ctypes.data % 8 == 0 and (out == R.XP_BYTE).all()
        assert R.xp_unpack(c, out)["err"] == R.XP_WORD
    for c in XU.values():
        params, inp, out = R.xu_pack(c)
        assert len(params) == 18 and inp.ctypes.data % 8 == 0 and out.ctypes.data % 8 == 0 and (out == R.XP_BYTE).all()
        assert R.xu_unpack(c, out)["sc"]["err"] == R.XP_WORD


# ---------------------------------------------------------------------------------------------- gossip data plane
GS = R.gs_cases()


def test_gs_period_is_the_nearest_period_with_that_tag():
    for P in (0, 5, 511, 512, 1023, 1024, 1030, 3071, 10**6):
        for tag in range(1024):
            near = [p for p in range(P - 512, P + 512) if p & 1023 == tag]
            assert near == [R.gs_period(tag, P)], (P, tag)


@pytest.mark.parametrize("name", list(GS))
def test_gs_case_meets_the_engine_invariants(name):
    assert R.gs_invariants(GS[name]) == [], name


@pytest.mark.parametrize("name", list(GS))
def test_gs_round_reference_against_the_range_formulation(name):
    """Classifying every ring entry on its own against searching the sorted periods for the two boundaries."""
    c = GS[name]
    listed = 0
    for m in range(c["N"]):
        a, b = R.gs_round_ref(c, m), R.gs_round_ref_ranges(c, m)
        assert a == b, (name, m)
        listed += a is not None
    if name.startswith(("rounds_edges", "rounds_sweeps", "send_", "contacts")):
        assert listed, name


def test_gs_round_cases_hold_the_boundaries_they_name():
    c = R.gs_rounds_edges()
    assert R.gs_round_ref(c, c["idle"]) is None and R.gs_ref(c)["dead_tick"][c["leaver"]] == c["k"] + 1
    for m in range(5):  # an entry at, one below and one above both boundaries
        P, sp = int(c["tperiod"][m]), int(c["tspread"][m])
        per = {p for _, _, p in R.gs_ring(c, m)}
        want = {P - 2 * (sp + 1) + d for d in (-1, 0, 1)} | {P - sp + d for d in (-1, 0, 1)}
        assert {p for p in want if p >= 0} <= per, (m, sorted(per))
    tags = lambda m: {int(e) >> 22 for e in c["rg"][m] if e != R.GS_SENT}
    assert any({1023, 0} <= tags(m) for m in range(5)), "a ring with entries on both sides of the tag wrap"
    assert any(int(c["rhead"][m]) > int(c["rtail"][m]) for m in range(c["N"])), "a ring across 2^32"
    assert any(int(c["rhead"][m]) // c["BCAP"] != (int(c["rtail"][m]) - 1) // c["BCAP"] for m in range(c["N"]) if c["rtail"][m] > c["rhead"][m])
    grown = [m for m in range(c["N"]) if R.gs_round_ref(c, m) and ((R.gs_round_ref(c, m)["wnew"] - int(c["rwin"][m])) & R.M32) >> 31]
    assert grown, "a window that starts earlier than at the previous round (the spread grew)"
    s = R.gs_rounds_sweeps()
    assert [len(R.gs_round_ref(s, m)["swept"]) for m in range(s["N"])] == R.GS_SWEEP_NS


@pytest.mark.parametrize("name", [n for n in GS if n.startswith(("scatter", "send_nag", "contacts"))])
def test_gs_scatter_reference_by_sorting_the_pairs(name):
    c, r = GS[name], R.gs_ref(GS[name])
    pairs = sorted((int(c["T"][m][s]), m * c["F"] + s) for m in range(c["N"]) if c["tround"][m] for s in range(int(c["tcnt"][m])))
    flat = [ms for _, ms in pairs]
    for t in range(c["N"]):
        o, n = int(r["tin_off"][t]), int(r["tin_cnt"][t]) if not c["flags"] & R.GS_APPLY else int(r["tin_cnt_send"][t])
        assert flat[o:o + n] == r["tin"].get(t, []) and all(p[0] == t for p in pairs[o:o + n]), (name, t)
    assert sum(len(v) for v in r["tin"].values()) == len(pairs)


def _words(slots, QW):
    return [int(x) for x in R.gs_words(slots, QW)]


@pytest.mark.parametrize("name", [n for n in GS if n.startswith("send_")])
def test_gs_send_reference_against_word_arithmetic(name):
    """gs_ref decides one gossip at a time; here a target's receipts are built 64 slots at a time: window word & ~held word,
    minus the word of lost draws, OR-ed over the senders."""
    c, r = GS[name], R.gs_ref(GS[name])
    QW, F = c["SLOTS"] // 64, c["F"]
    for t, senders in r["tin"].items():
        held = _words(r["HB"][t] - r["new"][t], QW)
        got = [0] * QW
        for ms in senders:
            m, s = divmod(ms, F)
            win, pct = _words(r["WB"][m], QW), R.gs_pct(c, m, t)
            for q in range(QW):
                cand = win[q] & ~held[q] & R.M64
                lost = 0
                for b in range(64):
                    if cand >> b & 1 and (pct >= 100 or (pct > 0 and R.gs_lost(c, m, s, [q * 64 + b], pct))):
                        lost |= 1 << b
                got[q] |= cand & ~lost
        assert R.gs_bits(np.array(got, np.uint64)) == r["new"][t], (name, t)
    assert r["ctr_g"] == sum(len(r["WB"][ms // F]) for v in r["tin"].values() for ms in v)


def test_gs_send_cases_hold_the_shapes_they_name():
    twice = 0  # cases with a receipt that two senders of the target deliver
    for name, (nag, ntl) in list(R.GS_SEND_SHAPES.items()) + [("nag130", (130, 2))]:
        r = R.gs_ref(GS[f"send_{name}"])
        assert (r["nag"], len(r["tlist"])) == (nag, ntl), name
        assert nag == 64 or (nag * ntl) % 64, name
        if nag not in (1, 64):  # some target's items lie on both sides of a wave boundary
            assert any((i * nag) // 64 != ((i + 1) * nag - 1) // 64 for i in range(ntl)), name
        assert len({len(v) for v in r["tin"].values()}) > 1, "uneven sender counts"
        twice += any(len(v) > 1 and sum(len(r["WB"][ms // 8] & r["new"][t]) for ms in v) > len(r["new"][t]) for t, v in r["tin"].items())
        assert r["dead_rx"].max() == GS[f"send_{name}"]["k"] + 1, "a DEAD record delivered"
    assert twice >= 3
    assert R.gs_ref(GS["send_ring_full"])["err"] == R.E_RING
    assert 0 < sum(len(v) for v in R.gs_ref(GS["send_loss37"])["new"].values()) < sum(len(v) for v in R.gs_ref(GS["send_nag3"])["new"].values())
    assert sum(len(v) for v in R.gs_ref(GS["send_loss100"])["new"].values()) == 0
    em = R.gs_ref(GS["send_loss37_em"])["em"]
    assert em[1::2].sum() > 0 and (em[0::2] + em[1::2]) .sum() == 2 * sum(
        len(R.gs_ref(GS["send_loss37_em"])["WB"][ms // 8]) for t, v in R.gs_ref(GS["send_loss37_em"])["tin"].items()
        for ms in v if t != GS["send_loss37_em"]["targets"] // 2)


def test_gs_apply_case_holds_the_shapes_it_names():
    c = GS["apply_gains"]
    r = R.gs_ref(c)
    assert [len(r["new"][t]) for t in range(7)] == c["gains"] == [0, 1, 8, 9, 64, 65, 4096 + 65]
    reborn = int(((r["S"] & R.S16_REBORN) != 0).sum())
    assert reborn == len(r["hist"]) > 0 and reborn < sum(c["gains"]) // 2, "stale entries of an earlier gossip are no rebirth"
    assert r["rc_ndrop"].sum() > 0 and len(r["routed"]) > 0 and r["rc_ndrop"][5] == 0, "dead_rx routes every receipt of target 5"
    assert r["fexp"] == [1, 2, 40, 41, 2240, 2241, 2244] and r["free"] == [2240, 2241, 2244] and 2 in R.gs_bits(c["DM"]) - r["DM"]
    assert r["err"] == 0 and R.gs_ref(GS["apply_slife"])["err"] == R.E_SLIFE and R.gs_ref(GS["apply_rcap_short"])["err"] == R.E_RECEIPTS


def test_gs_contact_cases_encode_their_explicit_answer():
    """Every replayed gossip of a contact case is one its target never held (the S plane says so, and so does its ring), so
    `t not in infectedFrom_m(g)` and the send happens; the events sit where the case says."""
    c = GS["contacts"]
    r = R.gs_ref(c)
    k = c["k"]
    for v in r["rp"] + r["slow"]:
        g, ms = v >> 32, v & R.M32
        t = int(c["T"][ms // c["F"]][ms % c["F"]])
        assert c["S"][t][g] == 0 and g not in R.gs_bits(c["HB"][t])
    assert [r["tcontact"][ms] for ms in (0, 17)] == [0, 1], "a contact at the cut and one tick after it"
    assert r["cev"][64][0] == R.CEV and r["cev"][81][0] == R.CEV + 1 and r["cin"][81] == 0xFFFFFFFE
    assert r["cin"][49] == R.NEVER and r["cev"][113][1] == k - 16 and len(r["rx"]) == 3
    assert R.gs_ref(GS["contacts_cev1"])["cin"][64] == 0xFFFFFFFE
    assert R.gs_ref(GS["contacts_crcap1"])["fb"][R.FB_RX_ALL] == 2 and R.gs_ref(GS["contacts_rpcap_short"])["err"] == R.E_CONTACTS
    big = GS["contacts_logw128"]
    assert any(t2 == k - 6 and e >= 64 for e, t2 in enumerate(big["log_tick"][15].tolist())), "the contact lies in the second pass"


@pytest.mark.parametrize("name", list(R.gs_replay_cases()))
def test_gs_replay_case_encoding_against_its_explicit_sets(name):
    """The simulation's infectedFrom sets against what it wrote down for the engine: every holder's set is the members whose
    logged rounds targeted it while both held the gossip (a lossless link: each such send arrived); a window gossip whose
    target is in the set is among the sends the reference diverts to the replay lists, never on the fast path."""
    c = GS[name]
    r = R.gs_ref(c)
    diverted = {(v >> 32, v & R.M32) for v in r["rp"] + r["slow"]}
    for ms, t in ((m * c["F"] + s, int(c["T"][m][s])) for m in range(c["N"]) if c["tround"][m] for s in range(int(c["tcnt"][m]))):
        m = ms // c["F"]
        for g in r["WB"][m]:
            if t in c["infected"][m, g]:
                assert (g, ms) in diverted, (name, g, ms)
    for (x, g), inf in c["infected"].items():
        assert g in R.gs_bits(c["HB"][x]) and x not in inf
        for y in inf:  # y's log holds a round that targeted x at or after x's receipt less the latency
            cx = R.gs_s_get(c, int(c["S"][x][g]), g, c["k"] + c["lat"])
            assert any(t2 != R.NEVER and t2 + c["lat"] >= cx and x in c["log_tg"][y][e][:c["log_cnt"][y][e]].tolist()
                       for e, t2 in enumerate(c["log_tick"][y].tolist())), (name, x, g, y)
    blocked = {(g, ms) for g, ms in diverted if int(c["T"][ms // c["F"]][ms % c["F"]]) in c["infected"][ms // c["F"], g]}
    want = {"replay_a_c_e": ({(0, 0)}, {1, 2}), "replay_d_slow": ({(0, 0)}, {1, 2}), "replay_b_older": (set(), {0}),
            "replay_f_rebirth": ({(0, 0)}, set())}[name]
    assert (blocked, r["new"][1]) == want, (name, blocked, r["new"][1])
    assert (len(r["slow"]) > 0) == (name == "replay_d_slow")
    if name in ("replay_b_older", "replay_f_rebirth"):
        assert c["S"][0][0] & R.S16_REBORN and len(R.gs_hist_decode(c["hist"])) >= 1, "m's current incarnation is a rebirth"
    if name == "replay_a_c_e":
        assert (2, 0) not in diverted, "(e) the gossip created after the contact arrived takes the fast path"


def test_gs_pack_round_trip():
    c = GS["contacts"]
    params, inp, out = R.gs_pack(c)
    got = R.gs_unpack(c, out)
    assert len(params) == len(R.GS_PARAMS) == 27 and inp.nbytes % 8 == 0
    for f in ("HB", "WB", "S", "rg", "rhead", "rtail", "slot_exp", "hist"):
        assert np.array_equal(got[f], c[f]), f
    assert got["free_top"] == c["free_top"] and got["rc_n"] == 0 and (got["tin"] == R.GS_SENT).all()


# ---------------------------------------------------------------------------------------------- P4 (tests/test_gpu_p4.py)
P4_INCS = [0, 1, 2, 62, 63, 64, 2**30 - 2, 2**30 - 1]


def test_p4_is_overrides_matches_the_oracle(oracle):
    for s1 in range(1, 4):
        for s0 in range(4):
            for i1 in P4_INCS:
                for i0 in P4_INCS:
                    assert R.p4_is_overrides(s1, i1, s0, i0) == bool(oracle.swim_is_overrides(s1, i1, s0, i0)), \
                        (s1, i1, s0, i0)
    for n in (0, 1, 2, 3, 4, 94, 96, 127, 128, 300, 8320, 100_000):
        assert R.p4_ceil_log2(n) == oracle.swim_ceil_log2(n), n


def test_p4_batching_claim_equals_the_serial_fold():
    """A few thousand seeded lists of fast receipts: present rows, ALIVE / SUSPECT records about other members."""
    rng = np.random.default_rng(4242)
    accepted = 0
    for t in range(4000):
        nsub = int(rng.integers(1, 6))
        incs = [0, 1, 2, 3] if t % 3 else [61, 62, 63, 64]
        key0 = {s: (int(rng.choice(incs)) << 2) | int(rng.integers(1, 3)) for s in range(nsub)}
        lst = [(int(rng.integers(0, nsub)), int(rng.integers(1, 3)), int(rng.choice(incs)))
               for _ in range(int(rng.integers(1, 140)))]
        a, b = R.p4_batch_accepts(key0, lst), R.p4_serial_accepts(key0, lst)
        assert a == b, (key0, lst)
        accepted += sum(a)
    assert accepted > 4000
    # and through the whole fold: the rows it leaves are the largest key of each subject
    st = R.p4_member(0, 8, range(1, 8), range(1, 8))
    lst = [("M", int(rng.integers(1, 8)), int(rng.integers(1, 3)), int(rng.integers(0, 5))) for _ in range(300)]
    R.p4_fold(st, 1, 0, lst, set(), {"suspicion_mult": 5, "ping_t": 10, "md_t": 30, "lat": 2})
    for s in range(1, 8):
        top = max([(0 << 2) | 1] + [(i << 2) | x for _, q, x, i in lst if q == s])
        assert (st["row"][s][1] << 2) | st["row"][s][0] == top


def test_p4_fold_known_answers():
    cfg = {"suspicion_mult": 5, "ping_t": 10, "md_t": 30, "lat": 2}
    st = R.p4_member(2, 8, [0, 1, 3, 4, 5, 6, 7], [7, 6, 5, 4, 3, 1, 0])
    A, S, D = R.P4_ALIVE, R.P4_SUSPECT, R.P4_DEAD
    r = R.p4_fold(st, 5, 2, [("M", 3, S, 0), ("M", 3, A, 1), ("M", 3, S, 1), ("M", 4, D, 0), ("M", 4, S, 3), ("M", 4, A, 2),
                             ("M", 2, S, 0), ("U", 6, (9 << 32) | 8, 4), ("M", 7, A, 1), ("M", 5, A, 0)], {7}, cfg)
    dl = 5 + 5 * 4 * 10  # bitlen(8) = 4
    assert st["row"][3] == [S, 1, True, dl] and st["row"][4] == [A, 2, False, 0] and st["row"][2] == [A, 1, True, 0]
    assert st["tsize"] == 8 and st["cid"] == 3 and st["timerMin"] == dl and st["fnext"] == 7 and st["gcnt"] == 1
    # (SUSPECT 1 after ALIVE 1 is accepted without a fetch: the incarnation did not rise; the request to dead 7 is lost)
    assert [f[:4] for f in st["fetch"]] == [[0, 3, 1, A | 1 << 8 | 1 << 24], [1, 4, 2, A | 1 << 8 | 1 << 16 | 1 << 24]]
    assert st["fetch"][0][4:] == [R.M32, 35, 7, R.M32]
    assert r["events"] == [(5, 2, 0, "REMOVED", 4, 0, None, 0), (5, 2, 1, "GOSSIP", 6, 8, 9, 4)]
    assert st["fd"] == [0, 1, 3, 5, 6, 7] and st["gl"] == [7, 6, 5, 3, 1, 0]
    assert (r["R"], r["W"], r["M"], r["E"], r["LOST"]) == (11, 7, 3, 2, 1) and r["gossips"] == [(2, A, 1)]
    assert r["tl"] == [3, 4, 2, 7] and r["tl_n"] == 4 and not r["einc"]
    r = R.p4_fold(st, 6, 0, [("M", s % 8, S, 9 + s // 8) for s in range(40) if s % 8 != 2], set(), cfg)
    assert r["tl_n"] == R.P4_TL + 1 and len(r["tl"]) == R.P4_TL
    dead = R.p4_fold(R.p4_member(1, 4, [], []), 0, 3, [("M", 0, S, 0)], {1}, cfg)
    assert dead["R"] == 0 and dead["W"] == 0


@pytest.mark.parametrize("N", [66, 96, 300])
def test_p4_cases_meet_the_injector_preconditions(N):
    c = R.p4_case(N)
    names = set(c["who"].values())
    assert {f"count:{n}" for n in R.P4_COUNTS} <= names and len(c["who"]) == len(names)
    assert {f"slow:{w},{a}" for w in R.P4_SLOW_KINDS for a in R.P4_SLOW_AT} <= names
    assert max(c["who"]) >= 256 or N < 256, "members of the second k_member_tick block take part"
    slots = max(1024, 64 * N)  # swim_create's default slot table
    for i, tick in enumerate(c["ticks"] + R.p4_case_einc(N)["ticks"]):
        recs, lists = R.p4_pack(tick)
        assert R.p4_injectable(N, recs, lists, 1 << 16, slots), i
        assert len(set(recs)) == len(recs)
    for m, (_, lst) in c["ticks"][0].items():  # the preparation tick creates no gossip: no own record
        assert all(r[0] == "M" and r[1] != m for r in lst)
    # the patterns are what they say, on the reference itself
    cfg = {"suspicion_mult": 5, "ping_t": 10, "md_t": 30, "lat": 1}
    by = {v: k for k, v in c["who"].items()}
    res = {}
    for name, m in by.items():
        st = R.p4_member(m, N, [], [])
        for k, tick in enumerate(c["ticks"]):
            nd, lst = tick.get(m, (0, []))
            assert R.p4_hops(st, k, set(c["killed"]), cfg) == (6 if k == 1 and m in c["ticks"][0] else 0)  # the six requests
            # of the preparation tick
            res[name] = (st, R.p4_fold(st, k, nd, lst, set(c["killed"]), cfg), lst)
    for n in R.P4_COUNTS:
        assert len(res[f"count:{n}"][2]) == n
    for n in R.P4_ACCEPTED:  # n distinct accepted subjects: the write log overflows past 16
        for f in "sf":
            r = res[f"accepted:{n},{f}"][1]
            assert r["W"] == n and r["tl_n"] == min(n, R.P4_TL + 1) and r["M"] == (n if f == "f" else 0)
    for w in R.P4_SLOW_KINDS:
        for a in R.P4_SLOW_AT:
            st, r, lst = res[f"slow:{w},{a}"]
            assert len(lst) == 70 and (lst[a][0] == "U" or lst[a][1] == by[f"slow:{w},{a}"] or lst[a][2] == R.P4_DEAD
                                       or w == "absent")
            assert (len(r["gossips"]) == 1) == w.startswith("own") and (len(r["events"]) == 1) == (w in ("dead", "user"))
    for o in (0, 62):
        st, r, lst = res[f"triple:timer,{o}"]
        assert r["W"] == 3 and r["M"] == 2 and len(lst) == o + 3
        assert st["row"][lst[-1][1]][3] == 1 + 5 * (N - 2).bit_length() * 10  # a new timer, at the size after the removals
        assert res[f"triple:notimer,{o}"][1]["W"] == 3 and res[f"triple:notimer,{o}"][1]["M"] == 1
    assert res["killed:"][1]["LOST"] == 4 and res["killed:"][1]["M"] == 5 and res["incs:"][1]["W"] >= 8 and not res["incs:"][1]["einc"]
    if N == 66:  # a removal inside the list takes the table from 64 to 63 records: later timers use ceilLog2 = 6
        for name in ("slow:dead,0", "slow2:", "mixed:100"):
            assert {row[3] for row in res[name][0]["row"].values()} >= {5 * 7 * 10, 1 + 5 * 6 * 10}, name
    assert R.p4_fold(R.p4_member(3, N, [], []), 0, 0, R.p4_case_einc(N)["ticks"][0][3][1], set(), cfg)["einc"]
