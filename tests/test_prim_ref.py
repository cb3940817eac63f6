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
