"""Plain references and fixed-seed inputs for the device-primitive tests (tests/test_gpu_primitives.py).

Every reference is the most obvious formulation of the operation (np.cumsum, np.argsort, Python-int division,
np.searchsorted, popcounts through bin()), in numpy or Python integers, never a transcription of the device code.
tests/test_prim_ref.py checks each of them against a second naive formulation and every generated input set against
the conditions the primitives state (unique keys per segment, window bounds, totals), without a GPU.
"""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
NEVER = 0xFFFFFFFF
CH = 2048  # subjects per dirty / shipped chunk (engine.h CH)
SORT_MAX = 4096
MAX_EPOCHS = 8
S16_TICK = (1 << 13) - 1
RG_SLOT = (1 << 22) - 1
CHUNKS = [0, 63, 64, 65, 127, 128, 191]  # the mask-word edges of MW = 1, 2, 3


def u32(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------- exclusive scan
SCAN_NS = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4099, 2**20 - 1, 2**20]
SCAN_KINDS = ["zero", "one", "random", "wrap"]


def scan_input(n, kind):
    rng = np.random.default_rng(1000 + n)
    if kind == "zero":
        return np.zeros(n, np.uint32)
    if kind == "one":
        return np.ones(n, np.uint32)
    if kind == "random":
        return rng.integers(0, 4096, n, dtype=np.uint32)
    return rng.integers(2**31, 2**32, n, dtype=np.uint32)  # two of them already pass 2^32


def scan_ref(v):
    c = np.cumsum(v.astype(np.uint64), dtype=np.uint64)
    return (np.concatenate([np.zeros(1, np.uint64), c[:-1]]) & np.uint64(M32)).astype(np.uint32)


# ---------------------------------------------------------------------------------------------- segmented sort
def seg_lengths(run):
    if run == SORT_MAX:
        return [4095, 4096, 4097, 3 * 4096 + 5]
    return [2, 3, run - 1, run, run + 1, 2 * run - 1, 2 * run, 2 * run + 1, 3 * run, 5 * run + 7]


def seg_keys(rng, n, order):
    """n keys, unique, with 0 and values >= 2^63 among them (n >= 2), never ~0 (k_seg_sort's pad value)."""
    k = np.unique(rng.integers(1, 2**64 - 2, 2 * n + 8, dtype=np.uint64))
    k = rng.permutation(k)[:n]
    assert len(k) == n
    if n >= 2:
        k[0], k[1] = 0, 2**64 - 2
    if n >= 3:
        k[2] = 2**63
    k = rng.permutation(k)
    if order == "sorted":
        k = np.sort(k)
    elif order == "reversed":
        k = np.sort(k)[::-1]
    return np.ascontiguousarray(k)


def seg_case(lengths, listed, run, order, seed, gap=3):
    """Segments of the given lengths laid out with `gap` untouched entries around each; member ids are shuffled, so the
    list is in no order; listed[i]: whether segment i is in sg."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(len(lengths))
    total = gap + sum(n + gap for n in lengths)
    key = rng.integers(0, 2**64 - 1, total, dtype=np.uint64)
    val = rng.integers(0, 2**32, total, dtype=np.uint32)
    off = np.zeros(len(lengths), np.uint32)
    cnt = np.zeros(len(lengths), np.uint32)
    o = gap
    for i, n in enumerate(lengths):
        off[ids[i]], cnt[ids[i]] = o, n
        key[o:o + n] = seg_keys(rng, n, order)
        o += n + gap
    sg = rng.permutation(np.array([ids[i] for i in range(len(lengths)) if listed[i]], dtype=np.uint32))
    return dict(key=key, val=val, off=off, cnt=cnt, sg=u32(sg), run=run)


def seg_cases():
    """{name: case}: every (run, order) over the issue's lengths, 1500 listed segments (more than the 1024 blocks), and
    unlisted segments with cnt > 1 next to listed ones with cnt <= 1."""
    out = {}
    for run in (2, 64, SORT_MAX):
        for oi, order in enumerate(("random", "sorted", "reversed")):
            L = seg_lengths(run)
            out[f"run{run}-{order}"] = seg_case(L, [True] * len(L), run, order, 7 * run + oi)
    rng = np.random.default_rng(5)
    L = [int(x) for x in rng.integers(2, 6, 1500)]
    out["1500-segments"] = seg_case(L, [True] * len(L), SORT_MAX, "random", 11, gap=1)
    L = [5, 0, 1, 9, 130, 1, 0, 70, 2, 64]
    listed = [True, True, True, False, False, True, True, True, False, True]
    out["unlisted"] = seg_case(L, listed, 64, "random", 13)
    return out


def seg_sort_ref(c):
    """(key, val, merges) after k_seg_sort: listed segments of two entries or more sorted by key, values carried."""
    key, val = c["key"].copy(), c["val"].copy()
    merges = 0
    for s in c["sg"]:
        o, n = int(c["off"][s]), int(c["cnt"][s])
        if n <= 1:
            continue
        idx = np.argsort(c["key"][o:o + n], kind="stable")
        key[o:o + n] = c["key"][o:o + n][idx]
        val[o:o + n] = c["val"][o:o + n][idx]
        merges += n > c["run"]
    return key, val, merges


# ---------------------------------------------------------------------------------------------- receipt routing
ROUTE_SORT_CAP = 64


def routing_case(N, over, seed):
    """Receipts member << 32 | slot: the last member gets 150 (> sort_cap = 64, an odd number of runs), a third get
    exactly one, some a handful, the rest none. over: RCAP is five short of what *rc_n claims."""
    rng = np.random.default_rng(seed)
    slots = 1 << 12
    per = np.zeros(N, np.int64)
    per[np.arange(N) % 3 == 1] = 1
    few = np.arange(N) % 7 == 2
    per[few] = rng.integers(2, 6, int(few.sum()))
    per[N - 1] = 150
    assert (per == 0).any() and (per == 1).any()
    raw = []
    for m in range(N):
        for s in rng.choice(slots, int(per[m]), replace=False):  # a member receives a gossip once
            raw.append((m << 32) | int(s))
    raw = rng.permutation(np.array(raw, dtype=np.uint64))
    gid = np.unique(rng.integers(0, 2**64 - 1, 2 * slots, dtype=np.uint64))
    gid = np.ascontiguousarray(rng.permutation(gid)[:slots])  # injective, in no order: gid order is not slot order
    assert len(gid) == slots
    if over:
        rcap = len(raw) - 40
        return dict(N=N, RCAP=rcap, rc_n=rcap + 5, SLOTS=slots, raw=np.ascontiguousarray(raw[:rcap]), gid=gid)
    return dict(N=N, RCAP=len(raw) + 10, rc_n=len(raw), SLOTS=slots, raw=raw, gid=gid)


def routing_ref(c):
    """cnt, off, per-member (slots, keys) in ascending gossip id, and the set of members to sort."""
    raw = c["raw"][:min(c["rc_n"], c["RCAP"])]
    mem, slot = (raw >> np.uint64(32)).astype(np.int64), (raw & np.uint64(M32)).astype(np.int64)
    cnt = np.bincount(mem, minlength=c["N"]).astype(np.uint32)
    off = scan_ref(cnt)
    rows = {}
    for m in np.flatnonzero(cnt):
        s = slot[mem == m]
        s = s[np.argsort(c["gid"][s], kind="stable")]
        rows[int(m)] = (s.astype(np.uint32), c["gid"][s])
    return cnt, off, rows, set(int(m) for m in np.flatnonzero(cnt >= 2))


# ---------------------------------------------------------------------------------------------- lane patterns
def lane_patterns(blocks, seed=3):
    """{name: bool[blocks * 256]}: the active-lane masks every collective runs under."""
    rng = np.random.default_rng(seed)
    T, lane = blocks * 256, np.arange(blocks * 256) % 64
    per_wave = np.zeros(T, bool)
    for w in range(T // 64):  # a different mask in each of the 4 waves of a block, other ones in the next block
        kind = (w + w // 4) % 4
        m = [np.ones(64, bool), np.arange(64) == 63, np.arange(64) % 2 == 1, rng.random(64) < 0.2][kind]
        per_wave[64 * w:64 * w + 64] = m
    return {"full": np.ones(T, bool), "lane0": lane == 0, "lane63": lane == 63, "alternating": lane % 2 == 0,
            "sparse": rng.random(T) < 0.1, "per-wave": per_wave}


def append_ok(active, res, ctr0, ctr1):
    """wave_append: the active lanes' indices are a permutation of [ctr0, ctr0 + total), consecutive and ascending in
    lane order within a wave; the counter ends at ctr0 + total."""
    a = np.flatnonzero(active)
    r = res[a].astype(np.int64)
    if ctr1 != ctr0 + len(a) or sorted(r.tolist()) != list(range(ctr0, ctr0 + len(a))):
        return False
    for w in range(len(active) // 64):
        rw = res[64 * w:64 * w + 64][active[64 * w:64 * w + 64]].astype(np.int64)
        if len(rw) and not np.array_equal(rw, rw[0] + np.arange(len(rw))):
            return False
    return True


def reserve_ok(n, res, group, ctr0, ctr1):
    """wave_reserve (group = 64) / block_reserve (group = 256; several calls: concatenate them): within a group that
    reserves anything each thread's range starts where the previous thread's ends, and the groups' ranges tile
    [ctr0, ctr1) without a gap or an overlap, modulo 2^32. A group that reserves nothing leaves the counter alone."""
    n, res = n.astype(np.int64).reshape(-1, group), res.astype(np.int64).reshape(-1, group)
    tot = n.sum(axis=1)
    by_base = {}
    for g in np.flatnonzero(tot):
        excl = np.cumsum(n[g]) - n[g]
        if not np.array_equal(res[g], (res[g][0] + excl) & M32) or int(res[g][0]) in by_base:
            return False
        by_base[int(res[g][0])] = int(tot[g])
    cur = ctr0
    while by_base:
        if cur not in by_base:
            return False
        cur = (cur + by_base.pop(cur)) & M32
    return cur == ctr1 and ctr1 == (ctr0 + int(tot.sum())) & M32


def wave_sum32_ref(v):
    s = v.astype(np.uint64).reshape(-1, 64).sum(axis=1) & np.uint64(M32)
    return np.repeat(s.astype(np.uint32), 64)


def wave_min_ref(v):
    return np.repeat(v.reshape(-1, 64).min(axis=1), 64)


def wave_sum64_ref(v):
    """v: uint64[T]; the sum of each wave's 64 values modulo 2^64, in every lane."""
    return np.repeat(np.array([sum(int(x) for x in w) & M64 for w in v.reshape(-1, 64)], dtype=np.uint64), 64)


def sum64_values(seed=9):
    """uint64[512]: waves whose sums carry from the low half into the high one and out of bit 63."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**64 - 1, 512, dtype=np.uint64)
    v[0:64] = 2**32 - 1                      # 64 x (2^32 - 1): every step carries into the high word
    v[64:128] = 2**63                        # pairs wrap to 0
    v[128:192] = 2**63 - 1
    v[192:256] = 0
    v[192], v[255] = 2**32 - 1, 1            # one carry, from the first and the last lane
    v[256:320] = np.arange(64, dtype=np.uint64) << np.uint64(26)  # only lane-dependent bits around bit 32
    v[320:384] = 2**64 - 1
    return v


# ---------------------------------------------------------------------------------------------- dirty masks
def mask_int(words):
    return sum(int(w) << (64 * i) for i, w in enumerate(words))


def dirty_thread_case(MW, seed=21):
    """256 rows, one thread each: three subjects per row (NEVER: none) in the edge chunks below 64 MW, preset bits."""
    rng = np.random.default_rng(seed + MW)
    ch = [c for c in CHUNKS if c < 64 * MW]
    T = 256
    a = np.full((3, T), NEVER, np.uint32)
    for t in range(T):
        for j in range(3):
            if rng.random() < 0.8:
                c = ch[(t + j * (1 + t // len(ch))) % len(ch)]
                a[j, t] = c * CH + int(rng.choice([0, CH - 1, int(rng.integers(0, CH))]))
    pre = rng.integers(0, 2**64, (T, MW), dtype=np.uint64) & rng.integers(0, 2**64, (T, MW), dtype=np.uint64)
    pre[::2] = 0
    return a, pre


def dirty_wave_case(MW, seed=22):
    """8 rows, a wave each (2 blocks): s and wr per lane. Row 0 spans three chunks, row 1 has lane 0 unwritten, row 2
    writes nothing, row 3 one chunk from every lane, row 4 a chunk per lane, row 5 only lane 63, rows 6-7 random."""
    rng = np.random.default_rng(seed + MW)
    ch = [c for c in CHUNKS if c < 64 * MW]
    T, nch = 512, 64 * MW
    s = np.zeros(T, np.uint32)
    wr = np.zeros(T, np.uint32)
    lane = np.arange(64)
    sub = lambda c: (np.asarray(c) * CH + rng.integers(0, CH, 64)).astype(np.uint32)
    s[0:64], wr[0:64] = sub(np.array([ch[-1], ch[-2], 1])[lane % 3]), 1
    s[64:128], wr[64:128] = sub(np.array(ch)[lane % len(ch)]), (lane != 0)
    s[64] = 1 * CH  # lane 0's own chunk (no other lane's) must not be marked
    s[128:192], wr[128:192] = sub(np.array(ch)[lane % len(ch)]), 0
    s[192:256], wr[192:256] = sub(np.full(64, ch[-1])), 1
    s[256:320], wr[256:320] = sub((lane * MW + MW - 1) % nch), 1
    s[320:384], wr[320:384] = sub(np.array(ch)[lane % len(ch)]), (lane == 63)
    s[384:512], wr[384:512] = (rng.integers(0, nch, 128) * CH + rng.integers(0, CH, 128)), rng.random(128) < 0.3
    a = np.zeros((3, T), np.uint32)
    a[0], a[1] = s, wr
    pre = rng.integers(0, 2**64, (T // 64, MW), dtype=np.uint64) & rng.integers(0, 2**64, (T // 64, MW), dtype=np.uint64)
    pre[1] = 0
    return a, pre


def dirty_ref(pre, rows_subjects):
    """pre: uint64[rows][MW]; rows_subjects: per row the subjects written. The masks afterwards."""
    out = pre.copy()
    MW = pre.shape[1]
    for r, subs in enumerate(rows_subjects):
        m = mask_int(pre[r])
        for s in subs:
            m |= 1 << (int(s) // CH)
        out[r] = [(m >> (64 * i)) & M64 for i in range(MW)]
    return out


# ---------------------------------------------------------------------------------------------- window arithmetic
GOSSIP_TS = [1, 2, 3, 7, 10, 20, 64, 1000, 4095]


def div_gt_inputs(g):
    rng = np.random.default_rng(100 + g)
    x = [0, 1, g - 1, g, g + 1, 2**31 - 1, 2**31, 2**32 - g, 2**32 - 1]
    for k in rng.integers(1, 2**32 // g, 200):
        x += [int(k) * g - 1, int(k) * g]
    x += [int(v) for v in rng.integers(0, 2**32, 10000)]
    return u32([v & M32 for v in x])


def div_gt_ref(x, g):
    return u32([int(v) // g for v in x])


def s16_cases(seed=31):
    """(entry, ref, c): the stored bits of creation tick c (plus flag bits above them), read at c <= ref < c + 8192."""
    rng = np.random.default_rng(seed)
    cs = [0, 1, 8191, 8192, 8193, 2**29, 2**32 - 8193] + [int(v) for v in rng.integers(0, 2**32 - 8192, 300)]
    rows = []
    for c in cs:
        for d in [0, 1, 4095, 4096, 8190, 8191] + [int(v) for v in rng.integers(0, 8192, 6)]:
            flags = int(rng.integers(0, 8)) << 13  # EVER / SWEPT / REBORN: not part of the tick
            rows.append(((c & S16_TICK) | flags, c + d, c))
    return np.array(rows, dtype=np.uint64)


def rg_cases(seed=32):
    """(slot, infp, P): a ring entry written at infection period infp and read at round P, P - 500 <= infp <= P."""
    rng = np.random.default_rng(seed)
    rows = []
    for P in [0, 1, 511, 512, 1023, 1024, 2**32 - 1] + [int(v) for v in rng.integers(0, 2**32, 12)]:
        for infp in range(max(0, P - 500), P + 1):
            g = [0, RG_SLOT, int(rng.integers(0, RG_SLOT + 1))][infp % 3]
            rows.append((g, infp, P))
    return np.array(rows, dtype=np.uint64)


KEY8_KEYS = list(range(0x200)) + [2**32 - 1]


def key8_ref(k):
    return u32([int(v) if int(v) < 0xFF else 0xFF for v in k])


def delay_cases(seed=33):
    """[(di, thresholds, x)]: ascending tables of length 0, 1, 2, 255, 256 with repeats; x below, at, above each."""
    rng = np.random.default_rng(seed)
    out = []
    for di, n in [(0, 0), (1, 1), (15, 2), (7, 255), (3, 256)]:
        thr = np.sort(rng.integers(1, 2**32 - 1, n, dtype=np.uint32))
        if n >= 2:
            thr[1] = thr[0]  # ties
        if n >= 255:
            thr[100:110] = thr[100]
            thr[-2] = thr[-1]
        x = [0, 1, 2**31, 2**32 - 1]
        for t in thr:
            x += [int(t) - 1, int(t), int(t) + 1]
        out.append((di, u32(thr), u32(x)))
    return out


def delay_ref(thr, x):
    return np.searchsorted(thr, x, side="right").astype(np.uint32)


def epoch_cases():
    """[(ep_from[8], k)]: unused entries in the middle, two epochs from the same tick, k before every epoch and at
    2^32 - 2."""
    tabs = [[0, 10, NEVER, 10, NEVER, 50, NEVER, NEVER],
            [5, NEVER, NEVER, NEVER, NEVER, NEVER, NEVER, NEVER],
            [7, 7, 7, NEVER, 3, NEVER, 2**32 - 2, 2**32 - 2],
            [NEVER] * 8,
            [100, 90, NEVER, 80, 80, 70, NEVER, 60]]
    out = []
    for t in tabs:
        k = {0, 1, 2**32 - 2, 2**31}
        for f in t:
            if f != NEVER:
                k |= {max(f - 1, 0), f, f + 1}
        out.append((u32(t), u32(sorted(k))))
    return out


def epoch_ref(tab, k):
    """Index of the epoch in force at k: the latest start at or before k, the later index on a tie; -1 if none."""
    res = []
    for kk in k:
        c = [(int(f), e) for e, f in enumerate(tab) if int(f) != NEVER and int(f) <= int(kk)]
        res.append(max(c)[1] if c else -1)
    return np.array(res, dtype=np.int64)


def ship_value(r, j):
    return 0x80000000 | (r << 12) | j  # word j of the r-th shipped chunk; base_row[s] = s has the top bit clear


def paykey_cases(seed=34):
    """[(MW, mask words, subjects)]: for each MW a random mask and its complement, so every edge chunk is met both
    shipped and unshipped."""
    out = []
    for MW in (1, 2, 3):
        rng = np.random.default_rng(seed + MW)
        m = rng.integers(0, 2**64, MW, dtype=np.uint64)
        subs = []
        for c in [c for c in CHUNKS if c < 64 * MW] + [int(v) for v in rng.integers(0, 64 * MW, 20)]:
            subs += [c * CH, c * CH + CH - 1, c * CH + int(rng.integers(0, CH))]
        out.append((MW, m, u32(subs)))
        out.append((MW, ~m, u32(subs)))
    return out


def paykey_input(MW, mask):
    """(NS, base_row, shipped words) of a received payload with that chunk mask."""
    NS = MW * 64 * CH
    nship = bin(mask_int(mask)).count("1")
    ship = (0x80000000 | (np.arange(nship, dtype=np.uint32)[:, None] << 12) | np.arange(CH, dtype=np.uint32)[None, :])
    return NS, np.arange(NS, dtype=np.uint32), np.ascontiguousarray(ship.astype(np.uint32))


def paykey_ref(mask, subs):
    m = mask_int(mask)
    out = []
    for s in subs:
        c = int(s) // CH
        if not (m >> c) & 1:
            out.append(int(s))
        else:
            out.append(ship_value(bin(m & ((1 << c) - 1)).count("1"), int(s) % CH))
    return u32(out)


# ---------------------------------------------------------------------------------------------- Feistel
FEISTEL_NS = [1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 65535, 65536, 65537, 10**6, 2**20]
FEISTEL_KEYS = [(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0, 0xFFFFFFFF, 1, 0x80000000)]


def _fmix32(h):
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    return h ^ (h >> np.uint64(16))


def feistel_ref(n, keys):
    """SEMANTICS.md §3: four Feistel rounds (murmur3's finaliser as the round function) on the smallest even-width
    domain 2^b >= n, b >= 2, cycle-walked into [0, n); the image of 0 .. n - 1."""
    b = 2
    while (1 << b) < n:
        b += 2
    half, mask = np.uint64(b // 2), np.uint64((1 << (b // 2)) - 1)

    def once(x):
        L, R = x >> half, x & mask
        for k in keys:
            L, R = R, L ^ (_fmix32(R ^ np.uint64(k)) & mask)
        return (L << half) | R

    y = once(np.arange(n, dtype=np.uint64))
    while True:
        bad = y >= np.uint64(n)
        if not bad.any():
            return y.astype(np.uint32)
        y[bad] = once(y[bad])


# ---------------------------------------------------------------------------------------------- ring move
RING_SENTINEL = 0xDEADBEEF


def ring_case(B, B2, seed=41):
    """One member per (held entries, head position): t - h in {0, 1, 17, B}, h in {0, 5, 2^32 - 3} (positions wrap)."""
    rng = np.random.default_rng(seed)
    hs = [(h, (h + n) & M32) for n in (0, 1, 17, B) for h in (0, 5, 2**32 - 3)]
    rg = rng.integers(0, 2**32, (len(hs), B), dtype=np.uint32)
    rg[rg == RING_SENTINEL] = 0
    return rg, u32([h for h, _ in hs]), u32([t for _, t in hs])


def ring_ref(rg, rhead, rtail, B2):
    N, B = rg.shape
    out = np.full((N, B2), RING_SENTINEL, np.uint32)
    for m in range(N):
        p = int(rhead[m])
        while p != int(rtail[m]):
            out[m, p % B2] = rg[m, p % B]
            p = (p + 1) & M32
    return out


# ---------------------------------------------------------------------------------------------- SYNC diff and lister
# References for k_sync_diff and k_ack_resolve (tests/test_gpu_sync_diff.py, SWIM_PRIM_SYNC_DIFF). A key is
# inc << 2 | status (status 0 = ABSENT); a candidate word is subject << 34 | status << 32 | inc.
MCH, TL, NPER, PINWALK = 1024, 16, 4, 8
KF_DEFER, KF_ABS, KF_RES = 0x100, 0x200, 0x400
PAY_RX, DESC_PIN, DESC_DEFER = 0x40000000, 0x80000000, 0xFFFFFFFE
E_POOL = 128
SD_K8, SD_LISTER, SD_LISTS, SD_SHARDED, SD_DIRTY = 1, 2, 4, 8, 16
LS_SPEC, LS_NODIFF = 1, 2
SD_SENT = 0xA5A5A5A5
SD_SENT64 = SD_SENT | SD_SENT << 32
SD_NS = [1000, 1025, 2048, 2049, 2056, 8192, 8200, 131080, 262152]
SD_CTR = ["diffmsg", "diffmsg_all", "diffwide", "diffwide_all", "ackres", "ackres_all", "dstream", "dsubj", "dsubj_all",
          "dmsgskip", "pindec", "spare"]


def sd_sizes(N):
    """The sizes swim_create derives from the member count."""
    NS, NS8 = -(-N // 8) * 8, -(-N // 16) * 16
    NCHUNK, NMETA = -(-NS // CH), -(-NS // MCH)
    return dict(N=N, NS=NS, NS8=NS8, NCHUNK=NCHUNK, NMETA=NMETA, MW=-(-NCHUNK // 64), nit=-(-NCHUNK // NPER))


def key34(k):
    k = np.asarray(k).astype(np.uint64)
    return (k >> np.uint64(2)) | ((k & np.uint64(3)) << np.uint64(32))


def sync_diff_ref(payload_keys, receiver_keys):
    """(segments, absent): for each 1024-subject segment the words subject << 34 | key34(key), in subject order, of the
    payload records that are present and unequal to the receiver's; absent: some subject is ABSENT in the payload and
    present in the receiver (KF_ABS)."""
    p, r = np.asarray(payload_keys, np.uint32), np.asarray(receiver_keys, np.uint32)
    assert p.shape == r.shape
    present = (p & 3) != 0
    subj = np.flatnonzero(present & (p != r))
    words = (subj.astype(np.uint64) << np.uint64(34)) | key34(p[subj])
    nseg = -(-len(p) // MCH)
    cut = np.searchsorted(subj, np.arange(nseg + 1) * MCH)
    return [words[cut[g]:cut[g + 1]] for g in range(nseg)], bool((~present & ((r & 3) != 0)).any())


def rx_payload(base, mask, shipped):
    """A payload received from another shard: the baseline row overlaid with the shipped chunks, which are the chunks
    whose mask bit is set, in ascending chunk order. shipped: uint32[popcount(mask)][CH]."""
    out = np.array(base, np.uint32)
    j = 0
    for c in range(-(-len(out) // CH)):
        if (mask >> c) & 1:
            n = min(CH, len(out) - c * CH)
            out[c * CH:c * CH + n] = shipped[j][:n]
            j += 1
    assert j == bin(mask).count("1") == len(shipped)
    return out


def sd_payload(case, m):
    """The keys of message m's payload (NS of them): the sender's live row (pinned or not), its arena snapshot, or a
    received payload."""
    pay = m["payload"]
    if pay == NEVER:
        return case["rows"][m["src"] - case.get("lo", 0)]
    if pay & PAY_RX:
        rx = case["rx"][pay & ~PAY_RX]
        return rx_payload(case["base"], rx["mask"], rx["chunks"])
    return case["arena"][pay]


def sd_msg(src, dst, kind=1, payload=NEVER, pin=NEVER, tln=0):
    return dict(src=src, dst=dst, kind=kind, payload=payload, pin=pin, tln=tln)


def desc_pay(m):
    """Where a list entry says the payload is (engine.h DESC_*)."""
    if m["kind"] & KF_DEFER:
        return DESC_DEFER
    if m["payload"] != NEVER:
        return m["payload"]
    return NEVER if m["pin"] == NEVER else DESC_PIN | m["pin"]


def sd_log_subjects(case, m):
    """The subjects only which a SYNC_ACK's payload and its receiver's row can differ in when the ACK is resolvable: the
    responder's log prefix of tick k - 1 and the requester's logs of ticks k - 2 and k - 1; None when not resolvable
    (k < 2, no KF_RES, delayed, pinned, or a log past TL)."""
    k = case["k"]
    if k < 2 or not m["kind"] & KF_RES or m["kind"] & KF_DEFER or m["pin"] != NEVER or m["tln"] > TL:
        return None
    p0, p1, dst, src = k & 1, (k - 1) & 1, m["dst"], m["src"]
    n0 = int(case["tl_n"][p0][dst]) if int(case["tl_tick"][p0][dst]) == k - 2 else 0
    n1 = int(case["tl_n"][p1][dst]) if int(case["tl_tick"][p1][dst]) == k - 1 else 0
    if n0 > TL or n1 > TL:
        return None
    return sorted(set(case["tlog"][p1][src][:m["tln"]].tolist()) | set(case["tlog"][p0][dst][:n0].tolist())
                  | set(case["tlog"][p1][dst][:n1].tolist()))


def inbound_list(case, dst):
    out, q = [], int(case["m_head"][dst])
    while q != NEVER:
        out.append(q)
        q = int(case["m_next"][q])
    return out


def pin_clean_ref(case, i, dst):
    """A pinned live-row payload is decided from the masks when its receiver's inbound list has at most PINWALK messages,
    holds the message, all of them carry live rows and none is delayed, and the receiver's and every sender's masks are
    clear."""
    lst, MW = inbound_list(case, dst), sd_sizes(case["N"])["MW"]
    if len(lst) > PINWALK or i not in lst:
        return False
    msgs = [case["msgs"][q] for q in lst]
    if any(m["payload"] != NEVER or m["kind"] & KF_DEFER for m in msgs):
        return False
    return not any(int(case["dirty"][r][w]) for r in [dst] + [m["src"] for m in msgs] for w in range(MW))


def ack_resolve_ref(case):
    """What k_ack_resolve does with each message of a one-GPU case, by the documented conditions: a list of dicts with
    how = "resolved" (cand: the candidate words among the de-duplicated log subjects, in subject order), "pin" (a pinned
    live row decided from the masks), "decided" (a narrow payload with no chunk to stream), "narrow" (items: {item:
    chunk bits}) or "wide" (place: the entry's fourth word)."""
    z = sd_sizes(case["N"])
    k8, masks = bool(case["flags"] & SD_K8), bool(case["flags"] & SD_DIRTY)
    out = []
    for i, m in enumerate(case["msgs"]):
        subs = sd_log_subjects(case, m)
        if subs is not None:
            p, r = sd_payload(case, m), case["rows"][m["dst"]]
            c = [s for s in subs if p[s] & 3 and p[s] != r[s]]
            out.append(dict(how="resolved", cand=[(s << 34) | int(key34(p[s])) for s in c]))
            continue
        pw = desc_pay(m)
        if k8 and masks and m["payload"] == NEVER and pw not in (NEVER, DESC_DEFER) and pin_clean_ref(case, i, m["dst"]):
            out.append(dict(how="pin"))
        elif k8 and pw == NEVER:
            items = {}
            for c in range(z["NCHUNK"]):
                need = not masks or ((int(case["dirty"][m["src"]][c >> 6]) | int(case["dirty"][m["dst"]][c >> 6])) >> (c & 63)) & 1
                if need:
                    items[c // NPER] = items.get(c // NPER, 0) | 1 << (c % NPER)
            out.append(dict(how="narrow", items=items) if items else dict(how="decided"))
        else:
            out.append(dict(how="wide", place=pw))
    return out


def sd_pack(case):
    """(params, in words, out words) of a SWIM_PRIM_SYNC_DIFF call (include/swimhip_debug.h). MSGCAP defaults to one
    more than the messages: the buffer's last entry stays unused, as in an engine that is not at capacity."""
    z = sd_sizes(case["N"])
    fl, R, msgs = case["flags"], len(case["rows"]), case["msgs"]
    MSGCAP = case.get("MSGCAP", len(msgs) + 1)
    arena = case.get("arena", np.zeros((0, z["NS"]), np.uint32))
    nar, wide = case.get("narrow", []), case.get("wide", [])
    rx = case.get("rx", [])
    parts = [np.asarray(case.get("dirty", np.zeros((R, 3), np.uint64)), np.uint64)]
    if fl & SD_SHARDED:
        parts.append(np.array([[(r["mask"] >> (64 * q)) & M64 for q in range(z["MW"])] for r in rx], np.uint64).reshape(-1))
        parts.append(np.array([r["off"] for r in rx], np.uint64))
    parts += [u32(case["rows"]), u32(arena)]
    parts.append(u32([[m[f] for f in ("src", "dst", "kind", "payload", "pin", "tln")] for m in msgs]).reshape(-1))
    if fl & SD_LISTS:
        parts.append(u32(list(nar) + list(wide)).reshape(-1))
    if fl & SD_LISTER:
        parts += [u32(case["tl_tick"]), u32(case["tl_n"]), u32(case["tlog"]), u32(case["m_head"]), u32(case["m_next"])]
    if fl & SD_SHARDED:
        parts += [u32(case["base"]), u32(case["recv"])]
    inp = np.frombuffer(b"".join(np.ascontiguousarray(a).tobytes() for a in parts), dtype=np.uint32).copy()
    ncap = MSGCAP if fl & SD_SHARDED else MSGCAP * z["nit"]
    POOLCAP = case["POOLCAP"]
    nout = (2 * (POOLCAP + 64) + 24 + 6 * z["NCHUNK"] + 2 * z["NMETA"] * len(msgs) + 3 * len(msgs) + arena.size + 4 * ncap
            + 4 * MSGCAP + 8)
    params = [case["N"], R, fl, len(msgs), MSGCAP, len(arena), POOLCAP, case["k"], case.get("grid", 0), SD_SENT,
              len(nar), len(wide), case.get("lo", 0), len(rx), case.get("ls", 0)]
    return params, inp, np.zeros(nout, np.uint32)


def sd_unpack(case, out):
    z = sd_sizes(case["N"])
    n, MSGCAP = len(case["msgs"]), case.get("MSGCAP", len(case["msgs"]) + 1)
    A = len(case.get("arena", []))
    ncap = MSGCAP if case["flags"] & SD_SHARDED else MSGCAP * z["nit"]
    pos = [0]

    def take(words, dtype=np.uint32):
        a = out[pos[0]:pos[0] + words]
        pos[0] += words
        return a.view(dtype)

    r = dict(pool=take(2 * (case["POOLCAP"] + 64), np.uint64))
    r["ctr"] = dict(zip(SD_CTR, (int(v) for v in take(24, np.uint64))))
    r["cstat"] = take(6 * z["NCHUNK"], np.uint64).reshape(-1, 3)
    r["meta"] = take(2 * z["NMETA"] * n).reshape(n, z["NMETA"], 2)
    mk = take(3 * n).reshape(n, 3)
    r["kind"], r["ncand"], r["pin"] = mk[:, 0], mk[:, 1], mk[:, 2]
    r["arena"] = take(A * z["NS"]).reshape(A, z["NS"])
    r["narrow"] = take(4 * ncap).reshape(-1, 4)
    r["wide"] = take(4 * MSGCAP).reshape(-1, 4)
    s = take(8)
    r.update(pool_used=int(s[0]), err=int(s[1]), nnar=int(s[2]), nwide=int(s[3]), halt=s[4:7].tolist(), streamed=int(s[7]))
    assert pos[0] == len(out)
    return r


def sd_expect(case, narrow, wide):
    """What k_sync_diff must leave for the lists it streams: per message {segment: candidate words} for the segments it
    must write (an unlisted one stays untouched) and whether it sets KF_ABS; and per chunk the number of narrow compares
    of it (one GPU) that found a difference or an absent record (MS::cstat[1]). narrow / wide: entries (message, sender,
    receiver, fourth word). A narrow chunk whose bit is clear gets zero counts whatever the rows hold, a deferred
    message zero counts everywhere."""
    z = sd_sizes(case["N"])
    sharded = bool(case["flags"] & SD_SHARDED)
    exp = [dict(segs={}, absent=False) for _ in case["msgs"]]
    lo = case.get("lo", 0)
    differed = np.zeros(z["NCHUNK"], np.int64)

    def add(i, p, r, chunks):
        for c in chunks:
            a, b = c * CH, min((c + 1) * CH, z["NS"])
            segs, ab = sync_diff_ref(p[a:b], r[a:b])
            exp[i]["absent"] |= ab
            yield ab or any(len(w) for w in segs)
            for g, w in enumerate(segs):
                exp[i]["segs"][2 * c + g] = w + (np.uint64(a) << np.uint64(34))

    for i, src, dst, w in wide:
        r = case["rows"][dst - lo]
        if w == DESC_DEFER:
            for g in range(z["NMETA"]):
                exp[i]["segs"][g] = np.zeros(0, np.uint64)
            continue
        if w == NEVER or w & DESC_PIN:
            p = case["rows"][src - lo]
        elif w & PAY_RX:
            rx = case["rx"][w & ~PAY_RX]
            p = rx_payload(case["base"], rx["mask"], rx["chunks"])
        else:
            p = case["arena"][w]
        list(add(i, p, r, range(z["NCHUNK"])))
    for i, src, dst, w in narrow:
        r = case["rows"][dst - lo]
        if sharded:
            if w == NEVER:
                p = case["rows"][src - lo]
            else:
                rx = case["rx"][w & ~PAY_RX]
                p = rx_payload(case["base"], rx["mask"], rx["chunks"])
            list(add(i, p, r, range(z["NCHUNK"])))
            continue
        t, m4 = w >> 4, w & 15
        p = case["rows"][src - lo]
        for j in range(NPER):
            c = NPER * t + j
            if c >= z["NCHUNK"]:
                break
            if (m4 >> j) & 1:
                differed[c] += list(add(i, p, r, [c]))[0]
            else:
                for g in (2 * c, 2 * c + 1):
                    if g < z["NMETA"]:
                        exp[i]["segs"][g] = np.zeros(0, np.uint64)
    return exp, differed


# ---------------------------------------------------------------------------------------------- row-shard exchange codec
# References for k_pack_all, k_pack_b, k_inline_out and k_inline_in (tests/test_gpu_exchange.py; SWIM_PRIM_XPACK, PACK_B,
# INLINE_IN), written from the layout shard.hip's header comment states:
#   region A: u32 hdr[8] = {nslot, nround, nsync, nchunk, data_off, 0, 0, 0}; slot records [8 words]; round records
#   [12 words]; SYNC entries {SyncMsg, u32 chunk base, u32 0, u64 mask[MW], u32 log[16]}; chunks of 2048 keys at data_off,
#   which is the entries' end rounded up to 256.
# Everything the packer does not write keeps the caller's preset byte, so a comparison is equality of whole buffers.
SM_FIELDS = ("src", "dst", "kind", "seq", "cid_iss", "cid_cnt", "payload", "psize", "ncand", "pad", "pin", "due", "tln")
SMW = len(SM_FIELDS)          # words of a SyncMsg (engine.h; tests/test_prim_ref.py reads the struct's text)
NSW, RRW = 8, 12              # words of a new-slot and of a round record
XCNT_MASK, XFLAG_GOSSIP, XFLAG_OVER = (1 << 48) - 1, 1 << 62, 1 << 61
E_MSGS, E_ARENA, E_XCAP = 32, 64, 1 << 17
XP_ACKRES, XP_INLINE, XP_SPEC, XP_HALTED, XP_TLOG, XP_INLINE_OUT = 1, 2, 4, 8, 16, 32
XP_BYTE = 0xA5                # the preset of every output byte
XP_WORD, XP_WORD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def shard_lo(N, W, r):
    """First member of shard r: contiguous ranges floor(r N / W)."""
    return r * N // W


def shard_of(N, W, m):
    return max(r for r in range(W) if shard_lo(N, W, r) <= m)


def sync_entry_size(MW):
    return 4 * SMW + 8 + 8 * MW + 4 * TL


def xp_msg(i, src, dst, kind=1, payload=NEVER, tln=0):
    """A whole SyncMsg; the fields the packer only carries get distinct values derived from i."""
    return dict(src=src, dst=dst, kind=kind, seq=1000 + i, cid_iss=(7 * i + 3) & M32, cid_cnt=i ^ 0x55, payload=payload,
                psize=17 + i, ncand=0x00C0FFEE, pad=0x0BAD0000 | i, pin=NEVER, due=0x0D0E0000 | i, tln=tln)


def msg_words(m):
    return u32([m[f] for f in SM_FIELDS])


def mask_chunks(mask):
    return [c for c in range(mask.bit_length()) if (mask >> c) & 1]


def xp_payload(c, m):
    """(keys, dirty mask) of message m's payload on the sending rank."""
    lo = shard_lo(c["N"], c["W"], c["rank"])
    if m["payload"] == NEVER:
        return c["rows"][m["src"] - lo], c["rdirty"][m["src"] - lo]
    return c["arena"][m["payload"]], c["arena_dirty"][m["payload"]]


def xpack_ref(c):
    """What k_pack_all leaves in buffers preset to XP_BYTE: xa_send uint8[W][XA_PEER], xa_scnt uint64[W], xi_send and
    xi_out (k_inline_out on the same regions) uint8[W][XI], mtmp[MSGCAP][13], mlog[MSGCAP][16], xn[8], err; and per peer
    the region's parts, for the field-by-field comparisons: regions[q] = dict(fits, bytes, nslot, nround, nsync, nchunk,
    off_sync, data_off, entries = [(message index, chunk base, mask, log words shipped)]); None for the own rank."""
    z = sd_sizes(c["N"])
    N, W, rank, NS, MW, fl = c["N"], c["W"], c["rank"], z["NS"], z["MW"], c["flags"]
    XA, XI, CAP = c["XA_PEER"], c["XI"], c["MSGCAP"]
    lo = shard_lo(N, W, rank)
    out = dict(xa_send=np.full((W, XA), XP_BYTE, np.uint8), xa_scnt=np.full(W, XP_WORD64, np.uint64),
               xi_send=np.full((W, XI), XP_BYTE, np.uint8), xi_out=np.full((W, XI), XP_BYTE, np.uint8),
               mtmp=np.full((CAP, SMW), XP_WORD, np.uint32), mlog=np.full((CAP, TL), XP_WORD, np.uint32),
               xn=u32([c["xn0"], c["xn1"], XP_WORD, XP_WORD, c["xn4"], XP_WORD, XP_WORD, XP_WORD]), err=0, regions=[None] * W)
    xa, scnt, xi = out["xa_send"], out["xa_scnt"], out["xi_send"]
    halted = bool(fl & XP_SPEC and fl & XP_HALTED)
    if not halted:
        msgs = list(enumerate(c["msgs"]))[:CAP]
        ackres = bool(fl & XP_ACKRES)

        def log_prefix(m):  # a resolvable SYNC_ACK's sender's write-log prefix; nothing for the other messages
            n = m["tln"] if m["kind"] & KF_RES and m["tln"] <= TL else 0
            return c["tlog"][m["src"] - lo][:n] if n else u32([])

        nslot, nround = min(c["xn0"], c["NSCAP"]), min(c["xn1"], c["RRCAP"])
        SE = sync_entry_size(MW)
        for q in range(W):
            sel = [(i, m) for i, m in msgs if shard_of(N, W, m["dst"]) == q]
            if q == rank:  # the local column: straight to the next tick's inbound list, in message order
                for j, (i, m) in enumerate(sel, start=c["xn4"]):
                    if j < CAP:
                        out["mtmp"][j] = msg_words(m)
                        if ackres:
                            lp = log_prefix(m)
                            out["mlog"][j][:len(lp)] = lp
                    elif j == CAP:
                        out["err"] |= E_MSGS
                out["xn"][4] = (c["xn4"] + len(sel)) & M32
                if fl & XP_INLINE:
                    xi[q][:8] = 0
                continue
            nsync, nchunk = len(sel), sum(bin(xp_payload(c, m)[1]).count("1") for _, m in sel)
            off_sync = 32 + 4 * NSW * nslot + 4 * RRW * nround
            data_off = -(-(off_sync + SE * nsync) // 256) * 256
            total = data_off + nchunk * CH * 4
            fits = nsync <= c["RQCAP"] and total <= XA and nchunk <= c["CHCAP"]
            reg = dict(fits=fits, bytes=total if fits else 32, nslot=nslot if fits else 0, nround=nround if fits else 0,
                       nsync=nsync if fits else 0, nchunk=nchunk if fits else 0, off_sync=off_sync,
                       data_off=data_off if fits else 256, entries=[])
            out["regions"][q] = reg
            if not fits:
                out["err"] |= E_XCAP
            xa[q][:32] = u32([reg["nslot"], reg["nround"], reg["nsync"], reg["nchunk"], reg["data_off"], 0, 0, 0]).view(np.uint8)
            scnt[q] = reg["bytes"] | (XFLAG_GOSSIP if c["used"] > 0 else 0)
            if not fits:
                continue
            rec = np.concatenate([u32(c["ns_rec"]).reshape(-1)[:NSW * nslot], u32(c["rr_rec"]).reshape(-1)[:RRW * nround]])
            xa[q][32:off_sync] = u32(rec).view(np.uint8)
            base = 0
            for j, (i, m) in enumerate(sel):
                keys, mask = xp_payload(c, m)
                lp = log_prefix(m) if ackres else u32([])
                e = np.concatenate([msg_words(m), u32([base, 0]),
                                    u32([(mask >> (32 * w)) & M32 for w in range(2 * MW)]), u32(lp)])
                o = off_sync + SE * j
                xa[q][o:o + 4 * len(e)] = e.view(np.uint8)
                reg["entries"].append((i, base, mask, len(lp)))
                for c_ in mask_chunks(mask):  # the payload's dirty chunks in ascending order; the last one may be partial
                    n = min(CH, NS - c_ * CH)
                    o = data_off + base * CH * 4
                    xa[q][o:o + 4 * n] = u32(keys[c_ * CH:c_ * CH + n]).view(np.uint8)
                    base += 1
            assert base == nchunk
        if fl & XP_INLINE:  # the count word, then the region's head; OVER on every peer's word if any region is past it
            over = any(q != rank and (int(scnt[q]) & XCNT_MASK) > XI - 8 for q in range(W))
            for q in range(W):
                if q != rank:
                    word = int(scnt[q]) | (XFLAG_OVER if over else 0)
                    n = min(word & XCNT_MASK, XI - 8)
                    xi[q][:8] = np.array([word], np.uint64).view(np.uint8)
                    xi[q][8:8 + n] = xa[q][:n]
    for q in range(W):  # k_inline_out: the same block from the same region and count word, without the OVER mark
        n = min(int(scnt[q]) & XCNT_MASK, XI - 8)
        out["xi_out"][q][:8] = np.array([scnt[q]], np.uint64).view(np.uint8)
        out["xi_out"][q][8:8 + n] = xa[q][:n]
    return out


def xp_pack(c, inline_out=True):
    """(params, in, out) of a SWIM_PRIM_XPACK call; out is preset to XP_BYTE."""
    z = sd_sizes(c["N"])
    MW, CAP, W = z["MW"], c["MSGCAP"], c["W"]
    words64 = lambda masks: np.array([[(m >> (64 * w)) & M64 for w in range(MW)] for m in masks], np.uint64).reshape(-1)
    parts = [words64(c["rdirty"]), words64(c["arena_dirty"]), u32(c["rows"]), u32(c["arena"]),
             u32([msg_words(m) for m in c["msgs"]]).reshape(-1)]
    fl = c["flags"] | (XP_INLINE_OUT if inline_out else 0)
    if c["tlog"] is not None:
        parts.append(u32(c["tlog"]))
        fl |= XP_TLOG
    parts += [u32(c["ns_rec"]).reshape(-1), u32(c["rr_rec"]).reshape(-1)]
    raw = b"".join(np.ascontiguousarray(a).tobytes() for a in parts)
    inp = np.frombuffer(raw + b"\0" * (-len(raw) % 8 + 8), np.uint64).copy()  # 8-byte aligned, whatever its length
    nin = len(raw)
    params = [c["N"], W, c["rank"], len(c["rows"]), c["b"], fl, len(c["msgs"]), CAP, len(c["arena"]), c["NSCAP"], c["RRCAP"],
              c["RQCAP"], c["CHCAP"], c["XA_PEER"], c["XI"], c["used"], c["xn0"], c["xn1"], len(c["ns_rec"]), len(c["rr_rec"]),
              c["xn4"], XP_WORD]
    nout = W * c["XA_PEER"] + 8 * W + 2 * W * c["XI"] + 4 * (SMW * CAP + TL * CAP + 10)
    return params, inp.view(np.uint8)[:nin], np.full(nout // 8 + 1, XP_WORD64, np.uint64).view(np.uint8)[:nout]


def xp_unpack(c, out):
    W, XA, XI, CAP = c["W"], c["XA_PEER"], c["XI"], c["MSGCAP"]
    pos = [0]

    def take(nbytes, dtype=np.uint8):
        a = out[pos[0]:pos[0] + nbytes]
        pos[0] += nbytes
        return np.frombuffer(a.tobytes(), dtype=dtype)

    r = dict(xa_send=take(W * XA).reshape(W, XA), xa_scnt=take(8 * W, np.uint64), xi_send=take(W * XI).reshape(W, XI),
             xi_out=take(W * XI).reshape(W, XI), mtmp=take(4 * SMW * CAP, np.uint32).reshape(CAP, SMW),
             mlog=take(4 * TL * CAP, np.uint32).reshape(CAP, TL), xn=take(32, np.uint32))
    tail = take(8, np.uint32)
    r.update(err=int(tail[0]), halt=int(tail[1]))
    assert pos[0] == len(out)
    return r


def xp_rows(N, specs, seed):
    """(base_row, rows, masks): a baseline row of present keys (padding 0) and one row per spec = (chunks that differ from
    the baseline, chunks marked dirty although equal). A mask bit is set iff the chunk differs, plus the extra bits; a
    differing chunk differs in its first and last key and in one between."""
    z = sd_sizes(N)
    rng = np.random.default_rng(seed)
    base = np.zeros(z["NS"], np.uint32)  # the same for every case of one N: the ranks of a cluster share the baseline
    base[:N] = (np.random.default_rng(7000 + N).integers(1, 2**20, N).astype(np.uint32) << np.uint32(2)) | np.uint32(1)
    rows, masks = [], []
    for differ, extra in specs:
        row = base.copy()
        for c_ in differ:
            a, b = c_ * CH, min((c_ + 1) * CH, N)
            for s in {a, b - 1, a + int(rng.integers(0, b - a))}:
                row[s] += np.uint32(4 * int(rng.integers(1, 100)))
        rows.append(row)
        masks.append(sum(1 << c_ for c_ in set(differ) | set(extra)))
    return base, np.array(rows, np.uint32).reshape(len(specs), z["NS"]), masks


def xp_case(N, W, rank, rows, arena, msgs, seed, **kw):
    """A case with the capacities an engine that is not at capacity has (every region fits, one spare message), unless
    kw says otherwise. rows / arena: specs of xp_rows."""
    z = sd_sizes(N)
    base, allrows, masks = xp_rows(N, list(rows) + list(arena), seed)
    R = len(rows)
    rng = np.random.default_rng(seed + 1)
    c = dict(N=N, W=W, rank=rank, b=seed & 1, flags=0, base=base, rows=allrows[:R], rdirty=masks[:R], arena=allrows[R:],
             arena_dirty=masks[R:], msgs=msgs, MSGCAP=len(msgs) + 1, NSCAP=4, RRCAP=4, RQCAP=len(msgs) + 1, CHCAP=4096,
             XI=16384, used=0, xn0=0, xn1=0, xn4=0, ns_rec=np.zeros((0, NSW), np.uint32), rr_rec=np.zeros((0, RRW), np.uint32),
             tlog=rng.integers(0, N, (R, TL)).astype(np.uint32))
    c.update(kw)
    if "XA_PEER" not in c:
        nch = sum(bin(xp_payload(c, m)[1]).count("1") for m in msgs)
        head = 32 + 4 * NSW * c["NSCAP"] + 4 * RRW * c["RRCAP"] + sync_entry_size(z["MW"]) * len(msgs)
        c["XA_PEER"] = max(-(-head // 256) * 256 + 256 + nch * CH * 4, -(-c["XI"] // 16) * 16)  # k_inline_out reads XI - 8
    return c


def xp_records(N, slots, cnts, seed, origins=None, members=None):
    """(ns_rec, rr_rec): new-slot records {slot, gid lo, gid hi, subject, tick, key lo, key hi, origin} and round records
    {member, cnt, spread, period, targets[8]} with the given target counts; the targets past cnt are noise that the
    packer ships as it is."""
    rng = np.random.default_rng(seed)
    ns = u32([[g, int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)), int(rng.integers(0, N)), 40, int(rng.integers(0, 2**30)),
               int(rng.integers(1, 4)), origins[i] if origins else int(rng.integers(0, N))] for i, g in enumerate(slots)]).reshape(-1, NSW)
    rr = u32([[members[i] if members else int(rng.integers(0, N)), n, 3 + i, 10 + i] + [int(t) for t in rng.integers(0, N, 8)]
              for i, n in enumerate(cnts)])
    return ns, rr.reshape(-1, RRW)


def _n2049_msgs():
    # rank 1 of N = 2049, W = 3 owns 683 .. 1365; rows 683 .. 688
    return [xp_msg(0, 683, 5), xp_msg(1, 684, 1400), xp_msg(2, 685, 7), xp_msg(3, 686, 2000), xp_msg(4, 686, 700),
            xp_msg(5, 687, 100), xp_msg(6, 683, 1500, payload=0), xp_msg(7, 688, 0, kind=2, payload=1), xp_msg(8, 688, 2048),
            xp_msg(9, 684, 1365), xp_msg(10, 685, 682), xp_msg(11, 686, 1366, kind=2)]


N2049_ROWS = [([], []), ([0], []), ([1], []), ([0, 1], []), ([], [1]), ([0], [1])]
N2049_ARENA = [([1], []), ([], [])]


def xpack_cases():
    """{name: case}: the smallest shapes that reach each edge of k_pack_all (tests/test_prim_ref.py asserts that each one
    does). A region of k_pack_all is a multiple of 256 B (or 32 B after an overflow), so the inline edges are reached by
    moving XI around a 256-B region: XI = 272, 264, 256, 248 put it at XI - 16, XI - 8, XI and XI + 8."""
    out = {}
    # NS = 8: one chunk, and that one partial; a local, a peer and a local destination
    out["n5-w2"] = xp_case(5, 2, 0, [([0], []), ([], [])], [], [xp_msg(0, 0, 1), xp_msg(1, 0, 3), xp_msg(2, 1, 0)], 51)
    # NS = 2056: the second chunk has 8 keys; clean, one-chunk and two-chunk payloads, live and arena rows, records
    ns, rr = xp_records(2049, [5, 64, 127], [0, 1, 8], 52, origins=[700, 700, 1000], members=[683, 684, 1365])
    big = dict(ns_rec=ns, rr_rec=rr, xn0=3, xn1=3, used=3, flags=XP_INLINE)
    out["n2049-w3-r1"] = xp_case(2049, 3, 1, N2049_ROWS, N2049_ARENA, _n2049_msgs(), 53, **big)
    out["n2049-clamped"] = xp_case(2049, 3, 1, N2049_ROWS, N2049_ARENA, _n2049_msgs(), 53, **dict(big, NSCAP=2, RRCAP=1, xn0=9, xn1=3,
                                   ns_rec=ns[:2], rr_rec=rr[:1]))
    out["spec-halted"] = xp_case(2049, 3, 1, N2049_ROWS, N2049_ARENA, _n2049_msgs(), 53, **dict(big, flags=XP_INLINE | XP_SPEC | XP_HALTED))
    out["spec-runs"] = xp_case(2049, 3, 1, N2049_ROWS, N2049_ARENA, _n2049_msgs(), 53, **dict(big, flags=XP_INLINE | XP_SPEC))
    # three batches of the block scans: 600 messages to the peer, 300 local, dirty payloads around the batch edges
    dirty_src = {255: 4, 256: 5, 257: 6, 511: 7, 512: 4, 2: 5, 700: 6, 898: 4}
    msgs = []
    for i in range(900):
        local = (i % 3 == 0 and i != 255) or i == 1
        msgs.append(xp_msg(i, dirty_src.get(i, i % 4), (i * 5) % 2050 if local else 2050 + (i * 7) % 2050))
    rows = [([], [])] * 4 + [([0, 1, 2], []), ([0, 2], []), ([1], []), ([2], [0])]
    out["n4100-batches"] = xp_case(4100, 2, 0, rows, [], msgs, 54, flags=XP_INLINE)
    # MW = 2, NCHUNK = 65: mask bits 0, 63 and 64; a message to every peer but shard 5, which gets a header only
    lo = shard_lo(131073, 8, 3)
    rows = [([0], []), ([63], []), ([64], []), ([0, 63, 64], [])]
    msgs = [xp_msg(0, lo, 0), xp_msg(1, lo + 1, 16384), xp_msg(2, lo + 2, 49151), xp_msg(3, lo + 3, 65536), xp_msg(4, lo, lo + 10),
            xp_msg(5, lo + 1, 98304, payload=0), xp_msg(6, lo + 3, 131072), xp_msg(7, lo + 2, 100), xp_msg(8, lo + 1, 70000)]
    out["n131073-w8-r3"] = xp_case(131073, 8, 3, rows, [([63, 64], [])], msgs, 55, flags=XP_INLINE)
    # the inline block's edges: a 256-B region (one clean message) against XI; XI = 64 is the floor of the xinl capacity
    for XI in (272, 264, 256, 248, 64):
        out[f"inl-xi{XI}"] = xp_case(5, 2, 0, [([], [])], [], [xp_msg(0, 0, 4)], 56, flags=XP_INLINE, XI=XI)
    out["inl-off"] = xp_case(5, 2, 0, [([], [])], [], [xp_msg(0, 0, 4)], 56, flags=0, XI=248)
    # one of two peers over: shard 1 gets 256 B = XI - 8, shard 2 a chunk more; the OVER mark must land on both
    out["inl-one-over"] = xp_case(5, 3, 0, [([0], [])], [([], [])], [xp_msg(0, 0, 1, payload=0), xp_msg(1, 0, 3)], 57,
                                  flags=XP_INLINE, XI=264)
    # overflows: the region that does not fit is a header of zero counts, the other peer's is complete
    m3 = [xp_msg(0, 683, 1), xp_msg(1, 683, 2), xp_msg(2, 683, 3), xp_msg(3, 684, 1400)]
    out["ovf-rqcap"] = xp_case(2049, 3, 1, N2049_ROWS, [], m3, 58, flags=XP_INLINE, RQCAP=2, MSGCAP=8)
    m2 = [xp_msg(0, 686, 1), xp_msg(1, 684, 1400)]
    out["ovf-chcap"] = xp_case(2049, 3, 1, N2049_ROWS, [], m2, 59, flags=XP_INLINE, CHCAP=1)
    out["ovf-xa-peer"] = xp_case(2049, 3, 1, N2049_ROWS, [], m2, 60, flags=XP_INLINE, XA_PEER=256 + CH * 4, XI=1024)
    # MSGCAP = 4 and six local messages: k_pack_all reads at most MSGCAP messages of a tick, so the column passes MSGCAP only
    # with messages already queued (xn[4] = 2, as k_sync_redeliver leaves them) and four more
    m4 = [xp_msg(i, i % 2, (i + 1) % 2) for i in range(4)]
    out["ovf-msgcap"] = xp_case(5, 2, 0, [([0], []), ([], [])], [], m4, 61, MSGCAP=4, xn4=2, RQCAP=4)
    # ack resolution: log prefixes of 0, 1, 16 and 17 (past TL: none shipped) subjects, to a peer and locally
    ma = [xp_msg(i, 683 + i % 4, [9, 690][i // 4], kind=2 | KF_RES, tln=[0, 1, 16, 17][i % 4]) for i in range(8)]
    ma += [xp_msg(8, 684, 10, kind=1, tln=5), xp_msg(9, 685, 691, kind=2, tln=5)]  # no KF_RES: no prefix
    out["ackres-on"] = xp_case(2049, 3, 1, N2049_ROWS, [], ma, 62, flags=XP_INLINE | XP_ACKRES)
    out["ackres-off"] = xp_case(2049, 3, 1, N2049_ROWS, [], ma, 62, flags=XP_INLINE)
    return out


def xp_shape(c):
    """What a case reaches, for tests/test_prim_ref.py: batches of the block scans, chunks copied per block of each peer
    column (chunk r of a column goes to block r % 16), MW, and each peer region's bytes."""
    ref = xpack_ref(c)
    per_block = {q: [sum(1 for r in range(reg["nchunk"]) if r % 16 == x) for x in range(16)]
                 for q, reg in enumerate(ref["regions"]) if reg}
    return dict(batches=-(-min(len(c["msgs"]), c["MSGCAP"]) // 256), per_block=per_block, MW=sd_sizes(c["N"])["MW"],
                bytes={q: reg["bytes"] for q, reg in enumerate(ref["regions"]) if reg}, err=ref["err"],
                fits={q: reg["fits"] for q, reg in enumerate(ref["regions"]) if reg})


# ---- k_unpack_a (with msgs_commit, tick_end and the speculative gate), optionally behind k_inline_in
XU_END, XU_SPEC, XU_HALTED, XU_ACKRES, XU_INLINE_IN, XU_GOSSIP = 1, 2, 4, 8, 16, 32
XU_SC = ["nmsg0", "nmsg1", "arena0", "arena1"] + [f"xn{i}" for i in range(8)] + ["err", "halt", "pool_used", "rc_n", "ndl", "ndlw"]
S16_EVER, USER_SUBJ, ST_DEAD = 1 << 13, 0xFFFFFFFF, 3
XU_GOSSIP_DEFAULT = dict(SLOTS=128, BCAP=4, LOGW=2, F=8, EXPB=30, gossip_t=3)


def rg_entry(g, infp):
    return g | ((infp & 1023) << 22)


def rounds_before(first, c, gossip_t):
    """Gossip rounds of a member (first round at tick `first`, one every gossip_t ticks) strictly before tick c."""
    return 0 if first == NEVER or c <= first else -(-(c - first) // gossip_t)


def xu_case(q, senders, local=(), k=7, flags=0, gossip=None, **kw):
    """What rank q receives in one tick. senders: {p: XPACK case of rank p}; the region of p is xpack_ref's, so the
    unpacker is tested against a known-good packer. local: the messages already queued in mtmp. What the case expects is
    derived from the senders' messages, not from the regions' bytes: entries = [dict(msg, mask, off, keys, log)]."""
    c0 = next(iter(senders.values()))
    N, W = c0["N"], c0["W"]
    XA = kw.pop("XA_PEER", max(c["XA_PEER"] for c in senders.values()))
    recv, rcnt, entries = np.full((W, XA), XP_BYTE, np.uint8), np.zeros(W, np.uint64), []
    for p, c in senders.items():
        assert c["rank"] == p != q and (c["N"], c["W"]) == (N, W) and c["XA_PEER"] <= XA
        ref = xpack_ref(c)
        reg, lo = ref["regions"][q], shard_lo(N, W, p)
        recv[p][:c["XA_PEER"]] = ref["xa_send"][q]
        rcnt[p] = ref["xa_scnt"][q]
        for i, base, mask, _ in reg["entries"]:
            m = c["msgs"][i]
            log = c["tlog"][m["src"] - lo][:m["tln"]] if m["kind"] & KF_RES and m["tln"] <= TL else u32([])
            entries.append(dict(msg=m, mask=mask, off=p * XA + reg["data_off"] + base * CH * 4, keys=xp_payload(c, m)[0], log=log))
    scnt = np.full(W, 32, np.uint64)
    scnt[q] = 0
    case = dict(N=N, W=W, rank=q, k=k, flags=flags | (XU_GOSSIP if gossip is not None else 0), AR=64, XA_PEER=XA, XI=1024,
                local=[dict(m) for m in local], recv=recv, rcnt=rcnt, scnt=scnt, entries=entries, base=c0["base"],
                senders=senders, MSGCAP=len(local) + len(entries) + 1, RXCAP=len(entries) + 1, gossip=gossip)
    case.update(kw)
    return case


def xu_gossip_state(N, seed, **kw):
    """The small gossip-plane state slot_create and the round replay read: every member's first round tick (some NEVER),
    ring head and end, log position (0, mid-ring and wrapped ones) and the spreads logged before."""
    g = dict(XU_GOSSIP_DEFAULT, **kw)
    rng = np.random.default_rng(seed)
    first = rng.integers(0, 40, N).astype(np.uint32)
    first[::5] = NEVER
    rhead = rng.integers(0, 2**32, N, dtype=np.uint32)
    rhead[::3] = 0
    g.update(first=first, rhead=rhead, rtail=rhead.copy(), log_pos=(np.arange(N) % 5).astype(np.uint32),
             log_spread=rng.integers(3, 6, (N, g["LOGW"])).astype(np.uint32))
    return g


def xu_blocks(case):
    """The inline blocks [W][XI] of the case's regions: the count word, then the region's head."""
    XI = case["XI"]
    blocks = np.full((case["W"], XI), XP_BYTE, np.uint8)
    for p in range(case["W"]):
        blocks[p][:8] = np.array([case["rcnt"][p]], np.uint64).view(np.uint8)
        blocks[p][8:] = case["recv"][p][:XI - 8]
    return blocks


def xu_sizes(case):
    z, g = sd_sizes(case["N"]), case["gossip"]
    N, W, CAP, RX = case["N"], case["W"], case["MSGCAP"], case["RXCAP"]
    core = [("msgs", np.uint32, (CAP, SMW)), ("m_head", np.uint32, (N,)), ("m_next", np.uint32, (CAP,)),
            ("rx_mask", np.uint64, (RX, z["MW"])), ("rx_off", np.uint64, (RX,)), ("mlog", np.uint32, (CAP, TL)),
            ("sc", np.uint32, (18,)), ("xa_scnt", np.uint64, (W,)), ("xb_scnt", np.uint64, (W,)), ("xdone", np.uint32, (2 * W,)),
            ("xa_rcnt", np.uint64, (W,)), ("host", np.uint64, (2 * W,))]
    if g is not None:
        S, Q, B, L, F = g["SLOTS"], g["SLOTS"] // 64, g["BCAP"], g["LOGW"], g["F"]
        core += [("slot_gid", np.uint64, (S,)), ("slot_key", np.uint64, (S,)), ("slot4", np.uint32, (4, S)), ("gudm", np.uint64, (2, Q)),
                 ("S", np.uint16, (N, S)), ("HB", np.uint64, (N, Q)), ("rg", np.uint32, (N, B)), ("mem8", np.uint32, (8, N)),
                 ("T", np.uint32, (N, F)), ("log3", np.uint32, (3, N, L)), ("log_tg", np.uint32, (N, L, F))]
    return core


def xu_pack(case):
    """(params, in, out) of a SWIM_PRIM_XUNPACK call; out is preset to XP_BYTE."""
    g, fl = case["gossip"], case["flags"]
    parts = [xu_blocks(case) if fl & XU_INLINE_IN else case["recv"], case["rcnt"], case["scnt"],
             u32([msg_words(m) for m in case["local"]]).reshape(-1)]
    if g is not None:
        parts += [u32(g["first"]), u32(g["rhead"]), u32(g["rtail"]), u32(g["log_pos"]), u32(g["log_spread"])]
    raw = b"".join(np.ascontiguousarray(a).tobytes() for a in parts)
    inp = np.frombuffer(raw + b"\0" * (-len(raw) % 8 + 8), np.uint64).copy().view(np.uint8)[:len(raw)]
    gg = g or dict(SLOTS=0, BCAP=0, LOGW=0, F=0, EXPB=0, gossip_t=0)
    params = [case["N"], case["W"], case["rank"], case["k"], fl, case["MSGCAP"], case["RXCAP"], case["AR"], case["XA_PEER"],
              case["XI"], len(case["local"]), gg["SLOTS"], gg["BCAP"], gg["LOGW"], gg["F"], gg["EXPB"], gg["gossip_t"], XP_WORD]
    nout = sum(np.dtype(dt).itemsize * int(np.prod(sh)) for _, dt, sh in xu_sizes(case))
    return params, inp, np.full(nout // 8 + 1, XP_WORD64, np.uint64).view(np.uint8)[:nout]


def xu_unpack(case, out):
    r, pos = {}, 0
    for name, dt, sh in xu_sizes(case):
        n = np.dtype(dt).itemsize * int(np.prod(sh))
        r[name] = np.frombuffer(out[pos:pos + n].tobytes(), dt).reshape(sh)
        pos += n
    assert pos == len(out)
    r["sc"] = dict(zip(XU_SC, (int(v) for v in r["sc"])))
    return r


def xu_gate(case):
    """The speculative gate: some shard has a gossip slot in use or a region past its inline block."""
    f = 0
    for p in range(case["W"]):
        f |= int(case["rcnt"][p]) | int(case["scnt"][p])
        if int(case["scnt"][p]) & XCNT_MASK > case["XI"] - 8:
            f |= XFLAG_OVER
    return bool(f & (XFLAG_GOSSIP | XFLAG_OVER))


def xu_region(case, p):
    """An independent parse of peer p's region, by the layout: (slot records, round records, [(message words, chunk base,
    mask, log words)], data_off); None if the peer contributes nothing."""
    MW = sd_sizes(case["N"])["MW"]
    if p == case["rank"] or int(case["rcnt"][p]) & XCNT_MASK < 32:
        return None
    Rg = case["recv"][p]
    H = np.frombuffer(Rg[:32].tobytes(), np.uint32)
    nslot, nround, nsync, data_off = (int(H[i]) for i in (0, 1, 2, 4))
    o = 32
    ns = np.frombuffer(Rg[o:o + 4 * NSW * nslot].tobytes(), np.uint32).reshape(nslot, NSW)
    o += 4 * NSW * nslot
    rr = np.frombuffer(Rg[o:o + 4 * RRW * nround].tobytes(), np.uint32).reshape(nround, RRW)
    o += 4 * RRW * nround
    SE, ent = sync_entry_size(MW), []
    for j in range(nsync):
        w = np.frombuffer(Rg[o + SE * j:o + SE * (j + 1)].tobytes(), np.uint32)
        ent.append((w[:SMW], int(w[SMW]), mask_int(w[SMW + 2:SMW + 2 + 2 * MW].view(np.uint64)), w[SMW + 2 + 2 * MW:]))
    return ns, rr, ent, data_off


def xunpack_ref(case):
    """What k_unpack_a leaves (the arrays of xu_unpack, preset to the sentinel), with the indices the atomics hand out
    taken in region order: peers ascending, entries in order. Any other order is as valid; xu_props states what does not
    depend on it."""
    z, fl = sd_sizes(case["N"]), case["flags"]
    N, W, CAP, RX, k = case["N"], case["W"], case["MSGCAP"], case["RXCAP"], case["k"]
    r = {name: np.full(sh, {1: XP_BYTE, 2: 0xA5A5, 4: XP_WORD, 8: XP_WORD64}[np.dtype(dt).itemsize], dt) for name, dt, sh in xu_sizes(case)}
    b, nloc = k & 1, len(case["local"])
    sc = dict(zip(XU_SC, [XP_WORD] * 18))
    sc.update({f"arena{b}": 0, "xn4": nloc, "xn5": 0, "xn6": 0, "err": 0, "halt": 1 if fl & XU_HALTED else 0})
    r.update(sc=sc, m_head=np.full(N, NEVER, np.uint32), xa_scnt=np.array(case["scnt"], np.uint64),
             xa_rcnt=np.array(case["rcnt"], np.uint64))
    if fl & XU_INLINE_IN and not (fl & XU_SPEC and fl & XU_HALTED):
        r["host"] = np.concatenate([case["scnt"], case["rcnt"]]).astype(np.uint64)
    elif fl & XU_INLINE_IN:
        r["xa_rcnt"] = np.full(W, XP_WORD64, np.uint64)
    g = case["gossip"]
    if g is not None:
        r["gudm"][:] = 0
        r["HB"][:] = 0
        r["mem8"][0], r["mem8"][1], r["mem8"][7], r["log3"][1] = g["rtail"], 0, g["log_pos"], g["log_spread"]
    if fl & XU_SPEC and (fl & XU_HALTED or xu_gate(case)):
        if not fl & XU_HALTED:
            sc["halt"] = k + 1
        return r
    mtmp = [msg_words(m) for m in case["local"]]
    xn4, xn5 = nloc, 0
    for p in range(W):
        reg = xu_region(case, p)
        if reg is None:
            continue
        ns, rr, ent, data_off = reg
        for rec in ns:
            gs, origin, kc = int(rec[0]), int(rec[7]), int(rec[4])
            gid, key = int(rec[1]) | int(rec[2]) << 32, int(rec[5]) | int(rec[6]) << 32
            r["slot_gid"][gs], r["slot_key"][gs] = gid, key
            r["slot4"][:, gs] = [int(rec[3]), kc, (kc + g["EXPB"]) & M32, 1]
            r["gudm"][0][gs >> 6] |= np.uint64(1 << (gs & 63))
            if int(rec[3]) != USER_SUBJ and (key >> 32) & 3 == ST_DEAD:
                r["gudm"][1][gs >> 6] |= np.uint64(1 << (gs & 63))
            r["S"][origin][gs] = S16_EVER | (kc & S16_TICK)
            r["HB"][origin][gs >> 6] |= np.uint64(1 << (gs & 63))
            pos = int(r["mem8"][0][origin])
            r["rg"][origin][pos & (g["BCAP"] - 1)] = rg_entry(gs, rounds_before(int(g["first"][origin]), kc, g["gossip_t"]))
            r["mem8"][0][origin] = (pos + 1) & M32
            r["mem8"][1][origin] += 1
        for rec in rr:
            m, cnt = int(rec[0]), int(rec[1])
            lp = int(r["mem8"][7][m])
            pos = lp % g["LOGW"]
            r["mem8"][2][m], r["mem8"][3][m], r["mem8"][4][m], r["mem8"][5][m] = 1, cnt, rec[2], rec[3]
            if lp > 0 and int(r["log3"][1][m][(lp - 1) % g["LOGW"]]) != int(rec[2]):
                r["mem8"][6][m] = k
            r["log3"][0][m][pos], r["log3"][1][m][pos], r["log3"][2][m][pos] = k, rec[2], cnt
            r["T"][m][:cnt] = rec[4:4 + cnt]
            r["log_tg"][m][pos][:cnt] = rec[4:4 + cnt]
            r["mem8"][7][m] = lp + 1
        for mw, base, mask, logw in ent:
            ri, j = xn5, xn4
            xn5, xn4 = xn5 + 1, xn4 + 1
            if ri >= RX or j >= CAP:
                sc["err"] |= E_XCAP
                continue
            m = dict(zip(SM_FIELDS, (int(v) for v in mw)))
            r["rx_mask"][ri] = [(mask >> (64 * w)) & M64 for w in range(z["MW"])]
            r["rx_off"][ri] = p * case["XA_PEER"] + data_off + base * CH * 4
            if fl & XU_ACKRES and m["kind"] & KF_RES and m["tln"] <= TL:
                r["mlog"][j][:m["tln"]] = logw[:m["tln"]]
            m.update(payload=PAY_RX | ri, ncand=0)
            while len(mtmp) < j:
                mtmp.append(np.zeros(SMW, np.uint32))  # a slot a refused entry took: mtmp as it was (zero here)
            mtmp.append(msg_words(m))
    n = min(xn4, CAP)
    while len(mtmp) < n:
        mtmp.append(np.zeros(SMW, np.uint32))
    PIN, PAY, DST, KIND = (SM_FIELDS.index(f) for f in ("pin", "payload", "dst", "kind"))
    used = 0
    for i in range(n):
        r["msgs"][i] = mtmp[i]
        r["msgs"][i][PIN] = NEVER
    for i in range(n):
        if int(r["msgs"][i][KIND]) & KF_DEFER:
            continue
        dst = int(r["msgs"][i][DST])
        old = int(r["m_head"][dst])
        r["m_head"][dst], r["m_next"][i] = i, old
        if old != NEVER:
            for t in (i, old):
                if int(r["msgs"][t][PAY]) == NEVER and int(r["msgs"][t][PIN]) == NEVER:
                    if used < case["AR"]:
                        r["msgs"][t][PIN] = used
                    else:
                        sc["err"] |= E_ARENA
                    used += 1
    sc.update({f"nmsg{b}": n, f"arena{b}": used, "xn4": xn4, "xn5": xn5, "xn6": 32 * W})
    if fl & XU_END:
        sc.update({f"xn{i}": 0 for i in range(8)})
        sc.update({f"nmsg{b ^ 1}": 0, f"arena{b ^ 1}": 0, "pool_used": 0, "rc_n": 0})
        if fl & XU_ACKRES:
            sc.update(ndl=0, ndlw=0)
        r["xa_scnt"][:], r["xb_scnt"][:], r["xdone"][:] = 0, 0, 0
    return r


def xu_props(case, res, holes=0):
    """Properties 1-4 of an unpacked tick, none of which depends on the order the atomics hand out indices in; holes: the
    committed slots that entries refused for want of an rx index took and never wrote (an overflow case only)."""
    z, N, CAP, nloc = sd_sizes(case["N"]), case["N"], case["MSGCAP"], len(case["local"])
    b = case["k"] & 1
    sc, msgs = res["sc"], res["msgs"]
    F = {f: i for i, f in enumerate(SM_FIELDS)}
    total = nloc + len(case["entries"])
    assert sc[f"nmsg{b}"] == min(total, CAP), ("nmsg", sc[f"nmsg{b}"], total, CAP)
    n = min(total, CAP)
    # 1. the local messages were queued before the launch and keep their places; the received ones are a multiset
    for i, m in enumerate(case["local"][:n]):
        want = msg_words(dict(m, pin=int(msgs[i][F["pin"]])))
        assert np.array_equal(msgs[i], want), ("local message", i, msgs[i].tolist(), want.tolist())
    ident = lambda w: tuple(int(v) for j, v in enumerate(w) if SM_FIELDS[j] not in ("payload", "ncand", "pin"))
    expect = {}
    for e in case["entries"]:
        key = ident(msg_words(e["msg"]))
        assert key not in expect, "the case's entries are distinct"
        expect[key] = e
    seen, ris, nhole = set(), set(), 0
    for i in range(nloc, n):
        w = msgs[i]
        if holes and not np.delete(w, F["pin"]).any():
            nhole += 1
            continue
        key = ident(w)
        assert key in expect and key not in seen, ("message", i, "is a complete one from the input, once", w.tolist())
        seen.add(key)
        e, pay = expect[key], int(w[F["payload"]])
        assert pay & PAY_RX and pay != NEVER and int(w[F["ncand"]]) == 0, ("message", i, "payload PAY_RX | ri, ncand 0", hex(pay))
        ri = pay & ~PAY_RX
        assert ri < min(sc["xn5"], case["RXCAP"]) or case["flags"] & XU_END and ri < case["RXCAP"], ("message", i, "ri", ri)
        assert ri not in ris, ("message", i, "ri", ri, "handed out twice")
        ris.add(ri)
        assert mask_int(res["rx_mask"][ri]) == e["mask"], ("message", i, "rx_mask", ri, hex(mask_int(res["rx_mask"][ri])), hex(e["mask"]))
        assert int(res["rx_off"][ri]) == e["off"], ("message", i, "rx_off", ri, int(res["rx_off"][ri]), e["off"])
        if case["flags"] & XU_ACKRES:
            assert np.array_equal(res["mlog"][i][:len(e["log"])], e["log"]), ("message", i, "mlog prefix")
        # 4. payload closure: baseline + shipped chunks = the sender's row, for every subject
        nch = bin(e["mask"]).count("1")
        flat = case["recv"].reshape(-1)[e["off"]:e["off"] + nch * CH * 4]
        ship = np.frombuffer(flat.tobytes(), np.uint32).reshape(nch, CH)
        assert np.array_equal(rx_payload(case["base"], e["mask"], ship)[:N], e["keys"][:N]), ("message", i, "payload closure")
    assert nhole == holes, ("slots taken and never written", nhole, holes)
    if not holes and total <= CAP:
        assert len(seen) == len(expect), "every entry of every region is committed"
    # 2. inbound lists: exactly the non-deferred messages of each member, each list ends
    by_dst = {}
    for i in range(n):
        if not int(msgs[i][F["kind"]]) & KF_DEFER:
            by_dst.setdefault(int(msgs[i][F["dst"]]), set()).add(i)
    heads = {int(m): int(res["m_head"][m]) for m in np.flatnonzero(res["m_head"] != NEVER)}
    assert set(heads) == set(by_dst), ("members with a list", sorted(heads), sorted(by_dst))
    for dst, want in by_dst.items():
        got, qi = [], heads[dst]
        while qi != NEVER and len(got) <= n:
            assert qi < n, ("m_next link", dst, qi)
            got.append(qi)
            qi = int(res["m_next"][qi])
        assert qi == NEVER and len(got) == len(set(got)) and set(got) == want, ("inbound list of", dst, got, sorted(want))
    # 3. pins: a live-row payload of a receiver with two messages or more; at most two live rows per receiver in the cases,
    # so only the second arrival's thread pins and no arena row is lost to a race (pin_msg, dev_util.h)
    pins = []
    for i in range(n):
        w = msgs[i]
        listed = not int(w[F["kind"]]) & KF_DEFER
        must = listed and int(w[F["payload"]]) == NEVER and len(by_dst[int(w[F["dst"]])]) >= 2
        assert (int(w[F["pin"]]) != NEVER) == must, ("pin of message", i, int(w[F["pin"]]), must)
        if must:
            pins.append(int(w[F["pin"]]))
    assert len(set(pins)) == len(pins) and all(p < sc[f"arena{b}"] for p in pins), ("pins", pins, sc[f"arena{b}"])
    assert sc[f"arena{b}"] == len(pins), ("arena_used", sc[f"arena{b}"], len(pins))

def _sender(N, W, p, dsts, seed, n_rows=4, **kw):
    """An XPACK case of rank p whose message i goes from its row i % n_rows to dsts[i]; rows 1 and 3 are dirty."""
    lo = shard_lo(N, W, p)
    nch = sd_sizes(N)["NCHUNK"]
    rows = [([], []), ([0], []), ([], [nch - 1]), ([nch - 1], [])][:n_rows]
    msgs = [xp_msg(i, lo + i % n_rows, d, **(kw.get("msg_kw", {}).get(i, {}))) for i, d in enumerate(dsts)]
    return xp_case(N, W, p, rows, [], msgs, seed, **{k_: v for k_, v in kw.items() if k_ != "msg_kw"})


def xunpack_cases():
    """{name: case}: the regions xpack_ref produces for the XPACK cases as a receiving rank sees them (W = 2, 3 and 8),
    two peers with 300 entries each on top of queued local messages, the pin paths, the region edges, and the gate,
    end-of-tick, overflow and inline variants."""
    xp = xpack_cases()
    g2049 = xu_gossip_state(2049, 81)
    g2049["log_spread"][683][(3 - 1) % 2], g2049["log_spread"][684][(4 - 1) % 2] = 3, 9  # the rounds' spreads are 3, 4, 5:
    # member 683 (log_pos 3) logged the same spread before, 684 (log_pos 4) another one, 1365 (log_pos 0) none
    out = {"n5-w2>1": xu_case(1, {0: xp["n5-w2"]}),
           "n2049>0": xu_case(0, {1: xp["n2049-w3-r1"]}, gossip=g2049),
           "n2049>2-end": xu_case(2, {1: xp["n2049-w3-r1"]}, gossip=g2049, flags=XU_END, k=8),
           "n2049>2-end-ackres": xu_case(2, {1: xp["n2049-w3-r1"]}, gossip=g2049, flags=XU_END | XU_ACKRES),
           "n4100>1": xu_case(1, {0: xp["n4100-batches"]}),
           "ackres>0": xu_case(0, {1: xp["ackres-on"]}, flags=XU_ACKRES)}
    for q in (0, 4, 5, 7):
        out[f"n131073>{q}"] = xu_case(q, {3: xp["n131073-w8-r3"]})
    # two peers, 300 entries each, 20 local messages already queued: 96 blocks contend on xn[4] and xn[5]
    two = {p: _sender(2049, 3, p, [683 + (7 * i + p) % 683 for i in range(300)], 90 + p) for p in (0, 2)}
    loc = [xp_msg(5000 + i, 683 + i, 900 + i) for i in range(20)]
    out["two-peers-300"] = xu_case(1, two, local=loc)
    # overflows of the same tick: MSGCAP less the local messages, then RXCAP, smaller than the entries received
    out["ovf-msgcap"] = xu_case(1, two, local=loc, MSGCAP=520)
    out["ovf-rxcap"] = xu_case(1, two, local=loc, RXCAP=500)
    # pins: receiver 700 gets a local live-row SYNC and a received one; 701 two received; 702 a local arena payload and
    # a received one; 703 a local live row and a delayed received one; 704 two local live rows; 705 one; 700 also a
    # delayed local live row, which is in no list
    snd = _sender(2049, 3, 0, [700, 701, 701, 702, 703], 95, msg_kw={4: dict(kind=1 | KF_DEFER)})
    loc = [xp_msg(6000, 690, 700), xp_msg(6001, 691, 702, payload=3), xp_msg(6002, 692, 703), xp_msg(6003, 693, 704),
           xp_msg(6004, 694, 704, kind=2), xp_msg(6005, 695, 705), xp_msg(6006, 696, 700, kind=1 | KF_DEFER)]
    out["pins"] = xu_case(1, {0: snd}, local=loc)
    # region edges: a peer whose count is below 32 contributes nothing, the own region is ignored even if it holds bytes
    e = xu_case(0, {1: xp["n2049-w3-r1"]}, gossip=g2049)
    rng = np.random.default_rng(96)
    e["recv"][0], e["recv"][2] = rng.integers(0, 256, e["XA_PEER"], dtype=np.uint8), rng.integers(0, 256, e["XA_PEER"], dtype=np.uint8)
    e["rcnt"][0], e["rcnt"][2] = 4096, 24
    out["edges"] = e
    # W = 8 with the gossip plane: every peer of rank 2 created two gossips (one origin both) and ran one round
    send = {}
    for p in (0, 1, 3, 4, 5, 6, 7):
        lo = shard_lo(64, 8, p)
        ns, rr = xp_records(64, [16 * p + 1, 16 * p + 9], [p % 9], 100 + p, origins=[lo + 1, lo + 1], members=[lo + 2])
        send[p] = xp_case(64, 8, p, [([], [])], [], [], 100 + p, ns_rec=ns, rr_rec=rr, xn0=2, xn1=1, used=2)
    out["gossip-w8"] = xu_case(2, send, gossip=xu_gossip_state(64, 82))
    # the speculative gate (k_unpack_a): flags or an oversized sent region stop the launch, nothing else does
    plain = lambda **kw: xu_case(1, {0: xp["n5-w2"]}, **kw)
    out["spec-runs"] = plain(flags=XU_SPEC)
    out["spec-halted"] = plain(flags=XU_SPEC | XU_HALTED)
    out["spec-gossip-received"] = xu_case(0, {1: xp["n2049-w3-r1"]}, gossip=g2049, flags=XU_SPEC)
    for name, arr, p, v in (("spec-over-received", "rcnt", 0, XFLAG_OVER), ("spec-gossip-sent", "scnt", 0, XFLAG_GOSSIP),
                            ("spec-over-sent", "scnt", 1, XFLAG_OVER)):
        c = plain(flags=XU_SPEC)
        c[arr][p] = int(c[arr][p]) | v
        out[name] = c
    c = plain(flags=XU_SPEC)
    c["scnt"][0] = c["XI"]  # past the inline block, without the flag
    out["spec-sent-past-inline"] = c
    c = plain(flags=XU_SPEC)
    c["scnt"][0] = c["XI"] - 8  # exactly the inline block: runs
    out["spec-sent-at-inline"] = c
    # behind k_inline_in: a region that is exactly the inline block, one with a partial chunk, and a halted launch
    out["inline-in-256"] = xu_case(1, {0: xp["inl-xi264"]}, flags=XU_INLINE_IN, XI=264)
    out["inline-in-chunk"] = xu_case(1, {0: xp["n5-w2"]}, flags=XU_INLINE_IN | XU_SPEC, XI=16384)
    out["inline-in-halted"] = xu_case(1, {0: xp["inl-xi264"]}, flags=XU_INLINE_IN | XU_SPEC | XU_HALTED, XI=264)
    return out


# ---- k_pack_b and k_inline_in
PACKB_NDS = [0, 1, 16384, 16385]  # around the 64 x 256 grid stride


def pack_b_ref(W, rank, DCAP, xd_n, XB, xd):
    """(xb_send uint8[W][XB], xb_scnt uint64[W], err) in buffers preset to XP_BYTE: header {nd, 0, 0, 0}, then the
    records; nd clamps to DCAP; records that pass XB_PEER raise E_XCAP and ship a header only."""
    send, scnt, err = np.full((W, XB), XP_BYTE, np.uint8), np.full(W, XP_WORD64, np.uint64), 0
    nd = min(xd_n, DCAP)
    if 16 + 8 * nd > XB:
        err, nd = E_XCAP, 0
    for q in range(W):
        if q != rank:
            send[q][:16] = u32([nd, 0, 0, 0]).view(np.uint8)
            send[q][16:16 + 8 * nd] = np.asarray(xd[:nd], np.uint64).view(np.uint8)
            scnt[q] = 16 + 8 * nd
    return send, scnt, err


def inline_in_ref(W, XI, cap, irecv, scnt, halted):
    """(recv uint8[W][cap], rcnt uint64[W], host uint64[2 W]) in buffers preset to XP_BYTE."""
    recv, rcnt, host = np.full((W, cap), XP_BYTE, np.uint8), np.full(W, XP_WORD64, np.uint64), np.full(2 * W, XP_WORD64, np.uint64)
    if not halted:
        for p in range(W):
            w = int(np.frombuffer(irecv[p][:8].tobytes(), np.uint64)[0])
            n = min(w & XCNT_MASK, XI - 8) // 8 * 8
            recv[p][:n] = irecv[p][8:8 + n]
            rcnt[p], host[p], host[W + p] = w, scnt[p], w
    return recv, rcnt, host


# ---------------------------------------------------------------------------------------------- Philox4x32-10
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over numpy arrays (swim_common.h philox); known answers in tests/test_gpu_c5_scale.py."""
    m = np.uint64(M32)
    c = [np.asarray(x, dtype=np.uint64) & m for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & m, p1 & m, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & m, p0 & m]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m
        k1 = (k1 + np.uint64(0xBB67AE85)) & m
    return c


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# ---------------------------------------------------------------------------------------------- gossip data plane
# SWIM_PRIM_GOSSIP (include/swimhip_debug.h): launch_gossip_send and launch_gossip_apply for one tick k on a holder state
# built here. A state is a dict of the op's params and numpy arrays under the names of engine.h; gs_ref states what the
# tick does to it member by member with Python sets of slot ids, never with the kernels' word arithmetic.
GS_SENT = 0xA5A5A5A5
GS_SENT64 = GS_SENT | GS_SENT << 32
GS_APPLY, GS_EM, GS_FB = 1, 2, 4
CEV, CEVW, HREC, HKEEP, FB_N, SLIFE, APPLY_LANE = 6, 22, 11, 16, 16, 4096, 8
S16_SWEPT, S16_REBORN = 1 << 14, 1 << 15
E_RECEIPTS, E_CONTACTS, E_RING, E_SLIFE = 1024, 2048, 1 << 22, 1 << 25
SALT_LOSS_GOSSIP = 0x474F5353
FB_CEV_SLOW, FB_REPLAY, FB_RX_ALL = 4, 5, 8
GS_PARAMS = ("N", "F", "SLOTS", "BCAP", "LOGW", "lat", "gossip_t", "EXPB", "k", "seed_lo", "seed_hi", "rr_atomic", "cev_cap",
             "CRCAP", "RPCAP", "SLOWCAP", "RCAP", "HCAP", "sort_cap", "rank", "SPR", "flags", "cw", "cb", "cx", "ep_loss", "ep_part")
GS_SC = ("nag", "span", "nrwl", "ntl", "nrx", "rp_n", "slow_n", "rc_n", "nap", "nsg", "nfexp", "free_top", "hist_n", "ncfl",
         "xd_n", "pad")
# the paths of k_round_apply_w / _b one round state runs through (5-word rows and up: cw = 2 sends them to the workgroup
# kernel, cb then gives its chunks); QW is the state's
GS_PATHS = {"atomic": dict(rr_atomic=1 << 31), "wave": dict(rr_atomic=0), "block1": dict(rr_atomic=0, cw=2),
            "block2": dict(rr_atomic=0, cw=2, cb=lambda QW: (QW + 1) // 2 + (QW % 2 == 0)),
            "block3": dict(rr_atomic=0, cw=2, cb=lambda QW: (QW + 2) // 3)}


def gs_layout(c):
    """(in fields, out fields) as (name, dtype, elements); every array starts 8-byte aligned."""
    N, F, SLOTS, BCAP, LOGW = c["N"], c["F"], c["SLOTS"], c["BCAP"], c["LOGW"]
    QW, NF, NL, NS = SLOTS // 64, N * F, N * LOGW, (N + 7) & ~7
    u4, u8 = np.uint32, np.uint64
    inp = [("slot_gid", u8, SLOTS), ("slot_key", u8, SLOTS), ("slot_subj", u4, SLOTS), ("slot_ctick", u4, SLOTS)]
    inp += [(n, u4, N) for n in ("firstGossip", "tround", "tcnt", "tspread", "tperiod", "spchg", "log_pos")]
    inp += [("T", u4, NF), ("log_tick", u4, NL), ("log_spread", u4, NL), ("log_cnt", u4, NL), ("log_tg", u4, NL * F),
            ("ep_group", u4, N), ("leaving", u4, N)]
    if c["flags"] & GS_APPLY:
        inp.append(("rowk", u4, N * NS))
    out = [("GU", u8, QW), ("DM", u8, QW), ("HB", u8, N * QW), ("WB", u8, N * QW), ("RX", u8, c["CRCAP"] * QW), ("rp", u8, c["RPCAP"]),
           ("slow", u8, c["SLOWCAP"]), ("hist", u8, c["HCAP"] * HREC), ("rc_raw", u8, c["RCAP"]), ("rc_key", u8, c["RCAP"]),
           ("ctr_g", u8, 1), ("em", u8, 2 * N), ("fb", u8, FB_N), ("S", np.uint16, N * SLOTS), ("rg", u4, N * BCAP)]
    out += [(n, u4, N) for n in ("dead_tick", "rhead", "rtail", "rwin", "rseen", "held", "rsend", "rwnew", "rt0", "tin_cnt_send",
                                 "tin_cnt", "tin_fill", "tin_off", "dead_rx", "rc_ndrop", "rwl", "tlist", "ap_list", "rc_off",
                                 "rc_cnt", "sg_list")]
    out += [(n, u4, SLOTS) for n in ("slot_exp", "slot_used", "fexp", "free_list")]
    out += [("agroup", u4, QW), ("tin", u4, NF), ("tcontact", u4, NF), ("cin", u4, NF), ("crow", u4, NF), ("cev", u4, NF * CEVW),
            ("rxl", u4, 3 * c["CRCAP"]), ("rc_slot", u4, c["RCAP"]), ("sc", u4, 16), ("err", u4, 8)]
    return inp, out


def _gs_blob(c, fields):
    parts = []
    for name, dt, n in fields:
        if name in c:
            a = np.ascontiguousarray(c[name], dtype=dt).reshape(-1)
        else:  # an output the caller has nothing to say about: the sentinel shows what was not written
            a = np.full(n, GS_SENT64 if dt == np.uint64 else GS_SENT & (0xFFFF if dt == np.uint16 else M32), dt)
        assert a.size == n, (name, a.size, n)
        b = a.view(np.uint8)
        parts.append(b)
        if b.size % 8:
            parts.append(np.zeros(8 - b.size % 8, np.uint8))
    return np.concatenate(parts).view(np.uint64)


def gs_pack(c):
    """(params, in, out) of SWIM_PRIM_GOSSIP for state c."""
    inp, out = gs_layout(c)
    sc = np.full(16, GS_SENT, np.uint32)
    sc[[GS_SC.index("rc_n"), GS_SC.index("hist_n")]] = 0
    sc[GS_SC.index("free_top")] = c["free_top"]
    return [c[p] for p in GS_PARAMS], _gs_blob(c, inp), _gs_blob(dict(c, sc=sc, em=np.zeros(2 * c["N"], np.uint64),
                                                                     fb=np.zeros(FB_N, np.uint64)), out)


def gs_unpack(c, out):
    N, F, SLOTS, BCAP, QW = c["N"], c["F"], c["SLOTS"], c["BCAP"], c["SLOTS"] // 64
    b, o, r = out.view(np.uint8), 0, {}
    for name, dt, n in gs_layout(c)[1]:
        nb = n * np.dtype(dt).itemsize
        r[name] = b[o:o + nb].view(dt).copy()
        o += (nb + 7) & ~7
    assert o == b.size
    for name, shape in (("HB", (N, QW)), ("WB", (N, QW)), ("S", (N, SLOTS)), ("rg", (N, BCAP)), ("RX", (c["CRCAP"], QW)),
                        ("cev", (N * F, CEVW)), ("hist", (c["HCAP"], HREC)), ("rxl", (c["CRCAP"], 3))):
        r[name] = r[name].reshape(shape)
    r.update({n: int(r["sc"][i]) for i, n in enumerate(GS_SC)})
    r["free_top"] -= (r["free_top"] >> 31) << 32
    return r


def gs_bits(words):
    """The set of bit indices set in a row of u64 words."""
    out = set()
    for q, w in enumerate(np.asarray(words).tolist()):
        while w:
            b = w & -w
            out.add(q * 64 + b.bit_length() - 1)
            w ^= b
    return out


def gs_words(slots, QW):
    row = [0] * QW
    for g in slots:
        row[g >> 6] |= 1 << (g & 63)
    return np.array(row, np.uint64)


def gs_new(N, SLOTS, k=9000, F=8, BCAP=64, LOGW=4, **kw):
    """An idle plane: no slot in use, every ring empty, no round this tick, empty round logs."""
    c = dict(N=N, F=F, SLOTS=SLOTS, BCAP=BCAP, LOGW=LOGW, lat=1, gossip_t=2, EXPB=40, k=k, seed_lo=0x1234ABCD, seed_hi=0x0BADF00D,
             rr_atomic=64, cev_cap=CEV, CRCAP=8, RPCAP=64, SLOWCAP=64, RCAP=64, HCAP=64, sort_cap=64, rank=0, SPR=SLOTS, flags=0,
             cw=0, cb=0, cx=0, ep_loss=0, ep_part=0, free_top=0)
    c.update(kw)
    QW, NS = SLOTS // 64, (N + 7) & ~7
    z = lambda *s: np.zeros(s, np.uint32)
    c.update(slot_gid=np.zeros(SLOTS, np.uint64), slot_key=np.zeros(SLOTS, np.uint64), slot_subj=np.full(SLOTS, USER_SUBJ, np.uint32),
             slot_ctick=z(SLOTS), firstGossip=z(N), tround=z(N), tcnt=z(N), tspread=z(N), tperiod=z(N), spchg=z(N), log_pos=z(N),
             T=np.full((N, F), NEVER, np.uint32), log_tick=np.full((N, LOGW), NEVER, np.uint32), log_spread=z(N, LOGW),
             log_cnt=z(N, LOGW), log_tg=np.full((N, LOGW, F), NEVER, np.uint32), ep_group=z(N), leaving=z(N), rowk=z(N, NS),
             GU=np.zeros(QW, np.uint64), DM=np.zeros(QW, np.uint64), HB=np.zeros((N, QW), np.uint64), WB=np.zeros((N, QW), np.uint64),
             hist=np.zeros((c["HCAP"], HREC), np.uint64), S=np.zeros((N, SLOTS), np.uint16), rg=np.full((N, BCAP), GS_SENT, np.uint32),
             dead_tick=np.full(N, NEVER, np.uint32), rhead=z(N), rtail=z(N), rwin=z(N), rseen=z(N), held=z(N), dead_rx=z(N),
             rc_ndrop=z(N), slot_exp=z(SLOTS), slot_used=z(SLOTS), free_list=np.full(SLOTS, GS_SENT, np.uint32))
    return c


def gs_variant(c, **kw):
    """The same state with other params (arrays shared: no reference or launch writes them)."""
    v = dict(c)
    for n, x in kw.items():
        v[n] = x(c["SLOTS"] // 64) if callable(x) else x
    return v


def gs_use(c, g, gid, subj=USER_SUBJ, key=0, ctick=None, exp=None):
    """Slot g carries gossip gid (created at ctick, recycled at exp); a DEAD membership record sets its DM bit."""
    c["slot_gid"][g], c["slot_subj"][g], c["slot_key"][g], c["slot_used"][g] = gid, subj, key, 1
    c["slot_ctick"][g] = c["k"] - 20 if ctick is None else ctick
    c["slot_exp"][g] = c["k"] + 30 if exp is None else exp
    c["GU"][g >> 6] |= np.uint64(1 << (g & 63))
    if subj != USER_SUBJ and (key >> 32) & 3 == ST_DEAD:
        c["DM"][g >> 6] |= np.uint64(1 << (g & 63))


def gs_hold(c, m, g, period, ctick=None):
    """Member m received slot g's gossip in its gossip period `period` (at tick ctick): ring entry, held bit, S entry."""
    p = int(c["rtail"][m])
    c["rg"][m][p & (c["BCAP"] - 1)] = rg_entry(g, period)
    c["rtail"][m] = (p + 1) & M32
    c["HB"][m][g >> 6] |= np.uint64(1 << (g & 63))
    c["S"][m][g] = S16_EVER | ((c["k"] - 10 if ctick is None else ctick) & S16_TICK)
    c["held"][m] += 1


def gs_seen(c, m, win, seen):
    """m's previous round left its window at ring offsets [win, seen) from rhead (entries past `seen` arrived since)."""
    h = int(c["rhead"][m])
    c["rwin"][m], c["rseen"][m] = (h + win) & M32, (h + seen) & M32
    c["WB"][m] = gs_words([s for _, s, _ in gs_ring(c, m)[win:seen]], c["SLOTS"] // 64)


def gs_round(c, m, P, spread, targets=()):
    c["tround"][m], c["tperiod"][m], c["tspread"][m], c["tcnt"][m] = 1, P, spread, len(targets)
    c["T"][m][:len(targets)] = targets
    c["firstGossip"][m] = c["k"] - P * c["gossip_t"]  # rounds_before(m, k) = P


def gs_period(tag, P):
    """The one period within 512 of P whose low 10 bits are `tag`."""
    return P + ((tag - P + 512) % 1024) - 512


def gs_ring(c, m, P=None):
    """m's live ring entries in order: (absolute position, slot, period as seen from period P)."""
    P = int(c["tperiod"][m]) if P is None else P
    h, n = int(c["rhead"][m]), (int(c["rtail"][m]) - int(c["rhead"][m])) & M32
    es = [int(c["rg"][m][((h + j) & M32) & (c["BCAP"] - 1)]) for j in range(n)]
    return [((h + j) & M32, e & RG_SLOT, gs_period(e >> 22, P)) for j, e in enumerate(es)]


def gs_round_ref(c, m):
    """Member m's round by classifying each ring entry: None if m has no round or the round changes nothing, else
    dict(send, wnew, swept slots, window slots)."""
    if not c["tround"][m]:
        return None
    P, sp, ring = int(c["tperiod"][m]), int(c["tspread"][m]), gs_ring(c, m)
    swept = [s for _, s, p in ring if p < P - 2 * (sp + 1)]
    before = [s for _, s, p in ring if p < P - sp]
    h, tl = int(c["rhead"][m]), int(c["rtail"][m])
    send, wnew = (h + len(swept)) & M32, (h + len(before)) & M32
    if send == h and wnew == int(c["rwin"][m]) and int(c["rseen"][m]) == tl:
        return None
    return dict(send=send, wnew=wnew, swept=swept, window=[s for _, s, _ in ring[len(before):]])


def gs_round_ref_ranges(c, m):
    """The same by searching the sorted periods (the second formulation test_prim_ref.py compares with)."""
    if not c["tround"][m]:
        return None
    P, sp, ring = int(c["tperiod"][m]), int(c["tspread"][m]), gs_ring(c, m)
    per = np.array([p for _, _, p in ring], np.int64)
    a, b = int(np.searchsorted(per, P - 2 * (sp + 1), "left")), int(np.searchsorted(per, P - sp, "left"))
    h = int(c["rhead"][m])
    if a == 0 and (h + b) & M32 == int(c["rwin"][m]) and c["rseen"][m] == c["rtail"][m]:
        return None
    slots = [s for _, s, _ in ring]
    return dict(send=(h + a) & M32, wnew=(h + b) & M32, swept=slots[:a], window=slots[b:])


def gs_pct(c, m, t):
    """NetworkEmulator's loss percent of a send m -> t at tick k."""
    if c["k"] >= c["dead_tick"][t] or (c["ep_part"] and c["ep_group"][m] != c["ep_group"][t]):
        return 100
    return c["ep_loss"]


def gs_lost(c, m, s, slots, pct):
    """Which of m's sends of `slots` through target slot s are lost (LOSS_GOSSIP draw, SEMANTICS.md §2)."""
    slots = list(slots)
    if pct == 0 or not slots:
        return set()
    if pct >= 100:
        return set(slots)
    gid = c["slot_gid"][slots]
    r = philox(np.full(len(slots), m), c["k"] ^ ((s >> 2) << 31), gid >> np.uint64(32), gid & np.uint64(M32),
               c["seed_lo"] ^ SALT_LOSS_GOSSIP, c["seed_hi"])[s & 3]
    return {g for g, x in zip(slots, ((r * np.uint64(100)) >> np.uint64(32)).tolist()) if x < pct}


def gs_s_get(c, e, g, ref):
    """The creation tick of S entry e of slot g read at tick ref, or None when it reads as never held."""
    if not e & S16_EVER:
        return None
    t = ref - ((ref - (e & S16_TICK)) & S16_TICK)
    return None if t < c["slot_ctick"][g] else t


def gs_overrides(s1, i1, s0, i0):
    """MembershipRecord.isOverrides (ABSENT 0, ALIVE 1, SUSPECT 2, DEAD 3)."""
    if s0 == 0:
        return s1 == 1
    if s0 == 3:
        return False
    if s1 == 3:
        return True
    return s1 == 2 and s0 != 2 if i1 == i0 else i1 > i0


def gs_hist_tag(gid, member):
    return mix64(gid ^ ((member * 0x9E3779B97F4A7C15) & M64)) | 1


def gs_hist_decode(hist):
    """{(gid, member): (n, creation ticks kept)} of an incarnation-history table."""
    out = {}
    for e in np.asarray(hist).reshape(-1, HREC):
        if int(e[0]):
            gid, member, n = int(e[1]), int(e[2]) & M32, int(e[2]) >> 32
            assert int(e[0]) == gs_hist_tag(gid, member) and (gid, member) not in out
            out[gid, member] = (n, tuple(e[3:].view(np.uint32)[:min(n, HKEEP)].tolist()))
    return out


def gs_events(c, m, t):
    """The contact events of the pair (m, T[m][s] = t) up to tick k - lat in both round logs, in the order (tick, side,
    target slot): (tick, side, slot, the round's spread, loss percent, sender's rounds before it); side 0 is t -> m. And the
    oldest tick of each wrapped log (0: never wrapped)."""
    ev, oldest = [], []
    for side, (frm, to) in enumerate(((t, m), (m, t))):
        for e in range(c["LOGW"]):
            t2 = int(c["log_tick"][frm][e])
            if t2 == NEVER or t2 + c["lat"] > c["k"]:
                continue
            for s2 in range(int(c["log_cnt"][frm][e])):
                if c["log_tg"][frm][e][s2] == to:
                    pct = 100 if t2 >= c["dead_tick"][to] or (c["ep_part"] and c["ep_group"][frm] != c["ep_group"][to]) else c["ep_loss"]
                    ev.append((t2, side, s2, int(c["log_spread"][frm][e]), pct,
                               rounds_before(int(c["firstGossip"][frm]), t2, c["gossip_t"])))
        ticks = [int(x) for x in c["log_tick"][frm] if x != NEVER]
        oldest.append(min(ticks) if c["log_pos"][frm] > c["LOGW"] and ticks else 0)
    return sorted(ev), oldest


def gs_contacts_ref(c, r, window, rows=None):
    """The contact stage for this tick's pairs. window[m]: m's window entries after its round as (slot, period) in ring
    order. rows: the pairs that got an RX row when more than CRCAP wanted one (which ones is an atomic's order)."""
    k, lat, gt, F = c["k"], c["lat"], c["gossip_t"], c["F"]
    r.update(tcontact={}, cin={}, crow={}, cev={}, rx={}, fb=np.zeros(FB_N, np.int64))
    split = []
    for t, mss in r["tin"].items():
        for ms in mss:
            m = ms // F
            cut = k - (int(c["tspread"][m]) + 1) * gt - lat
            hit = any(t2 != NEVER and cut < t2 < k and m in c["log_tg"][t][e][:c["log_cnt"][t][e]].tolist()
                      for e, t2 in enumerate(c["log_tick"][t].tolist()))
            r["tcontact"][ms], r["cin"][ms] = int(hit), NEVER
            if not hit:
                continue
            ev, oldest = gs_events(c, m, t)
            over = len(ev) > min(CEV, c["cev_cap"])
            ins = [e[0] for e in ev if e[1] == 0]
            rec = [CEV + 1 if over else len(ev), oldest[0], oldest[1], NEVER if over or not ins else ins[-1]]
            if not over:
                for t2, side, s2, sp, pct, rb in ev:
                    rec += [t2, s2 | side << 8 | pct << 9 | sp << 16, rb]
            r["cev"][ms], r["crow"][ms] = rec, NEVER  # RX_ALL
            if over:
                r["cin"][ms] = 0xFFFFFFFE  # CIN_SLOW
                continue
            last_in = ins[-1]  # a flagged pair has one after the horizon
            b1 = rounds_before(int(c["firstGossip"][m]), last_in + lat + 1, gt)
            early = [g for g, p in window[m] if p <= b1]
            if early:
                r["cin"][ms] = last_in
                if len(early) < len(window[m]):
                    split.append((ms, early))
    r["nrx"] = len(split)
    granted = [ms for ms, _ in split][:c["CRCAP"]] if rows is None else sorted(rows)
    assert len(granted) == min(len(split), c["CRCAP"]) and set(granted) <= {ms for ms, _ in split}
    for ms, early in split:
        if ms in granted:
            r["rx"][ms] = (int(r["rwin"][ms // F]), (int(r["rwin"][ms // F]) + len(early)) & M32, set(early))
        else:
            r["fb"][FB_RX_ALL] += 1
    r["ncfl"] = sum(r["tcontact"].values())


def gs_ref(c, rows=None, dropped=()):
    """What one tick leaves. Sends of pairs with a logged contact are diverted to the replay lists; here every diverted
    gossip is one its target never held, so the replay's answer is `not in infectedFrom`: it is sent. rows, dropped: the
    outcomes of the two capacity races (gs_contacts_ref; the list entries that found no place), taken from the run."""
    N, F, QW, k, lat = c["N"], c["F"], c["SLOTS"] // 64, c["k"], c["lat"]
    r = dict(err=0)
    active = [q for q in range(QW) if c["GU"][q]]
    r["agroup"], r["nag"], r["span"] = active, len(active), active[-1] + 1 if active else 0
    # ---- rounds
    HB, WB = [gs_bits(c["HB"][m]) for m in range(N)], [gs_bits(c["WB"][m]) for m in range(N)]
    S = c["S"].copy()
    for n in ("rhead", "rwin", "rseen", "held", "dead_tick", "dead_rx", "slot_exp", "slot_used", "rc_ndrop"):
        r[n] = c[n].astype(np.int64)
    r["rwl"], r["rsend"], r["rwnew"] = set(), {}, {}
    for m in range(N):
        rr = gs_round_ref(c, m)
        if rr is None:
            continue
        r["rwl"].add(m)
        r["rsend"][m], r["rwnew"][m] = rr["send"], rr["wnew"]
        HB[m] -= set(rr["swept"])
        WB[m] = set(rr["window"])
        for g in rr["swept"]:
            S[m][g] |= S16_SWEPT
            if c["slot_gid"][g] >> np.uint64(32) == m and c["slot_subj"][g] == m and (int(c["slot_key"][g]) >> 32) & 3 == ST_DEAD:
                r["dead_tick"][m] = k + 1  # its own leave notification: the leave completes
        r["rhead"][m], r["rwin"][m], r["rseen"][m] = rr["send"], rr["wnew"], c["rtail"][m]
        r["held"][m] -= len(rr["swept"])
    # ---- scatter
    pairs = [(int(c["T"][m][s]), m * F + s) for m in range(N) if c["tround"][m] for s in range(int(c["tcnt"][m]))]
    r["tin"] = {t: sorted(ms for t2, ms in pairs if t2 == t) for t in set(t for t, _ in pairs)}
    r["tin_cnt"] = np.array([len(r["tin"].get(t, ())) for t in range(N)], np.uint32)
    r["tin_off"] = np.concatenate([[0], np.cumsum(r["tin_cnt"])[:-1]]).astype(np.uint32)
    r["tlist"] = set(r["tin"])
    r["rt0"] = {t: int(c["rtail"][t]) for t in r["tlist"]}
    # ---- sends
    r["new"], r["tag"], sends = {}, {}, 0
    em = np.zeros(2 * N, np.int64)
    dm = gs_bits(c["DM"])
    r["rtail"] = c["rtail"].astype(np.int64)
    window = []
    for m in range(N):  # the window entries [rwin', rseen') in ring order
        ring, a, n = gs_ring(c, m), (int(r["rwin"][m]) - int(c["rhead"][m])) & M32, (int(r["rseen"][m]) - int(r["rwin"][m])) & M32
        window.append([(g, p) for _, g, p in ring[a:a + n]])
        assert {g for g, _ in window[m]} == WB[m]
    gs_contacts_ref(c, r, window, rows)
    r["rp"], r["slow"] = [], []
    for t in sorted(r["tlist"]):
        new = set()
        for ms in r["tin"][t]:
            m, s = divmod(ms, F)
            sent = set(WB[m])
            if r["cin"][ms] != NEVER:
                slow = r["cin"][ms] == 0xFFFFFFFE
                wr = WB[m] & r["rx"][ms][2] if ms in r["rx"] else set(WB[m])
                if wr:
                    r["fb"][FB_CEV_SLOW if slow else FB_REPLAY] += len(wr)
                    r["slow" if slow else "rp"] += [(g << 32) | ms for g in wr]
                for g in wr:  # isInfected (:247): the explicit set if the case has one; else nobody who never held it
                    if "infected" in c:
                        sent -= {g} if t in c["infected"][m, g] else set()
                    elif gs_s_get(c, int(c["S"][t][g]), g, k + lat) is not None:
                        raise NotImplementedError("a replayed gossip its target held: the answer needs the pair's history")
                sent -= {g for g in wr if (g << 32) | ms in dropped}
            sends += len(sent)
            pct = gs_pct(c, m, t)
            if c["flags"] & GS_EM and k < c["dead_tick"][t]:  # a dead target refuses the connection: not counted
                nl = len(gs_lost(c, m, s, sent, pct))
                em[2 * m] += 2 * len(sent) - nl
                em[2 * m + 1] += nl
            cand = sent - HB[t]
            new |= cand - gs_lost(c, m, s, cand, pct)
        r["new"][t], r["tag"][t] = new, rounds_before(int(c["firstGossip"][t]), k + lat, c["gossip_t"]) & 1023
        HB[t] |= new
        r["rtail"][t] = (r["rt0"][t] + len(new)) & M32
        if new & dm:
            r["dead_rx"][t] = k + lat
        if (r["rtail"][t] - r["rhead"][t]) & M32 > c["BCAP"]:
            r["err"] |= E_RING
    r["ctr_g"], r["em"], r["HB"], r["WB"] = sends, em, HB, WB
    if len(r["rp"]) > c["RPCAP"] or len(r["slow"]) > c["SLOWCAP"]:
        r["err"] |= E_CONTACTS
    if not c["flags"] & GS_FB:
        r["fb"][:] = 0
    r["tin_cnt_send"] = r["tin_cnt"]
    if not c["flags"] & GS_APPLY:
        r["tin_fill"], r["S"] = r["tin_cnt"], S
        return r
    # ---- apply
    r["tin_cnt"] = r["tin_fill"] = np.zeros(N, np.uint32)
    routed, hist = [], {kk: list(v[1]) for kk, v in gs_hist_decode(c["hist"]).items()}
    r["hist_old"] = set(hist)
    for t in sorted(r["tlist"]):
        for g in sorted(r["new"][t]):
            prev = gs_s_get(c, int(S[t][g]), g, k + lat)
            S[t][g] = S16_EVER | ((k + lat) & S16_TICK) | (S16_REBORN if prev is not None else 0)
            if prev is not None:
                hist.setdefault((int(c["slot_gid"][g]), t), []).append(prev)
            r["slot_exp"][g] = k + lat + c["EXPB"]
            subj, key = int(c["slot_subj"][g]), int(c["slot_key"][g])
            if subj == USER_SUBJ:
                route = True
            else:
                r0 = int(c["rowk"][t][subj])
                route = (r0 & 3 == 0 or gs_overrides((key >> 32) & 3, key & M32, r0 & 3, r0 >> 2) or r["dead_rx"][t] == k + lat
                         or bool(c["leaving"][subj]))
            if route:
                routed.append((t << 32) | g)
            else:
                r["rc_ndrop"][t] += 1
        r["held"][t] += len(r["new"][t])
    r["S"], r["routed"], r["hist"] = S, sorted(routed), {kk: (len(v), tuple(v)) for kk, v in hist.items()}
    r["ap"] = {t for t in r["tlist"] if len(r["new"][t]) > APPLY_LANE}
    if len(routed) > c["RCAP"]:
        r["err"] |= E_RECEIPTS
    # ---- expire and free
    gone = sorted(g for g in gs_bits(c["GU"]) if r["slot_exp"][g] <= k)
    if any(((k - int(c["slot_ctick"][g])) & M32) > SLIFE for g in gs_bits(c["GU"])):
        r["err"] |= E_SLIFE
    r["GU"], r["DM"] = gs_bits(c["GU"]) - set(gone), dm - set(gone)
    r["slot_used"][gone] = 0
    r["fexp"], r["free"] = gone, [g for g in gone if g // c["SPR"] == c["rank"]]
    return r


def gs_invariants(c):
    """The conditions a state of the engine meets between ticks; a list of the violations."""
    bad, used = [], gs_bits(c["GU"])
    for g in range(c["SLOTS"]):
        if c["slot_used"][g] and g not in used:
            bad.append(("used slot without its GU bit", g))
    if not gs_bits(c["DM"]) <= used:
        bad.append("DM bit of a free slot")
    for m in range(c["N"]):
        ring = gs_ring(c, m, rounds_before(int(c["firstGossip"][m]), c["k"], c["gossip_t"]))
        slots, per = [s for _, s, _ in ring], [p for _, _, p in ring]
        h, n = int(c["rhead"][m]), len(ring)
        w, s = (int(c["rwin"][m]) - h) & M32, (int(c["rseen"][m]) - h) & M32
        if n > c["BCAP"] or not w <= s <= n:
            bad.append(("ring positions", m))
            continue
        if per != sorted(per):
            bad.append(("ring periods decrease", m))
        if len(set(slots)) != n or not set(slots) <= used:
            bad.append(("ring slots repeat or are free", m))
        if gs_bits(c["HB"][m]) != set(slots):
            bad.append(("HB is not the ring's slots", m))
        if gs_bits(c["WB"][m]) != set(slots[w:s]):
            bad.append(("WB is not the slots of [rwin, rseen)", m))
        if c["held"][m] != n:
            bad.append(("held", m))
        if any(not c["S"][m][g] & S16_EVER or c["S"][m][g] & S16_SWEPT for g in slots):
            bad.append(("S entry of a held slot", m))
        if c["tround"][m] and (c["tcnt"][m] > c["F"] or any(t >= c["N"] or t == m for t in c["T"][m][:c["tcnt"][m]])):
            bad.append(("round targets", m))
        ticks = sorted(int(t) for t in c["log_tick"][m] if t != NEVER)
        if any(b - a < c["gossip_t"] for a, b in zip(ticks, ticks[1:])) or (ticks and ticks[-1] >= c["k"]):
            bad.append(("log ticks closer than a gossip interval", m))
    return bad


# ---- case builders (fixed seeds; test_prim_ref.py checks every one against gs_invariants)
GS_GROUP_QWS = [1, 2, 64, 1024, 1025, 2049]  # one scan batch, its last thread, a second batch, a third with one word
GS_GROUP_KINDS = ["empty", "full", "last", "every7"]


def gs_group_case(QW, kind):
    """One member, no rings: only the group words matter (and the counters k_gossip_groups resets)."""
    c = gs_new(1, 64 * QW)
    words = {"empty": [], "full": range(QW), "last": [QW - 1], "every7": range(0, QW, 7)}[kind]
    for q in words:
        c["GU"][q] = M64 if kind == "full" else 1 << (q % 64)
    c["slot_used"][sorted(gs_bits(c["GU"]))] = 1
    return c


def _gs_fill(c, m, periods, slots, gid0=1 << 40):
    for g, p in zip(slots, periods):
        if not c["slot_used"][g]:
            gs_use(c, g, gid0 + g)
        gs_hold(c, m, g, p)


def gs_prev_window(c, m, Pprev, sp_prev, nnew):
    """m's window as its previous round (period Pprev, spread sp_prev) left it; the last nnew entries arrived since."""
    ring = gs_ring(c, m, Pprev)
    gs_seen(c, m, sum(1 for _, _, p in ring[:len(ring) - nnew] if p < Pprev - sp_prev), len(ring) - nnew)


def gs_rounds_edges():
    """Round members at every boundary of the sweep and the window (spread 2: swept below P - 6, window from P - 2), for
    periods on both sides of the 10-bit tag wrap; rings that cross a multiple of BCAP and 2^32; a spread that grew and one
    that shrank since the previous round; a round with nothing to do; a completed leave. 5-word rows, the last one active."""
    c = gs_new(12, 320, BCAP=64)
    m, free = 0, iter(range(320))
    for P in (5, 1023, 1024, 1030, 3071):
        sp = 2
        per = [p for p in (P - 9, P - 8, P - 7, P - 6, P - 5, P - 3, P - 2, P - 1, P, P) if p >= 0]
        c["rhead"][m] = c["rtail"][m] = (60, 0xFFFFFFF0, 0, 7, 0xFFFFFFFF)[m]
        _gs_fill(c, m, per, [next(free) for _ in per])
        gs_round(c, m, P, sp)
        gs_prev_window(c, m, P - 1, sp, 2)
        m += 1
    # the spread grew from 1 to 4 (entries re-enter the window), and shrank from 4 to 1
    for sp0, sp1 in ((1, 4), (4, 1)):
        P = 2000
        per = [P - 12, P - 7, P - 5, P - 4, P - 3, P - 2, P - 1, P - 1]
        _gs_fill(c, m, per, [next(free) for _ in per])
        gs_round(c, m, P, sp1)
        gs_prev_window(c, m, P - 1, sp0, 1)
        m += 1
    # nothing to do: the previous round was this very plan and nothing arrived (not listed, nothing moves)
    P = 700
    _gs_fill(c, m, [P - 6, P - 2, P - 1], [next(free) for _ in range(3)])
    gs_round(c, m, P, 2)
    gs_prev_window(c, m, P, 2, 0)
    idle = m
    m += 1
    # the leave completion: the swept entry is m's own DEAD record
    g = next(free)
    gs_use(c, g, (m << 32) | 5, subj=m, key=(ST_DEAD << 32) | 3)
    _gs_fill(c, m, [10, 30], [g, next(free)])
    gs_round(c, m, 30, 2)
    gs_prev_window(c, m, 29, 2, 0)
    leaver = m
    m += 1
    # a member without a round whose ring looks like work (not touched), and one holding the last slot (the span)
    _gs_fill(c, m, [1, 2, 3], [next(free) for _ in range(3)])
    c["firstGossip"][m] = c["k"] - 40 * c["gossip_t"]
    gs_seen(c, m, 0, 1)
    m += 1
    _gs_fill(c, m, [8, 9], [318, 319])
    gs_round(c, m, 9, 3)
    gs_prev_window(c, m, 8, 3, 1)
    c["idle"], c["leaver"] = idle, leaver
    return c


GS_SWEEP_NS = [1, 63, 64, 65, 255, 256, 257, 1025]


def gs_rounds_sweeps():
    """Member i sweeps GS_SWEEP_NS[i] entries and keeps 3 (ring_walk's four-deep unroll and remainder, on 64 and on 256
    threads); 17-word rows. The rings start just below 2^32."""
    c = gs_new(len(GS_SWEEP_NS), 64 * 17, BCAP=2048)
    for g in range(c["SLOTS"]):
        gs_use(c, g, (9 << 32) | g)
    rng = np.random.default_rng(77)
    for m, n in enumerate(GS_SWEEP_NS):
        P = 900 + m
        c["rhead"][m] = c["rtail"][m] = (0xFFFFFC00 + 37 * m) & M32
        slots = rng.permutation(c["SLOTS"])[:n + 3].tolist()
        _gs_fill(c, m, [P - 30] * n + [P - 4, P - 1, P], slots)
        gs_round(c, m, P, 2)
        gs_prev_window(c, m, P - 20, 2, 1)  # the swept entries were in the window then
    return c


def gs_rounds_empty():
    """span = 0: no slot in use, round members with empty rings."""
    c = gs_new(3, 320)
    gs_round(c, 0, 10, 2)
    gs_round(c, 2, 11, 2)
    return c


def gs_scatter_case():
    """600 members (block_reserve crosses workgroups), F = 8: target 7 has 40 senders, 9 two, 11 one whose send is slot 7 of
    a full round; members with fewer targets than F, with an empty round and without a round."""
    c = gs_new(600, 64)
    rng = np.random.default_rng(5)
    for m in range(100, 140):
        gs_round(c, m, 50, 2, [7] + rng.choice(np.arange(300, 600), int(rng.integers(0, 4)), replace=False).tolist())
    gs_round(c, 20, 50, 2, [9])
    gs_round(c, 21, 50, 2, [250, 9, 251])
    gs_round(c, 22, 50, 2, [252, 253, 254, 255, 256, 257, 258, 11])
    gs_round(c, 23, 50, 2, [])
    for m in range(300, 600, 3):
        gs_round(c, m, 50, 2, rng.choice(np.arange(0, 100), int(rng.integers(1, 8)), replace=False).tolist())
    return c


def gs_send_case(nag, ntl, seed, QW=None, hold=0.5, BCAP=1024, **kw):
    """ntl targets with 1..3 senders each over nag active groups; every member has a round, holds about `hold` of the
    gossips (so windows overlap and targets hold some), a dead target, DEAD membership records among the gossips."""
    rng = np.random.default_rng(seed)
    QW = QW or (nag + 2 if nag > 1 else 1)
    N = ntl + 4
    c = gs_new(N, 64 * QW, BCAP=BCAP, **kw)
    c["rowk"] = rng.integers(0, 16, (N, (N + 7) & ~7)).astype(np.uint32)  # status | inc << 2
    groups = sorted(rng.choice(QW - 1, nag - 1, replace=False).tolist() + [QW - 1]) if nag > 1 else [0]
    slots = []
    for i, q in enumerate(groups):
        bits = range(64) if i == 0 else rng.choice(64, int(rng.integers(1, 5)), replace=False).tolist()
        slots += [q * 64 + b for b in bits]
    for g in slots:
        kind = rng.integers(0, 4)
        subj = USER_SUBJ if kind == 0 else int(rng.integers(0, N))
        key = int(rng.integers(0, 2**32)) | int(rng.integers(0, 2**32)) << 32 if kind == 0 else \
            (int(rng.integers(1, 4)) << 32) | int(rng.integers(0, 4))
        gs_use(c, g, int(rng.integers(1, 2**63)), subj, key, ctick=c["k"] - int(rng.integers(5, 30)))
    c["leaving"][rng.choice(N, 2, replace=False)] = 1
    c["ep_group"][:] = np.arange(N) % 2
    cap = [c["F"]] * N
    targets = [[] for _ in range(N)]
    for t in range(ntl):
        want = 1 + t % 3
        for m in rng.permutation(N).tolist():
            if want and m != t and cap[m] and t not in targets[m]:
                targets[m].append(t)
                cap[m] -= 1
                want -= 1
        assert want == 0
    for m in range(N):
        P, sp = 300 + 7 * m, 2 + m % 3
        mine = [g for g in slots if rng.random() < hold]
        rng.shuffle(mine)
        per = sorted(int(P - min(rng.integers(0, 2 * sp + 2), rng.integers(0, 2 * sp + 6))) for _ in mine)
        c["rhead"][m] = c["rtail"][m] = int(rng.integers(0, 2**32))
        for g, p in zip(mine, per):
            gs_hold(c, m, g, p, ctick=max(int(c["slot_ctick"][g]), c["k"] - 2 * (P - p) - 1))
        gs_round(c, m, P, sp, targets[m])
        gs_prev_window(c, m, P - 1, sp, min(len(mine), int(rng.integers(0, 3))))
        # entries of earlier incarnations and of the slots' earlier gossips in the rows of S the apply reads
        for g in rng.choice(slots, min(len(slots), 12), replace=False).tolist():
            if g not in mine:
                old = rng.random() < 0.5
                tick = int(c["slot_ctick"][g]) - 3 if old else int(c["slot_ctick"][g]) + 1
                c["S"][m][g] = S16_EVER | S16_SWEPT | (tick & S16_TICK)
    c["dead_tick"][ntl // 2] = c["k"] - 3
    c["targets"] = ntl
    return c


GS_SEND_SHAPES = {"nag1": (1, 70), "nag3": (3, 30), "nag64": (64, 3), "nag65": (65, 3)}


def gs_apply_case(RCAP=None, slife=False):
    """Targets 0..6 gain 0, 1, 8, 9, 64, 65 and 4096 + 65 entries from one lossless sender each (member 7 + i); gossips of
    every routing kind, rebirths and stale S entries, slots that expire at k - 1, k, k + 1, in and out of rank 1's range."""
    gains = [0, 1, 8, 9, 64, 65, 4096 + 65]
    rng = np.random.default_rng(99)
    N, SLOTS = 14, 64 * 70
    c = gs_new(N, SLOTS, BCAP=8192, flags=GS_APPLY, RCAP=RCAP or 8192, sort_cap=64, rank=1, SPR=SLOTS // 2, free_top=3, HCAP=4096,
               lat=1, EXPB=40)
    c["rowk"] = rng.integers(0, 16, (N, 16)).astype(np.uint32)
    c["rowk"][:, ::2] |= 3  # every other subject DEAD in every row: no record overrides it
    c["leaving"][[2, 9]] = 1
    pool = rng.permutation([g for g in range(64, SLOTS) if not 2240 <= g < 2245]).tolist()  # the others: the expiry slots
    for i, n in enumerate(gains):
        t, m = i, 7 + i
        P = 400 + i
        own = [pool.pop() for _ in range(n)]
        both = [pool.pop() for _ in range(3)]  # held by the target too: no receipt
        for g in own + both:
            kind = rng.integers(0, 3)
            subj = USER_SUBJ if kind == 0 else int(rng.integers(0, N))
            # DEAD records (their receipt stamps dead_rx: every receipt of the target is routed) only to target 5
            key = int(rng.integers(0, 2**63)) if kind == 0 else (int(rng.integers(1, 4 if i == 5 else 3)) << 32) | int(rng.integers(0, 4))
            gs_use(c, g, int(rng.integers(1, 2**63)), subj, key, ctick=c["k"] - 50)
        c["rhead"][m] = c["rtail"][m] = int(rng.integers(0, 2**32))
        for g in own + both:
            gs_hold(c, m, g, P - 1)
        gs_round(c, m, P, 2, [t])
        gs_prev_window(c, m, P - 1, 2, 0)
        c["rhead"][t] = c["rtail"][t] = (0xFFFFFFF8, 5, 8190, 0, 77, 8100, 4000)[i]
        for g in both:
            gs_hold(c, t, g, 100)
        c["firstGossip"][t] = c["k"] - 102 * c["gossip_t"]
        gs_seen(c, t, 0, 3)
        for j, g in enumerate(own):  # a third swept this gossip before (a rebirth), a third an earlier gossip of the slot
            if j % 3 == 0:
                c["S"][t][g] = S16_EVER | S16_SWEPT | ((c["k"] - 30 - j % 7) & S16_TICK)
            elif j % 3 == 1:
                c["S"][t][g] = S16_EVER | S16_SWEPT | ((c["k"] - 51 - j % 5) & S16_TICK)
    for j, (g, e) in enumerate([(1, -1), (2, 0), (3, 1), (40, -1), (41, 0), (63, 5)]):
        gs_use(c, g, (77 << 32) | g, subj=3 if j == 1 else USER_SUBJ, key=(ST_DEAD << 32) | 1 if j == 1 else 7,
               ctick=c["k"] - SLIFE - (1 if slife and j == 5 else 0), exp=c["k"] + e)
    for g, e in ((2240, -1), (2241, 0), (2242, 1), (2244, -7)):  # rank 1's range starts at SLOTS / 2 = 2240
        gs_use(c, g, (78 << 32) | g, exp=c["k"] + e)
    c["free_list"][:3] = [9001, 9002, 9003]
    c["gains"] = gains
    return c


def gs_log(c, x, rounds, pos=None):
    """Member x's round log: rounds = [(tick, spread, targets)] oldest first, the newest at ring index (log_pos - 1)."""
    L = c["LOGW"]
    pos = len(rounds) if pos is None else pos
    assert len(rounds) <= L and pos >= len(rounds) and (pos <= L or len(rounds) == L)
    c["log_pos"][x] = pos
    for i, (tick, sp, tg) in enumerate(rounds):
        e = (pos - len(rounds) + i) & (L - 1)
        c["log_tick"][x][e], c["log_spread"][x][e], c["log_cnt"][x][e] = tick, sp, len(tg)
        c["log_tg"][x][e][:len(tg)] = tg


def gs_contact_case(LOGW=8, **kw):
    """Pairs (sender 2 i, target 2 i + 1) with logged contacts around the look-back cut k - (spread + 1) gossip_t - lat = k - 7
    (spread 2, gossip_t 2, lat 1). Every sender's window holds periods P - 2, P - 2, P - 1, P, P (and an entry out of the
    window); no target ever held a gossip of its sender, so each replayed gossip is sent (situation (c))."""
    c = gs_new(18, 192, LOGW=LOGW, BCAP=64, flags=GS_FB, **kw)
    k, free = c["k"], iter([g for g in range(192) if not 64 <= g < 128])  # group 1 stays empty
    P, sp = 1200, 2
    filler = lambda ticks: [(t2, 2, [17]) for t2 in ticks]  # rounds that target somebody else
    def pair(i, per, tlog, mlog=(), tpos=None, mpos=None):
        m, t = 2 * i, 2 * i + 1
        _gs_fill(c, m, per, [next(free) for _ in per])
        gs_round(c, m, P, sp, [16, t] if i % 2 else [t])
        gs_prev_window(c, m, P - 1, sp, 1)
        _gs_fill(c, t, [40, 41], [next(free) for _ in range(2)])
        c["firstGossip"][t] = k - 2 * 60 - 1  # t's rounds fall on the other parity
        gs_seen(c, t, 0, 2)
        gs_log(c, t, tlog, tpos)
        if mlog:
            gs_log(c, m, mlog, mpos)
    full = [P - 5, P - 2, P - 2, P - 1, P, P]
    pair(0, full, [(k - 9, 2, [0]), (k - 7, 2, [0])] + filler([k - 5, k - 3, k - 1]))      # exactly at the cut: no contact
    pair(1, full, filler([k - 8]) + [(k - 6, 2, [16, 2])] + filler([k - 4, k - 2]))        # one tick after it: a split window
    pair(2, full, filler([k - 6, k - 4]) + [(k - 2, 3, [4])])                              # the whole window is older
    pair(3, [P - 5, P - 1, P, P], [(k - 6, 2, [6])] + filler([k - 4, k - 2]))              # every window gossip is newer
    pair(4, full, [(k - 6, 2, [8]), (k - 4, 2, [8]), (k - 2, 2, [17, 8])],                 # CEV events
         [(k - 5, 2, [9]), (k - 3, 2, [9]), (k - 1, 2, [9])])
    pair(5, full, [(k - 8, 2, [10]), (k - 6, 2, [10]), (k - 4, 2, [10]), (k - 2, 2, [10])],  # CEV + 1: the slow path
         [(k - 5, 2, [11]), (k - 3, 2, [11]), (k - 1, 2, [11])])
    pair(6, full, filler([k - 8]) + [(k - 6, 4, [12])] + filler([k - 4, k - 2]))           # a second split window
    # a wrapped log, the contact in target slot 7 of a full round; with LOGW > 64 it lies in the second 64 entries
    ticks = [k - 2 * (LOGW - j) for j in range(LOGW)]
    pair(7, full, [(t2, 2, [17, 16, 15, 13, 12, 11, 10, 14] if t2 == k - 6 else [17]) for t2 in ticks], tpos=LOGW + (70 if LOGW > 64 else 3))
    c["ep_group"][:] = (np.arange(18) // 2) % 2  # pairs share a side, except through the partition variant's members
    return c


class GsSim:
    """A tiny forward simulation of GossipProtocolImpl with explicit infectedFrom sets (two to four members, scripted
    rounds, lossless links or, across the two sides of a partition, fully blocked ones). It keeps what the reference keeps:
    per member the held gossips with their infection period and `infected` set, and writes down as it goes what the engine
    keeps instead: receipt rings, round logs, holder-table entries, the incarnation history. encode() gives the device
    state at tick k together with the explicit sets, so a case carries both the encoding and the answer."""

    def __init__(self, N, gossip_t=2, lat=1, side=None):
        self.N, self.gt, self.lat, self.side = N, gossip_t, lat, side or [0] * N
        self.held = [dict() for _ in range(N)]      # g -> dict(ctick, infp, infected, reborn)
        self.ring = [[] for _ in range(N)]          # (g, infp) in receipt order
        self.swept = [0] * N                        # entries swept so far: the ring's absolute head
        self.win = [(0, 0)] * N                     # absolute (rwin, rseen) as the member's latest round left them
        self.log = [[] for _ in range(N)]
        self.last = [dict() for _ in range(N)]      # g -> (ctick, reborn) of the latest incarnation, swept or not
        self.hist, self.born, self.due = {}, {}, []

    def rb(self, x, tick):
        return rounds_before(0, tick, self.gt)  # every member's first round is at tick 0

    def _arrive(self, now):
        for at, x, y, g in [d for d in self.due if d[0] <= now]:
            if g in self.held[y]:
                self.held[y][g]["infected"].add(x)  # onGossipReq (:171-183): a known gossip only notes the sender
            else:
                reborn = g in self.last[y]
                if reborn:
                    self.hist.setdefault((g, y), []).append(self.last[y][g][0])
                self.held[y][g] = dict(ctick=at, infp=self.rb(y, at), infected={x}, reborn=reborn)
                self.last[y][g] = (at, reborn)
                self.ring[y].append((g, self.rb(y, at)))
        self.due = [d for d in self.due if d[0] > now]

    def create(self, x, g, tick):
        self._arrive(tick)
        self.born[g] = (x, tick)
        self.held[x][g] = dict(ctick=tick, infp=self.rb(x, tick), infected=set(), reborn=False)
        self.last[x][g] = (tick, False)
        self.ring[x].append((g, self.rb(x, tick)))

    def round(self, x, tick, targets, sp):
        """doSpreadGossip (:139-157) of x at `tick`: the sweep, then to each target the window gossips it is not infected by."""
        assert tick % self.gt == 0
        self._arrive(tick)
        P = self.rb(x, tick)
        gone = [g for g, st in self.held[x].items() if st["infp"] + 2 * (sp + 1) < P]
        for g in gone:
            del self.held[x][g]
        self.swept[x] += len(gone)
        self.ring[x] = [(g, p) for g, p in self.ring[x] if g not in gone]
        for y in targets:
            for g, st in self.held[x].items():
                if st["infp"] + sp >= P and y not in st["infected"] and self.side[x] == self.side[y]:
                    self.due.append((tick + self.lat, x, y, g))
        self.log[x].append((tick, sp, list(targets)))
        inwin = sum(1 for _, p in self.ring[x] if p + sp < P)
        self.win[x] = (self.swept[x] + inwin, self.swept[x] + len(self.ring[x]))

    def encode(self, k, rounds, LOGW=16, **kw):
        """The state at tick k before its rounds {m: (targets, spread)}; c["infected"][m, g] is infectedFrom_m(g)."""
        self._arrive(k)
        c = gs_new(self.N, 64, k=k, LOGW=LOGW, BCAP=16, gossip_t=self.gt, lat=self.lat, flags=GS_FB | GS_APPLY, HCAP=64,
                   ep_part=int(len(set(self.side)) > 1), **kw)
        c["ep_group"][:] = self.side
        c["firstGossip"][:] = 0
        for g, (x, tick) in self.born.items():
            gs_use(c, g, (x << 32) | (g + 1), ctick=tick, exp=k + 100)
        for x in range(self.N):
            c["rhead"][x] = c["rtail"][x] = self.swept[x]
            for g, p in self.ring[x]:
                gs_hold(c, x, g, p)
            for g, (ctick, reborn) in self.last[x].items():
                c["S"][x][g] = S16_EVER | (ctick & S16_TICK) | (S16_REBORN if reborn else 0) | (0 if g in self.held[x] else S16_SWEPT)
            c["rwin"][x], c["rseen"][x] = self.win[x]
            w, s = self.win[x][0] - self.swept[x], self.win[x][1] - self.swept[x]
            c["WB"][x] = gs_words([g for g, _ in self.ring[x][max(w, 0):s]], 1)
            gs_log(c, x, self.log[x][-LOGW:], len(self.log[x]))
        for (g, x), ticks in self.hist.items():  # hist_push's table: linear probing from the tag
            gid = int(c["slot_gid"][g])
            tag, n = gs_hist_tag(gid, x), len(ticks)
            i = next((tag + p) & 63 for p in range(64) if c["hist"][(tag + p) & 63][0] == 0)
            c["hist"][i][:3] = [tag, gid, x | n << 32]
            c["hist"][i][3:].view(np.uint32)[:n] = ticks
        for m, (targets, sp) in rounds.items():
            c["tround"][m], c["tperiod"][m], c["tspread"][m], c["tcnt"][m] = 1, self.rb(m, k), sp, len(targets)
            c["T"][m][:len(targets)] = targets
        c["infected"] = {(x, g): set(st["infected"]) for x in range(self.N) for g, st in self.held[x].items()}
        return c


def gs_replay_cases():
    """The canonical infectedFrom situations. Members: m = 0 sends to t = 1 at tick k; u = 2 (a long spread) and v = 3 help.
    gossip_t 2, lat 1, m and t spread 1 (window P - 1, swept below P - 4)."""
    cs = {}
    # (a) t delivered g0 to m inside m's current incarnation: not sent back. (c) g1, which t never held: sent.
    # (e) g2, created after the contact arrived: not even replayed. m -> t at k - 2 makes a second contact event.
    def sim_a():
        s = GsSim(3)
        for tick in range(2, 20, 2):
            s.round(2, tick, [], 1)
        s.create(1, 0, 16)
        s.round(1, 16, [0], 1)
        s.round(0, 18, [2, 1], 1)
        s.round(1, 18, [], 1)
        s.create(0, 1, 18)
        s.create(0, 2, 19)
        return s
    cs["replay_a_c_e"] = sim_a().encode(20, {0: ([1], 1)})
    cs["replay_d_slow"] = sim_a().encode(20, {0: ([1], 1)}, cev_cap=1)  # (d) the same through the full log scan
    # (b) t delivered g0 to m long ago; m swept it and got it again from u; t's recent round reached m without g0: sent.
    # (f) the same, but t got g0 again too (from v: u has t in its own infectedFrom) and sent it to m inside m's new
    # incarnation: not sent.
    for name, again in (("replay_b_older", False), ("replay_f_rebirth", True)):
        s = GsSim(4)
        s.create(1, 0, 2)
        for tick in range(2, 20, 2):
            s.round(1, tick, [0, 2] if tick == 2 else [0] if tick == 18 else [], 1)
            s.round(0, tick, [], 1)
            s.round(2, tick, [3] if tick == 4 else [0] if tick == 16 else [], 6)
            s.round(3, tick, [1] if tick == 16 and again else [], 6)
        cs[name] = s.encode(20, {0: ([1], 1), 3: ([2], 6)})
    return cs


def gs_cases():
    """name -> state: every case of tests/test_gpu_gossip.py (one launch each)."""
    cs = {}
    for QW in GS_GROUP_QWS:
        for kind in GS_GROUP_KINDS:
            cs[f"groups_{QW}_{kind}"] = gs_group_case(QW, kind)
    for base, c in (("edges", gs_rounds_edges()), ("sweeps", gs_rounds_sweeps()), ("empty", gs_rounds_empty())):
        for path, kw in GS_PATHS.items():
            cs[f"rounds_{base}_{path}"] = gs_variant(c, **kw)
    cs["scatter"] = gs_scatter_case()
    for name, (nag, ntl) in GS_SEND_SHAPES.items():
        cs[f"send_{name}"] = gs_send_case(nag, ntl, 11)
    # 2049-word rows: the workgroup path at the engine's own chunk sizes, and the third batch of the group scan
    cs["send_nag130"] = gs_send_case(130, 2, 12, QW=2049, hold=0.7)
    cs["send_loss37"] = gs_variant(cs["send_nag3"], ep_loss=37)
    cs["send_loss100"] = gs_variant(cs["send_nag3"], ep_loss=100)
    cs["send_partition"] = gs_variant(cs["send_nag3"], ep_part=1)
    cs["send_ring_full"] = gs_send_case(3, 30, 11, BCAP=64)
    for name in list(GS_SEND_SHAPES) + ["nag130", "loss37"]:
        cs[f"send_{name}_em"] = gs_variant(cs[f"send_{name}"], flags=GS_EM)
    cs["contacts"] = gs_contact_case()
    cs["contacts_logw128"] = gs_contact_case(LOGW=128)
    cs["contacts_cev1"] = gs_variant(cs["contacts"], cev_cap=1)
    cs["contacts_crcap1"] = gs_variant(cs["contacts"], CRCAP=1)
    cs["contacts_rpcap_short"] = gs_variant(cs["contacts"], RPCAP=len(gs_ref(cs["contacts"])["rp"]) - 1)
    cs["contacts_loss37"] = gs_variant(cs["contacts"], ep_loss=37, flags=GS_FB | GS_EM)
    cs["contacts_cx1"] = gs_variant(cs["contacts"], cx=1, flags=GS_FB | GS_APPLY)  # RX rows staged in three chunks
    cs["contacts_cx2"] = gs_variant(cs["contacts"], cx=2)  # in two, the last one partial
    cs.update(gs_replay_cases())
    cs["apply_nag3"] = gs_variant(cs["send_nag3"], flags=GS_APPLY)
    cs["apply_loss37"] = gs_variant(cs["send_loss37"], flags=GS_APPLY | GS_FB)
    cs["apply_gains"] = gs_apply_case()
    cs["apply_rcap_short"] = gs_apply_case(RCAP=len(gs_ref(cs["apply_gains"])["routed"]) - 1)
    cs["apply_slife"] = gs_apply_case(slife=True)
    return cs


# ------------------------------------------------------------------- P4: the gossip first-receipt phase of one member
# onMembershipGossip -> updateMembership(r1, MEMBERSHIP_GOSSIP) (MembershipProtocolImpl.java:401-408,475-541; SEMANTICS.md
# §7) for one member and one ordered receipt list, as a serial fold over dictionaries: the yardstick of
# tests/test_gpu_p4.py for both device versions of the phase (the lane-serial fold and the wave version). Loss 0, no
# link delay, no per-member config, every metadata version 0.
P4_ABSENT, P4_ALIVE, P4_SUSPECT, P4_DEAD = 0, 1, 2, 3
P4_INC_LIMIT = 1 << 30  # an incarnation the key plane cannot hold: the engine's E_INC
P4_TL = 16  # entries of a member's per-tick write log; its length saturates at P4_TL + 1
P4_COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 128, 129, 200]
P4_SLOW_AT = [0, 31, 63, 64, 69]  # positions of the slow receipt in a list of 70 (69: last)
P4_SLOW_KINDS = ["own_alive", "own_suspect", "dead", "absent", "user"]
P4_ACCEPTED = [16, 17, 40]


def p4_is_overrides(s1, i1, s0, i0):
    """MembershipRecord.isOverrides (MembershipRecord.java:66-84); s0 = P4_ABSENT is `r0 == null`."""
    if s0 == P4_ABSENT:
        return s1 == P4_ALIVE
    if s0 == P4_DEAD:
        return False
    if s1 == P4_DEAD:
        return True
    if i1 == i0:
        return s1 != s0 and s1 == P4_SUSPECT
    return i1 > i0


def p4_ceil_log2(n):
    """ClusterMath.ceilLog2 (ClusterMath.java:133-135): the bit length."""
    return int(n).bit_length()


def p4_member(m, N, fd, gl):
    """Member m of a PRECONVERGED cluster before its first tick: every subject ALIVE at incarnation 0 with known
    metadata, no timer, no fetch. fd / gl: its pingMembers and remoteMembers lists as the engine shuffled them."""
    return {"m": m, "row": {s: [P4_ALIVE, 0, True, 0] for s in range(N)}, "tsize": N, "cid": 0, "fetch": [],
            "fnext": NEVER, "timerMin": NEVER, "gcnt": 0, "evseq": 0, "fd": list(fd), "gl": list(gl)}


def p4_fold(st, k, ndrop, receipts, dead, cfg):
    """One tick's P4 of member state `st` (changed in place) at tick k. receipts: ("M", subject, status, incarnation) or
    ("U", origin, payload, counter) in order; ndrop: receipts the routing dropped (compares only); dead: the members
    that are dead at k; cfg: suspicion_mult, ping_t, md_t, lat (ticks). Returns the tick's events, write log, its
    length, counter deltas, gossips created (subject, status, incarnation) and whether an incarnation >= 2^30 was
    written."""
    m = st["m"]
    out = {"events": [], "tl": [], "tl_n": 0, "R": 0, "W": 0, "M": 0, "E": 0, "LOST": 0, "gossips": [], "einc": False}
    if m in dead:  # a crashed member holds no P4: its receipts are dropped
        return out
    out["R"] += ndrop
    last = [None]

    def wrote(s):  # the tick's write log: a repeat of the last subject is one entry; the length saturates
        if out["tl_n"] and last[0] == s:
            return
        if out["tl_n"] < P4_TL:
            out["tl"].append(s)
        if out["tl_n"] <= P4_TL:
            out["tl_n"] += 1
        last[0] = s

    def event(typ, subj, old, new, pad=0):
        out["events"].append((k, m, st["evseq"], typ, subj, old, new, pad))
        st["evseq"] += 1
        out["E"] += 1

    def fetch(subj, s1, i1, added):
        cid = st["cid"]
        st["cid"] += 1
        out["M"] += 1
        if subj in dead:  # connection refused: the request is lost, nothing is recorded
            out["LOST"] += 1
            return
        st["fetch"].append([cid, subj, i1, s1 | (1 << 8) | (added << 16) | (1 << 24), M32, k + cfg["md_t"],
                            k + cfg["lat"], M32])
        st["fnext"] = min(st["fnext"], k + cfg["md_t"], k + cfg["lat"])

    for r in receipts:
        if r[0] == "U":  # listenGossips: not membership, no record compare
            event("GOSSIP", r[1], r[2] & M32, (r[2] >> 32) & M32, r[3])
            continue
        _, subj, s1, i1 = r
        out["R"] += 1
        row = st["row"].get(subj)
        s0, i0 = (row[0], row[1]) if row else (P4_ABSENT, 0)
        if not p4_is_overrides(s1, i1, s0, i0):
            continue
        if subj == m:  # refute: max(inc) + 1, the status kept, one gossip, no event
            row[1] = max(i0, i1) + 1
            out["einc"] |= row[1] >= P4_INC_LIMIT
            out["W"] += 1
            wrote(subj)
            st["gcnt"] += 1
            out["gossips"].append((subj, s0, row[1]))
            continue
        out["einc"] |= i1 >= P4_INC_LIMIT
        out["W"] += 1
        wrote(subj)
        if s1 == P4_DEAD:  # the row goes, with its metadata and its timer
            del st["row"][subj]
            st["tsize"] -= 1
            event("REMOVED", subj, 0 if row[2] else None, None)
            for name in ("fd", "gl"):
                if subj in st[name]:
                    st[name].remove(subj)
            continue
        if row is None:
            row = st["row"][subj] = [s1, i1, False, 0]
            st["tsize"] += 1
        row[0], row[1] = s1, i1
        if s1 == P4_SUSPECT:
            if row[3] == 0:  # computeIfAbsent
                row[3] = k + cfg["suspicion_mult"] * p4_ceil_log2(st["tsize"]) * cfg["ping_t"]
                st["timerMin"] = min(st["timerMin"], row[3])
        else:
            row[3] = 0  # cancel
        if s0 == P4_ABSENT:
            fetch(subj, s1, i1, 1)
        elif i0 < i1:
            fetch(subj, s1, i1, 0)
    return out


def p4_hops(st, k, dead, cfg):
    """What the tick does to the member's pending fetches before P4 (swim_create takes a latency of one tick only, so
    the requests of tick k - 1 reach their subjects at k): a live subject answers with GET_METADATA_RESP carrying its
    metadata version 0, one message, and the record waits for the arrival at k + lat; a dead one answers nothing and
    only the timeout remains. Returns the messages sent."""
    sent = 0
    if st["m"] in dead:
        return 0
    for f in st["fetch"]:
        if f[3] >> 24 == 1 and f[6] == k:
            if f[1] in dead:
                f[3] &= 0x00FFFFFF
            else:
                sent += 1
                f[3] = (f[3] & 0x00FFFFFF) | (2 << 24)
                f[6], f[7] = k + cfg["lat"], 0
    due = [min(f[5], f[6]) if f[3] >> 24 else f[5] for f in st["fetch"]]
    if any(f[5] <= k or (f[3] >> 24 == 2 and f[6] <= k) for f in st["fetch"]):
        raise ValueError("an arrival or a timeout in this tick: outside what this reference restates")
    st["fnext"] = min(due) if due else st["fnext"]
    return sent


def p4_row_words(st, N):
    """The member's table as swim_read_row returns it: inc | status << 32 | metadata known << 34 | deadline << 35."""
    out = np.zeros(N, np.uint64)
    for s, (s0, i0, meta, timer) in st["row"].items():
        out[s] = (i0 & M32) | (s0 << 32) | (int(meta) << 34) | (timer << 35)
    return out


def p4_batch_accepts(key0, receipts):
    """The batching claim of the wave version, restated on its own: on present rows, with no DEAD and no own-record
    receipt, a receipt (subject, status, incarnation) is accepted iff its key inc << 2 | status is above the running
    maximum of the row's key and the earlier keys of the same subject. key0: subject -> the row's key before the list.
    Returns one bool per receipt."""
    top = dict(key0)
    acc = []
    for s, s1, i1 in receipts:
        key = (i1 << 2) | s1
        acc.append(key > top[s])
        top[s] = max(top[s], key)
    return acc


def p4_serial_accepts(key0, receipts):
    """The same list through isOverrides one receipt after another (what p4_fold does)."""
    row = {s: [k & 3, k >> 2] for s, k in key0.items()}
    acc = []
    for s, s1, i1 in receipts:
        ok = p4_is_overrides(s1, i1, row[s][0], row[s][1])
        acc.append(ok)
        if ok:
            row[s] = [s1, i1]
    return acc


def p4_pool(N, m, killed):
    """The subjects member m's lists are about, in the order the patterns index them: every live other member,
    starting after m."""
    p = [s for s in range(N) if s != m and s not in killed]
    r = m % len(p)
    return p[r:] + p[:r]


def p4_prep(p, top=P4_INC_LIMIT - 2):
    """The preparation tick's receipts for a member with pool p (no own record, so no gossip is created): the pre-states
    the tick under test meets. p[0], p[1] SUSPECT 0 (a timer held), p[2] ALIVE 2, p[3] SUSPECT 1, p[4], p[5] removed,
    p[6] ALIVE 62, p[7] ALIVE 63 (the 8-bit key shadow's edge), p[8] SUSPECT top, p[9] ALIVE top (2^30 - 2: the
    largest incarnation that can still rise)."""
    return [("M", p[0], P4_SUSPECT, 0), ("M", p[1], P4_SUSPECT, 0), ("M", p[2], P4_ALIVE, 2), ("M", p[3], P4_SUSPECT, 1),
            ("M", p[4], P4_DEAD, 0), ("M", p[5], P4_DEAD, 7), ("M", p[6], P4_ALIVE, 62), ("M", p[7], P4_ALIVE, 63),
            ("M", p[8], P4_SUSPECT, top), ("M", p[9], P4_ALIVE, top)]


def p4_fast(rng, p, n):
    """n receipts that are fast after p4_prep unless an earlier one of the list removed their row: ALIVE / SUSPECT about
    twelve present subjects at incarnations around the rows', so that one subject recurs within a batch, keys repeat
    and stale records sit between accepted ones."""
    subj = [p[0], p[1], p[2], p[3], p[6], p[7]] + p[10:16]
    base = [0, 0, 2, 1, 62, 63] + [0] * 6
    out = []
    for _ in range(n):
        j = int(rng.integers(0, len(subj)))
        out.append(("M", subj[j], int(rng.integers(1, 3)), base[j] + int(rng.integers(0, 4))))
    return out


def p4_slow(kind, m, p, j=0):
    """One receipt that the wave version hands to lane 0."""
    return {"own_alive": ("M", m, P4_ALIVE, 1 + j), "own_suspect": ("M", m, P4_SUSPECT, 0),
            "dead": ("M", p[11 + j], P4_DEAD, 0), "absent": ("M", p[4 + (j & 1)], P4_ALIVE, 5 + j),
            "user": ("U", p[20], 0x1122334455667788 + j, 9 + j)}[kind]


def p4_patterns(N, m, killed, name, top=P4_INC_LIMIT - 2):
    """The receipt list of the tick under test for pattern `name` at member m."""
    p = p4_pool(N, m, killed)
    rng = np.random.default_rng(7000 + 131 * m + N)
    A, S, D = P4_ALIVE, P4_SUSPECT, P4_DEAD
    kind, _, arg = name.partition(":")
    if kind == "count":
        return p4_fast(rng, p, int(arg))
    if kind == "triple":  # SUSPECT i / ALIVE i + 1 / SUSPECT i + 1 after `off` stale fast receipts
        who, off = arg.split(",")
        pad = [("M", p[12], A, 0)] * int(off)
        if who == "notimer":
            return pad + [("M", p[10], S, 0), ("M", p[10], A, 1), ("M", p[10], S, 1)]
        if who == "timer":
            return pad + [("M", p[0], S, 1), ("M", p[0], A, 2), ("M", p[0], S, 2)]
        return pad + [("M", p[10], S, 0), ("M", p[0], S, 1), ("M", p[10], A, 1), ("M", p[0], A, 2), ("M", p[0], S, 2),
                      ("M", p[10], S, 1)]
    if kind == "stale":  # stale records between accepted ones, equal keys
        return [("M", p[10], S, 1), ("M", p[10], A, 0), ("M", p[10], A, 1), ("M", p[10], S, 1), ("M", p[11], A, 0),
                ("M", p[10], A, 2), ("M", p[10], A, 2), ("M", p[0], S, 0), ("M", p[0], A, 0), ("M", p[1], A, 1),
                ("M", p[1], A, 1), ("M", p[1], S, 1), ("M", p[1], S, 1)]
    if kind == "slow":
        what, at = arg.split(",")
        lst = p4_fast(rng, p, 69)
        lst.insert(int(at), p4_slow(what, m, p))
        return lst
    if kind == "slow2":  # two slow receipts back to back, inside a batch and across its end
        lst = p4_fast(rng, p, 100)
        for at, (a, b) in ((63, ("own_alive", "absent")), (10, ("dead", "user"))):
            lst[at:at] = [p4_slow(a, m, p, 1), p4_slow(b, m, p, 1)]
        return lst
    if kind == "allslow":
        return [p4_slow(x, m, p, j) for j in range(3) for x in P4_SLOW_KINDS]
    if kind == "accepted":  # distinct accepted subjects: the write log fills and overflows
        n, fetching = arg.split(",")
        return [("M", p[10 + j], A, 1) if fetching == "f" else ("M", p[10 + j], S, 0) for j in range(int(n))]
    if kind == "incs":
        top += 1
        return [("M", p[6], S, 62), ("M", p[6], A, 63), ("M", p[7], A, 63), ("M", p[7], S, 63), ("M", p[7], A, 64),
                ("M", p[6], S, 64), ("M", p[6], D, 3), ("M", p[8], A, top), ("M", p[9], S, top), ("M", p[9], A, top),
                ("M", p[8], S, top - 1), ("M", p[8], S, top)]
    if kind == "killed":  # subjects that are dead at the tick: the metadata request is lost
        return [("M", killed[0], A, 1), ("M", p[10], A, 1), ("M", killed[1], S, 1), ("M", killed[1], A, 2),
                ("M", killed[0], D, 0), ("M", killed[0], A, 4)]
    if kind == "mixed":
        lst = p4_fast(rng, p, int(arg))
        for j in range(int(arg) // 9):
            at = int(rng.integers(0, len(lst) + 1))
            lst.insert(at, p4_slow(P4_SLOW_KINDS[int(rng.integers(0, 5))], m, p, j % 3))
        return lst
    if kind == "none":
        return []
    raise KeyError(name)


def p4_pattern_names():
    names = [f"count:{n}" for n in P4_COUNTS]
    names += [f"triple:{w},{o}" for w in ("notimer", "timer", "both") for o in (0, 62)] + ["stale:"]
    names += [f"slow:{w},{a}" for w in P4_SLOW_KINDS for a in P4_SLOW_AT] + ["slow2:", "allslow:"]
    names += [f"accepted:{n},{f}" for n in P4_ACCEPTED for f in ("s", "f")] + ["incs:", "killed:"]
    names += [f"mixed:{n}" for n in (30, 100, 150)] + ["none:"]
    return names


def p4_case(N, top=P4_INC_LIMIT - 2):
    """The known-answer case at N members (top: the incarnation of the rows at the field's edge; a run that goes on for
    many ticks takes a smaller one, since a member that hears of its own record at 2^30 - 1 refutes it with 2^30): kills (before the first tick), then per tick {member: (ndrop, receipts)} for
    the preparation tick 0 and the tick under test 1. Every pattern runs at a member of its own, spread over the member
    range (two blocks of k_member_tick at N = 300); the last two members are killed: one keeps receipts and dropped
    receipts (nothing applied, counts cleared), one only dropped receipts; an idle live member has dropped receipts too."""
    killed = [N - 1, N - 2]
    names = p4_pattern_names()
    stride = (N - 3) // len(names)
    assert stride >= 1
    prep, test, who = {}, {}, {}
    for i, name in enumerate(names):
        m = i * stride
        who[m] = name
        prep[m] = (0, p4_prep(p4_pool(N, m, killed), top))
        test[m] = (5 if name in ("count:65", "slow:dead,31") else 0, p4_patterns(N, m, killed, name, top))
    test[N - 3] = (3, [])  # idle, alive
    who[N - 3] = "idle ndrop"
    test[N - 2] = (4, [])  # dead, idle
    test[N - 1] = (2, p4_fast(np.random.default_rng(5), p4_pool(N, 0, killed), 70))  # dead, with receipts
    prep[N - 1] = (1, [("M", 0, P4_SUSPECT, 0)])
    return {"N": N, "killed": killed, "ticks": [prep, test], "who": who}


def p4_case_einc(N):
    """One record at incarnation 2^30 in a serial-sized list and behind a batch boundary: every path reports E_INC."""
    p0, p1 = p4_pool(N, 3, []), p4_pool(N, 40, [])
    rng = np.random.default_rng(11)
    a = [("M", p0[10], P4_ALIVE, 1), ("M", p0[10], P4_ALIVE, P4_INC_LIMIT), ("M", p0[12], P4_SUSPECT, 0)]
    b = [("M", p1[10 + int(rng.integers(0, 6))], int(rng.integers(1, 3)), int(rng.integers(0, 4))) for _ in range(70)]
    b.insert(64, ("M", p1[11], P4_SUSPECT, P4_INC_LIMIT))
    return {"N": N, "killed": [], "ticks": [{3: (0, a), 40: (0, b)}], "who": {3: "einc short", 40: "einc at 64"}}


def p4_pack(tick):
    """{member: (ndrop, receipts)} as swim_debug_receipts_set takes it: the table of distinct records (6 words each) and
    {member: (ndrop, indices)}."""
    table, recs, lists = {}, [], {}
    for m, (nd, lst) in tick.items():
        idx = []
        for r in lst:
            if r not in table:
                table[r] = len(recs)
                if r[0] == "M":
                    recs.append((0, r[1], r[2], r[3], r[1], len(recs)))
                else:
                    recs.append((1, r[1], r[2] & M32, (r[2] >> 32) & M32, 0, r[3]))
            idx.append(table[r])
        lists[m] = (nd, idx)
    return recs, lists


def p4_injectable(N, recs, lists, rcap, free_slots):
    """swim_debug_receipts_set's own preconditions (include/swimhip_debug.h), restated for the CPU check."""
    for r in recs:
        if r[0] == 0 and not (r[1] < N and 1 <= r[2] <= 3 and r[4] < N):
            return False
        if r[0] == 1 and not (r[1] < N and r[4] == 0):
            return False
        if r[0] > 1:
            return False
    if any(m >= N or any(i >= len(recs) for i in idx) for m, (_, idx) in lists.items()):
        return False
    return sum(len(idx) for _, idx in lists.values()) <= rcap and len(recs) <= free_slots
