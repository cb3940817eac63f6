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
