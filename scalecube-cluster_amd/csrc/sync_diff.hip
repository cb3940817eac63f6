// sync_diff.hip — the SYNC-payload diff: its lister (k_ack_resolve), the dirty-mask maintenance and their launchers.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "dev_util.h"

namespace swim {

// ------------------------------------------------------------------------------------------------------------
// k_sync_diff: for every SYNC / SYNC_ACK sent in tick k-1, stream the payload's key plane (the sender's live row,
// or its copy-on-write snapshot) against the receiver's key plane and extract, per 2048-subject chunk and in
// subject order, the records that differ (the eager `!r1.equals(table.get(id))` filter of syncMembership,
// :456-467). This is the HBM-bound hot loop: 2 x 1 B read per subject per merge on one GPU (the keys' 8-bit
// shadows, key8; an escaped key is compared on its 4-B key32), 2 x 4 B for the rest. SHARDED adds payloads
// received from other shards (baseline row + shipped chunks); the single-GPU instance has only local rows and
// snapshots.
//
// an item's message as k_sync_diff reads it (the 16-B entries of Dev::dlist / dlist_w, written by k_ack_resolve;
// without a list, read from the message): x = the message index, y = sender, z = receiver, w = where the payload is
// (desc_pay)
__device__ __forceinline__ uint32_t desc_pay(const SyncMsg& mm) {
  if (mm.kind & KF_DEFER) return DESC_DEFER;  // merged in a later tick: nothing to compare now
  if (mm.payload != NEVER) return mm.payload;  // an arena snapshot, or (W > 1) PAY_RX | rx index
  return mm.pin == NEVER ? NEVER : DESC_PIN | mm.pin;  // the live row (pinned: copied into the arena as it streams)
}

// a peer's payload (PAY_RX | rx index): was chunk c shipped (it differs from the baseline row)?
__device__ __forceinline__ bool rx_shipped(const Dev& d, uint32_t pay, uint32_t c) {
  const uint64_t* mk = d.rx_mask + (size_t)(pay & ~PAY_RX) * d.MW;
  return (mk[c >> 6] >> (c & 63)) & 1ull;
}
// the 4-B payload keys from subject s on (within one chunk) of the entry's payload: the local sender's row, or a peer's
// shipped chunk, or the baseline row
template <bool SHARDED>
__device__ __forceinline__ const uint32_t* pay_keys(const Dev& d, const uint4& D, uint32_t s) {
  if (!SHARDED || D.w == NEVER) return d.rowk + lidx(d, D.y) * d.NS + s;
  const uint32_t ri = D.w & ~PAY_RX, c = s / CH;
  const uint64_t* mk = d.rx_mask + (size_t)ri * d.MW;
  if (!((mk[c >> 6] >> (c & 63)) & 1ull)) return d.base_row + s;
  uint32_t rank = __popcll(mk[c >> 6] & ((1ull << (c & 63)) - 1ull));
  for (uint32_t q = 0; q < (c >> 6); ++q) rank += __popcll(mk[q]);
  return (const uint32_t*)(d.xa_recv + d.rx_off[ri]) + (size_t)rank * CH + s % CH;
}

// this lane's keys of the item's chunk c: narrow (an entry of the narrow list: a local sender's unpinned live row, or
// on a row shard a peer's payload): the item is chunks c .. c + 3 of the message, lane i the 32 subjects c CH + 32 i
// ..., and x holds their 8-bit shadow keys (key8): payload x[0..1], receiver x[2..3], the same 64 B per lane in
// flight as one chunk of 4-B keys.
// Otherwise 8 payload keys and 8 receiver keys of chunk c: the payload is the sender's live row or its copy-on-write
// snapshot; for a payload received from another shard, the shipped chunk if it differs from the baseline, else the
// baseline. pinw: the arena row a live-row payload is copied into while it streams (pin_msg), else NEVER. Every lane
// of the block takes the same item, so the mode is uniform.
template <bool SHARDED>
__device__ __forceinline__ void diff_fetch(const Dev& d, uint32_t b, const uint4& D, uint32_t c, uint4 (&x)[4],
                                           uint32_t& pinw, bool& narrow, bool narrow_item) {
  pinw = NEVER;
  narrow = false;
  if (narrow_item) {
    narrow = true;
    const uint32_t n0 = c * CH + threadIdx.x * 32;  // NS8 is a multiple of 16: 16-subject groups wholly in or out
    // the payload: the local sender's row, or (a peer's payload) the baseline row's shadow for a chunk that was not
    // shipped; a shipped chunk has no shadow: its lanes read as escaped (0xFF) and diff_wave8 compares its u32 keys
    const uint8_t* p8 = nullptr;
    if (!SHARDED || D.w == NEVER) {
      p8 = d.rowk8 + lidx(d, D.y) * d.NS8 + n0;
    } else if (n0 < d.NS8 && !rx_shipped(d, D.w, n0 / CH)) {
      p8 = d.base_row8 + n0;
    }
    const uint8_t* r8 = d.rowk8 + lidx(d, D.z) * d.NS8 + n0;
    const uint4 z = make_uint4(0, 0, 0, 0), e = make_uint4(~0u, ~0u, ~0u, ~0u);
    // one GPU: a chunk of the item that the lister found clean in both rows (equal, row_dirty) is not loaded: its
    // wave compares zeros and writes the two segments' zero counts
    if (!SHARDED && !((D.w >> __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) & 1u)) {
      x[0] = x[1] = x[2] = x[3] = z;
      return;
    }
    x[0] = n0 < d.NS8 ? (p8 ? ld_c4((const uint32_t*)p8) : e) : z;
    x[1] = n0 + 16 < d.NS8 ? (p8 ? ld_c4((const uint32_t*)(p8 + 16)) : e) : z;
    x[2] = n0 < d.NS8 ? ld_c4((const uint32_t*)r8) : z;
    x[3] = n0 + 16 < d.NS8 ? ld_c4((const uint32_t*)(r8 + 16)) : z;
    return;
  }
  const uint32_t s0 = c * CH + threadIdx.x * 8;
  // NS is a multiple of 8: a 32-B group is wholly in or out; padding entries are 0 (absent)
  if (s0 >= d.NS || D.w == DESC_DEFER || D.w == DESC_HOLE) {
    x[0] = x[1] = x[2] = x[3] = make_uint4(0, 0, 0, 0);
    return;
  }
  const uint32_t* p8;
  if (D.w == NEVER || (D.w & DESC_PIN)) {
    pinw = D.w == NEVER ? NEVER : D.w & ~DESC_PIN;
    p8 = d.rowk + lidx(d, D.y) * d.NS + s0;
  } else if (SHARDED && (D.w & PAY_RX)) {  // the shipped chunk, or the baseline row
    p8 = pay_keys<SHARDED>(d, D, s0);
  } else {
    p8 = d.arena[b] + (size_t)D.w * d.NS + s0;
  }
  const uint32_t* r8 = d.rowk + lidx(d, D.z) * d.NS + s0;
  // (non-temporal loads measured 1.5x slower here on gfx950)
  x[0] = ld_c4(p8);
  x[1] = ld_c4(p8 + 4);
  x[2] = ld_c4(r8);
  x[3] = ld_c4(r8 + 4);
}

// chunk c of message mi against this lane's 8 payload keys p and receiver keys r (s0: its first subject): the
// differing records in subject order into the candidate pool, the chunk's (offset, count) into chunk_meta
__device__ __forceinline__ void diff_chunk(const Dev& d, uint32_t b, uint32_t mi, uint32_t c, uint32_t s0,
                                           const uint32_t (&p)[8], const uint32_t (&r)[8], uint32_t* scan,
                                           uint32_t& base) {
  const bool dl = d.ackres != 0;
  uint32_t mask = 0, ab = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if ((p[j] & 3u) != ST_ABSENT && p[j] != r[j]) mask |= 1u << j;
    ab |= (uint32_t)((p[j] & 3u) == ST_ABSENT && (r[j] & 3u) != ST_ABSENT);
  }
  uint32_t nc = __popc(mask);
  const bool two = 2 * c + 1 < d.NMETA;  // the chunk's second candidate segment (lanes 128-255)
  if (!__syncthreads_or(nc | ab)) {  // steady state: the whole 2048-subject chunk matches
    if (threadIdx.x == 0) {
      uint32_t* cm = d.chunk_meta + ((size_t)mi * d.NMETA + 2 * c) * 2;
      cm[0] = cm[1] = 0;
      if (two) cm[2] = cm[3] = 0;
    }
    return;
  }
  if (dl && ab) atomicOr(&d.msgs[b][mi].kind, KF_ABS);  // (rare: a record the payload lacks)
  scan[threadIdx.x] = nc;
  __syncthreads();
  for (uint32_t o = 1; o < 256; o <<= 1) {
    uint32_t v = threadIdx.x >= o ? scan[threadIdx.x - o] : 0;
    __syncthreads();
    scan[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t incl = scan[threadIdx.x];
  uint32_t totc = scan[255];
  if (threadIdx.x == 0) {
    const uint32_t first = scan[127];  // the first segment's candidates (lanes 0-127)
    uint32_t bo = atomicAdd(d.pool_used, totc);
    if (bo + totc > d.POOLCAP) {  // no room: nothing of this chunk is written (the error aborts the step)
      atomicOr(d.err, E_POOL);
      totc = 0;
      bo = NEVER;
    }
    base = bo;
    uint32_t* cm = d.chunk_meta + ((size_t)mi * d.NMETA + 2 * c) * 2;
    cm[0] = bo;
    cm[1] = bo == NEVER ? 0u : first;
    if (two) {
      cm[2] = bo == NEVER ? NEVER : bo + first;
      cm[3] = bo == NEVER ? 0u : totc - first;
    }
    if (totc) atomicAdd(&d.msgs[b][mi].ncand, totc);
  }
  __syncthreads();
  uint32_t o = base + incl - nc;
  if (base != NEVER)  // (an overflowed chunk must not overwrite other chunks' candidates)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (mask & (1u << j)) d.pool[o++] = ((uint64_t)(s0 + j) << 34) | key34(p[j]);
  __syncthreads();
}

// a narrow item: chunks c .. c + 3 of message mi, each wave two 1024-subject candidate segments (wave w: segments
// 2c + 2w (lanes 0-31) and 2c + 2w + 1 (lanes 32-63), 32 subjects per lane from x), tested, scanned and written by the
// wave alone: no block barrier. A lane with an escaped shadow (0xFF: an incarnation past 62 among its subjects)
// compares its 32 full keys of both rows.
template <bool SHARDED>
__device__ __forceinline__ void diff_wave8(const Dev& d, uint32_t b, const uint4& D, uint32_t c, const uint4 (&x)[4]) {
  const uint32_t mi = D.x;
  const bool dl = d.ackres != 0;
  const uint32_t lane = threadIdx.x & 63u, seg = 2 * c + 2 * (threadIdx.x >> 6) + (lane >> 5);
  const uint32_t n0 = c * CH + threadIdx.x * 32;  // = seg * MCH + (lane & 31) * 32
  const uint32_t pw[8] = {x[0].x, x[0].y, x[0].z, x[0].w, x[1].x, x[1].y, x[1].z, x[1].w};
  const uint32_t rw[8] = {x[2].x, x[2].y, x[2].z, x[2].w, x[3].x, x[3].y, x[3].z, x[3].w};
  uint32_t esc = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q)  // a 0xFF byte in either word (a zero byte of the complement)
    esc |= ((~pw[q] - 0x01010101u) & pw[q] & 0x80808080u) | ((~rw[q] - 0x01010101u) & rw[q] & 0x80808080u);
  uint32_t mask = 0, ab = 0;
  const uint32_t *pk = nullptr, *rk = nullptr;
  if (esc) {  // (rare) the 32 subjects' 4-B keys, one at a time
    pk = pay_keys<SHARDED>(d, D, n0);  // (32 subjects: within one chunk)
    rk = d.rowk + lidx(d, D.z) * d.NS + n0;
#pragma unroll 1
    for (uint32_t j = 0; j < 32; ++j) {
      const uint32_t p = n0 + j < d.NS ? pk[j] : 0u, r = n0 + j < d.NS ? rk[j] : 0u;
      if ((p & 3u) != ST_ABSENT && p != r) mask |= 1u << j;
      ab |= (uint32_t)((p & 3u) == ST_ABSENT && (r & 3u) != ST_ABSENT);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const uint32_t p = (pw[j >> 2] >> (8 * (j & 3))) & 0xFFu, r = (rw[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      if ((p & 3u) != ST_ABSENT && p != r) mask |= 1u << j;
      ab |= (uint32_t)((p & 3u) == ST_ABSENT && (r & 3u) != ST_ABSENT);
    }
  }
  const uint32_t nc = __popc(mask);
  uint32_t* cm = d.chunk_meta + ((size_t)mi * d.NMETA + seg) * 2;
  const bool live = seg < d.NMETA, head = (lane & 31u) == 0;
  if (!__ballot(nc | ab)) {  // steady state: the wave's 2048 subjects match
    if (head && live) cm[0] = cm[1] = 0;
    return;
  }
  if (dl && __ballot(ab) && lane == 0) atomicOr(&d.msgs[b][mi].kind, KF_ABS);  // (rare: a record the payload lacks)
  if (!SHARDED && d.MW && lane == 0)  // a streamed chunk that differed (k_rebase's policy)
    atomicAdd(&d.ms[c + (threadIdx.x >> 6)].cstat[1], 1ull);
  uint32_t incl = nc;
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  const uint32_t totc = __shfl(incl, 63), first = __shfl(incl, 31);  // both segments, the first one
  uint32_t bo = 0;
  if (lane == 0 && totc) {
    bo = atomicAdd(d.pool_used, totc);
    if (bo + totc > d.POOLCAP) {  // no room: nothing of these segments is written (the error aborts the step)
      atomicOr(d.err, E_POOL);
      bo = NEVER;
    }
    if (bo != NEVER) atomicAdd(&d.msgs[b][mi].ncand, totc);
  }
  bo = __shfl(bo, 0);
  if (head && live) {
    const uint32_t off = lane ? first : 0u, cnt = lane ? totc - first : first;
    cm[0] = bo == NEVER ? NEVER : bo + off;
    cm[1] = bo == NEVER ? 0u : cnt;
  }
  if (bo == NEVER) return;  // (an overflowed segment must not overwrite other segments' candidates)
  uint32_t o = bo + incl - nc;
  if (esc) {
    for (uint32_t m = mask; m; m &= m - 1, ++o) {
      const uint32_t j = (uint32_t)(__ffs(m) - 1);
      d.pool[o] = ((uint64_t)(n0 + j) << 34) | key34(pk[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 32; ++j)
      if (mask & (1u << j)) d.pool[o++] = ((uint64_t)(n0 + j) << 34) | key34((pw[j >> 2] >> (8 * (j & 3))) & 0xFFu);
  }
}

// k_sync_diff's work, two lists of 16-B entries (message, sender, receiver, payload place; desc_pay) over the blocks
// blk of nblk, grid-stride, each with the next item's keys in flight while the current one is tested and the entry of
// the item after that in flight too, so that an item's key loads never wait for its message:
// * stream_wide: payloads compared on 4-B keys (snapshots, pinned live rows, payloads from other shards, or no 8-bit
//   plane), one 2048-subject chunk per item, block barriers per chunk (diff_chunk);
// * stream_narrow: unpinned live-row payloads (on a row shard: of local senders) on the 8-bit plane, four chunks per
//   item, one wave per two 1024-subject candidate segments and no block barrier (diff_wave8).
// Two loops rather than one with both kinds of item: the narrow loop's registers are then not sized by the wide
// path's (with both in one loop it spilled, and a scratch reload made every iteration wait for the prefetched keys).
// A list entry is block-uniform: held in scalar registers once loaded (uni), so that the addresses, modes and
// branches derived from it are scalar.
__device__ __forceinline__ uint4 uni(const uint4& v) {
  return make_uint4(__builtin_amdgcn_readfirstlane(v.x), __builtin_amdgcn_readfirstlane(v.y),
                    __builtin_amdgcn_readfirstlane(v.z), __builtin_amdgcn_readfirstlane(v.w));
}
// list entry j (without a list: the message at position j of the buffer's walk, read from the message buffer; a hole
// of the walk, msg_slots.h, is a DESC_HOLE entry)
__device__ __forceinline__ uint4 diff_entry(const Dev& d, uint32_t b, const uint4* lst, uint32_t j, uint32_t mnf,
                                            uint32_t mR, uint32_t msh, const uint32_t* mfill) {
  if (lst) return lst[j];
  MsgLayout L;
  MsgEnum E;
  msg_walk_from(msh, mR, mnf, L, E);
  const uint32_t i = msg_at(L, E, mfill, j);
  if (i == NEVER) return make_uint4(0u, 0u, 0u, DESC_HOLE);
  const SyncMsg& mm = d.msgs[b][i];
  return make_uint4(i, mm.src, mm.dst, desc_pay(mm));
}

// mnf, mR, msh (the walk's fast positions, R and log2 of the shards, by value: scalars), mfill: the buffer's walk, read
// only without a list (n is then its positions)
template <bool SHARDED>
__device__ __forceinline__ void stream_wide(const Dev& d, uint32_t b, const uint4* lst, uint32_t n, uint32_t blk,
                                            uint32_t nblk, uint32_t* scan, uint32_t& base, uint32_t timed,
                                            uint32_t mnf, uint32_t mR, uint32_t msh, const uint32_t* mfill) {
  const uint32_t nch = d.NCHUNK, total = n * nch;
  uint4 cur[4], dc = make_uint4(0, 0, 0, 0), dn = dc;
  uint32_t pcur = NEVER;
  bool nw;
  if (blk < total) {
    dc = uni(diff_entry(d, b, lst, blk / nch, mnf, mR, msh, mfill));
    diff_fetch<SHARDED>(d, b, dc, blk % nch, cur, pcur, nw, false);
  }
  if (blk + nblk < total) dn = diff_entry(d, b, lst, (blk + nblk) / nch, mnf, mR, msh, mfill);
  for (uint32_t w = blk; w < total; w += nblk) {
    uint4 nxt[4], dnn = make_uint4(0, 0, 0, 0);
    uint32_t pnxt = NEVER;
    const uint4 du = uni(dn);
    if (w + nblk < total) diff_fetch<SHARDED>(d, b, du, (w + nblk) % nch, nxt, pnxt, nw, false);
    if (w + 2 * nblk < total) dnn = diff_entry(d, b, lst, (w + 2 * nblk) / nch, mnf, mR, msh, mfill);
    const uint32_t mi = dc.x, c = w % nch, s0 = c * CH + threadIdx.x * 8;
    const bool hole = dc.w == DESC_HOLE;  // (block-uniform: no message here, nothing counted, compared or written)
    if (!SHARDED && c == 0 && threadIdx.x == 0 && !hole) {  // priced at 8 B per subject (swim_counters)
      atomicAdd(&d.ctr[C_DIFFWIDE_ALL], 1ull);
      if (timed) atomicAdd(&d.ctr[C_DIFFWIDE], 1ull);
    }
    if (pcur != NEVER && s0 < d.NS) {  // a live-row payload read again later (pin_msg)
      uint4* dst = (uint4*)(d.arena[b] + (size_t)pcur * d.NS + s0);
      dst[0] = cur[0];
      dst[1] = cur[1];
    }
    const uint32_t p[8] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y, cur[1].z, cur[1].w};
    const uint32_t r[8] = {cur[2].x, cur[2].y, cur[2].z, cur[2].w, cur[3].x, cur[3].y, cur[3].z, cur[3].w};
    if (!hole) diff_chunk(d, b, mi, c, s0, p, r, scan, base);
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
    dc = du;
    dn = dnn;
    pcur = pnxt;
  }
}

// e0 (uniform), e1: the entries of items blk and blk + nblk, loaded by the caller before the list's length was known
// (indices clamped to the list's capacity: an entry past the length is never used)
template <bool SHARDED>
__device__ __forceinline__ void stream_narrow(const Dev& d, uint32_t b, const uint4* lst, uint32_t n, uint32_t blk,
                                              uint32_t nblk, const uint4& e0, const uint4& e1) {
  // a row shard's list has an entry per message (every item of it is streamed); one GPU's an entry per item, its
  // fourth word item index << 4 | chunks to stream (k_ack_resolve)
  constexpr uint32_t PER = NPER;
  const uint32_t nit = SHARDED ? (d.NCHUNK + PER - 1) / PER : 1u, total = n * nit;
  uint4 cur[4], dc = make_uint4(0, 0, 0, 0), dn = e1;
  uint32_t pw;
  bool nr;
  if (blk < total) {
    dc = e0;
    diff_fetch<SHARDED>(d, b, dc, (SHARDED ? blk % nit : dc.w >> 4) * PER, cur, pw, nr, true);
  }
  for (uint32_t w = blk; w < total; w += nblk) {
    uint4 nxt[4], dnn = make_uint4(0, 0, 0, 0);
    const uint4 du = uni(dn);
    if (w + nblk < total) diff_fetch<SHARDED>(d, b, du, (SHARDED ? (w + nblk) % nit : du.w >> 4) * PER, nxt, pw, nr, true);
    if (w + 2 * nblk < total) dnn = lst[SHARDED ? (w + 2 * nblk) / nit : w + 2 * nblk];
    diff_wave8<SHARDED>(d, b, dc, (SHARDED ? w % nit : dc.w >> 4) * PER, cur);
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
    dc = du;
    dn = dnn;
  }
}

// k_sync_diff: the diff of every payload streamed this tick (see diff_fetch and the stream loops above). The narrow
// items go first, on blocks 0, 1, ... (so a block's first entries are loaded together with the lists' lengths, not
// after them); the wide ones continue from the block after the last narrow one.
// DIFF_WAVES waves per SIMD; the grid is DIFF_WAVES blocks per CU, all resident (diff_grid)
constexpr uint32_t DIFF_WAVES = 7;
template <bool SHARDED>
__global__ void __launch_bounds__(256, DIFF_WAVES) k_sync_diff(const Dev* __restrict__ dp, uint32_t b, uint32_t timed, uint32_t spec) {
  const Dev& d = *dp;  // global, not kernarg (as k_member_tick): a by-value Dev of this size was copied to scratch
  if (spec && halted_diff(d.halt, (spec & LS_LF) != 0u)) return;  // a speculative batch halted at an earlier tick (spec.h)
  __shared__ uint32_t scan[256];
  __shared__ uint32_t base;
  // (timed launches are bracketed by HIP events on the stream. A self-timing variant, first block start to last block
  // end by wall clock and atomics, made every launch of this kernel 30 % slower by its mere presence in the code:
  // 85 -> 112 us per launch at C3, profiles/r03_*)
  // with SYNC_ACK resolution, only the messages k_ack_resolve listed (and counted); without it every message, on
  // 4-B keys
  const bool dl = d.ackres != 0;
  // this block's first two narrow entries, issued before the lengths arrive
  uint4 e0 = make_uint4(0, 0, 0, 0), e1 = e0;
  if (dl) {
    // (one GPU: an entry per item, MSGCAP x items per message of them)
    const uint32_t nit = (d.NCHUNK + NPER - 1) / NPER, cap = (SHARDED ? d.MSGCAP : d.MSGCAP * nit) - 1;
    e0 = ((const uint4*)d.dlist)[min(SHARDED ? blockIdx.x / nit : blockIdx.x, cap)];
    e1 = ((const uint4*)d.dlist)[min(SHARDED ? (blockIdx.x + gridDim.x) / nit : blockIdx.x + gridDim.x, cap)];
  }
  // without lists: the buffer's walk (msg_slots.h), its positions and among them the messages (the holes left out)
  __shared__ uint32_t mfill[MSG_SHARDS_MAX];
  uint32_t mnf = 0, mR = 0, msh = 0;  // the walk's fast positions, R, log2 of the shards
  uint32_t nwide, nnar = 0;
  if (dl) {  // (block-uniform)
    nwide = *(volatile uint32_t*)d.ndlw;
    nnar = *(volatile uint32_t*)d.ndl;
  } else {
    const MsgWalk mw = msg_walk_block(d.ctr_sh, d.msh, d.MSGCAP, b, d.nmsg[b], mfill);
    mnf = mw.E.nfast, mR = mw.L.R, msh = mw.L.sh, nwide = mw.E.total;
  }
  if (!dl && blockIdx.x == 0 && threadIdx.x == 0) {
    uint32_t nmsg = nwide - mnf;
    for (uint32_t s = 0; msh && s < (1u << msh); ++s) nmsg += mfill[s];
    atomicAdd(&d.ctr[C_DIFFMSG_ALL], (unsigned long long)nmsg);
    if (timed) atomicAdd(&d.ctr[C_DIFFMSG], (unsigned long long)nmsg);
    if (SHARDED) {  // (one GPU: stream_wide counts its messages)
      atomicAdd(&d.ctr[C_DIFFWIDE_ALL], (unsigned long long)nmsg);
      if (timed) atomicAdd(&d.ctr[C_DIFFWIDE], (unsigned long long)nmsg);
    }
  }
  const uint32_t nblk = gridDim.x, ntot = SHARDED ? nnar * ((d.NCHUNK + NPER - 1) / NPER) : nnar;
  if (nnar) stream_narrow<SHARDED>(d, b, (const uint4*)d.dlist, nnar, blockIdx.x, nblk, uni(e0), e1);
  stream_wide<SHARDED>(d, b, dl ? (const uint4*)d.dlist_w : nullptr, nwide, (blockIdx.x + nblk - ntot % nblk) % nblk,
                       nblk, scan, base, timed, mnf, mR, msh, mfill);
}

// ------------------------------------------------------------------------------------------------------------
// k_ack_resolve (W == 1): the SYNC_ACKs of tick k-1 whose diff follows from logs instead of a stream.
// Member A's SYNC of tick k-2 carried A's row as of its send; B's diff at tick k-1 extracted D = {s : payload[s] !=
// B's row[s]} (no record the payload lacked, else KF_ABS), B merged D and answered in the same tick with its row at
// that moment. For any subject outside D, outside what B wrote in tick k-1 before the answer and outside what A
// wrote in ticks k-2 and k-1, B's answer and A's row now both equal A's payload. So only the subjects of those three
// logs (tl_add: every key change and every merged candidate) can differ; they are tested here, in subject order,
// into the same pool / chunk_meta form k_sync_diff writes. A message that cannot be resolved this way (no KF_RES, a
// log past TL, a pinned live-row payload, a delayed one) goes to dlist for k_sync_diff. One wave per message.
// the fields k_ack_resolve reads, passed as kernel arguments: through Dev* every one of them was a dependent load of
// its own before the loads that use it (the kernel is a chain of short dependent loads)
struct ResArgs {
  uint32_t* halt;  // Dev::halt
  const uint32_t *nmsg, *tl_tick, *tl_n, *tlog, *rowk, *arena;
  SyncMsg* msgs;
  uint32_t *dlist, *ndl, *dlist_w, *ndlw, *chunk_meta, *pool_used, *err;
  uint64_t* pool;
  unsigned long long* ctr;
  uint32_t NL, NS, MSGCAP, NCHUNK, POOLCAP, NMETA;
  uint32_t k8;  // the 8-bit key plane exists (k_sync_diff streams live-row payloads narrow)
  // W > 1: this shard's first observer, the senders' log prefixes by message (Dev::mlog), and the received payloads
  // (baseline row + shipped chunks, as diff_fetch reads them)
  uint32_t lo, W, MW;
  const uint32_t *mlog, *base_row;
  const uint64_t *rx_mask, *rx_off;
  const uint8_t* xa_recv;
  // one GPU: the rows' dirty-chunk masks when they are consulted (null: every chunk of a narrow payload is streamed),
  // whether the skip statistics are kept (one GPU with masks), the members' records (masks, rebase counters) and the
  // subjects
  MS* dms;
  uint32_t dstat;
  uint32_t N;
  uint32_t* hflag;  // host-mapped (Dev::hflag): HF_STREAMED set when a chunk was streamed (the host then looks at the counters)
  // one GPU with masks consulted and the 8-bit plane: this buffer's inbound lists (Dev::m_head, m_next), walked for
  // the pinned live-row payloads (pin_clean); null otherwise (they go to the wide list)
  const uint32_t *m_head, *m_next;
  unsigned long long* pindec;  // the count of those decided (engine.h SH_PINDEC)
  // the buffer's message-slot shards (msg_slots.h): the counter rows, Dev::msh and the buffer (nmsg above: its overflow
  // count)
  unsigned long long* ctr_sh;
  uint32_t msh, b;
};

// one GPU: the chunks of item t (chunks NPER t ...) of a narrow payload src -> dst that k_sync_diff must stream, one bit
// each: a chunk clean in both rows equals the baseline's in both (row_dirty), so all its compares are decided (equal: no
// candidate, no absent record) without a load. Without masks: every chunk the payload has.
__device__ __forceinline__ uint32_t item_need(const ResArgs& d, uint32_t src, uint32_t dst, uint32_t t) {
  const uint32_t nv = min(NPER, d.NCHUNK - NPER * t), valid = (1u << nv) - 1u;
  if (!d.dms) return valid;
  const uint32_t w = (NPER * t) >> 6;  // (64 is a multiple of NPER: an item's bits lie in one word)
  const uint64_t need = d.dms[src].dirty[w] | d.dms[dst].dirty[w];
  return (uint32_t)(need >> ((NPER * t) & 63u)) & valid;
}

// one GPU: a pinned live-row payload (message i, one of several payloads of receiver dst in this tick: pin_msg) is
// decided from the masks when every payload of the receiver's inbound list is a live row and the receiver's row and
// every one of those senders' rows are clean in every chunk: all those rows equal the baseline, so no payload of the
// list has a candidate or lacks a record, the receiver's P1 merges nothing and tracks no subject, and no later payload
// of the list is ever read (merge_payload, payload_key_at): the pinned copy is not needed either. Every message of the
// list gets the same verdict from the same list. At most PINWALK entries are walked (a longer list, a snapshot or a
// delayed sibling, any dirty bit: false, the payload is streamed wide as before). Wave-uniform.
constexpr uint32_t PINWALK = 8;
__device__ __forceinline__ bool pin_clean(const ResArgs& d, uint32_t i, uint32_t dst, uint32_t lane) {
  uint64_t any = lane < d.MW ? d.dms[dst].dirty[lane] : 0ull;
  bool ok = true, found = false;
  uint32_t q = d.m_head[dst];
  for (uint32_t n = 0; q != NEVER && n < PINWALK; ++n) {
    if (q >= d.MSGCAP) return false;
    const SyncMsg& sm = d.msgs[q];
    const uint32_t nx = d.m_next[q], pay = sm.payload, kind = sm.kind, ssrc = sm.src;
    ok &= pay == NEVER && !(kind & KF_DEFER) && ssrc < d.NL;
    found |= q == i;
    if (ok && lane < d.MW) any |= d.dms[ssrc].dirty[lane];
    q = nx;
  }
  return ok && found && q == NEVER && !__ballot(any != 0ull);
}

// subject v of a message's payload: the sender's live row, its arena snapshot, or (W > 1) a payload received from
// another shard (the shipped chunk if the chunk mask has it, else the baseline row)
__device__ __forceinline__ uint32_t res_payload_key(const ResArgs& d, uint32_t pay, uint32_t src, uint32_t v) {
  if (pay == NEVER) return d.rowk[(size_t)(src - d.lo) * d.NS + v];
  if (!(pay & PAY_RX) || d.W == 1) return d.arena[(size_t)pay * d.NS + v];
  const uint32_t ri = pay & ~PAY_RX, c = v / CH;
  const uint64_t* mk = d.rx_mask + (size_t)ri * d.MW;
  if (!((mk[c >> 6] >> (c & 63)) & 1ull)) return d.base_row[v];
  uint32_t rank = __popcll(mk[c >> 6] & ((1ull << (c & 63)) - 1ull));
  for (uint32_t q = 0; q < (c >> 6); ++q) rank += __popcll(mk[q]);
  return ((const uint32_t*)(d.xa_recv + d.rx_off[ri]))[(size_t)rank * CH + v % CH];
}
// one SYNC_ACK (message i of buffer d.msgs) by one wave: true if it was resolved from the write logs (its candidates
// written), false if k_sync_diff must stream it
__device__ __forceinline__ bool res_wave(const ResArgs& d, uint32_t i, uint32_t k, uint32_t lane, volatile uint32_t* sv,
                                         volatile uint32_t* sc) {
  const SyncMsg& mm = d.msgs[i];
  const uint32_t kind = mm.kind, src = mm.src, dst = mm.dst, tln = mm.tln, pay = mm.payload;
  bool res = k >= 2 && (kind & KF_RES) && !(kind & KF_DEFER) && mm.pin == NEVER && tln <= TL;
  uint32_t n0 = 0, n1 = 0;  // A's log entries of ticks k-2 and k-1
  const uint32_t ld = dst - d.lo;  // the requester: an observer of this shard
  if (res) {
    const size_t a0 = (size_t)(k & 1) * d.NL + ld, a1 = (size_t)((k - 1) & 1) * d.NL + ld;
    n0 = d.tl_tick[a0] == k - 2 ? d.tl_n[a0] : 0u;
    n1 = d.tl_tick[a1] == k - 1 ? d.tl_n[a1] : 0u;
    res = n0 <= TL && n1 <= TL;
  }
  const uint32_t nall = tln + n0 + n1;
  if (!res) return false;
  if (nall == 0) {  // nothing written on either side and nothing merged: nothing can differ
    if (lane == 0) d.msgs[i].ncand = 0;
    return true;
  }
  // gather: B's prefix, then A's two ticks (at most 3 TL <= 64 subjects, one per lane)
  uint32_t v = NEVER;
  if (lane < tln)  // W > 1: the prefix came with the message (the responder may live on another shard)
    v = d.W > 1 ? d.mlog[(size_t)i * TL + lane] : d.tlog[((size_t)((k - 1) & 1) * d.NL + src) * TL + lane];
  else if (lane < tln + n0) v = d.tlog[((size_t)(k & 1) * d.NL + ld) * TL + (lane - tln)];
  else if (lane < tln + n0 + n1) v = d.tlog[((size_t)((k - 1) & 1) * d.NL + ld) * TL + (lane - tln - n0)];
  sv[lane] = v;
  __builtin_amdgcn_wave_barrier();
  bool first = v != NEVER;
  for (uint32_t j = 0; j < min(lane, nall); ++j) first &= sv[j] != v;
  uint32_t key = 0;
  bool cand = false;
  if (first) {
    key = res_payload_key(d, pay, src, v);
    cand = (key & 3u) != ST_ABSENT && key != d.rowk[(size_t)ld * d.NS + v];
  }
  sc[lane] = cand ? v : NEVER;
  __builtin_amdgcn_wave_barrier();
  const uint64_t cb = __ballot(cand);
  const uint32_t total = (uint32_t)__popcll(cb);
  uint32_t off = 0;
  if (total) {  // (wave-uniform; none in the C3 steady state)
    uint32_t pos = 0;
    for (uint32_t j = 0; j < nall; ++j) pos += sc[j] < v;
    if (lane == 0) {
      off = atomicAdd(d.pool_used, total);
      if (off + total > d.POOLCAP) {
        atomicOr(d.err, E_POOL);
        off = NEVER;
      }
    }
    off = __shfl(off, 0);
    if (cand && off != NEVER) d.pool[(size_t)off + pos] = ((uint64_t)v << 34) | key34(key);
  }
  // per chunk: first candidate and count (the chunk walk of merge_payload, which reads none of it when ncand is 0)
  if (total && off != NEVER)
    for (uint32_t c = lane; c < d.NMETA; c += 64) {
      uint32_t before = 0, in = 0;
      for (uint32_t j = 0; j < nall; ++j) {
        const uint32_t t = sc[j];
        before += t < c * MCH;
        in += t != NEVER && t / MCH == c;
      }
      uint32_t* cm = d.chunk_meta + ((size_t)i * d.NMETA + c) * 2;
      cm[0] = off + before;
      cm[1] = in;
    }
  if (lane == 0) d.msgs[i].ncand = off == NEVER ? 0u : total;
  return true;
}

// sharded handles: every message of the tick, one wave each; the unresolved ones go to the list k_sync_diff streams
// One GPU: an unresolved narrow payload is listed item by item, only the items with a chunk that is dirty in the
// sender's or in the receiver's row (item_need); the other items' candidate segments get their zero counts here, and a
// payload without any such chunk is decided here (ncand = 0, no entry: merge_payload reads no chunk_meta then).
// spec: LS_SPEC = a launch of a speculative batch; | LS_NODIFF = no k_sync_diff follows this launch (one GPU, an untimed
// tick of a batch that elides the diff, step.hip): a block that lists an entry raises the diff-halt of its tick, after
// which every later launch of the batch returns at once and the host runs diff(k) itself. The blocks of this launch go
// on whatever their own tick's diff-halt says (halted_lister: the list must be complete); nothing waits on the device.
__global__ void __launch_bounds__(512) k_ack_resolve(ResArgs d, uint32_t k, uint32_t spec, uint32_t timed) {
  if (spec && halted_lister(d.halt, k, (spec & LS_LF) != 0u)) return;
  __shared__ uint32_t sv_[8][64], sc_[8][64];
  __shared__ uint4 wlist[8];
  // per block and round: narrow list entries, wide ones, resolved messages, narrow messages (listed or decided here),
  // those decided here, their chunks streamed and the subjects of those
  // (npind: pinned live-row payloads decided from the masks, counted with the narrow ones decided here)
  __shared__ uint32_t nstream, nwide, nres, nnarm, nskipm, nchs, nsubj, sbase, wbase, npind;
  // chunk compares streamed, per chunk, added up per block (k_rebase's policy; a chunk past SCH: global atomics)
  constexpr uint32_t SCH = 512;
  __shared__ uint32_t sch[SCH];
  if (d.dms) {
    if (threadIdx.x < SCH) sch[threadIdx.x] = 0;
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  volatile uint32_t* sv = sv_[wv];  // this wave's lists (volatile: read across lanes)
  volatile uint32_t* sc = sc_[wv];
  // the buffer's messages: its slots in use, walked densely (msg_slots.h)
  const MsgDense mw = msg_walk_wave(d.ctr_sh, d.msh, d.MSGCAP, d.b, d.nmsg, lane);
  const uint32_t npos = mw.total;
  const bool items = d.W == 1;  // the narrow list's form (engine.h NPER)
  const uint32_t nit = (d.NCHUNK + NPER - 1) / NPER;
  // block-uniform loop, one message per wave; the stream list and the counters take one atomic per block (a few
  // hundred waves adding to one address one by one took ~17 us per tick at C3)
  for (uint32_t base = blockIdx.x * 8; base < npos; base += gridDim.x * 8) {
    if (threadIdx.x == 0) nstream = nwide = nres = nnarm = nskipm = nchs = nsubj = npind = 0;
    __syncthreads();
    const uint32_t i = base + wv < npos ? msg_at_wave(mw, base + wv) : NEVER;  // (NEVER: past the end)
    uint32_t woff = 0, wcnt = 0, src = 0, dst = 0, pw = 0;  // this wave's narrow entries: place in the block's, count
    if (i != NEVER) {  // wave-uniform
      if (res_wave(d, i, k, lane, sv, sc)) {
        if (lane == 0) atomicAdd(&nres, 1u);
      } else {  // its entries in the narrow list (one GPU, unpinned live row) or its entry in the wide one
        const SyncMsg& mm = d.msgs[i];
        src = mm.src, dst = mm.dst, pw = desc_pay(mm);
        if (d.m_head && mm.payload == NEVER && pw != NEVER && pw != DESC_DEFER && pin_clean(d, i, dst, lane)) {
          if (lane == 0) {  // decided: no entry, no pinned copy; a read of it would raise E_PIN (payload_key_at)
            d.msgs[i].ncand = 0;
            d.msgs[i].pin = NEVER;
            atomicAdd(&nnarm, 1u);
            atomicAdd(&nskipm, 1u);
            atomicAdd(&npind, 1u);
          }
        } else if (d.k8 && (pw == NEVER || (d.W > 1 && pw != DESC_DEFER && (pw & PAY_RX) && !(pw & DESC_PIN)))) {
          uint32_t nc = 0;  // this lane's items' chunks to stream
          if (items) {
            for (uint32_t t0 = 0; t0 < nit; t0 += 64) {
              const uint32_t m4 = t0 + lane < nit ? item_need(d, src, dst, t0 + lane) : 0u;
              wcnt += (uint32_t)__popcll(__ballot(m4 != 0));
              nc += __popc(m4);
              if (d.dms)  // (with masks a streamed chunk is the rare case)
                for (uint32_t q = m4; q; q &= q - 1) {
                  const uint32_t c = NPER * (t0 + lane) + (uint32_t)(__ffs(q) - 1);
                  if (c < SCH) atomicAdd(&sch[c], 1u);
                  else atomicAdd(&d.dms[c].cstat[0], 1ull);
                  d.dms[c].cstat[2] = src;  // (any sender of the chunk serves as k_rebase's row)
                }
            }
          } else {
            wcnt = 1;
          }
          if (items && nc) {
            atomicAdd(&nchs, nc);
            atomicAdd(&nsubj, nc * CH);
          }
          if (lane == 0) {
            atomicAdd(&nnarm, 1u);
            if (wcnt) woff = atomicAdd(&nstream, wcnt);
            else {
              d.msgs[i].ncand = 0;  // every compare decided: nothing differs
              atomicAdd(&nskipm, 1u);
            }
            // (the last chunk's subjects: up to N)
            if (items && (item_need(d, src, dst, nit - 1) >> ((d.NCHUNK - 1) % NPER)) & 1u)
              atomicSub(&nsubj, d.NCHUNK * CH - d.N);
          }
          woff = __shfl(woff, 0);
        } else if (lane == 0) {
          wlist[atomicAdd(&nwide, 1u)] = make_uint4(i, src, dst, pw);
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      if (nstream) sbase = atomicAdd(d.ndl, nstream);
      if (nwide) wbase = atomicAdd(d.ndlw, nwide);
      if (d.m_head && nstream + nwide) {  // work for k_sync_diff: counted for the host, and a halt if none is queued
        count_listed(d.halt, nstream + nwide);
        if (spec & LS_NODIFF) raise_diff_halt(d.halt, k);
      }
      if (nnarm + nwide) {  // the messages k_sync_diff streams (the wide ones: 8 B per subject) or this kernel decided
        atomicAdd(&d.ctr[C_DIFFMSG_ALL], (unsigned long long)(nnarm + nwide));
        if (timed) atomicAdd(&d.ctr[C_DIFFMSG], (unsigned long long)(nnarm + nwide));
      }
      if (nwide && d.W > 1) {  // (one GPU: k_sync_diff counts its wide messages)
        atomicAdd(&d.ctr[C_DIFFWIDE_ALL], (unsigned long long)nwide);
        if (timed) atomicAdd(&d.ctr[C_DIFFWIDE], (unsigned long long)nwide);
      }
      if (nres) {
        atomicAdd(&d.ctr[C_ACKRES_ALL], (unsigned long long)nres);
        if (timed) atomicAdd(&d.ctr[C_ACKRES], (unsigned long long)nres);
      }
      if (d.dstat && nnarm) {
        if (nchs) {
          atomicAdd(&d.ctr[C_DSTREAM], (unsigned long long)nchs);
          atomicAdd(&d.ctr[C_DSUBJ_ALL], (unsigned long long)nsubj);
          if (timed) atomicAdd(&d.ctr[C_DSUBJ], (unsigned long long)nsubj);
        }
        if (nskipm) atomicAdd(&d.ctr[C_DMSGSKIP], (unsigned long long)nskipm);
        if (npind) atomicAdd(d.pindec, (unsigned long long)npind);
        if (nchs && d.dms) *(volatile uint32_t*)(d.hflag + HF_STREAMED) = 1u;
      }
    }
    __syncthreads();
    if (d.dms && nchs)  // (block-uniform)
      for (uint32_t c = threadIdx.x; c < min(d.NCHUNK, SCH); c += blockDim.x)
        if (const uint32_t v = sch[c]) {
          atomicAdd(&d.dms[c].cstat[0], (unsigned long long)v);
          sch[c] = 0;
        }
    if (wcnt && !items) {
      if (lane == 0) ((uint4*)d.dlist)[sbase + woff] = make_uint4(i, src, dst, pw);
    } else if (wcnt) {
      uint32_t o = sbase + woff;
      for (uint32_t t0 = 0; t0 < nit; t0 += 64) {
        const uint32_t t = t0 + lane, m4 = t < nit ? item_need(d, src, dst, t) : 0u;
        const unsigned long long em = __ballot(m4 != 0);
        if (m4) ((uint4*)d.dlist)[o + (uint32_t)__popcll(em & ((1ull << lane) - 1ull))] = make_uint4(i, src, dst, t << 4 | m4);
        o += (uint32_t)__popcll(em);
        if (t < nit && !m4)  // an item without a chunk to stream: its segments' zero counts (merge_payload's chunk walk)
          for (uint32_t g = 2 * NPER * t; g < min(2 * NPER * (t + 1), d.NMETA); ++g) {
            uint32_t* cm = d.chunk_meta + ((size_t)i * d.NMETA + g) * 2;
            cm[0] = cm[1] = 0;
          }
      }
    }
    if (threadIdx.x >= 64 && threadIdx.x - 64 < nwide) ((uint4*)d.dlist_w)[wbase + threadIdx.x - 64] = wlist[threadIdx.x - 64];
    __syncthreads();  // (wlist and the counts are reused)
  }
}

// one GPU, between steps: a host write of one key (swim_debug_set_incarnation)
__global__ void k_key_set(Dev d, uint32_t m, uint32_t s, uint32_t key) {
  uint32_t* rk = d.rowk + (size_t)m * d.NS;
  key_put(d, rk, row_dirty(d, m), m, s, key, rk[s]);
}
void launch_key_set(const Dev& d, uint32_t m, uint32_t s, uint32_t key, void* stream) {
  hipLaunchKernelGGL(k_key_set, dim3(1), dim3(1), 0, (hipStream_t)stream, d, m, s, key);
}

// one GPU, between ticks: chunk c of row r becomes chunk c of the baseline. Every row's bit c is recomputed against it
// (set iff the row's chunk differs from row r's: exact for any r, which only decides how many rows come out clean).
// The baseline is not stored: it is what the clean rows hold. The chunk's policy counters start again. One block per
// row, grid-strided.
__global__ void __launch_bounds__(256) k_rebase(Dev d, uint32_t c, uint32_t r) {
  const uint32_t s0 = c * CH, s1 = min((c + 1) * CH, d.NS);
  const uint32_t* rr = d.rowk + (size_t)r * d.NS;
  for (uint32_t li = blockIdx.x; li < d.NL; li += gridDim.x) {
    const uint32_t* rk = d.rowk + (size_t)li * d.NS;
    bool diff = false;
    for (uint32_t s = s0 + threadIdx.x; s < s1; s += blockDim.x) diff |= rk[s] != rr[s];
    diff = __syncthreads_or(diff);
    if (threadIdx.x == 0) {
      uint64_t* w = row_dirty(d, li) + (c >> 6);
      const uint64_t bit = 1ull << (c & 63);
      *w = diff ? *w | bit : *w & ~bit;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) d.ms[c].cstat[0] = d.ms[c].cstat[1] = 0;
}
void launch_rebase(const Dev& d, uint32_t c, uint32_t r, void* stream) {
  hipLaunchKernelGGL(k_rebase, dim3(min(d.NL, 4096u)), dim3(256), 0, (hipStream_t)stream, d, c, r);
}

// one GPU, between batches (step.hip, before the lister-free mode is entered): is any chunk of any row dirty? One pass
// over the members' records; a wave that finds a set bit stores HALT_MASKS (the host cleared it).
__global__ void __launch_bounds__(256) k_masks_any(Dev d) {
  const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t any = 0;
  if (li < d.NL)
    for (uint32_t w = 0; w < d.MW; ++w) any |= d.ms[li].dirty[w];
  if (__ballot(any != 0ull) && (threadIdx.x & 63u) == 0) *(volatile uint32_t*)(d.halt + HALT_MASKS) = 1u;
}
void launch_masks_any(const Dev& d, void* stream) {
  hipMemsetAsync(&d.halt[HALT_MASKS], 0, 4, (hipStream_t)stream);
  hipLaunchKernelGGL(k_masks_any, dim3((d.NL + 255) / 256), dim3(256), 0, (hipStream_t)stream, d);
}

// one GPU: the dirty masks' invariant, tested directly: all the rows whose bit c is clear hold the same chunk c (keys,
// and their 8-bit shadows): the baseline's. k_dirty_ref finds, per chunk, the first such row; k_dirty_check compares
// every other one with it, one block per (row, chunk), grid-strided, and counts the dirty pairs.
__global__ void k_dirty_ref(Dev d, uint32_t* ref) {
  const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= d.NL) return;
  const uint64_t* rd = row_dirty(d, li);
  for (uint32_t c = 0; c < d.NCHUNK; ++c)
    if (!((rd[c >> 6] >> (c & 63)) & 1ull)) atomicMin(&ref[c], li);
}
__global__ void __launch_bounds__(256) k_dirty_check(Dev d, uint32_t* viol, uint32_t* ndirty, const uint32_t* ref) {
  const uint64_t total = (uint64_t)d.NL * d.NCHUNK;
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint32_t li = (uint32_t)(w / d.NCHUNK), c = (uint32_t)(w % d.NCHUNK);
    if ((row_dirty(d, li)[c >> 6] >> (c & 63)) & 1ull) {
      if (threadIdx.x == 0) atomicAdd(ndirty, 1u);
      continue;
    }
    const size_t r = ref[c];  // (a clean row exists: this one)
    bool bad = false;
    for (uint32_t s = c * CH + threadIdx.x; s < min((c + 1) * CH, d.NS); s += blockDim.x) {
      bad |= d.rowk[(size_t)li * d.NS + s] != d.rowk[r * d.NS + s];
      if (d.rowk8) bad |= d.rowk8[(size_t)li * d.NS8 + s] != key8(d.rowk[r * d.NS + s]);
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicAdd(viol, 1u);
  }
}
void launch_dirty_check(const Dev& d, uint32_t* viol, uint32_t* ndirty, uint32_t* ref, void* stream) {
  hipMemsetAsync(ref, 0xFF, 4ull * d.NCHUNK, (hipStream_t)stream);
  hipLaunchKernelGGL(k_dirty_ref, dim3((d.NL + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, ref);
  hipLaunchKernelGGL(k_dirty_check, dim3(4096), dim3(256), 0, (hipStream_t)stream, d, viol, ndirty, ref);
}

// timed: this launch is bracketed by profiling events; it adds its message count to ctr[C_DIFFMSG]
// DIFF_WAVES resident blocks per CU (the launch bounds), all of them resident; SWIM_DIFF_GRID overrides it
// (measurements; a value that does not parse, or 0, keeps the default)
static uint32_t diff_grid() {
  const char* e = getenv("SWIM_DIFF_GRID");
  const unsigned long v = e ? strtoul(e, nullptr, 0) : 0ul;
  if (v >= 1 && v <= (1ul << 20)) return (uint32_t)v;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  return DIFF_WAVES * (uint32_t)cus;
}

// a timed launch carries its start / stop events in its own dispatch (hipExtLaunchKernelGGL): the interval is the
// kernel's, not that of two marker packets around it (those read ~4 us per launch longer than rocprofv3)
// grid_arg: 0 = that grid (every engine launch); the known-answer tests pass their own (swim_debug_prim_eval)
static void launch_sync_diff(const Dev& d, uint32_t b, hipStream_t st, uint32_t timed, uint32_t spec = 0,
                             const TickEvents* prof = nullptr, uint32_t grid_arg = 0) {
  static const uint32_t own = diff_grid();
  const uint32_t grid = grid_arg ? grid_arg : own;
  if (prof) {
    hipEvent_t e0 = (hipEvent_t)prof->ev[0], e1 = (hipEvent_t)prof->ev[1];
    if (d.W > 1)
      hipExtLaunchKernelGGL(k_sync_diff<true>, dim3(grid), dim3(256), 0, st, e0, e1, 0, d.self, b, timed, spec);
    else
      hipExtLaunchKernelGGL(k_sync_diff<false>, dim3(grid), dim3(256), 0, st, e0, e1, 0, d.self, b, timed, spec);
  } else if (d.W > 1) {
    hipLaunchKernelGGL(k_sync_diff<true>, dim3(grid), dim3(256), 0, st, d.self, b, timed, spec);
  } else {
    hipLaunchKernelGGL(k_sync_diff<false>, dim3(grid), dim3(256), 0, st, d.self, b, timed, spec);
  }
}

// single GPU: the tick is cut in three so that the host can hold back the gossip data plane when no slot is in
// use; the SYNC diff of tick k+1 does not depend on the gossip plane of tick k and is queued in between
// SYNC_ACKs of tick k - 1 resolved from write logs (the rest go to the list k_sync_diff streams)
static void launch_ack_resolve(const Dev& d, uint32_t k, hipStream_t st, uint32_t ls, bool timed) {
  if (k == 0 || !d.ackres) return;
  const uint32_t b = (k - 1) & 1;
  const bool lists = diff_elidable(d);
  const ResArgs ra{d.halt, d.nmsg + b, d.tl_tick, d.tl_n, d.tlog, d.rowk, d.arena[b], d.msgs[b], d.dlist, d.ndl,
                   d.dlist_w, d.ndlw, d.chunk_meta, d.pool_used, d.err, d.pool, d.ctr, d.NL, d.NS, d.MSGCAP, d.NCHUNK, d.POOLCAP, d.NMETA,
                   d.rowk8 ? 1u : 0u, d.lo, d.W, d.MW, d.mlog, d.base_row, d.rx_mask, d.rx_off, d.xa_recv,
                   (d.ackres & ACKRES_DIRTY) ? d.ms : nullptr, d.W == 1 && d.MW ? 1u : 0u, d.N, d.hflag,
                   lists ? d.m_head + (size_t)b * d.N : nullptr, lists ? d.m_next + (size_t)b * d.MSGCAP : nullptr,
                   d.ctr_sh + SH_PINDEC, d.ctr_sh, d.msh, b};
  hipLaunchKernelGGL(k_ack_resolve, dim3(128), dim3(512), 0, st, ra, k, ls, timed ? 1u : 0u);
}

void launch_diff(const Dev& d, uint32_t k, void* stream, const TickEvents* prof, uint32_t ls, uint32_t grid) {
  hipStream_t st = (hipStream_t)stream;
  if (!diff_elidable(d)) ls &= ~LS_NODIFF;
  launch_ack_resolve(d, k, st, ls, prof != nullptr);
  if (k > 0 && !(ls & LS_NODIFF)) launch_sync_diff(d, (k - 1) & 1, st, prof ? 1u : 0u, ls & (LS_SPEC | LS_LF), prof, grid);
}

void launch_diff_listed(const Dev& d, uint32_t k, void* stream, uint32_t grid) {
  if (k > 0) launch_sync_diff(d, (k - 1) & 1, (hipStream_t)stream, 0u, 0u, nullptr, grid);
}

}  // namespace swim
