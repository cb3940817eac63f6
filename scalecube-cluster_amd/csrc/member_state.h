// member_state.h — one member's protocol state as the member kernels hold it (ML), its load and store, the state a
// parked member keeps between the three launches of a split tick, and the operations every handler goes through: row
// reads and writes with the deferred copy-on-write of SYNC payloads, the write log, SYNC sends and the selector draws.
// The handlers are in member_proto.h; the kernels in member.hip (k_member_tick_t) and inbox.hip (k_inbox_apply).
#pragma once
#include "dev_util.h"

namespace swim {

enum Reason : uint32_t { R_FD = 0, R_GOSSIP = 1, R_SYNC = 2, R_INITIAL = 3, R_TIMEOUT = 4 };
enum : uint32_t { INIT_ACTIVE = 1, INIT_RECEIVED = 2 };
enum : uint32_t { GF_USED = 1, GF_ERROR = 2, GF_SEALED = 4 };
// path stages: 1..3 = pending hop at `tick`, 9 = ack arrives at `tick`
enum : uint32_t { P_DIRECT = 0x10, P_REQ = 0x20, P_ARRIVE = 9 };

struct ML {
  const Dev* d;
  uint32_t m, k, N;
  uint32_t tsize, fdLen, gLen, fdPeriod, gCounter, nextPing, nextGossip, nextSync, cidCnt, syncSeq, evSeq,
      held, timerMin, initFlags, initDeadline, initCidBase, initN, nsub, npath, nfetch;
  int ep;          // NetworkEmulator settings epoch of tick k (epoch_at, looked up once)
  uint32_t fnext;  // earliest tick at which a pending fetch needs the member (hop, arrival or timeout); NEVER: none
  int32_t pingIdx, remoteIdx;
  uint64_t evHash;
  uint32_t *rk, *ra;  // this observer's row: key plane and aux plane (swim_common.h)
  uint64_t* rd;       // its dirty-chunk mask (row_dirty); null when none is kept
  uint32_t *fdl, *gl, *subs, *paths, *fetch, *groups;
  uint32_t c[8];  // this tick's op counters (one member, one tick: u32; summed per wave in u64)
  uint32_t pend;  // this tick's SYNC messages that carry the live row: a chain through SyncMsg.pad (NEVER = none)
  uint32_t tround;
  // subjects whose key changed in this tick's P1 (several payloads only): the first TRKL listed, all of them in the
  // bitmap tb (one bit per subject); ntrk counts them
  uint32_t* trk;
  uint32_t ntrk;
  bool trk_on;
  // deferred copy-on-write (cow): open snapshots of this member (indices into the block's list cw) and its undo log
  uint4* cw;       // block list (LDS): member, arena row, first log entry, log length at the end of the body
  uint32_t* cw_n;  // LDS counter of cw
  uint32_t* ulog;  // this member's log: (subject, key before the write) per row write while a snapshot is open
  uint32_t ncreq, nlog;  // open snapshots (their cw entries carry this member's id), logged writes
  uint32_t* spq;  // gossips created this tick that wait for their slots (flush_spreads): [SPQ][8] gid, subj, key
  uint32_t nsp;
  // ArrayList.add(index) inserts of this tick not applied to fdl yet (fd_flush), sorted by their final position;
  // fdLen counts them
  uint32_t* fpend;
  uint32_t npend;
  // SYNC_ACK resolution (d.ackres): this tick's write log (Dev::tlog), its length (> TL: overflowed) and last entry;
  // the group of the SYNC merged just now whose SYNC_ACK may be resolved (-1: none)
  uint32_t* tl;
  uint32_t ntl, tlast;
  // the FD list entry the P6 ping takes and its dead_tick, loaded with the member state when the ping is due and the
  // cursor needs no reshuffle (compared only at the ping, so nothing waits for them before); pre = NEVER when not
  // loaded or once the list changes in this tick
  uint32_t pre, pre_dt;
  // the last SYNC / SYNC_ACK this lane linked into its receiver's inbound list (W == 1): the list-link exchange's old
  // head, written to m_next with the pins at the next send or at the end of the body (link_flush), so that the
  // exchange's round trip overlaps the lane's next loads instead of holding them (NEVER: none pending)
  uint32_t lk_i, lk_o;
  // the earliest pending path tick and subscription deadline, kept in registers once P2 and P5 have walked the lists
  // (NEVER: none), so the next-event minimum at the end of the body needs no loads of entries just stored; ev_ok says
  // whether they are known (not in a resumed launch, whose P2 ran in the launch before)
  uint32_t pmin, smin;
  bool ev_ok;
  int rgrp;
  bool spec;  // a launch of a one-GPU speculative batch: a member that takes a gossip slot raises d.halt (k_member_tick)
};

// A tick without a lister launch (a lister-free batch: every row equals the baseline, both write logs k_ack_resolve
// would read are empty, no payload is a snapshot or delayed): what the lister would have counted for
// one message, from the fields it tests. Resolved from the (empty) write logs under res_wave's preconditions (k >= 2
// holds in the mode); else a narrow message decided without a stream, pinned or not (pin_clean holds for every list of
// at most PINWALK payloads: all its rows are clean). The limit of this: the lister sends the pinned payloads of a
// longer list to the wide diff, which finds nothing in them either, and counts them there (C_DIFFWIDE_ALL, 8 B per
// subject in diff_key_bytes, a diff-halt under elision); here they count as decided like the others. The results are
// the same (ncand = 0 either way); those counters would differ from a run with a lister on every tick. Nine payloads
// for one receiver in one tick of a clean steady state is a ~10^-12 event per receiver and tick at a SYNC every 10
// ticks and rarer at the default interval.
// Packed, LFC_BITS bits each: resolved, narrow decided, of those pinned (SH_LF's order).
constexpr uint32_t LFC_BITS = 21, LFC_MASK = (1u << LFC_BITS) - 1u;
__device__ __forceinline__ uint64_t lf_count(uint32_t kind, uint32_t pin, uint32_t tln) {
  if ((kind & KF_RES) && !(kind & KF_DEFER) && pin == NEVER && tln <= TL) return 1ull;
  return (1ull << LFC_BITS) | (pin != NEVER ? 1ull << (2 * LFC_BITS) : 0ull);
}

// a subject whose key this member's row changed in this tick, or a candidate of a payload it merged (k_ack_resolve)
// (in a speculative batch the first entry of a tick also tells the host that this launch wrote: note_wrote, spec.h; not
// elsewhere: 10^5 members that accept one gossip in one tick would queue as many stores at that word's L2 channel)
__device__ __forceinline__ void tl_add(ML& L, uint32_t s) {
  if (L.ntl && L.tlast == s) return;  // merge_record's candidate, then its row_put
  if (!L.ntl && L.spec) note_wrote(L.d->halt, L.k);
  if (L.ntl < TL) L.tl[L.ntl] = s;
  if (L.ntl <= TL) L.ntl++;
  L.tlast = s;
}

// the selector counters live in memory (Dev::sel), not in the member's registers: draws are rare next to the
// registers every member-kernel wave would hold for them
__device__ __forceinline__ uint32_t draw_at(const ML& L, uint32_t stream, uint32_t c) {
  return philox(L.m, stream, c, 0, L.d->seed_lo ^ SALT_SEL, L.d->seed_hi).x;
}
__device__ __forceinline__ uint32_t draw(ML& L, uint32_t stream) {
  uint32_t* p = L.d->sel + (size_t)L.m * 8 + stream;
  const uint32_t c = *p;
  *p = c + 1u;
  return draw_at(L, stream, c);
}

// Collections.shuffle: for i = size..2: swap(i-1, nextInt(i))
__device__ __forceinline__ void shuffle_list(ML& L, uint32_t* v, uint32_t n, uint32_t stream) {
  uint32_t* p = L.d->sel + (size_t)L.m * 8 + stream;
  uint32_t c = *p;
  if (n > 1) *p = c + (n - 1u);
  for (uint32_t i = n; i > 1; --i) {
    uint32_t j = next_int(draw_at(L, stream, c++), i);
    uint32_t t = v[i - 1];
    v[i - 1] = v[j];
    v[j] = t;
  }
}

// copy-on-write of the live row for SYNC payloads sent earlier in this tick. The payloads take an
// arena row; the copy itself is deferred to the end of k_member_tick, where the member's whole block copies the row
// (coalesced) and then undoes, newest first, the writes the member logged after this point (row_put). One lane
// copying N words would hold the whole kernel (~3 ms per tick at 100k members when a SYNC sender also merges a
// gossip in the same tick). Past CREQ open snapshots, ULOG logged writes or CWMAX snapshots per block, the copy is
// made here, by this lane (cow_now).
__device__ __forceinline__ void copy_row_to(ML& L, uint32_t r) {
  const Dev& d = *L.d;
  const uint32_t b = L.k & 1;
  const uint4* src4 = (const uint4*)L.rk;  // keys only, with the zero padding k_sync_diff reads up to NS
  uint4* dst4 = (uint4*)(d.arena[b] + (size_t)r * d.NS);
#pragma unroll 16
  for (uint32_t s = 0; s < d.NS / 4; ++s) dst4[s] = src4[s];
  if (d.W > 1)
    for (uint32_t w = 0; w < d.MW; ++w) d.arena_dirty[b][(size_t)r * d.MW + w] = L.rd[w];
}

// the open snapshots, now: live row, then the logged writes since each one opened undone newest first
__device__ __forceinline__ void cow_now(ML& L) {
  const Dev& d = *L.d;
  const uint32_t b = L.k & 1;
  const uint32_t n = min(*L.cw_n, d.cwmax_cap);
  for (uint32_t q = 0; q < n; ++q) {
    uint4& e = L.cw[q];
    if (e.x != L.m) continue;  // another member's (entries are NEVER until written)
    copy_row_to(L, e.y);
    uint32_t* dst = d.arena[b] + (size_t)e.y * d.NS;
    for (uint32_t j = L.nlog; j-- > e.z;) dst[L.ulog[2 * j]] = L.ulog[2 * j + 1];
    e.x = NEVER;  // done: the block epilogue skips it
  }
  L.ncreq = 0;
  L.nlog = 0;
}

__device__ __forceinline__ void cow(ML& L) {
  const Dev& d = *L.d;
  uint32_t b = L.k & 1;
  uint32_t r = atomicAdd(&d.arena_used[b], 1u);
  if (r >= d.ARENA_ROWS) {
    set_err(d, E_ARENA);
    L.pend = NEVER;
    return;
  }
  if (L.spec) note_wrote(d.halt, L.k);  // snapshot payloads: the lister's verdict on them is no constant (spec.h)
  for (uint32_t i = L.pend; i != NEVER; i = d.msgs[b][i].pad) d.msgs[b][i].payload = r;
  L.pend = NEVER;
  if (L.ncreq == d.creq_cap) {  // rare: many send-then-write rounds in one tick
    fb_add(d, FB_CREQ);
    cow_now(L);
  }
  const uint32_t idx = atomicAdd(L.cw_n, 1u);  // LDS
  if (idx >= d.cwmax_cap) {  // the block's list is full: this snapshot now, by this lane
    fb_add(d, FB_CWMAX);
    copy_row_to(L, r);
    return;
  }
  L.cw[idx] = make_uint4(L.m, r, L.nlog, 0u);
  L.ncreq++;
}

// the member's open snapshots sealed when it leaves the launch: the log length the block epilogue of k_member_tick
// undoes from (the writes logged so far)
__device__ __forceinline__ void cow_seal(ML& L) {
  if (L.ncreq)
    for (uint32_t q = 0, n = min(*L.cw_n, L.d->cwmax_cap); q < n; ++q)
      if (L.cw[q].x == L.m) L.cw[q].w = L.nlog;
}

__device__ __forceinline__ uint64_t row_ld(const ML& L, uint32_t s) { return rec_join(L.rk[s], L.ra[s]); }
__device__ __forceinline__ uint32_t row_status(const ML& L, uint32_t s) { return L.rk[s] & 3u; }

// old: the key the row holds for s now (callers that loaded it already pass it: no load after this lane's stores)
__device__ __forceinline__ void row_put(ML& L, uint32_t s, uint64_t v, uint32_t old) {
  const uint32_t k = key32(v);
  if (rec_inc(v) >= INC_LIMIT) set_err(*L.d, E_INC);
  if (L.pend != NEVER && old != k) cow(L);
  if (L.ncreq && old != k) {  // an open snapshot: log the key this write replaces
    if (L.nlog == L.d->ulog_cap) {
      fb_add(*L.d, FB_ULOG);
      cow_now(L);
    } else {
      L.ulog[2 * L.nlog] = s;
      L.ulog[2 * L.nlog + 1] = old;
      L.nlog++;
    }
  }
  if (L.trk_on && old != k) {  // merge_payload re-checks it against the later payloads
    unsigned long long* tw = L.d->tbm + lidx(*L.d, L.m) * L.d->NW + (s >> 6);
    const unsigned long long bit = 1ull << (s & 63u), old = *tw;
    if (!(old & bit)) {
      *tw = old | bit;
      if (L.ntrk < TRKL) L.trk[L.ntrk] = s;
      L.ntrk++;
    }
  }
  if (L.d->ackres && old != k) tl_add(L, s);
  key_put(*L.d, L.rk, L.rd, lidx(*L.d, L.m), s, k, old);
  L.ra[s] = aux32(v);
}
__device__ __forceinline__ void row_put(ML& L, uint32_t s, uint64_t v) { row_put(L, s, v, L.rk[s]); }

__device__ __forceinline__ void link_flush(ML& L) {
  if (L.lk_i == NEVER) return;
  const Dev& d = *L.d;
  const uint32_t b = L.k & 1, i = L.lk_i, old = L.lk_o;
  d.m_next[(size_t)b * d.MSGCAP + i] = old;
  if (old != NEVER) {  // a receiver with several payloads this tick: both pinned (pin_msg)
    pin_msg(d, b, i);
    pin_msg(d, b, old);
  }
  L.lk_i = NEVER;
}

// SWIM_EXP & 512 (the wave clock, member.hip), on the light path only (send_sync<true>, member_light.h: the steady
// state's sends; the general body's sends, k_inbox_apply's among them, compile without the stamps, which cost its
// split-tick instance 18 more spilled VGPRs): the first lane active here stamps the wall clock into word w of its wave's
// stamps, once `after` has arrived (the result of the atomic the stamp follows: the wave waits for it here, under the
// experiment only). Nothing executes with the bit off. The light path runs only in k_member_tick_t<BODY_FULL>, whose
// grid Dev::wt is sized for.
template <bool STAMP>
__device__ __forceinline__ void send_stamp(const Dev& d, uint32_t w, uint32_t after = 0u) {
  if constexpr (STAMP) {
    if (!(d.exp & EXP_WAVE_CLOCK)) return;
    asm volatile("" ::"v"(after));
    if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)__ballot(1)) - 1))
      d.wt[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * WT_WORDS + w] = wall_clock64();
  }
}

// prepareSyncDataMsg (MembershipProtocolImpl.java:446-454) + transport.send; false if the send failed
// res: a SYNC_ACK sent in the tick its SYNC was merged (k_ack_resolve may derive its diff from the write logs)
// dd: xmit_ep's (whether dst is dead at k, when the caller knows; -1: looked up)
// STAMP: the light path's instance, with the wave clock's stamps (send_stamp)
template <bool STAMP = false>
__device__ __forceinline__ bool send_sync(ML& L, uint32_t kind, uint32_t dst, uint32_t ciss, uint32_t ccnt,
                                          bool res = false, int dd = -1) {
  const Dev& d = *L.d;
  uint32_t seq = L.syncSeq++;
  L.c[C_M]++;
  const int e = xmit_ep(d, L.ep, kind, L.m, dst, L.k, L.m, seq, dd);
  if (e < 0) {
    L.c[C_LOST]++;
    return false;
  }
  uint32_t b = L.k & 1;
  // one atomic per wave for the lanes sending here together (~1 300 SYNC / SYNC_ACK sends per tick at C3 on one
  // counter would otherwise serialise at its L2 channel, ~90 per µs), on the wave's shard of the buffer's slots:
  // the sending waves of a launch reach this together and would queue on one word (msg_slots.h)
  send_stamp<STAMP>(d, WT_SLOT0);
  uint32_t i = msg_take(d, b);
  send_stamp<STAMP>(d, WT_SLOT1, i);
  if (i >= d.MSGCAP) {
    set_err(d, E_MSGS);
    return true;
  }
  SyncMsg mm;
  mm.src = L.m;
  mm.dst = dst;
  // a delayed one is stored at the end of the tick (k_sync_defer)
  mm.kind = kind | (e > 0 ? KF_DEFER : (res && d.ackres && L.ntl <= TL ? KF_RES : 0u));
  mm.seq = seq;
  mm.cid_iss = ciss;
  mm.cid_cnt = ccnt;
  mm.payload = NEVER;
  mm.psize = L.tsize;
  mm.ncand = 0;
  mm.pad = L.pend;  // chained so that a later row write can redirect the payload to a snapshot (cow)
  // every field but `pin`: pin_msg of another sender may set that one by atomics in this same tick (from another
  // XCD, whose L2 is not this one's), so this sender never stores it. It is NEVER already: the receiver of the
  // slot's previous message reset it after use (P1, member.hip), or the buffer's initialisation did. Without a store to
  // it no release fence is needed (one per send cost an L2 write-back and invalidate: ~14 us per tick at C3).
  SyncMsg* q = &d.msgs[b][i];
  q->src = mm.src, q->dst = mm.dst, q->kind = mm.kind, q->seq = mm.seq, q->cid_iss = mm.cid_iss;
  q->cid_cnt = mm.cid_cnt, q->payload = mm.payload, q->psize = mm.psize, q->ncand = mm.ncand, q->pad = mm.pad;
  q->due = L.k + d.lat + (uint32_t)e;
  q->tln = L.ntl;
  L.pend = i;
  if (e > 0) {  // not linked to the receiver's inbound list before its delivery tick
    if (L.spec) note_wrote(d.halt, L.k);
    return true;
  }
  // the receiver's inbound list for the next tick (sharded handles build it when the exchange commits the list);
  // a receiver with several payloads gets them pinned (pin_msg)
  if (d.W == 1) {
    link_flush(L);
    L.lk_o = atomicExch(&d.m_head[(size_t)b * d.N + dst], i);
    L.lk_i = i;
    send_stamp<STAMP>(d, WT_LINK, L.lk_o);
  }
  return true;
}

// the member's state as member_tick_body holds it (one lane per member; k_inbox_apply: every lane of the member's wave)
__device__ __forceinline__ void ml_init(ML& L, const Dev& d, uint32_t m, uint32_t k, uint4* cw, uint32_t* cw_n, bool spec) {
  L.d = &d;
  L.m = m;
  L.k = k;
  L.N = d.N;
  {  // the body-only state: one 128-B record, five 16-B loads
    const uint4* mp = (const uint4*)(d.ms + m);
    const uint4 w0 = mp[0], w1 = mp[1], w2 = mp[2], w3 = mp[3], w4 = mp[4];
    L.tsize = w0.x, L.fdLen = w0.y, L.gLen = w0.z, L.fdPeriod = w0.w;
    L.gCounter = w1.y, L.cidCnt = w1.z, L.syncSeq = w1.w;  // (w1.x: MS::rsv_period)
    L.evSeq = w2.x, L.initDeadline = w2.y, L.initCidBase = w2.z, L.initN = w2.w;
    L.nsub = w3.x, L.npath = w3.y, L.nfetch = w3.z, L.fnext = w3.w;
    L.pingIdx = (int32_t)w4.x, L.remoteIdx = (int32_t)w4.y, L.evHash = ((uint64_t)w4.w << 32) | w4.z;
  }
  L.nextPing = d.nextPing[m];
  L.nextGossip = d.nextGossip[m];
  L.nextSync = d.nextSync[m];
  L.held = d.held[m];
  L.timerMin = d.timerMin[m];
  L.initFlags = d.initFlags[m];
  L.ep = epoch_at(d, k);
  const size_t li = lidx(d, m);  // per-observer arrays hold only this shard's rows
  L.rk = d.rowk + li * d.NS;
  L.ra = d.rowa + li * d.NS;
  L.rd = row_dirty(d, li);
  L.fdl = d.fdl + li * d.LCAP;
  L.gl = d.gl + li * d.LCAP;
  L.subs = d.subs + li * SUBCAP * 4;
  L.paths = d.paths + li * d.PCAP * 5;
  L.fetch = d.fetch + li * d.FCAP * FREC;
  L.groups = d.groups + li * d.GRCAP * GREC;
  L.fpend = d.fpend + li * KP * 2;
  L.npend = 0;
  for (int i = 0; i < 8; ++i) L.c[i] = 0;
  L.pend = NEVER;
  L.tround = 0;
  L.trk = d.trk + li * TRKL;
  L.ntrk = 0;
  L.trk_on = false;
  L.cw = cw;
  L.cw_n = cw_n;
  L.spec = spec;
  L.ulog = d.ulog + li * d.ULOGC * 2;
  L.ncreq = 0;
  L.nlog = 0;
  L.spq = d.spq + li * SPQ * 8;
  L.nsp = 0;
  L.tl = d.ackres ? d.tlog + ((size_t)(k & 1) * d.NL + li) * TL : nullptr;
  L.ntl = 0;
  L.tlast = NEVER;
  L.rgrp = -1;
  L.pre = NEVER;
  L.lk_i = NEVER;
  L.pmin = L.smin = NEVER;
  L.ev_ok = false;
}

// this tick's write-log length, stamped with the tick (no entry this tick: the stale stamp reads as an empty log)
__device__ __forceinline__ void tl_len_store(const ML& L) {
  if (!L.ntl) return;
  const Dev& d = *L.d;
  const size_t i = (size_t)(L.k & 1) * d.NL + lidx(d, L.m);
  d.tl_n[i] = L.ntl;
  d.tl_tick[i] = L.k;
}

// member_tick_body's state back (everything but next_evt and tround, which only a finished tick stores)
__device__ __forceinline__ void ml_store(ML& L) {
  link_flush(L);
  const Dev& d = *L.d;
  const uint32_t m = L.m;
  {  // the body-only state: five 16-B stores into the member's record
    uint4* mp = (uint4*)(d.ms + m);
    mp[0] = make_uint4(L.tsize, L.fdLen, L.gLen, L.fdPeriod);
    mp[1] = make_uint4(0u, L.gCounter, L.cidCnt, L.syncSeq);
    mp[2] = make_uint4(L.evSeq, L.initDeadline, L.initCidBase, L.initN);
    mp[3] = make_uint4(L.nsub, L.npath, L.nfetch, L.fnext);
    mp[4] = make_uint4((uint32_t)L.pingIdx, (uint32_t)L.remoteIdx, (uint32_t)L.evHash, (uint32_t)(L.evHash >> 32));
  }
  d.nextPing[m] = L.nextPing;
  d.nextGossip[m] = L.nextGossip;
  d.nextSync[m] = L.nextSync;
  d.held[m] = L.held;
  d.timerMin[m] = L.timerMin;
  d.initFlags[m] = L.initFlags;
  tl_len_store(L);
}

// What a parked member keeps between the three launches of a split tick beside ml_store's state: the chain of SYNC
// messages that still carry the live row, the write log's last entry and (with ml_store) its length. Saved by the
// launch that parks it and by k_inbox_apply; loaded, after ml_init, by k_inbox_apply and the resumed launch.
__device__ __forceinline__ void park_load(ML& L) {
  const Dev& d = *L.d;
  const size_t li = lidx(d, L.m);
  L.pend = d.hv_pend[li];
  L.tlast = d.hv_tlast[li];
  if (d.ackres && d.tl_tick[(size_t)(L.k & 1) * d.NL + li] == L.k) L.ntl = d.tl_n[(size_t)(L.k & 1) * d.NL + li];
}
__device__ __forceinline__ void park_store(const ML& L) {
  const size_t li = lidx(*L.d, L.m);
  L.d->hv_pend[li] = L.pend;
  L.d->hv_tlast[li] = L.tlast;
}

// lane 0's member state to every lane of the wave (after a receipt lane 0 ran alone)
__device__ __forceinline__ void ml_bcast(ML& L) {
  L.tsize = __shfl(L.tsize, 0), L.fdLen = __shfl(L.fdLen, 0), L.gLen = __shfl(L.gLen, 0);
  L.cidCnt = __shfl(L.cidCnt, 0), L.evSeq = __shfl(L.evSeq, 0), L.held = __shfl(L.held, 0);
  L.gCounter = __shfl(L.gCounter, 0), L.timerMin = __shfl(L.timerMin, 0), L.nfetch = __shfl(L.nfetch, 0);
  L.fnext = __shfl(L.fnext, 0), L.ntl = __shfl(L.ntl, 0), L.tlast = __shfl(L.tlast, 0), L.nsp = __shfl(L.nsp, 0);
  L.npend = __shfl(L.npend, 0), L.pend = __shfl(L.pend, 0);
  const uint32_t hl = __shfl((uint32_t)L.evHash, 0), hh = __shfl((uint32_t)(L.evHash >> 32), 0);
  L.evHash = ((uint64_t)hh << 32) | hl;
}

}  // namespace swim
