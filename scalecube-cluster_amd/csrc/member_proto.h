// member_proto.h — the protocol handlers of one member over its state (member_state.h), following the reference's
// classes: FailureDetectorImpl (the FD list edits, pings and ping-reqs), MembershipProtocolImpl (updateMembership,
// onFailureDetectorEvent, SYNC merges, doSync), MetadataStoreImpl (fetchMetadata) and the selection half of
// GossipProtocolImpl (spread, doSpreadGossip); and the records of a member's pending requests (ping paths,
// subscriptions, metadata fetches). The phases that call them are in member.hip and inbox.hip.
#pragma once
#include "member_state.h"

namespace swim {

// ---- the records of a member's pending requests ----
// a subscription (Dev::subs, 4 words): a ping (kind 0) or ping-req (kind 1) waiting for its PING_ACK until `deadline`
enum : uint32_t { SUB_CID = 0, SUB_KIND = 1, SUB_TARGET = 2, SUB_DEADLINE = 3 };
__device__ __forceinline__ void sub_copy(uint32_t* D4, const uint32_t* S4) {
  D4[0] = S4[0];
  D4[1] = S4[1];
  D4[2] = S4[2];
  D4[3] = S4[3];
}
// a ping path (Dev::paths, 5 words): the message of request `cid` in flight, its hop or arrival due at `tick`; a is
// the target (direct ping) or the helper (ping-req), b the ping-req's target
enum : uint32_t { PATH_CID = 0, PATH_STAGE = 1, PATH_TICK = 2, PATH_A = 3, PATH_B = 4 };
__device__ __forceinline__ void path_put(uint32_t* Q, uint32_t cnt, uint32_t stage, uint32_t tick, uint32_t a, uint32_t b) {
  Q[0] = cnt;
  Q[1] = stage;
  Q[2] = tick;
  Q[3] = a;
  Q[4] = b;
}
__device__ __forceinline__ void path_copy(uint32_t* Q, const uint32_t* P) {
  for (uint32_t q = 0; q < 5; ++q) Q[q] = P[q];
}
// a metadata fetch (Dev::fetch, FREC = 8 words, moved as two 16-B halves): the words in memory order
struct FetchRec {
  uint32_t cid, subj, inc;
  uint32_t packed;    // status | reason << 8 | added << 16 | stage << 24 (fetch_pack)
  uint32_t group;     // the Mono.whenDelayError group it belongs to (-1: none), or FETCH_ORPHAN
  uint32_t deadline;  // the tick its timeout fires
  uint32_t hop;       // the tick its pending hop (stage 1) or its response's arrival (stage 2) is due
  uint32_t meta;      // the metadata version the response carries (stage 2)
};
// a fetch whose timeout fired while its request was still in flight (a delay): only its hops remain
constexpr uint32_t FETCH_ORPHAN = 0xFFFFFFFEu;
// stage: 1 = response hop pending at the subject, 2 = response in flight, 0 = none (only the timeout remains)
__device__ __forceinline__ uint32_t fetch_pack(uint32_t st, uint32_t reason, uint32_t added, uint32_t stage) {
  return st | (reason << 8) | (added << 16) | (stage << 24);
}
__device__ __forceinline__ uint32_t fetch_stage(const FetchRec& f) { return f.packed >> 24; }
__device__ __forceinline__ void fetch_set_stage(FetchRec& f, uint32_t stage) {
  f.packed = (f.packed & 0x00FFFFFFu) | (stage << 24);
}
__device__ __forceinline__ uint32_t fetch_status(const FetchRec& f) { return f.packed & 0xFF; }
__device__ __forceinline__ uint32_t fetch_reason(const FetchRec& f) { return (f.packed >> 8) & 0xFF; }
__device__ __forceinline__ uint32_t fetch_added(const FetchRec& f) { return (f.packed >> 16) & 0xFF; }
// the next tick the fetch needs its (live) issuer: the hop or arrival while one is pending, and the timeout
__device__ __forceinline__ uint32_t fetch_due(const FetchRec& f) {
  return fetch_stage(f) != 0 ? min(f.deadline, f.hop) : f.deadline;
}
__device__ __forceinline__ FetchRec fetch_ld(const uint32_t* p) {
  const uint4 lo = *(const uint4*)p, hi = *(const uint4*)(p + 4);
  return FetchRec{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}
__device__ __forceinline__ void fetch_st(uint32_t* p, const FetchRec& f) {
  *(uint4*)p = make_uint4(f.cid, f.subj, f.inc, f.packed);
  *(uint4*)(p + 4) = make_uint4(f.group, f.deadline, f.hop, f.meta);
}

// ---- the FD and gossip lists ----
// ArrayList.remove(Object) on one lane: find subj, then shift the tail down by one in blocks of 8 (the loads of a
// block are independent of the stores before it, so they are in flight together instead of one load per element)
__device__ __forceinline__ bool list_remove(uint32_t* a, uint32_t len, uint32_t subj) {
  uint32_t i = 0;
  for (; i + 8 <= len; i += 8) {
    uint32_t v[8];
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t) v[t] = a[i + t];
    bool hit = false;
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t) hit |= v[t] == subj;
    if (hit) break;
  }
  for (; i < len && a[i] != subj; ++i) {
  }
  if (i >= len) return false;
  uint32_t j = i + 1;
  for (; j + 8 <= len; j += 8) {
    uint32_t v[8];
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t) v[t] = a[j + t];
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t) a[j + t - 1] = v[t];
  }
  for (; j < len; ++j) a[j - 1] = a[j];
  return true;
}

// The FD list with its pending inserts applied: one pass over the part of the list at or above the first insert,
// instead of one tail shift per ArrayList.add(index, e). Entry p (ascending final positions f_0 < ... < f_{k-1}) ends
// at f_p; the originals between f_p and f_{p+1} move up by p + 1, segment by segment from the top (8 loads in flight,
// then 8 stores), so no original is overwritten before it is read.
// (not inlined: `inline` gives each translation unit that includes this header its own copy)
__device__ __noinline__ inline void fd_flush(uint32_t* a, const uint32_t* pend, uint32_t k, uint32_t len) {
  for (int p = (int)k - 1; p >= 0; --p) {
    const uint32_t fp = pend[2 * p + 1], fnext = (uint32_t)p + 1 < k ? pend[2 * p + 3] : len;
    const uint32_t s = (uint32_t)p + 1, lo = fp + 1 - s, hi = fnext - s;  // originals [lo, hi) move to [lo + s, hi + s)
    uint32_t j = hi;
    for (; j >= lo + 8; j -= 8) {
      uint32_t v[8];
#pragma unroll
      for (uint32_t t = 0; t < 8; ++t) v[t] = a[j - 8 + t];
#pragma unroll
      for (uint32_t t = 0; t < 8; ++t) a[j - 8 + t + s] = v[t];
    }
    for (; j > lo; --j) a[j - 1 + s] = a[j - 1];
    a[fp] = pend[2 * p];
  }
}
__device__ __forceinline__ void fd_ready(ML& L) {
  if (L.npend) {
    fd_flush(L.fdl, L.fpend, L.npend, L.fdLen);
    L.npend = 0;
  }
}

// ---- membership events ----
__device__ __forceinline__ void on_member_event(ML& L, uint32_t type, uint32_t subj) {
  const Dev& d = *L.d;
  L.pre = NEVER;
  if (type == 1) {  // REMOVED: FailureDetectorImpl.onMemberEvent (:321-325), GossipProtocolImpl (:187-189)
    fd_ready(L);
    if (list_remove(L.fdl, L.fdLen, subj)) L.fdLen--;
    if (list_remove(L.gl, L.gLen, subj)) L.gLen--;
  } else if (type == 0) {  // ADDED: insert at nextInt(size) (:326-331); append (:190-192)
    if (L.fdLen >= d.LCAP || L.gLen >= d.LCAP) {
      set_err(d, E_LIST);
      return;
    }
    const uint32_t idx = L.fdLen > 0 ? next_int(draw(L, S_FD_INSERT), L.fdLen) : 0;
    if (L.npend == KP) fd_ready(L);
    // ArrayList.add(index, e), deferred: the pending inserts at or above idx move up by one, the new one takes idx
    uint32_t j = L.npend;
    for (; j > 0 && L.fpend[2 * j - 1] >= idx; --j) {
      L.fpend[2 * j] = L.fpend[2 * j - 2];
      L.fpend[2 * j + 1] = L.fpend[2 * j - 1] + 1u;
    }
    L.fpend[2 * j] = subj;
    L.fpend[2 * j + 1] = idx;
    L.npend++;
    L.fdLen++;
    L.gl[L.gLen++] = subj;
  }
}

// pad: the gossip counter of a GOSSIP event (its id is (subject, pad)), 0 otherwise. RUMOR mode hashes the events
// as a sum (SEMANTICS.md §9), so slot shards that each emit a member's events for their own gossips add up.
__device__ __forceinline__ void emit_event(ML& L, uint32_t type, uint32_t subj, uint32_t oldm, uint32_t newm,
                                           uint32_t pad = 0) {
  const Dev& d = *L.d;
  uint32_t seq = L.evSeq++;
  if (d.mode == 1u) {  // SWIM_MODE_RUMOR
    L.evHash += hpair(hpair(((uint64_t)L.k << 32) | ((uint64_t)type << 30) | subj, ((uint64_t)oldm << 32) | newm), pad);
  } else {
    L.evHash = hpair(L.evHash, ((uint64_t)L.k << 32) | ((uint64_t)type << 30) | subj);
    L.evHash = hpair(L.evHash, ((uint64_t)oldm << 32) | newm);
  }
  L.c[C_E]++;
  if (d.flags & 1u) {
    uint32_t i = atomicAdd(d.ev_n, 1u);
    if (i < d.EVCAP) {
      uint32_t* e = d.ev + (size_t)i * 8;
      e[0] = L.k;
      e[1] = L.m;
      e[2] = seq;
      e[3] = type;
      e[4] = subj;
      e[5] = oldm;
      e[6] = newm;
      e[7] = pad;
    } else {
      set_err(d, E_EVENTS);
    }
  }
  on_member_event(L, type, subj);
}

// ---- gossips this member creates ----
// the member's queued gossips of this tick get their slots with one atomic on the free stack: a member that re-spreads
// hundreds of SYNC records in one tick (C2) would otherwise wait for one round trip on that hot word per gossip
__device__ __forceinline__ void flush_spreads(ML& L) {
  const uint32_t n = L.nsp;
  if (n == 0) return;
  L.nsp = 0;
  const Dev& d = *L.d;
  if (L.spec) raise_gossip_halt(d.halt, L.k);  // a slot in use: the batch stops after this tick
  const int base = atomicSub(d.free_top, (int)n) - (int)n;
  uint32_t rt = d.rtail[L.m];  // only this lane appends to the member's ring in this kernel
  for (uint32_t i = 0; i < n; ++i) {
    const int pos = base + (int)i;
    if (pos < 0) {
      set_err(d, E_SLOTS);
      continue;
    }
    const uint4 e0 = *(const uint4*)(L.spq + 8 * i), e1 = *(const uint4*)(L.spq + 8 * i + 4);
    slot_init(d, d.free_list[pos], L.m, L.k, ((uint64_t)e0.y << 32) | e0.x, e0.z, ((uint64_t)e1.x << 32) | e0.w, rt++);
    L.c[C_GCREATED]++;
  }
  d.rtail[L.m] = rt;
}

// GossipProtocolImpl.spread -> createAndPutGossip (:124-128,163-169): a membership gossip held by this member; its
// slot is taken at the end of the member's tick (flush_spreads: slot ids are not observable)
__device__ __forceinline__ void spread(ML& L, uint32_t subj, uint32_t st, uint32_t inc) {
  uint64_t gid = ((uint64_t)L.m << 32) | L.gCounter++;
  if (slot_mine(*L.d, gid)) {  // slot sharding: only the owning shard stores it; every shard counts it as held
    if (L.nsp == SPQ) flush_spreads(L);
    const uint64_t key = rec_key(st, inc);
    *(uint4*)(L.spq + 8 * L.nsp) = make_uint4((uint32_t)gid, (uint32_t)(gid >> 32), subj, (uint32_t)key);
    *(uint4*)(L.spq + 8 * L.nsp + 4) = make_uint4((uint32_t)(key >> 32), 0u, 0u, 0u);
    L.nsp++;
  }
  L.held++;
}

// the own record at incarnation + 1 with status st, spread: updateIncarnation (MembershipProtocolImpl.java:178-190,
// ALIVE) and leaveCluster (:197-206: DEAD, the only DEAD record a table keeps)
__device__ __forceinline__ void bump_own(ML& L, uint32_t st) {
  uint64_t v0 = row_ld(L, L.m);
  uint32_t ni = rec_inc(v0) + 1u;
  row_put(L, L.m, (v0 & ~KEY_MASK) | rec_key(st, ni));
  L.c[C_W]++;
  spread(L, L.m, st, ni);
}

// ---- metadata fetches and the groups that wait for them ----
// the metadata version this observer stores for subj (MetadataStoreImpl.membersMetadata), NONE32 if unknown
__device__ __forceinline__ uint32_t known_meta(const ML& L, uint32_t subj, uint64_t v) {
  if (!(v & META_BIT)) return NONE32;
  const Dev& d = *L.d;
  const uint32_t u = d.md_uidx[subj];
  return u == NONE32 ? 0u : d.md_ver[lidx(d, L.m) * MDU + u];
}

__device__ __forceinline__ uint32_t* grp(ML& L, int g) { return L.groups + (size_t)g * GREC; }

__device__ __forceinline__ void complete_group(ML& L, int g) {
  uint32_t* G = grp(L, g);
  uint32_t kind = G[0], flags = G[5];
  G[5] = 0;
  if (kind == 0) {
    // onSync doOnSuccess (MembershipProtocolImpl.java:351-365): SYNC_ACK with the post-merge table
    if (!(flags & GF_ERROR)) send_sync(L, K_SYNC_ACK, G[1], G[2], G[3], g == L.rgrp);
  } else {
    // start0 doFinally (:244-248): schedulePeriodicSync
    L.initFlags &= ~INIT_ACTIVE;
    L.nextSync = L.k + L.d->sync_t;
  }
}

// one inner Mono of Mono.whenDelayError terminated
__device__ __forceinline__ void finish(ML& L, int g, bool error) {
  if (g < 0) return;
  uint32_t* G = grp(L, g);
  if (error) G[5] |= GF_ERROR;
  if ((G[5] & GF_SEALED) && G[4] == 0) complete_group(L, g);
}

__device__ __forceinline__ int alloc_group(ML& L, uint32_t kind, uint32_t reply, uint32_t ciss, uint32_t ccnt) {
  for (int g = 0; g < (int)L.d->GRCAP; ++g) {
    uint32_t* G = grp(L, g);
    if (!(G[5] & GF_USED)) {
      G[0] = kind;
      G[1] = reply;
      G[2] = ciss;
      G[3] = ccnt;
      G[4] = 0;
      G[5] = GF_USED;
      return g;
    }
  }
  set_err(*L.d, E_GROUPS);
  return -1;
}

// doFinally of updateMembership (:526-539)
__device__ __forceinline__ void do_finally(ML& L, uint32_t subj, uint32_t st, uint32_t inc, uint32_t reason) {
  if (reason != R_GOSSIP && reason != R_INITIAL) spread(L, subj, st, inc);
}

// MetadataStoreImpl.fetchMetadata (:149-186); the response hop is evaluated in P3 at k + lat
// dd: whether subj is dead at this tick, when the caller loaded it already (-1: look it up)
__device__ __forceinline__ void fetch_md(ML& L, uint32_t subj, uint32_t st, uint32_t inc, uint32_t reason, uint32_t added, int g,
                                         int dd = -1) {
  const Dev& d = *L.d;
  uint32_t cnt = L.cidCnt++;
  L.c[C_M]++;
  const int e = xmit_ep(d, L.ep, K_GMD_REQ, L.m, subj, L.k, L.m, cnt, dd);
  if (e < 0) {
    L.c[C_LOST]++;
    if (g >= 0) grp(L, g)[5] |= GF_ERROR;
    do_finally(L, subj, st, inc, reason);
    return;
  }
  if (L.nfetch >= d.FCAP) {
    set_err(d, E_FETCH);
    return;
  }
  uint32_t* f = L.fetch + (size_t)(L.nfetch++) * FREC;  // (FetchRec's words, one store each)
  f[0] = cnt;
  f[1] = subj;
  f[2] = inc;
  f[3] = fetch_pack(st, reason, added, 1);  // stage 1: response hop pending
  f[4] = (uint32_t)g;
  f[5] = L.k + d.md_t;
  f[6] = L.k + d.lat + (uint32_t)e;
  f[7] = NONE32;
  L.fnext = min(L.fnext, min(f[5], f[6]));
  if (g >= 0) grp(L, g)[4]++;
}

// ---- MembershipProtocolImpl ----
// MembershipProtocolImpl.updateMembership (:475-541) + emitMembershipEvent (:543-588)
__device__ __forceinline__ void update_membership(ML& L, uint32_t subj, uint32_t s1, uint32_t i1, uint32_t reason, int g) {
  const Dev& d = *L.d;
  uint64_t v0 = row_ld(L, subj);
  uint32_t s0 = rec_status(v0), i0 = rec_inc(v0);
  if (!overrides(s1, i1, s0, i0)) return;
  if (subj == L.m) {  // :488-509 refute with max(inc)+1, keep r0's status, spread, no event
    uint32_t ni = (i0 > i1 ? i0 : i1) + 1u;
    row_put(L, subj, (v0 & ~KEY_MASK) | rec_key(s0, ni));
    L.c[C_W]++;
    spread(L, subj, s0, ni);
    return;
  }
  if (s1 == ST_DEAD) {
    row_put(L, subj, 0);  // row removed; REMOVED below removes the metadata; the timer is cancelled
    L.tsize--;
  } else {
    if (s0 == ST_ABSENT) L.tsize++;
    uint64_t v = (v0 & ~KEY_MASK) | rec_key(s1, i1);
    if (s1 == ST_SUSPECT) {  // scheduleSuspicionTimeoutTask (:597-606): computeIfAbsent
      if (rec_timer(v) == 0) {
        uint32_t dl = L.k + suspicion_ticks(d, L.tsize, mc_ping_t(d, L.m));
        v = rec_with_timer(v, dl);
        if (dl < L.timerMin) L.timerMin = dl;
      }
    } else {
      v = rec_with_timer(v, 0);  // cancelSuspicionTimeoutTask (:590-595)
    }
    row_put(L, subj, v);
  }
  L.c[C_W]++;
  if (s1 == ST_DEAD) {
    uint32_t oldm = known_meta(L, subj, v0);  // metadataStore.removeMetadata
    emit_event(L, 1, subj, oldm, NONE32);
    finish(L, g, false);
    do_finally(L, subj, s1, i1, reason);
    return;
  }
  if (s0 == ST_ABSENT && s1 == ST_ALIVE) {
    fetch_md(L, subj, s1, i1, reason, 1, g);
    return;
  }
  if (s0 != ST_ABSENT && i0 < i1) {
    fetch_md(L, subj, s1, i1, reason, 0, g);
    return;
  }
  finish(L, g, false);
  do_finally(L, subj, s1, i1, reason);
}

// onFailureDetectorEvent (:370-398)
__device__ __forceinline__ void on_fd_event(ML& L, uint32_t target, uint32_t status) {
  uint64_t v0 = row_ld(L, target);
  uint32_t s0 = rec_status(v0);
  if (s0 == ST_ABSENT || s0 == status) return;
  if (status == ST_ALIVE) {
    send_sync(L, K_SYNC, target, NONE32, 0);
  } else {
    L.c[C_R]++;
    update_membership(L, target, ST_SUSPECT, rec_inc(v0), R_FD, -1);
  }
}

// ---- FailureDetectorImpl ----
__device__ __forceinline__ void add_sub(ML& L, uint32_t cnt, uint32_t kind, uint32_t target, uint32_t deadline) {
  if (L.nsub >= SUBCAP) {
    set_err(*L.d, E_SUBS);
    return;
  }
  uint32_t* s = L.subs + (size_t)(L.nsub++) * 4;
  s[0] = cnt;
  s[1] = kind;
  s[2] = target;
  s[3] = deadline;
  L.smin = min(L.smin, deadline);
}
__device__ __forceinline__ void add_path(ML& L, uint32_t cnt, uint32_t stage, uint32_t tick, uint32_t a, uint32_t b) {
  if (L.npath >= L.d->PCAP) {
    set_err(*L.d, E_PATHS);
    return;
  }
  path_put(L.paths + (size_t)(L.npath++) * 5, cnt, stage, tick, a, b);
  L.pmin = min(L.pmin, tick);
}

// doPing error branch (FailureDetectorImpl.java:159-175), selectPingReqMembers (:349-361), doPingReq (:178-213)
__device__ __forceinline__ void ping_req_step(ML& L, uint32_t target, uint32_t cnt) {
  const Dev& d = *L.d;
  uint32_t helpers[8];
  uint32_t nh = 0;
  const uint32_t kreq = mc_kreq(d, L.m);
  if (kreq > 0) {
    fd_ready(L);
    uint32_t pos = L.fdLen;
    for (uint32_t i = 0; i < L.fdLen; ++i)
      if (L.fdl[i] == target) {
        pos = i;
        break;
      }
    uint32_t n = L.fdLen - (pos < L.fdLen ? 1u : 0u);
    if (n > 0) {
      uint32_t kk = kreq < n ? kreq : n;
      uint32_t ovp[16], ovv[16], nov = 0;  // positions touched by the partial Fisher-Yates
      auto get = [&](uint32_t i) -> uint32_t {
        for (uint32_t q = 0; q < nov; ++q)
          if (ovp[q] == i) return ovv[q];
        return L.fdl[i < pos ? i : i + 1];
      };
      auto set = [&](uint32_t i, uint32_t v) {
        for (uint32_t q = 0; q < nov; ++q)
          if (ovp[q] == i) {
            ovv[q] = v;
            return;
          }
        ovp[nov] = i;
        ovv[nov] = v;
        nov++;
      };
      for (uint32_t i = 0; i < kk; ++i) {
        uint32_t j = i + next_int(draw(L, S_PINGREQ), n - i);
        uint32_t vi = get(i), vj = get(j);
        set(i, vj);
        set(j, vi);
      }
      for (uint32_t i = 0; i < kk; ++i) helpers[i] = get(i);
      nh = kk;
    }
  }
  int timeLeft = (int)mc_ping_t(d, L.m) - (int)mc_timeout_t(d, L.m);
  if (timeLeft <= 0 || nh == 0) {
    on_fd_event(L, target, ST_SUSPECT);
    return;
  }
  for (uint32_t q = 0; q < nh; ++q) {
    uint32_t h = helpers[q];
    L.c[C_M]++;
    const int e = xmit_ep(d, L.ep, K_PING_REQ, L.m, h, L.k, L.m, cnt);
    if (e < 0) {
      L.c[C_LOST]++;
      on_fd_event(L, target, ST_SUSPECT);
      continue;
    }
    add_sub(L, cnt, 1, target, L.k + (uint32_t)timeLeft);
    add_path(L, cnt, P_REQ | 1, L.k + d.lat + (uint32_t)e, h, target);
  }
}

// doPing (:128-176) + selectPingMember (:338-347)
__device__ __forceinline__ void do_ping(ML& L) {
  const Dev& d = *L.d;
  L.fdPeriod++;
  if (L.fdLen == 0) return;
  fd_ready(L);
  if (L.pingIdx >= (int32_t)L.fdLen) {
    L.pingIdx = 0;
    shuffle_list(L, L.fdl, L.fdLen, S_FD_SHUFFLE);
  }
  uint32_t target;
  int dd = -1;  // the target's liveness, when loaded with the member state (L.pre)
  if (L.pre != NEVER) {
    target = L.pre;
    dd = L.k >= L.pre_dt ? 1 : 0;
    L.pingIdx++;
  } else {
    target = L.fdl[L.pingIdx++];
  }
  uint32_t cnt = L.cidCnt++;
  L.c[C_M]++;
  const int e = xmit_ep(d, L.ep, K_PING, L.m, target, L.k, L.m, cnt, dd);
  if (e < 0) {
    L.c[C_LOST]++;
    ping_req_step(L, target, cnt);
    return;
  }
  add_sub(L, cnt, 0, target, L.k + mc_timeout_t(d, L.m));
  add_path(L, cnt, P_DIRECT | 1, L.k + d.lat + (uint32_t)e, target, 0);
}

// ---- GossipProtocolImpl, the selection half ----
// doSpreadGossip (GossipProtocolImpl.java:139-157) target selection (:252-273). The sends and the sweep run in
// the gossip data plane (gossip_round.hip on) from T / tspread / tperiod; the round is logged for infectedFrom replay.
__device__ __forceinline__ void do_spread_gossip(ML& L) {
  const Dev& d = *L.d;
  if (L.held == 0) return;
  // period = gPeriod++ (:140): the value before this round's advance (p6_periodic has added gossip_t to nextGossip)
  const uint32_t period = gossip_period(d, L.nextGossip - d.gossip_t, d.firstGossip[L.m]);
  uint32_t F = d.F;
  uint32_t* T = d.T + (size_t)L.m * F;
  uint32_t cnt;
  if (d.implicit) {  // RUMOR at scale: the PRECONVERGED permutation, read where a stored list would be (engine.h)
    const FeistelPerm P = list_perm(d, L.m, 1);
    if (L.gLen < F) {
      for (uint32_t i = 0; i < L.gLen; ++i) T[i] = list_at(P, L.m, i);
      cnt = L.gLen;
    } else {
      if (L.remoteIdx < 0 || (uint32_t)L.remoteIdx + F > L.gLen) {
        set_err(d, E_LIST);  // the reshuffle of a wrapped cursor needs a stored list (N / F rounds: never at C5)
        L.remoteIdx = 0;
      }
      for (uint32_t i = 0; i < F; ++i) T[i] = list_at(P, L.m, L.remoteIdx + i);
      L.remoteIdx += (int32_t)F;
      cnt = F;
    }
  } else if (L.gLen < F) {
    for (uint32_t i = 0; i < L.gLen; ++i) T[i] = L.gl[i];
    cnt = L.gLen;
  } else {
    if (L.remoteIdx < 0 || (uint32_t)L.remoteIdx + F > L.gLen) {
      shuffle_list(L, L.gl, L.gLen, S_GOSSIP_SHUFFLE);
      L.remoteIdx = 0;
    }
    for (uint32_t i = 0; i < F; ++i) T[i] = L.gl[L.remoteIdx + i];
    L.remoteIdx += (int32_t)F;
    cnt = F;
  }
  uint32_t sp = spread_of(d, L.gLen + 1);
  L.tround = 1;
  d.tcnt[L.m] = cnt;
  d.tspread[L.m] = sp;
  d.tperiod[L.m] = period;
  uint32_t pos = d.log_pos[L.m] % d.LOGW;
  size_t lo = (size_t)L.m * d.LOGW + pos;
  if (d.log_pos[L.m] > 0 && d.log_spread[(size_t)L.m * d.LOGW + (d.log_pos[L.m] - 1) % d.LOGW] != sp) d.spchg[L.m] = L.k;
  d.log_tick[lo] = L.k;
  d.log_spread[lo] = sp;
  d.log_cnt[lo] = cnt;
  for (uint32_t i = 0; i < cnt; ++i) d.log_tg[lo * F + i] = T[i];
  d.log_pos[L.m]++;
  if (d.W > 1) {  // the round is replayed into the other shards' replicated logs from exchange A
    uint32_t i = atomicAdd(&d.xn[1], 1u);
    if (i >= d.RRCAP) {
      set_err(d, E_XCAP);
      return;
    }
    uint32_t* r = d.rr_rec + (size_t)i * RRW;
    r[0] = L.m;
    r[1] = cnt;
    r[2] = sp;
    r[3] = period;
    for (uint32_t j = 0; j < cnt; ++j) r[4 + j] = T[j];
  }
}

// ---- SYNC ----
// the member's seedMembers: its own list if it joined through swim_join, else the config's (deduplicated; self is
// skipped by the callers, MembershipProtocolImpl.java:160-166)
__device__ __forceinline__ const uint32_t* member_seeds(const Dev& d, uint32_t m, uint32_t* n) {
  const uint32_t jn = d.jseed_n[m];
  if (jn != NONE32) {
    *n = jn;
    return d.jseeds + (size_t)m * 16;
  }
  *n = d.n_seeds;
  return d.seeds;
}

__device__ __forceinline__ bool is_seed(const Dev& d, uint32_t m, uint32_t s) {
  if (s == m) return false;
  uint32_t n;
  const uint32_t* sd = member_seeds(d, m, &n);
  for (uint32_t i = 0; i < n; ++i)
    if (sd[i] == s) return true;
  return false;
}

// doSync (MembershipProtocolImpl.java:298-314) + selectSyncAddress (:410-421)
__device__ __forceinline__ void do_sync(ML& L) {
  const Dev& d = *L.d;
  uint32_t extra = 0, nsd;
  const uint32_t* sd = member_seeds(d, L.m, &nsd);
  for (uint32_t i = 0; i < nsd; ++i) {
    uint32_t s = sd[i];
    if (s != L.m && row_status(L, s) == ST_ABSENT) extra++;
  }
  uint32_t count = (L.tsize - 1u) + extra;
  if (count == 0) return;
  uint32_t i = next_int(draw(L, S_SYNC_PICK), count);
  uint32_t target;
  if (L.tsize == L.N) {
    target = i < L.m ? i : i + 1u;
  } else {
    target = NONE32;
    for (uint32_t s = 0; s < L.N; ++s) {
      bool in = (s != L.m && row_status(L, s) != ST_ABSENT) || is_seed(d, L.m, s);
      if (!in) continue;
      if (i == 0) {
        target = s;
        break;
      }
      --i;
    }
  }
  send_sync(L, K_SYNC, target, NONE32, 0);
}

// the order a member handles one tick's inbound SYNC / SYNC_ACK messages in: (src, syncSeq)
__device__ __forceinline__ uint64_t sync_order_key(const SyncMsg& mq) { return ((uint64_t)mq.src << 32) | mq.seq; }

// payload record r1 (key32 k1) of subject s against the live row: `.filter(r1 -> !r1.equals(table.get(id)))`, then
// updateMembership (:462-464)
__device__ __forceinline__ void merge_record(ML& L, uint32_t s, uint32_t k1, uint32_t reason, int g) {
  if ((k1 & 3u) == ST_ABSENT || k1 == L.rk[s]) return;
  if (L.d->ackres) tl_add(L, s);
  const uint64_t key = key34(k1);
  update_membership(L, s, rec_status(key), rec_inc(key), reason, g);
}

// syncMembership (:456-467) of one payload. The reference filters every payload record against the live table when
// that payload is processed. k_sync_diff extracted the records that differ from the receiver's row as it stood at
// the start of the tick, in subject order; that is exact for the first payload of the tick. A later payload can
// also hold, for a subject an earlier payload changed, a record equal to the start row but not to the live one (a
// leaver's own DEAD record removes it, then another member's ALIVE record of the old incarnation re-adds it,
// MembershipRecord.java:67-69). Those subjects are read from the payload itself and merged into the candidate walk
// in subject order: up to trk_cap of them from the sorted list L.trk, more from the bitmap Dev::tbm, word by word with the
// next word's load in flight (C2's receivers change hundreds of subjects in one P1: comparing every later payload with
// the whole row on one lane held the member kernel).
__device__ __forceinline__ void merge_payload(ML& L, uint32_t mi, uint32_t reason, int g) {
  const Dev& d = *L.d;
  const uint32_t b = (L.k - 1) & 1;
  const SyncMsg& mm = d.msgs[b][mi];
  L.c[C_R] += mm.psize;
  L.c[C_SYNCMERGE]++;
  const uint32_t nt = L.ntrk;
  const bool bmap = nt > d.trk_cap;  // many subjects changed earlier in this tick: walk the bitmap
  if (bmap) fb_add(d, FB_TRK_WALK);
  if (d.exp & EXP_CYCLES_MAX) {  // timing experiments: full walks, largest candidate count
    if (bmap) atomicAdd(&d.ctr[14], 1ull);
    atomicMax(&d.ctr[15], (unsigned long long)mm.ncand);
  }
  if (mm.ncand == 0 && nt == 0) return;  // steady state: nothing differs, skip the chunk walk
  if (!bmap)
    for (uint32_t i = 1; i < nt; ++i)  // the tracked subjects in ascending order (insertion sort, at most TRK)
      for (uint32_t j = i; j > 0 && L.trk[j - 1] > L.trk[j]; --j) {
        const uint32_t t = L.trk[j];
        L.trk[j] = L.trk[j - 1];
        L.trk[j - 1] = t;
      }
  // One walk with a single merge site: update_membership is large, and each inlined copy of it costs instruction
  // cache in every wave of this kernel. The next record comes from the candidate pool and the tracked subjects merged
  // in subject order (a tracked candidate takes the pool's record).
  uint32_t ti = 0, c = 0, e = 0, n = 0, off = 0;
  bool pool = mm.ncand != 0;
  // the bitmap cursor: word wi - 1 is being consumed (bits left: wcur), word wi is loading (wnxt)
  uint32_t wi = 0;
  unsigned long long wcur = 0, wnxt = 0;
  const unsigned long long* tb = d.tbm + lidx(d, L.m) * d.NW;
  if (bmap && d.NW) {
    wcur = tb[0];
    wnxt = d.NW > 1 ? tb[1] : 0ull;
    wi = 1;
  }
  auto tnext = [&]() -> uint32_t {  // the next tracked subject in ascending order (bitmap mode), NEVER at the end
    while (wcur == 0ull) {
      if (wi >= d.NW) return NEVER;
      wcur = wnxt;
      ++wi;
      wnxt = wi < d.NW ? tb[wi] : 0ull;
    }
    const uint32_t v = (wi - 1u) * 64u + (uint32_t)(__ffsll((long long)wcur) - 1);
    wcur &= wcur - 1ull;
    return v;
  };
  uint32_t tsb = bmap ? tnext() : NEVER;
  for (;;) {
    uint32_t subj, k1;
    {
      while (pool && e == n) {
        if (c == d.NMETA) {
          pool = false;
          break;
        }
        const uint32_t* cm = d.chunk_meta + ((size_t)mi * d.NMETA + c) * 2;
        off = cm[0];
        n = cm[1];
        e = 0;
        ++c;
      }
      uint64_t prec = 0;
      uint32_t ps = NEVER;
      if (pool) {
        prec = d.pool[(size_t)off + e];
        ps = (uint32_t)(prec >> 34);
      }
      const uint32_t ts = bmap ? tsb : ti < nt ? L.trk[ti] : NEVER;
      if (ps == NEVER && ts == NEVER) break;
      if (ts < ps) {
        subj = ts;
        k1 = payload_key_at(d, mm, b, ts);
        if (bmap) tsb = tnext(); else ++ti;
      } else {
        subj = ps;
        k1 = key32(prec & KEY_MASK);
        ++e;
        if (ts == ps) {
          if (bmap) tsb = tnext(); else ++ti;
        }
      }
    }
    merge_record(L, subj, k1, reason, g);
  }
}

}  // namespace swim
