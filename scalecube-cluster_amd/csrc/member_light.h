// member_light.h — the light path of k_member_tick_t<BODY_FULL> (member.hip): the member-ticks of a clean cluster's
// steady state (a ping, its hop, its ack, one or two SYNC / SYNC_ACK receipts, the periodic SYNC send) without the
// general body's code size, registers and whole-state load and store.
//
// member_tick_body reaches each of these cases through phases that load what they need when they get there, often
// behind the lane's own stores. Here the lane loads in rounds of independent loads (round 1: every address that follows
// from m, k and the triage; round 2: what those values name; round 3, only while some member may be dead: the ping
// target's dead_tick), decides in
// registers whether the tick is one of the cases below, and only then commits: until the decision nothing is stored
// and no atomic is issued, so a lane that finds anything else runs member_tick_body from scratch (the fallback and
// the reference: SWIM_NO_LIGHT=1 runs every member through it). What is committed is what the general body would have
// left in memory, word for word: only the words that change are stored.
//
// While no member has ever died, left or been dormant (k < first_dead, one launch-uniform word: engine.h) every dead_tick
// lookup answers "alive": the hop's, the warming loads, round 3 and send_sync's own are skipped, so a ping is two
// rounds and a commit. Once the word stops holding, the path is the one described above.
//
// Who comes here (member_triage, lc): a live member whose only causes this tick are an inbound SYNC list, a due
// request event (next_evt), a due ping, a due periodic SYNC or an empty gossip round; no routed receipts, host
// request, suspicion timer, initial sync or start. Further conditions, checked on the loaded state:
//   FD    nfetch == 0; at most one path, a direct ping's; at most one subscription, a ping's, not timing out now
//         ping: 0 <= pingIdx < fdLen (no reshuffle) and the send succeeds (a failed one starts a ping-req)
//         hop: the target's PING_ACK; a dead target or a lost ack drops the path, as p2_fd
//         ack: the row holds the target as ALIVE or ABSENT (else onFailureDetectorEvent sends a SYNC)
//   P1    one or two messages (two: only while P1 sorts two in registers, Dev::mq_cap), each of this sync group, not
//         delayed, the sender's live row, no candidate: a SYNC (counters and the SYNC_ACK through send_sync) or a
//         SYNC_ACK of a periodic SYNC (counters)
//   SYNC  doSync with a full table (tsize == N: every seed is present, the target follows from the draw by arithmetic)
#pragma once
#include "member_proto.h"

namespace swim {

// what a light attempt did, one bit per counter of swim_debug_light (include/swimhip_debug.h): words SH_LIGHT + i of
// the block's counter row
enum : uint32_t {
  LT_TICKS = 0,    // member-ticks finished by the light path
  LT_FD,           // of them with a ping, a hop or an ack arrival
  LT_P1,           // with a SYNC / SYNC_ACK receipt
  LT_SYNC,         // with the periodic SYNC send
  LT_GENERAL,      // member-ticks run by member_tick_body (fallbacks included)
  LT_FB_RESHUFFLE, // fallbacks: the ping cursor reached the end of the list
  LT_FB_SEND,      // the ping's send failed
  LT_FB_PAYLOADS,  // three inbound payloads or more (two, when the handle sorts fewer in registers: Dev::mq_cap)
  LT_FB_CAND,      // a payload with candidates
  LT_FB_BUSY,      // pending fetches, several paths or subscriptions, a ping-req's
  LT_FB_STATUS,    // an ack for a target the row holds as neither ALIVE nor ABSENT
  LT_FB_OTHER,
  LT_N
};
constexpr uint32_t lt_bit(uint32_t i) { return 1u << i; }
// beside them, the counter of swim_debug_light_sure: word SH_LIGHT_SURE. A light attempt returns it as a bit above
// the LT_ bits
enum : uint32_t {
  LS_SKIP = 0,  // member-ticks finished by the light path without a dead_tick lookup (nobody dead: first_dead)
  LS_N
};
constexpr uint32_t LS_SKIP_BIT = 1u << 16;
static_assert(SH_LIGHT + LT_N == SH_LIGHT_SURE && SH_LIGHT_SURE + LS_N <= CSTRIDE && LT_N <= 16,
              "the light path's words fit its line of the counter row");
constexpr uint32_t LT_FALLBACK = ((1u << LT_N) - 1u) & ~((1u << LT_FB_RESHUFFLE) - 1u);

// the launch takes the light path: never with link delays (a delayed message is stored, redelivered and ordered by
// kernels of their own) or per-link settings (their lookup is a loop over the link table)
__device__ __forceinline__ uint32_t light_mode(const Dev& d) { return d.dly_on || d.link_n ? 0u : d.light; }

// xmit_ep without its side effects (the emulator counter, E_EPOCH), for a send the decision depends on: -2 refused (a
// dead destination: not counted by the emulator), -1 lost, 0 sent. No link delay exists in this mode (light_mode).
__device__ __forceinline__ int light_xmit(const Dev& d, int ep, uint32_t kind, uint32_t src, uint32_t dst, uint32_t k,
                                          uint32_t aux, uint32_t id, bool dst_dead) {
  if (dst_dead) return -2;
  const uint32_t loss = link_set(d, ep, src, dst, k) & 0xFFu;
  const bool lost = loss >= 100 || (loss > 0 && loss_roll(d.seed_lo, d.seed_hi, kind, src, dst, k, aux, id) < loss);
  return lost ? -1 : 0;
}

// an inbound message as the light path holds it: the fields p1_sync, lf_count and the SYNC_ACK read
struct LightMsg {
  uint32_t i, src, kind, seq, ciss, ccnt, pay, psize, ncand, pin, tln;
  __device__ __forceinline__ bool sync() const { return (kind & ~KF_FLAGS) == K_SYNC; }
};
__device__ __forceinline__ void light_msg_load(const Dev& d, uint32_t pb, LightMsg& q) {
  const SyncMsg& s = d.msgs[pb][q.i];
  q.src = s.src, q.kind = s.kind, q.seq = s.seq, q.ciss = s.cid_iss, q.ccnt = s.cid_cnt, q.pay = s.payload;
  q.psize = s.psize, q.ncand = s.ncand, q.pin = s.pin, q.tln = s.tln;
}
// 0 when the light path takes the message: of this sync group, not delayed, the sender's live row, no candidate; a
// SYNC, or the SYNC_ACK of a periodic SYNC. Else the fallback's LT_ bit.
__device__ __forceinline__ uint32_t light_msg_check(const Dev& d, uint32_t m, const LightMsg& q) {
  if ((q.kind & KF_DEFER) || q.pay != NEVER) return lt_bit(LT_FB_OTHER);
  if (q.ncand != 0) return lt_bit(LT_FB_CAND);
  if (!q.sync() && !((q.kind & ~KF_FLAGS) == K_SYNC_ACK && q.ciss == NONE32)) return lt_bit(LT_FB_OTHER);
  if (mc_group(d, q.src) != mc_group(d, m)) return lt_bit(LT_FB_OTHER);
  return 0u;
}

// One member's tick on the light path. head0: the member's inbound list head (the triage's load). Returns the LT_ bits
// of what it did; a fallback bit means nothing was stored and member_tick_body must run. cnt, lfp: as member_tick_body's.
__device__ __forceinline__ uint32_t member_light(const Dev& d, uint32_t m, uint32_t k, uint32_t head0, bool spec,
                                                 uint64_t* lfp, unsigned long long (&cnt)[8]) {
  const size_t li = lidx(d, m);
  MS* const ms = d.ms + m;
  const uint32_t pb = (k - 1) & 1;
  // ---- round 1: the member's record, its schedule, its first path and subscription, the inbound message
  const uint4* mp = (const uint4*)ms;
  const uint4 w0 = mp[0], w1 = mp[1], w3 = mp[3];
  const int32_t pingIdx = ms->pingIdx;
  const uint32_t np = d.nextPing[m], ns = d.nextSync[m], ng = d.nextGossip[m];
  uint32_t* const paths = d.paths + li * d.PCAP * 5;
  uint32_t* const subs = d.subs + li * SUBCAP * 4;
  const uint4 p0 = *(const uint4*)paths;  // cid, stage, tick, a
  const uint4 s0 = *(const uint4*)subs;   // cid, kind, target, deadline
  const bool p1 = head0 != NEVER;
  LightMsg ma, mb;  // the first two messages of the list (mb: loaded in round 2)
  ma.i = head0, mb.i = NEVER;
  if (p1) {
    light_msg_load(d, pb, ma);
    mb.i = d.m_next[(size_t)pb * d.MSGCAP + head0];
  }
  const bool pg = k == np, sy = k == ns;
  uint32_t* const selp = d.sel + (size_t)m * 8 + S_SYNC_PICK;
  const uint32_t selc = sy ? *selp : 0u;
  const uint32_t ping_t = pg ? mc_ping_t(d, m) : 0u, timeout_t = pg ? mc_timeout_t(d, m) : 0u;
  const int ep = epoch_at(d, k);
  const uint32_t fdead = first_dead_at(d);  // (one word, the same for every lane)

  const uint32_t tsize = w0.x, fdLen = w0.y, nsub = w3.x, npath = w3.y, nfetch = w3.z, fnext = w3.w;
  if (ep < 0) return lt_bit(LT_FB_OTHER);
  if (nfetch != 0 || npath > 1 || nsub > 1) return lt_bit(LT_FB_BUSY);
  if (npath == 1 && (p0.y & 0xF0u) != P_DIRECT) return lt_bit(LT_FB_BUSY);
  if (nsub == 1 && s0.y != 0u) return lt_bit(LT_FB_BUSY);
  if (nsub == 1 && s0.w == k) return lt_bit(LT_FB_OTHER);  // the ping's timeout: a ping-req
  const bool due = npath == 1 && p0.z == k;
  const bool hop = due && (p0.y & 0xFu) == 1u, arr = due && (p0.y & 0xFu) == P_ARRIVE;
  if (due && !hop && !arr) return lt_bit(LT_FB_OTHER);
  if (p1) {
    const uint32_t why = light_msg_check(d, m, ma);
    if (why) return why;
  }
  if (sy && (tsize != d.N || d.N < 2)) return lt_bit(LT_FB_OTHER);
  if (pg) {
    if (fdLen == 0 || pingIdx < 0) return lt_bit(LT_FB_OTHER);
    if (pingIdx >= (int32_t)fdLen) return lt_bit(LT_FB_RESHUFFLE);
  }

  // Nobody is dead at k while k < first_dead (engine.h): every "is x dead at k" below is answered without its load.
  const bool alive_all = k < fdead;
  const int dd = alive_all ? 0 : -1;  // xmit_ep's: the destination is known alive, or looked up

  // ---- round 2: what those values name (while some member may be dead, the two sends' destinations are only warmed
  // below: send_sync loads them; with alive_all it is told they are alive and loads nothing)
  const bool hit = arr && nsub == 1 && s0.x == p0.x;  // the pending subscription takes the PING_ACK
  const uint32_t tgt = pg ? d.fdl[li * d.LCAP + (uint32_t)pingIdx] : 0u;
  const uint32_t hop_dt = hop && !alive_all ? d.dead_tick[p0.w] : NEVER;
  const uint32_t ack_st = hit ? d.rowk[li * d.NS + s0.z] & 3u : ST_ALIVE;
  uint32_t starget = 0;
  if (sy) {
    const uint32_t i = next_int(philox(m, S_SYNC_PICK, selc, 0, d.seed_lo ^ SALT_SEL, d.seed_hi).x, d.N - 1u);
    starget = i < m ? i : i + 1u;
  }
  const bool two = mb.i != NEVER;  // a second payload, and no third
  if (two) {
    // (a handle whose P1 sorts fewer than two messages in registers takes its list-walk path and counts FB_MQ)
    if (d.mq_cap < 2u) return lt_bit(LT_FB_PAYLOADS);
    light_msg_load(d, pb, mb);
    if (d.m_next[(size_t)pb * d.MSGCAP + mb.i] != NEVER) return lt_bit(LT_FB_PAYLOADS);
  }
  uint32_t tgt_dt = NEVER;
  if (!alive_all) {
    uint32_t warm = 0;
    if (p1 && ma.sync()) warm += d.dead_tick[ma.src];
    if (sy) warm += d.dead_tick[starget];
    asm volatile("" ::"v"(warm));  // keep the warming loads
    // ---- round 3
    if (pg) tgt_dt = d.dead_tick[tgt];
  }

  if (two) {
    const uint32_t why = light_msg_check(d, m, mb);
    if (why) return why;
  }
  if (hit && ack_st != ST_ALIVE && ack_st != ST_ABSENT) return lt_bit(LT_FB_STATUS);
  const uint32_t cid = w1.z;
  if (pg && light_xmit(d, ep, K_PING, m, tgt, k, m, cid, k >= tgt_dt) < 0) return lt_bit(LT_FB_SEND);

  // ---- commit: the general body's phases in their order, on the words they change
  uint32_t did = lt_bit(LT_TICKS) | (alive_all ? LS_SKIP_BIT : 0u);
  ML L;  // the fields send_sync and link_flush read
  L.d = &d, L.m = m, L.k = k, L.ep = ep, L.tsize = tsize, L.syncSeq = w1.w, L.pend = NEVER, L.ntl = 0, L.spec = spec;
  L.lk_i = NEVER, L.lk_o = NEVER;
  for (int i = 0; i < 8; ++i) L.c[i] = 0;
  if (p1) {  // p1_sync with nothing to merge: the messages in (src, syncSeq) order
    did |= lt_bit(LT_P1);
    if (lfp) *lfp += lf_count(ma.kind, ma.pin, ma.tln) + (two ? lf_count(mb.kind, mb.pin, mb.tln) : 0ull);
    d.m_head[(size_t)pb * d.N + m] = NEVER;
    if (two) {  // several payloads were pinned: the pins back to NEVER for the slots' next use
      d.msgs[pb][ma.i].pin = NEVER;
      d.msgs[pb][mb.i].pin = NEVER;
    }
    const bool swap = two && (((uint64_t)mb.src << 32) | mb.seq) < (((uint64_t)ma.src << 32) | ma.seq);
    for (uint32_t r = 0; r < (two ? 2u : 1u); ++r) {
      const LightMsg& q = (r == 0) == swap ? mb : ma;
      L.c[C_R] += q.psize;
      L.c[C_SYNCMERGE]++;
      if (q.sync()) send_sync<true>(L, K_SYNC_ACK, q.src, q.ciss, q.ccnt, !(q.kind & (KF_ABS | KF_LATE)), dd);
    }
  }
  uint32_t nsub2 = nsub, npath2 = npath, pmin = NEVER, smin = NEVER;
  if (hop) {  // p2_fd: onPing at the target
    did |= lt_bit(LT_FD);
    if (k >= hop_dt) {
      npath2 = 0;
    } else {
      L.c[C_M]++;
      const int e = light_xmit(d, ep, K_PING_ACK, p0.w, m, k, m, p0.x, false);
      em_count(d, p0.w, 1u, e < 0 ? 1u : 0u);
      if (e < 0) {
        L.c[C_LOST]++;
        npath2 = 0;
      } else {
        pmin = k + d.lat;
        paths[PATH_STAGE] = P_DIRECT | P_ARRIVE;
        paths[PATH_TICK] = pmin;
      }
    }
  } else if (arr) {  // the PING_ACK: the subscription resolves (publishPingResult(ALIVE) finds nothing to do)
    did |= lt_bit(LT_FD);
    npath2 = 0;
    if (hit) nsub2 = 0;
  } else if (npath == 1) {
    pmin = p0.z;
  }
  if (nsub2 == 1) smin = s0.w;
  if (pg) {  // p6_periodic: do_ping
    did |= lt_bit(LT_FD);
    L.c[C_M]++;
    em_count(d, m, 1u, 0u);
    const uint32_t dl = k + timeout_t, hopt = k + d.lat;
    *(uint4*)(subs + (size_t)nsub2 * 4) = make_uint4(cid, 0u, tgt, dl);
    path_put(paths + (size_t)npath2 * 5, cid, P_DIRECT | 1u, hopt, tgt, 0u);
    nsub2++, npath2++;
    smin = min(smin, dl), pmin = min(pmin, hopt);
    d.nextPing[m] = np + ping_t;
    ms->fdPeriod = w0.w + 1u;
    ms->cidCnt = cid + 1u;
    ms->pingIdx = pingIdx + 1;
  }
  if (k == ng) d.nextGossip[m] = ng + d.gossip_t;  // an empty round (the triage: held == 0)
  if (sy) {  // do_sync
    did |= lt_bit(LT_SYNC);
    d.nextSync[m] = ns + d.sync_t;
    *selp = selc + 1u;
    send_sync<true>(L, K_SYNC, starget, NONE32, 0, false, dd);
  }
  link_flush(L);
  if (L.syncSeq != w1.w) ms->syncSeq = L.syncSeq;
  if (nsub2 != nsub) ms->nsub = nsub2;
  if (npath2 != npath) ms->npath = npath2;
  d.next_evt[m] = min(fnext, min(pmin, smin));
  d.tround[m] = 0;
  for (int i = 0; i < 8; ++i) cnt[i] += L.c[i];
  return did;
}

// the wave's LT_ bits into the block's counter row: one ballot per counter, an atomic for those that fired
__device__ __forceinline__ void light_count(const Dev& d, uint32_t bits, uint32_t lane) {
  if (!__ballot(bits != 0u)) return;
  unsigned long long* cs = d.ctr_sh + (size_t)(blockIdx.x % CSH) * CSTRIDE + SH_LIGHT;
#pragma unroll
  for (uint32_t i = 0; i < LT_N; ++i) {
    const uint32_t v = (uint32_t)__popcll(__ballot((bits >> i) & 1u));
    if (lane == 0 && v) atomicAdd(&cs[i], (unsigned long long)v);
  }
  const uint32_t skip = (uint32_t)__popcll(__ballot(bits & LS_SKIP_BIT));
  if (lane == 0 && skip) atomicAdd(&cs[SH_LIGHT_SURE - SH_LIGHT + LS_SKIP], (unsigned long long)skip);
}

// the general body's member-ticks of a wave (LT_GENERAL)
__device__ __forceinline__ void light_count_general(const Dev& d, bool ran, uint32_t lane) {
  const uint32_t v = (uint32_t)__popcll(__ballot(ran));
  if (lane == 0 && v)
    atomicAdd(&d.ctr_sh[(size_t)(blockIdx.x % CSH) * CSTRIDE + SH_LIGHT + LT_GENERAL], (unsigned long long)v);
}

}  // namespace swim
