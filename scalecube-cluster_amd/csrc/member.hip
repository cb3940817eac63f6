// member.hip — k_member_tick: one thread per simulated member runs phases P0..P6 of SEMANTICS.md §4.
//
// This kernel is the control plane of the protocol stack of every member: FailureDetectorImpl, MembershipProtocolImpl,
// MetadataStoreImpl and the selection half of GossipProtocolImpl. Its work per member per tick is O(1) in the
// common case. The O(N) work runs elsewhere: the SYNC-payload diff (k_sync_diff) and the gossip data plane
// (gossip_*.hip). Remote hops of stateless request handlers (onPing, onPingReq, onTransitPingAck,
// onMetadataRequest) are evaluated at the issuer, at the hop's own tick and against that tick's network
// settings. The payload they would carry is only the correlation id, so no message is materialised.
//
// Here: the triage, one function per phase, member_tick_body (the tick of one member, a page that reads like
// SEMANTICS.md §4) and the kernel. The member's state is in member_state.h, the handlers the phases call in
// member_proto.h, P4 of a parked member on a wave of its own in inbox.hip.
#include "member_kernels.h"
#include "member_light.h"
#include "member_proto.h"

namespace swim {

// Triage (k_member_triage): the idle fast path. Most members have nothing due in most ticks (a ping every 10 ticks,
// a SYNC every 300); they only advance an empty gossip round here. Returns whether the member needs the full
// control path of k_member_tick this tick, and its work class: 1 = a ping and / or a periodic SYNC is due (P6) and
// nothing else, 2 = only request-state events (ping hops, ack arrivals, timeouts), 3 = both, 0 = anything else (SYNC
// receipt, gossip receipts or round, timers, host requests, start).
// nolist: no lister ran for this tick (MT_NOLIST); lfc: what it would have counted for the payloads dropped here
// light (member_light.h light_mode; 0: the classes above): a member whose causes the light path knows (an inbound SYNC
// list, a request event, a ping, the periodic SYNC, an empty gossip round) gets class 1 (a list), 3 (a
// ping or a SYNC due) or 2, everything that needs the general body class 0; head: its inbound list head, for that path
// tw: the member's triage words (triage_load)
struct TriageWords {
  uint32_t mh, rc, pi, ne, tm, np, ns, inf, ng, held, dt, st, nd;
};
// every word is loaded up front (no short-circuit chain of dependent loads); the SoA loads coalesce per wave
// (BODY_SPLIT: through Dev, as before the split from member_triage)
__device__ __forceinline__ TriageWords triage_load(const Dev& d, uint32_t m, uint32_t k) {
  return TriageWords{d.m_head[(size_t)((k - 1) & 1) * d.N + m], d.rc_cnt[m], d.pending_inc[m], d.next_evt[m], d.timerMin[m],
                     d.nextPing[m], d.nextSync[m], d.initFlags[m], d.nextGossip[m], d.held[m], d.dead_tick[m],
                     d.start_tick[m], d.rc_ndrop[m]};
}
// the same from the launch's argument (member_kernels.h MemberFront): no load of a pointer in front of the loads
__device__ __forceinline__ TriageWords triage_load(const MemberFront& f, uint32_t m, uint32_t k) {
  return TriageWords{f.m_head[(size_t)((k - 1) & 1) * f.N + m], f.rc_cnt[m], f.pending_inc[m], f.next_evt[m], f.timerMin[m],
                     f.nextPing[m], f.nextSync[m], f.initFlags[m], f.nextGossip[m], f.held[m], f.dead_tick[m],
                     f.start_tick[m], f.rc_ndrop[m]};
}
// the triage's loads and the halt words' (spec.h halt_load) are issued here and have arrived behind this point: the
// launch's halt decision and the triage then wait once, for both
__device__ __forceinline__ void triage_arrived(const TriageWords& t, const HaltWords& h) {
  asm volatile("" ::"v"(t.mh), "v"(t.rc), "v"(t.pi), "v"(t.ne), "v"(t.tm), "v"(t.np), "v"(t.ns), "v"(t.inf), "v"(t.ng),
               "v"(t.held), "v"(t.dt), "v"(t.st), "v"(t.nd), "v"(h.hg), "v"(h.hd), "v"(h.listed), "v"(h.hw));
}
__device__ __forceinline__ bool member_triage(const Dev& d, uint32_t m, uint32_t k, uint32_t& cls, uint32_t& drops,
                                              uint32_t& evs, bool nolist, uint64_t& lfc, uint32_t light, uint32_t& head,
                                              const TriageWords& tw) {
  // A dead member does nothing itself, but the remote hops of its in-flight requests still run at the live
  // responders (their sends fail against the dead issuer), so those hops are still evaluated for the counters.
  const uint32_t mh = tw.mh, rc = tw.rc, pi = tw.pi, ne = tw.ne, tm = tw.tm, np = tw.np, ns = tw.ns, inf = tw.inf, ng = tw.ng,
                 held = tw.held, dt = tw.dt, st = tw.st, nd = tw.nd;
  const bool dead = k >= dt;
  cls = 0;
  drops = 0;
  if (d.fastp4) {  // RUMOR mode: P4's GOSSIP events of this tick, hashed and counted when they were applied
    const uint32_t pn = d.evp_n[m];
    if (pn) {
      if (!dead) {  // a member crashed since holds no P4 (its receipts are dropped, as rc_cnt below)
        d.ms[m].evHash += d.evp_hash[m];
        d.ms[m].evSeq += pn;
        evs = pn;
      }
      d.evp_hash[m] = 0;
      d.evp_n[m] = 0;
    }
  }
  if (nd) {  // receipts that could not change the row: P4's record compares (none for a dead member)
    d.rc_ndrop[m] = 0;
    if (!dead) drops = nd;
  }
  if (dead) {
    d.rc_cnt[m] = 0;
    d.rc_fill[m] = 0;
    if (k > 0 && mh != NEVER) {  // dropped payloads: their pins go back to NEVER (send_sync)
      const uint32_t pb = (k - 1) & 1;
      for (uint32_t q = mh; q != NEVER; q = d.m_next[(size_t)pb * d.MSGCAP + q]) {
        SyncMsg& sm = d.msgs[pb][q];
        if (nolist) lfc += lf_count(sm.kind, sm.pin, sm.tln);
        sm.pin = NEVER;
      }
      d.m_head[(size_t)pb * d.N + m] = NEVER;
    }
  } else {
    const bool busy = (k > 0 && mh != NEVER) | (rc != 0) | (pi != 0) | (ne <= k) | (tm <= k) | (k == np) | (k == ns) |
                      ((inf & INIT_ACTIVE) != 0) | (k == st);
    // a periodic SYNC send (doSync, P6) is scheduled with the pings (P6 too), not with the SYNC receivers: in one wave
    // their chains would run one after the other
    const bool other = (k > 0 && mh != NEVER) | (rc != 0) | (pi != 0) | (tm <= k) | ((inf & INIT_ACTIVE) != 0) |
                       (k == st) | (k == ng && held != 0);
    cls = other ? 0u : (k == np || k == ns ? 1u : 0u) | (ne <= k ? 2u : 0u);
    if (light) {
      const bool list = k > 0 && mh != NEVER;
      const bool general = (rc != 0) | (pi != 0) | (tm <= k) | ((inf & INIT_ACTIVE) != 0) | (k == st) |
                           (k == ng && held != 0);
      cls = general ? 0u : list ? 1u : (k == np || k == ns) ? 3u : 2u;
      head = list ? mh : NEVER;
    }
    if (!busy) {
      if (k != ng) {
        d.tround[m] = 0;
        return false;
      }
      // doSpreadGossip with no gossips: period++ only (GossipProtocolImpl.java:141-146); the period is derived from
      // nextGossip (gossip_period), so the member's record is not touched
      if (held == 0) {
        d.nextGossip[m] = ng + d.gossip_t;
        d.tround[m] = 0;
        return false;
      }
    }
  }
  if (dead && d.ms[m].npath == 0 && (d.ms[m].nfetch == 0 || d.ms[m].fnext > k)) {
    d.tround[m] = 0;
    return false;
  }
  return true;
}

// The timing experiments' lap clock of one member's body, called after each phase group (slots 0-4) and inside P1 and
// P2 (slots 5-11).
// SWIM_EXP & 16 (timing experiment): shader cycles per phase summed over members, ctr[8..12]
// SWIM_EXP & 128: the largest per-member cycles of each phase instead (which phase makes the longest lane)
// SWIM_EXP & 512: the wave's first busy lane stamps the wall clock after each phase group (wt[4 + slot])
// (the first lane active at the lap stamps it: a lap inside a branch times the lanes that took it)
struct Lap {
  const Dev& d;
  const bool prof;
  unsigned long long tp;
  __device__ __forceinline__ explicit Lap(const Dev& dev)
      : d(dev), prof((dev.exp & EXP_CYCLES) != 0), tp(prof ? clock64() : 0) {}
  __device__ __forceinline__ void operator()(int slot) {
    if ((d.exp & EXP_WAVE_CLOCK) && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)__ballot(1)) - 1))
      d.wt[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * WT_WORDS + 4 + slot] = wall_clock64();
    if (!prof || slot > 4) return;  // (slots 5-10: finer wall-clock laps only)
    const unsigned long long t = clock64();
    if (d.exp & EXP_CYCLES_SUM)
      atomicAdd(&d.ctr[8 + slot], t - tp);
    else
      atomicMax(&d.ctr[8 + slot], t - tp);
    tp = t;
  }
};

// ---- P0 host requests: updateIncarnation (MembershipProtocolImpl.java:178-190), then leaveCluster (:197-206) ----
__device__ __forceinline__ void p0_host_requests(ML& L, bool dead) {
  const Dev& d = *L.d;
  const uint32_t m = L.m;
  const uint32_t preq = dead ? 0u : d.pending_inc[m];
  if (preq) {
    d.pending_inc[m] = 0;
    // one bump and one gossip per swim_update_incarnation call
    for (uint32_t b = preq >> 2; b > 0; --b) bump_own(L, ST_ALIVE);
    // the own record becomes DEAD inc+1 (the only DEAD record a table keeps) and is spread
    if (preq & 2u) bump_own(L, ST_DEAD);
  }
}

// ---- P0 start: ClusterImpl.join0 -> MembershipProtocolImpl.start0 (:216-251): COLD_JOIN members at tick 0, joined
// (swim_join) members at their join tick, with their own seeds ----
__device__ __forceinline__ void p0_start(ML& L, bool dead) {
  const Dev& d = *L.d;
  const uint32_t m = L.m, k = L.k;
  if (!dead && k == d.start_tick[m]) {
    uint32_t nsd;
    const uint32_t* sd = member_seeds(d, m, &nsd);
    uint32_t ns = 0;
    for (uint32_t i = 0; i < nsd; ++i)
      if (sd[i] != m) ns++;
    if (ns == 0) {
      L.nextSync = k + d.sync_t;
    } else {
      L.initFlags = INIT_ACTIVE;
      L.initDeadline = k + d.syncTimeout_t;
      L.initCidBase = L.cidCnt;
      L.initN = ns;
      uint32_t failed = 0;
      for (uint32_t i = 0; i < nsd; ++i) {
        if (sd[i] == m) continue;
        uint32_t cnt = L.cidCnt++;
        if (!send_sync(L, K_SYNC, sd[i], m, cnt)) failed++;
      }
      if (failed == ns) {
        L.initFlags = 0;
        L.nextSync = k + d.sync_t;
      }
    }
  }
}

// ---- P1 SYNC / SYNC_ACK (onMessage :320-331, onSync :346-367, onSyncAck :337-343) ----
// the senders linked this member's inbound messages into a list (head0: its head, loaded with the member's state);
// they are handled in (src, syncSeq) order
// lfp: no lister ran for this tick (MT_NOLIST): where this lane adds what the lister would have counted for its
// messages (lf_count; LDS); null otherwise
__device__ __forceinline__ void p1_sync(ML& L, uint32_t head0, Lap& lap, uint64_t* lfp) {
  const Dev& d = *L.d;
  const uint32_t m = L.m, k = L.k;
  const uint32_t* mnext = d.m_next + (size_t)((k - 1) & 1) * d.MSGCAP;
  if (head0 != NEVER) {
    const uint32_t pb = (k - 1) & 1;
    const uint32_t head = head0;
    uint64_t key[MQ];
    uint32_t idx[MQ], n = 0;
    bool more = false;
    uint64_t lfc = 0;
    for (uint32_t q = head; q != NEVER; q = mnext[q]) {
      if (n == d.mq_cap) {
        more = true;
        fb_add(d, FB_MQ);
        if (lfp)  // (the rest of the list, counted only)
          for (uint32_t r = q; r != NEVER; r = mnext[r]) lfc += lf_count(d.msgs[pb][r].kind, d.msgs[pb][r].pin, d.msgs[pb][r].tln);
        break;
      }
      const SyncMsg& sq = d.msgs[pb][q];
      uint64_t kq = sync_order_key(sq);
      // no lister ran: the message counted as it would have (fields of the entry the key comes from: no further trip)
      if (lfp) lfc += lf_count(sq.kind, sq.pin, sq.tln);
      uint32_t j = n++;
      while (j > 0 && key[j - 1] > kq) {
        key[j] = key[j - 1];
        idx[j] = idx[j - 1];
        --j;
      }
      key[j] = kq;
      idx[j] = q;
    }
    // (reset after the walk's loads: on gfx950 a load issued after this lane's store waits for the store)
    d.m_head[(size_t)pb * d.N + m] = NEVER;
    // no lister ran: its decision on a pinned payload, here (a read of the pinned copy raises E_PIN, payload_key_at)
    const bool unpinned = lfp != nullptr;
    if (unpinned && more) {  // (a list past mq_cap: by a walk)
      for (uint32_t q = head; q != NEVER; q = mnext[q]) d.msgs[pb][q].pin = NEVER;
    } else if (unpinned && n > 1) {
      for (uint32_t r = 0; r < n; ++r) d.msgs[pb][idx[r]].pin = NEVER;
    }
    if (lfp) *lfp += lfc;
    lap(5);
    uint64_t last = 0;
    L.trk_on = n > 1 || more;  // several payloads: later ones re-check the subjects earlier ones changed
    for (uint32_t r = 0;; ++r) {
      uint32_t mi;
      if (!more) {
        if (r == n) break;
        mi = idx[r];
      } else {  // rare: more than MQ messages in one tick (a seed during a cold join): select the next key
        uint64_t best = ~0ull;
        mi = NEVER;
        for (uint32_t q = head; q != NEVER; q = mnext[q]) {
          uint64_t kq = sync_order_key(d.msgs[pb][q]);
          if ((r == 0 || kq > last) && kq < best) {
            best = kq;
            mi = q;
          }
        }
        if (mi == NEVER) break;
        last = best;
      }
      SyncMsg mm = d.msgs[pb][mi];
      const uint32_t mflags = mm.kind & KF_FLAGS;
      mm.kind &= ~KF_FLAGS;
      if (mc_group(d, mm.src) != mc_group(d, m)) continue;  // checkSyncGroup (:320-321,431-437): another group's data
      if (mm.kind == K_SYNC && mm.ncand == 0 && L.ntrk == 0 && L.nfetch == 0) {
        // onSync with nothing to merge (the steady state): merge_payload finds no record, and with no fetch pending
        // every group is free, so the group alloc_group would take completes at once; its SYNC_ACK goes out without
        // the group table's round trips (a free group's fields are never read before alloc_group rewrites them)
        L.c[C_R] += mm.psize;
        L.c[C_SYNCMERGE]++;
        send_sync(L, K_SYNC_ACK, mm.src, mm.cid_iss, mm.cid_cnt, !(mflags & (KF_ABS | KF_LATE)));
        continue;
      }
      // one merge_payload / finish site for the three cases (each inlined copy is large)
      int g = -1;
      uint32_t reason = R_SYNC;
      bool grouped = false;
      if (mm.kind == K_SYNC) {
        g = alloc_group(L, 0, mm.src, mm.cid_iss, mm.cid_cnt);
        grouped = true;
      } else if (mm.cid_iss == NONE32) {
      } else if (mm.cid_iss == m && (L.initFlags & INIT_ACTIVE) && !(L.initFlags & INIT_RECEIVED) &&
                 mm.cid_cnt >= L.initCidBase && mm.cid_cnt < L.initCidBase + L.initN) {
        L.initFlags |= INIT_RECEIVED;  // mergeDelayError(...).take(1) (:239-243)
        g = alloc_group(L, 1, NONE32, NONE32, 0);
        reason = R_INITIAL;
        grouped = true;
      } else {
        continue;  // a SYNC_ACK of another initial sync or of an expired one (:326-328)
      }
      merge_payload(L, mi, reason, g);
      if (grouped && g >= 0) {
        grp(L, g)[5] |= GF_SEALED;
        // its SYNC_ACK, if sent now, may be resolved unless the payload lacked records this row holds or came late
        L.rgrp = (mm.kind == K_SYNC && !(mflags & (KF_ABS | KF_LATE))) ? g : -1;
        finish(L, g, false);
        lap(8);
        L.rgrp = -1;
      }
    }
    L.trk_on = false;
    if (L.ntrk) {  // the written-subject bitmap back to zero: the listed subjects' words, or the whole row
      unsigned long long* tb = d.tbm + lidx(d, m) * d.NW;
      if (L.ntrk <= TRKL)
        for (uint32_t q = 0; q < L.ntrk; ++q) tb[L.trk[q] >> 6] = 0ull;
      else
        for (uint32_t q = 0; q < d.NW; ++q) tb[q] = 0ull;
      L.ntrk = 0;
    }
    if ((n > 1 || more) && !unpinned)  // the pins of this tick's payloads go back to NEVER for the slots' next use (send_sync)
      for (uint32_t q = head; q != NEVER; q = mnext[q]) d.msgs[pb][q].pin = NEVER;
  }
}

// ---- P2 FD: remote hops of pending pings, then PING_ACK arrivals in cid order ----
__device__ __forceinline__ void p2_fd(ML& L, bool dead, Lap& lap) {
  const Dev& d = *L.d;
  const uint32_t m = L.m, k = L.k;
  if (L.npath) {
    // arrivals stay in the compacted list this pass, marked by their new index (at most PATHCAP_DELAY = 32 entries)
    uint32_t arrmask = 0;
    uint32_t w = 0, pm = NEVER;
    for (uint32_t p = 0; p < L.npath; ++p) {
      uint32_t* P = L.paths + (size_t)p * 5;
      uint32_t cnt = P[PATH_CID], stage = P[PATH_STAGE], tk = P[PATH_TICK], a = P[PATH_A], b = P[PATH_B];
      bool keep = true, arr = false;
      if (tk == k) {
        lap(9);
        uint32_t kind = stage & 0xF0, st = stage & 0xF;
        if (st == P_ARRIVE) {
          if (dead) keep = false;
          else arrmask |= 1u << w, arr = true;
        } else if (kind == P_DIRECT) {  // onPing at the target (:230-255): PING_ACK back to the issuer
          if (dead_at(d, a, k)) {
            keep = false;
          } else {
            L.c[C_M]++;
            const int e = xmit_ep(d, L.ep, K_PING_ACK, a, m, k, m, cnt);
            if (e < 0) {
              L.c[C_LOST]++;
              keep = false;
            } else {
              stage = P_DIRECT | P_ARRIVE;
              tk = k + d.lat + (uint32_t)e;
            }
          }
        } else {  // ping-req chain: helper a, target b
          uint32_t who = st == 2 ? b : a;
          if (dead_at(d, who, k)) {
            keep = false;
          } else {
            L.c[C_M]++;
            int e;
            if (st == 1)  // onPingReq (:258-284): transit PING helper -> target
              e = xmit_ep(d, L.ep, K_PING, a, b, k, m, cnt);
            else if (st == 2)  // onPing at the target: PING_ACK target -> helper
              e = xmit_ep(d, L.ep, K_PING_ACK, b, a, k, m, cnt);
            else  // onTransitPingAck (:290-315): PING_ACK helper -> issuer
              e = xmit_ep(d, L.ep, K_PING_ACK, a, m, k, m, cnt);
            if (e < 0) {
              L.c[C_LOST]++;
              keep = false;
            } else {
              stage = P_REQ | (st == 3 ? P_ARRIVE : st + 1);
              tk = k + d.lat + (uint32_t)e;
            }
          }
        }
        lap(10);
      }
      if (keep) {
        path_put(L.paths + (size_t)w * 5, cnt, stage, tk, a, b);
        w++;
        if (!arr) pm = min(pm, tk);  // (an arrival leaves the list below)
      }
    }
    L.npath = w;
    L.pmin = min(L.pmin, pm);
    lap(6);
    // arrivals: every pending subscription on the cid takes the first PING_ACK (TransportImpl.java:205-232), in cid
    // order; then the arrived entries leave the list
    const uint32_t narr = __popc(arrmask);
    for (uint32_t done = 0, last = 0; done < narr;) {
      uint32_t cnt = NEVER;  // the smallest arrived cid above the last one handled
      for (uint32_t q = 0; q < w; ++q) {
        const uint32_t c = L.paths[(size_t)q * 5 + PATH_CID];
        if (((arrmask >> q) & 1u) && (done == 0 || c > last) && c < cnt) cnt = c;
      }
      for (uint32_t q = 0; q < w; ++q) done += ((arrmask >> q) & 1u) && L.paths[(size_t)q * 5 + PATH_CID] == cnt;
      last = cnt;
      uint32_t hit[SUBCAP], nh = 0, w2 = 0;
      for (uint32_t s = 0; s < L.nsub; ++s) {
        uint32_t* S4 = L.subs + (size_t)s * 4;
        if (S4[SUB_CID] == cnt) {
          hit[nh++] = S4[SUB_TARGET];
        } else {
          sub_copy(L.subs + (size_t)w2 * 4, S4);
          w2++;
        }
      }
      L.nsub = w2;
      lap(11);
      for (uint32_t q = 0; q < nh; ++q) on_fd_event(L, hit[q], ST_ALIVE);  // publishPingResult(ALIVE)
    }
    lap(7);
    if (arrmask) {
      uint32_t w3 = 0;
      for (uint32_t p = 0; p < w; ++p)
        if (!((arrmask >> p) & 1u)) {
          if (w3 != p) path_copy(L.paths + (size_t)w3 * 5, L.paths + (size_t)p * 5);
          w3++;
        }
      L.npath = w3;
    }
  }
}

// ---- P3 metadata: response hops at the subject, then GET_METADATA_RESP arrivals in cid order ----
// One pass over the pending fetches (kept in cid order), only when one of them is due: the response hops due now
// (onMetadataRequest at the subject, MetadataStoreImpl.java:202-241) and the responses arriving now, compacted in
// place. A hop reads nothing an arrival writes (its loss draw is keyed by the message, SEMANTICS.md §2), so one pass
// runs both. A dead issuer keeps only its pending hops (their responses still count as sent at the live subject).
__device__ __forceinline__ void p3_metadata(ML& L, bool dead) {
  const Dev& d = *L.d;
  const uint32_t m = L.m, k = L.k;
  if (L.nfetch && L.fnext <= k) {
    uint32_t w = 0, fn = NEVER;
    const uint32_t nf = L.nfetch;  // no fetch is issued in P3
    for (uint32_t q = 0; q < nf; ++q) {
      FetchRec f = fetch_ld(L.fetch + (size_t)q * FREC);
      const uint32_t stage = fetch_stage(f);
      bool keep = true, mod = false;
      if (stage == 1 && f.hop == k) {
        mod = true;
        const uint32_t subj = f.subj;
        if (dead_at(d, subj, k)) {
          fetch_set_stage(f, 0);
        } else {
          L.c[C_M]++;
          const int e = xmit_ep(d, L.ep, K_GMD_RESP, subj, m, k, m, f.cid);
          if (e < 0) {
            L.c[C_LOST]++;
            fetch_set_stage(f, 0);
          } else {
            fetch_set_stage(f, 2);
            f.hop = k + d.lat + (uint32_t)e;
            f.meta = d.md_version[subj];
          }
        }
        keep = (!dead && f.group != FETCH_ORPHAN) || fetch_stage(f) == 1;
      } else if (stage == 2 && f.hop == k) {
        keep = false;
        if (!dead && f.group != FETCH_ORPHAN) {  // doOnSuccess (:563-567, :576-581): updateMetadata then sink.next
          const uint32_t subj = f.subj, inc = f.inc, meta = f.meta;
          const int g = (int)f.group;
          const uint32_t st = fetch_status(f), reason = fetch_reason(f), added = fetch_added(f);
          uint64_t v = row_ld(L, subj);
          uint32_t oldm = known_meta(L, subj, v);
          L.ra[subj] = aux32(v | META_BIT);
          const uint32_t u = d.md_uidx[subj];
          if (u != NONE32) d.md_ver[lidx(d, m) * MDU + u] = meta;
          if (added)
            emit_event(L, 0, subj, NONE32, meta);
          else
            emit_event(L, 2, subj, oldm, meta);
          if (g >= 0) grp(L, g)[4]--;
          finish(L, g, false);
          do_finally(L, subj, st, inc, reason);
        }
      } else if (dead) {
        keep = stage == 1;
      }
      if (keep) {
        if (w != q || mod) fetch_st(L.fetch + (size_t)w * FREC, f);
        w++;
        // the next due event (P5 recomputes it after its own pass)
        fn = min(fn, dead ? (fetch_stage(f) == 1 ? f.hop : NEVER) : fetch_due(f));
      }
    }
    L.nfetch = w;
    L.fnext = fn;
  }
}

// ---- P4 gossip first receipts in gossip-id order -> onMembershipGossip (:401-408) ----
// only the receipts that can change the row were routed (receipt_matters, gossip_apply.hip); the others were counted
// as record compares by the triage. off, n: the member's routed receipts (Dev::rc_off, rc_cnt)
__device__ __forceinline__ void p4_receipts(ML& L, uint32_t off, uint32_t n) {
  const Dev& d = *L.d;
  const uint32_t m = L.m;
  if (n) {
    d.rc_cnt[m] = 0;  // the next receipt routing counts from zero
    d.rc_fill[m] = 0;
  }
  // batches of PB receipts: their slot words and the rows they touch are loaded together (independent loads in
  // flight at once), then the updates run in order; update_membership re-reads the row (cache-hot), so a batch
  // that touches one subject twice still sees its own earlier write. (A member with many receipts in a tick after a
  // gossip plane runs them on a wave of its own instead: k_inbox_apply.)
  constexpr uint32_t PB = 8;
  for (uint32_t q0 = 0; q0 < n; q0 += PB) {
    const uint32_t nb = min(PB, n - q0);
    uint32_t gs[PB], subj[PB];
    uint64_t key[PB];
#pragma unroll
    for (uint32_t i = 0; i < PB; ++i) gs[i] = i < nb ? d.rc_slot[off + q0 + i] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < PB; ++i) {
      subj[i] = i < nb ? d.slot_subj[gs[i]] : USER_SUBJ;
      key[i] = i < nb ? d.slot_key[gs[i]] : 0ull;
    }
    uint32_t warm = 0;
#pragma unroll
    for (uint32_t i = 0; i < PB; ++i)
      if (subj[i] != USER_SUBJ) warm += L.rk[subj[i]] + L.ra[subj[i]];
    asm volatile("" ::"v"(warm));  // keep the warming loads
    for (uint32_t i = 0; i < nb; ++i) {
      if (subj[i] == USER_SUBJ) {  // sink.next -> ClusterImpl.listenGossips (:213-216), not membership
        const uint64_t gid = d.slot_gid[gs[i]];
        emit_event(L, 3, (uint32_t)(gid >> 32), (uint32_t)key[i], (uint32_t)(key[i] >> 32), (uint32_t)gid);
        continue;
      }
      L.c[C_R]++;
      update_membership(L, subj[i], rec_status(key[i]), rec_inc(key[i]), R_GOSSIP, -1);
    }
  }
}

// ---- P5 timers ----
__device__ __forceinline__ void p5_timers(ML& L) {
  const Dev& d = *L.d;
  const uint32_t k = L.k;
  if (L.nsub) {  // FD subscription timeouts in (cid, subscription) order
    uint32_t dcnt[SUBCAP], dkind[SUBCAP], dtgt[SUBCAP], nd = 0, w = 0, sm = NEVER;
    for (uint32_t s = 0; s < L.nsub; ++s) {
      uint32_t* S4 = L.subs + (size_t)s * 4;
      if (S4[SUB_DEADLINE] == k) {
        uint32_t j = nd++;
        while (j > 0 && dcnt[j - 1] > S4[SUB_CID]) {
          dcnt[j] = dcnt[j - 1];
          dkind[j] = dkind[j - 1];
          dtgt[j] = dtgt[j - 1];
          --j;
        }
        dcnt[j] = S4[SUB_CID];
        dkind[j] = S4[SUB_KIND];
        dtgt[j] = S4[SUB_TARGET];
      } else {
        sub_copy(L.subs + (size_t)w * 4, S4);
        w++;
        sm = min(sm, S4[SUB_DEADLINE]);
      }
    }
    L.nsub = w;
    L.smin = sm;  // (no subscription was added in this body before this pass)
    for (uint32_t q = 0; q < nd; ++q) {
      if (dkind[q] == 0)
        ping_req_step(L, dtgt[q], dcnt[q]);  // ping timeout (:159-175)
      else
        on_fd_event(L, dtgt[q], ST_SUSPECT);  // ping-req timeout (:204-212)
    }
  }
  if (L.nfetch && L.fnext <= k) {  // metadata timeouts: onErrorResume(TimeoutException) swallows the event (:568,582)
    uint32_t w = 0, fn = NEVER;
    const uint32_t nf = L.nfetch;  // no fetch is issued in P5
    for (uint32_t q = 0; q < nf; ++q) {
      FetchRec f = fetch_ld(L.fetch + (size_t)q * FREC);
      const uint32_t g0 = f.group;
      if (f.deadline == k) {
        const int g = (int)g0;
        if (g >= 0) grp(L, g)[4]--;
        finish(L, g, false);
        do_finally(L, f.subj, fetch_status(f), f.inc, fetch_reason(f));
        if (fetch_stage(f) != 1) continue;
        // the request is still in flight (delayed past the timeout): the subject still answers it, into nothing
        f.group = FETCH_ORPHAN;
        f.deadline = NEVER;
      }
      fn = min(fn, fetch_due(f));
      if (w != q || f.group != g0) fetch_st(L.fetch + (size_t)w * FREC, f);
      w++;
    }
    L.nfetch = w;
    L.fnext = fn;
  }
  if ((L.initFlags & INIT_ACTIVE) && !(L.initFlags & INIT_RECEIVED) && k == L.initDeadline) {
    L.initFlags &= ~INIT_ACTIVE;  // .timeout(syncTimeout) (:241) -> doFinally -> schedulePeriodicSync
    L.nextSync = k + d.sync_t;
  }
  if (L.timerMin <= k) {  // suspicion timeouts (:608-618), ascending subject; lazy minimum
    uint32_t nmin = NEVER;
    // one lane scans the whole aux plane: 16-B loads, four subjects each (rows are 32-B aligned); processing
    // subject s writes only entry s, so the loaded words of the later subjects stay current
    for (uint32_t s4 = 0; s4 < L.N; s4 += 4) {
      const uint4 a4 = *(const uint4*)(L.ra + s4);
      const uint32_t av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t s = s4 + j, a = av[j];  // the aux plane alone holds the deadline
        uint32_t dl = rec_timer((uint64_t)a << 34);
        if (dl == 0 || s >= L.N) continue;
        const uint64_t v = rec_join(L.rk[s], a);
        if (dl == k) {
          L.ra[s] = aux32(rec_with_timer(v, 0));
          if (rec_status(v) != ST_ABSENT) {
            L.c[C_R]++;
            update_membership(L, s, ST_DEAD, rec_inc(v), R_TIMEOUT, -1);
          }
        } else if (dl < nmin) {
          nmin = dl;
        }
      }
    }
    L.timerMin = nmin;
  }
}

// ---- P6 periodic tasks (schedulePeriodically) ----
__device__ __forceinline__ void p6_periodic(ML& L) {
  const Dev& d = *L.d;
  const uint32_t k = L.k;
  if (k == L.nextPing) {
    L.nextPing += mc_ping_t(d, L.m);
    do_ping(L);
  }
  if (k == L.nextGossip) {
    L.nextGossip += d.gossip_t;
    do_spread_gossip(L);
  }
  if (k == L.nextSync) {
    L.nextSync += d.sync_t;
    do_sync(L);
  }
}

// the member's next due event: a pending fetch, a ping path's hop or arrival, a subscription's deadline
__device__ __forceinline__ uint32_t next_event(const ML& L) {
  uint32_t nev = L.fnext;
  if (L.ev_ok) {  // from registers (P2, P5 and every add since)
    nev = min(nev, min(L.pmin, L.smin));
  } else {  // a resumed launch: the first four paths and subscriptions loaded together (one round trip)
    uint32_t t[8];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      t[q] = q < L.npath ? L.paths[(size_t)q * 5 + PATH_TICK] : NEVER;
      t[4 + q] = q < L.nsub ? L.subs[(size_t)q * 4 + SUB_DEADLINE] : NEVER;
    }
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) nev = min(nev, t[q]);
    for (uint32_t q = 4; q < L.npath; ++q) nev = min(nev, L.paths[(size_t)q * 5 + PATH_TICK]);
    for (uint32_t q = 4; q < L.nsub; ++q) nev = min(nev, L.subs[(size_t)q * 4 + SUB_DEADLINE]);
  }
  return nev;
}

// One member's tick (mode: member_kernels.h). cnt: the wave's op counters, this member's added. lfp: as p1_sync's.
template <uint32_t mode>
__device__ __forceinline__ void member_tick_body(const Dev& d, uint32_t m, uint32_t k, unsigned long long (&cnt)[8],
                                                 uint4* cw, uint32_t* cw_n, bool spec, uint64_t* lfp) {
  const bool dead = dead_at(d, m, k);
  ML L;
  ml_init(L, d, m, k, cw, cw_n, spec);
  if (mode == BODY_RESUME) park_load(L);  // what the parked member kept between the launches (k_inbox_apply updated it)
  // P1's inbound list head, loaded with the state above (P0's sends link into the other buffer)
  const uint32_t head0 = (mode != BODY_RESUME && !dead && k > 0) ? d.m_head[(size_t)((k - 1) & 1) * d.N + m] : NEVER;
  // the P6 ping's target and its liveness, loaded now (do_ping's loads would wait for this tick's stores)
  if (!dead && k == L.nextPing && L.fdLen > 0 && L.pingIdx >= 0 && L.pingIdx < (int32_t)L.fdLen) {
    L.pre = L.fdl[L.pingIdx];
    L.pre_dt = d.dead_tick[L.pre];
  }
  Lap lap(d);

  if (mode != BODY_RESUME) {
    p0_host_requests(L, dead);
    p0_start(L, dead);
    p1_sync(L, head0, lap, lfp);
    lap(0);  // P0 + P1
    L.ev_ok = true;  // this launch walks the path list (P2) and the subscriptions (P5)
    p2_fd(L, dead, lap);
    p3_metadata(L, dead);
    lap(1);  // P2 + P3
    if (dead) {  // only the hops of its in-flight requests ran (member_triage)
      fd_ready(L);
      link_flush(L);
      d.tround[m] = 0;
      d.ms[m].npath = L.npath;
      d.ms[m].nfetch = L.nfetch;
      d.ms[m].fnext = L.fnext;
      d.next_evt[m] = NEVER;
      tl_len_store(L);
      for (int i = 0; i < 8; ++i) cnt[i] += L.c[i];
      return;
    }
    const uint32_t off = d.rc_off[m], n = d.rc_cnt[m];
    if (mode == BODY_SPLIT && n >= d.hv) {  // many receipts: P4 in k_inbox_apply, P5 and P6 in the resumed launch
      d.hv_list[wave_append(d.nhv)] = m;
      park_store(L);
      flush_spreads(L);
      fd_ready(L);
      cow_seal(L);  // this launch's epilogue completes the open snapshots, undoing the writes logged so far
      ml_store(L);
      for (int i = 0; i < 8; ++i) cnt[i] += L.c[i];
      return;
    }
    p4_receipts(L, off, n);
    lap(2);  // P4
  }
  p5_timers(L);
  lap(3);  // P5
  p6_periodic(L);
  lap(4);  // P6

  flush_spreads(L);
  const uint32_t nev = next_event(L);
  cow_seal(L);
  fd_ready(L);
  d.next_evt[m] = nev;
  d.tround[m] = L.tround;
  ml_store(L);
  for (int i = 0; i < 8; ++i) cnt[i] += L.c[i];
}

// One launch per tick for member control. Each block triages its 256 members (the idle fast path, one thread per
// member, unconditional coalesced loads) and places the busy ones in an LDS list grouped by work class, each class
// starting on a wave boundary when they fit (block-local ballot prefixes, no atomics). Its waves then run the full
// control path for them: a wave holds one kind of work, so it does not serialise the latency chains of a ping, a
// ping hop and an ack arrival, and no wave runs mostly idle lanes. Counters are summed across the wave first
// (ctr_wave_add). With `flag` (W == 1) the block that finishes last runs the end-of-tick resets and raises the host
// flag. flag: MT_END = W == 1 (end-of-tick work), MT_SPEC = a launch of a speculative batch (spec.h).
// BODY_FULL on a one-GPU handle (light_mode): classes 1-3 are the members whose tick the light path knows
// (member_light.h) and run it; class 0, and whatever a light lane cannot finish, runs the general body afterwards.
// (MODE: BODY_FULL, or the two launches around k_inbox_apply, BODY_SPLIT and BODY_RESUME: three kernels, each with its
// own register allocation, so the steady-state one keeps the code it had before the split)
template <uint32_t MODE>
__global__ void __launch_bounds__(256, 2) k_member_tick_t(const Dev* __restrict__ dp, uint32_t k, uint32_t flag,
                                                          const MemberFront f) {
  // SWIM_EXP & 512: the wave's clock at its true entry, in front of the halt check and every load (stored as wt[WT_ENTRY]
  // once the launch is known to run: a halted launch stores nothing). Read only with the bit set, which the launch's
  // argument carries (f.exp: no load in front of it), and only by BODY_FULL, the instance the experiment traces.
  const unsigned long long t_entry = MODE == BODY_FULL && (f.exp & EXP_WAVE_CLOCK) ? wall_clock64() : 0ull;
  const Dev& d = *dp;  // global, not kernarg: taking its address must not copy ~1 KB into per-lane scratch
  const uint32_t m = (MODE == BODY_FULL ? f.lo : d.lo) + blockIdx.x * blockDim.x + threadIdx.x;
  // a speculative batch halted at an earlier tick (this tick's own halt is raised while it runs), or by a diff-halt:
  // returning before tick_reset keeps the lists and the pool as the lister left them (spec.h)
  // BODY_FULL: the halt words are loaded together with the triage's words, and the launch decides when both have
  // arrived: one wait where the halt check took its own in front of everything. Until the decision nothing is stored
  // and no atomic is issued, so a halted launch leaves no trace. (A lane past f.hi loads the last member's words: no
  // branch around the loads; member_triage is not called for it. f.hi >= 1: a launch has a block only if its range
  // [lo, hi) holds a member, so f.hi - 1 is the last member and the clamp keeps every lane inside the arrays.)
  TriageWords tw;
  if constexpr (MODE == BODY_FULL) {
    // Every address comes from the launch's argument f (member_kernels.h): no scalar load through dp lies in front.
    const HaltWords hw = halt_load(f.halt);  // (every launch: a branch around the load would wait for it at its end)
    tw = triage_load(f, min(m, f.hi - 1u), k);
    triage_arrived(tw, hw);
    if (mt_spec(flag) && halted_member(hw, k, mt_lf(flag))) return;
  } else {
    if (mt_spec(flag) && halted_member(d.halt, k, mt_lf(flag))) return;
  }
  // a speculative launch resets the next tick's counters at its start (nothing in this kernel uses them), so no block
  // waits for the last one at its end: the halt that tick_flag would raise is raised by the member taking a slot
  // (a split tick's launches are never speculative: kernels.hip launch_member)
  const bool spec1 = MODE == BODY_FULL && mt_spec_one_gpu(flag);
  if (mt_spec_one_gpu(flag) && blockIdx.x == 0 && threadIdx.x == 0) tick_reset(d, k);
  // SWIM_EXP & 512 (timing experiment): wall clock of each wave at entry, after triage, after its bodies, at exit
  const bool wtime = (d.exp & EXP_WAVE_CLOCK) != 0;
  unsigned long long* wt = wtime ? d.wt + ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * WT_WORDS : nullptr;
  if (wtime && (threadIdx.x & 63) == 0) {
    wt[0] = wall_clock64();
    if (MODE == BODY_FULL) wt[WT_ENTRY] = t_entry;
  }
  __shared__ uint32_t wc[4][4];  // [wave][class] busy members
  __shared__ uint32_t list[256];
  __shared__ uint4 cw[CWMAX];  // deferred copy-on-write snapshots of this block's members (cow)
  __shared__ uint32_t cw_n;
  if (threadIdx.x == 0) cw_n = 0;
  if (threadIdx.x < CWMAX) cw[threadIdx.x].x = NEVER;  // no member until written (cow scans by member)
  constexpr bool resume = MODE == BODY_RESUME;  // the parked members' P5 and P6 (one lane each, from the list)
  uint32_t cls = 0, drops = 0, evs = 0;
  // no lister ran for this tick: each lane's share of the lister's counts (lf_count), from the triage and from P1 (in
  // LDS: a register would be held across the whole body)
  const bool nolist = MODE == BODY_FULL && mt_nolist(flag);  // (a split tick is never queued without its lister)
  __shared__ uint64_t lfs[256];
  uint64_t lft = 0;
  // the light path (member_light.h): the launch's mode, and beside list[] each listed member's inbound list head (the
  // triage's load) and the members whose light attempt fell back to the general body
  uint32_t light = 0;
  if constexpr (MODE == BODY_FULL) light = light_mode(d);
  __shared__ uint32_t lhead[MODE == BODY_FULL ? 256 : 1], fbl[MODE == BODY_FULL ? 256 : 1];
  __shared__ uint32_t fb_n;
  if (MODE == BODY_FULL && threadIdx.x == 0) fb_n = 0;
  uint32_t mhead = NEVER;
  const bool busy = !resume && m < d.hi &&
                    member_triage(d, m, k, cls, drops, evs, nolist, lft, light, mhead,
                                  MODE == BODY_FULL ? tw : triage_load(d, m, k));
  if (nolist) lfs[threadIdx.x] = lft;
  {  // the triage's record compares and folded RUMOR events, one atomic each per wave
    const uint32_t v = wave_sum(drops), e = wave_sum(evs);
    unsigned long long* cs = d.ctr_sh + (size_t)(blockIdx.x % CSH) * CSTRIDE;
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&cs[C_R], (unsigned long long)v);
    if ((threadIdx.x & 63) == 0 && e) atomicAdd(&cs[C_E], (unsigned long long)e);
  }
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t b0 = __ballot(busy && cls == 0), b1 = __ballot(busy && cls == 1), b2 = __ballot(busy && cls == 2),
                 b3 = __ballot(busy && cls == 3);
  if (lane == 0) {
    wc[w][0] = (uint32_t)__popcll(b0);
    wc[w][1] = (uint32_t)__popcll(b1);
    wc[w][2] = (uint32_t)__popcll(b2);
    wc[w][3] = (uint32_t)__popcll(b3);
  }
  list[threadIdx.x] = NEVER;
  __syncthreads();
  uint32_t aligned = 0, dense = 0, all = 0, before = 0;
  for (uint32_t c = 0; c < 4; ++c) {
    const uint32_t t = wc[0][c] + wc[1][c] + wc[2][c] + wc[3][c];
    all += (t + 63u) & ~63u;
    if (c < cls) aligned += (t + 63u) & ~63u, dense += t;
  }
  const uint32_t start = all <= 256 ? aligned : dense;  // classes on wave boundaries when they fit, else packed
  for (uint32_t j = 0; j < w; ++j) before += wc[j][cls];
  const uint64_t bal = cls == 0 ? b0 : cls == 1 ? b1 : cls == 2 ? b2 : b3;
  uint32_t slot = start + before + __popcll(bal & ((1ull << lane) - 1ull));
  if (busy) list[slot] = m | (cls << 30);  // m < 2^30
  if (MODE == BODY_FULL && busy && light) lhead[slot] = mhead;
  __syncthreads();
  uint32_t ent = list[threadIdx.x];
  if (resume) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    ent = i < *d.nhv ? d.hv_list[i] : NEVER;  // class 0
  }
  const uint32_t me = ent == NEVER ? NEVER : (ent & 0x3FFFFFFFu), mcls = ent >> 30;
  if (wtime) {  // [1]: after triage, with the wave's class mix in the top byte
    const uint64_t cm = (__ballot(me != NEVER && mcls == 0) ? 1ull : 0ull) | (__ballot(me != NEVER && mcls == 1) ? 2ull : 0ull) |
                        (__ballot(me != NEVER && mcls == 2) ? 4ull : 0ull) | (__ballot(me != NEVER && mcls == 3) ? 8ull : 0ull);
    const uint32_t nb = (uint32_t)__popcll(__ballot(me != NEVER));
    if ((threadIdx.x & 63) == 0) wt[1] = wall_clock64() | (cm << 56) | ((uint64_t)nb << 48);
  }
  // SWIM_EXP & 32 / 64 (timing experiments, wrong results): skip the bodies of class 0 / of classes 1-3
  if constexpr (MODE != BODY_FULL) {
    if (__ballot(me != NEVER)) {  // waves with no busy member skip to the end
      unsigned long long cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      const bool skip = ((d.exp & EXP_SKIP_CLASS0) && mcls == 0) || ((d.exp & EXP_SKIP_CLASS123) && mcls != 0);
      if (me != NEVER && !skip)
        member_tick_body<MODE>(d, me, k, cnt, cw, &cw_n, spec1, nolist ? &lfs[threadIdx.x] : nullptr);
      ctr_wave_add(d, cnt, lane);
    }
  } else {
    // With the light path on, the waves of classes 1-3 try it first. Every member that needs the general body (class 0,
    // and a light lane that must fall back: beside its wave's light lanes divergence would run both paths one after the
    // other) is listed in LDS, and after a barrier the block's first lanes run the general body for the list: one call
    // site, reached with nothing of the light path live. With it off the lanes run their own entries, as BODY_SPLIT.
    const bool skip = ((d.exp & EXP_SKIP_CLASS0) && mcls == 0) || ((d.exp & EXP_SKIP_CLASS123) && mcls != 0);
    uint32_t gm = skip ? NEVER : me;  // the member whose general body this lane runs
    bool any = __ballot(me != NEVER) != 0ull;  // waves with no busy member skip to the end
    if (light) {
      if (any) {
        unsigned long long lc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t did = 0;  // the attempt's LT_ bits
        bool gen = gm != NEVER && mcls == 0;
        if (gm != NEVER && mcls != 0) {
          did = member_light(d, gm, k, lhead[threadIdx.x], spec1, nolist ? &lfs[threadIdx.x] : nullptr, lc);
          gen = (did & LT_FALLBACK) != 0u;
        }
        if (gen) fbl[wave_append(&fb_n)] = gm;  // (LDS)
        if (__ballot(did != 0u)) {
          ctr_wave_add(d, lc, lane);
          light_count(d, did, lane);
        }
      }
      if (wtime && (threadIdx.x & 63) == 0) wt[2] = wall_clock64();
      __syncthreads();
      gm = threadIdx.x < fb_n && !(d.exp & EXP_SKIP_CLASS0) ? fbl[threadIdx.x] : NEVER;
      any = __ballot(gm != NEVER) != 0ull;
    }
    if (any) {
      unsigned long long cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (gm != NEVER) member_tick_body<MODE>(d, gm, k, cnt, cw, &cw_n, spec1, nolist ? &lfs[threadIdx.x] : nullptr);
      ctr_wave_add(d, cnt, lane);
      // (counted with the path on, and for a handle that counts its fallbacks: the tests' reference path)
      if (light || d.fb) light_count_general(d, gm != NEVER, lane);
    }
    if (!light && wtime && (threadIdx.x & 63) == 0) wt[2] = wall_clock64();
  }
  const uint64_t lfc = nolist ? lfs[threadIdx.x] : 0ull;
  if (nolist && __ballot(lfc != 0ull)) {  // (wave-uniform) into the block's counter row, as the op counters
    unsigned long long* cs = d.ctr_sh + (size_t)(blockIdx.x % CSH) * CSTRIDE + SH_LF;
#pragma unroll
    for (uint32_t i = 0; i < 3; ++i) {
      const uint32_t v = wave_sum((uint32_t)(lfc >> (LFC_BITS * i)) & LFC_MASK);
      if (lane == 0 && v) atomicAdd(&cs[i], (unsigned long long)v);
    }
  }
  if (MODE != BODY_FULL && wtime && (threadIdx.x & 63) == 0) wt[2] = wall_clock64();  // (BODY_FULL: above)
  // deferred copy-on-write: the block copies each snapshot's row (final for this tick: only its member writes it),
  // then one lane undoes the member's logged writes since the snapshot opened, newest first
  __syncthreads();
  const uint32_t ncw = min(cw_n, d.cwmax_cap);
  for (uint32_t q = 0; q < ncw; ++q) {
    const uint4 e = cw[q];
    if (e.x == NEVER) continue;  // made by its lane already (cow_now)
    const uint32_t b = k & 1;
    const size_t li = lidx(d, e.x);
    const uint4* src4 = (const uint4*)(d.rowk + li * d.NS);
    uint4* dst4 = (uint4*)(d.arena[b] + (size_t)e.y * d.NS);
    for (uint32_t s = threadIdx.x; s < d.NS / 4; s += blockDim.x) dst4[s] = src4[s];
    if (d.W > 1)
      for (uint32_t w = threadIdx.x; w < d.MW; w += blockDim.x)
        d.arena_dirty[b][(size_t)e.y * d.MW + w] = d.rdirty[li * d.MW + w];
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t* dst = d.arena[b] + (size_t)e.y * d.NS;
      const uint32_t* lg = d.ulog + li * d.ULOGC * 2;
      for (uint32_t j = e.w; j-- > e.z;) dst[lg[2 * j]] = lg[2 * j + 1];
    }
    __syncthreads();
  }
  if (wtime && (threadIdx.x & 63) == 0) wt[3] = wall_clock64();
  if (!mt_closes_tick(flag)) return;
  if (!last_block_ticket(d.mdone, gridDim.x) || threadIdx.x != 0) return;
  *d.mdone = 0;
  if (resume) *d.nhv = 0;  // every block has read the list
  tick_flag(d, k);
}

template __global__ void k_member_tick_t<BODY_FULL>(const Dev* __restrict__, uint32_t, uint32_t, const MemberFront);
template __global__ void k_member_tick_t<BODY_SPLIT>(const Dev* __restrict__, uint32_t, uint32_t, const MemberFront);
template __global__ void k_member_tick_t<BODY_RESUME>(const Dev* __restrict__, uint32_t, uint32_t, const MemberFront);

}  // namespace swim
