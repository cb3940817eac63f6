// inbox.hip — k_inbox_apply: P4 of a parked member on one wave, between the two k_member_tick_t launches of a split
// tick (member.hip; kernels.hip launch_member).
//
// A member with many routed gossip receipts (C2: a few hundred in a tick) ran them one after another on its lane,
// each a chain of dependent loads, while 63 lanes of another member's wave waited. Here the member's receipts are taken
// 64 at a time in gossip-id order. A receipt of the common case (another member's present row, a record that is not
// DEAD) touches only its subject's row entry, the metadata-fetch list, the correlation counter and the write log, and
// on a present row isOverrides (MembershipRecord.java:66-84) is the order of the packed keys: a receipt is accepted iff
// its key is above the largest of the row's and every earlier same-subject key of the batch (a segmented prefix
// maximum). Its correlation id, fetch-list place and write-log place are prefix sums in gossip-id order, so every
// per-member sequence is the one the lane-serial P4 produces. Any other receipt (the member's own record, a DEAD
// record, an absent row, a user gossip) runs the full update on lane 0 between batches.
#include "member_kernels.h"
#include "member_proto.h"

namespace swim {

// one batch: lanes [0, cnt) hold common-case receipts (subject s, record s1 / i1, row entry k0 / a0 before the batch)
__device__ __forceinline__ void inbox_batch(ML& L, uint32_t lane, uint32_t cnt, uint32_t s, uint32_t s1, uint32_t i1,
                                            uint32_t k0, uint32_t a0, bool dead) {
  const Dev& d = *L.d;
  const bool act = lane < cnt;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const uint32_t kk = (i1 << 2) | s1;
  uint32_t pm = 0;  // the largest earlier key of this subject in the batch
  for (uint32_t o = 0; o < cnt; ++o) {
    const uint32_t so = __shfl(s, (int)o), ko = __shfl(kk, (int)o);
    if (o < lane && so == s) pm = max(pm, ko);
  }
  const uint32_t run = max(k0, pm);  // the subject's key just before this receipt
  const bool acc = act && kk > run;
  const unsigned long long am = __ballot(acc);
  // the accepted receipts before this one: of any subject (write log) and of this subject (suspicion timer)
  uint32_t pacc = 0, prev = L.tlast;
  bool alive_before = false, acc_before = false, acc_later = false;
  for (uint32_t o = 0; o < cnt; ++o) {
    if (!((am >> o) & 1ull)) continue;
    const uint32_t so = __shfl(s, (int)o), sto = __shfl(s1, (int)o);
    if (o < lane) {
      acc_before = true;
      prev = so;
      if (so == s) {
        pacc = sto;
        alive_before |= sto == ST_ALIVE;
      }
    } else if (o > lane && so == s) {
      acc_later = true;
    }
  }
  // scheduleSuspicionTimeoutTask (:597-606, computeIfAbsent) / cancelSuspicionTimeoutTask (:590-595) along the chain:
  // every deadline set in this tick is the same
  const uint32_t dl = L.k + suspicion_ticks(d, L.tsize, mc_ping_t(d, L.m));
  const uint64_t v0 = rec_join(k0, a0);
  const uint32_t T0 = rec_timer(v0);
  if (__ballot(acc && s1 == ST_SUSPECT && (pacc == ST_ALIVE || (pacc == 0 && T0 == 0)))) L.timerMin = min(L.timerMin, dl);
  if (acc && !acc_later) {  // the subject's last accepted record is what the row holds after the batch
    uint64_t v = (v0 & ~KEY_MASK) | rec_key(s1, i1);
    v = rec_with_timer(v, s1 == ST_SUSPECT ? ((alive_before || T0 == 0) ? dl : T0) : 0u);
    key_put(d, L.rk, L.rd, lidx(d, L.m), s, key32(v), k0, false);
    L.ra[s] = aux32(v);
  }
  dirty_mark_wave(L.rd, acc && !acc_later, s);  // (an accepted key is above the row's: every one is a change)
  if (act) L.c[C_R]++;
  if (acc) L.c[C_W]++;
  if (d.ackres) {  // tl_add of each accepted write, in order
    const bool flag = acc && !((L.ntl > 0 || acc_before) && prev == s);
    const unsigned long long fm = __ballot(flag);
    const uint32_t p = L.ntl + (uint32_t)__popcll(fm & lt);
    if (flag && p < TL) L.tl[p] = s;
    L.ntl = min(TL + 1u, L.ntl + (uint32_t)__popcll(fm));
    if (am) L.tlast = __shfl(s, 63 - (int)__clzll(am));
  }
  // fetchMetadata for an incarnation increase (:572-584): ids and fetch-list places in gossip-id order
  const bool fet = acc && (run >> 2) < i1;
  const unsigned long long fm = __ballot(fet);
  int e = -1;
  if (fet) {
    L.c[C_M]++;
    e = xmit_ep(d, L.ep, K_GMD_REQ, L.m, s, L.k, L.m, L.cidCnt + (uint32_t)__popcll(fm & lt), dead ? 1 : 0);
    if (e < 0) L.c[C_LOST]++;
  }
  L.cidCnt += (uint32_t)__popcll(fm);
  const bool kept = fet && e >= 0;
  const unsigned long long km = __ballot(kept);
  uint32_t fn = NEVER;
  if (kept) {
    const uint32_t q = L.nfetch + (uint32_t)__popcll(km & lt);
    if (q >= d.FCAP) {
      set_err(d, E_FETCH);
    } else {  // the record fetch_md writes: no group, stage 1 (response hop pending)
      const uint32_t cid = L.cidCnt - (uint32_t)__popcll(fm) + (uint32_t)__popcll(fm & lt);
      const FetchRec f{cid, s, i1, fetch_pack(s1, R_GOSSIP, 0, 1),
                       0xFFFFFFFFu, L.k + d.md_t, L.k + d.lat + (uint32_t)e, NONE32};
      fetch_st(L.fetch + (size_t)q * FREC, f);
      fn = min(f.deadline, f.hop);
    }
  }
  fn = wave_min(fn);
  L.nfetch = min(d.FCAP, L.nfetch + (uint32_t)__popcll(km));
  L.fnext = min(L.fnext, fn);
}

__device__ void inbox_member(const Dev& d, uint32_t m, uint32_t k, uint32_t lane) {
  ML L;
  ml_init(L, d, m, k, nullptr, nullptr, false);  // every lane holds the member's state
  park_load(L);
  const uint32_t off = d.rc_off[m], n = d.rc_cnt[m];
  // a SYNC / SYNC_ACK of this tick still carries the live row: its snapshot, copied by the wave before the first batch
  // that may write the row (an accepted receipt's key is above the row's; lane 0's receipts may write), not before
  auto snapshot = [&]() {
    const uint32_t b = k & 1;
    uint32_t r = 0;
    if (lane == 0) r = atomicAdd(&d.arena_used[b], 1u);
    r = __shfl(r, 0);
    if (r >= d.ARENA_ROWS) {
      if (lane == 0) set_err(d, E_ARENA);
    } else {
      const uint4* src4 = (const uint4*)L.rk;
      uint4* dst4 = (uint4*)(d.arena[b] + (size_t)r * d.NS);
      for (uint32_t q = lane; q < d.NS / 4; q += 64) dst4[q] = src4[q];
      if (lane == 0)
        for (uint32_t i = L.pend; i != NEVER; i = d.msgs[b][i].pad) d.msgs[b][i].payload = r;
    }
    L.pend = NEVER;
    __threadfence_block();
  };
  for (uint32_t pos = 0; pos < n;) {
    const uint32_t j = pos + lane;
    const bool act = j < n;
    const uint32_t g = act ? d.rc_slot[off + j] : 0u;
    const uint32_t s = act ? d.slot_subj[g] : USER_SUBJ;
    const uint64_t key = act ? d.slot_key[g] : 0ull;
    const bool mem = act && s != USER_SUBJ;
    const uint32_t k0 = mem ? L.rk[s] : 0u, a0 = mem ? L.ra[s] : 0u, dt = mem ? d.dead_tick[s] : NEVER;
    const uint32_t s1 = rec_status(key), i1 = rec_inc(key);
    const bool fast = mem && s != m && (k0 & 3u) != ST_ABSENT && s1 != ST_DEAD && i1 < INC_LIMIT;
    const unsigned long long slow = __ballot(act && !fast);
    const uint32_t f = slow ? (uint32_t)__ffsll((long long)slow) - 1u : 64u;
    const uint32_t cnt = min(f, n - pos);
    if (L.pend != NEVER && __ballot((lane < cnt && key32(key) > k0) || (f < 64u && lane == f))) snapshot();
    if (cnt) inbox_batch(L, lane, cnt, s, s1, i1, k0, a0, k >= dt);
    __threadfence_block();  // the batch's row writes, before any lane reads the row again
    if (f == 64u) {
      pos += cnt;
      continue;
    }
    const uint32_t gs = __shfl(g, (int)f), ss = __shfl(s, (int)f);
    const uint32_t klo = __shfl((uint32_t)key, (int)f), khi = __shfl((uint32_t)(key >> 32), (int)f);
    const uint64_t kf = ((uint64_t)khi << 32) | klo;
    if (lane == 0) {
      if (ss == USER_SUBJ) {  // sink.next -> ClusterImpl.listenGossips (:213-216)
        const uint64_t gid = d.slot_gid[gs];
        emit_event(L, 3, (uint32_t)(gid >> 32), (uint32_t)kf, (uint32_t)(kf >> 32), (uint32_t)gid);
      } else {
        L.c[C_R]++;
        update_membership(L, ss, rec_status(kf), rec_inc(kf), R_GOSSIP, -1);
      }
    }
    ml_bcast(L);
    __threadfence_block();
    pos += f + 1;
  }
  if (lane == 0) {  // the gossips lane 0 created (refutations) take their slots; the FD list inserts land
    flush_spreads(L);
    fd_ready(L);
  }
  ctr_wave_add(d, L.c, lane);
  if (lane != 0) return;
  ml_store(L);
  park_store(L);
  d.rc_cnt[m] = 0;  // the next receipt routing counts from zero
  d.rc_fill[m] = 0;
}

__global__ void __launch_bounds__(256) k_inbox_apply(const Dev* __restrict__ dp, uint32_t k) {
  const Dev& d = *dp;
  const uint32_t nh = *d.nhv, lane = threadIdx.x & 63u;
  for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nh; i += gridDim.x * 4) inbox_member(d, d.hv_list[i], k, lane);
}

}  // namespace swim
