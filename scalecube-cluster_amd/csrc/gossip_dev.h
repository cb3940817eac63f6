// gossip_dev.h — the gossip data plane: GossipProtocolImpl.doSpreadGossip (:139-157), selectGossipsToSend (:239-250),
// onGossipReq (:171-183) and sweepGossips (:283-308) for every member at once. One file per stage of
// the tick, in launch order (launch_gossip_send, launch_gossip_apply):
//   gossip_round.hip     1-4  active groups, round planning, senders by target, the rounds' sweeps and windows
//   gossip_contacts.hip  5    the pairs with a logged contact: their contact caches and RX rows
//   gossip_send.hip      6-7  target-major sends; the replayed, slow and delayed sends; launch_gossip_send
//   gossip_apply.hip     8-9  the receivers' side, slot recycling, exchange B; launch_gossip_apply, launch_unpack_b
//   gossip_replay.h           infectedFrom without storing it (stages 5 and 7)
// Here: the device helpers more than one stage uses, and the kernels as launch_gossip_send names them.
//
// Holder state. Per member, the held gossips are a bit row HB over slot ids and a ring of (slot, infection period)
// entries in receipt order. The infection period of an entry is the member's gossip period at its receipt
// (GossipState.infectionPeriod), so it never decreases along the ring: a round's sweep (period > infP + 2(spread+1))
// removes a prefix and the spread window (infP + spread >= period) is a suffix. The window bit row WB is rebuilt
// at each of the member's rounds from the ring entries whose status changed since its previous round (swept, left
// the window, re-entered it after the spread grew, or received since), so a round costs the entries it moves, not a
// scan of the slot table. (Ring entries and the row accessors: dev_util.h.)
#pragma once
#include "dev_util.h"

namespace swim {

// incarnation history of (gid, member): creation ticks of swept incarnations (rebirths are rare)
__device__ __forceinline__ uint64_t hist_tag(uint64_t gid, uint32_t member) {
  return mix64(gid ^ ((uint64_t)member * 0x9E3779B97F4A7C15ull)) | 1ull;
}

__device__ void hist_push(const Dev& d, uint64_t gid, uint32_t member, uint32_t cprev) {
  uint64_t tag = hist_tag(gid, member);
  uint32_t mask = d.HCAP - 1;
  for (uint32_t p = 0; p < d.HCAP; ++p) {
    unsigned long long* e = (unsigned long long*)(d.hist + (size_t)((tag + p) & mask) * HREC);
    unsigned long long old = atomicCAS(e, 0ull, (unsigned long long)tag);
    if (old != 0ull && old != tag) continue;
    if (old == 0ull) {
      e[1] = gid;
      e[2] = member;
      // entries in use, sampled: one entry in 8 counts 8 (grow_caps enlarges the table past half full; one counter
      // taking an atomic per rebirth would serialise the heal of a C4 storm)
      if (d.hist_n && (tag & 0x700ull) == 0) atomicAdd(d.hist_n, 8u);
    }
    uint32_t n = (uint32_t)(e[2] >> 32);  // total rebirths so far; the ring keeps the latest HKEEP
    uint32_t* c = (uint32_t*)(e + 3);
    c[n % HKEEP] = cprev;
    e[2] = (uint64_t)member | ((uint64_t)(n + 1) << 32);
    return;
  }
  if (atomicOr(d.err, E_REBORN) == 0) d.err[1] = 1;  // info 1: the history table is full (HCAP)
}

// creation tick of member's incarnation of g that existed at tick tau (NEVER if none)
__device__ uint32_t inc_at(const Dev& d, uint32_t member, uint32_t g, uint64_t gid, uint32_t tau, uint32_t ref) {
  uint32_t e = s_get(d, g, member, ref);
  if (!s_ever(e)) return NEVER;
  uint32_t c = s_ctick(e);
  if (c <= tau) return c;
  if (!(e & S_REBORN)) return NEVER;
  uint64_t tag = hist_tag(gid, member);
  uint32_t mask = d.HCAP - 1;
  for (uint32_t p = 0; p < d.HCAP; ++p) {
    const uint64_t* h = d.hist + (size_t)((tag + p) & mask) * HREC;
    if (h[0] == 0) break;
    if (h[0] != tag || h[1] != gid || (uint32_t)h[2] != member) continue;
    uint32_t n = (uint32_t)(h[2] >> 32), best = NEVER, oldest = NEVER;
    const uint32_t* cc = (const uint32_t*)(h + 3);
    uint32_t kept = n < HKEEP ? n : HKEEP;
    for (uint32_t i = 0; i < kept; ++i) {
      if (cc[i] < oldest) oldest = cc[i];
      if (cc[i] <= tau && (best == NEVER || cc[i] > best)) best = cc[i];
    }
    if (best == NEVER && n > HKEEP && tau < oldest && atomicOr(d.err, E_REBORN) == 0)
      d.err[1] = 2;  // info 2: an incarnation the ring dropped (more than HKEEP rebirths)
    return best;
  }
  return NEVER;
}

// a first receipt of (g, t) at this tick (one lane owns it): the receiver-side bookkeeping that does not depend on
// the other receipts of the tick happens at once (held bit, ring entry, DEAD-record stamp, exchange record)
__device__ __forceinline__ void receipt_mark(const Dev& d, uint32_t g, uint32_t t, uint32_t k, uint32_t pos) {
  ring(d, t)[pos & (d.BCAP - 1)] = rg_entry(g, rounds_before(d, t, k + d.lat));
  if (pos + 1u - d.rhead[t] > d.BCAP) set_err(d, E_RING);
}

// the rest of it for a single send whose lane has just won the held bit of (g, t) by an atomic (deliver_one,
// k_gossip_due): a DEAD membership record arrives in P4 of k + lat, the next ring entry, the exchange-B record
__device__ __forceinline__ void first_receipt(const Dev& d, uint32_t g, uint32_t t, uint32_t k) {
  if (d.DM[g >> 6] & (1ull << (g & 63u))) d.dead_rx[t] = k + d.lat;
  receipt_mark(d, g, t, k, atomicAdd(&d.rtail[t], 1u));
  xd_push(d, g, t);
}

// the holder-table entry of a first receipt (onGossipReq :176-180): the incarnation created at tick k + lat; a
// rebirth after a sweep keeps the swept incarnation's creation tick in the history (infectedFrom replay)
__device__ __forceinline__ void receipt_create(const Dev& d, uint32_t g, uint32_t t, uint32_t k) {
  const uint32_t e = s_get(d, g, t, k + d.lat);
  if (s_ever(e)) hist_push(d, d.slot_gid[g], t, s_ctick(e));
  s_put(d, g, t, k + d.lat, s_ever(e));
  if (d.dly_on)  // a delayed first receipt still queued may have pushed it further (delay_push)
    atomicMax(&d.slot_exp[g], k + d.lat + d.EXPB);
  else
    d.slot_exp[g] = k + d.lat + d.EXPB;  // every holder sweeps it by then (all receipts of a tick store the same value)
}

// a cooperative group of threads: one workgroup (BLOCK) or one wavefront
template <bool BLOCK>
__device__ __forceinline__ void grp_sync() {
  if (BLOCK) {
    __syncthreads();
  } else {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
}

// f(slot) for the ring entries at positions [a, b) of ring R, a group of nth threads (tid) taking every nth: four
// loads in flight per thread before their uses (a plain loop waited out each load: C2 walks ~10^4 entries per member)
template <typename F>
__device__ __forceinline__ void ring_walk(const uint32_t* R, uint32_t mask, uint32_t a, uint32_t b, uint32_t tid,
                                          uint32_t nth, F f) {
  const uint32_t n = b - a;
  uint32_t o = tid;
  for (; o + 3 * nth < n; o += 4 * nth) {
    const uint32_t g0 = R[(a + o) & mask], g1 = R[(a + o + nth) & mask], g2 = R[(a + o + 2 * nth) & mask],
                   g3 = R[(a + o + 3 * nth) & mask];
    f(g0 & RG_SLOT);
    f(g1 & RG_SLOT);
    f(g2 & RG_SLOT);
    f(g3 & RG_SLOT);
  }
  for (; o < n; o += nth) f(R[(a + o) & mask] & RG_SLOT);
}

// ------------------------------------------------------------------------------------------------------------
// the kernels launch_gossip_send (gossip_send.hip) launches from the earlier stages' files, and the LDS row chunks it
// sizes for them
constexpr uint32_t RCW = 4096;  // words per row chunk, block per member (large rows): k_round_apply_b
constexpr uint32_t RCS = 1024;  // words per row, wave per member (rows of up to 65 536 slots): k_round_apply_w
constexpr uint32_t RXW = 8192;  // words per RX row chunk at most: k_rx_build
__global__ void k_gossip_groups(Dev d);                                                            // gossip_round.hip
__global__ void k_round_plan(Dev d, uint32_t k);
__global__ void k_tin_scatter(Dev d);
__global__ void k_round_apply_w(const Dev* __restrict__ dp, uint32_t k, uint32_t cw);
__global__ void k_round_apply_b(const Dev* __restrict__ dp, uint32_t k, uint32_t cb, uint32_t cw);
__global__ void k_gossip_contacts(Dev d, uint32_t k);                                              // gossip_contacts.hip
__global__ void k_contact_cache(const Dev* __restrict__ dp, uint32_t k);
__global__ void k_rx_build(const Dev* __restrict__ dp, uint32_t cx);

}  // namespace swim
