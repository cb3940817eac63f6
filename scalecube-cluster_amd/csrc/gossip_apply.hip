// gossip_apply.hip — the gossip data plane, steps 8-9 and exchange B: the receivers' side of this tick's first
// receipts (holder table, P4 routing), slot recycling, and the peers' first receipts into a shard's replicated holder
// state (gossip_dev.h: the plane's file map and the holder state).
#include "gossip_dev.h"

namespace swim {

// P4 pre-filter (onMembershipGossip -> updateMembership, MembershipProtocolImpl.java:401-408,475-485). A first
// receipt is routed to P4 of tick k4 unless it provably cannot change t's row there: its record does not override
// the row as it stands now (= at the start of tick k4), the row is present, and the row cannot be removed before the
// receipt in that tick. Present rows only move up the isOverrides order except through a removal, so a record that
// does not override the start row overrides no later one. A removal needs a DEAD record: in P4 another receipt
// (dead_rx[t] = k4, stamped by the delivering send), or in P1 a leaver's own record in SYNC data (leaving[subject]);
// after one the row is absent or re-added at any incarnation (an absent row accepts any ALIVE,
// MembershipRecord.java:67-69), so every receipt is kept then. An absent start row keeps every receipt (the row may
// become present earlier in the tick). User gossips are always routed (each one emits a GOSSIP event).
__device__ __forceinline__ bool receipt_matters(const Dev& d, uint32_t t, uint32_t g, uint32_t k4) {
  const uint32_t subj = d.slot_subj[g];
  if (subj == USER_SUBJ || (d.exp & EXP_ROUTE_ALL)) return true;  // SWIM_EXP & 8: route every receipt (debugging aid)
  const uint64_t key = d.slot_key[g];
  const uint32_t r0 = d.rowk[lidx(d, t) * d.NS + subj], s1 = rec_status(key);
  if ((r0 & 3u) == ST_ABSENT || overrides(s1, rec_inc(key), r0 & 3u, r0 >> 2)) return true;
  return d.dead_rx[t] == k4 || d.leaving[subj];
}

// 8. first receipts of this shard's targets: the entries each target's ring gained this tick. Holder table, expiry,
// gossip count, then membership: records that can change the row are queued for P4 of k + lat in gossip-id order
// (receipt routing), the others are counted as record compares; RUMOR mode hashes the GOSSIP events here (fastp4).
// The senders' lists are reset for the next tick. A wave takes 64 targets: those with at most APPLY_LANE new entries
// (C3 with membership evolution: one to three) on a lane each; the others (C2: a few hundred) are listed for
// k_gossip_apply_big, a wave each, so neither 63 idle lanes per target nor one lane walking hundreds of entries hold
// the launch.
constexpr uint32_t APPLY_LANE = 8;

// the target's bookkeeping once its entries are applied (one lane)
__device__ __forceinline__ void apply_target_end(const Dev& d, uint32_t t, uint32_t a, uint32_t b, uint32_t drops,
                                                 unsigned long long eh) {
  const uint32_t nr = b - a;
  // the host grows the rings before they can overflow (the atomic only when the fill beats the maximum so far:
  // one address taking an atomic from every target serialises, ~13 ns each)
  if (d.rfill && b - d.rhead[t] > __hip_atomic_load(d.rfill, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(d.rfill, b - d.rhead[t]);
  if (nr) {
    if (d.XW > 1)
      atomicAdd(&d.held_delta[t], (int)nr);
    else
      atomicAdd(&d.held[t], nr);
  }
  if (drops) atomicAdd(&d.rc_ndrop[t], drops);
  if (d.fastp4 && nr) {
    atomicAdd(&d.evp_hash[t], eh);
    atomicAdd(&d.evp_n[t], nr);
  }
  d.tin_cnt[t] = 0;
  d.tin_fill[t] = 0;
}

// one entry at ring position p of target t: holder table and expiry; true if its record is routed to P4
__device__ __forceinline__ bool apply_entry(const Dev& d, uint32_t t, uint32_t g, uint32_t k, uint32_t& drops,
                                            unsigned long long& eh) {
  receipt_create(d, g, t, k);
  if (d.fastp4 && d.slot_subj[g] == USER_SUBJ) {  // RUMOR mode: the GOSSIP event of P4 (k + lat), hashed now
    const uint64_t gid = d.slot_gid[g], key = d.slot_key[g];
    const uint64_t ev = ((uint64_t)(k + d.lat) << 32) | (3ull << 30) | (uint32_t)(gid >> 32);
    const uint64_t meta = ((uint64_t)(uint32_t)key << 32) | (key >> 32);  // (oldMeta, newMeta) = payload (lo, hi)
    eh += hpair(hpair(ev, meta), (uint32_t)gid);
    return false;
  }
  if (!receipt_matters(d, t, g, k + d.lat)) {  // counted as a record compare in P4, nothing else
    drops++;
    return false;
  }
  return true;
}

__global__ void __launch_bounds__(256) k_gossip_apply(const Dev* __restrict__ dp, uint32_t k) {
  const Dev& d = *dp;
  const uint32_t lane = threadIdx.x & 63u, ntl = *d.ntl, mask = d.BCAP - 1;
  const uint32_t nw = gridDim.x * 4;
  for (uint32_t t0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; t0 < ntl; t0 += nw * 64) {
    const uint32_t ti = t0 + lane;
    uint32_t t = 0, a = 0, b = 0;
    if (ti < ntl) {
      t = d.tlist[ti];
      a = d.rt0[t];
      b = d.rtail[t];
    }
    const bool small = ti < ntl && b - a <= APPLY_LANE;
    // the small targets, a lane each: which entries are routed is kept as a bit per entry, then the wave reserves
    // their places in the routing list with one atomic (a per-entry append would serialise on rc_n)
    uint32_t routed = 0, drops = 0;
    unsigned long long eh = 0;
    if (small) {
      const uint32_t* R = ring(d, t);
      for (uint32_t i = 0; i < b - a; ++i)
        if (apply_entry(d, t, R[(a + i) & mask] & RG_SLOT, k, drops, eh)) routed |= 1u << i;
    }
    uint32_t ri = wave_reserve(d.rc_n, (uint32_t)__popc(routed));
    if (small) {
      const uint32_t* R = ring(d, t);
      for (uint32_t r = routed; r; r &= r - 1, ++ri) {
        const uint32_t p = a + (uint32_t)(__ffs(r) - 1);
        if (ri < d.RCAP)
          d.rc_raw[ri] = ((uint64_t)t << 32) | (R[p & mask] & RG_SLOT);
        else
          set_err(d, E_RECEIPTS);
      }
      apply_target_end(d, t, a, b, drops, eh);
    }
    // the large targets go to a list for k_gossip_apply_big (a wave each, all of them in parallel)
    const bool big = ti < ntl && !small;
    const uint32_t bi = wave_reserve(d.nap, big ? 1u : 0u);
    if (big) d.ap_list[bi] = t;
  }
}

__global__ void __launch_bounds__(256) k_gossip_apply_big(const Dev* __restrict__ dp, uint32_t k) {
  const Dev& d = *dp;
  const uint32_t lane = threadIdx.x & 63u, n = *d.nap, mask = d.BCAP - 1;
  for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w < n; w += gridDim.x * 4) {
    const uint32_t t = d.ap_list[w], a = d.rt0[t], b = d.rtail[t];
    const uint32_t* R = ring(d, t);
    uint32_t dr = 0;
    unsigned long long h = 0;
    for (uint32_t p0 = a; p0 - a < b - a; p0 += 64u * 64u) {  // 64 entries per lane per batch
      unsigned long long rt = 0;
      // the next entry's ring load is issued before this one's holder-table and row accesses (their stores would
      // otherwise keep the compiler from hoisting it)
      uint32_t g = p0 + lane - a < b - a ? R[(p0 + lane) & mask] & RG_SLOT : 0u;
      for (uint32_t it = 0; it < 64; ++it) {
        const uint32_t p = p0 + it * 64u + lane;
        if (p - a >= b - a) break;
        const uint32_t pn = p + 64u;
        const uint32_t gn = it + 1 < 64 && pn - a < b - a ? R[pn & mask] & RG_SLOT : 0u;
        if (apply_entry(d, t, g, k, dr, h)) rt |= 1ull << it;
        g = gn;
      }
      uint32_t rj = wave_reserve(d.rc_n, (uint32_t)__popcll(rt));
      for (; rt; rt &= rt - 1, ++rj) {
        const uint32_t p = p0 + (uint32_t)(__ffsll((long long)rt) - 1) * 64u + lane;
        if (rj < d.RCAP)
          d.rc_raw[rj] = ((uint64_t)t << 32) | (R[p & mask] & RG_SLOT);
        else
          set_err(d, E_RECEIPTS);
      }
    }
    dr = wave_sum(dr);
    h = wave_sum(h);
    if (lane == 0) apply_target_end(d, t, a, b, dr, h);
  }
}

// 9. slots every holder has swept (slot_exp): nobody can send them again. Pass 1 lists them and clears their
// group bits; pass 2 returns each one to its owner shard's free list. Their holder-table entries stay: they predate
// the slot's next gossip, so s_get reads them as never held.
__global__ void k_gossip_expire(Dev d, uint32_t k) {
  const uint32_t nag = d.nagroup[0];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nag * 64u) return;
  const uint32_t q = d.agroup[i >> 6], g = q * 64u + (i & 63u);
  if (!((d.GU[q] >> (g & 63u)) & 1ull)) return;
  if (k - d.slot_ctick[g] > SLIFE) set_err(d, E_SLIFE);  // its 16-bit holder entries could alias (engine.h)
  if (d.slot_exp[g] > k) return;
  const unsigned long long bit = 1ull << (g & 63u);
  atomicAnd(&d.GU[q], ~bit);
  atomicAnd(&d.DM[q], ~bit);
  d.fexp[wave_append(d.nfexp)] = g;
}
__global__ void __launch_bounds__(256) k_gossip_free(Dev d) {
  const uint32_t n = *d.nfexp;
  for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < n; a += gridDim.x * blockDim.x) {
    const uint32_t g = d.fexp[a];
    d.slot_used[g] = 0;
    if (g / d.SPR == d.rank) d.free_list[atomicAdd(d.free_top, 1)] = g;  // back to the owning shard's free list
  }
}

// W > 1: peers' first receipts into this shard's replicated holder state (the owning shard did the membership part)
__global__ void k_unpack_b(Dev d, uint32_t k) {
  const uint32_t p = blockIdx.y;
  if (p == d.rank || (d.xb_rcnt[p] & XCNT_MASK) < 16) return;
  const uint8_t* R = d.xb_recv + (size_t)p * d.XB_PEER;
  const uint32_t nd = ((const uint32_t*)R)[0];
  const uint64_t* V = (const uint64_t*)(R + 16);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nd; i += gridDim.x * blockDim.x) {
    const uint32_t g = (uint32_t)(V[i] >> 32), t = (uint32_t)V[i];
    if (t & XD_EXT) {  // a peer's delayed send keeps the slot (delay_push)
      atomicMax(&d.slot_exp[g], (t & ~XD_EXT) + d.EXPB);
      continue;
    }
    atomicOr(&hrow(d, t)[g >> 6], 1ull << (g & 63u));
    const uint32_t pos = atomicAdd(&d.rtail[t], 1u);
    receipt_mark(d, g, t, k, pos);
    receipt_create(d, g, t, k);
    atomicAdd(&d.held[t], 1u);
    // the ring fill for grow_caps_shard (an atomic only on a new maximum)
    if (d.rfill && pos + 1u - d.rhead[t] > __hip_atomic_load(d.rfill, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(d.rfill, pos + 1u - d.rhead[t]);
  }
}

// the receivers' side of this tick's first receipts, P4 routing and slot recycling
void launch_gossip_apply(const Dev& d, uint32_t k, hipStream_t st) {
  hipLaunchKernelGGL(k_gossip_apply, dim3(2048), dim3(256), 0, st, d.self, k);
  hipLaunchKernelGGL(k_gossip_apply_big, dim3(2048), dim3(256), 0, st, d.self, k);
  launch_receipt_routing(d, st);
  hipLaunchKernelGGL(k_gossip_expire, dim3(cdiv((uint64_t)d.QW * 64, 256)), dim3(256), 0, st, d, k);
  hipLaunchKernelGGL(k_gossip_free, dim3(1024), dim3(256), 0, st, d);
}

void launch_unpack_b(const Dev& d, uint32_t k, hipStream_t st) {
  hipLaunchKernelGGL(k_unpack_b, dim3(64, d.W), dim3(256), 0, st, d, k);
}

}  // namespace swim
