// gossip_send.hip — the gossip data plane, steps 6-7: this tick's sends up to the targets' first receipts, and
// launch_gossip_send, which runs steps 1-7 (gossip_dev.h: the plane's file map and the holder state).
//
// Target-major sends. All senders of one target in a tick are evaluated by the same lane for each 64-slot group:
// the first receipts of the target are OR-ed in a register (no per-receipt atomics for deduplication), the sends are
// counted by popcount, and the target's held bits and receipt ring are updated by the lane that owns them. Loss is
// drawn per message only where the link is lossy (NetworkLinkSettings.evaluateLoss, SEMANTICS.md §2) and only for
// messages that can still be a first receipt. The sends of a pair with a logged contact take the per-send kernels
// (k_gossip_replay, k_gossip_send_slow) after their infectedFrom replay (gossip_replay.h).
#include "gossip_replay.h"

namespace swim {

// the slot of the lowest set bit of b, a word of slot group q
__device__ __forceinline__ uint32_t low_slot(uint32_t q, unsigned long long b) {
  return q * 64u + (uint32_t)(__ffsll((long long)b) - 1);
}

// debugging aid (swim_debug_sends): one counted send into the send log; false once the log is full
__device__ __forceinline__ bool dbg_send_record(const Dev& d, uint32_t k, uint32_t m, uint64_t gid, uint32_t t) {
  const uint32_t di = atomicAdd(d.dbg_send_n, 1u);
  if (di >= d.dbg_send_cap) return false;
  uint32_t* r = d.dbg_send + (size_t)di * 5;
  r[0] = k, r[1] = m, r[2] = (uint32_t)gid, r[3] = (uint32_t)(gid >> 32), r[4] = t;
  return true;
}

// a workgroup of 256's sends into the gossip-message counter: one atomic per workgroup (red: 4 words of LDS)
__device__ __forceinline__ void count_sends(const Dev& d, unsigned long long sends, unsigned long long* red) {
  sends = wave_sum(sends);
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = sends;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long tot = red[0] + red[1] + red[2] + red[3];
    if (tot) atomicAdd(&d.ctr[C_G], tot);
  }
}

// k_gossip_send's operands. A lane's work item (send_item): target t, slot group q, t's held word h of the group, and
// t's senders tin[o, o + ns)
struct SendItem {
  bool act;  // false: a lane past the last item (t = NEVER, no senders)
  uint32_t t, q, o, ns;
  unsigned long long h;
};
// sender p of an item (send_word): ms = m * F + s, its window word of the group split into w (sent here) and wr (the
// gossips that can have t in infectedFrom_m: a logged contact, cin; the pair's RX row bounds them unless it has none)
struct SendWord {
  uint32_t ms, m, s, ci;
  unsigned long long w, wr;
};

// ------------------------------------------------------------------------------------------------------------
// The draws of a send (NetworkEmulator.tryFail, NetworkLinkSettings.evaluateLoss: SEMANTICS.md §2), word-wide for
// k_gossip_send (cand: the bits of sw.w that can still be a first receipt; returns those that are one now) and per
// send for the replayed sends (deliver_one).
//
// The exact path (link delays or emulator counters on the handle) exists in both forms, send_draw_exact and the first
// branch of deliver_one, and the two must stay one rule: a dead target refuses the send before the emulator (nothing
// delivered or counted); the counters need every send's loss outcome, and so does a delayed send to a holder (the
// target may sweep the gossip before it arrives, and then it is a first receipt again: onGossipReq :171-183 at
// arrival); a surviving send with a delay is queued (delay_push: k_gossip_due decides at arrival) and is no receipt
// now. They differ only in the dedup: the word-wide form returns bits its lane owns, the per-send form reads the held
// bit here and wins it by an atomic afterwards.
__device__ __forceinline__ unsigned long long send_draw_exact(const Dev& d, int ep, uint32_t k, const SendItem& it,
                                                              const SendWord& sw, unsigned long long cand) {
  const uint32_t t = it.t, q = it.q, m = sw.m, s = sw.s;
  const unsigned long long w = sw.w;
  if (ep < 0) {
    set_err(d, E_EPOCH);
    return 0;
  }
  if (dead_at(d, t, k)) return 0;
  const uint32_t ls = link_set(d, ep, m, t, k), pct = ls & 0xFFu, di = ls >> 8;
  const unsigned long long drawn = (d.em || di) ? w : cand;
  unsigned long long lostm = 0;
  if (pct >= 100) {
    lostm = drawn;
  } else if (pct > 0) {
    for (unsigned long long b = drawn; b; b &= b - 1) {
      const uint32_t g = low_slot(q, b);
      if (next_int(gossip_loss_word(d, m, k, s, d.slot_gid[g]), 100) < pct) lostm |= 1ull << (g & 63u);
    }
  }
  em_count(d, m, (uint32_t)__popcll(w), (uint32_t)__popcll(lostm & w));
  unsigned long long ok = cand & ~lostm;
  if (di)  // every delivered send that arrives after the next tick is queued
    for (unsigned long long b = w & ~lostm; b; b &= b - 1) {
      const uint32_t g = low_slot(q, b);
      const uint32_t e = gossip_delay(d, di, m, k, s, d.slot_gid[g]);
      if (e) {
        ok &= ~(1ull << (g & 63u));
        delay_push(d, g, t, k + d.lat + e);
      }
    }
  return ok;
}

// the fast path: one loss percent for the word, a draw per candidate only where the link is lossy
__device__ __forceinline__ unsigned long long send_draw_fast(const Dev& d, int ep, uint32_t k, const SendItem& it,
                                                             const SendWord& sw, unsigned long long cand) {
  if (ep < 0) {
    set_err(d, E_EPOCH);
    return 0;
  }
  const uint32_t pct = link_loss(d, ep, sw.m, it.t, k);
  if (pct == 0) return cand;
  unsigned long long ok = 0;
  if (pct < 100)
    for (unsigned long long b = cand; b; b &= b - 1) {
      const uint32_t g = low_slot(it.q, b);
      if (!lost_gossip_pct(d, pct, sw.m, k, sw.s, d.slot_gid[g])) ok |= 1ull << (g & 63u);
    }
  return ok;
}

// one send of the replay / slow paths, after its isInfected check: a first receipt unless t holds g past this tick
// (or received it already this tick: the held bit), subject to the loss draw; the held bit deduplicates by atomics
__device__ __forceinline__ void deliver_one(const Dev& d, uint32_t g, uint32_t m, uint32_t s, uint32_t t, uint32_t k,
                                            uint64_t gid, int ep) {
  if (d.dbg_send) dbg_send_record(d, k, m, gid, t);
  unsigned long long* hw = hrow(d, t) + (g >> 6);
  const unsigned long long bit = 1ull << (g & 63u);
  if (d.dly_on || d.em) {  // the exact path, per send
    if (ep < 0) {
      set_err(d, E_EPOCH);
      return;
    }
    if (dead_at(d, t, k)) return;
    const uint32_t ls = link_set(d, ep, m, t, k), pct = ls & 0xFFu, di = ls >> 8;
    const bool held = (*hw & bit) != 0ull;
    if (held && !d.em && !di) return;
    const bool lost = pct >= 100 || (pct > 0 && next_int(gossip_loss_word(d, m, k, s, gid), 100) < pct);
    em_count(d, m, 1u, lost ? 1u : 0u);
    if (lost) return;
    const uint32_t e = gossip_delay(d, di, m, k, s, gid);
    if (e) {
      delay_push(d, g, t, k + d.lat + e);
      return;
    }
    if (held) return;
  } else {
    if (*hw & bit) return;
    if (lost_gossip_ep(d, ep, m, t, k, s, gid)) return;
  }
  if (atomicOr(hw, bit) & bit) return;
  first_receipt(d, g, t, k);
}

// ------------------------------------------------------------------------------------------------------------
// 6. target-major sends (the fast path). Work item = (target t, active group q); the lanes of a wave take 64
// consecutive items (64 groups of one target when there are that many). For each sender (m, s) of t: its window word
// (sends = popcount), and the first-receipt candidates WB & ~HB[t] (t does not hold them past this tick: the rounds'
// sweeps ran in k_round_apply), each surviving its loss draw. A receipt needs one surviving send from any sender;
// draws of candidates another sender already delivered are skipped (they change nothing). Pairs with a cached contact
// go to k_gossip_replay and pairs whose contact list overflowed to k_gossip_send_slow (isInfected, :247).
// Its body is the list of its steps: send_item, per sender send_word, send_divert and one of the draws above, then
// send_reserve and send_commit.
__device__ __forceinline__ SendItem send_item(const Dev& d, uint64_t i, uint64_t items, uint32_t nag) {
  SendItem it{i < items, NEVER, 0, 0, 0, 0};
  if (it.act) {
    it.t = d.tlist[(uint32_t)(i / nag)];
    it.q = d.agroup[(uint32_t)(i % nag)];
    it.h = hrow(d, it.t)[it.q];
    it.o = d.tin_off[it.t];
    it.ns = d.tin_cnt[it.t];
  }
  return it;
}

__device__ __forceinline__ SendWord send_word(const Dev& d, const SendItem& it, uint32_t p) {
  SendWord sw{0, 0, 0, NEVER, 0, 0};
  if (p < it.ns) {
    sw.ms = d.tin[it.o + p];
    sw.m = sw.ms / d.F;
    sw.s = sw.ms - sw.m * d.F;
    sw.w = wrow(d, sw.m)[it.q];
    if (sw.w) sw.ci = d.cin[sw.ms];
    if (sw.ci != NEVER) {
      const uint32_t r = sw.ci == CIN_SLOW ? RX_ALL : d.crow[sw.ms];
      sw.wr = r == RX_ALL ? sw.w : sw.w & d.RX[(size_t)r * d.QW + it.q];
      sw.w &= ~sw.wr;
    }
  }
  return sw;
}

// wr onto the replay list (k_gossip_replay), or the slow list past the contact cache (k_gossip_send_slow: it replays
// from a full scan of both round logs): (slot, ms) per bit, one atomic per wave and list (every lane of the wave calls)
__device__ __forceinline__ void send_divert(const Dev& d, uint32_t q, const SendWord& sw, uint32_t& st_bits) {
  if (!__ballot(sw.wr != 0ull)) return;
  const bool slow = sw.ci == CIN_SLOW;
  const uint32_t c = (uint32_t)__popcll(sw.wr);
  if (d.exp & EXP_GOSSIP_WORK) st_bits += c;
  fb_add(d, slow ? FB_CEV_SLOW : FB_REPLAY, c);
  uint32_t jr = wave_reserve(d.rp_n, slow ? 0u : c), js = wave_reserve(d.slow_n, slow ? c : 0u);
  uint32_t j = slow ? js : jr;
  for (unsigned long long b = sw.wr; b; b &= b - 1, ++j) {
    const uint64_t v = ((uint64_t)low_slot(q, b) << 32) | sw.ms;
    if (j < (slow ? d.SLOWCAP : d.RPCAP))
      (slow ? d.slow : d.rp)[j] = v;
    else
      set_err(d, E_CONTACTS);
  }
}

// the targets' receipt rings: c entries for this lane, one reservation (atomic on rtail) per run of lanes with the
// same target; returns the lane's first ring position
__device__ __forceinline__ uint32_t send_reserve(const Dev& d, const SendItem& it, uint32_t c, uint32_t lane) {
  const uint32_t incl = wave_incl_scan(c, lane);
  const uint32_t tp = __shfl_up(it.t, 1);
  const unsigned long long heads = __ballot(lane == 0 || tp != it.t);
  const uint32_t head = 63u - (uint32_t)__clzll(heads & ((2ull << lane) - 1ull));  // this lane's run head
  const unsigned long long above = heads & ~((2ull << lane) - 1ull);
  const uint32_t last = above ? (uint32_t)(__ffsll((long long)above) - 2) : 63u;  // the run's last lane
  const uint32_t excl_head = __shfl(incl, (int)head) - __shfl(c, (int)head);
  const uint32_t run_total = __shfl(incl, (int)last) - excl_head;
  uint32_t base = 0;
  if (lane == head && it.act && run_total) base = atomicAdd(&d.rtail[it.t], run_total);
  return __shfl(base, (int)head) + (incl - c - excl_head);
}

// the item's first receipts nb (c of them, ring positions from base): what first_receipt does per send, for the word
__device__ __forceinline__ void send_commit(const Dev& d, uint32_t k, const SendItem& it, unsigned long long nb,
                                            uint32_t base, uint32_t c) {
  const uint32_t t = it.t, q = it.q;
  hrow(d, t)[q] = it.h | nb;  // the lane owns (t, q) in this kernel: later receipts of the tick see it held
  if (nb & d.DM[q]) d.dead_rx[t] = k + d.lat;  // a DEAD membership record arrives in P4 of k + lat
  // the receipts' ring entries (receipt_mark, with the loop-invariant parts hoisted)
  const uint32_t tag = rounds_before(d, t, k + d.lat) << 22, mask = d.BCAP - 1;
  uint32_t* Rt = ring(d, t);
  if (base + c - d.rhead[t] > d.BCAP) set_err(d, E_RING);
  uint32_t pos = base;
  for (unsigned long long b = nb; b; b &= b - 1, ++pos) Rt[pos & mask] = low_slot(q, b) | tag;
  if (d.W > 1) {  // replicated on the other shards from exchange B: one reservation for the word
    uint32_t xi = atomicAdd(d.xd_n, c);
    for (unsigned long long b = nb; b; b &= b - 1, ++xi) xd_put(d, xi, low_slot(q, b), t);
  }
}

// SWIM_EXP & 4, once per launch: the work units, (target, group) items and their sender words
__device__ __forceinline__ void send_work_units(const Dev& d, uint32_t ntl, uint32_t nag) {
  uint64_t pairs = 0;
  for (uint32_t i = 0; i < ntl; ++i) pairs += d.tin_cnt[d.tlist[i]];
  atomicAdd(&d.ctr[C_XU], (unsigned long long)ntl * nag);
  atomicAdd(&d.ctr[C_XU + 1], (unsigned long long)pairs * nag);
}

__global__ void __launch_bounds__(256, 8) k_gossip_send(const Dev* __restrict__ dp, uint32_t k) {
  const Dev& d = *dp;
  __shared__ unsigned long long red[4];
  const uint32_t nag = d.nagroup[0], ntl = *d.ntl;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t items = (uint64_t)ntl * nag;
  const int ep = epoch_at(d, k);
  const bool work = d.exp & EXP_GOSSIP_WORK;
  if (work && blockIdx.x == 0 && threadIdx.x == 0) send_work_units(d, ntl, nag);
  unsigned long long sends = 0;
  uint32_t st[4] = {0, 0, 0, 0};  // SWIM_EXP & 4: items with window bits, contact-path bits, -, candidates
  for (uint64_t i0 = ((uint64_t)blockIdx.x * 4 + wave) * 64; i0 < items; i0 += (uint64_t)gridDim.x * 256) {
    const SendItem it = send_item(d, i0 + lane, items, nag);
    unsigned long long nb = 0;  // the item's first receipts so far
    // the senders loop is wave-uniform (lanes past their own target's senders idle), so the replay lists take one
    // atomic per wave
    const uint32_t nsw = wave_max(it.ns);
    for (uint32_t p = 0; p < nsw; ++p) {
      const SendWord sw = send_word(d, it, p);
      if ((sw.w | sw.wr) && work) st[0]++;
      send_divert(d, it.q, sw, st[1]);
      if (!sw.w) continue;
      sends += __popcll(sw.w);
      if (d.dbg_send)  // every counted send
        for (unsigned long long b = sw.w; b; b &= b - 1)
          if (!dbg_send_record(d, k, sw.m, d.slot_gid[low_slot(it.q, b)], it.t)) break;
      const unsigned long long cand = sw.w & ~it.h & ~nb;
      if (d.dly_on || d.em) {
        nb |= send_draw_exact(d, ep, k, it, sw, cand);
        continue;
      }
      if (!cand) continue;
      if (work) st[3] += (uint32_t)__popcll(cand);
      nb |= send_draw_fast(d, ep, k, it, sw, cand);
    }
    const uint32_t c = (uint32_t)__popcll(nb);
    const uint32_t base = send_reserve(d, it, c, lane);
    if (it.act && nb) send_commit(d, k, it, nb, base, c);
  }
  if (work)
    for (int q2 = 0; q2 < 4; ++q2)
      if (st[q2]) atomicAdd(&d.ctr[8 + q2], (unsigned long long)st[q2]);
  count_sends(d, sends, red);
}

// 7a. sends of pairs with a cached contact, one thread per (slot, sender, target): the isInfected replay runs only
// where the contact can matter (t -> m at or after m's incarnation start and after the gossip existed), then the send
__global__ void __launch_bounds__(256, 8) k_gossip_replay(const Dev* __restrict__ dp, uint32_t k) {
  const Dev& d = *dp;
  __shared__ unsigned long long red[4];
  const uint32_t n = min(*d.rp_n, d.RPCAP);
  const int ep = epoch_at(d, k);
  unsigned long long sends = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint64_t v = d.rp[i];
    const uint32_t g = (uint32_t)(v >> 32), ms = (uint32_t)v, m = ms / d.F, s = ms % d.F;
    const uint32_t t = d.T[ms], c = s_ctick(s_get(d, g, m, k + d.lat)), ci = d.cin[ms];  // m holds g: a current entry
    const uint64_t gid = d.slot_gid[g];
    const bool maybe = ci >= d.slot_ctick[g] && ci + d.lat + dmax(d) >= c;
    if (d.exp & EXP_GOSSIP_WORK) {  // timing experiment: replay items that reach the contact replay, and those it blocks
      if (maybe) atomicAdd(&d.ctr[10], 1ull);
    }
    if (maybe && blocked_pair_cached(d, m, t, g, gid, k, c, d.cev + (size_t)ms * CEVW)) {
      if (d.exp & EXP_GOSSIP_WORK) atomicAdd(&d.ctr[12], 1ull);
      continue;
    }
    sends++;
    deliver_one(d, g, m, s, t, k, gid, ep);
  }
  count_sends(d, sends, red);
}

// 7b. sends whose pair had more contact events than the cache holds (small clusters): full log scan + replay
__global__ void __launch_bounds__(64) k_gossip_send_slow(const Dev* __restrict__ dp, uint32_t k) {
  const Dev& d = *dp;
  const uint32_t n = min(*d.slow_n, d.SLOWCAP);
  const int ep = epoch_at(d, k);
  unsigned long long sends = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint64_t v = d.slow[i];
    const uint32_t g = (uint32_t)(v >> 32), ms = (uint32_t)v, m = ms / d.F, s = ms % d.F;
    const uint32_t t = d.T[ms], c = s_ctick(s_get(d, g, m, k + d.lat));
    const uint64_t gid = d.slot_gid[g];
    if (blocked_pair(d, m, t, g, gid, k, c)) continue;  // isInfected (:247)
    sends++;
    deliver_one(d, g, m, s, t, k, gid, ep);
  }
  if (sends) atomicAdd(&d.ctr[C_G], sends);
}

// 7c. delayed first-receipt candidates due in P4 of k + lat (delay_push). Targets without senders this tick join the
// target list first (their ring end before this tick's receipts: k_gossip_apply takes [rt0, rtail)), then each
// candidate is a first receipt unless the target holds the gossip by now or is dead then.
__global__ void k_gossip_due_mark(Dev d, uint32_t k) {
  const uint32_t b = (k + d.lat) % (d.EMAX + 2u), n = min(d.dq_n[b], d.DQCAP);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t t = (uint32_t)d.dq[(size_t)b * d.DQCAP + i];
    if (dead_at(d, t, k + d.lat) || d.tin_cnt[t]) continue;
    if (atomicExch(&d.dmark[t], k + 1u) != k + 1u) {
      d.rt0[t] = d.rtail[t];
      d.tlist[atomicAdd(d.ntl, 1u)] = t;
    }
  }
}
__global__ void k_gossip_due(Dev d, uint32_t k) {
  const uint32_t b = (k + d.lat) % (d.EMAX + 2u), n = min(d.dq_n[b], d.DQCAP);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint64_t v = d.dq[(size_t)b * d.DQCAP + i];
    const uint32_t g = (uint32_t)(v >> 32), t = (uint32_t)v;
    if (dead_at(d, t, k + d.lat)) continue;
    const unsigned long long bit = 1ull << (g & 63u);
    if (atomicOr(hrow(d, t) + (g >> 6), bit) & bit) continue;  // held, or made a receipt by another delivery
    first_receipt(d, g, t, k);
  }
}
__global__ void k_dq_reset(Dev d, uint32_t k) { d.dq_n[(k + d.lat) % (d.EMAX + 2u)] = 0; }

constexpr uint32_t SEND_GRID = 4096;  // 16 blocks per CU, grid-stride

// the sends of this tick and the holder-state changes they need, up to the first receipts (the sharded tick
// exchanges them before launch_gossip_apply)
void launch_gossip_send(const Dev& d, uint32_t k, hipStream_t st, const TickEvents* prof,
                        const GossipChunks* chunks) {
  hipLaunchKernelGGL(k_gossip_groups, dim3(1), dim3(1024), 0, st, d);
  hipLaunchKernelGGL(k_round_plan, dim3(cdiv(d.N, 256)), dim3(256), 0, st, d, k);
  launch_scan(d.tin_cnt, d.tin_off, d.scan_part, d.N, st);
  hipLaunchKernelGGL(k_tin_scatter, dim3(cdiv(d.N, 256)), dim3(256), 0, st, d);
  {  // LDS rows sized by the slot table (the active span never exceeds QW words)
    // (chunks: the known-answer tests' sizes, engine.h GossipChunks)
    const uint32_t cw = chunks && chunks->cw ? chunks->cw : std::min<uint32_t>(RCS, d.QW);
    const uint32_t cb = chunks && chunks->cb ? chunks->cb : std::min<uint32_t>(RCW, d.QW);
    hipLaunchKernelGGL(k_round_apply_w, dim3(4096), dim3(256), 4 * 2 * 8 * cw, st, d.self, k, cw);
    hipLaunchKernelGGL(k_round_apply_b, dim3(2048), dim3(256), 2 * 8 * cb, st, d.self, k, cb, cw);
  }
  hipLaunchKernelGGL(k_gossip_contacts, dim3(2048), dim3(256), 0, st, d, k);
  hipLaunchKernelGGL(k_contact_cache, dim3(1024), dim3(256), 0, st, d.self, k);
  {
    const uint32_t cx = chunks && chunks->cx ? chunks->cx : std::min<uint32_t>(RXW, d.QW);
    hipLaunchKernelGGL(k_rx_build, dim3(512), dim3(256), 8 * cx, st, d.self, cx);
  }
  if (prof && prof->all) hipEventRecord((hipEvent_t)prof->ev[4], st);
  hipLaunchKernelGGL(k_gossip_send, dim3(SEND_GRID), dim3(256), 0, st, d.self, k);
  hipLaunchKernelGGL(k_gossip_send_slow, dim3(64), dim3(64), 0, st, d.self, k);  // rare; ~14 KB of stack per lane
  hipLaunchKernelGGL(k_gossip_replay, dim3(2048), dim3(256), 0, st, d.self, k);
  if (d.dly_on) {
    hipLaunchKernelGGL(k_gossip_due_mark, dim3(256), dim3(256), 0, st, d, k);
    hipLaunchKernelGGL(k_gossip_due, dim3(256), dim3(256), 0, st, d, k);
    hipLaunchKernelGGL(k_dq_reset, dim3(1), dim3(1), 0, st, d, k);
  }
  if (prof && prof->all) hipEventRecord((hipEvent_t)prof->ev[5], st);
}

}  // namespace swim
