// gossip_contacts.hip — the gossip data plane, step 5: which of this tick's (sender, target) pairs have a logged
// contact inside the look-back window, those pairs' contact caches, and the RX rows that bound what the send replays
// (gossip_replay.h: what a contact is and why it is replayed).
#include "gossip_replay.h"

namespace swim {

// 5. contact lists: did target t = T[m][s] choose m in a logged round inside the look-back window? If so, cache the
// pair's contact events in both directions (independent of the gossip) for blocked_pair_cached. Eight lanes per
// (sender, target) pair of this shard's targets, eight pairs per wave: the lanes read consecutive entries of the
// target's round log for the sender (a wave per target walked its senders one after another, ~12 targets per wave at
// C3 with membership evolution; a lane per pair made every load touch 64 lines).
__global__ void __launch_bounds__(256) k_gossip_contacts(Dev d, uint32_t k) {
  __shared__ uint32_t sh[5];
  const uint32_t np = d.tin_off[d.N - 1] + d.tin_cnt[d.N - 1];  // this tick's (sender, target) pairs, by target
  const uint32_t sub = threadIdx.x & 7u;
  for (uint32_t j0 = blockIdx.x * 32; j0 < np; j0 += gridDim.x * 32) {  // block-uniform trip count (block_reserve)
    const uint32_t j = j0 + (threadIdx.x >> 3);
    uint32_t i = 0;
    bool hit = false;
    if (j < np) {
      i = d.tin[j];
      const uint32_t m = i / d.F, t = d.T[i];
      const uint32_t pos = d.log_pos[t], nlog = min(pos, d.LOGW);
      // Only a contact t -> m that arrived after m's window horizon can put t in infectedFrom_m (contact_cache): t's
      // rounds since then, newest first. t logs at most one round per gossip interval, so they are its last R entries.
      const int64_t cut = (int64_t)k - (int64_t)(d.tspread[m] + 1u) * d.gossip_t - d.lat - dmax(d);
      const uint32_t R = min(nlog, d.tspread[m] + 2u + (d.lat + dmax(d) + d.gossip_t - 1u) / d.gossip_t);
      for (uint32_t e = sub; e < R; e += 8) {
        const size_t lo = (size_t)t * d.LOGW + ((pos - 1u - e) & (d.LOGW - 1u));
        const uint32_t t2 = d.log_tick[lo];
        if (t2 == NEVER || t2 >= k || (int64_t)t2 <= cut) continue;
        const uint32_t n = d.log_cnt[lo];
        for (uint32_t s2 = 0; s2 < n; ++s2) hit |= d.log_tg[lo * d.F + s2] == m;
      }
    }
    // the pair's eight lanes
    uint32_t h = hit ? 1u : 0u;
    h |= __shfl_xor(h, 1);
    h |= __shfl_xor(h, 2);
    h |= __shfl_xor(h, 4);
    const bool lead = j < np && sub == 0;
    if (lead) {
      d.tcontact[i] = h;
      d.cin[i] = NEVER;
    }
    const uint32_t c = block_reserve(d.ncfl, lead && h ? 1u : 0u, sh);
    if (lead && h) d.cfl[c] = i;  // its contact events are cached by k_contact_cache
  }
}

// The pair's contact events (collect_contacts for x = m, y = t), gathered by one wave: lanes test 64 log entries of
// one side at a time, a wave prefix sum places the hits, and lane 0 orders them by (tick, side, target slot) as the
// serial insertion does. n = CEV + 1 on overflow.
__device__ uint32_t collect_contacts_wave(const Dev& d, uint32_t m, uint32_t t, uint32_t k, uint32_t lane, Contact* ev,
                                          uint32_t* oldest) {
  uint32_t n = 0;
  for (uint32_t side = 0; side < 2; ++side) {
    const uint32_t from = side == 0 ? t : m, to = side == 0 ? m : t;
    uint32_t old = NEVER;
    for (uint32_t e0 = 0; e0 < d.LOGW; e0 += 64) {
      const uint32_t e = e0 + lane;
      uint32_t hits = 0, t2 = NEVER, sp = 0;
      if (e < d.LOGW) {
        const size_t li = (size_t)from * d.LOGW + e;
        t2 = d.log_tick[li];
        if (t2 != NEVER) {
          old = min(old, t2);
          if (t2 + d.lat <= k) {
            const uint32_t cnt = d.log_cnt[li];
            for (uint32_t s2 = 0; s2 < cnt; ++s2) hits |= (d.log_tg[li * d.F + s2] == to ? 1u : 0u) << s2;
            if (hits) sp = d.log_spread[li];
          }
        }
      }
      const uint32_t c = __popc(hits), incl = wave_incl_scan(c, lane);
      const uint32_t tot = __shfl(incl, 63);
      if (n <= CEV && n + tot <= CEV)
        for (uint32_t j = n + incl - c; hits; hits &= hits - 1, ++j)
          ev[j] = make_contact(d, t2, (uint32_t)(__ffs(hits) - 1), sp, side, from, to);
      n = min(n + tot, CEV + 1u);
    }
    old = wave_min(old);
    oldest[side] = d.log_pos[from] > d.LOGW ? old : 0u;
  }
  grp_sync<false>();  // the lanes' LDS writes, before lane 0 orders them
  if (lane == 0 && n <= CEV)
    for (uint32_t a = 1; a < n; ++a)  // insertion by (tick, side, slot): the order collect_contacts produces
      for (uint32_t b = a; b > 0; --b) {
        const Contact &p = ev[b - 1], &q = ev[b];
        if (p.tick < q.tick || (p.tick == q.tick && (p.dir < q.dir || (p.dir == q.dir && p.slot <= q.slot)))) break;
        const Contact tmp = ev[b];
        ev[b] = ev[b - 1];
        ev[b - 1] = tmp;
      }
  return n;
}

// lane 0 of the wave that gathered ev (collect_contacts_wave): the pair's cache record and its replay row
__device__ void contact_cache(const Dev& d, uint32_t i, uint32_t m, uint32_t t, uint32_t k, const Contact* ev,
                              uint32_t n, const uint32_t* oldest) {
  uint32_t* rec = d.cev + (size_t)i * CEVW;
  if (n > d.cev_cap) n = CEV + 1;  // SWIM_CAPS: a smaller cache overflows into k_gossip_send_slow
  rec[0] = n;
  rec[1] = oldest[0];
  rec[2] = oldest[1];
  uint32_t last_in = NEVER;  // latest t -> m contact (NEVER: none); overflow is flagged by n alone
  if (n <= CEV)
    for (uint32_t j = 0; j < n; ++j) {
      cev_put(rec, j, ev[j]);
      if (ev[j].dir == 0) last_in = ev[j].tick;  // events are in tick order
    }
  rec[3] = last_in;
  // a gossip inside m's window this round was received after tick k - (spread + 1) * gossip_t, so a contact t -> m
  // that arrived at or before that tick (sent at most lat + dmax ticks earlier) can never put t in infectedFrom_m of
  // any gossip m sends now
  const int64_t horizon = (int64_t)k - (int64_t)(d.tspread[m] + 1u) * d.gossip_t;
  uint32_t ci;
  if (n > CEV)
    ci = CIN_SLOW;
  else
    ci = last_in == NEVER || (int64_t)last_in + d.lat + dmax(d) <= horizon ? NEVER : last_in;
  d.crow[i] = RX_ALL;
  if (ci != NEVER && ci != CIN_SLOW) {
    // Only gossips m received at or before the latest contact t -> m arrived (last_in + lat) can have t in
    // infectedFrom_m. Their infection periods are at most B1 = rounds_before(last_in + lat + 1); the window entries
    // of m's ring with a period above B1 were received later (sorted ring: a suffix) and are sent normally.
    const uint32_t P = d.tperiod[m], B1 = rounds_before(d, m, last_in + d.lat + dmax(d) + 1u);
    const uint32_t* R = ring(d, m);
    const uint32_t w0 = d.rwin[m], tl = d.rseen[m];  // the window as k_round_apply left it for this round
    uint32_t lo = 0, hi = tl - w0;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (rg_period(R[(w0 + mid) & (d.BCAP - 1)], P) <= (int64_t)B1)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo == 0) {
      ci = NEVER;  // every window gossip arrived after the contact: no replay at all
    } else if (lo < tl - w0) {
      const uint32_t r = wave_append(d.nrx);
      if (r < d.CRCAP) {
        d.crow[i] = r;
        d.rxl[3 * r] = i;
        d.rxl[3 * r + 1] = w0;
        d.rxl[3 * r + 2] = w0 + lo;
      } else {
        fb_add(d, FB_RX_ALL);
      }
    }
  }
  d.cin[i] = ci;
}

// the flagged pairs' contact caches, one wave each: its lanes scan the two round logs 64 entries at a time
// (Dev through a pointer: the contacts' loss percents index its epoch table by a per-lane epoch, which a by-value Dev
// would copy to scratch, 2.3 KB per lane)
__global__ void __launch_bounds__(256, 8) k_contact_cache(const Dev* __restrict__ dp, uint32_t k) {
  const Dev& d = *dp;
  __shared__ Contact sev[4][CEV];
  const uint32_t n = *d.ncfl, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t j = blockIdx.x * 4 + wave; j < n; j += gridDim.x * 4) {
    const uint32_t i = d.cfl[j], m = i / d.F, t = d.T[i];
    uint32_t oldest[2];
    const uint32_t ne = collect_contacts_wave(d, m, t, k, lane, sev[wave], oldest);
    if (lane == 0) contact_cache(d, i, m, t, k, sev[wave], ne, oldest);
    grp_sync<false>();  // lane 0 is done with sev before the next pair's lanes write it
  }
}

// the RX rows of this tick's contact pairs: bit g set for the window gossips received no later than the contact (one
// workgroup per row, staged through LDS in chunks of at most RXW words)
// (cx = min(RXW, QW) words of LDS, sized at launch)
__global__ void __launch_bounds__(256) k_rx_build(const Dev* __restrict__ dp, uint32_t cx) {
  const Dev& d = *dp;
  extern __shared__ unsigned long long lr[];
  const uint32_t n = min(*d.nrx, d.CRCAP), span = d.nagroup[1];
  for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
    const uint32_t m = d.rxl[3 * r] / d.F, a = d.rxl[3 * r + 1], b = d.rxl[3 * r + 2];
    const uint32_t* R = ring(d, m);
    unsigned long long* row = d.RX + (size_t)r * d.QW;
    for (uint32_t c0 = 0; c0 < span; c0 += cx) {
      const uint32_t c1 = min(span, c0 + cx);
      for (uint32_t j = threadIdx.x; j < c1 - c0; j += blockDim.x) lr[j] = 0ull;
      __syncthreads();
      ring_walk(R, d.BCAP - 1, a, b, threadIdx.x, blockDim.x, [&](uint32_t g) {
        const uint32_t q = g >> 6;
        if (q >= c0 && q < c1) atomicOr(&lr[q - c0], 1ull << (g & 63u));
      });
      __syncthreads();
      for (uint32_t j = threadIdx.x; j < c1 - c0; j += blockDim.x) row[c0 + j] = lr[j];
      __syncthreads();
    }
  }
}

}  // namespace swim
