// gossip_replay.h — infectedFrom without storing it (selectGossipsToSend's isInfected check, :247). The reference
// keeps a set per (holder, gossip); here `y ∈ infectedFrom_x(g)` is recomputed only for pairs with a logged contact.
// Slots are recycled at a bound after their latest creation or receipt by which every holder has swept them
// (slot_exp), so no holder count is kept. gossip_contacts.hip gathers the pairs' contact events; gossip_send.hip
// replays them per gossip.
//
// `y ∈ infectedFrom_x(g)` at x's round at tick tau holds iff y delivered g to x by
// a send in one of y's logged rounds t2 with c_x <= t2 + lat <= tau, where c_x is the creation tick of x's current
// state for g. Whether such a send was delivered depends, one level down, on whether x had delivered g to y earlier
// (then y skips x), and so on. The dependency only runs over the contact events between the pair (x's rounds that
// targeted y, y's rounds that targeted x). Those are replayed in tick order as a small dynamic program.
#pragma once
#include "gossip_dev.h"

namespace swim {

// pct: NetworkEmulator's loss percent of the send (link_loss at its tick: 100 for a dead receiver or a blocked link),
// rb: the sender's gossip rounds before its tick (rounds_before); both independent of the gossip, so they are evaluated
// once per pair (k_contact_cache) instead of once per replayed gossip
struct Contact {
  uint32_t tick, slot, spread, dir;  // dir 0: y -> x, 1: x -> y
  uint32_t pct, rb;
};

// The pair's cache record (Dev::cev, CEVW words: engine.h): the event count (CEV + 1: overflowed), oldest[2], the
// latest y -> x contact (contact_cache writes these four), then three words per event: its tick; slot (8 bits: a
// target slot, below gossip_fanout <= 8) | dir (1 bit) << 8 | pct (7 bits: make_contact caps it at 100) << 9 | spread
// (16 bits: swim_create bounds spreadMax below 248) << 16; and rb.
__device__ __forceinline__ void cev_put(uint32_t* rec, uint32_t j, const Contact& c) {
  uint32_t* e = rec + 4 + 3 * j;
  e[0] = c.tick;
  e[1] = c.slot | (c.dir << 8) | (c.pct << 9) | (c.spread << 16);
  e[2] = c.rb;
}
__device__ __forceinline__ Contact cev_get(const uint32_t* rec, uint32_t j) {
  const uint32_t* e = rec + 4 + 3 * j;
  const uint32_t w = e[1];
  return Contact{e[0], w & 0xFFu, w >> 16, (w >> 8) & 1u, (w >> 9) & 0x7Fu, e[2]};
}

// the pair-level parts of a contact event: sender snd -> receiver rcv at tick t2
__device__ __forceinline__ Contact make_contact(const Dev& d, uint32_t t2, uint32_t s2, uint32_t spread, uint32_t dir,
                                                uint32_t snd, uint32_t rcv) {
  const int ep = epoch_at(d, t2);
  uint32_t pct = 100;
  if (ep < 0)
    set_err(d, E_EPOCH);  // (lost_gossip_ep's answer: the send fails)
  else
    pct = link_loss(d, ep, snd, rcv, t2);
  return Contact{t2, s2, spread, dir, pct, rounds_before(d, snd, t2)};
}

// lost_gossip_ep with the link's loss percent already known (Contact.pct, or looked up once per sender word)
__device__ __forceinline__ bool lost_gossip_pct(const Dev& d, uint32_t pct, uint32_t src, uint32_t k, uint32_t slot,
                                                uint64_t gid) {
  if (pct == 0) return false;
  if (pct >= 100) return true;
  const u32x4 r = philox(src, k ^ ((slot >> 2) << 31), (uint32_t)(gid >> 32), (uint32_t)gid, d.seed_lo ^ SALT_LOSS_GOSSIP,
                         d.seed_hi);
  return next_int(pick(r, slot & 3), 100) < pct;
}

// Was x's incarnation of a gossip created at tick cs swept (sweepGossips :283-308) in one of x's rounds at ticks
// [cs, t)? The window check alone is not enough: the spread is recomputed from the gossip list every round, so a
// list that shrinks (members removed during a partition) and grows back reopens the window of a gossip already swept.
// The ring holds every round in that range: the window at t bounds t - cs to ~spread rounds, LOGW >= 4 (spread + 2).
// The ring is walked from the newest round back to cs (ring order is tick order), so the cost is the rounds since cs.
// While x's spread has not changed since cs (spchg: tick of x's latest round whose spread differs from the round
// before), the sweep condition is monotone in the round, so only the latest round before t needs a check.
__device__ bool swept_before(const Dev& d, uint32_t x, uint32_t cs, uint32_t t) {
  const uint32_t infP = rounds_before(d, x, cs);
  const uint32_t pos = d.log_pos[x], n = min(pos, d.LOGW);
  const bool steady = d.spchg[x] <= cs;
  for (uint32_t e = 1; e <= n; ++e) {
    const size_t li = (size_t)x * d.LOGW + ((pos - e) & (d.LOGW - 1u));  // LOGW is a power of two
    const uint32_t tr = d.log_tick[li];
    if (tr == NEVER || tr >= t) continue;
    if (tr < cs) break;
    if (rounds_before(d, x, tr) > infP + sweep_after(d.log_spread[li])) return true;
    if (steady) break;
  }
  return false;
}

// The replay over the sorted contact events of the pair (x, y) for gossip g (see the head of this file).
// oldest[0]: oldest tick in y's log, oldest[1]: in x's log (0 if that ring never wrapped).
template <uint32_t CM>
__device__ __forceinline__ bool replay_pair(const Dev& d, uint32_t x, uint32_t y, uint32_t g, uint64_t gid,
                                            uint32_t tau, uint32_t cx, const Contact* ev, uint32_t n,
                                            const uint32_t* oldest) {
  const uint32_t lat = d.lat;
  // Find which deliveries can matter: into x from cx on (the answer), and into a sender from its incarnation start
  // for every relevant event (its isInfected check). The fixpoint runs over at most CM events. The ring must cover
  // those ranges.
  uint32_t lo_in[2] = {cx, NEVER};  // [0]: deliveries into x, [1]: deliveries into y
  uint32_t cinc[CM];
  uint8_t swc[CM];  // swept_before of event i's sender: 0 not computed yet, 1 no, 2 yes (both loops ask)
  for (uint32_t i = 0; i < n; ++i) {
    cinc[i] = NEVER - 1;  // not computed yet
    swc[i] = 0;
  }
  auto swept = [&](uint32_t i, uint32_t snd, uint32_t cs) {
    if (!swc[i]) swc[i] = swept_before(d, snd, cs, ev[i].tick) ? 2 : 1;
    return swc[i] == 2;
  };
  for (int pass = 0; pass < 8; ++pass) {
    bool changed = false;
    for (int i = (int)n - 1; i >= 0; --i) {
      const Contact& c = ev[i];
      uint32_t rin = c.dir == 0 ? 0 : 1;  // receiver index into lo_in
      if (lo_in[rin] == NEVER || c.tick + lat + dmax(d) < lo_in[rin]) continue;
      if (d.dly_on && gossip_arrival(d, c.dir == 0 ? y : x, c.dir == 0 ? x : y, c.tick, c.slot, gid) < lo_in[rin]) continue;
      if (cinc[i] == NEVER - 1) cinc[i] = inc_at(d, c.dir == 0 ? y : x, g, gid, c.tick, tau + lat);
      uint32_t cs = cinc[i];
      uint32_t snd = c.dir == 0 ? y : x;
      if (cs == NEVER || rounds_before(d, snd, cs) + c.spread < c.rb) continue;
      if (swept((uint32_t)i, snd, cs)) continue;
      uint32_t sin = 1 - rin;
      if (lo_in[sin] == NEVER || cs < lo_in[sin]) {
        lo_in[sin] = cs;
        changed = true;
      }
    }
    if (!changed) break;
  }
  // deliveries into x come from y's log (oldest[0]); into y from x's log (oldest[1])
  // (oldest 0: that ring never wrapped, so it holds every round since tick 0; a delayed send arrives up to dmax
  // ticks later, so the log must reach that much further back)
  if ((lo_in[0] != NEVER && oldest[0] && lo_in[0] < oldest[0] + lat + dmax(d)) ||
      (lo_in[1] != NEVER && oldest[1] && lo_in[1] < oldest[1] + lat + dmax(d))) {
    if (atomicOr(d.err, E_LOGWIN) == 0) {
      d.err[1] = tau;
      d.err[2] = lo_in[0];
      d.err[3] = lo_in[1];
      d.err[4] = oldest[0];
      d.err[5] = oldest[1];
    }
  }
  uint32_t del[2][CM];  // arrival ticks of the delivered sends, per direction
  uint32_t nd[2] = {0, 0};
  // the answer reads only the deliveries y -> x; an x -> y delivery matters only by blocking a later y -> x send, so
  // the events after the last y -> x one change nothing
  uint32_t nlast = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (ev[i].dir == 0) nlast = i + 1;
  for (uint32_t i = 0; i < nlast; ++i) {
    const Contact& c = ev[i];
    uint32_t snd = c.dir == 0 ? y : x;
    // the sender held g at that round (its incarnation then), inside its spread window (selectGossipsToSend :246)
    uint32_t cs = cinc[i] != NEVER - 1 ? cinc[i] : inc_at(d, snd, g, gid, c.tick, tau + lat);
    if (cs == NEVER) continue;
    if (rounds_before(d, snd, cs) + c.spread < c.rb) continue;
    if (swept(i, snd, cs)) continue;  // x no longer held it
    // the receiver delivered g to the sender during that incarnation: infectedFrom (isInfected :247)
    uint32_t od = 1 - c.dir;  // opposite direction
    bool blocked = false;
    for (uint32_t q = 0; q < nd[od] && !blocked; ++q) blocked = del[od][q] >= cs && del[od][q] <= c.tick;
    if (blocked) continue;
    const uint32_t rcv = c.dir == 0 ? x : y;
    if (lost_gossip_pct(d, c.pct, snd, c.tick, c.slot, gid)) continue;
    const uint32_t at = d.dly_on ? gossip_arrival(d, snd, rcv, c.tick, c.slot, gid) : c.tick + lat;
    // a delivery depends only on earlier events: the first y -> x one inside [cx, tau] is the answer
    if (c.dir == 0 && at >= cx && at <= tau) return true;
    del[c.dir][nd[c.dir]++] = at;
  }
  for (uint32_t q = 0; q < nd[0]; ++q)
    if (del[0][q] >= cx && del[0][q] <= tau) return true;
  return false;
}

// contact events of the pair (x, y) in both logs up to tick tau - lat, in tick order; n = CM + 1 on overflow
template <uint32_t CM>
__device__ __forceinline__ uint32_t collect_contacts(const Dev& d, uint32_t x, uint32_t y, uint32_t tau, uint32_t born,
                                                     Contact* ev, uint32_t* oldest) {
  uint32_t n = 0;
  for (int side = 0; side < 2; ++side) {
    uint32_t from = side == 0 ? y : x, to = side == 0 ? x : y;
    bool wrapped = d.log_pos[from] > d.LOGW;
    uint32_t old = NEVER;
    for (uint32_t e = 0; e < d.LOGW; ++e) {
      size_t li = (size_t)from * d.LOGW + e;
      uint32_t t2 = d.log_tick[li];
      if (t2 == NEVER) continue;
      if (t2 < old) old = t2;
      if (t2 + d.lat > tau || t2 < born) continue;
      uint32_t cnt = d.log_cnt[li];
      for (uint32_t s2 = 0; s2 < cnt; ++s2)
        if (d.log_tg[li * d.F + s2] == to) {
          if (n == CM) return CM + 1;
          uint32_t j = n++;
          while (j > 0 && ev[j - 1].tick > t2) {
            ev[j] = ev[j - 1];
            --j;
          }
          ev[j] = make_contact(d, t2, s2, d.log_spread[li], (uint32_t)side, from, to);
        }
    }
    oldest[side] = wrapped ? old : 0;
  }
  return n;
}

// isInfected replay from a full scan of both logs (used when the cached contact list of the pair overflowed)
__device__ __noinline__ bool blocked_pair(const Dev& d, uint32_t x, uint32_t y, uint32_t g, uint64_t gid,
                                          uint32_t tau, uint32_t cx) {
  constexpr uint32_t CMAX = 512;  // contact events between one pair inside the log window (small clusters: many)
  Contact ev[CMAX];
  uint32_t oldest[2];
  const uint32_t n = collect_contacts<CMAX>(d, x, y, tau, d.slot_ctick[g], ev, oldest);
  if (n > CMAX) {
    atomicOr(d.err, E_CONTACTS);
    return false;
  }
  return replay_pair<CMAX>(d, x, y, g, gid, tau, cx, ev, n, oldest);
}

// isInfected replay from the pair's contact list cached by k_contact_cache (gossip-independent; the creation
// tick of g filters it: nobody could send g before it existed)
__device__ __forceinline__ bool blocked_pair_cached(const Dev& d, uint32_t x, uint32_t y, uint32_t g, uint64_t gid,
                                                    uint32_t tau, uint32_t cx, const uint32_t* rec) {
  const uint32_t nall = rec[0];  // <= CEV: overflowed pairs go to k_gossip_send_slow
  const uint32_t born = d.slot_ctick[g];
  // only a delivery y -> x at or after x's incarnation start cx can put y in infectedFrom_x (most cached contacts
  // are older than the gossip)
  bool relevant = false;
  for (uint32_t i = 0; i < nall; ++i) {
    const Contact c = cev_get(rec, i);
    relevant |= c.dir == 0 && c.tick >= born && c.tick + d.lat + dmax(d) >= cx;
  }
  if (!relevant) return false;
  // y never held g up to now: no send y -> x carried it (inc_at of every y -> x event is NEVER)
  if (!s_ever(s_get(d, g, y, tau + d.lat))) return false;
  Contact ev[CEV];
  uint32_t n = 0;
  for (uint32_t i = 0; i < nall; ++i) {
    const Contact c = cev_get(rec, i);
    if (c.tick >= born) ev[n++] = c;
  }
  const uint32_t oldest[2] = {rec[1], rec[2]};
  return replay_pair<CEV>(d, x, y, g, gid, tau, cx, ev, n, oldest);
}

}  // namespace swim
