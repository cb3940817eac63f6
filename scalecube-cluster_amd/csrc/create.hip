// create.hip — swim_create: swim_config, the shard spec and the environment become the Dev constants (no GPU needed),
// the allocation table makes and fills every device buffer, and the rest of the initial state follows.
#include "handle.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace swim;

namespace swim {

// NetworkLinkSettings.evaluateDelay (:64-74) quantised to ticks (SEMANTICS.md §2): thresholds on the 32-bit delay draw
// x, the extra ticks are the number of thresholds x reaches. false: a delay of 256 ticks or more is reachable.
bool delay_table(uint32_t D, uint32_t T, std::vector<uint32_t>* out) {
  out->clear();
  if (D == 0) return true;
  for (uint32_t j = 1; j <= 256; ++j) {
    const double th = std::ceil((1.0 - std::exp(-(double)j * (double)T / (double)D)) * 4294967296.0);
    if (th > 4294967295.0) return true;
    if (j == 256) return false;
    out->push_back((uint32_t)th);
  }
  return true;
}

bool to_ticks(uint32_t ms, uint32_t tick, uint32_t* out) {
  if (tick == 0 || ms % tick) return false;
  *out = ms / tick;
  return true;
}

// SWIM_CAPS="trk=1,ulog=2,creq=1,cwmax=1,cev=1,mq=1,sort=2,..." (include/swimhip_debug.h), parsed once at create: lowers
// the fast structures' capacities in d (already at their defaults); rx= and rp= size allocations
static void parse_caps(const char* caps, Dev& d, uint32_t* rx_cap, uint32_t* rp_cap, uint32_t* rb_thr, uint32_t* rb_int) {
  std::string s(caps);
  size_t p = 0;
  while (p < s.size()) {
    size_t e = s.find(',', p);
    if (e == std::string::npos) e = s.size();
    const std::string kv = s.substr(p, e - p);
    p = e + 1;
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) continue;
    const std::string k = kv.substr(0, eq);
    const uint32_t v = (uint32_t)strtoul(kv.c_str() + eq + 1, nullptr, 0);
    auto clampv = [&](uint32_t lo, uint32_t hi) { return std::max(lo, std::min(hi, v)); };
    if (k == "trk") d.trk_cap = clampv(0, TRK);
    else if (k == "ulog") d.ulog_cap = clampv(0, d.ULOGC);
    else if (k == "creq") d.creq_cap = clampv(1, CREQ);
    else if (k == "cwmax") d.cwmax_cap = clampv(0, CWMAX);
    else if (k == "cev") d.cev_cap = clampv(0, CEV);
    else if (k == "mq") d.mq_cap = clampv(1, MQ);
    else if (k == "hv") d.hv = std::max<uint32_t>(1, v);  // k_inbox_apply from this many receipts
    else if (k == "rbt") *rb_thr = std::max<uint32_t>(1, v);  // rebase a chunk after this many wasted compares
    else if (k == "rbi") *rb_int = std::max<uint32_t>(1, v);  // ... looked at every this many ticks
    else if (k == "rx") *rx_cap = v;
    else if (k == "rp") *rp_cap = std::max<uint32_t>(64, v);  // replay / slow-path send lists (grow_caps tests)
    else if (k == "xinl") d.XI = std::max<uint32_t>(64, std::min<uint32_t>(XINL, v)) & ~7u;  // send/recv group past it
    else if (k == "sort") {
      uint32_t r = 2;
      while (r * 2 <= clampv(2, SORT_MAX)) r *= 2;  // a power of two (bitonic runs)
      d.sort_cap = r;
    }
  }
}

// The scalar fields of Dev (and the handle's rx= pin) from the config, the shard spec and the environment: every
// capacity the allocation table below uses. No HIP call.
static int fill_dev(swim_handle* h) {
  const swim_config& c = h->cfg;
  Dev& d = h->d;
  std::memset(&d, 0, sizeof(d));
  d.N = c.n_members;
  const KeyPlaneSizes kp = key_plane_sizes(c.n_members);
  d.NS = kp.NS;
  d.W = h->spec.world ? h->spec.world : 1u;
  d.rank = h->spec.rank;
  d.XW = 1;
  if (d.W > 1 && c.mode == SWIM_MODE_RUMOR) {  // slot sharding (engine.h): every shard runs every member
    d.XW = d.W;
    d.xrank = d.rank;
    d.W = 1;
    d.rank = 0;
  }
  d.lo = shard_lo(d.N, d.W, d.rank);
  d.hi = shard_lo(d.N, d.W, d.rank + 1);
  d.NL = d.hi - d.lo;
  d.F = c.gossip_fanout;
  d.kreq = c.ping_req_members;
  if (!to_ticks(c.ping_interval_ms, c.tick_ms, &d.ping_t) || !to_ticks(c.ping_timeout_ms, c.tick_ms, &d.pingTimeout_t) ||
      !to_ticks(c.gossip_interval_ms, c.tick_ms, &d.gossip_t) || !to_ticks(c.sync_interval_ms, c.tick_ms, &d.sync_t) ||
      !to_ticks(c.sync_timeout_ms, c.tick_ms, &d.syncTimeout_t) || !to_ticks(c.metadata_timeout_ms, c.tick_ms, &d.md_t) ||
      d.ping_t == 0 || d.gossip_t == 0 || d.sync_t == 0) {
    h->err = "every interval/timeout must be a positive multiple of tick_ms";
    return SWIM_EINVAL;
  }
  d.lat = c.latency_ticks;
  d.suspMult = c.suspicion_mult;
  d.repeatMult = c.gossip_repeat_mult;
  d.seed_lo = (uint32_t)c.seed;
  d.seed_hi = (uint32_t)(c.seed >> 32);
  d.init_mode = c.init_mode;
  d.mode = c.mode;
  d.n_dormant = c.n_dormant;
  d.churn = c.mode == SWIM_MODE_RUMOR ? c.churn_per_period : 0u;
  d.flags = c.flags;
  d.implicit = c.mode == SWIM_MODE_RUMOR && (c.n_members > 65536 || (c.flags & SWIM_FLAG_IMPLICIT_VIEWS)) ? 1u : 0u;
  d.fastp4 = c.mode == SWIM_MODE_RUMOR && !(c.flags & SWIM_FLAG_RECORD_EVENTS) ? 1u : 0u;
  d.exp = getenv("SWIM_EXP") ? (uint32_t)atoi(getenv("SWIM_EXP")) : 0u;  // timing experiments: wrong results
  // fast-structure capacities (include/swimhip_debug.h): SWIM_CAPS="trk=1,ulog=2,creq=1,cwmax=1,cev=1,mq=1,sort=2"
  // lowers them so that the exact fallbacks run; results stay bit-exact, only slower
  // undo log per member: a receiver merging thousands of records after a SYNC_ACK send (C2) would otherwise copy its
  // row on its own lane (cow_now); 1024 entries up to 65 536 members (8 KB each), 256 above
  d.ULOGC = c.n_members <= 65536 ? ULOG : 256;
  d.trk_cap = TRK, d.ulog_cap = d.ULOGC, d.creq_cap = CREQ, d.cwmax_cap = CWMAX, d.cev_cap = CEV, d.mq_cap = MQ;
  d.rr_atomic = getenv("SWIM_RR_ATOMIC") ? (uint32_t)atoi(getenv("SWIM_RR_ATOMIC")) : 64u;  // (measurements)
  h->rb_thr = 0, h->rb_int = REBASE_CHECK;
  d.hv = 24;  // routed receipts from which a member's P4 runs on a wave of its own (k_inbox_apply)
  d.XI = XINL;
  d.sort_cap = SORT_MAX;
  uint32_t rx_cap = NEVER, rp_cap = 0;
  if (const char* caps = getenv("SWIM_CAPS")) parse_caps(caps, d, &rx_cap, &rp_cap, &h->rb_thr, &h->rb_int);
  h->rx_pinned = rx_cap != NEVER;  // (growth keeps the pin: the variable may be gone by then)
  // seeds: LinkedHashSet of valid ids (MembershipProtocolImpl.java:160-166); self is skipped per member
  for (uint32_t i = 0; i < c.n_seeds; ++i) {
    uint32_t s = c.seeds[i];
    if (s >= d.N) continue;
    bool dup = false;
    for (uint32_t j = 0; j < d.n_seeds; ++j) dup |= d.seeds[j] == s;
    if (!dup) d.seeds[d.n_seeds++] = s;
  }
  const uint64_t N = d.N;
  // FD / gossip lists: a member can be listed twice when its REMOVED overtakes the metadata fetch of its ADDED
  // (emitMembershipEvent :543-588 is asynchronous), so the lists get slack beyond N - 1 entries
  d.LCAP = d.N + (c.list_slack ? c.list_slack : 64);
  d.FCAP = c.pending_fetch_cap ? c.pending_fetch_cap : 256;
  d.GRCAP = c.init_mode == SWIM_INIT_COLD_JOIN ? std::min<uint32_t>(d.N + 16, 1024) : 32;
  if (d.implicit) d.FCAP = d.GRCAP = 1;  // RUMOR mode: no metadata fetch, no SYNC reply group
  uint32_t maxSpread = d.repeatMult * (32u - (uint32_t)__builtin_clz(d.LCAP + 1));
  // link delays (swim_config.delay_cap_ms): the longest delay in ticks past lat
  {
    std::vector<uint32_t> t;
    if (!delay_table(c.delay_cap_ms, c.tick_ms, &t)) {
      h->err = "delay_cap_ms above 11 x tick_ms";
      return SWIM_EINVAL;
    }
    d.EMAX = (uint32_t)t.size();
    d.PCAP = c.delay_cap_ms ? PATHCAP_DELAY : PATHCAP;
  }
  d.LOGW = 8;
  // rounds kept for the infectedFrom replay (a delayed send arrives up to EMAX ticks after its round)
  while (d.LOGW < 4 * (maxSpread + 2) + 2 * ((d.EMAX + d.gossip_t - 1) / d.gossip_t + 1)) d.LOGW <<= 1;
  d.LOOKBACK = d.LOGW * d.gossip_t;
  d.gt_mul = gt_mul_of(d.gossip_t);
  // incarnation history of reborn (gossip, member) pairs (88 B per entry). 2^20 entries (92 MB) by default; a run
  // that asks for a large slot table (a storm: C4's heal rebirths a large share of the holder states) gets one
  // entry per 8 holder states, up to 2^24; SWIM_HIST_CAP overrides (a full table raises E_REBORN, info 1)
  {
    uint64_t hc = 1u << 20;
    if (c.gossip_slot_cap) {
      const uint64_t want = (uint64_t)c.gossip_slot_cap * N / 8;
      while (hc < want && hc < (1u << 24)) hc <<= 1;
    }
    if (const char* e = getenv("SWIM_HIST_CAP")) {
      hc = 1024;
      while (hc < strtoull(e, nullptr, 0) && hc < (1u << 26)) hc <<= 1;
    }
    d.HCAP = (uint32_t)hc;
  }
  // default: 64 slots per member, at most 32 GB of holder table (C2's SYNC re-spread storm keeps ~10^5 gossips alive)
  uint64_t slots = c.gossip_slot_cap ? c.gossip_slot_cap
                                     : std::min<uint64_t>(1ull << 22, std::max<uint64_t>(1024, std::min<uint64_t>(64 * N, (32ull << 30) / (4 * N))));
  // RUMOR mode with churn (C5): the rumors alive together follow from the config. A rumor reaches every member in
  // about 2 log2(N) rounds and its slot is recycled EXPB = 2 maxSpread + 4 rounds after its last receipt, so about
  // churn x (2 maxSpread + 4 + 2 bitlen(N)) gossip intervals' worth are alive, split over the XW slot shards (+10 %);
  // a member holds the ones of its last 2 maxSpread + 3 rounds (its receipt ring, below). Growth (grow_caps) covers
  // what this misses.
  uint64_t rumor_ring = 0;
  if (!c.gossip_slot_cap && c.mode == SWIM_MODE_RUMOR && c.churn_per_period) {
    const uint64_t life = (2ull * maxSpread + 4 + 2ull * bitlen(d.N)) * d.gossip_t;
    const uint64_t held = (2ull * maxSpread + 3) * d.gossip_t;
    slots = std::min<uint64_t>(1ull << 22, std::max<uint64_t>(1024, 11 * c.churn_per_period * life / (10 * d.ping_t * d.XW)));
    rumor_ring = 21 * c.churn_per_period * held / (20 * d.ping_t * d.XW);
  }
  // every shard allocates new gossips from its own slot range; the slot table itself is replicated, so the ranges
  // split the budget (twice over, for shards that create more than their share) instead of multiplying it by W: at
  // 100k members and W = 8 a full range per shard would be a 275 GB holder table on every GPU
  const uint64_t share = d.W == 1 ? slots : std::max<uint64_t>(1024, (2 * slots + d.W - 1) / d.W);
  d.SPR = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(slots, share), (1ull << 22) / d.W);
  d.SPR = (d.SPR + 63u) & ~63u;  // whole 64-slot groups per shard (holder bit rows)
  d.SLOTS = d.SPR * d.W;
  d.QW = d.SLOTS / 64;
  // a gossip's holders have all swept it within 2 (spread + 1) + 2 of their rounds after their receipt
  // (sweepGossips :283-308, spread <= maxSpread): its slot is recycled after that (slot_exp)
  d.EXPB = (2u * maxSpread + 4u) * d.gossip_t;
  if (2u * maxSpread + 4u >= 500u) {  // receipt-ring entries keep the infection period modulo 1024 (dev_util.h rg_entry)
    h->err = "gossipRepeatMult x ceilLog2(members) too large (at most 248)";
    return SWIM_EINVAL;
  }
  // 16-bit holder entries (engine.h S16_*): a gossip slot may stay in use SLIFE ticks. Its holders sweep it EXPB
  // ticks after their receipt, and an epidemic's first receipts come within about maxSpread + 1 rounds of its
  // creation, so a slot lives about (3 maxSpread + 6) gossip intervals. A config whose gossip interval is so many
  // ticks that this reaches SLIFE is refused here instead of failing with E_SLIFE mid-run
  if ((3ull * maxSpread + 6ull) * d.gossip_t >= SLIFE) {
    h->err = "gossipInterval / tick_ms x (3 x gossipRepeatMult x ceilLog2(members) + 6) must stay below " +
             std::to_string(SLIFE) + " ticks (the holder entries' tick window): use a coarser tick_ms";
    return SWIM_EINVAL;
  }
  // receipt ring per member: at least as many entries as the member can hold gossips; by default the slot table's
  // size, within about 16-24 GB in all (C2 holds ~3·10^5 gossips per member at 10k members), and
  // swim_config.gossip_ring_cap overrides (a full ring raises E_RING)
  {
    const uint64_t want = c.gossip_ring_cap ? c.gossip_ring_cap : rumor_ring ? std::max<uint64_t>(4096, rumor_ring)
                                            : std::min<uint64_t>(d.SLOTS, std::max<uint64_t>(4096, (16ull << 30) / (4 * N)));
    uint64_t bc = 64;
    while (bc < want && bc < (1ull << 31)) bc <<= 1;
    if (!c.gossip_ring_cap && !rumor_ring && bc > 4096 && bc * N * 4 > (24ull << 30)) bc >>= 1;
    d.BCAP = (uint32_t)bc;
  }
  uint64_t mc = N / d.sync_t * 4 + N / d.ping_t + 1024;
  if (c.init_mode == SWIM_INIT_COLD_JOIN) mc = std::max<uint64_t>(mc, N + 1024);
  d.MSGCAP = (uint32_t)mc;
  d.NCHUNK = kp.NCHUNK;
  d.NMETA = kp.NMETA;
  d.POOLCAP = (uint32_t)std::min<uint64_t>(1ull << 26, std::max<uint64_t>(1ull << 20, N * 64));
  d.EVCAP = c.event_cap ? c.event_cap : (1u << 20);
  // first receipts per tick: routed to P4 (RCAP), shipped to the other row shards (DCAP)
  d.DCAP = (uint32_t)std::min<uint64_t>(1ull << 27, std::max<uint64_t>(1ull << 16, N * 16384));
  d.RCAP = d.DCAP;
  // infectedFrom replays: in a small cluster most pairs have a logged contact, so under a DEAD-gossip storm nearly
  // every send is replayed (C4 at 2 000 members: ~4·10^7 per tick)
  d.SLOWCAP = d.RPCAP = std::max<uint32_t>(d.DCAP, 1u << 26);
  if (const char* dc = getenv("SWIM_DELIV_CAP")) {  // experiments (tools/exp_c4.py): first receipts per tick
    d.DCAP = d.RCAP = (uint32_t)std::min<uint64_t>(1ull << 30, strtoull(dc, nullptr, 0));
    d.SLOWCAP = d.RPCAP = std::max(d.SLOWCAP, d.DCAP);
  }
  if (rp_cap) d.SLOWCAP = d.RPCAP = rp_cap;
  if (d.implicit) {
    // C5: every period's rumors start at one tick, so their epidemics peak together: on one of 8 slot shards a tick
    // can deliver ~7·10^8 first receipts (8 B each). Their GOSSIP events skip the receipt routing (fastp4), and
    // infectedFrom replays are rare at this size.
    d.DCAP = 1u << 30;
    d.RCAP = d.fastp4 ? 1u << 22 : 1u << 28;
    d.SLOWCAP = d.RPCAP = 1u << 26;
  }
  // copy-on-write snapshots and pinned payload copies (pin_msg) per tick: up to 256 MB per buffer, at least 64 rows
  d.ARENA_ROWS = (uint32_t)std::min<uint64_t>(d.MSGCAP, std::max<uint64_t>(64, (256ull << 20) / (4ull * d.NS)));
  if (d.implicit) {  // no SYNC traffic: minimal message buffers
    d.MSGCAP = 1024;
    d.ARENA_ROWS = 1;
    d.POOLCAP = 1024;
  }
  d.NS8 = kp.NS8;  // row stride of the 8-bit shadow plane
  // the per-tick contact rows follow the row width; SWIM_CAPS rx=...: contact pairs past it replay their whole window
  d.CRCAP = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(4096, (512ull << 20) / (8ull * d.QW)));
  if (rx_cap != NEVER) d.CRCAP = rx_cap;
  d.NW = d.implicit ? 0u : (d.N + 63u) / 64u;  // (RUMOR mode with implicit views has no SYNC)
  // SYNC_ACK resolution (k_ack_resolve); SWIM_NO_ACKRES streams every payload (measurements)
  d.ackres = !d.implicit && !getenv("SWIM_NO_ACKRES") ? 1u : 0u;
  if (d.EMAX) {  // delayed gossip receipts by delivery tick; delayed SYNC / SYNC_ACK messages with their payloads
    d.DQCAP = (uint32_t)std::min<uint64_t>(1ull << 22, std::max<uint64_t>(1ull << 16, (1ull << 30) / (8ull * (d.EMAX + 2))));
    d.DSCAP = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(4096, (256ull << 20) / (4ull * d.NS)));
  }
  if (getenv("SWIM_SEND_LOG")) d.dbg_send_cap = (uint32_t)atoi(getenv("SWIM_SEND_LOG"));  // debugging aid: every counted gossip send
  // one GPU, stored tables: the rows' dirty-chunk masks decide SYNC-diff chunks without a load (k_ack_resolve);
  // SWIM_NO_DIRTY keeps the masks but never consults them (measurements, and the tests' reference path)
  // (RUMOR mode sends no SYNC: no masks)
  // the masks and the rebase counters live in the members' records' spare words (MS), no allocation of their own
  if (d.W == 1 && !d.implicit && d.mode != SWIM_MODE_RUMOR && kp.MW <= MSW) {
    d.MW = kp.MW;
    if (d.ackres && !getenv("SWIM_NO_DIRTY")) d.ackres |= ACKRES_DIRTY;
  }
  // the member kernel's light path (member_light.h): one GPU, FULL mode, stored tables, no timing experiment that laps
  // the general body's phases. SWIM_NO_LIGHT (any value but 0) turns it off: the tests' reference path. (Not the
  // parent kernel of the round that added the path: the launch keeps its LDS lists, so an A/B against that needs both builds.)
  if (d.W == 1 && d.XW == 1 && !d.implicit && d.mode != SWIM_MODE_RUMOR && !(d.exp & ~LIGHT_EXP_OK)) {
    const char* nl = getenv("SWIM_NO_LIGHT");
    d.light = nl && strcmp(nl, "0") ? 0u : LIGHT_ON;
  }
  // message-slot shards (msg_slots.h): the same handles from MSG_SHARD_MIN_N members on, except a cold join's (its seed
  // answers every member's SYNC from one lane: one shard's demand, which the sharded buffer serves only up to about
  // three quarters of MSGCAP). SWIM_MSG_SHARDS=n, a power of two from 1 to 32, overrides it on any one-GPU handle with
  // stored tables, whatever its init mode: 1 is the tests' reference path and the A/B switch on one build.
  // A value that is no such number is refused on every handle; on a row or slot shard and with implicit views a valid
  // one is read and not used: those keep one counter.
  d.msh = 1;
  const bool one_gpu_stored = d.W == 1 && d.XW == 1 && !d.implicit;
  if (one_gpu_stored && d.mode != SWIM_MODE_RUMOR && c.init_mode != SWIM_INIT_COLD_JOIN && d.N >= MSG_SHARD_MIN_N)
    d.msh = MSG_SHARDS_MAX;
  if (const char* e = getenv("SWIM_MSG_SHARDS")) {
    const unsigned long v = strtoul(e, nullptr, 0);
    if (v > MSG_SHARDS_MAX || !msg_shards_ok((uint32_t)v)) {
      h->err = "SWIM_MSG_SHARDS must be a power of two from 1 to 32";
      return SWIM_EINVAL;
    }
    if (one_gpu_stored) d.msh = (uint32_t)v;
  }
  if (d.W > 1) {
    d.MW = kp.MW;
    d.NSCAP = 1u << 16;
    d.RRCAP = d.NL;
    d.RQCAP = d.MSGCAP;
    d.RXCAP = d.MSGCAP;
    d.CHCAP = h->spec.chunk_cap ? h->spec.chunk_cap : (uint32_t)std::min<uint64_t>(4096, (uint64_t)d.MSGCAP * d.NCHUNK);
    uint64_t se = sync_entry_size(d.MW);
    d.XA_PEER = ((32 + 4ull * NSW * d.NSCAP + 4ull * RRW * d.RRCAP + se * d.RQCAP + 511) & ~255ull) +
                (uint64_t)d.CHCAP * CH * 4;
    d.XB_PEER = 16 + 8ull * std::min<uint64_t>((uint64_t)d.DCAP, 1ull << 25);
    d.inl = h->spec.transport == SWIM_TRANSPORT_RCCL ? 1u : 0u;
  }
  return SWIM_OK;
}

template <class T>
static int dalloc_fill(swim_handle* h, T** p, size_t count, int byte) {
  const int rc = dalloc(h, p, count);
  if (rc != SWIM_OK) return rc;
  HIPCK(hipMemsetAsync(*p, byte, (count ? count : 1) * sizeof(T), h->stream));
  return SWIM_OK;
}

// The allocation table: every device buffer once, with its element count and its initial fill. A: allocated only
// (launch_init or its first user writes it; SWIM_POISON exists to catch the ones nothing writes), Z: zeroed, F: every
// byte 0xFF. The fills are ordered on the engine stream, ahead of the Dev upload and launch_init. The order is the
// allocation numbering of SWIM_POISON_ONLY.
static int alloc_table(swim_handle* h) {
  const swim_config& c = h->cfg;
  Dev& d = h->d;
  const uint64_t N = d.N;
  const uint64_t NL = d.NL;  // per-observer arrays: this shard's rows only
  const uint64_t NV = d.implicit ? 1 : NL;  // implicit views: no table or list is stored
  int rc;
#define A(p, n) \
  if ((rc = dalloc(h, &(p), (size_t)(n))) != 0) return rc;
#define Z(p, n) \
  if ((rc = dalloc_fill(h, &(p), (size_t)(n), 0)) != 0) return rc;
#define F(p, n) \
  if ((rc = dalloc_fill(h, &(p), (size_t)(n), 0xFF)) != 0) return rc;
  Z(d.link_key, LKCAP) A(d.link_hist, (uint64_t)LKCAP * LKH * 2)
  A(d.dead_tick, N)
  A(d.dly_thr, DTAB * 256) A(d.dly_len, DTAB)
  A(d.ep_group, MAX_EPOCHS * N) A(d.md_version, N)
  A(d.nextPing, N) A(d.nextGossip, N) A(d.nextSync, N) A(d.held, N) A(d.timerMin, N) A(d.initFlags, N)
  A(d.firstGossip, N) A(d.ms, N) A(d.sel, N * 8)
  A(d.rowk, NV * d.NS) A(d.rowa, NV * d.NS) A(d.fdl, NV * d.LCAP) A(d.gl, NV * d.LCAP)
  Z(d.subs, NL * SUBCAP * 4) A(d.paths, NL * d.PCAP * 5) A(d.fetch, NL * d.FCAP * FREC) A(d.groups, NL * d.GRCAP * GREC)
  A(d.tround, N) Z(d.tcnt, N) A(d.tspread, N) A(d.tperiod, N) A(d.T, N * d.F) A(d.tcontact, N * d.F)
  // (slow_n, rp_n: the gossip plane resets them, but tick_flag publishes them for grow_caps from the first tick on)
  A(d.slow, d.SLOWCAP) Z(d.slow_n, 1) A(d.rp, d.RPCAP) Z(d.rp_n, 1) A(d.start_tick, N) A(d.jseed_n, N) A(d.jseeds, 16 * N)
  A(d.md_uidx, N) A(d.mcfg, 4 * N) A(d.md_ver, NL * MDU) A(d.churn_q, 2ull * d.churn) Z(d.ucnt, N) A(d.cin, N * d.F)
  Z(d.HB, (uint64_t)d.QW * N) Z(d.WB, (uint64_t)d.QW * N) A(d.cev, N * d.F * CEVW)
  A(d.rg, (uint64_t)d.BCAP * N) A(d.rhead, N) A(d.rwin, N) A(d.rseen, N) A(d.rtail, N) A(d.rwl, N) A(d.nrwl, 1)
  A(d.rsend, N) A(d.rwnew, N) Z(d.GU, d.QW) Z(d.DM, d.QW) A(d.agroup, d.QW) Z(d.nagroup, 2)
  A(d.tin_cnt, N) A(d.tin_off, N) A(d.tin_fill, N) A(d.tin, N * d.F) A(d.tlist, N) A(d.ntl, 1) A(d.rt0, N)
  A(d.crow, N * d.F) A(d.RX, (uint64_t)d.CRCAP * d.QW) A(d.rxl, 3ull * d.CRCAP) A(d.nrx, 1) A(d.cfl, N * d.F) A(d.ncfl, 1)
  A(d.log_tick, N * d.LOGW) A(d.log_spread, N * d.LOGW) A(d.log_cnt, N * d.LOGW) A(d.log_tg, N * d.LOGW * d.F)
  A(d.log_pos, N) A(d.spchg, N)
  A(d.slot_gid, d.SLOTS) A(d.slot_subj, d.SLOTS) A(d.slot_ctick, d.SLOTS) A(d.slot_key, d.SLOTS) A(d.slot_exp, d.SLOTS)
  A(d.slot_used, d.SLOTS) Z(d.S, (uint64_t)d.SLOTS * N) A(d.free_list, d.SLOTS) A(d.free_top, 1)
  A(d.xd, d.W > 1 ? d.DCAP : 1) Z(d.xd_n, 1) A(d.rc_raw, d.RCAP) Z(d.rc_n, 1) A(d.rc_cnt, N) A(d.rc_off, N) A(d.rc_fill, N)
  A(d.scan_part, 1024)
  A(d.rc_slot, d.RCAP) Z(d.rc_ndrop, N) Z(d.dead_rx, N) Z(d.leaving, N) A(d.rc_key, d.RCAP) A(d.rc_slot2, d.RCAP)
  A(d.rc_key2, d.RCAP) A(d.fexp, d.SLOTS) A(d.nfexp, 1) Z(d.hist, (uint64_t)d.HCAP * HREC)
  F(d.msgs[0], d.MSGCAP) F(d.msgs[1], d.MSGCAP) Z(d.nmsg, 2)  // (msgs: pin = NEVER, send_sync)
  A(d.arena[0], (uint64_t)d.ARENA_ROWS * d.NS) A(d.arena[1], (uint64_t)d.ARENA_ROWS * d.NS) Z(d.arena_used, 2)
  A(d.m_next, 2ull * d.MSGCAP) F(d.m_head, 2 * N) A(d.next_evt, N) Z(d.mdone, 2) A(d.trk, NL * TRKL)
  A(d.ulog, NL * d.ULOGC * 2) A(d.spq, NL * SPQ * 8) A(d.fpend, NL * KP * 2) A(d.pending_inc, N)
  A(d.chunk_meta, (uint64_t)d.MSGCAP * d.NMETA * 2)
  A(d.pool, d.POOLCAP) Z(d.pool_used, 1)
  A(d.hv_list, NL) Z(d.nhv, 1) A(d.hv_pend, NL) A(d.hv_tlast, NL) A(d.sg_list, N) A(d.nsg, 1) A(d.ap_list, N) A(d.nap, 1)
  Z(d.tbm, NL * d.NW)
  if (d.ackres) {
    A(d.tlog, 2 * NL * TL) A(d.tl_n, 2 * NL) F(d.tl_tick, 2 * NL) Z(d.ndl, 1)
    // (one GPU: an entry per narrow item, engine.h NPER)
    A(d.dlist, 4ull * d.MSGCAP * (d.W == 1 ? (d.NCHUNK + NPER - 1) / NPER : 1u))
    A(d.dlist_w, 4ull * d.MSGCAP) Z(d.ndlw, 1)
    if (d.W > 1) A(d.mlog, (uint64_t)d.MSGCAP * TL)
  }
  // capacity growth between ticks (grow_caps) reads these; SWIM_NO_GROW keeps the sizes fixed, and so does SWIM_GUARD
  // (a choice: a guarded run keeps every buffer, and its guard zones, where create put them). A row shard grows its
  // receipt rings and incarnation history (grow_caps_shard); its slot ids and exchange capacities are global
  if (!getenv("SWIM_NO_GROW") && !h->mem.guard) {
    Z(d.rfill, 1) Z(d.hist_n, 1)
  }
  A(d.ev, (uint64_t)d.EVCAP * 8) Z(d.ev_n, 1) Z(d.ctr, C_NCTR) Z(d.ctr_sh, (uint64_t)CSH * CSTRIDE) Z(d.err, 8)
  if (c.flags & SWIM_FLAG_EMULATOR_COUNTERS) Z(d.em, 2 * N)
  if (d.EMAX) {
    A(d.dq, (uint64_t)(d.EMAX + 2) * d.DQCAP) Z(d.dq_n, d.EMAX + 2) Z(d.dmark, N)
    A(d.ds_msg, d.DSCAP) A(d.ds_row, (uint64_t)d.DSCAP * d.NS) Z(d.ds_used, d.DSCAP) A(d.ds_free, d.DSCAP) A(d.ds_top, 1)
  }
  if (d.exp & EXP_WAVE_CLOCK) Z(d.wt, (uint64_t)(NL + 255) / 256 * 4 * WT_WORDS)
  if (d.fastp4) {
    Z(d.evp_hash, N) Z(d.evp_n, N)
  }
  if (d.XW > 1) Z(d.held_delta, N)
  if (getenv("SWIM_CAPS") || getenv("SWIM_FALLBACKS")) Z(d.fb, FB_N)  // count the capacity fallbacks (swim_debug_fallbacks)
  if (d.dbg_send_cap) {
    A(d.dbg_send, 5ull * d.dbg_send_cap) Z(d.dbg_send_n, 1)
  }
  if (d.W > 1) {
    A(d.rdirty, (uint64_t)NL * d.MW) A(d.arena_dirty[0], (uint64_t)d.ARENA_ROWS * d.MW)
    A(d.arena_dirty[1], (uint64_t)d.ARENA_ROWS * d.MW)
    A(d.base_row, d.NS) Z(d.xn, 8) A(d.ns_rec, (uint64_t)d.NSCAP * NSW) A(d.rr_rec, (uint64_t)d.RRCAP * RRW)
    A(d.mtmp, d.MSGCAP) A(d.rx_mask, (uint64_t)d.RXCAP * d.MW) A(d.rx_off, d.RXCAP)
    A(d.xa_send, d.W * d.XA_PEER) A(d.xa_recv, d.W * d.XA_PEER) A(d.xb_send, d.W * d.XB_PEER)
    A(d.xb_recv, d.W * d.XB_PEER) Z(d.xa_scnt, d.W) Z(d.xa_rcnt, d.W) Z(d.xb_scnt, d.W) Z(d.xb_rcnt, d.W)
    A(d.xi_send, (uint64_t)d.W * XINL) A(d.xi_recv, (uint64_t)d.W * XINL)
    Z(d.xdone, 2ull * d.W)  // [0]: peer columns done (k_pack_all), [1 + q]: blocks of column q done
  }
  // stored tables: the diff's 8-bit shadow plane of this shard's rows, last, only when it fits beside everything else
  // with the usual growth reserve (an optimisation: without it k_sync_diff and row_put use the u32 keys; SWIM_NO_K8
  // forces that). On a row shard it serves the payloads of local senders; peers' payloads arrive as u32 chunks
  if (!d.implicit && !getenv("SWIM_NO_K8")) {
    size_t fr = 0, tot = 0;
    HIPCK(hipMemGetInfo(&fr, &tot));
    if ((uint64_t)fr > NV * d.NS8 + (4ull << 30)) {
      A(d.rowk8, NV * d.NS8)
      if (d.W > 1) A(d.base_row8, d.NS8)
    }
  }
#undef A
#undef Z
#undef F
  return SWIM_OK;
}

// What the table does not express: host-side buffers and host-mapped words, the delayed-store free list, the slot
// free-list top, the members' config, the settings epochs, the device copy of Dev and the init kernels.
static int init_state(swim_handle* h) {
  Dev& d = h->d;
  const uint64_t N = d.N;
  int rc;
  d.halt = (uint32_t*)(d.ctr_sh + SH_HALT);  // (spare words of counter row 0, engine.h)
  if (d.EMAX) {
    std::vector<uint32_t> fl(d.DSCAP);
    for (uint32_t i = 0; i < d.DSCAP; ++i) fl[i] = i;
    const int32_t top = (int32_t)d.DSCAP;
    HIPCK(h2d(h->stream, d.ds_free, fl.data(), 4ull * d.DSCAP));
    HIPCK(h2d(h->stream, d.ds_top, &top, 4));
  }
  if (d.XW > 1 && h->spec.transport == SWIM_TRANSPORT_HOST) {
    h->hsend.resize(4ull * N * d.XW);
    h->hrecv.resize(4ull * N * d.XW);
  }
  if (d.W > 1) {
    HIPCK(hipHostMalloc((void**)&h->hcnt, 16ull * d.W, hipHostMallocDefault));
    HIPCK(hipHostMalloc((void**)&h->xi_host_h, 16ull * d.W, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCK(hipHostGetDevicePointer((void**)&d.xi_host, (void*)h->xi_host_h, 0));
    if (h->spec.transport == SWIM_TRANSPORT_HOST) {
      h->hsend.resize(d.W * std::max(d.XA_PEER, d.XB_PEER));
      h->hrecv.resize(d.W * std::max(d.XA_PEER, d.XB_PEER));
    }
  }
  HIPCK(hipHostMalloc((void**)&h->hflag, HF_BYTES, hipHostMallocMapped | hipHostMallocCoherent));
  for (uint32_t i = 0; i < HF_BYTES / 4; ++i) h->hflag[i] = 0;
  HIPCK(hipHostGetDevicePointer((void**)&d.hflag, (void*)h->hflag, 0));
  if ((rc = dalloc_fill(h, &d.hsh, 8, 0)) != 0) return rc;  // (hflag above: all zero)
  HIPCK(hipEventCreateWithFlags(&h->ev_member, hipEventDisableTiming));
  const int32_t top = (int32_t)d.SPR;
  HIPCK(h2d(h->stream, d.free_top, &top, 4));
  {  // every member starts with the swim_config FailureDetectorConfig and sync group 0 (swim_set_member_config)
    std::vector<uint32_t> mc(4ull * N);
    for (uint64_t m = 0; m < N; ++m) {
      mc[4 * m] = d.ping_t;
      mc[4 * m + 1] = d.pingTimeout_t;
      mc[4 * m + 2] = d.kreq;
      mc[4 * m + 3] = 0;
    }
    HIPCK(h2d(h->stream, d.mcfg, mc.data(), 16ull * N));
  }
  for (uint32_t e = 0; e < MAX_EPOCHS; ++e) d.ep_from[e] = NEVER;  // (uploaded with Dev below)
  h->group.assign(d.N, 0);
  for (uint32_t e = 0; e < MAX_EPOCHS; ++e) h->ep_from[e] = NEVER;
  h->cur_ep = 0;
  // every initialisation above is ordered on the engine stream (a non-blocking stream does not wait for the
  // legacy null stream, so a plain hipMemset could still be running when the first tick starts)
  Dev* dcopy = nullptr;
  if ((rc = dalloc(h, &dcopy, 1)) != 0) return rc;
  d.self = dcopy;
  HIPCK(h2d(h->stream, dcopy, &d, sizeof(Dev)));
  launch_init(d, h->stream);
  if ((rc = push_epoch(h)) != 0) return rc;
  return check_err(h);
}

static int build(swim_handle* h) {
  int rc;
  if ((rc = fill_dev(h)) != SWIM_OK || (rc = alloc_table(h)) != SWIM_OK) return rc;
  return init_state(h);
}

int create(const swim_config* cfg, const swim_shard_spec* spec, swim_handle** out) {
  if (!cfg || !out) return SWIM_EINVAL;
  *out = nullptr;
  const swim_config& c = *cfg;
  if (c.n_members < 2 || c.n_members > (1u << 20) || c.ping_timeout_ms >= c.ping_interval_ms || c.gossip_fanout == 0 || c.gossip_fanout > 8 ||
      c.ping_req_members > 8 || c.n_seeds > 16 || c.mode > SWIM_MODE_RUMOR ||
      (c.mode == SWIM_MODE_RUMOR && c.init_mode != SWIM_INIT_PRECONVERGED) || c.n_dormant > c.n_members ||
      (c.n_dormant && c.init_mode != SWIM_INIT_COLD_JOIN))
    return SWIM_EINVAL;
  if (c.latency_ticks != 1) return SWIM_EUNSUPPORTED;  // gossip data plane assumes one-tick hops
  if (spec) {
    if (spec->world < 1 || spec->world > 64 || spec->rank >= spec->world || spec->world > c.n_members / 2) return SWIM_EINVAL;
    if (spec->world > 1 && spec->transport != SWIM_TRANSPORT_RCCL &&
        !(spec->transport == SWIM_TRANSPORT_HOST && spec->exchange))
      return SWIM_EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= (int)c.device) return SWIM_EDEVICE;
  auto* h = new swim_handle();
  h->cfg = c;
  if (spec) h->spec = *spec;
  if (h->spec.world == 0) h->spec.world = 1;
  if (hipSetDevice((int)c.device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return SWIM_EDEVICE;
  }
  h->mem.stream = h->stream;
  if (h->spec.world > 1 && h->spec.transport == SWIM_TRANSPORT_RCCL) {
    ncclUniqueId id;
    static_assert(sizeof(id) == 128, "ncclUniqueId size");
    std::memcpy(&id, h->spec.rccl_id, sizeof(id));
    if (ncclCommInitRank(&h->comm, (int)h->spec.world, id, (int)h->spec.rank) != ncclSuccess) {
      fprintf(stderr, "swim_create_sharded: ncclCommInitRank failed (rank %u of %u)\n", h->spec.rank, h->spec.world);
      h->comm = nullptr;
      swim_destroy(h);
      return SWIM_EDEVICE;
    }
  }
  int rc = build(h);
  if (rc != SWIM_OK) {
    fprintf(stderr, "swim_create: %s\n", h->err.c_str());
    swim_destroy(h);
    return rc;
  }
  *out = h;
  return SWIM_OK;
}

}  // namespace swim
