// kernels.hip — initialisation, state hashes, the small between-tick kernels and the tick launchers (the SYNC diff is
// in sync_diff.hip, the delayed-SYNC store in sync_delay.hip, receipt routing in route.hip, the gossip data plane in
// gossip_*.hip).
#include <hip/hip_runtime.h>

#include "dev_util.h"
#include "member_kernels.h"

namespace swim {

__global__ void k_pack_all(Dev d, uint32_t b, uint32_t spec);  // shard.hip
__global__ void k_unpack_a(Dev d, uint32_t k, uint32_t end, uint32_t spec);
__global__ void k_pack_b(Dev d);
__global__ void k_round_reset(Dev d);

// ------------------------------------------------------------------------------------------------------------
// init (SEMANTICS.md §3)
__device__ __forceinline__ uint32_t init_draw(const Dev& d, uint32_t m, uint32_t what, uint32_t i) {
  return philox(m, what, i, 0, d.seed_lo ^ SALT_INIT, d.seed_hi).x;
}

__global__ void k_init_members(Dev d) {
  uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= d.N) return;
  bool pre = d.init_mode == 1;
  d.ms[m].tsize = pre ? d.N : 1;
  d.ms[m].fdLen = pre ? d.N - 1 : 0;
  d.ms[m].gLen = pre ? d.N - 1 : 0;
  d.ms[m].fdPeriod = d.ms[m].rsv_period = d.ms[m].gCounter = 0;
  d.nextPing[m] = pre ? 1 + init_draw(d, m, 1, 0) % d.ping_t : d.ping_t;
  uint32_t ng = pre ? 1 + init_draw(d, m, 2, 0) % d.gossip_t : d.gossip_t;
  d.nextGossip[m] = ng;
  d.firstGossip[m] = ng;
  d.nextSync[m] = pre ? 1 + init_draw(d, m, 3, 0) % d.sync_t : NEVER;
  if (d.mode == 1u) d.nextPing[m] = d.nextSync[m] = NEVER;  // RUMOR: gossip layer only (SEMANTICS.md §9)
  const bool dormant = m >= d.N - d.n_dormant;  // not started until swim_join (k_join)
  d.start_tick[m] = (pre || dormant) ? NEVER : 0u;
  d.jseed_n[m] = NONE32;
  d.md_uidx[m] = NONE32;
  d.ms[m].cidCnt = d.ms[m].syncSeq = d.ms[m].evSeq = d.held[m] = 0;
  d.timerMin[m] = NEVER;
  d.initFlags[m] = d.ms[m].initDeadline = d.ms[m].initCidBase = d.ms[m].initN = 0;
  d.ms[m].nsub = d.ms[m].npath = d.ms[m].nfetch = 0;
  d.ms[m].fnext = NEVER;
  d.ms[m].pingIdx = 0;
  d.ms[m].remoteIdx = pre ? 0 : -1;
  for (int i = 0; i < 8; ++i) d.sel[(size_t)m * 8 + i] = 0;
  d.ms[m].evHash = 0;
  d.tround[m] = 0;
  d.log_pos[m] = 0;
  d.spchg[m] = 0;
  d.dead_tick[m] = dormant ? 0u : NEVER;  // a process not started yet refuses connections, like a dead one
  if (m == 0) *first_dead_word(d) = d.n_dormant ? 0u : NEVER;  // the lower bound of the entries above (engine.h)
  d.md_version[m] = 0;
  d.rc_cnt[m] = 0;
  d.rc_off[m] = 0;
  d.rc_fill[m] = 0;
  d.m_head[m] = d.m_head[d.N + m] = NEVER;
  d.next_evt[m] = NEVER;
  d.pending_inc[m] = 0;
  d.rhead[m] = d.rwin[m] = d.rseen[m] = d.rtail[m] = 0;  // empty receipt ring (gossip_dev.h)
  d.tin_cnt[m] = d.tin_fill[m] = 0;
  if (m >= d.lo && m < d.hi)
    for (uint32_t g = 0; g < d.GRCAP; ++g) d.groups[(lidx(d, m) * d.GRCAP + g) * GREC + 5] = 0;
  for (uint32_t e = 0; e < d.LOGW; ++e) d.log_tick[(size_t)m * d.LOGW + e] = NEVER;
}

// one block per observer row (grid-strided): both planes are written with coalesced 4-B stores
__global__ void k_init_rows(Dev d) {
  if (d.implicit) return;
  const uint64_t full = rec_key(ST_ALIVE, 0) | META_BIT;
  for (uint32_t li = blockIdx.x; li < d.NL; li += gridDim.x) {
    uint32_t m = d.lo + li;
    uint32_t* rk = d.rowk + (size_t)li * d.NS;
    uint32_t* ra = d.rowa + (size_t)li * d.NS;
    for (uint32_t s = threadIdx.x; s < d.NS; s += blockDim.x) {
      const uint64_t v = s >= d.N ? 0ull : (d.init_mode == 1 || m == s) ? full : 0ull;
      key_put(d, rk, nullptr, li, s, key32(v), 0u);  // (the mask: below, the whole row's at once)
      ra[s] = aux32(v);
    }
    if (d.rowk8)  // (the 8-bit plane's wider padding: zero, absent)
      for (uint32_t s = d.NS + threadIdx.x; s < d.NS8; s += blockDim.x) d.rowk8[(size_t)li * d.NS8 + s] = 0;
    // dirty chunks against the baseline (the PRECONVERGED row, an empty row for a cold join): none for a PRECONVERGED
    // row, the own chunk for a cold join
    if (uint64_t* rd = row_dirty(d, li))
      for (uint32_t w = threadIdx.x; w < d.MW; w += blockDim.x)
        rd[w] = (d.init_mode != 1 && (m / CH) >> 6 == w) ? 1ull << ((m / CH) & 63) : 0ull;
    if (d.W == 1 && d.MW && threadIdx.x < 3) d.ms[li].cstat[threadIdx.x] = 0;  // (one GPU: the rebase counters)
  }
}

// PRECONVERGED lists: position p of observer m holds the other member of rank feistel_m(p) (SEMANTICS.md §3)
__global__ void k_init_lists(Dev d) {
  if (d.init_mode != 1 || d.N < 2 || d.implicit) return;
  uint32_t n = d.N - 1;
  for (uint32_t m = d.lo + blockIdx.x; m < d.hi; m += gridDim.x) {
    for (uint32_t w = 0; w < 2; ++w) {
      FeistelPerm P = make_perm(n, init_draw(d, m, 16 + 4 * w + 0, 0), init_draw(d, m, 16 + 4 * w + 1, 0),
                                init_draw(d, m, 16 + 4 * w + 2, 0), init_draw(d, m, 16 + 4 * w + 3, 0));
      uint32_t* L = (w == 0 ? d.fdl : d.gl) + lidx(d, m) * d.LCAP;
      for (uint32_t p = threadIdx.x; p < n; p += blockDim.x) {
        uint32_t j = feistel(P, p);
        L[p] = j < m ? j : j + 1;
      }
    }
  }
}

__global__ void k_init_slots(Dev d) {
  uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= d.SLOTS) return;
  d.slot_used[g] = 0;
  d.slot_exp[g] = NEVER;
  // each shard allocates only from its own slot range [rank SPR, (rank+1) SPR), so slot ids are global
  if (g < d.SPR) d.free_list[g] = d.rank * d.SPR + d.SPR - 1 - g;
}

// the SYNC baseline row (record keys): what a PRECONVERGED row starts as, an empty row for a cold join
// (and its 8-bit shadow, what a narrow item reads for a peer's payload chunk that was not shipped)
__global__ void k_init_base(Dev d) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t v = (s < d.N && d.init_mode == 1) ? key32(rec_key(ST_ALIVE, 0)) : 0u;
  if (s < d.NS) d.base_row[s] = v;
  if (d.base_row8 && s < d.NS8) d.base_row8[s] = key8(v);
}

// ------------------------------------------------------------------------------------------------------------
// state hashes (SEMANTICS.md §8), one block per member
__global__ void __launch_bounds__(256) k_hash(Dev d, uint64_t* out, uint32_t now) {
  __shared__ unsigned long long red[4][256];
  uint32_t m = d.lo + blockIdx.x;
  if (m >= d.hi) return;
  unsigned long long hr = 0, hf = 0, hg = 0, hgs = 0;
  const uint32_t* rk = d.rowk + lidx(d, m) * d.NS;
  const uint32_t* ra = d.rowa + lidx(d, m) * d.NS;
  uint32_t fl = d.ms[m].fdLen, gl = d.ms[m].gLen;
  if (d.implicit) {  // the PRECONVERGED row and lists, computed (engine.h list_at)
    const FeistelPerm P0 = list_perm(d, m, 0), P1 = list_perm(d, m, 1);
    for (uint32_t s = threadIdx.x; s < d.N; s += blockDim.x) hr += hpair(s, PRE_REC);
    for (uint32_t p = threadIdx.x; p < fl; p += blockDim.x) hf += hpair((uint64_t)p | (1ull << 40), list_at(P0, m, p));
    for (uint32_t p = threadIdx.x; p < gl; p += blockDim.x) hg += hpair((uint64_t)p | (2ull << 40), list_at(P1, m, p));
  } else {
    for (uint32_t s = threadIdx.x; s < d.N; s += blockDim.x) {
      const uint32_t k = rk[s];
      if ((k & 3u) != ST_ABSENT) hr += hpair(s, rec_join(k, ra[s]));
    }
    for (uint32_t p = threadIdx.x; p < fl; p += blockDim.x) hf += hpair((uint64_t)p | (1ull << 40), d.fdl[lidx(d, m) * d.LCAP + p]);
    for (uint32_t p = threadIdx.x; p < gl; p += blockDim.x) hg += hpair((uint64_t)p | (2ull << 40), d.gl[lidx(d, m) * d.LCAP + p]);
  }
  const bool dead = d.dead_tick[m] != NEVER;  // a crashed member keeps no gossips (SEMANTICS.md §1)
  for (uint32_t g = threadIdx.x; g < d.SLOTS && !dead; g += blockDim.x) {
    if (!d.slot_used[g]) continue;
    uint32_t e = s_get(d, g, m, now + d.lat);
    // receipts applied at the end of tick now-1 belong to P4 of tick `now`: not yet visible
    if (s_held(e) && s_ctick(e) < now) hgs += hpair(d.slot_gid[g], rounds_before(d, m, s_ctick(e)));
  }
  red[0][threadIdx.x] = hr;
  red[1][threadIdx.x] = hf;
  red[2][threadIdx.x] = hg;
  red[3][threadIdx.x] = hgs;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
      for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    uint64_t* o6 = out + (size_t)m * 6;
    o6[0] = red[0][0];
    o6[1] = red[1][0] + mix64((uint64_t)(int64_t)d.ms[m].pingIdx ^ 0xF00Dull) + fl;
    o6[2] = red[2][0] + mix64((uint64_t)(int64_t)d.ms[m].remoteIdx ^ 0xBEEFull) + gl;
    o6[3] = d.ms[m].evHash;
    o6[4] = red[3][0];
    uint64_t ns = d.nextSync[m] == NEVER ? ~0ull : (uint64_t)d.nextSync[m];
    o6[5] = hpair(hpair(hpair(d.ms[m].cidCnt, d.ms[m].syncSeq), d.ms[m].gCounter), ns) +
            mix64((uint64_t)d.ms[m].fdPeriod * 3 + (uint64_t)gossip_period(d, d.nextGossip[m], d.firstGossip[m]) * 7);
  }
}

__global__ void k_tick_end(Dev d, uint32_t k) { tick_end(d, k); }

// slot sharding: the all-reduced gossip-count deltas of this tick
__global__ void k_held_add(Dev d, const int32_t* sum) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= d.N) return;
  d.held[m] = (uint32_t)((int32_t)d.held[m] + sum[m]);
  d.held_delta[m] = 0;
}
void launch_held_add(const Dev& d, const int32_t* sum, void* stream) {
  hipLaunchKernelGGL(k_held_add, dim3((d.N + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, sum);
}

// every SCRUB ticks (engine.h): the holder entries of recycled slots are cleared, 8 entries (16 B) per lane, so that
// no stale entry outlives the 13-bit tick window of s_get. SLOTS is a multiple of 64: a lane's 8 entries share a member.
__global__ void __launch_bounds__(256) k_s_scrub(Dev d, uint32_t now) {
  const uint64_t nq = (uint64_t)d.N * d.SLOTS / 8;
  const uint32_t ref = now + d.lat;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * blockDim.x) {
    uint4* p = (uint4*)d.S + i;
    uint4 v = *p;
    if ((v.x | v.y | v.z | v.w) == 0u) continue;
    const uint32_t g0 = (uint32_t)((i * 8) % d.SLOTS);
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    bool changed = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint16_t e = (uint16_t)(w[j >> 1] >> ((j & 1) * 16));
      if (!(e & S16_EVER)) continue;
      const uint32_t g = g0 + j;
      if (!d.slot_used[g] || s16_tick(e, ref) < d.slot_ctick[g]) {
        w[j >> 1] &= ~(0xFFFFu << ((j & 1) * 16));
        changed = true;
      }
    }
    if (changed) *p = make_uint4(w[0], w[1], w[2], w[3]);
  }
}
void launch_s_scrub(const Dev& d, uint32_t now, void* stream) {
  hipLaunchKernelGGL(k_s_scrub, dim3(8192), dim3(256), 0, (hipStream_t)stream, d, now);
}

// ------------------------------------------------------------------------------------------------------------
// host launchers
void launch_init(const Dev& d, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_init_members, dim3(cdiv(d.N, 256)), dim3(256), 0, st, d);
  hipLaunchKernelGGL(k_init_rows, dim3(4096), dim3(256), 0, st, d);
  hipLaunchKernelGGL(k_init_lists, dim3(4096), dim3(256), 0, st, d);
  hipLaunchKernelGGL(k_init_slots, dim3(cdiv(d.SLOTS, 256)), dim3(256), 0, st, d);
  if (d.base_row) hipLaunchKernelGGL(k_init_base, dim3(cdiv(d.NS8, 256)), dim3(256), 0, st, d);
}

void launch_member(const Dev& d, uint32_t k, void* stream, const TickEvents* prof, bool spec, bool split, uint32_t lf) {
  hipStream_t st = (hipStream_t)stream;
  const MemberFront f = member_front(d);  // the front's addresses as an argument (member_kernels.h)
  if (prof && prof->all) hipEventRecord((hipEvent_t)prof->ev[2], st);
  if (split) {  // a gossip plane ran last tick: members with many routed receipts run P4 a wave each (k_inbox_apply)
    // (the second launch closes the tick)
    hipLaunchKernelGGL(k_member_tick_t<BODY_SPLIT>, dim3(cdiv(d.NL, 256)), dim3(256), 0, st, d.self, k, 0u, f);
    hipLaunchKernelGGL(k_inbox_apply, dim3(2048), dim3(256), 0, st, d.self, k);
    hipLaunchKernelGGL(k_member_tick_t<BODY_RESUME>, dim3(cdiv(d.NL, 256)), dim3(256), 0, st, d.self, k, MT_END, f);  // + tick_flag
  } else {
    hipLaunchKernelGGL(k_member_tick_t<BODY_FULL>, dim3(cdiv(d.NL, 256)), dim3(256), 0, st, d.self, k,
                       MT_END | (spec ? MT_SPEC | lf : 0u), f);  // + tick_flag, or (speculative) tick_reset
  }
  if (d.dly_on) {
    launch_sync_redeliver(d, k, st, spec);
    launch_sync_defer(d, k, st, spec);
  }
  if (prof && prof->all) hipEventRecord((hipEvent_t)prof->ev[3], st);
}

void launch_gossip(const Dev& d, uint32_t k, void* stream, const TickEvents* prof) {
  hipStream_t st = (hipStream_t)stream;
  launch_gossip_send(d, k, st, prof);
  launch_gossip_apply(d, k, st);
}

// sharded tick (W > 1): A = SYNC diff + member control + pack exchange A; B = unpack A, the rounds' holder-state
// changes and this shard's targets' sends, pack exchange B (their first receipts); C = peers' first receipts into the
// replicated holder state, this shard's receipts, routing, slot recycling
void launch_tick_a(const Dev& d, uint32_t k, void* stream, const TickEvents* prof, bool spec) {
  hipStream_t st = (hipStream_t)stream;
  uint32_t b = k & 1;
  const uint32_t sp = spec ? 1u : 0u;
  launch_diff(d, k, stream, prof, spec ? LS_SPEC : 0u);
  if (prof && prof->all) hipEventRecord((hipEvent_t)prof->ev[2], st);
  hipLaunchKernelGGL(k_member_tick_t<BODY_FULL>, dim3(cdiv(d.NL, 256)), dim3(256), 0, st, d.self, k, spec ? MT_SPEC : 0u,
                     member_front(d));
  if (prof && prof->all) hipEventRecord((hipEvent_t)prof->ev[3], st);
  if (d.dly_on) launch_sync_redeliver(d, k, st, spec);
  hipLaunchKernelGGL(k_pack_all, dim3(16, d.W), dim3(256), 0, st, d, b, sp);  // route + exchange-A regions
}

void launch_tick_b(const Dev& d, uint32_t k, void* stream, const TickEvents* prof, bool gossip, bool spec) {
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_unpack_a, dim3(32, d.W), dim3(256), 0, st, d, k, gossip ? 0u : 1u, spec ? 1u : 0u);
  if (d.dly_on) launch_sync_defer(d, k, st, spec);
  if (!gossip) {  // no gossip slot in use on any shard: nothing to send, deliver or recycle; no exchange B
    if (prof && prof->all) hipEventRecord((hipEvent_t)prof->ev[4], st);
    if (prof && prof->all) hipEventRecord((hipEvent_t)prof->ev[5], st);
    return;
  }
  launch_gossip_send(d, k, st, prof);
  hipLaunchKernelGGL(k_pack_b, dim3(64, d.W), dim3(256), 0, st, d);
}

void launch_tick_c(const Dev& d, uint32_t k, void* stream, bool gossip) {
  hipStream_t st = (hipStream_t)stream;
  if (!gossip) return;  // k_unpack_a closed the tick
  launch_unpack_b(d, k, st);
  launch_gossip_apply(d, k, st);
  hipLaunchKernelGGL(k_round_reset, dim3(16, d.W), dim3(256), 0, st, d);
  hipLaunchKernelGGL(k_tick_end, dim3(1), dim3(64), 0, st, d, k);
}

// swim_update_metadata of a member with no column yet: column u; every local observer stores version 0 (the only
// version it could have fetched so far)
__global__ void k_md_column(Dev d, uint32_t m, uint32_t u) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) d.md_uidx[m] = u;
  if (i < d.NL) d.md_ver[(size_t)i * MDU + u] = 0;
}

void launch_md_column(const Dev& d, uint32_t m, uint32_t u, void* stream) {
  hipLaunchKernelGGL(k_md_column, dim3((d.NL + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, m, u);
}

// swim_join: a dormant member starts at tick k as a fresh process (ClusterImpl.join0, schedules from k) with its seeds
struct JoinSeeds {
  uint32_t s[16];
};
__global__ void k_join(Dev d, uint32_t m, uint32_t k, JoinSeeds js, uint32_t n) {
  if (threadIdx.x != 0) return;
  d.dead_tick[m] = NEVER;  // (first_dead stays: a lower bound only ever goes down)
  d.start_tick[m] = k;
  d.nextPing[m] = k + mc_ping_t(d, m);
  d.nextGossip[m] = d.firstGossip[m] = k + d.gossip_t;
  d.jseed_n[m] = n;
  for (uint32_t i = 0; i < n; ++i) d.jseeds[(size_t)m * 16 + i] = js.s[i];
}

void launch_join(const Dev& d, uint32_t m, uint32_t k, const uint32_t* seeds, uint32_t n, void* stream) {
  JoinSeeds js{};
  for (uint32_t i = 0; i < n && i < 16; ++i) js.s[i] = seeds[i];
  hipLaunchKernelGGL(k_join, dim3(1), dim3(64), 0, (hipStream_t)stream, d, m, k, js, n);
}

// swim_kill: member m is dead from tick t; the lower bound of dead_tick first (engine.h first_dead_word)
__global__ void k_kill(Dev d, uint32_t m, uint32_t t) {
  if (threadIdx.x != 0) return;
  atomicMin(first_dead_word(d), t);
  d.dead_tick[m] = t;
}

void launch_kill(const Dev& d, uint32_t m, uint32_t t, void* stream) {
  hipLaunchKernelGGL(k_kill, dim3(1), dim3(64), 0, (hipStream_t)stream, d, m, t);
}

void launch_hash(const Dev& d, uint64_t* out, uint32_t now, void* stream) {
  hipLaunchKernelGGL(k_hash, dim3(d.NL), dim3(256), 0, (hipStream_t)stream, d, out, now);
}

}  // namespace swim
