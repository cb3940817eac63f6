// gossip_round.hip — the gossip data plane, steps 1-4: this tick's active slot groups and list counters, what each
// member's gossip round sweeps and where its window starts, the senders of each target, and the rounds' changes to
// the holder state (gossip_dev.h: the plane's file map and the holder state).
#include "gossip_dev.h"

namespace swim {

// 1. the active 64-slot groups of this tick in ascending order (one block: a block-wide scan over the group words),
// and the per-tick list counters
__global__ void __launch_bounds__(1024) k_gossip_groups(Dev d) {
  __shared__ uint32_t sh[1024];
  __shared__ uint32_t base;
  if (threadIdx.x == 0) {
    base = 0;
    *d.slow_n = *d.rp_n = *d.nrwl = *d.ntl = *d.xd_n = *d.nfexp = *d.nrx = *d.ncfl = *d.nsg = *d.nap = 0;
  }
  __syncthreads();
  for (uint32_t q0 = 0; q0 < d.QW; q0 += 1024) {
    const uint32_t q = q0 + threadIdx.x;
    const uint32_t f = q < d.QW && d.GU[q] != 0ull ? 1u : 0u;
    sh[threadIdx.x] = f;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
      const uint32_t v = threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
      __syncthreads();
      sh[threadIdx.x] += v;
      __syncthreads();
    }
    if (f) d.agroup[base + sh[threadIdx.x] - 1] = q;
    __syncthreads();
    if (threadIdx.x == 0) base += sh[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    d.nagroup[0] = base;
    d.nagroup[1] = base ? d.agroup[base - 1] + 1 : 0;  // span of the holder rows touched this tick
  }
}

// 2. per member with a gossip round this tick (every member on every shard: the holder state is replicated): where
// its sweep ends and its window starts in the ring (binary searches: the infection periods are sorted), and whether
// the round changes anything; the (sender, target) pairs of this shard's targets are counted per target
__global__ void __launch_bounds__(256) k_round_plan(Dev d, uint32_t k) {
  __shared__ uint32_t sh[5];
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  bool listed = false;
  if (m < d.N && d.tround[m]) {
    const uint32_t cnt = d.tcnt[m];
    for (uint32_t s = 0; s < cnt; ++s) {
      const uint32_t t = d.T[(size_t)m * d.F + s];
      if (t >= d.lo && t < d.hi) atomicAdd(&d.tin_cnt[t], 1u);
    }
    const uint32_t P = d.tperiod[m], sp = d.tspread[m];
    const int64_t slo = (int64_t)P - (int64_t)sweep_after(sp), wlo = (int64_t)P - (int64_t)sp;
    const uint32_t h = d.rhead[m], tl = d.rtail[m];
    const uint32_t* R = ring(d, m);
    const uint32_t mask = d.BCAP - 1;
    uint32_t lo = 0, hi = tl - h;  // offsets from h
    while (lo < hi) {  // first entry not swept: sweepGossips (:283-308) removes infP < P - 2 (spread + 1)
      const uint32_t mid = lo + (hi - lo) / 2;
      if (rg_period(R[(h + mid) & mask], P) < slo)
        lo = mid + 1;
      else
        hi = mid;
    }
    const uint32_t send = h + lo;
    hi = tl - h;
    while (lo < hi) {  // first entry inside the window: selectGossipsToSend (:246) keeps infP + spread >= P
      const uint32_t mid = lo + (hi - lo) / 2;
      if (rg_period(R[(h + mid) & mask], P) < wlo)
        lo = mid + 1;
      else
        hi = mid;
    }
    const uint32_t wnew = h + lo;
    listed = send != h || wnew != d.rwin[m] || d.rseen[m] != tl;
    if (listed) {
      d.rsend[m] = send;
      d.rwnew[m] = wnew;
    }
  }
  const uint32_t i = block_reserve(d.nrwl, listed ? 1u : 0u, sh);
  if (listed) d.rwl[i] = m;
}

// 3. senders of each target in one contiguous list (counting sort over this tick's pairs); the targets with senders;
// each target's ring end before this tick's receipts
__global__ void __launch_bounds__(256) k_tin_scatter(Dev d) {
  __shared__ uint32_t sh[5];
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t firsts = 0;  // bit s: this member's send s is its target's first this tick (the target is listed)
  if (m < d.N && d.tround[m]) {
    const uint32_t cnt = d.tcnt[m];
    for (uint32_t s = 0; s < cnt; ++s) {
      const uint32_t ms = m * d.F + s, t = d.T[ms];
      if (t < d.lo || t >= d.hi) continue;
      const uint32_t j = atomicAdd(&d.tin_fill[t], 1u);
      d.tin[d.tin_off[t] + j] = ms;
      if (j == 0) {
        d.rt0[t] = d.rtail[t];
        firsts |= 1u << s;  // gossip_fanout <= 8
      }
    }
  }
  uint32_t i = block_reserve(d.ntl, (uint32_t)__popc(firsts), sh);
  for (; firsts; firsts &= firsts - 1, ++i) d.tlist[i] = d.T[m * d.F + (uint32_t)(__ffs(firsts) - 1)];
}

// 4. the rounds' holder-state changes (sweepGossips :283-308 and the window of selectGossipsToSend :239-250), a
// wavefront (rows up to RCS words) or a workgroup (larger rows) per round member with work. Ring ranges (positions;
// see k_round_plan):
//   [h, send)                      swept: HB cleared, S marked SWEPT, the gossip count drops
//   [max(w0, h), min(seen, wnew))  out of the window: WB cleared (includes the swept entries that were in it)
//   [wnew, max(w0, h))             back in the window (the spread grew): WB set
//   [max(seen, wnew), tail)        received or created since the member's previous round: WB set
// Few changes (<= 64): one global atomic per entry. More: the member's HB / WB rows are staged through LDS in chunks
// of RCW words, so every word is read and written once per chunk and the bits change by LDS atomics.
// (RCW, RCS: gossip_dev.h, beside the kernels' declarations.)
__device__ __forceinline__ void rr_bits(const Dev& d, uint32_t m, uint32_t a, uint32_t b, uint32_t op,
                                        unsigned long long* lh, unsigned long long* lw, uint32_t c0, uint32_t c1,
                                        uint32_t tid, uint32_t nth) {
  ring_walk(ring(d, m), d.BCAP - 1, a, b, tid, nth, [&](uint32_t g) {
    const uint32_t q = g >> 6;
    const unsigned long long bit = 1ull << (g & 63u);
    if (lh) {  // LDS chunk [c0, c1) of the rows
      if (q < c0 || q >= c1) return;
      if (op == 0) atomicAnd(&lh[q - c0], ~bit);
      else if (op == 1) atomicAnd(&lw[q - c0], ~bit);
      else atomicOr(&lw[q - c0], bit);
    } else {
      if (op == 0) atomicAnd(&hrow(d, m)[q], ~bit);
      else if (op == 1) atomicAnd(&wrow(d, m)[q], ~bit);
      else atomicOr(&wrow(d, m)[q], bit);
    }
  });
}

// one round member's ring ranges (see above) by a group of nth threads; lh / lw: LDS rows of cw words
template <bool BLOCK>
__device__ void round_member(const Dev& d, uint32_t m, uint32_t k, unsigned long long* lh, unsigned long long* lw,
                             uint32_t cw, uint32_t span, uint32_t tid, uint32_t nth) {
  const uint32_t h = d.rhead[m], send = d.rsend[m], wnew = d.rwnew[m], tl = d.rtail[m], seen = d.rseen[m];
  const uint32_t w0 = (int32_t)(d.rwin[m] - h) > 0 ? d.rwin[m] : h;
  const uint32_t r2 = (int32_t)(seen - wnew) < 0 ? seen : wnew;  // min(seen, wnew)
  const uint32_t r4 = (int32_t)(seen - wnew) > 0 ? seen : wnew;  // max(seen, wnew)
  const uint32_t r3 = (int32_t)(w0 - wnew) > 0 ? w0 : wnew;      // end of the re-entry range
  // side effects of the sweeps (sweepGossips :283-308; on_sweep: a completed leave)
  ring_walk(ring(d, m), d.BCAP - 1, h, send, tid, nth, [&](uint32_t g) {
    d.S[s_idx(d, g, m)] |= S16_SWEPT;
    on_sweep(d, g, m, k);
  });
  const uint32_t nch = (send - h) + ((int32_t)(r2 - w0) > 0 ? r2 - w0 : 0u) + (r3 - wnew) + (tl - r4);
  if (nch <= d.rr_atomic || span == 0) {  // few changes: atomics on the rows
    rr_bits(d, m, h, send, 0, nullptr, nullptr, 0, 0, tid, nth);
    if ((int32_t)(r2 - w0) > 0) rr_bits(d, m, w0, r2, 1, nullptr, nullptr, 0, 0, tid, nth);
    rr_bits(d, m, wnew, r3, 2, nullptr, nullptr, 0, 0, tid, nth);
    rr_bits(d, m, r4, tl, 2, nullptr, nullptr, 0, 0, tid, nth);
  } else {
    for (uint32_t c0 = 0; c0 < span; c0 += cw) {
      const uint32_t c1 = min(span, c0 + cw);
      unsigned long long* H = hrow(d, m) + c0;
      unsigned long long* Wr = wrow(d, m) + c0;
      for (uint32_t j = tid; j < c1 - c0; j += nth) {
        lh[j] = H[j];
        lw[j] = Wr[j];
      }
      grp_sync<BLOCK>();
      rr_bits(d, m, h, send, 0, lh, lw, c0, c1, tid, nth);
      if ((int32_t)(r2 - w0) > 0) rr_bits(d, m, w0, r2, 1, lh, lw, c0, c1, tid, nth);
      rr_bits(d, m, wnew, r3, 2, lh, lw, c0, c1, tid, nth);
      rr_bits(d, m, r4, tl, 2, lh, lw, c0, c1, tid, nth);
      grp_sync<BLOCK>();
      for (uint32_t j = tid; j < c1 - c0; j += nth) {
        H[j] = lh[j];
        Wr[j] = lw[j];
      }
      grp_sync<BLOCK>();
    }
  }
  if (tid == 0) {
    d.rhead[m] = send;
    d.rwin[m] = wnew;
    d.rseen[m] = tl;
    if (send != h) {
      if (d.XW > 1)
        atomicSub(&d.held_delta[m], (int)(send - h));
      else
        atomicSub(&d.held[m], send - h);
    }
  }
}

// rows of up to cw = min(RCS, QW) words: one wavefront per round member (2 cw words of LDS each, four per workgroup,
// sized at launch: a slot table of 45 056 slots takes 11 KB per wave, so three workgroups fit a CU instead of two)
__global__ void __launch_bounds__(256) k_round_apply_w(const Dev* __restrict__ dp, uint32_t k, uint32_t cw) {
  const Dev& d = *dp;
  extern __shared__ unsigned long long lds_rows[];
  const uint32_t n = *d.nrwl, span = d.nagroup[1], wave = threadIdx.x >> 6;
  if (span > cw) return;  // k_round_apply_b
  unsigned long long* lh = lds_rows + (size_t)wave * 2 * cw;
  for (uint32_t i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4)
    round_member<false>(d, d.rwl[i], k, lh, lh + cw, cw, span, threadIdx.x & 63u, 64u);
}

// larger rows: one workgroup per round member, the rows staged in chunks of RCW words
// (cb = min(RCW, QW): the chunk in LDS; cw: k_round_apply_w's row limit)
__global__ void __launch_bounds__(256) k_round_apply_b(const Dev* __restrict__ dp, uint32_t k, uint32_t cb, uint32_t cw) {
  const Dev& d = *dp;
  extern __shared__ unsigned long long lds_rows[];
  unsigned long long *lh = lds_rows, *lw = lds_rows + cb;
  const uint32_t n = *d.nrwl, span = d.nagroup[1];
  if (span <= cw) return;  // k_round_apply_w
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    round_member<true>(d, d.rwl[i], k, lh, lw, cb, span, threadIdx.x, blockDim.x);
    __syncthreads();
  }
}

}  // namespace swim
