// user_gossip.hip — gossips the host queues at P0 of a tick, outside the members' own control path: user gossips
// (swim_spread_gossip) and the RUMOR-mode churn rumors. They touch the gossip tables and a member's gossip counters,
// never the per-member protocol state of member_state.h.
#include "dev_util.h"

namespace swim {

// Cluster.spreadGossip (ClusterImpl.java:208-211) queued by swim_spread_gossip: user gossips of this shard's live
// members, in call order, at P0 of tick k (before the member kernel loads gCounter / held). Only the order of one
// member's calls is observable (its gossip counters follow them, GossipProtocolImpl.generateGossipId :207-209), so
// the queue runs one thread per entry in three passes: count the entries per member, create each gossip with
// counter gCounter[m] + (its rank among the member's entries), then advance the member's counter and gossip count
// once. Slot ids are not observable; a wave takes its slots with one atomic on the free stack.
__device__ __forceinline__ bool ug_live(const Dev& d, uint32_t m, uint32_t k) {
  return m >= d.lo && m < d.hi && !dead_at(d, m, k);
}
__global__ void k_ug_count(Dev d, uint32_t k, const uint64_t* q, uint32_t n, uint32_t* ucnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = (uint32_t)q[2 * i];
  if (ug_live(d, m, k)) atomicAdd(&ucnt[m], 1u);
}
// rank of entry i among the queue entries of member m before it (members with one entry: 0, no scan), and among
// those whose gossip this (slot) shard stores (its ring position); gc0 = the member's gossip counter before the queue
struct UgRank {
  uint32_t all, mine;
};
__device__ __forceinline__ UgRank ug_rank(const Dev& d, const uint64_t* q, uint32_t i, uint32_t m, uint32_t cnt,
                                          uint32_t gc0) {
  UgRank r{0, 0};
  if (cnt <= 1) return r;
  for (uint32_t j = 0; j < i; ++j)
    if ((uint32_t)q[2 * j] == m) r.mine += slot_mine(d, ((uint64_t)m << 32) | (gc0 + r.all++)) ? 1u : 0u;
  return r;
}
__global__ void __launch_bounds__(256) k_ug_create(Dev d, uint32_t k, const uint64_t* q, uint32_t n, const uint32_t* ucnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t m = i < n ? (uint32_t)q[2 * i] : 0u;
  bool mine = false;
  uint64_t gid = 0;
  UgRank rk{0, 0};
  if (i < n && ug_live(d, m, k)) {
    rk = ug_rank(d, q, i, m, ucnt[m], d.ms[m].gCounter);
    gid = ((uint64_t)m << 32) | (d.ms[m].gCounter + rk.all);
    mine = slot_mine(d, gid);  // slot sharding: only the owning shard stores it; every shard counts it as held
  }
  const uint64_t bm = __ballot(mine);
  const uint32_t lane = __lane_id(), nb = (uint32_t)__popcll(bm);
  int top = 0;
  if (lane == 0 && nb) top = atomicSub(d.free_top, (int)nb);
  top = __shfl(top, 0);
  if (mine) {
    const int pos = top - (int)nb + (int)__popcll(bm & ((1ull << lane) - 1ull));
    if (pos < 0)
      set_err(d, E_SLOTS);
    else  // ring position: the member's stored gossips of this queue take consecutive positions in call order
      slot_init(d, d.free_list[pos], m, k, gid, USER_SUBJ, q[2 * i + 1], d.rtail[m] + rk.mine);
  }
  if (lane == 0 && nb) atomicAdd(&d.ctr[C_GCREATED], (unsigned long long)nb);
}
__global__ void k_ug_finish(Dev d, uint32_t k, const uint64_t* q, uint32_t n, uint32_t* ucnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = (uint32_t)q[2 * i];
  if (!ug_live(d, m, k)) return;
  const uint32_t c = ucnt[m], gc0 = d.ms[m].gCounter;
  if (c > 1 && ug_rank(d, q, i, m, c, gc0).all != 0) return;  // the member's first entry advances it once
  uint32_t mine = 0;  // ring entries this shard appended for the member
  for (uint32_t r = 0; r < c; ++r) mine += slot_mine(d, ((uint64_t)m << 32) | (gc0 + r)) ? 1u : 0u;
  d.ms[m].gCounter = gc0 + c;
  d.held[m] += c;
  d.rtail[m] += mine;
  ucnt[m] = 0;
}
void launch_ug(const Dev& d, uint32_t k, const uint64_t* q, uint32_t n, hipStream_t st) {
  if (n == 0) return;
  const dim3 g((n + 255) / 256), b(256);
  hipLaunchKernelGGL(k_ug_count, g, b, 0, st, d, k, q, n, d.ucnt);
  hipLaunchKernelGGL(k_ug_create, g, b, 0, st, d, k, q, n, d.ucnt);
  hipLaunchKernelGGL(k_ug_finish, g, b, 0, st, d, k, q, n, d.ucnt);
}

// RUMOR-mode churn of period p = k / ping_t (SEMANTICS.md §9): event i picks the churned member v and an origin
// o != v; the rumor (p << 32 | v) is then spread by o through k_user_gossips, in event order
__global__ void k_churn(Dev d, uint32_t k) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.churn) return;
  const uint32_t p = k / d.ping_t;
  const u32x4 r = philox(p, i, 0, 0, d.seed_lo ^ SALT_CHURN, d.seed_hi);
  const uint32_t v = next_int(r.x, d.N);
  uint32_t o = next_int(r.y, d.N - 1);
  o += o >= v ? 1u : 0u;
  d.churn_q[2 * i] = o;
  d.churn_q[2 * i + 1] = ((uint64_t)p << 32) | v;
}

void launch_churn(const Dev& d, uint32_t k, void* stream) {
  hipLaunchKernelGGL(k_churn, dim3((d.churn + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, k);
  launch_ug(d, k, d.churn_q, d.churn, (hipStream_t)stream);
}

void launch_user_gossips(const Dev& d, uint32_t k, const uint64_t* q, uint32_t n, void* stream) {
  launch_ug(d, k, q, n, (hipStream_t)stream);
}

}  // namespace swim
