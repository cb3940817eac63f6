// grow.hip — capacity growth between ticks.
// One GPU: the gossip slot table, the receipt rings and the per-tick receipt / replay lists start at the config's size
// and grow between ticks before they can overflow: after each member kernel of a tick with the gossip plane active,
// tick_flag has published the slots in use, the largest ring fill and the previous gossip plane's list lengths
// (Dev::hflag). A structure past half (slots, rings) or a quarter (per-tick lists) of its capacity is reallocated
// larger, within the free HBM, its contents moved: slot ids, ring positions and every held bit keep their meaning, so
// the simulation is unchanged (slot ids are not observable). SWIM_NO_GROW: fixed sizes.
//
// Each structure has one stage below. A stage allocates every replacement first (Staged, dev_alloc.h), then moves the
// contents, then commits: a failed allocation leaves the handle, and the device state, on its old buffers. A stage
// takes what it allocates from *budget, and sets *grew when it replaced something.
#include "handle.h"

#include <algorithm>

using namespace swim;

namespace swim {

// per-tick lists: nothing in them between ticks, so no contents move
static int grow_lists(swim_handle* h, uint64_t rcap, uint64_t pcap, uint64_t* budget, bool* grew) {
  Dev& d = h->d;
  const uint64_t need = (rcap - d.RCAP) * 32 + (pcap - d.RPCAP) * 16;
  if (need > *budget) return SWIM_OK;
  *budget -= need;
  if (rcap != d.RCAP) {
    Staged s(&h->mem);
    s.add(&d.rc_raw, rcap), s.add(&d.rc_slot, rcap), s.add(&d.rc_key, rcap), s.add(&d.rc_slot2, rcap), s.add(&d.rc_key2, rcap);
    if (!s.ok()) return alloc_failed(h);
    s.commit();
    d.RCAP = d.DCAP = (uint32_t)rcap;
    *grew = true;
  }
  if (pcap != d.RPCAP) {
    Staged s(&h->mem);
    s.add(&d.rp, pcap), s.add(&d.slow, pcap);
    if (!s.ok()) return alloc_failed(h);
    s.commit();
    d.RPCAP = d.SLOWCAP = (uint32_t)pcap;
    *grew = true;
  }
  return SWIM_OK;
}

// every entry of the incarnation history re-inserted into a table of cap2 entries (same probing as hist_push,
// gossip_dev.h: linear from its tag)
__global__ void __launch_bounds__(256) k_hist_rehash(const uint64_t* h1, uint32_t cap1, uint64_t* h2, uint32_t cap2) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cap1; i += gridDim.x * blockDim.x) {
    const uint64_t* e = h1 + (size_t)i * HREC;
    const uint64_t tag = e[0];
    if (!tag) continue;
    for (uint32_t p = 0; p < cap2; ++p) {
      unsigned long long* o = (unsigned long long*)(h2 + (size_t)((tag + p) & (cap2 - 1)) * HREC);
      if (atomicCAS(o, 0ull, (unsigned long long)tag) != 0ull) continue;
      for (uint32_t j = 1; j < HREC; ++j) o[j] = e[j];
      break;
    }
  }
}
void launch_hist_rehash(const uint64_t* h1, uint32_t cap1, uint64_t* h2, uint32_t cap2, void* stream) {
  hipLaunchKernelGGL(k_hist_rehash, dim3(2048), dim3(256), 0, (hipStream_t)stream, h1, cap1, h2, cap2);
}

// member m's held ring entries [rhead, rtail) at their positions in a ring of B2 entries (positions are absolute; a
// ring of B entries keeps position p at p & (B - 1))
__global__ void __launch_bounds__(256) k_ring_move(const uint32_t* rg, uint32_t* rg2, const uint32_t* rhead,
                                                   const uint32_t* rtail, uint32_t N, uint32_t B, uint32_t B2) {
  for (uint32_t m = blockIdx.x; m < N; m += gridDim.x) {
    const uint32_t h = rhead[m], t = rtail[m];
    for (uint32_t p = h + threadIdx.x; p - h < t - h; p += blockDim.x)
      rg2[(size_t)m * B2 + (p & (B2 - 1))] = rg[(size_t)m * B + (p & (B - 1))];
  }
}
void launch_ring_move(const uint32_t* rg, uint32_t* rg2, const uint32_t* rhead, const uint32_t* rtail, uint32_t N,
                      uint32_t B, uint32_t B2, void* stream) {
  hipLaunchKernelGGL(k_ring_move, dim3(4096), dim3(256), 0, (hipStream_t)stream, rg, rg2, rhead, rtail, N, B, B2);
}

// incarnation history: a larger table, every entry re-inserted
static int grow_history(swim_handle* h, uint64_t hcap2, uint64_t* budget, bool* grew) {
  Dev& d = h->d;
  if (8ull * hcap2 * HREC > *budget) return SWIM_OK;
  *budget -= 8 * hcap2 * HREC;
  Staged s(&h->mem);
  uint64_t* h2 = s.add(&d.hist, hcap2 * HREC);
  if (!s.ok()) return alloc_failed(h);
  HIPCK(hipMemsetAsync(h2, 0, 8 * hcap2 * HREC, h->stream));
  launch_hist_rehash(d.hist, d.HCAP, h2, (uint32_t)hcap2, h->stream);
  HIPCK(hipStreamSynchronize(h->stream));
  s.commit();
  d.HCAP = (uint32_t)hcap2;
  *grew = true;
  return SWIM_OK;
}

// receipt rings: twice the entries, every held entry moved to its position's new index
static int grow_rings(swim_handle* h, uint64_t* budget, bool* grew) {
  Dev& d = h->d;
  const uint64_t N = d.N, b2 = 2ull * d.BCAP;
  if (N * b2 * 4 > *budget) return SWIM_OK;
  *budget -= N * b2 * 4;
  Staged s(&h->mem);
  uint32_t* rg2 = s.add(&d.rg, N * b2);
  if (!s.ok()) return alloc_failed(h);
  launch_ring_move(d.rg, rg2, d.rhead, d.rtail, d.N, d.BCAP, (uint32_t)b2, h->stream);
  HIPCK(hipStreamSynchronize(h->stream));
  s.commit();
  d.BCAP = (uint32_t)b2;
  *grew = true;
  return SWIM_OK;
}

// slot table: twice the slots (whole 64-slot groups), or what the free HBM holds
static int grow_slots(swim_handle* h, uint64_t* budget, bool* grew) {
  Dev& d = h->d;
  hipStream_t st = h->stream;
  const uint64_t N = d.N;
  const uint64_t per = 2 * N + N / 4 + 64;  // S + HB + WB per slot, plus the slot arrays
  const uint64_t s2 = std::min<uint64_t>(2ull * d.SPR, std::min<uint64_t>(1ull << 22, *budget / per)) & ~63ull;
  if (s2 <= d.SPR) return SWIM_OK;
  const uint64_t s1 = d.SPR, q1 = d.QW, q2 = s2 / 64;
  // the per-tick contact rows follow the row width (SWIM_CAPS rx= at create: they keep their pinned count)
  const uint32_t crcap = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(4096, (512ull << 20) / (8ull * q2)));
  const uint32_t cr = h->rx_pinned ? d.CRCAP : crcap;
  // every allocation comes before the first write to existing device state (free_top, below)
  Staged s(&h->mem);
  uint16_t* S2 = s.add(&d.S, N * s2);
  unsigned long long *HB2 = s.add(&d.HB, N * q2), *WB2 = s.add(&d.WB, N * q2), *GU2 = s.add(&d.GU, q2), *DM2 = s.add(&d.DM, q2);
  s.add(&d.agroup, q2);
  uint64_t *gid2 = s.add(&d.slot_gid, s2), *key2 = s.add(&d.slot_key, s2);
  uint32_t *subj2 = s.add(&d.slot_subj, s2), *ct2 = s.add(&d.slot_ctick, s2), *exp2 = s.add(&d.slot_exp, s2);
  uint32_t *used2 = s.add(&d.slot_used, s2), *fl2 = s.add(&d.free_list, s2);
  s.add(&d.fexp, s2);
  s.add(&d.RX, (uint64_t)cr * q2), s.add(&d.rxl, 3ull * cr);
  if (!s.ok()) return alloc_failed(h);  // the old table stays in use
  // rows: the old columns, then zero (no holder of a new slot)
  HIPCK(hipMemcpy2DAsync(S2, 2 * s2, d.S, 2 * s1, 2 * s1, N, hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemset2DAsync(S2 + s1, 2 * s2, 0, 2 * (s2 - s1), N, st));
  HIPCK(hipMemcpy2DAsync(HB2, 8 * q2, d.HB, 8 * q1, 8 * q1, N, hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemset2DAsync(HB2 + q1, 8 * q2, 0, 8 * (q2 - q1), N, st));
  HIPCK(hipMemcpy2DAsync(WB2, 8 * q2, d.WB, 8 * q1, 8 * q1, N, hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemset2DAsync(WB2 + q1, 8 * q2, 0, 8 * (q2 - q1), N, st));
  HIPCK(hipMemsetAsync(GU2, 0, 8 * q2, st));
  HIPCK(hipMemsetAsync(DM2, 0, 8 * q2, st));
  HIPCK(hipMemcpyAsync(GU2, d.GU, 8 * q1, hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemcpyAsync(DM2, d.DM, 8 * q1, hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemcpyAsync(gid2, d.slot_gid, 8 * s1, hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemcpyAsync(key2, d.slot_key, 8 * s1, hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemcpyAsync(subj2, d.slot_subj, 4 * s1, hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemcpyAsync(ct2, d.slot_ctick, 4 * s1, hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemsetAsync(exp2, 0xFF, 4 * s2, st));  // new slots: unused, no expiry
  HIPCK(hipMemcpyAsync(exp2, d.slot_exp, 4 * s1, hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemsetAsync(used2, 0, 4 * s2, st));
  HIPCK(hipMemcpyAsync(used2, d.slot_used, 4 * s1, hipMemcpyDeviceToDevice, st));
  // free list: the new ids below the old free entries (the old ones are taken first; ids are not observable)
  int32_t top = 0;
  HIPCK(hipMemcpyAsync(&top, d.free_top, 4, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  std::vector<uint32_t> ids(s2 - s1);
  for (uint64_t i = 0; i < s2 - s1; ++i) ids[i] = (uint32_t)(s2 - 1 - i);
  HIPCK(hipMemcpyAsync(fl2, ids.data(), 4 * ids.size(), hipMemcpyHostToDevice, st));
  if (top > 0) HIPCK(hipMemcpyAsync(fl2 + ids.size(), d.free_list, 4ull * top, hipMemcpyDeviceToDevice, st));
  const int32_t top2 = top + (int32_t)ids.size();
  HIPCK(hipMemcpyAsync(d.free_top, &top2, 4, hipMemcpyHostToDevice, st));
  HIPCK(hipStreamSynchronize(st));
  s.commit();
  d.CRCAP = cr;
  d.SPR = d.SLOTS = (uint32_t)s2;
  d.QW = (uint32_t)q2;
  *grew = true;
  return SWIM_OK;
}

static int grow_caps_(swim_handle* h) {
  Dev& d = h->d;
  if (!d.rfill) return SWIM_OK;
  // (a row shard publishes only the ring fill and the history entries, grow_caps_shard: [0], [3..5] stay 0)
  const volatile uint32_t* f = h->hflag;
  const uint64_t used = f[HF_USED], fill = f[HF_FILL], nrc = f[HF_NRC], nrp = f[HF_NRP], nsl = f[HF_NSL], nhist = f[HF_NHIST];
  const uint64_t N = d.N;
  const bool gs = used > d.SPR / 2 && d.SPR < (1u << 22), gr = fill > d.BCAP / 2 && d.BCAP < (1u << 30);
  const bool grc = nrc > d.RCAP / 4 && d.RCAP < (1u << 30), grp = (nrp > d.RPCAP / 4 || nsl > d.SLOWCAP / 4) && d.RPCAP < (1u << 30);
  // the history scales with the holder states that can be reborn: the create-time rule (slots x members / 8, up to
  // 2^24) for the grown slot table, or four times the entries in use
  uint64_t hwant = d.HCAP;
  if (nhist > d.HCAP / 2) hwant = 4 * nhist;
  if (gs) hwant = std::max<uint64_t>(hwant, std::min<uint64_t>(1ull << 24, 2ull * d.SPR * N / 8));
  uint64_t hcap2 = d.HCAP;
  while (hcap2 < hwant && hcap2 < (1ull << 28)) hcap2 <<= 1;
  const bool gh = hcap2 > d.HCAP;
  if (!gs && !gr && !grc && !grp && !gh) return SWIM_OK;
  // an attempt the free HBM could not serve is not repeated every tick (each one waits for the stream): the sizes
  // that fit stay, and the next attempt is SCRUB ticks later
  if (h->tick < h->grow_next) return SWIM_OK;
  HIPCK(hipStreamSynchronize(h->stream));
  size_t fr = 0, tot = 0;
  HIPCK(hipMemGetInfo(&fr, &tot));
  const uint64_t reserve = 2ull << 30;
  uint64_t budget = fr > reserve ? fr - reserve : 0;
  bool grew = false;
  int rc;
  if (grc || grp) {
    const uint64_t rcap = grc ? std::min<uint64_t>(1ull << 30, std::max<uint64_t>(4ull * nrc, 4ull * d.RCAP)) : d.RCAP;
    const uint64_t pcap = grp ? std::min<uint64_t>(1ull << 30, 4ull * std::max<uint64_t>(d.RPCAP, std::max(nrp, nsl))) : d.RPCAP;
    if ((rc = grow_lists(h, rcap, pcap, &budget, &grew)) != SWIM_OK) return rc;
  }
  if (gh && (rc = grow_history(h, hcap2, &budget, &grew)) != SWIM_OK) return rc;
  if (gr && (rc = grow_rings(h, &budget, &grew)) != SWIM_OK) return rc;
  if (gs && (rc = grow_slots(h, &budget, &grew)) != SWIM_OK) return rc;
  if (!grew) {  // nothing fitted
    h->grow_next = h->tick + SCRUB;
    return SWIM_OK;
  }
  HIPCK(h2d(h->stream, (void*)d.self, &d, sizeof(Dev)));
  h->growths++;
  return SWIM_OK;
}

int grow_caps(swim_handle* h) {
  const int rc = grow_caps_(h);
  // a structure replaced before a later allocation failed: the device copy of Dev must name the new buffers (the old
  // ones are freed), so it is uploaded on that path too
  if (rc != SWIM_OK) (void)h2d(h->stream, (void*)h->d.self, &h->d, sizeof(Dev));
  return rc;
}

// Capacity growth on a row shard (W > 1), after a tick whose gossip plane ran: the receipt rings and the incarnation
// history hold the replicated holder state, indexed by absolute ring positions and (gid, member) tags, so each shard
// sizes them for itself. The largest ring fill (this shard's targets in k_gossip_apply, the peers' first receipts in
// k_unpack_b) and the history entries are read back here (the speculative sharded batches never run the gossip
// plane, so this costs a stream sync only on gossip ticks). Slot ids are global (owner = id / SPR) and the per-tick
// lists feed fixed-size exchange regions, so those keep the sizes the config gives them.
int grow_caps_shard(swim_handle* h) {
  Dev& d = h->d;
  if (!d.rfill) return SWIM_OK;
  uint32_t v[2] = {0, 0};
  HIPCK(hipMemcpyAsync(&v[0], d.rfill, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipMemcpyAsync(&v[1], d.hist_n, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipMemsetAsync(d.rfill, 0, 4, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  volatile uint32_t* f = h->hflag;
  f[HF_USED] = 0;  // slots: not grown on a shard
  f[HF_FILL] = v[0];
  f[HF_NRC] = f[HF_NRP] = f[HF_NSL] = 0;
  f[HF_NHIST] = v[1];
  return grow_caps(h);
}

}  // namespace swim
