// exchange.hip — the shard exchanges (row sharding: A and B; slot sharding: the gossip-count all-reduce) over RCCL or
// the host callback of swimhip_shard.h.
#include "handle.h"

#include <chrono>
#include <cstring>

using namespace swim;

namespace swim {

// The host waits for the end of every tick's exchange A. A blocking event wait falls back to an interrupt after a
// short active phase, and that wake-up would stall the GPU, which has nothing queued behind the exchange: spin.
static hipError_t spin_wait(hipEvent_t ev) {
  hipError_t e;
  while ((e = hipEventQuery(ev)) == hipErrorNotReady) {
  }
  return e;
}

// RCCL, fixed-size part of an exchange: the inline all-to-all and its unpacking into the regions (k_inline_in also
// publishes the count words to the host-mapped xi_host)
int exchange_inline(swim_handle* h, uint8_t* recv, uint64_t cap, unsigned long long* scnt, unsigned long long* rcnt,
                    bool spec) {
  if (ncclAllToAll(h->d.xi_send, h->d.xi_recv, h->d.XI, ncclUint8, h->comm, h->stream) != ncclSuccess) {
    h->err = "ncclAllToAll (inline exchange) failed";
    return SWIM_EDEVICE;
  }
  launch_inline_in(h->d, recv, cap, scnt, rcnt, h->stream, spec);
  return SWIM_OK;
}

// RCCL, after the inline part has completed: the count words from xi_host (the gossip flag, the sizes) and a
// send/recv group for the regions that did not fit inline
int exchange_rest(swim_handle* h, uint8_t* send, uint8_t* recv, uint64_t cap) {
  const uint32_t W = h->d.W, me = h->d.rank;
  unsigned long long* hc = h->hcnt;
  volatile unsigned long long* xh = h->d.xi_host;
  for (uint32_t q = 0; q < 2 * W; ++q) hc[q] = xh[q];
  h->xflag = false;
  bool rest = false;
  for (uint32_t q = 0; q < 2 * W; ++q) {
    h->xflag |= (hc[q] & XFLAG_GOSSIP) != 0;
    rest |= (hc[q] & XCNT_MASK) > h->d.XI - 8;
    if ((hc[q] & XCNT_MASK) > cap) {
      h->err = "exchange block larger than its region";
      return SWIM_ECAPACITY;
    }
  }
  if (rest) {
    bool ok = ncclGroupStart() == ncclSuccess;
    for (uint32_t q = 0; q < W && ok; ++q) {
      if (q == me) continue;
      const uint64_t sb = hc[q] & XCNT_MASK, rb = hc[W + q] & XCNT_MASK;
      const uint64_t X = h->d.XI - 8;
      if (sb > X) ok &= ncclSend(send + (size_t)q * cap + X, sb - X, ncclUint8, (int)q, h->comm, h->stream) == ncclSuccess;
      if (rb > X) ok &= ncclRecv(recv + (size_t)q * cap + X, rb - X, ncclUint8, (int)q, h->comm, h->stream) == ncclSuccess;
    }
    ok &= ncclGroupEnd() == ncclSuccess;
    if (!ok) {
      h->err = "RCCL send/recv group failed";
      return SWIM_EDEVICE;
    }
  }
  return SWIM_OK;
}

// one all-to-all of per-peer byte blocks (fixed-capacity regions of `cap` bytes in send / recv, rank order).
// The byte counts are device-resident (written by the pack kernels); the transport needs them on the host.
int exchange(swim_handle* h, uint8_t* send, uint8_t* recv, uint64_t cap, unsigned long long* scnt,
             unsigned long long* rcnt, bool inline_packed) {
  const uint32_t W = h->d.W;
  hipStream_t st = h->stream;
  unsigned long long* hc = h->hcnt;
  auto t0 = std::chrono::steady_clock::now();
  if (h->spec.transport == SWIM_TRANSPORT_RCCL) {
    // one fixed-size all-to-all (count word + the first XINL - 8 bytes of each region), one host read of the
    // count words through mapped memory, and a send/recv group only for regions that did not fit
    if (!inline_packed) launch_inline_out(h->d, send, cap, scnt, st);  // exchange A: k_pack_all wrote them
    int rc;
    if ((rc = exchange_inline(h, recv, cap, scnt, rcnt, false)) != SWIM_OK) return rc;
    HIPCK(hipEventRecord(h->ev_member, st));
    HIPCK(spin_wait(h->ev_member));
    if ((rc = exchange_rest(h, send, recv, cap)) != SWIM_OK) return rc;
  } else {
    HIPCK(hipMemcpyAsync(hc, scnt, 8ull * W, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    uint64_t off = 0;
    for (uint32_t q = 0; q < W; ++q) {
      const uint64_t sb = hc[q] & XCNT_MASK;
      if (sb > cap) {
        h->err = "exchange block larger than its region";
        return SWIM_ECAPACITY;
      }
      if (sb) HIPCK(hipMemcpyAsync(h->hsend.data() + off, send + (size_t)q * cap, sb, hipMemcpyDeviceToHost, st));
      off += sb;
    }
    HIPCK(hipStreamSynchronize(st));
    uint64_t sb[64], rb[64];
    for (uint32_t q = 0; q < W; ++q) sb[q] = hc[q], rb[q] = 0;
    if (h->spec.exchange(h->spec.ctx, h->hsend.data(), sb, h->hrecv.data(), h->hrecv.size(), rb) != 0) {
      h->err = "host exchange callback failed";
      return SWIM_EDEVICE;
    }
    off = 0;
    h->xflag = false;
    for (uint32_t p = 0; p < W; ++p) {
      const uint64_t n = rb[p] & XCNT_MASK;
      if (n > cap) {
        h->err = "received exchange block larger than its region";
        return SWIM_ECAPACITY;
      }
      if (n) HIPCK(hipMemcpyAsync(recv + (size_t)p * cap, h->hrecv.data() + off, n, hipMemcpyHostToDevice, st));
      off += n;
      hc[W + p] = rb[p];
      h->xflag |= ((rb[p] | sb[p]) & XFLAG_GOSSIP) != 0;
    }
    HIPCK(hipMemcpyAsync(rcnt, hc + W, 8ull * W, hipMemcpyHostToDevice, st));
    HIPCK(hipStreamSynchronize(st));
  }
  h->xchg_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SWIM_OK;
}

// slot sharding: sum the shards' gossip-count deltas of this tick and apply them (k_held_add). RCCL: one in-place
// all-reduce on the stream. HOST: every shard sends its delta vector to every peer and sums what it receives.
int held_allreduce(swim_handle* h) {
  Dev& d = h->d;
  hipStream_t st = h->stream;
  auto t0 = std::chrono::steady_clock::now();
  if (h->lone) {
    launch_held_add(d, d.held_delta, st);
  } else if (h->spec.transport == SWIM_TRANSPORT_RCCL) {
    if (ncclAllReduce(d.held_delta, d.held_delta, d.N, ncclInt32, ncclSum, h->comm, st) != ncclSuccess) {
      h->err = "ncclAllReduce (gossip counts) failed";
      return SWIM_EDEVICE;
    }
    launch_held_add(d, d.held_delta, st);
  } else {
    const uint64_t bytes = 4ull * d.N;
    HIPCK(hipMemcpyAsync(h->hsend.data(), d.held_delta, bytes, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (uint32_t q = 1; q < d.XW; ++q) std::memcpy(h->hsend.data() + q * bytes, h->hsend.data(), bytes);
    uint64_t sb[64], rb[64];
    for (uint32_t q = 0; q < d.XW; ++q) sb[q] = q == d.xrank ? 0 : bytes, rb[q] = 0;
    if (h->spec.exchange(h->spec.ctx, h->hsend.data(), sb, h->hrecv.data(), h->hrecv.size(), rb) != 0) {
      h->err = "host exchange callback failed";
      return SWIM_EDEVICE;
    }
    std::vector<int32_t> sum((size_t)d.N);
    std::memcpy(sum.data(), h->hsend.data(), bytes);
    uint64_t off = 0;
    for (uint32_t p = 0; p < d.XW; ++p) {
      const uint64_t n = rb[p] & XCNT_MASK;
      if (n != (p == d.xrank ? 0 : bytes)) {
        h->err = "gossip-count exchange: unexpected block size";
        return SWIM_EDEVICE;
      }
      const int32_t* v = (const int32_t*)(h->hrecv.data() + off);
      for (uint32_t m = 0; m < n / 4; ++m) sum[m] += v[m];
      off += n;
    }
    HIPCK(hipMemcpyAsync(d.held_delta, sum.data(), bytes, hipMemcpyHostToDevice, st));
    launch_held_add(d, d.held_delta, st);
    HIPCK(hipStreamSynchronize(st));
  }
  h->xchg_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SWIM_OK;
}

}  // namespace swim
