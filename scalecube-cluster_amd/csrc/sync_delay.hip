// sync_delay.hip — the delayed-SYNC store (link delays): a SYNC / SYNC_ACK whose link delays it past the next tick
// waits here, with its payload as sent, until the tick before its delivery.
//
// One GPU: after the member kernel of tick k, the stored messages due in tick k + 1 go back into this tick's buffer
// (k_sync_redeliver<false>), then the delayed messages of this tick go into the store (k_sync_defer<false>; k_sync_diff
// of the next tick skips them).
// Row-sharded handles (W > 1): a delayed message travels to its receiver's shard in the tick it is sent (the route and
// exchange A carry it like any other message, flagged KF_DEFER, and msgs_commit leaves it out of the inbound lists); the
// receiver's shard stores it with its payload as sent at the end of that tick (k_sync_defer<true>, after k_unpack_a),
// and puts it back into the inbound list of the tick before its delivery while that list is assembled
// (k_sync_redeliver<true>, before the list is committed).
// A launch of a speculative batch returns at once by the rules of spec.h.
#include <hip/hip_runtime.h>

#include "dev_util.h"

namespace swim {

template <bool SHARDED>
__global__ void __launch_bounds__(256) k_sync_redeliver(Dev d, uint32_t k, uint32_t spec) {
  // one GPU: halt = k + 1 is this tick's member kernel's (it ran, and its delayed messages still move); a diff-halt at
  // this tick or earlier: member(k) did not run
  if (spec && (SHARDED ? halted_before(d.halt, k) : halted_member(d.halt, k))) return;
  __shared__ uint32_t slot[2];
  const uint32_t b = k & 1;
  for (uint32_t e = blockIdx.x; e < d.DSCAP; e += gridDim.x) {
    if (!d.ds_used[e] || d.ds_msg[e].due != k + 1u) continue;
    if (threadIdx.x == 0) {
      slot[0] = SHARDED ? atomicAdd(&d.xn[4], 1u) : msg_take(d, b);  // (one lane: its wave's shard, msg_slots.h)
      slot[1] = atomicAdd(&d.arena_used[b], 1u);
      if (slot[0] >= d.MSGCAP) set_err(d, E_MSGS);
      if (slot[1] >= d.ARENA_ROWS) set_err(d, E_ARENA);
    }
    __syncthreads();
    const uint32_t i = slot[0], r = slot[1];
    if (i < d.MSGCAP && r < d.ARENA_ROWS) {
      const uint32_t* src = d.ds_row + (size_t)e * d.NS;
      uint32_t* dst = d.arena[b] + (size_t)r * d.NS;
      for (uint32_t s = threadIdx.x; s < d.NS; s += blockDim.x) dst[s] = src[s];
      if constexpr (!SHARDED) __syncthreads();
      if (threadIdx.x == 0) {
        SyncMsg m = d.ds_msg[e];
        m.kind = (m.kind & ~KF_DEFER) | KF_LATE;
        m.payload = r;
        m.ncand = 0;
        m.pad = NEVER;
        m.pin = NEVER;
        if (!SHARDED && spec) note_wrote(d.halt, k);  // a snapshot payload in the next tick's lists (spec.h)
        if constexpr (SHARDED) {  // the inbound list of the next tick while it is assembled
          d.mtmp[i] = m;
        } else {
          d.msgs[b][i] = m;
          const uint32_t old = atomicExch(&d.m_head[(size_t)b * d.N + m.dst], i);
          d.m_next[(size_t)b * d.MSGCAP + i] = old;
          if (old != NEVER) {
            pin_msg(d, b, i);
            pin_msg(d, b, old);
          }
        }
      }
    }
    if (threadIdx.x == 0) {
      d.ds_used[e] = 0;
      d.ds_free[atomicAdd(d.ds_top, 1)] = e;
    }
    __syncthreads();
  }
}

template <bool SHARDED>
__global__ void __launch_bounds__(256) k_sync_defer(Dev d, uint32_t k, uint32_t spec) {
  // row shards: this tick's list was not committed when the batch halted at it or earlier
  if (spec && (SHARDED ? halted_uncommitted(d.halt, k) : halted_member(d.halt, k))) return;
  __shared__ int32_t slot;
  __shared__ uint32_t mfill[MSG_SHARDS_MAX];
  const uint32_t b = k & 1;
  // this tick's messages: the buffer's slots in use (msg_slots.h; a row shard's list is dense, msh == 1)
  const MsgWalk mw = msg_walk_block(d.ctr_sh, d.msh, d.MSGCAP, b, d.nmsg[b], mfill);
  for (uint32_t j = blockIdx.x; j < mw.E.total; j += gridDim.x) {
    const uint32_t i = msg_at(mw, mfill, j);
    if (i == NEVER) continue;  // (block-uniform)
    const SyncMsg mm = d.msgs[b][i];
    if (!(mm.kind & KF_DEFER)) continue;
    if (threadIdx.x == 0) {
      const int32_t top = atomicSub(d.ds_top, 1) - 1;
      slot = top >= 0 ? (int32_t)d.ds_free[top] : -1;
      if (top < 0) set_err(d, E_SYNCQ);
    }
    __syncthreads();
    const int32_t e = slot;
    if (e >= 0) {  // the payload as sent: the sender's row at the end of the tick, or its copy-on-write snapshot, or
                   // (row shards) the chunks a peer shipped over the baseline row
      uint32_t* dst = d.ds_row + (size_t)e * d.NS;
      if (SHARDED && mm.payload & PAY_RX && mm.payload != NEVER) {
        const uint32_t ri = mm.payload & ~PAY_RX;
        const uint64_t* mk = d.rx_mask + (size_t)ri * d.MW;
        const uint32_t* data = (const uint32_t*)(d.xa_recv + d.rx_off[ri]);
        for (uint32_t s = threadIdx.x; s < d.NS; s += blockDim.x) {
          const uint32_t c = s / CH;
          uint32_t v = d.base_row[s];
          if ((mk[c >> 6] >> (c & 63)) & 1ull) {
            uint32_t rank = __popcll(mk[c >> 6] & ((1ull << (c & 63)) - 1ull));
            for (uint32_t q = 0; q < (c >> 6); ++q) rank += __popcll(mk[q]);
            v = data[(size_t)rank * CH + s % CH];
          }
          dst[s] = v;
        }
      } else {
        const uint32_t* src = mm.payload == NEVER ? d.rowk + lidx(d, mm.src) * d.NS : d.arena[b] + (size_t)mm.payload * d.NS;
        for (uint32_t s = threadIdx.x; s < d.NS; s += blockDim.x) dst[s] = src[s];
      }
      if (threadIdx.x == 0) {
        d.ds_msg[e] = mm;
        d.ds_used[e] = 1;
      }
    }
    __syncthreads();
  }
}

void launch_sync_redeliver(const Dev& d, uint32_t k, hipStream_t st, bool spec) {
  auto* kern = d.W > 1 ? k_sync_redeliver<true> : k_sync_redeliver<false>;
  hipLaunchKernelGGL(kern, dim3(256), dim3(256), 0, st, d, k, spec ? 1u : 0u);
}
void launch_sync_defer(const Dev& d, uint32_t k, hipStream_t st, bool spec) {
  auto* kern = d.W > 1 ? k_sync_defer<true> : k_sync_defer<false>;
  hipLaunchKernelGGL(kern, dim3(256), dim3(256), 0, st, d, k, spec ? 1u : 0u);
}

}  // namespace swim
