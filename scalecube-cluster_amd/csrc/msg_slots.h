// msg_slots.h — how the slots of a tick's SYNC message buffer msgs[b] (and with it m_next, chunk_meta, mlog) are handed
// out to the senders and enumerated by the readers. Said once, for the device and for the host (no HIP type: a plain
// C++ program can include it, tests/test_msg_slots_host.py).
//
// One counter for the whole buffer made every sending wave of the member kernel queue on one word (~420 returning
// atomics per tick at 100k members). With S > 1 shards (a power of two, at most
// MSG_SHARDS_MAX) the buffer of MSGCAP slots is cut in two regions:
//   fast      [0, R), R = S * Q, Q = MSGCAP / (4 S): shard s's j-th slot (j < Q) is j * S + s. A sender's shard follows
//             from its wave's place in the grid; each shard has a counter of its own, on a 128-B line of its own
//             (word MSG_CTR_WORD + b of counter row s + 1, engine.h).
//   overflow  [R, MSGCAP): handed out in order by the buffer's old counter nmsg[b], which counts overflow entries only.
//             A sender whose shard index reaches Q takes one.
// With S == 1 there is no fast region (Q = R = 0): every slot comes from nmsg[b], in order, as before the shards.
//
// A shard's counter goes on counting past Q (it is never taken back): its slots in use are min(counter, Q).
//
// Readers of "the messages of buffer b" walk positions j = 0 .. total - 1 (msg_enum):
//   c_max = max over the shards of min(counter_s, Q)
//   j <  S * c_max   slot j, of shard j % S, in use iff j / S < min(counter_[j % S], Q)   (else a hole: skipped)
//   j >= S * c_max   overflow slot R + (j - S * c_max), up to min(nmsg[b], MSGCAP - R) of them
// Positions ascend with the slots.
// A reader that needs no order and has a lane per shard may skip the holes (msg_dense_slot): the q-th message is shard
// s's j-th fast slot, where the shards' fills before s sum to q - j (shard-major), and past the fast messages the
// overflow slots in order. The lister does (k_ack_resolve: the sending waves of a block sit in its waves 1 and 3, so
// half the shards stay empty and half the fast positions are holes).
//
// Capacity. With the senders spread evenly over the shards nothing changes. Under skew a shard's demand beyond Q goes to
// the overflow region, MSGCAP - R slots (about three quarters of MSGCAP) shared by all: E_MSGS fires once the overflow
// demand exceeds that, so a single shard can be served Q + (MSGCAP - R) messages where the unsharded buffer held MSGCAP.
// Handles whose traffic comes from one lane (a cold join's seed answers every member's SYNC) therefore stay unsharded
// unless SWIM_MSG_SHARDS asks otherwise (create.hip).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MSG_HD __host__ __device__ __forceinline__
#else
#define MSG_HD inline
#endif

namespace swim {

constexpr uint32_t MSG_SHARDS_MAX = 32;    // shards of a sharded handle (Dev::msh), and the most SWIM_MSG_SHARDS takes
constexpr uint32_t MSG_SHARD_MIN_N = 8192; // members from which a handle is sharded by default
constexpr uint32_t MSG_CTR_WORD = 16;      // shard s, buffer b: word MSG_CTR_WORD + b of counter row s + 1 (its low half)

struct MsgLayout {
  uint32_t S, sh;  // shards (1: off) and log2 of it
  uint32_t Q, R;   // fast slots per shard, fast region [0, R)
  uint32_t cap;    // MSGCAP
};
MSG_HD MsgLayout msg_layout(uint32_t msgcap, uint32_t shards) {
  MsgLayout L;
  L.S = shards > 1u ? shards : 1u;  // (0: a Dev built by hand, without counter rows)
  L.sh = (uint32_t)__builtin_ctz(L.S);
  L.Q = L.S > 1u ? msgcap >> (2u + L.sh) : 0u;
  L.R = L.Q << L.sh;
  L.cap = msgcap;
  return L;
}
// a power of two from 1 to MSG_SHARDS_MAX
MSG_HD bool msg_shards_ok(uint32_t s) { return s >= 1u && s <= MSG_SHARDS_MAX && (s & (s - 1u)) == 0u; }

// shard s's j-th fast slot (j < Q)
MSG_HD uint32_t msg_fast_slot(const MsgLayout& L, uint32_t s, uint32_t j) { return (j << L.sh) | s; }
// the o-th overflow slot; cap when the region is full (the sender raises E_MSGS and stores nothing)
MSG_HD uint32_t msg_over_slot(const MsgLayout& L, uint32_t o) { return o < L.cap - L.R ? L.R + o : L.cap; }
// a shard's fast slots in use
MSG_HD uint32_t msg_fill(const MsgLayout& L, uint32_t counter) { return counter < L.Q ? counter : L.Q; }

// the readers' enumeration: positions [0, total), the first nfast of them in the fast region
struct MsgEnum {
  uint32_t nfast, total;
};
MSG_HD MsgEnum msg_enum(const MsgLayout& L, uint32_t c_max, uint32_t nover) {
  MsgEnum E;
  E.nfast = c_max << L.sh;
  E.total = E.nfast + (nover < L.cap - L.R ? nover : L.cap - L.R);
  return E;
}
MSG_HD uint32_t msg_pos_shard(const MsgLayout& L, uint32_t j) { return j & (L.S - 1u); }
MSG_HD uint32_t msg_pos_slot(const MsgLayout& L, const MsgEnum& E, uint32_t j) {
  return j < E.nfast ? j : L.R + (j - E.nfast);
}
// fill: msg_fill of shard msg_pos_shard(j) (read only for a fast position)
MSG_HD bool msg_pos_used(const MsgLayout& L, const MsgEnum& E, uint32_t j, uint32_t fill) {
  return j >= E.nfast || (j >> L.sh) < fill;
}

// the walk again from the three numbers a reader may keep of it (log2 of the shards, R, the fast positions): every field
// msg_pos_shard, msg_pos_used and msg_pos_slot read; Q, cap and the total are not kept (0)
MSG_HD void msg_walk_from(uint32_t sh, uint32_t R, uint32_t nfast, MsgLayout& L, MsgEnum& E) {
  L.S = 1u << sh, L.sh = sh, L.Q = 0u, L.R = R, L.cap = 0u;
  E.nfast = nfast, E.total = 0u;
}

// the dense walk's q-th message (q < the fills' sum + the overflow slots in use), from the shards' counters: serial here,
// by a prefix sum over the lanes on the device (msg_walk_wave, dev_util.h)
MSG_HD uint32_t msg_dense_slot(const MsgLayout& L, const uint32_t* counter, uint32_t q) {
  uint32_t before = 0;
  for (uint32_t s = 0; L.S > 1u && s < L.S; ++s) {
    const uint32_t f = msg_fill(L, counter[s]);
    if (q < before + f) return msg_fast_slot(L, s, q - before);
    before += f;
  }
  return L.R + (q - before);
}

// ---- host side: one take at a time, and the walk over counters read back from the device ----
// what a sender of shard s gets (the device does the same for a wave's lanes at once, msg_take in dev_util.h): its slot,
// or cap when it needed an overflow slot and none was left (E_MSGS). counter: [S], nover: nmsg[b].
inline uint32_t msg_take_serial(const MsgLayout& L, uint32_t* counter, uint32_t* nover, uint32_t s) {
  if (L.S > 1u) {
    const uint32_t j = counter[s]++;
    if (j < L.Q) return msg_fast_slot(L, s, j);
  }
  return msg_over_slot(L, (*nover)++);
}
// f(slot) for every slot in use, ascending; returns how many. counter: [S] (unused with S == 1)
template <class F>
inline uint32_t msg_for_each(const MsgLayout& L, const uint32_t* counter, uint32_t nover, F f) {
  uint32_t c_max = 0, n = 0;
  for (uint32_t s = 0; L.S > 1u && s < L.S; ++s) c_max = msg_fill(L, counter[s]) > c_max ? msg_fill(L, counter[s]) : c_max;
  const MsgEnum E = msg_enum(L, c_max, nover);
  for (uint32_t j = 0; j < E.total; ++j) {
    if (!msg_pos_used(L, E, j, j < E.nfast ? msg_fill(L, counter[msg_pos_shard(L, j)]) : 0u)) continue;
    f(msg_pos_slot(L, E, j));
    ++n;
  }
  return n;
}

}  // namespace swim
