// member_kernels.h — the member-control kernels as their launcher (kernels.hip launch_member, launch_tick_a) names them.
#pragma once
#include <hip/hip_runtime.h>

#include "engine.h"

namespace swim {

// k_member_tick_t's mode: BODY_FULL = the whole tick; BODY_SPLIT = the whole tick, except that a member with at least
// Dev::hv routed gossip receipts stops before P4 and is listed for k_inbox_apply (P4, a wave per member) and the
// resumed launch; BODY_RESUME = P5 and P6 of a listed member (its P0-P4 ran in the two launches before)
enum : uint32_t { BODY_FULL = 0, BODY_SPLIT = 1, BODY_RESUME = 2 };

// What the front of k_member_tick_t<BODY_FULL> reads before its first wait, as a kernel argument: the triage's thirteen
// arrays, the halt words' address and the launch's member range. Read out of Dev in memory, each pointer is a scalar
// load behind the load of dp, the loads through it are FLAT (the compiler cannot know the space), and the thirteen issue
// in groups behind the pointers' waits; as an argument they are in scalar registers when the wave starts and the loads
// are global loads with scalar bases. The host fills it from its copy of Dev at enqueue (member_front): every field is
// one that cannot change between enqueue and execution. Nothing on the device writes Dev, the arrays are allocated at
// create for the handle's N and never move (what grows, at host waits with the stream idle, are capacities of the
// gossip plane and the pools, none of them here), and lo, hi and N are fixed at create. The words the device does change
// stay loads (the halt words, through `halt`). Small, and consumed only by force-inlined code: a by-value struct whose
// address escapes is copied into per-lane scratch.
struct MemberFront {
  const uint32_t *m_head, *rc_cnt, *pending_inc, *next_evt, *timerMin, *nextPing, *nextSync, *initFlags, *nextGossip, *held,
      *dead_tick, *start_tick, *rc_ndrop;
  const uint32_t* halt;
  uint32_t lo, hi, N;  // hi >= 1 (a launch has blocks only over a range that holds a member)
  uint32_t exp;        // Dev::exp (SWIM_EXP, fixed at create): whether the entry stamp is read at all
};
inline MemberFront member_front(const Dev& d) {
  return MemberFront{d.m_head, d.rc_cnt, d.pending_inc, d.next_evt, d.timerMin, d.nextPing, d.nextSync, d.initFlags,
                     d.nextGossip, d.held, d.dead_tick, d.start_tick, d.rc_ndrop, d.halt, d.lo, d.hi, d.N, d.exp};
}

// f: read by BODY_FULL only
template <uint32_t MODE>
__global__ void k_member_tick_t(const Dev* __restrict__ dp, uint32_t k, uint32_t flag, const MemberFront f);  // member.hip
__global__ void k_inbox_apply(const Dev* __restrict__ dp, uint32_t k);                   // inbox.hip

}  // namespace swim
