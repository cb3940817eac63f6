// member_kernels.h — the member-control kernels as their launcher (kernels.hip launch_member, launch_tick_a) names them.
#pragma once
#include <hip/hip_runtime.h>

#include "engine.h"

namespace swim {

// k_member_tick_t's mode: BODY_FULL = the whole tick; BODY_SPLIT = the whole tick, except that a member with at least
// Dev::hv routed gossip receipts stops before P4 and is listed for k_inbox_apply (P4, a wave per member) and the
// resumed launch; BODY_RESUME = P5 and P6 of a listed member (its P0-P4 ran in the two launches before)
enum : uint32_t { BODY_FULL = 0, BODY_SPLIT = 1, BODY_RESUME = 2 };
template <uint32_t MODE>
__global__ void k_member_tick_t(const Dev* __restrict__ dp, uint32_t k, uint32_t flag);  // member.hip
__global__ void k_inbox_apply(const Dev* __restrict__ dp, uint32_t k);                   // inbox.hip

}  // namespace swim
