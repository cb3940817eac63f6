// group.h — private: one handle over several GPUs (swim_config.n_gpus = W > 1), group.hip.
#pragma once
#include <condition_variable>
#include <mutex>

#include "handle.h"

// ---------------------------------------------------------------------------------------------------------------
// One handle over several GPUs (swim_config.n_gpus = W > 1; SURVEY.md §8b: "RCCL communicators created in
// swim_create", ClusterConfig unchanged for the caller). The handle owns W row-sharded shard handles
// (swimhip_shard.h), one per device, and forwards every call: stepping runs the shards on W host threads in
// lockstep; fault injection goes to every shard; readback goes to the owning shard (rows, lists, gossips) or is
// summed / merged over them (hashes, counters, events), exactly as a multi-process deployment would combine them.
// Transport: RCCL between W distinct devices (one communicator per shard, initialised together); on a node with
// fewer devices (the single-GPU test box) the shards share the devices and exchange through host memory inside this
// process (SWIM_GROUP_HOST=1 forces that).
struct Group {
  std::vector<swim_handle*> shards;
  std::vector<uint32_t> lo, hi;
  uint32_t transport = SWIM_TRANSPORT_HOST;
  // in-process host exchange: each rank deposits its blocks, waits for all, copies its own, waits again
  std::mutex mu;
  std::condition_variable cv;
  uint32_t arrived = 0;
  uint64_t gen = 0;
  bool abort = false;
  struct Block {
    const uint8_t* data = nullptr;
    std::vector<uint64_t> words;
  };
  std::vector<Block> blocks;
  struct End {
    Group* g;
    uint32_t rank;
  };
  std::vector<End> ends;
  std::vector<swim_event> events;
  bool slots = false;             // slot-sharded (RUMOR mode): every shard runs every member, gossips are split
  std::vector<uint32_t> evcount;  // slot-sharded: events per observer drained so far (the merged seq)
};

namespace swim {
#pragma GCC visibility push(hidden)

// run f on every shard (on its device), in rank order; the first error is the group's
template <class F>
int group_all(swim_handle* h, F f) {
  Group* g = h->grp;
  for (size_t r = 0; r < g->shards.size(); ++r) {
    hipSetDevice((int)g->shards[r]->cfg.device);
    const int rc = f(g->shards[r]);
    if (rc != SWIM_OK) return fail(h, rc, "shard " + std::to_string(r) + ": " + g->shards[r]->err);
  }
  return SWIM_OK;
}

// run f on the shard that owns observer m
template <class F>
int group_owner(swim_handle* h, uint32_t m, F f) {
  Group* g = h->grp;
  for (size_t r = 0; r < g->shards.size(); ++r)
    if (m >= g->lo[r] && m < g->hi[r]) {
      hipSetDevice((int)g->shards[r]->cfg.device);
      const int rc = f(g->shards[r]);
      if (rc != SWIM_OK) return fail(h, rc, "shard " + std::to_string(r) + ": " + g->shards[r]->err);
      return rc;
    }
  return SWIM_EINVAL;
}

#pragma GCC visibility pop
}  // namespace swim

#define GROUP_ALL(call)                                            \
  if (h && h->grp) return group_all(h, [&](swim_handle* s) { return call; })
#define GROUP_OWNER(m, call)                                       \
  if (h && h->grp) return group_owner(h, (m), [&](swim_handle* s) { return call; })
