// group.hip — swim_config.n_gpus > 1: the group handle's creation, stepping and in-process host exchange (group.h).
#include "group.h"

#include <chrono>
#include <cstring>
#include <thread>

using namespace swim;

namespace swim {

static bool group_barrier(Group* g) {
  std::unique_lock<std::mutex> lk(g->mu);
  if (g->abort) return false;
  const uint64_t my = g->gen;
  if (++g->arrived == g->shards.size()) {
    g->arrived = 0;
    g->gen++;
    g->cv.notify_all();
    return true;
  }
  const bool ok = g->cv.wait_for(lk, std::chrono::seconds(600), [&] { return g->gen != my || g->abort; });
  return ok && !g->abort;
}

static void group_abort(Group* g) {
  std::lock_guard<std::mutex> lk(g->mu);
  g->abort = true;
  g->cv.notify_all();
}

// swim_exchange_fn of the in-process transport (the contract of swimhip_shard.h)
static int group_exchange(void* ctx, const void* send, const uint64_t* sb, void* recv, uint64_t cap, uint64_t* rb) {
  const Group::End* e = (const Group::End*)ctx;
  Group* g = e->g;
  const uint32_t W = (uint32_t)g->shards.size(), r = e->rank;
  g->blocks[r].data = (const uint8_t*)send;
  g->blocks[r].words.assign(sb, sb + W);
  if (!group_barrier(g)) return -1;
  uint64_t out = 0;
  for (uint32_t p = 0; p < W; ++p) {
    const Group::Block& B = g->blocks[p];
    uint64_t off = 0;
    for (uint32_t q = 0; q < r; ++q) off += B.words[q] & SWIM_XCOUNT_MASK;
    const uint64_t n = B.words[r] & SWIM_XCOUNT_MASK;
    if (out + n > cap) {
      group_abort(g);
      return -1;
    }
    if (n) std::memcpy((uint8_t*)recv + out, B.data + off, n);
    out += n;
    rb[p] = B.words[r];
  }
  return group_barrier(g) ? 0 : -1;  // every peer has copied before the send buffers are reused
}

int create_group(const swim_config* cfg, swim_handle** out) {
  const uint32_t W = cfg->n_gpus;
  if (W > 64 || W > cfg->n_members / 2) return SWIM_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= (int)cfg->device) return SWIM_EDEVICE;
  auto* h = new swim_handle();
  h->cfg = *cfg;
  Group* g = h->grp = new Group();
  const bool rccl = (uint64_t)cfg->device + W <= (uint64_t)ndev && !getenv("SWIM_GROUP_HOST");
  g->transport = rccl ? SWIM_TRANSPORT_RCCL : SWIM_TRANSPORT_HOST;
  g->shards.assign(W, nullptr);
  g->blocks.resize(W);
  for (uint32_t r = 0; r < W; ++r) g->ends.push_back(Group::End{g, r});
  std::vector<int> rc(W, SWIM_OK);
  auto make = [&](uint32_t r, const uint8_t* id) {
    swim_config c = *cfg;
    c.n_gpus = 1;
    c.device = rccl ? cfg->device + r : cfg->device + r % (uint32_t)(ndev - (int)cfg->device);
    swim_shard_spec sp{};
    sp.rank = r;
    sp.world = W;
    sp.transport = g->transport;
    if (rccl) {
      std::memcpy(sp.rccl_id, id, 128);
    } else {
      sp.exchange = group_exchange;
      sp.ctx = &g->ends[r];
    }
    rc[r] = create(&c, &sp, &g->shards[r]);
  };
  if (rccl) {  // ncclCommInitRank is collective: every rank's call runs on its own thread
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) {
      swim_destroy(h);
      return SWIM_EDEVICE;
    }
    std::vector<std::thread> th;
    for (uint32_t r = 0; r < W; ++r) th.emplace_back(make, r, (const uint8_t*)&id);
    for (auto& t : th) t.join();
  } else {
    for (uint32_t r = 0; r < W; ++r) make(r, nullptr);
  }
  for (uint32_t r = 0; r < W; ++r)
    if (rc[r] != SWIM_OK) {
      swim_destroy(h);
      return rc[r];
    }
  for (swim_handle* s : g->shards) {
    g->lo.push_back(s->d.lo);
    g->hi.push_back(s->d.hi);
  }
  g->slots = g->shards[0]->d.XW > 1;
  g->evcount.assign(g->slots ? cfg->n_members : 0, 0);
  h->d = g->shards[0]->d;  // constants only (N, ping_t, ...): the group handle itself launches nothing
  *out = h;
  return SWIM_OK;
}

// the shards in lockstep, one host thread each (their exchanges meet inside swim_step)
int group_step(swim_handle* h, uint32_t n) {
  Group* g = h->grp;
  std::vector<int> rc(g->shards.size(), SWIM_OK);
  std::vector<std::thread> th;
  for (size_t r = 0; r < g->shards.size(); ++r)
    th.emplace_back([&, r] {
      rc[r] = swim_step(g->shards[r], n);
      if (rc[r] != SWIM_OK) group_abort(g);  // peers waiting in an exchange give up
    });
  for (auto& t : th) t.join();
  h->tick = g->shards[0]->tick;
  for (size_t r = 0; r < rc.size(); ++r)
    if (rc[r] != SWIM_OK && g->shards[r]->err.size())
      return fail(h, rc[r], "shard " + std::to_string(r) + ": " + g->shards[r]->err);
  for (size_t r = 0; r < rc.size(); ++r)
    if (rc[r] != SWIM_OK) return fail(h, rc[r], "shard " + std::to_string(r) + " failed in a peer's exchange");
  return SWIM_OK;
}

void group_destroy(swim_handle* h) {
  for (swim_handle* s : h->grp->shards)
    if (s) swim_destroy(s);
  delete h->grp;
  delete h;
}

}  // namespace swim
