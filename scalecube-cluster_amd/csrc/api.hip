// api.hip — the C ABI of libswimhip (include/swimhip.h) apart from swim_step (step.hip): creation and destruction,
// fault injection, readback.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/swimhip_wire.h"
#include "../../include/swimhip_debug.h"
#include "../../include/swimhip_census.h"
#include "group.h"

using namespace swim;

namespace swim {

int check_err(swim_handle* h) {
  hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    h->err = std::string("device failure: ") + hipGetErrorString(e);
    return SWIM_EDEVICE;
  }
  for (size_t i = 0; h->mem.guard && i < h->mem.live.size(); ++i) {  // SWIM_GUARD
    std::vector<unsigned char> g(2 * GUARD);
    const DevAllocs::Entry& a = h->mem.live[i];
    if (hipMemcpy(g.data(), a.raw, GUARD, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(g.data() + GUARD, (char*)a.raw + GUARD + a.bytes, GUARD, hipMemcpyDeviceToHost) != hipSuccess)
      return SWIM_EDEVICE;
    for (size_t j = 0; j < 2 * GUARD; ++j)
      if (g[j] != 0x5A) {
        h->err = "guard of allocation #" + std::to_string(i) + " (" + std::to_string(a.bytes) + " B) overwritten at " +
                 (j < GUARD ? "-" + std::to_string(GUARD - j) : "+" + std::to_string(j - GUARD)) + " value " +
                 std::to_string(g[j]);
        fprintf(stderr, "%s\n", h->err.c_str());
        return SWIM_EDEVICE;
      }
  }
  uint32_t eb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hipMemcpy(eb, h->d.err, sizeof(eb), hipMemcpyDeviceToHost) != hipSuccess) return SWIM_EDEVICE;
  uint32_t bits = eb[0];
  if (bits) {
    char hex[160];
    snprintf(hex, sizeof hex, "%x [info %u %u %u %u %u %u %u]", bits, eb[1], eb[2], eb[3], eb[4], eb[5], eb[6], eb[7]);
    h->err = std::string("engine capacity/semantic error bits 0x") + hex +
             " (see engine.h E_* ; raise the matching capacity in swim_config)";
    return SWIM_ECAPACITY;
  }
  return SWIM_OK;
}

// open a new NetworkEmulator-settings epoch that starts at the next tick to run
int push_epoch(swim_handle* h) {
  lf_off(h);  // (link settings: loss, partitions, delays)
  int e = h->cur_ep;
  if (h->ep_from[e] != (uint32_t)h->tick) e = (e + 1) % (int)MAX_EPOCHS;
  h->cur_ep = e;
  h->ep_from[e] = (uint32_t)h->tick;
  h->ep_loss[e] = h->loss;
  h->ep_part[e] = h->partitioned ? 1u : 0u;
  h->ep_delay[e] = h->delay_idx;
  // the kernels that take Dev by value see h->d at launch; the others read the device copy (d.self)
  Dev& d = h->d;
  d.ep_delay[e] = h->ep_delay[e];
  d.ep_from[e] = h->ep_from[e];
  d.ep_loss[e] = h->ep_loss[e];
  d.ep_part[e] = h->ep_part[e];
  HIPCK(h2d(h->stream, (void*)(d.self->ep_delay + e), &d.ep_delay[e], 4));
  HIPCK(h2d(h->stream, (void*)(d.self->ep_from + e), &d.ep_from[e], 4));
  HIPCK(h2d(h->stream, (void*)(d.self->ep_loss + e), &d.ep_loss[e], 4));
  HIPCK(h2d(h->stream, (void*)(d.self->ep_part + e), &d.ep_part[e], 4));
  HIPCK(h2d(h->stream, h->d.ep_group + (size_t)e * h->d.N, h->group.data(), 4ull * h->d.N));
  return SWIM_OK;
}

// the host readers' walk of a message buffer (msg_slots.h msg_for_each): the overflow count, the shards' counters, then
// the two regions' slots in use, ascending. slots (optional): the slot of each message returned.
int msgs_read(swim_handle* h, uint32_t b, std::vector<SyncMsg>& out, std::vector<uint32_t>* slots_out) {
  const Dev& d = h->d;
  out.clear();
  uint32_t nover = 0;
  HIPCK(hipMemcpy(&nover, d.nmsg + b, 4, hipMemcpyDeviceToHost));
  const MsgLayout L = msg_layout(d.MSGCAP, d.msh);
  uint32_t cnt[MSG_SHARDS_MAX] = {0};
  if (L.S > 1) {
    std::vector<unsigned long long> sh((size_t)(L.S + 1) * CSTRIDE);
    HIPCK(hipMemcpy(sh.data(), d.ctr_sh, 8 * sh.size(), hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < L.S; ++s) cnt[s] = (uint32_t)sh[(size_t)(s + 1) * CSTRIDE + MSG_CTR_WORD + b];
  }
  std::vector<uint32_t> slots;
  msg_for_each(L, cnt, nover, [&](uint32_t i) { slots.push_back(i); });
  if (slots_out) *slots_out = slots;
  if (slots.empty()) return SWIM_OK;
  // (ascending: the fast region's slots lie in [0, first overflow slot), the overflow region's are contiguous)
  const uint32_t nf = (uint32_t)(std::lower_bound(slots.begin(), slots.end(), L.R) - slots.begin());
  std::vector<SyncMsg> fast(nf ? slots[nf - 1] + 1 : 0), over(slots.size() - nf);
  if (!fast.empty()) HIPCK(hipMemcpy(fast.data(), d.msgs[b], fast.size() * sizeof(SyncMsg), hipMemcpyDeviceToHost));
  if (!over.empty()) HIPCK(hipMemcpy(over.data(), d.msgs[b] + L.R, over.size() * sizeof(SyncMsg), hipMemcpyDeviceToHost));
  for (uint32_t q = 0; q < nf; ++q) out.push_back(fast[slots[q]]);
  out.insert(out.end(), over.begin(), over.end());
  return SWIM_OK;
}

}  // namespace swim

namespace {

// rebuild the device link table from the host history (fault calls are rare; the table is at most ~300 KB)
int upload_links(swim_handle* h) {
  lf_off(h);
  const uint32_t now = (uint32_t)h->tick, look = h->d.LOOKBACK + 2 * h->d.ping_t + 16;
  for (auto it = h->link_hist.begin(); it != h->link_hist.end();) {  // links back at default for long: forget them
    const auto& v = it->second;
    if (!h->link_cur.count(it->first) && v.back().second == LK_NONE && v.back().first + look < now)
      it = h->link_hist.erase(it);
    else
      ++it;
  }
  if (h->link_hist.size() > LKCAP / 2) {
    h->err = "more than 2048 links with custom NetworkEmulator settings";
    return SWIM_ECAPACITY;
  }
  std::vector<uint64_t> keys(LKCAP, 0);
  std::vector<uint32_t> hist((size_t)LKCAP * LKH * 2, LK_NONE);
  for (const auto& kv : h->link_hist) {
    uint32_t p = (uint32_t)mix64(kv.first) & (LKCAP - 1);
    while (keys[p]) p = (p + 1) & (LKCAP - 1);
    keys[p] = kv.first;
    const auto& v = kv.second;
    const size_t first = v.size() > LKH ? v.size() - LKH : 0;
    for (size_t i = first; i < v.size(); ++i) {
      hist[((size_t)p * LKH + (i - first)) * 2] = v[i].first;
      hist[((size_t)p * LKH + (i - first)) * 2 + 1] = v[i].second;
    }
    if (first) hist[(size_t)p * LKH * 2] |= LK_TRUNC;
  }
  uint32_t n = (uint32_t)h->link_hist.size();
  HIPCK(hipStreamSynchronize(h->stream));
  HIPCK(h2d(h->stream, h->d.link_key, keys.data(), 8ull * LKCAP));
  HIPCK(h2d(h->stream, h->d.link_hist, hist.data(), 4ull * hist.size()));
  h->d.link_n = n;
  HIPCK(h2d(h->stream, (void*)&h->d.self->link_n, &h->d.link_n, 4));
  return SWIM_OK;
}

// a change of link src -> dst effective from the next tick to run (NONE = back to the default settings)
void link_change(swim_handle* h, uint64_t key, uint32_t v) {
  auto& hv = h->link_hist[key];
  const uint32_t now = (uint32_t)h->tick;
  if (!hv.empty() && hv.back().first == now)
    hv.back().second = v;
  else
    hv.emplace_back(now, v);
  if (v == LK_NONE)
    h->link_cur.erase(key);
  else
    h->link_cur[key] = v;
}

uint64_t link_key_of(uint32_t src, uint32_t dst) { return (((uint64_t)src << 32) | dst) + 1ull; }

bool owns(const swim_handle* h, uint32_t m) { return m >= h->d.lo && m < h->d.hi; }

}  // namespace

extern "C" {

uint32_t swim_abi_version(void) { return SWIM_ABI_VERSION; }

void swim_default_config(swim_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->tick_ms = 100;
  c->latency_ticks = 1;
  c->init_mode = SWIM_INIT_PRECONVERGED;
  c->seed = 0x5EED5EEDull;
  c->sync_interval_ms = 30000;
  c->sync_timeout_ms = 3000;
  c->suspicion_mult = 5;
  c->ping_interval_ms = 1000;
  c->ping_timeout_ms = 500;
  c->ping_req_members = 3;
  c->gossip_interval_ms = 200;
  c->gossip_fanout = 3;
  c->gossip_repeat_mult = 3;
  c->metadata_timeout_ms = 3000;
  c->n_gpus = 1;
}

int swim_is_overrides(uint32_t s1, uint32_t i1, uint32_t s0, uint32_t i0) { return overrides(s1, i1, s0, i0) ? 1 : 0; }
uint32_t swim_ceil_log2(uint32_t n) { return bitlen(n); }

int swim_create(const swim_config* cfg, swim_handle** out) {
  // one handle for all N observers: on one GPU, or row-sharded over n_gpus devices inside this process (Group)
  if (cfg && out && cfg->n_gpus > 1) {
    *out = nullptr;
    return create_group(cfg, out);
  }
  return create(cfg, nullptr, out);
}

int swim_create_sharded(const swim_config* cfg, const swim_shard_spec* spec, swim_handle** out) {
  if (!spec) return SWIM_EINVAL;
  return create(cfg, spec, out);
}

int swim_rccl_unique_id(uint8_t* out128) {
  if (!out128) return SWIM_EINVAL;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return SWIM_EDEVICE;
  std::memcpy(out128, &id, 128);
  return SWIM_OK;
}

int swim_shard_range(swim_handle* h, uint32_t* lo, uint32_t* hi) {
  if (!h || !lo || !hi) return SWIM_EINVAL;
  if (h->grp) {  // the group reports on every observer
    *lo = 0;
    *hi = h->d.N;
    return SWIM_OK;
  }
  *lo = h->d.lo;
  *hi = h->d.hi;
  return SWIM_OK;
}

int swim_destroy(swim_handle* h) {
  if (!h) return SWIM_EINVAL;
  watch_free_all(h);  // (a group's watches before its shards: they hold the shards' parts)
  if (h->grp) {
    group_destroy(h);
    return SWIM_OK;
  }
  hipSetDevice((int)h->cfg.device);
  if (h->stream) hipStreamSynchronize(h->stream);
  h->mem.free_all();
  for (auto& te : h->prof)
    for (auto& e : te.ev) hipEventDestroy((hipEvent_t)e);
  if (h->comm) ncclCommDestroy(h->comm);
  if (h->hcnt) hipHostFree(h->hcnt);
  if (h->hflag) hipHostFree((void*)h->hflag);
  if (h->xi_host_h) hipHostFree(h->xi_host_h);
  if (h->ev_member) hipEventDestroy(h->ev_member);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return SWIM_OK;
}

int swim_run_periods(swim_handle* h, uint32_t n) {
  if (!h) return SWIM_EINVAL;
  return swim_step(h, n * h->d.ping_t);
}

int swim_sync(swim_handle* h) {
  GROUP_ALL(swim_sync(s));
  return h ? check_err(h) : SWIM_EINVAL;
}

int swim_kill(swim_handle* h, uint32_t m) {
  GROUP_ALL(swim_kill(s, m));
  if (!h || m >= h->d.N) return SWIM_EINVAL;
  launch_kill(h->d, m, (uint32_t)h->tick, h->stream);  // dead_tick[m], and its lower bound first_dead
  // (the crashed member's holder state stays as it is: it never sends again, sends to it fail, and its slots expire)
  return check_err(h);
}

int swim_join(swim_handle* h, uint32_t m, const uint32_t* seeds, uint32_t n) {
  GROUP_ALL(swim_join(s, m, seeds, n));
  if (!h || m >= h->d.N || n > 16 || (n && !seeds)) return SWIM_EINVAL;
  if (m < h->d.N - h->d.n_dormant) return SWIM_EINVAL;  // only a dormant member starts later
  if (h->joined.empty()) h->joined.assign(h->d.N, 0);
  if (h->joined[m]) return SWIM_EINVAL;
  h->joined[m] = 1;
  lf_off(h);
  uint32_t sd[16], ns = 0;  // LinkedHashSet of valid ids minus self (MembershipProtocolImpl.java:160-166)
  for (uint32_t i = 0; i < n; ++i) {
    bool dup = seeds[i] >= h->d.N || seeds[i] == m;
    for (uint32_t j = 0; j < ns; ++j) dup |= sd[j] == seeds[i];
    if (!dup) sd[ns++] = seeds[i];
  }
  launch_join(h->d, m, (uint32_t)h->tick, sd, ns, h->stream);  // every shard: the arrays are replicated
  return check_err(h);
}

int swim_spread_gossip(swim_handle* h, uint32_t m, uint64_t payload) {
  GROUP_ALL(swim_spread_gossip(s, m, payload));
  if (!h || m >= h->d.N) return SWIM_EINVAL;
  if (!owns(h, m)) return SWIM_OK;  // the owning shard creates it; the others receive its slot in exchange A
  uint32_t dt = 0;
  HIPCK(hipStreamSynchronize(h->stream));
  HIPCK(hipMemcpy(&dt, h->d.dead_tick + m, 4, hipMemcpyDeviceToHost));
  if (dt != NEVER) return SWIM_EINVAL;
  h->ugq.push_back(m);
  h->ugq.push_back(payload);
  return SWIM_OK;
}

int swim_update_metadata(swim_handle* h, uint32_t m) {
  GROUP_ALL(swim_update_metadata(s, m));
  if (!h || m >= h->d.N) return SWIM_EINVAL;
  if (h->d.implicit) return SWIM_EUNSUPPORTED;  // implicit views: the tables are not stored
  uint32_t dt = 0, ver = 0;
  HIPCK(hipStreamSynchronize(h->stream));
  HIPCK(hipMemcpy(&dt, h->d.dead_tick + m, 4, hipMemcpyDeviceToHost));
  if (dt != NEVER) return SWIM_EINVAL;
  if (std::find(h->md_cols.begin(), h->md_cols.end(), m) == h->md_cols.end()) {
    if (h->md_cols.size() >= MDU) {
      h->err = "swim_update_metadata: more than " + std::to_string(MDU) + " members with updated metadata";
      return SWIM_ECAPACITY;
    }
    launch_md_column(h->d, m, (uint32_t)h->md_cols.size(), h->stream);
    h->md_cols.push_back(m);
    HIPCK(hipStreamSynchronize(h->stream));
  }
  // every shard keeps the versions of all members (responses are evaluated at the issuer's shard)
  HIPCK(hipMemcpy(&ver, h->d.md_version + m, 4, hipMemcpyDeviceToHost));
  ++ver;
  HIPCK(h2d(h->stream, h->d.md_version + m, &ver, 4));
  return swim_update_incarnation(h, m);
}

int swim_update_incarnation(swim_handle* h, uint32_t m) {
  GROUP_ALL(swim_update_incarnation(s, m));
  if (!h || m >= h->d.N) return SWIM_EINVAL;
  if (h->d.implicit) return SWIM_EUNSUPPORTED;  // implicit views: the tables are not stored
  if (!owns(h, m)) return SWIM_OK;  // the owning shard bumps it; the others learn it from its gossip
  uint32_t req = 0, dt = 0;
  HIPCK(hipStreamSynchronize(h->stream));
  HIPCK(hipMemcpy(&dt, h->d.dead_tick + m, 4, hipMemcpyDeviceToHost));
  if (dt != NEVER) return SWIM_EINVAL;
  HIPCK(hipMemcpy(&req, h->d.pending_inc + m, 4, hipMemcpyDeviceToHost));
  req += 4u;  // bits 2..: incarnation bumps requested (one per call), bit 1: leave
  HIPCK(h2d(h->stream, h->d.pending_inc + m, &req, 4));
  return SWIM_OK;
}

// MembershipProtocolImpl.leaveCluster (:197-206) via ClusterImpl.shutdown -> doShutdown (:297-313): in P0 of the next
// tick the member's own record becomes DEAD inc+1 and is spread; when that gossip is swept at the member, it stops
int swim_leave(swim_handle* h, uint32_t m) {
  GROUP_ALL(swim_leave(s, m));
  if (!h || m >= h->d.N) return SWIM_EINVAL;
  if (h->d.implicit) return SWIM_EUNSUPPORTED;  // implicit views: the tables are not stored
  HIPCK(hipStreamSynchronize(h->stream));
  uint32_t dt = 0, req = 0;
  HIPCK(hipMemcpy(&dt, h->d.dead_tick + m, 4, hipMemcpyDeviceToHost));
  if (dt != NEVER) return SWIM_EINVAL;
  lf_off(h);
  const uint32_t one = 1;  // every shard: k_gossip_apply keeps ALIVE receipts about a leaver (its DEAD may arrive in P1)
  HIPCK(h2d(h->stream, h->d.leaving + m, &one, 4));
  if (!owns(h, m)) return SWIM_OK;
  HIPCK(hipMemcpy(&req, h->d.pending_inc + m, 4, hipMemcpyDeviceToHost));
  req |= 2u;
  HIPCK(h2d(h->stream, h->d.pending_inc + m, &req, 4));
  return SWIM_OK;
}

int swim_set_member_config(swim_handle* h, uint32_t m, const swim_member_config* mc) {
  GROUP_ALL(swim_set_member_config(s, m, mc));
  if (!h || !mc || m >= h->d.N) return SWIM_EINVAL;
  Dev& d = h->d;
  const bool dormant = m >= d.N - d.n_dormant && (h->joined.empty() || !h->joined[m]);
  if (h->tick > 0 && !dormant) return SWIM_EINVAL;  // a running member's ClusterConfig is fixed
  uint32_t pt = 0, tt = 0;
  if (mc->ping_timeout_ms >= mc->ping_interval_ms || mc->ping_req_members > 8 ||
      !to_ticks(mc->ping_interval_ms, h->cfg.tick_ms, &pt) || !to_ticks(mc->ping_timeout_ms, h->cfg.tick_ms, &tt) || pt == 0)
    return SWIM_EINVAL;
  const uint32_t v[4] = {pt, tt, mc->ping_req_members, mc->sync_group};
  lf_off(h);
  HIPCK(hipStreamSynchronize(h->stream));
  HIPCK(h2d(h->stream, d.mcfg + 4ull * m, v, sizeof(v)));
  if (h->cfg.init_mode == SWIM_INIT_PRECONVERGED && d.mode != SWIM_MODE_RUMOR) {
    // the PRECONVERGED schedule phase under the member's own interval (k_init_members, SEMANTICS.md §3)
    const uint32_t np = 1u + philox(m, 1, 0, 0, d.seed_lo ^ SALT_INIT, d.seed_hi).x % pt;
    HIPCK(h2d(h->stream, d.nextPing + m, &np, 4));
  } else if (h->cfg.init_mode == SWIM_INIT_COLD_JOIN && !dormant) {
    // an initial member starts at tick 0 (start0): its first ping follows its own pingInterval (a dormant member's
    // is set by k_join at its start tick)
    HIPCK(h2d(h->stream, d.nextPing + m, &pt, 4));
  }
  if (!d.permember) {  // the kernels read mcfg from now on (Dev is passed by value and through d.self)
    d.permember = 1;
    HIPCK(h2d(h->stream, (void*)d.self, &d, sizeof(Dev)));
  }
  return SWIM_OK;
}

int swim_set_default_loss(swim_handle* h, uint32_t pct) {
  GROUP_ALL(swim_set_default_loss(s, pct));
  if (!h || pct > 100) return SWIM_EINVAL;
  h->loss = pct;
  return push_epoch(h);
}

int swim_set_partition(swim_handle* h, const uint32_t* g) {
  GROUP_ALL(swim_set_partition(s, g));
  if (!h) return SWIM_EINVAL;
  if (g) {
    h->group.assign(g, g + h->d.N);
    h->partitioned = true;
    // block() writes DEAD_LINK_SETTINGS over a custom setting of every cross-group link (NetworkEmulator.java:141-150)
    std::vector<uint64_t> drop;
    for (const auto& kv : h->link_cur) {
      uint32_t src = (uint32_t)((kv.first - 1) >> 32), dst = (uint32_t)(kv.first - 1);
      if (g[src] != g[dst]) drop.push_back(kv.first);
    }
    for (uint64_t key : drop) link_change(h, key, LK_NONE);
    if (!drop.empty()) {
      int rc = upload_links(h);
      if (rc) return rc;
    }
  } else {
    h->partitioned = false;
  }
  return push_epoch(h);
}

int swim_unblock_all(swim_handle* h) {  // NetworkEmulator.unblockAll: customLinkSettings.clear() (:186-192)
  GROUP_ALL(swim_unblock_all(s));
  if (!h) return SWIM_EINVAL;
  h->partitioned = false;
  if (!h->link_cur.empty()) {
    std::vector<uint64_t> keys;
    for (const auto& kv : h->link_cur) keys.push_back(kv.first);
    for (uint64_t key : keys) link_change(h, key, LK_NONE);
    int rc = upload_links(h);
    if (rc) return rc;
  }
  return push_epoch(h);
}

int swim_set_link_loss(swim_handle* h, uint32_t src, uint32_t dst, uint32_t pct) {
  GROUP_ALL(swim_set_link_loss(s, src, dst, pct));
  if (!h || src >= h->d.N || dst >= h->d.N || pct > 100) return SWIM_EINVAL;
  link_change(h, link_key_of(src, dst), pct);
  return upload_links(h);
}

// the delay index of a mean delay (0: none, or a delay that never reaches a tick); registers its threshold table
static int delay_index(swim_handle* h, uint32_t delay_ms, uint32_t* idx) {
  std::vector<uint32_t> t;
  lf_off(h);
  if (!delay_table(delay_ms, h->cfg.tick_ms, &t)) return fail(h, SWIM_EINVAL, "mean delay above 11 x tick_ms");
  *idx = 0;
  if (t.empty()) return SWIM_OK;  // no message can be delayed past its tick
  if (t.size() > h->d.EMAX) return fail(h, SWIM_EUNSUPPORTED, "mean delay above swim_config.delay_cap_ms");
  for (uint32_t i = 1; i < (uint32_t)h->delays.size(); ++i)
    if (h->delays[i] == delay_ms) {
      *idx = i;
      return SWIM_OK;
    }
  if (h->delays.size() >= DTAB) return fail(h, SWIM_ECAPACITY, "more than 15 distinct mean delays");
  *idx = (uint32_t)h->delays.size();
  h->delays.push_back(delay_ms);
  const uint32_t len = (uint32_t)t.size();
  HIPCK(h2d(h->stream, h->d.dly_thr + (size_t)*idx * 256, t.data(), 4ull * len));
  HIPCK(h2d(h->stream, h->d.dly_len + *idx, &len, 4));
  if (!h->d.dly_on) {  // from now on the gossip plane queues delayed receipts and SYNC messages are stored
    h->d.dly_on = 1;
    HIPCK(h2d(h->stream, (void*)h->d.self, &h->d, sizeof(Dev)));
  }
  return SWIM_OK;
}

int swim_set_default_link_settings(swim_handle* h, uint32_t pct, uint32_t delay_ms) {
  GROUP_ALL(swim_set_default_link_settings(s, pct, delay_ms));
  if (!h || pct > 100) return SWIM_EINVAL;
  uint32_t idx;
  int rc = delay_index(h, delay_ms, &idx);
  if (rc) return rc;
  h->delay_idx = idx;
  return swim_set_default_loss(h, pct);  // a new settings epoch with both
}

int swim_set_link_settings(swim_handle* h, uint32_t src, uint32_t dst, uint32_t pct, uint32_t delay_ms) {
  GROUP_ALL(swim_set_link_settings(s, src, dst, pct, delay_ms));
  if (!h || src >= h->d.N || dst >= h->d.N || pct > 100) return SWIM_EINVAL;
  uint32_t idx;
  int rc = delay_index(h, delay_ms, &idx);
  if (rc) return rc;
  link_change(h, link_key_of(src, dst), pct | (idx << 8));
  return upload_links(h);
}

int swim_emulator_counters(swim_handle* h, uint64_t* out, size_t cap) {
  if (!h || !out || cap < 2ull * h->cfg.n_members) return SWIM_EINVAL;
  if (h->grp) {  // each shard counted the sends it evaluated (its issuers' FD / SYNC / metadata, its targets' gossip)
    std::vector<uint64_t> part(2ull * h->cfg.n_members);
    std::fill(out, out + part.size(), 0ull);
    return group_all(h, [&](swim_handle* s) {
      const int rc = swim_emulator_counters(s, part.data(), part.size());
      for (size_t i = 0; rc == SWIM_OK && i < part.size(); ++i) out[i] += part[i];
      return rc;
    });
  }
  if (!h->d.em) return fail(h, SWIM_EUNSUPPORTED, "emulator counters need SWIM_FLAG_EMULATOR_COUNTERS");
  HIPCK(hipStreamSynchronize(h->stream));
  HIPCK(hipMemcpy(out, h->d.em, 16ull * h->d.N, hipMemcpyDeviceToHost));
  return SWIM_OK;
}

int swim_unblock_link(swim_handle* h, uint32_t src, uint32_t dst) {
  GROUP_ALL(swim_unblock_link(s, src, dst));
  if (!h || src >= h->d.N || dst >= h->d.N) return SWIM_EINVAL;
  if (!h->link_cur.count(link_key_of(src, dst))) return SWIM_OK;
  link_change(h, link_key_of(src, dst), LK_NONE);
  return upload_links(h);
}

int swim_current_tick(swim_handle* h, uint64_t* t) {
  if (!h || !t) return SWIM_EINVAL;
  *t = h->tick;
  return SWIM_OK;
}

int swim_read_row(swim_handle* h, uint32_t obs, uint64_t* out, size_t cap) {
  GROUP_OWNER(obs, swim_read_row(s, obs, out, cap));
  if (!h || obs >= h->d.N || cap < h->d.N || !owns(h, obs)) return SWIM_EINVAL;
  HIPCK(hipStreamSynchronize(h->stream));
  if (h->d.implicit) {  // RUMOR mode: every row is the PRECONVERGED row
    for (uint32_t s = 0; s < h->d.N; ++s) out[s] = PRE_REC;
    return SWIM_OK;
  }
  std::vector<uint32_t> k(h->d.N), a(h->d.N);  // the two planes, joined into logical records (swim_common.h)
  HIPCK(hipMemcpy(k.data(), h->d.rowk + lidx(h->d, obs) * h->d.NS, 4ull * h->d.N, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(a.data(), h->d.rowa + lidx(h->d, obs) * h->d.NS, 4ull * h->d.N, hipMemcpyDeviceToHost));
  for (uint32_t s = 0; s < h->d.N; ++s) out[s] = (k[s] & 3u) == ST_ABSENT ? 0 : rec_join(k[s], a[s]);
  return SWIM_OK;
}

// the shards' partial censuses combined (swimhip_census.h): counts add, key ranges widen, by_observer rows are disjoint
static int group_census(swim_handle* h, swim_census* c) {
  const size_t N = h->cfg.n_members;
  if (h->grp->slots) {  // slot-sharded: every shard holds every view
    swim_handle* s = h->grp->shards[0];
    hipSetDevice((int)s->cfg.device);
    const int rc = swim_view_census(s, c);
    return rc == SWIM_OK ? rc : fail(h, rc, "shard 0: " + s->err);
  }
  std::vector<uint32_t> bs(c->by_subject ? 4 * N : 0), bo(c->by_observer ? 4 * N : 0), mn(c->key_min ? N : 0),
      mx(c->key_max ? N : 0);
  if (c->by_subject) std::fill(c->by_subject, c->by_subject + 4 * N, 0u);
  if (c->by_observer) std::fill(c->by_observer, c->by_observer + 4 * N, 0u);
  if (c->key_min) std::fill(c->key_min, c->key_min + N, 0xFFFFFFFFu);
  if (c->key_max) std::fill(c->key_max, c->key_max + N, 0u);
  swim_census p = *c, sum = *c;
  p.by_subject = c->by_subject ? bs.data() : nullptr;
  p.by_observer = c->by_observer ? bo.data() : nullptr;
  p.key_min = c->key_min ? mn.data() : nullptr;
  p.key_max = c->key_max ? mx.data() : nullptr;
  sum.n_observers = sum.bytes_read = 0;
  std::fill(sum.records, sum.records + 4, 0ull);
  const int rc = group_all(h, [&](swim_handle* s) {
    const int r = swim_view_census(s, &p);
    if (r != SWIM_OK) return r;
    for (size_t i = 0; i < bs.size(); ++i) c->by_subject[i] += bs[i];
    for (size_t i = 0; i < bo.size(); ++i) c->by_observer[i] += bo[i];
    for (size_t i = 0; i < mn.size(); ++i) c->key_min[i] = std::min(c->key_min[i], mn[i]);
    for (size_t i = 0; i < mx.size(); ++i) c->key_max[i] = std::max(c->key_max[i], mx[i]);
    sum.tick = p.tick;
    sum.path = p.path;
    sum.n_observers += p.n_observers;
    sum.bytes_read += p.bytes_read;
    for (int st = 0; st < 4; ++st) sum.records[st] += p.records[st];
    return r;
  });
  c->tick = sum.tick;
  c->path = sum.path;
  c->n_observers = sum.n_observers;
  c->bytes_read = sum.bytes_read;
  std::copy(sum.records, sum.records + 4, c->records);
  std::fill(c->reserved, c->reserved + 3, 0u);
  return rc;
}

int swim_view_census(swim_handle* h, swim_census* c) {
  if (!h || !c) return SWIM_EINVAL;
  if (h->grp) return group_census(h, c);
  const Dev& d = h->d;
  const size_t N = d.N;
  const uint32_t now = (uint32_t)h->tick;
  c->tick = h->tick;
  c->n_observers = c->bytes_read = 0;
  std::fill(c->records, c->records + 4, 0ull);
  std::fill(c->reserved, c->reserved + 3, 0u);
  HIPCK(hipStreamSynchronize(h->stream));
  if (d.implicit) {  // every row is the PRECONVERGED row (PRE_REC): nothing to read
    c->path = SWIM_CENSUS_PATH_IMPLICIT;
    std::vector<uint32_t> dt(N);
    if (!c->observers) HIPCK(hipMemcpy(dt.data(), d.dead_tick, 4 * N, hipMemcpyDeviceToHost));
    if (c->by_observer) std::fill(c->by_observer, c->by_observer + 4 * N, 0u);
    for (uint32_t m = d.lo; m < d.hi; ++m)
      if (c->observers ? c->observers[m] != 0 : dt[m] > now) {
        ++c->n_observers;
        if (c->by_observer) c->by_observer[4ull * m + ST_ALIVE] = d.N;
      }
    const uint32_t n = (uint32_t)c->n_observers, key = key32(PRE_REC);
    c->records[ST_ALIVE] = c->n_observers * N;
    for (size_t s = 0; s < N; ++s) {
      if (c->by_subject) {
        std::fill(c->by_subject + 4 * s, c->by_subject + 4 * s + 4, 0u);
        c->by_subject[4 * s + ST_ALIVE] = n;
      }
      if (c->key_min) c->key_min[s] = n ? key : 0xFFFFFFFFu;
      if (c->key_max) c->key_max[s] = n ? key : 0u;
    }
    return check_err(h);
  }
  c->path = d.rowk8 ? SWIM_CENSUS_PATH_KEY8 : SWIM_CENSUS_PATH_KEY32;
  // scratch of this call: the totals, the caller's mask, then the requested outputs (key_min and key_max together)
  const bool keys = c->key_min || c->key_max;
  const size_t o_sel = 64, o_bs = o_sel + ((N + 63) & ~(size_t)63), o_bo = o_bs + (c->by_subject ? 16 * N : 0),
               o_mn = o_bo + (c->by_observer ? 16 * N : 0), o_mx = o_mn + (keys ? 4 * N : 0),
               bytes = o_mx + (keys ? 4 * N : 0);
  static_assert(CT_N * sizeof(unsigned long long) <= 64, "the totals fit the scratch header");
  static_assert(SWIM_CENSUS_TILE_ROWS == CENSUS_ROWS && SWIM_CENSUS_TILE_COLS == CENSUS_COLS, "the documented tile");
  char* buf = nullptr;
  HIPCK(hipMalloc(&buf, bytes));
  CensusOut o{};
  o.tot = (unsigned long long*)buf;
  if (c->by_subject) o.by_subject = (uint32_t*)(buf + o_bs);
  if (c->by_observer) o.by_observer = (uint32_t*)(buf + o_bo);
  if (keys) o.key_min = (uint32_t*)(buf + o_mn), o.key_max = (uint32_t*)(buf + o_mx);
  unsigned long long tot[CT_N] = {};
  hipError_t e = hipMemsetAsync(buf, 0, bytes, h->stream);
  if (e == hipSuccess && keys) e = hipMemsetAsync(o.key_min, 0xFF, 4 * N, h->stream);
  if (e == hipSuccess && c->observers) e = h2d(h->stream, buf + o_sel, c->observers, N);
  if (e == hipSuccess) {
    launch_census(d, c->observers ? (const uint8_t*)(buf + o_sel) : nullptr, now, o, h->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = hipMemcpy(tot, o.tot, sizeof(tot), hipMemcpyDeviceToHost);
  if (e == hipSuccess && c->by_subject) e = hipMemcpy(c->by_subject, o.by_subject, 16 * N, hipMemcpyDeviceToHost);
  if (e == hipSuccess && c->by_observer) e = hipMemcpy(c->by_observer, o.by_observer, 16 * N, hipMemcpyDeviceToHost);
  if (e == hipSuccess && c->key_min) e = hipMemcpy(c->key_min, o.key_min, 4 * N, hipMemcpyDeviceToHost);
  if (e == hipSuccess && c->key_max) e = hipMemcpy(c->key_max, o.key_max, 4 * N, hipMemcpyDeviceToHost);
  hipFree(buf);
  HIPCK(e);
  // the kernel counts ABSENT, SUSPECT and DEAD; ALIVE is what remains of the rows counted
  c->n_observers = tot[CT_ROWS];
  for (uint32_t st = 0; st < 4; ++st) c->records[st] = tot[CT_ST + st];
  c->records[ST_ALIVE] = tot[CT_ROWS] * N - tot[CT_ST + ST_ABSENT] - tot[CT_ST + ST_SUSPECT] - tot[CT_ST + ST_DEAD];
  for (size_t s = 0; c->by_subject && s < N; ++s) {
    uint32_t* b = c->by_subject + 4 * s;
    b[ST_ALIVE] = (uint32_t)tot[CT_ROWS] - b[ST_ABSENT] - b[ST_SUSPECT] - b[ST_DEAD];
  }
  c->bytes_read = tot[CT_ROWS] * N * (d.rowk8 ? 1u : 4u) + 4 * tot[CT_ESC];
  return check_err(h);
}

int swim_export_sync_frame(swim_handle* h, uint32_t obs, uint32_t kind, uint8_t* buf, size_t cap, size_t* len) {
  if (!h || !len) return SWIM_EINVAL;
  std::vector<uint64_t> row(h->d.N);
  int rc = swim_read_row(h, obs, row.data(), row.size());
  if (rc != SWIM_OK) return rc;
  std::vector<swim_wire_record> recs;  // prepareSyncDataMsg (MembershipProtocolImpl.java:446-454): the whole table
  for (uint32_t s = 0; s < h->d.N; ++s)
    if (rec_status(row[s]) != ST_ABSENT) recs.push_back(swim_wire_record{s, rec_status(row[s]), rec_inc(row[s])});
  return swim_wire_sync_frame(kind, obs, nullptr, "default", recs.data(), recs.size(), buf, cap, len);
}

int swim_state_hash(swim_handle* h, uint64_t* out, size_t cap) {
  if (!h || cap < 6ull * h->d.N) return SWIM_EINVAL;
  if (h->grp) {  // each shard fills its observers' words and leaves the others zero
    std::vector<uint64_t> part(6ull * h->d.N);
    std::fill(out, out + 6ull * h->d.N, 0ull);
    const bool slots = h->grp->slots;
    bool first = true;
    return group_all(h, [&](swim_handle* s) {
      const int rc = swim_state_hash(s, part.data(), part.size());
      // slot-sharded: row, lists and scalars are replicated (taken once); the event and held-gossip words are
      // sums over each shard's own gossips (SEMANTICS.md §9)
      for (size_t i = 0; rc == SWIM_OK && i < part.size(); ++i)
        if (!slots || first || i % 6 == 3 || i % 6 == 4) out[i] += part[i];
      first = false;
      return rc;
    });
  }
  uint64_t* dout = nullptr;
  HIPCK(hipMalloc(&dout, 48ull * h->d.N));
  HIPCK(hipMemsetAsync(dout, 0, 48ull * h->d.N, h->stream));  // other shards' observers stay zero
  launch_hash(h->d, dout, (uint32_t)h->tick, h->stream);
  HIPCK(hipStreamSynchronize(h->stream));
  HIPCK(hipMemcpy(out, dout, 48ull * h->d.N, hipMemcpyDeviceToHost));
  hipFree(dout);
  return check_err(h);
}

int swim_read_lists(swim_handle* h, uint32_t obs, uint32_t* fd, uint32_t* fd_len, uint32_t* gl, uint32_t* g_len,
                    size_t cap, int32_t* cursors) {
  GROUP_OWNER(obs, swim_read_lists(s, obs, fd, fd_len, gl, g_len, cap, cursors));
  if (!h || obs >= h->d.N || !owns(h, obs)) return SWIM_EINVAL;
  HIPCK(hipStreamSynchronize(h->stream));
  uint32_t fl = 0, glen = 0;
  MS ms;
  HIPCK(hipMemcpy(&ms, h->d.ms + obs, sizeof(MS), hipMemcpyDeviceToHost));
  fl = ms.fdLen;
  glen = ms.gLen;
  if (fl > cap || glen > cap) return SWIM_EINVAL;
  if (h->d.implicit) {  // RUMOR mode: the PRECONVERGED permutations (list_at)
    const FeistelPerm P0 = list_perm(h->d, obs, 0), P1 = list_perm(h->d, obs, 1);
    for (uint32_t p = 0; p < fl; ++p) fd[p] = list_at(P0, obs, p);
    for (uint32_t p = 0; p < glen; ++p) gl[p] = list_at(P1, obs, p);
  } else {
    HIPCK(hipMemcpy(fd, h->d.fdl + lidx(h->d, obs) * h->d.LCAP, 4ull * fl, hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(gl, h->d.gl + lidx(h->d, obs) * h->d.LCAP, 4ull * glen, hipMemcpyDeviceToHost));
  }
  cursors[0] = ms.pingIdx;
  cursors[1] = ms.remoteIdx;
  *fd_len = fl;
  *g_len = glen;
  return SWIM_OK;
}

int swim_read_gossips(swim_handle* h, uint32_t obs, uint64_t* ids, uint32_t* inf, size_t cap, size_t* n_out) {
  if (h && h->grp && h->grp->slots) {  // slot-sharded: the union of every shard's own gossips, in id order
    if (!n_out || obs >= h->d.N) return SWIM_EINVAL;
    std::vector<std::pair<uint64_t, uint32_t>> all;
    std::vector<uint64_t> i2(cap);
    std::vector<uint32_t> f2(cap);
    const int rc = group_all(h, [&](swim_handle* s) {
      size_t n = 0;
      const int r = swim_read_gossips(s, obs, i2.data(), f2.data(), cap, &n);
      for (size_t i = 0; r == SWIM_OK && i < n; ++i) all.emplace_back(i2[i], f2[i]);
      return r;
    });
    if (rc != SWIM_OK) return rc;
    std::sort(all.begin(), all.end());
    if (all.size() > cap) return SWIM_ECAPACITY;
    for (size_t i = 0; i < all.size(); ++i) ids[i] = all[i].first, inf[i] = all[i].second;
    *n_out = all.size();
    return SWIM_OK;
  }
  GROUP_OWNER(obs, swim_read_gossips(s, obs, ids, inf, cap, n_out));
  if (!h || obs >= h->d.N || !n_out || !owns(h, obs)) return SWIM_EINVAL;
  HIPCK(hipStreamSynchronize(h->stream));
  const Dev& d = h->d;
  std::vector<uint32_t> used(d.SLOTS), born(d.SLOTS);
  std::vector<uint16_t> col(d.SLOTS);
  std::vector<uint64_t> gid(d.SLOTS);
  HIPCK(hipMemcpy(used.data(), d.slot_used, 4ull * d.SLOTS, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(gid.data(), d.slot_gid, 8ull * d.SLOTS, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(born.data(), d.slot_ctick, 4ull * d.SLOTS, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(col.data(), d.S + (size_t)obs * d.SLOTS, 2ull * d.SLOTS, hipMemcpyDeviceToHost));  // member-major
  uint32_t first = 0, dt = 0;
  HIPCK(hipMemcpy(&first, d.firstGossip + obs, 4, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(&dt, d.dead_tick + obs, 4, hipMemcpyDeviceToHost));
  if (dt != NEVER) {  // a crashed member keeps no gossips (its entries stay only for the infectedFrom replay)
    *n_out = 0;
    return SWIM_OK;
  }
  std::vector<std::pair<uint64_t, uint32_t>> out;
  for (uint32_t g = 0; g < d.SLOTS; ++g) {
    const uint16_t e = col[g];
    if (!used[g] || !(e & S16_EVER) || (e & S16_SWEPT)) continue;
    const uint32_t c = s16_tick(e, (uint32_t)h->tick + d.lat);
    if (c < born[g]) continue;   // an earlier gossip of the recycled slot (s_get)
    if (c >= h->tick) continue;  // receipt of the next tick's P4
    uint32_t rb = (first == NEVER || c <= first) ? 0 : (c - first + d.gossip_t - 1) / d.gossip_t;
    out.emplace_back(gid[g], rb);
  }
  std::sort(out.begin(), out.end());
  if (out.size() > cap) return SWIM_ECAPACITY;
  for (size_t i = 0; i < out.size(); ++i) {
    ids[i] = out[i].first;
    inf[i] = out[i].second;
  }
  *n_out = out.size();
  return SWIM_OK;
}

int swim_drain_events(swim_handle* h, swim_event* out, size_t cap, size_t* n_out) {
  if (!h || !n_out) return SWIM_EINVAL;
  if (h->grp) {  // every shard's events, merged in (tick, observer, seq) order
    auto& ev = h->grp->events;
    // events left over from an earlier call (cap smaller than what was buffered) are already sorted and numbered;
    // only this call's events, all of later ticks, are sorted and numbered here
    const size_t old = ev.size();
    std::vector<swim_event> buf(65536);
    const int rc = group_all(h, [&](swim_handle* s) {
      size_t n = 0;
      do {
        const int r = swim_drain_events(s, buf.data(), buf.size(), &n);
        if (r != SWIM_OK) return r;
        ev.insert(ev.end(), buf.begin(), buf.begin() + (long)n);
      } while (n == buf.size());
      return SWIM_OK;
    });
    if (rc != SWIM_OK) return rc;
    if (h->grp->slots) {  // one observer's events of a tick come from several shards: P4's gossip-id order, renumbered
      std::stable_sort(ev.begin() + (long)old, ev.end(), [](const swim_event& a, const swim_event& b) {
        if (a.tick != b.tick) return a.tick < b.tick;
        if (a.observer != b.observer) return a.observer < b.observer;
        return a.subject != b.subject ? a.subject < b.subject : a.pad < b.pad;
      });
      for (size_t i = old; i < ev.size(); ++i) ev[i].seq = h->grp->evcount[ev[i].observer]++;
    } else {
      std::stable_sort(ev.begin() + (long)old, ev.end(), [](const swim_event& a, const swim_event& b) {
        if (a.tick != b.tick) return a.tick < b.tick;
        if (a.observer != b.observer) return a.observer < b.observer;
        return a.seq < b.seq;
      });
    }
    const size_t k = std::min(cap, ev.size());
    std::copy(ev.begin(), ev.begin() + (long)k, out);
    ev.erase(ev.begin(), ev.begin() + (long)k);
    *n_out = k;
    return SWIM_OK;
  }
  HIPCK(hipStreamSynchronize(h->stream));
  uint32_t n = 0;
  HIPCK(hipMemcpy(&n, h->d.ev_n, 4, hipMemcpyDeviceToHost));
  n = std::min(n, h->d.EVCAP);
  if (n) {
    size_t base = h->host_events.size();
    h->host_events.resize(base + n);
    HIPCK(hipMemcpy(h->host_events.data() + base, h->d.ev, sizeof(swim_event) * n, hipMemcpyDeviceToHost));
    HIPCK(hipMemsetAsync(h->d.ev_n, 0, 4, h->stream));
  }
  auto& ev = h->host_events;
  std::stable_sort(ev.begin(), ev.end(), [](const swim_event& a, const swim_event& b) {
    if (a.tick != b.tick) return a.tick < b.tick;
    if (a.observer != b.observer) return a.observer < b.observer;
    return a.seq < b.seq;
  });
  size_t k = std::min(cap, ev.size());
  std::copy(ev.begin(), ev.begin() + (long)k, out);
  ev.erase(ev.begin(), ev.begin() + (long)k);
  *n_out = k;
  return SWIM_OK;
}

// the lister's counts of the ticks that ran without a lister launch (engine.h SH_LF), from the counter rows `sh`:
// messages resolved, narrow messages decided without a stream, of those pinned
static void lf_counts(const std::vector<unsigned long long>& sh, unsigned long long (&v)[3]) {
  v[0] = v[1] = v[2] = 0;
  for (uint32_t r = 0; r < CSH; ++r)
    for (uint32_t i = 0; i < 3; ++i) v[i] += sh[(size_t)r * CSTRIDE + SH_LF + i];
}

int swim_counters_get(swim_handle* h, swim_counters* out) {
  if (!h || !out) return SWIM_EINVAL;
  if (h->grp) {  // the shards' shares summed (the tick is common)
    swim_counters sum{}, c{};
    const int rc = group_all(h, [&](swim_handle* s) {
      const int r = swim_counters_get(s, &c);
      const uint64_t* a = (const uint64_t*)&c;
      uint64_t* t = (uint64_t*)&sum;
      for (size_t i = 1; r == SWIM_OK && i < sizeof(c) / 8; ++i) t[i] += a[i];
      sum.tick = c.tick;
      return r;
    });
    *out = sum;
    return rc;
  }
  HIPCK(hipStreamSynchronize(h->stream));
  unsigned long long c[C_NCTR];
  HIPCK(hipMemcpy(c, h->d.ctr, sizeof(c), hipMemcpyDeviceToHost));
  {  // the member kernel's rows of counters 0-7
    std::vector<unsigned long long> sh((size_t)CSH * CSTRIDE);
    HIPCK(hipMemcpy(sh.data(), h->d.ctr_sh, 8 * sh.size(), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < CSH; ++r)
      for (uint32_t i = 0; i < 8; ++i) c[i] += sh[(size_t)r * CSTRIDE + i];
    unsigned long long lf[3];
    lf_counts(sh, lf);
    c[C_ACKRES_ALL] += lf[0];
    c[C_DIFFMSG_ALL] += lf[1];
  }
  std::memset(out, 0, sizeof(*out));
  out->tick = h->tick;
  out->record_compares = c[C_R];
  out->row_writes = c[C_W];
  out->messages = c[C_M];
  out->gossip_messages = c[C_G];
  out->events = c[C_E];
  out->messages_lost = c[C_LOST];
  out->gossips_created = c[C_GCREATED];
  out->sync_merges = c[C_SYNCMERGE];
  out->device_bytes = h->mem.bytes;
  out->diff_ns = (uint64_t)(h->prof_ms[0] * 1e6);
  out->member_ns = (uint64_t)(h->prof_ms[1] * 1e6);
  out->gossip_ns = (uint64_t)(h->prof_ms[2] * 1e6);
  out->diff_launches = h->prof_diff_launches;
  out->diff_msgs = c[C_DIFFMSG];
  out->ack_resolved = c[C_ACKRES];
  out->ack_resolved_total = c[C_ACKRES_ALL];
  out->diff_msgs_total = c[C_DIFFMSG_ALL];
  // the payloads streamed from the 8-bit shadow plane compared 2 B per subject, the others (C_DIFFWIDE) 8 B
  const uint64_t nsub = h->d.N;
  if (h->d.W == 1 && h->d.MW) {  // one GPU: the narrow chunks actually streamed (the others: decided from the dirty masks)
    out->diff_key_bytes = 2 * c[C_DSUBJ] + 8 * nsub * c[C_DIFFWIDE];
    out->diff_key_bytes_total = 2 * c[C_DSUBJ_ALL] + 8 * nsub * c[C_DIFFWIDE_ALL];
  } else {
    out->diff_key_bytes = nsub * (2 * (c[C_DIFFMSG] - std::min(c[C_DIFFMSG], c[C_DIFFWIDE])) + 8 * c[C_DIFFWIDE]);
    out->diff_key_bytes_total =
        nsub * (2 * (c[C_DIFFMSG_ALL] - std::min(c[C_DIFFMSG_ALL], c[C_DIFFWIDE_ALL])) + 8 * c[C_DIFFWIDE_ALL]);
  }
  out->exchange_ns = (uint64_t)(h->xchg_ms * 1e6);
  return SWIM_OK;
}

const char* swim_last_error(swim_handle* h) { return h ? h->err.c_str() : "null handle"; }

int swim_debug_fallbacks(swim_handle* h, uint64_t* out, size_t n) {
  if (!h || !out || n > FB_N) return SWIM_EINVAL;
  std::fill(out, out + n, 0ull);
  if (h->grp) {  // summed over the shards
    std::vector<uint64_t> part(n);
    return group_all(h, [&](swim_handle* s) {
      const int rc = swim_debug_fallbacks(s, part.data(), n);
      for (size_t i = 0; rc == SWIM_OK && i < n; ++i) out[i] += part[i];
      return rc;
    });
  }
  if (!h->d.fb) return SWIM_EUNSUPPORTED;  // not counted (SWIM_CAPS / SWIM_FALLBACKS unset at create)
  HIPCK(hipStreamSynchronize(h->stream));
  HIPCK(hipMemcpy(out, h->d.fb, 8 * n, hipMemcpyDeviceToHost));
  return SWIM_OK;
}

int swim_debug_caps(swim_handle* h, uint64_t* out, size_t n) {
  if (!h || !out || n > 8) return SWIM_EINVAL;
  if (h->grp) return SWIM_EUNSUPPORTED;
  const uint64_t v[8] = {h->d.SPR, h->d.BCAP, h->d.RCAP, h->d.RPCAP, h->d.HCAP, h->growths, 0, 0};
  for (size_t i = 0; i < n; ++i) out[i] = v[i];
  return SWIM_OK;
}

int swim_debug_holders(swim_handle* h, uint32_t first, uint32_t n, uint32_t* out) {
  if (!h || !out) return SWIM_EINVAL;
  if (h->grp) return SWIM_EUNSUPPORTED;
  const Dev& d = h->d;
  if (d.W > 1 || (uint64_t)first + n > d.N) return d.W > 1 ? SWIM_EUNSUPPORTED : SWIM_EINVAL;
  if (n == 0) return SWIM_OK;
  uint32_t* buf = nullptr;
  HIPCK(hipMalloc(&buf, 20ull * n));
  launch_dbg_holders(d, first, n, buf, h->stream);
  HIPCK(hipStreamSynchronize(h->stream));
  const hipError_t e = hipMemcpy(out, buf, 20ull * n, hipMemcpyDeviceToHost);
  hipFree(buf);
  HIPCK(e);
  return SWIM_OK;
}

// one pass over the key plane: the clean (row, chunk) pairs that differ from the chunk's first clean row, and the
// dirty pairs
static int dirty_check(swim_handle* h, uint32_t* viol, uint64_t* dirty) {
  uint32_t* buf = nullptr;
  HIPCK(hipMalloc(&buf, 8 + 4ull * h->d.NCHUNK));
  hipError_t e = hipMemsetAsync(buf, 0, 8, h->stream);
  uint32_t r[2] = {0, 0};
  if (e == hipSuccess) {
    launch_dirty_check(h->d, buf, buf + 1, buf + 2, h->stream);
    e = hipStreamSynchronize(h->stream);
  }
  if (e == hipSuccess) e = hipMemcpy(r, buf, 8, hipMemcpyDeviceToHost);
  hipFree(buf);
  HIPCK(e);
  *viol = r[0];
  *dirty = r[1];
  return SWIM_OK;
}

int swim_debug_set_incarnation(swim_handle* h, uint32_t m, uint32_t inc) {
  if (!h) return SWIM_EINVAL;
  if (h->grp || h->d.W > 1) return SWIM_EUNSUPPORTED;
  const Dev& d = h->d;
  if (m >= d.N || d.implicit) return SWIM_EINVAL;
  if (inc >= INC_LIMIT) return SWIM_ECAPACITY;
  HIPCK(hipStreamSynchronize(h->stream));
  if (h->tick > 0) {  // a SYNC / SYNC_ACK of m still in flight carries m's live row: the host write would reach it
    const uint32_t b = (uint32_t)((h->tick - 1) & 1);
    std::vector<SyncMsg> v;
    if (const int rc = msgs_read(h, b, v)) return rc;
    for (const SyncMsg& q : v)
      if (q.src == m && q.payload == NEVER && !(q.kind & KF_DEFER)) {
        h->err = "swim_debug_set_incarnation: member " + std::to_string(m) + " has a live-row payload in flight";
        return SWIM_EINVAL;
      }
  }
  uint32_t k = 0;
  HIPCK(hipMemcpy(&k, d.rowk + lidx(d, m) * d.NS + m, 4, hipMemcpyDeviceToHost));
  launch_key_set(d, m, m, (inc << 2) | (k & 3u), h->stream);  // (the key, its shadow and the row's dirty mask)
  lf_off(h);  // a row no longer equals the baseline: the lister's verdict is no constant
  HIPCK(hipStreamSynchronize(h->stream));
  return SWIM_OK;
}

int swim_debug_diff_dirty(swim_handle* h, uint64_t* out, size_t n) {
  if (!h || !out || n > 10) return SWIM_EINVAL;
  if (h->grp || h->d.W > 1 || !h->d.MW) return SWIM_EUNSUPPORTED;
  const Dev& d = h->d;
  HIPCK(hipStreamSynchronize(h->stream));
  unsigned long long c[C_NCTR];
  HIPCK(hipMemcpy(c, d.ctr, sizeof(c), hipMemcpyDeviceToHost));
  unsigned long long lf[3];
  {  // what the receivers counted in the lister's place
    std::vector<unsigned long long> sh((size_t)CSH * CSTRIDE);
    HIPCK(hipMemcpy(sh.data(), d.ctr_sh, 8 * sh.size(), hipMemcpyDeviceToHost));
    lf_counts(sh, lf);
    c[C_DIFFMSG_ALL] += lf[1];
    c[C_DMSGSKIP] += lf[1];
  }
  // every narrow payload (listed or decided by the lister) has NCHUNK chunks: streamed or skipped
  const unsigned long long narrow = c[C_DIFFMSG_ALL] - std::min(c[C_DIFFMSG_ALL], c[C_DIFFWIDE_ALL]);
  uint32_t viol = 0;
  uint64_t dirty = 0;
  int rc;
  if (n > SWIM_DD_DIRTY_ROWS && (rc = dirty_check(h, &viol, &dirty)) != SWIM_OK) return rc;
  unsigned long long pindec = 0;
  HIPCK(hipMemcpy(&pindec, d.ctr_sh + SH_PINDEC, 8, hipMemcpyDeviceToHost));
  const uint64_t v[10] = {narrow * d.NCHUNK - c[C_DSTREAM], c[C_DSTREAM], c[C_DMSGSKIP], h->rebases, dirty,
                          pindec + lf[2], h->diff_elided, h->diff_halts, h->lf_ticks, h->lf_stops};
  for (size_t i = 0; i < n; ++i) out[i] = v[i];
  return SWIM_OK;
}

int swim_debug_dirty_check(swim_handle* h, uint64_t* violations) {
  if (!h || !violations) return SWIM_EINVAL;
  if (h->grp || h->d.W > 1 || !h->d.MW) return SWIM_EUNSUPPORTED;
  uint32_t viol = 0;
  uint64_t dirty = 0;
  const int rc = dirty_check(h, &viol, &dirty);
  *violations = viol;
  return rc;
}

// debugging aid (not part of the ABI header): the gossip send log of SWIM_SEND_LOG (tick, sender, gid lo/hi, target)
int swimdbg_send_log(swim_handle* h, uint32_t* out, size_t cap, size_t* n) {
  if (!h || !h->d.dbg_send) return SWIM_EINVAL;
  HIPCK(hipStreamSynchronize(h->stream));
  uint32_t cnt = 0;
  HIPCK(hipMemcpy(&cnt, h->d.dbg_send_n, 4, hipMemcpyDeviceToHost));
  cnt = std::min<uint32_t>(cnt, h->d.dbg_send_cap);
  cnt = (uint32_t)std::min<size_t>(cnt, cap);
  HIPCK(hipMemcpy(out, h->d.dbg_send, 20ull * cnt, hipMemcpyDeviceToHost));
  *n = cnt;
  return SWIM_OK;
}

// debugging aid (not part of the ABI header): the message buffer of the latest tick as the host readers walk it
// (msgs_read). out[0] shards (Dev::msh), out[1] Q, out[2] R, out[3] messages in fast slots, out[4] in overflow slots,
// out[5] the highest slot in use (~0: none), out[6] 1 if every message read from its slot names a member as its sender
int swimdbg_msg_slots(swim_handle* h, uint64_t* out) {
  if (!h || !out || h->grp || h->d.W > 1 || h->d.XW > 1 || h->d.implicit || h->tick == 0) return SWIM_EINVAL;
  HIPCK(hipStreamSynchronize(h->stream));
  const Dev& d = h->d;
  const MsgLayout L = msg_layout(d.MSGCAP, d.msh);
  std::vector<SyncMsg> v;
  std::vector<uint32_t> slots;
  if (const int rc = msgs_read(h, (uint32_t)((h->tick - 1) & 1), v, &slots)) return rc;
  uint64_t nfast = 0, ok = 1;
  for (uint32_t i : slots) nfast += i < L.R;
  for (const SyncMsg& q : v) ok &= q.src < d.N && q.dst < d.N;
  out[0] = L.S, out[1] = L.Q, out[2] = L.R, out[3] = nfast, out[4] = slots.size() - nfast;
  out[5] = slots.empty() ? ~0ull : slots.back(), out[6] = ok;
  return SWIM_OK;
}

// debugging aid (not part of the ABI header): the scalar fields folded into the "misc" state-hash word (out[0..5]),
// then the member's pending ping paths and subscriptions (out[6], out[7]: MS::npath, MS::nsub)
int swimdbg_scalars(swim_handle* h, uint32_t m, uint64_t* out) {
  if (!h || !owns(h, m)) return SWIM_EINVAL;
  HIPCK(hipStreamSynchronize(h->stream));
  MS ms;
  uint32_t ns = 0, ng = 0, fg = 0;
  HIPCK(hipMemcpy(&ms, h->d.ms + m, sizeof(MS), hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(&ns, h->d.nextSync + m, 4, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(&ng, h->d.nextGossip + m, 4, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(&fg, h->d.firstGossip + m, 4, hipMemcpyDeviceToHost));
  const uint32_t gp = fg == NEVER ? 0u : (ng - fg) / h->d.gossip_t;  // gossip_period (dev_util.h), on the host
  const uint32_t v[6] = {ms.cidCnt, ms.syncSeq, ms.gCounter, ns, ms.fdPeriod, gp};
  for (int i = 0; i < 6; ++i) out[i] = (i == 3 && v[i] == NEVER) ? ~0ull : v[i];
  out[6] = ms.npath;
  out[7] = ms.nsub;
  return SWIM_OK;
}

// debugging aid (not part of the ABI header): one member's gossip-round ring: [tick, spread, cnt, targets...] x LOGW
int swimdbg_read_log(swim_handle* h, uint32_t m, uint32_t* out, size_t cap, uint32_t* logw, uint32_t* fanout,
                     uint32_t* pos) {
  const Dev& d = h->d;
  size_t need = (size_t)d.LOGW * (3 + d.F);
  if (cap < need) return SWIM_EINVAL;
  HIPCK(hipStreamSynchronize(h->stream));
  std::vector<uint32_t> t(d.LOGW), sp(d.LOGW), c(d.LOGW), tg((size_t)d.LOGW * d.F);
  HIPCK(hipMemcpy(t.data(), d.log_tick + (size_t)m * d.LOGW, 4ull * d.LOGW, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(sp.data(), d.log_spread + (size_t)m * d.LOGW, 4ull * d.LOGW, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(c.data(), d.log_cnt + (size_t)m * d.LOGW, 4ull * d.LOGW, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(tg.data(), d.log_tg + (size_t)m * d.LOGW * d.F, 4ull * d.LOGW * d.F, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(pos, d.log_pos + m, 4, hipMemcpyDeviceToHost));
  for (uint32_t e = 0; e < d.LOGW; ++e) {
    uint32_t* o = out + (size_t)e * (3 + d.F);
    o[0] = t[e];
    o[1] = sp[e];
    o[2] = c[e];
    for (uint32_t i = 0; i < d.F; ++i) o[3 + i] = tg[(size_t)e * d.F + i];
  }
  *logw = d.LOGW;
  *fanout = d.F;
  return SWIM_OK;
}

}  // extern "C"
