// handle.h — private to libswimhip's host side: the handle behind include/swimhip.h and what its source files share.
//   create.hip    swim_config + environment -> Dev, the allocation table, initialisation
//   grow.hip      capacity growth between ticks
//   exchange.hip  the shard exchanges and their transports
//   step.hip      swim_step: the four tick paths
//   diag.hip      SWIM_STATS / SWIM_EXP dumps, profile events
//   group.hip     swim_config.n_gpus > 1: one handle over several shard handles
//   api.hip       the other extern "C" entry points: fault injection, readback
//   debug_receipts.hip  swim_debug_receipts_set / _read: injected P4 receipts (tests)
//   watch.hip     swim_watch_* / swim_run_until: the subject watch, its kernel and its recording included
// The device side (engine.h, spec.h, dev_util.h): member.hip (member control: triage, phases, k_member_tick_t) over
// member_state.h (a member's state, row writes, SYNC sends) and member_proto.h (the protocol handlers), inbox.hip
// (k_inbox_apply: P4 of a parked member on one wave), user_gossip.hip (host-queued gossips, churn), sync_diff.hip (SYNC
// diff and its lister), sync_delay.hip (delayed-SYNC store), route.hip (receipt routing), gossip_round.hip /
// gossip_contacts.hip / gossip_send.hip / gossip_apply.hip (the gossip data plane by stage, over gossip_dev.h and
// gossip_replay.h: the file map is in gossip_dev.h), shard.hip (row-shard pack / unpack), kernels.hip (initialisation, state hashes, the tick launchers; the
// member kernels it launches are declared in member_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/swimhip.h"
#include "../../include/swimhip_shard.h"
#include "dev_alloc.h"
#include "engine.h"

struct Group;  // group.hip
struct swim_watch;  // watch.hip

struct swim_handle {
  swim_config cfg;
  swim::Dev d;
  hipStream_t stream = nullptr;
  uint64_t tick = 0;
  std::string err;
  swim::DevAllocs mem;  // every device allocation; mem.bytes is swim_counters.device_bytes
  std::vector<swim_event> host_events;
  // settings-epoch ring mirrored on the host
  uint32_t ep_from[swim::MAX_EPOCHS], ep_loss[swim::MAX_EPOCHS], ep_part[swim::MAX_EPOCHS], ep_delay[swim::MAX_EPOCHS];
  int cur_ep = 0;
  uint32_t loss = 0;
  uint32_t delay_idx = 0;                 // default mean delay (index into delays)
  std::vector<uint32_t> delays{0};        // mean delay ms of each delay index (0: none)
  bool partitioned = false;
  std::vector<uint32_t> group;
  // per-link NetworkEmulator settings: current custom settings and each link's change history (mirrored to HBM)
  std::map<uint64_t, uint32_t> link_cur;
  std::map<uint64_t, std::vector<std::pair<uint32_t, uint32_t>>> link_hist;
  std::vector<swim::TickEvents> prof;  // SWIM_FLAG_PROFILE: one event set per tick of the current swim_step
  double prof_ms[3] = {0, 0, 0};  // accumulated k_sync_diff, k_member_tick, k_gossip_send
  uint64_t prof_diff_launches = 0;
  // row sharding (swimhip_shard.h)
  swim_shard_spec spec{};
  ncclComm_t comm = nullptr;
  unsigned long long* hcnt = nullptr;  // pinned [2W]: send then receive byte counts of the current exchange
  std::vector<uint8_t> hsend, hrecv;  // SWIM_TRANSPORT_HOST staging
  double xchg_ms = 0;                 // host time spent in the exchanges
  bool xflag = false;                 // last exchange: some shard has a gossip slot in use
  std::vector<uint8_t> joined;  // swim_join: dormant members that were started
  std::vector<uint32_t> md_cols;  // swim_update_metadata: members that own a metadata-version column
  std::vector<uint64_t> ugq;  // swim_spread_gossip queue: (member, payload) pairs for P0 of the next tick
  uint64_t* ug_dev = nullptr;  // device copy of ugq
  size_t ug_cap = 0;
  volatile uint32_t* hflag = nullptr; // host-mapped flag word written by k_tick_flag (W == 1)
  unsigned long long* xi_host_h = nullptr;  // host side of Dev::xi_host
  hipEvent_t ev_member = nullptr;
  // rebasing (step.hip rebase_check): a chunk's baseline is replaced once rb_thr streamed compares of it found no
  // difference (0: as many as there are rows), looked at no more often than every rb_int ticks (SWIM_CAPS rbt=, rbi=)
  uint32_t rb_thr = 0, rb_int = swim::REBASE_CHECK;
  uint64_t next_rebase = 0;  // tick of the next look at the rebase counters (step.hip rebase_check)
  uint64_t rebases = 0;  // k_rebase runs since create (swim_debug_diff_dirty)
  uint64_t next_scrub = swim::SCRUB;  // tick of the next k_s_scrub (16-bit holder entries, engine.h)
  bool no_skip = getenv("SWIM_NO_GOSSIP_SKIP") != nullptr;  // debugging aid: always run the gossip data plane
  bool no_pipe = getenv("SWIM_NO_PIPELINE") != nullptr;    // debugging aid: no early SYNC diff of the next tick
  bool no_spec = getenv("SWIM_NO_SPECULATION") != nullptr;  // debugging aid: a host wait after every member kernel
  // one GPU (engine.h diff_elidable): speculative batches queue no k_sync_diff on untimed ticks while elide_on
  // (step.hip spec_batch); SWIM_NO_ELIDE keeps a diff launch on every tick (measurements, the tests' reference path)
  bool no_elide = getenv("SWIM_NO_ELIDE") != nullptr;
  bool elide_on = true;       // off after a diff-halt or a gossip plane, on again after a batch that listed nothing
  uint32_t listed_seen = 0;   // Dev::halt[HALT_LISTED] as last read
  uint64_t diff_elided = 0;   // ticks run without a k_sync_diff launch (swim_debug_diff_dirty)
  uint64_t diff_halts = 0;    // batches stopped by a diff-halt
  // the lister-free mode (step.hip spec_batch), a stricter sibling of elide_on: untimed ticks of a
  // speculative batch queue no lister either. Entered after a whole elided batch that listed nothing and wrote nothing
  // (Dev::halt[HALT_WROTE]) when no delay is set and every dirty mask is zero; left when a member kernel writes, when a
  // gossip plane runs, and by every host call that touches rows, masks, messages or link settings (lf_off).
  // SWIM_NO_LISTERFREE keeps the lister on every tick (measurements, the tests' reference path)
  bool no_lf = getenv("SWIM_NO_LISTERFREE") != nullptr;
  bool lf_on = false;
  uint64_t lf_ticks = 0;  // ticks run without a lister launch (swim_debug_diff_dirty)
  uint64_t lf_stops = 0;  // batches the wrote word stopped
  bool gossip_idle = false;  // W == 1: no gossip slot was in use after the latest member kernel
  bool gossip_ran = false;   // W == 1: the latest tick ran the gossip plane (the next P4 may have routed receipts)
  uint64_t growths = 0;      // capacity growth steps so far (grow_caps)
  uint64_t grow_next = 0;    // grow_caps: no attempt before this tick (the last one found no room)
  bool rx_pinned = false;    // SWIM_CAPS rx= at create: slot growth keeps Dev::CRCAP
  // timing aid (bench.py --rehearse-shard): a slot shard alone, its peers' gossip-count deltas taken as zero without
  // any exchange (not the W-shard simulation's results)
  bool lone = getenv("SWIM_LONE_SHARD") != nullptr;
  // timing aid (SWIM_STATS): the gossip plane's work per tick on stderr (routed receipts, targets, active groups,
  // replay / slow-path sends, contact pairs, RX rows); one stream wait per tick
  bool stats = getenv("SWIM_STATS") != nullptr;
  // swim_debug_receipts_set (debug_receipts.hip): the gossip slots its records took off the free stack, the tick they
  // were installed for, and whether an injection is there to read back
  std::vector<uint32_t> dbg_slots;
  uint64_t dbg_tick = 0;
  bool dbg_armed = false;
  std::vector<swim_watch*> watches;  // the handle's live watches (swimhip_watch.h): swim_destroy frees what is left
  // those of them with a recording armed (swimhip_watch_series.h): step.hip queues their samples where a tick comes to
  // rest (watch_tick_done); empty unless a recording is armed
  std::vector<swim_watch*> recording;  // (a full series leaves it at the next swim_step's start)
  Group* grp = nullptr;  // n_gpus > 1: every call is forwarded to the shards (d holds shard 0's constants only)
};

#define HIPCK(expr)                                                        \
  do {                                                                     \
    hipError_t e_ = (expr);                                                \
    if (e_ != hipSuccess) {                                                \
      h->err = std::string(#expr " -> ") + hipGetErrorString(e_);          \
      return SWIM_EDEVICE;                                                 \
    }                                                                      \
  } while (0)

namespace swim {
#pragma GCC visibility push(hidden)

// a failed DevAllocs::alloc / Staged::add as the handle's error
inline int alloc_failed(swim_handle* h) {
  h->err = h->mem.err;
  return SWIM_ENOMEM;
}

// `count` elements (at least one) of device memory, registered with the handle
template <class T>
int dalloc(swim_handle* h, T** p, size_t count) {
  *p = (T*)h->mem.alloc((count ? count : 1) * sizeof(T));
  return *p ? SWIM_OK : alloc_failed(h);
}
inline void dfree(swim_handle* h, void* p) { h->mem.free(p); }

// a host call changed something the lister's verdict depends on: the next batch queues its listers again
inline void lf_off(swim_handle* h) { h->lf_on = false; }

inline int fail(swim_handle* h, int rc, const std::string& what) {
  h->err = what;
  return rc;
}

// Host -> device update of engine state between ticks: ordered on the engine stream, so the next tick's kernels see
// it (a plain hipMemcpy runs on the null stream, which a non-blocking stream does not wait for), and finished before
// returning (the source is often a stack or vector buffer)
inline hipError_t h2d(hipStream_t st, void* dst, const void* src, size_t bytes) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// create.hip
int create(const swim_config* cfg, const swim_shard_spec* spec, swim_handle** out);
bool delay_table(uint32_t D, uint32_t T, std::vector<uint32_t>* out);
bool to_ticks(uint32_t ms, uint32_t tick, uint32_t* out);
// api.hip
int check_err(swim_handle* h);
int push_epoch(swim_handle* h);
// grow.hip
int grow_caps(swim_handle* h);
int grow_caps_shard(swim_handle* h);
// exchange.hip
int exchange_inline(swim_handle* h, uint8_t* recv, uint64_t cap, unsigned long long* scnt, unsigned long long* rcnt,
                    bool spec);
int exchange_rest(swim_handle* h, uint8_t* send, uint8_t* recv, uint64_t cap);
int exchange(swim_handle* h, uint8_t* send, uint8_t* recv, uint64_t cap, unsigned long long* scnt,
             unsigned long long* rcnt, bool inline_packed);
int held_allreduce(swim_handle* h);
// api.hip: the messages of buffer b (one GPU, the stream idle), its slots in use in ascending slot order
// (msg_slots.h); slots: each one's slot
int msgs_read(swim_handle* h, uint32_t b, std::vector<SyncMsg>& out, std::vector<uint32_t>* slots = nullptr);
// diag.hip
int stats_dump(swim_handle* h, uint32_t k);
int exp_dump_member_cycles(swim_handle* h);
int exp_dump_wave_clock(swim_handle* h);
int exp_dump_gossip_work(swim_handle* h);

int prof_prepare(swim_handle* h, uint32_t n);
bool prof_timed(const swim_handle* h, uint64_t tick);
int prof_accumulate(swim_handle* h, uint64_t first, uint32_t n);
// group.hip
int create_group(const swim_config* cfg, swim_handle** out);
int group_step(swim_handle* h, uint32_t n);
void group_destroy(swim_handle* h);
// watch.hip
void watch_free_all(swim_handle* h);
int watch_record_tick(swim_handle* h, uint32_t t, bool in_batch, bool lf);
void watch_record_prune(swim_handle* h);
// The state at rest at tick t exists once everything queued so far has run: the armed recordings' samples of t go
// behind it. in_batch: queued inside a speculative batch (lf: a lister-free one), where the launches before it may
// return at once: the sample then reads the halt words (spec.h halted_sample) and the host queues it again where it
// resumes. No recording armed: nothing is queued.
inline int watch_tick_done(swim_handle* h, uint32_t t, bool in_batch, bool lf) {
  return h->recording.empty() ? SWIM_OK : watch_record_tick(h, t, in_batch, lf);
}

#pragma GCC visibility pop
}  // namespace swim
