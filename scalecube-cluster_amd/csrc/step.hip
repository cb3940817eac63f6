// step.hip — swim_step: the tick loop and its four paths (one GPU: a tick, a speculative batch; row shards: a
// speculative batch, a tick). The order of launches, event records, host waits and grow_caps calls on each path is
// what the results and the timed path depend on; the dumps and the profile bookkeeping are in diag.hip.
#include <cstddef>
#include "handle.h"

#include <algorithm>

using namespace swim;

namespace {

// where a swim_step(h, n) call stands: tick h->tick is the i-th of the call
struct Step {
  uint32_t n;
  uint32_t i = 0;
  uint32_t nb = 0;        // a speculative batch ends at the next scrub tick: the call's ticks before nb
  // W == 1: the front of tick k (its lister, and its SYNC diff unless the batch elides it) is not queued yet (it is
  // queued with the previous tick when it can be)
  bool need_front = true;
};

// the event set of the call's idx-th tick, if that tick is timed
const TickEvents* events_of(swim_handle* h, uint64_t tick, uint32_t idx) {
  return prof_timed(h, tick) ? &h->prof[idx] : nullptr;
}

// P0 gossip creations before the member kernel: the user gossips queued by the host
int upload_user_gossips(swim_handle* h, uint32_t k) {
  const Dev& d = h->d;
  const size_t pairs = h->ugq.size() / 2;
  if (pairs > h->ug_cap) {
    int rc;
    dfree(h, h->ug_dev);
    h->ug_dev = nullptr;
    h->ug_cap = 0;
    const size_t cap = std::max<size_t>(pairs, 1024);
    if ((rc = dalloc(h, &h->ug_dev, 2 * cap)) != SWIM_OK) return rc;
    h->ug_cap = cap;
  }
  HIPCK(hipMemcpyAsync(h->ug_dev, h->ugq.data(), h->ugq.size() * 8, hipMemcpyHostToDevice, h->stream));
  launch_user_gossips(d, k, h->ug_dev, (uint32_t)pairs, h->stream);
  lf_off(h);
  HIPCK(hipStreamSynchronize(h->stream));  // the host queue is reused after this
  h->ugq.clear();
  return SWIM_OK;
}

// One GPU, speculative batch: while no gossip slot is in use the host need not look at the flag after every member
// kernel. The rest of the call is queued as front / member pairs with no host wait; the member kernel after which
// a slot is in use raises d.halt, every later launch of the batch returns at once, and the host resumes after
// that tick with the gossip plane.
// The front of a tick is its lister and its k_sync_diff. While the handle elides (elide_on), an untimed tick's front is
// the lister alone: in a cluster whose rows agree it decides every payload and the diff would find two empty lists. A
// lister that does list something raises the diff-halt of its tick kd (HALT_DIFF): every later launch returns at once,
// member(kd) before its resets, and the host queues diff(kd) over the lists as they stand and goes on from member(kd),
// without elision until a whole batch has listed nothing (HALT_LISTED, read with the halt words): a cluster with dirty
// rows pays one extra host wait per dirty spell, not one per tick. Timed ticks keep their event-carrying diff launch.
// While the handle is lister-free as well (lf_on), an untimed tick has no front at all: member(k) runs
// straight after member(k - 1), flagged MT_NOLIST, and counts its messages in the lister's place. A member kernel that
// writes stores HALT_WROTE = its tick kw + 1: every launch of a later tick returns at once, and the host goes on from
// lister(kw + 1) with both modes off. Only the launches of speculative batches store the word (a tick run on its own,
// tick_one_gpu, leaves the mode instead), and the host clears it after every batch that set it.
int spec_batch(swim_handle* h, Step& s) {
  const Dev& d = h->d;
  const uint32_t k = (uint32_t)h->tick, i = s.i, nb = s.nb;
  const bool can = diff_elidable(d) && !h->no_elide, elide = can && h->elide_on;
  const bool lf = elide && h->lf_on;
  const uint32_t k0 = s.need_front ? k : k + 1u;  // the first tick whose front this batch queues
  auto front = [&](uint32_t kk, uint32_t jj) {
    const TickEvents* te = events_of(h, kk, jj);
    if (lf && !te) return;
    launch_diff(d, kk, h->stream, te, LS_SPEC | (lf ? LS_LF : 0u) | (elide && !te ? LS_NODIFF : 0u));
  };
  // the ticks of [from, to) that ran without a diff launch
  auto elided = [&](uint32_t from, uint32_t to) {
    uint64_t c = 0;
    for (uint32_t t = std::max(from, 1u); elide && t < to; ++t) c += !prof_timed(h, t);
    return c;
  };
  auto listerless = [&](uint32_t from, uint32_t to) { return lf ? elided(from, to) : 0ull; };  // ... without a lister
  for (uint32_t j = i; j < nb; ++j) {
    const uint32_t kj = k + (j - i);
    const TickEvents* te = events_of(h, kj, j);
    if (s.need_front) front(kj, j);
    // (the first tick's front may have been queued with the tick before it: then its lister ran)
    const uint32_t mlf = !lf ? 0u : MT_LF | (kj >= k0 && !te ? MT_NOLIST : 0u);
    launch_member(d, kj, h->stream, te, true, false, mlf);
    int wr;
    if ((wr = watch_tick_done(h, kj + 1u, true, lf)) != SWIM_OK) return wr;  // void if member(kj) halts or returned at once
    s.need_front = j + 1 == nb;
    if (!s.need_front) front(kj + 1, j + 1);
  }
  HIPCK(hipMemcpyAsync((void*)(h->hflag + HF_HALT), d.halt, HALT_WORDS * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  const volatile uint32_t* hw = h->hflag + HF_HALT;
  const uint32_t hk = hw[HALT_GOSSIP], hd = hw[HALT_DIFF], listed = hw[HALT_LISTED], hwr = hw[HALT_WROTE];
  const bool quiet = listed == h->listed_seen;
  h->listed_seen = listed;
  if (hwr != 0) HIPCK(hipMemsetAsync(&d.halt[HALT_WROTE], 0, 4, h->stream));
  if (hk != 0 && hd != 0) return fail(h, SWIM_EDEVICE, "speculative batch: a gossip halt and a diff-halt");
  if (lf && hd != 0) return fail(h, SWIM_EDEVICE, "lister-free batch: a diff-halt");
  if (lf && hwr != 0 && hk == 0) {  // member(kw) wrote: it is complete, nothing of a later tick ran
    h->lf_on = h->elide_on = false;
    const uint32_t kw = hwr - 1u;
    if (kw < k || kw >= k + (nb - i)) return fail(h, SWIM_EDEVICE, "lister-free batch: bad wrote tick");
    h->diff_elided += elided(k0, kw + 1u);
    h->lf_ticks += listerless(k0, kw + 1u);
    h->lf_stops++;
    h->gossip_ran = false;
    h->tick = kw + 1ull;
    s.i = i + (kw + 1u - k);
    s.need_front = true;  // from lister(kw + 1)
    return SWIM_OK;
  }
  if (hk == 0 && hd == 0) {  // the whole batch ran
    h->diff_elided += elided(k0, k + (nb - i));
    h->lf_ticks += listerless(k0, k + (nb - i));
    h->elide_on = quiet;
    h->tick += nb - i;
    s.i = nb;
    h->gossip_ran = false;
    if (lf) {
      h->lf_on = quiet;
    } else if (elide && quiet && hwr == 0 && nb - i >= 2 && !h->no_lf && !d.dly_on) {
      // an elided batch of two ticks or more that listed nothing and wrote nothing: both write logs the next lister
      // would read are empty. Lister-free from the next batch on if every row is clean as well (one pass, only here)
      launch_masks_any(d, h->stream);
      HIPCK(hipMemcpyAsync((void*)(h->hflag + HF_HALT + HALT_MASKS), &d.halt[HALT_MASKS], 4, hipMemcpyDeviceToHost, h->stream));
      HIPCK(hipStreamSynchronize(h->stream));
      h->lf_on = hw[HALT_MASKS] == 0;
    }
    return SWIM_OK;
  }
  if (hd != 0) {  // lister(kd) listed work and no diff was queued: ticks before kd are complete, member(kd) has not run
    const uint32_t kd = hd - 1u;
    if (!elide || kd < k0 || kd >= k + (nb - i) || prof_timed(h, kd))
      return fail(h, SWIM_EDEVICE, "speculative batch: bad diff-halt tick");
    HIPCK(hipMemsetAsync(&d.halt[HALT_DIFF], 0, 4, h->stream));
    launch_diff_listed(d, kd, h->stream);
    h->diff_elided += elided(k0, kd);
    h->diff_halts++;
    h->elide_on = h->lf_on = false;
    if (kd > k) h->gossip_ran = false;
    h->tick = kd;
    s.i = i + (kd - k);
    s.need_front = false;  // lister(kd) ran (its counter adds are not idempotent) and diff(kd) is queued
    return SWIM_OK;
  }
  const uint32_t kh = hk - 1u;  // member(kh) ran; the launches after it returned at once
  if (kh < k || kh >= k + (nb - i)) return fail(h, SWIM_EDEVICE, "speculative batch: bad halt tick");
  HIPCK(hipMemsetAsync(&d.halt[HALT_GOSSIP], 0, 4, h->stream));
  const uint32_t ih = i + (kh - k);
  // a speculative member launch publishes no flag (tick_flag): the slots in use after member(kh) are read here, so
  // the first gossip plane after an idle stretch gets the same capacity check as every other one (grow_caps); the
  // device copy of the flag word follows, so tick_flag keeps writing it only on a change
  {
    int32_t top = 0;
    HIPCK(hipMemcpyAsync(&top, d.free_top, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    const uint32_t used = (uint32_t)((int32_t)d.SPR - top);
    h->hflag[HF_USED] = used;
    HIPCK(hipMemcpyAsync(&d.hsh[HSH_USED], &used, 4, hipMemcpyHostToDevice, h->stream));
    int gr;
    if ((gr = grow_caps(h)) != SWIM_OK) return gr;
  }
  launch_gossip(d, kh, h->stream, events_of(h, kh, ih));
  int wr;
  if ((wr = watch_tick_done(h, kh + 1u, false, false)) != SWIM_OK) return wr;  // (the in-batch sample of kh + 1 was void)
  h->gossip_idle = false;
  h->gossip_ran = true;
  s.need_front = true;  // the front of kh + 1 returned at once
  h->diff_elided += elided(k0, kh + 1u);
  h->lf_ticks += listerless(k0, kh + 1u);
  // gossips change rows: the next batch queues its listers and diffs and looks at what the lister lists
  h->elide_on = h->lf_on = false;
  h->tick = kh + 1ull;
  s.i = ih + 1;
  return SWIM_OK;
}

// One GPU, one tick: diff, member kernel, the host's look at the slots in use, the gossip plane if there are any
int tick_one_gpu(swim_handle* h, Step& s) {
  const Dev& d = h->d;
  const uint32_t k = (uint32_t)h->tick, i = s.i;
  const TickEvents* te = events_of(h, h->tick, i);
  lf_off(h);  // (this member launch does not say whether it wrote: HALT_WROTE is a speculative batch's word)
  // SYNC diff(k) was queued in the previous iteration, except for the first tick of this call
  if (s.need_front) launch_diff(d, k, h->stream, te);
  launch_member(d, k, h->stream, te, false, h->gossip_ran && !d.fastp4);
  const bool nosync = (d.exp & EXP_NO_EVENT) != 0;  // timing experiment: no per-tick event (gossip plane never launched)
  if (!nosync) HIPCK(hipEventRecord(h->ev_member, h->stream));
  const bool pipe = i + 1 < s.n && !h->no_pipe;
  if (pipe) launch_diff(d, k + 1, h->stream, events_of(h, k + 1ull, i + 1));  // overlaps the wait
  s.need_front = !pipe;
  if (!nosync) HIPCK(hipEventSynchronize(h->ev_member));  // (a spin wait measured the same here: diff(k+1) hides the wake-up)
  h->gossip_idle = !nosync && h->hflag[HF_USED] == 0;
  if (!nosync && !h->gossip_idle) {  // slots, rings and receipt lists sized up before they can overflow
    int gr;
    if ((gr = grow_caps(h)) != SWIM_OK) return gr;
  }
  h->gossip_ran = !nosync && (h->hflag[HF_USED] != 0 || h->no_skip);
  if (nosync) {
  } else if (h->hflag[HF_USED] != 0 || h->no_skip) {
    launch_gossip(d, k, h->stream, te);
    lf_off(h);
    int sr;
    if (h->stats && (sr = stats_dump(h, k)) != SWIM_OK) return sr;
  } else if (te && te->all) {
    HIPCK(hipEventRecord((hipEvent_t)te->ev[4], h->stream));
    HIPCK(hipEventRecord((hipEvent_t)te->ev[5], h->stream));
  }
  if (d.XW > 1) {  // slot sharding: the members' gossip counts, every tick (collective)
    int xr;
    if ((xr = held_allreduce(h)) != SWIM_OK) return xr;
  }
  int wr;
  if ((wr = watch_tick_done(h, k + 1u, false, false)) != SWIM_OK) return wr;  // (diff(k + 1), if queued, writes no row)
  h->tick++;
  ++s.i;
  return SWIM_OK;
}

// the rest of a row-sharded tick after its exchange A: B, the exchange of first receipts, C, growth
int shard_tick_rest(swim_handle* h, uint32_t k, const TickEvents* te) {
  const Dev& d = h->d;
  int xr;
  const bool gossip = h->xflag;
  launch_tick_b(d, k, h->stream, te, gossip);
  if (gossip && (xr = exchange(h, d.xb_send, d.xb_recv, d.XB_PEER, d.xb_scnt, d.xb_rcnt, false)) != SWIM_OK) return xr;
  launch_tick_c(d, k, h->stream, gossip);
  if (gossip && (xr = grow_caps_shard(h)) != SWIM_OK) return xr;
  return SWIM_OK;
}

// Row shards, speculative batch: while no shard has a gossip slot in use and every exchange-A region fits its inline
// block, a tick needs nothing from the host. The rest of the call is queued as A / inline all-to-all / B with
// no host wait; the gate after the all-to-all of the first tick that needs the host (the same tick on every
// shard: the flags ride on the exchanged count words) raises d.halt, every later launch returns at once (the
// all-to-alls still run, carrying nothing anyone reads), and the host finishes that tick on the normal path.
int shard_spec_batch(swim_handle* h, Step& s) {
  const Dev& d = h->d;
  const uint32_t k = (uint32_t)h->tick, i = s.i, nb = s.nb;
  int xr;
  for (uint32_t j = i; j < nb; ++j) {
    const uint32_t kj = k + (j - i);
    const TickEvents* tj = events_of(h, kj, j);
    launch_tick_a(d, kj, h->stream, tj, true);
    if ((xr = exchange_inline(h, d.xa_recv, d.XA_PEER, d.xa_scnt, d.xa_rcnt, true)) != SWIM_OK) return xr;
    launch_tick_b(d, kj, h->stream, tj, false, true);
    if ((xr = watch_tick_done(h, kj + 1u, true, false)) != SWIM_OK) return xr;  // void from the gate's halt of kj on
  }
  HIPCK(hipMemcpyAsync((void*)(h->hflag + HF_SHARD_HALT), &d.halt[HALT_GOSSIP], 4, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  const uint32_t hk = h->hflag[HF_SHARD_HALT];
  if (hk == 0) {
    h->tick += nb - i;
    s.i = nb;
    return SWIM_OK;
  }
  const uint32_t kh = hk - 1u;  // tick kh ran up to its inline exchange; the launches after that returned at once
  if (kh < k || kh >= k + (nb - i)) return fail(h, SWIM_EDEVICE, "speculative sharded batch: bad halt tick");
  HIPCK(hipMemsetAsync(&d.halt[HALT_GOSSIP], 0, 4, h->stream));
  const uint32_t ih = i + (kh - k);
  if ((xr = exchange_rest(h, d.xa_send, d.xa_recv, d.XA_PEER)) != SWIM_OK) return xr;
  if ((xr = shard_tick_rest(h, kh, events_of(h, kh, ih))) != SWIM_OK) return xr;
  if ((xr = watch_tick_done(h, kh + 1u, false, false)) != SWIM_OK) return xr;
  h->tick = kh + 1ull;
  s.i = ih + 1;
  return SWIM_OK;
}

// Row shards, one tick: A, exchange A (the host waits for it: the gossip flag and the sizes), then the rest
int shard_tick(swim_handle* h, Step& s) {
  const Dev& d = h->d;
  const uint32_t k = (uint32_t)h->tick;
  const TickEvents* te = events_of(h, h->tick, s.i);
  int xr;
  launch_tick_a(d, k, h->stream, te);
  if ((xr = exchange(h, d.xa_send, d.xa_recv, d.XA_PEER, d.xa_scnt, d.xa_rcnt, true)) != SWIM_OK) return xr;
  if ((xr = shard_tick_rest(h, k, te)) != SWIM_OK) return xr;
  if ((xr = watch_tick_done(h, k + 1u, false, false)) != SWIM_OK) return xr;
  h->tick++;
  ++s.i;
  return SWIM_OK;
}

}  // namespace

// One GPU with dirty-chunk skipping: the baseline follows the cluster. The lister counts, per chunk,
// the compares it had streamed because the chunk was dirty, the diff those that found a difference; once the wasted
// ones (streamed without a difference) since the chunk's last rebase reach the number of rows, the chunk's baseline
// becomes some sender's chunk (k_rebase: one pass over the chunk of every row, about what those compares cost), and
// the rows that agree with it are clean again. Called between ticks, where the host holds no queued member launch; the
// counters are read back only when the lister flagged a streamed chunk (never in a cluster whose rows are all clean).
static int rebase_check(swim_handle* h) {
  const Dev& d = h->d;
  if (h->tick < h->next_rebase || !h->hflag[HF_STREAMED]) return SWIM_OK;
  h->next_rebase = h->tick + h->rb_int;
  h->hflag[HF_STREAMED] = 0;
  std::vector<unsigned long long> c(3ull * d.NCHUNK);  // chunk q's streamed, differed, sender: member q's record
  HIPCK(hipMemcpy2DAsync(c.data(), 24, (const char*)d.ms + offsetof(MS, cstat), sizeof(MS), 24, d.NCHUNK, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  const unsigned long long thr = h->rb_thr ? h->rb_thr : d.NL;
  for (uint32_t q = 0; q < d.NCHUNK; ++q) {
    const unsigned long long st = c[3ull * q], df = c[3ull * q + 1], r = c[3ull * q + 2];
    if (st < df + thr || r >= d.NL) continue;
    launch_rebase(d, q, (uint32_t)r, h->stream);
    lf_off(h);  // (the masks change)
    h->rebases++;
  }
  return SWIM_OK;
}

extern "C" int swim_step(swim_handle* h, uint32_t n) {
  if (!h) return SWIM_EINVAL;
  if (h->grp) return group_step(h, n);
  hipSetDevice((int)h->cfg.device);
  if (h->tick + n >= (1ull << 28)) return SWIM_ECAPACITY;  // deadlines are stored in 29 bits
  int rc;
  if ((rc = prof_prepare(h, n)) != SWIM_OK) return rc;
  if (!h->recording.empty()) watch_record_prune(h);
  const uint64_t first = h->tick;
  const Dev& d = h->d;
  const bool no_batch = d.churn || h->no_spec || (h->cfg.flags & SWIM_FLAG_PROFILE_ALL);  // (PROFILE_ALL times every tick's gossip plane)
  Step s{n};
  while (s.i < n) {
    const uint32_t k = (uint32_t)h->tick;
    if (h->tick >= h->next_scrub) {  // stale holder entries of recycled slots, before they can alias (engine.h)
      launch_s_scrub(d, k, h->stream);
      h->next_scrub = h->tick + SCRUB;
    }
    s.nb = (uint32_t)std::min<uint64_t>(n, s.i + (h->next_scrub - h->tick));
    if ((d.ackres & ACKRES_DIRTY) && d.W == 1 && (rc = rebase_check(h)) != SWIM_OK) return rc;
    // P0 gossip creations before the member kernel: RUMOR-mode churn rumors, then the user gossips queued by the host
    if (d.churn && k % d.ping_t == 0) launch_churn(d, k, h->stream);
    if (s.i == 0 && !h->ugq.empty() && (rc = upload_user_gossips(h, k)) != SWIM_OK) return rc;
    if (d.W == 1 && h->gossip_idle && s.i + 1 < s.nb && d.XW == 1 && !h->no_pipe && !h->no_skip && !no_batch)
      rc = spec_batch(h, s);
    else if (d.W == 1)
      rc = tick_one_gpu(h, s);
    else if (h->spec.transport == SWIM_TRANSPORT_RCCL && !h->xflag && s.i + 1 < s.nb && !no_batch)
      rc = shard_spec_batch(h, s);
    else
      rc = shard_tick(h, s);
    if (rc != SWIM_OK) return rc;
  }
  rc = check_err(h);
  if (rc == SWIM_OK && (d.exp & EXP_CYCLES)) rc = exp_dump_member_cycles(h);
  if (rc == SWIM_OK && (d.exp & EXP_WAVE_CLOCK)) rc = exp_dump_wave_clock(h);
  if (rc == SWIM_OK && (d.exp & EXP_GOSSIP_WORK)) rc = exp_dump_gossip_work(h);
  if (rc == SWIM_OK) rc = prof_accumulate(h, first, n);
  return rc;
}
