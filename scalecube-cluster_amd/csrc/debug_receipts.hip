// debug_receipts.hip — test surface (include/swimhip_debug.h): routed gossip receipts of the next tick's P4 installed
// into a live one-GPU handle by host copies, and the per-member state that P4 leaves read back. No kernel of its own:
// the member kernels that run the injected receipts are the engine's, launched by swim_step as on any tick.
#include <algorithm>
#include <cstring>

#include "../../include/swimhip_debug.h"
#include "handle.h"

using namespace swim;

static_assert(SWIM_DEBUG_TL == TL && SWIM_DEBUG_FREC == FREC, "swimhip_debug.h mirrors engine.h");

namespace {

int d2h(swim_handle* h, void* dst, const void* src, size_t bytes) {
  if (bytes) HIPCK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return SWIM_OK;
}

int injectable(swim_handle* h) {
  if (!h || h->grp) return SWIM_EINVAL;
  const Dev& d = h->d;
  if (d.W != 1 || d.XW != 1 || d.mode != 0 || d.implicit || d.fastp4) return SWIM_EINVAL;
  return SWIM_OK;
}

}  // namespace

extern "C" {

int swim_debug_receipts_set(swim_handle* h, const uint32_t* recs, size_t n_recs, const uint32_t* lists, size_t n_words,
                            uint32_t split) {
  int rc;
  if ((rc = injectable(h)) != SWIM_OK) return rc;
  const Dev& d = h->d;
  const uint32_t N = d.N;
  if ((n_recs && !recs) || (n_words && !lists) || split > 1) return SWIM_EINVAL;
  if (!h->dbg_slots.empty()) return fail(h, SWIM_EINVAL, "swim_debug_receipts_set: the last injection was not read back");
  if (!h->ugq.empty()) return fail(h, SWIM_EINVAL, "swim_debug_receipts_set: user gossips are queued");
  // ---- everything checked on the host before anything is written ----
  for (size_t i = 0; i < n_recs; ++i) {
    const uint32_t* r = recs + 6 * i;
    if (r[0] == SWIM_DEBUG_REC_MEMBER) {
      if (r[1] >= N || r[2] < ST_ALIVE || r[2] > ST_DEAD || r[4] >= N) return SWIM_EINVAL;
    } else if (r[0] == SWIM_DEBUG_REC_USER) {
      if (r[1] >= N || r[4] != 0) return SWIM_EINVAL;
    } else {
      return SWIM_EINVAL;
    }
  }
  std::vector<uint32_t> cnt(N, 0u), off(N, 0u), ndrop(N, 0u), slot_of;
  std::vector<uint8_t> seen(N, 0);
  uint64_t total = 0;
  for (size_t w = 0; w < n_words;) {
    if (n_words - w < 3) return SWIM_EINVAL;
    const uint32_t m = lists[w], nd = lists[w + 1], c = lists[w + 2];
    if (m >= N || seen[m] || c > n_words - w - 3) return SWIM_EINVAL;
    for (uint32_t j = 0; j < c; ++j)
      if (lists[w + 3 + j] >= n_recs) return SWIM_EINVAL;
    seen[m] = 1;
    cnt[m] = c;
    off[m] = (uint32_t)total;
    ndrop[m] = nd;
    total += c;
    if (total > d.RCAP) return SWIM_EINVAL;
    w += 3 + c;
  }
  HIPCK(hipStreamSynchronize(h->stream));
  int32_t top = 0;
  uint32_t rcn = 0;
  if ((rc = d2h(h, &top, d.free_top, 4)) != SWIM_OK || (rc = d2h(h, &rcn, d.rc_n, 4)) != SWIM_OK) return rc;
  // a slot in use or a routed receipt: the engine's own receipts of the next tick would collide with the injected ones
  if (top != (int32_t)d.SPR || rcn != 0) return fail(h, SWIM_EINVAL, "swim_debug_receipts_set: gossips in flight");
  if (n_recs > (size_t)top) return SWIM_EINVAL;
  // ---- the records' slots: the top n_recs entries of the free stack, taken off it (slot_used stays 0) ----
  std::vector<uint32_t> g(n_recs);
  if ((rc = d2h(h, g.data(), d.free_list + (top - (int32_t)n_recs), 4 * n_recs)) != SWIM_OK) return rc;
  for (uint32_t s : g)
    if (s >= d.SLOTS) return fail(h, SWIM_EDEVICE, "swim_debug_receipts_set: free list entry past the slot table");
  if (n_recs) {
    // (one read-modify-write of the span the taken slots lie in: the stream is idle and the other slots go back
    // unchanged; a copy per record would be one synchronising copy each, 16 640 of them in the largest test)
    const uint32_t lo = *std::min_element(g.begin(), g.end()), hi = *std::max_element(g.begin(), g.end()) + 1u;
    std::vector<uint32_t> subj(hi - lo);
    std::vector<uint64_t> key(hi - lo), gid(hi - lo);
    if ((rc = d2h(h, subj.data(), d.slot_subj + lo, 4ull * (hi - lo))) != SWIM_OK ||
        (rc = d2h(h, key.data(), d.slot_key + lo, 8ull * (hi - lo))) != SWIM_OK ||
        (rc = d2h(h, gid.data(), d.slot_gid + lo, 8ull * (hi - lo))) != SWIM_OK)
      return rc;
    for (size_t i = 0; i < n_recs; ++i) {
      const uint32_t* r = recs + 6 * i;
      const uint32_t q = g[i] - lo;
      if (r[0] == SWIM_DEBUG_REC_MEMBER) {
        subj[q] = r[1];
        key[q] = rec_key(r[2], r[3]);
        gid[q] = ((uint64_t)r[4] << 32) | r[5];
      } else {
        subj[q] = USER_SUBJ;
        key[q] = ((uint64_t)r[3] << 32) | r[2];
        gid[q] = ((uint64_t)r[1] << 32) | r[5];
      }
    }
    HIPCK(h2d(h->stream, d.slot_subj + lo, subj.data(), 4ull * (hi - lo)));
    HIPCK(h2d(h->stream, d.slot_key + lo, key.data(), 8ull * (hi - lo)));
    HIPCK(h2d(h->stream, d.slot_gid + lo, gid.data(), 8ull * (hi - lo)));
  }
  slot_of.reserve(total);
  for (size_t w = 0; w < n_words; w += 3 + lists[w + 2])  // (lists are laid out in the order their offsets were given)
    for (uint32_t j = 0; j < lists[w + 2]; ++j) slot_of.push_back(g[lists[w + 3 + j]]);
  if (total) HIPCK(h2d(h->stream, d.rc_slot, slot_of.data(), 4ull * total));
  HIPCK(h2d(h->stream, d.rc_off, off.data(), 4ull * N));
  HIPCK(h2d(h->stream, d.rc_cnt, cnt.data(), 4ull * N));
  HIPCK(h2d(h->stream, d.rc_fill, cnt.data(), 4ull * N));
  HIPCK(h2d(h->stream, d.rc_ndrop, ndrop.data(), 4ull * N));
  top -= (int32_t)n_recs;
  HIPCK(h2d(h->stream, d.free_top, &top, 4));
  // ---- the next swim_step(h, 1) runs tick_one_gpu with the chosen member launch ----
  h->dbg_slots = g;
  h->dbg_tick = h->tick;
  h->dbg_armed = true;
  h->gossip_ran = split != 0;
  h->gossip_idle = false;
  lf_off(h);
  return SWIM_OK;
}

int swim_debug_receipts_read(swim_handle* h, uint32_t first, uint32_t n, uint32_t fetch_cap, uint32_t* out,
                             uint32_t* msg_out) {
  int rc;
  if ((rc = injectable(h)) != SWIM_OK) return rc;
  const Dev& d = h->d;
  if ((uint64_t)first + n > d.N || (n && !out) || fetch_cap > d.FCAP) return SWIM_EINVAL;
  if (!h->dbg_armed) return fail(h, SWIM_EINVAL, "swim_debug_receipts_read: no injection to read");
  HIPCK(hipStreamSynchronize(h->stream));
  const uint32_t k = (uint32_t)h->dbg_tick, b = k & 1u;
  if (n) {
    const size_t stride = SWIM_DEBUG_RD_WORDS + (size_t)FREC * fetch_cap;
    std::vector<MS> ms(n);
    std::vector<uint32_t> tmin(n), held(n), tln(n, 0u), tlt(n, NEVER), tl((size_t)n * TL, 0u);
    if ((rc = d2h(h, ms.data(), d.ms + first, sizeof(MS) * n)) != SWIM_OK ||
        (rc = d2h(h, tmin.data(), d.timerMin + first, 4ull * n)) != SWIM_OK ||
        (rc = d2h(h, held.data(), d.held + first, 4ull * n)) != SWIM_OK)
      return rc;
    if (d.ackres && ((rc = d2h(h, tln.data(), d.tl_n + (size_t)b * d.NL + first, 4ull * n)) != SWIM_OK ||
                     (rc = d2h(h, tlt.data(), d.tl_tick + (size_t)b * d.NL + first, 4ull * n)) != SWIM_OK ||
                     (rc = d2h(h, tl.data(), d.tlog + ((size_t)b * d.NL + first) * TL, 4ull * n * TL)) != SWIM_OK))
      return rc;
    std::vector<uint32_t> fr((size_t)FREC * fetch_cap);
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t* o = out + stride * i;
      const MS& s = ms[i];
      const uint32_t ntl = tlt[i] == k ? tln[i] : 0u;
      const uint32_t v[9] = {s.tsize, s.cidCnt, s.nfetch, s.fnext, tmin[i], held[i], s.gCounter, s.evSeq, ntl};
      memcpy(o, v, sizeof v);
      for (uint32_t j = 0; j < TL; ++j) o[9 + j] = j < std::min(ntl, TL) ? tl[(size_t)i * TL + j] : 0u;
      const uint32_t nf = std::min(s.nfetch, fetch_cap);
      memset(o + SWIM_DEBUG_RD_WORDS, 0, 4ull * FREC * fetch_cap);
      if (nf && (rc = d2h(h, o + SWIM_DEBUG_RD_WORDS, d.fetch + (size_t)(first + i) * d.FCAP * FREC, 4ull * FREC * nf)) != SWIM_OK)
        return rc;
    }
  }
  if (msg_out) {  // the tick's message buffer: arena rows taken, messages, and per sender those whose payload is a snapshot
    uint32_t au = 0;
    std::vector<SyncMsg> v;
    if ((rc = d2h(h, &au, d.arena_used + b, 4)) != SWIM_OK || (rc = msgs_read(h, b, v)) != SWIM_OK) return rc;
    msg_out[0] = au;
    msg_out[1] = (uint32_t)v.size();
    std::fill(msg_out + 2, msg_out + 2 + d.N, 0u);
    for (const SyncMsg& q : v)
      if (q.src < d.N && q.payload != NEVER && !(q.payload & PAY_RX)) msg_out[2 + q.src]++;
    // what the tick left of the receipt lists: every member's count and fill (zero once P4 or the triage took them)
    if ((rc = d2h(h, msg_out + 2 + d.N, d.rc_cnt, 4ull * d.N)) != SWIM_OK ||
        (rc = d2h(h, msg_out + 2 + 2ull * d.N, d.rc_fill, 4ull * d.N)) != SWIM_OK)
      return rc;
  }
  if (!h->dbg_slots.empty()) {  // the injected slots back on top of the free stack (nothing else holds them)
    int32_t top = 0;
    if ((rc = d2h(h, &top, d.free_top, 4)) != SWIM_OK) return rc;
    if (top < 0 || (uint64_t)top + h->dbg_slots.size() > d.SLOTS)
      return fail(h, SWIM_EDEVICE, "swim_debug_receipts_read: free stack out of range");
    HIPCK(h2d(h->stream, d.free_list + top, h->dbg_slots.data(), 4ull * h->dbg_slots.size()));
    top += (int32_t)h->dbg_slots.size();
    HIPCK(h2d(h->stream, d.free_top, &top, 4));
    h->dbg_slots.clear();
    // the published count of slots in use follows the stack, as after a speculative batch's halt (step.hip)
    const uint32_t used = (uint32_t)((int32_t)d.SPR - top);
    h->hflag[HF_USED] = used;
    HIPCK(h2d(h->stream, &d.hsh[HSH_USED], &used, 4));
    h->gossip_idle = false;  // the next tick takes the one-tick path, which looks at the flag again
  }
  return SWIM_OK;
}

}  // extern "C"
