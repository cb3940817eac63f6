// diag.hip — what swim_step prints and measures besides stepping: the SWIM_STATS dump of a gossip tick, the SWIM_EXP
// dumps after a step (tools/ parse some of these lines), the SWIM_FLAG_PROFILE event bookkeeping, and the holder-state
// readback of swim_debug_holders.
#include "handle.h"

#include "../../include/swimhip_debug.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace swim;

namespace swim {

// SWIM_STATS: the gossip plane's work of tick k (it has just been launched)
int stats_dump(swim_handle* h, uint32_t k) {
  const Dev& d = h->d;
  uint32_t v[8];
  HIPCK(hipStreamSynchronize(h->stream));
  const uint32_t* src[8] = {d.rc_n, d.ntl, d.nagroup, d.rp_n, d.slow_n, d.ncfl, d.nrx, d.nrwl};
  for (int q = 0; q < 8; ++q) HIPCK(hipMemcpy(&v[q], src[q], 4, hipMemcpyDeviceToHost));
  std::vector<uint32_t> rc(d.N), nf(d.N);
  HIPCK(hipMemcpy(rc.data(), d.rc_cnt, 4ull * d.N, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy2D(nf.data(), 4, &d.ms[0].nfetch, sizeof(MS), 4, d.N, hipMemcpyDeviceToHost));
  std::sort(rc.begin(), rc.end());
  std::sort(nf.begin(), nf.end());
  // first receipts per target with senders this tick (rtail - rt0), and senders per target
  std::vector<uint32_t> tl(v[1]), r0(d.N), r1(d.N), tc(d.N), fr, sn;
  HIPCK(hipMemcpy(tl.data(), d.tlist, 4ull * v[1], hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(r0.data(), d.rt0, 4ull * d.N, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(r1.data(), d.rtail, 4ull * d.N, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(tc.data(), d.tin_off, 4ull * d.N, hipMemcpyDeviceToHost));  // (tin_cnt is reset by then)
  uint64_t tot = 0;
  for (uint32_t t : tl) {
    fr.push_back(r1[t] - r0[t]);
    if (t + 1 < d.N) sn.push_back(tc[t + 1] - tc[t]);
    tot += r1[t] - r0[t];
  }
  std::sort(fr.begin(), fr.end());
  std::sort(sn.begin(), sn.end());
  const size_t nt = fr.size();
  fprintf(stderr, "stats tick %u: routed %u targets %u groups %u replay %u slow %u contacts %u rx %u rounds %u; "
          "receipts per member median %u p99 %u max %u; pending fetches median %u p99 %u max %u; "
          "first receipts %llu, per target median %u p90 %u p99 %u max %u; senders per target median %u max %u\n",
          k, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], rc[d.N / 2], rc[d.N * 99 / 100], rc[d.N - 1],
          nf[d.N / 2], nf[d.N * 99 / 100], nf[d.N - 1], (unsigned long long)tot, nt ? fr[nt / 2] : 0,
          nt ? fr[nt * 9 / 10] : 0, nt ? fr[nt * 99 / 100] : 0, nt ? fr[nt - 1] : 0, sn.empty() ? 0 : sn[sn.size() / 2],
          sn.empty() ? 0 : sn.back());
  return SWIM_OK;
}

// SWIM_EXP & (16 | 128): member-kernel shader cycles per phase since the last step (16: sum over members, 128: max)
int exp_dump_member_cycles(swim_handle* h) {
  const Dev& d = h->d;
  unsigned long long c[5];
  HIPCK(hipMemcpy(c, d.ctr + 8, sizeof(c), hipMemcpyDeviceToHost));
  HIPCK(hipMemset(d.ctr + 8, 0, sizeof(c)));
  fprintf(stderr, "exp: member cycles P0+P1 %llu P2+P3 %llu P4 %llu P5 %llu P6 %llu\n", c[0], c[1], c[2], c[3], c[4]);
  if (d.exp & EXP_CYCLES_MAX) {
    unsigned long long w[2];
    HIPCK(hipMemcpy(w, d.ctr + 14, sizeof(w), hipMemcpyDeviceToHost));
    HIPCK(hipMemset(d.ctr + 14, 0, sizeof(w)));
    fprintf(stderr, "exp: SYNC full walks %llu, largest candidate count %llu\n", w[0], w[1]);
  }
  return SWIM_OK;
}

// SWIM_EXP & 512: per-wave wall clock of the latest member kernel
int exp_dump_wave_clock(swim_handle* h) {
  const Dev& d = h->d;
  const size_t nw = (size_t)(d.NL + 255) / 256 * 4;
  std::vector<unsigned long long> w16(nw * 16), w(nw * 4), wall(nw * WT_WORDS);
  HIPCK(hipMemcpy(wall.data(), d.wt, wall.size() * 8, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < nw; ++i) {
    for (int j = 0; j < 16; ++j) w16[16 * i + j] = wall[WT_WORDS * i + j];
    for (int j = 0; j < 4; ++j) w[4 * i + j] = w16[16 * i + j];
  }
  const unsigned long long M = (1ull << 48) - 1;
  unsigned long long t0 = ~0ull, tend = 0;
  for (size_t i = 0; i < nw; ++i) t0 = std::min(t0, w[4 * i]), tend = std::max(tend, w[4 * i + 3]);
  std::vector<size_t> ord(nw);
  for (size_t i = 0; i < nw; ++i) ord[i] = i;
  // the waves whose bodies end last (a block's waves also wait for each other at the deferred copy-on-write)
  std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return w[4 * a + 2] > w[4 * b + 2]; });
  double sst = 0, str = 0, sbd = 0, scw = 0;
  for (size_t i = 0; i < nw; ++i) {
    sst += (double)(w[4 * i] - t0), str += (double)((w[4 * i + 1] & M) - w[4 * i]);
    sbd += (double)(w[4 * i + 2] - (w[4 * i + 1] & M)), scw += (double)(w[4 * i + 3] - w[4 * i + 2]);
  }
  fprintf(stderr, "exp512: span %.2f us; mean per wave (us): start %.2f triage %.2f body %.2f cow %.2f\n",
          (tend - t0) / 100.0, sst / nw / 100.0, str / nw / 100.0, sbd / nw / 100.0, scw / nw / 100.0);
  {  // the front: from the wave's true entry (WT_ENTRY, in front of the halt check) to its first stamp behind the halt
     // decision, and from there to the stamp after the triage (an entry stamp outside the launch is an earlier one's)
    std::vector<double> fr, tr;
    for (size_t i = 0; i < nw; ++i) {
      const unsigned long long e = wall[WT_WORDS * i + WT_ENTRY], a = w[4 * i], b = w[4 * i + 1] & M;
      if (e == 0 || e > a || a - e > 100000ull || b < a) continue;
      fr.push_back((a - e) / 100.0), tr.push_back((b - a) / 100.0);
    }
    std::sort(fr.begin(), fr.end());
    std::sort(tr.begin(), tr.end());
    if (!fr.empty())
      fprintf(stderr, "exp512: front, waves %zu: entry to first stamp us q1 %.2f med %.2f q3 %.2f max %.2f; first stamp to "
              "post-triage us q1 %.2f med %.2f q3 %.2f max %.2f\n", fr.size(), fr[fr.size() / 4], fr[fr.size() / 2],
              fr[3 * fr.size() / 4], fr.back(), tr[tr.size() / 4], tr[tr.size() / 2], tr[3 * tr.size() / 4], tr.back());
    // the body (post-triage to body end) of the class-3 waves that sent nothing in this launch: pings only
    std::vector<double> pb;
    for (size_t i = 0; i < nw; ++i) {
      const unsigned long long a = wall[WT_WORDS * i + WT_SLOT0], lo = w[4 * i + 1] & M, hi = w[4 * i + 2];
      if ((w[4 * i + 1] >> 56) == 8ull && (a < lo || a > hi) && hi >= lo) pb.push_back((hi - lo) / 100.0);
    }
    std::sort(pb.begin(), pb.end());
    if (!pb.empty())
      fprintf(stderr, "exp512: class 3 waves without a send %zu: body us q1 %.2f med %.2f q3 %.2f max %.2f\n", pb.size(),
              pb[pb.size() / 4], pb[pb.size() / 2], pb[3 * pb.size() / 4], pb.back());
  }
  {  // send_sync's stamps (WT_SLOT0, WT_SLOT1, WT_LINK) of the waves that sent in this launch (a stamp outside the
     // wave's bodies is an earlier launch's): the slot reservation's round trip and the time from its return to the
     // list-link exchange's, per class; then the reservation's round trip against the order the waves issued it in
    struct Snd {
      unsigned long long at;
      double res, lnk;
      unsigned cls;
    };
    std::vector<Snd> snd;
    for (size_t i = 0; i < nw; ++i) {
      const unsigned long long a = wall[WT_WORDS * i + WT_SLOT0], b = wall[WT_WORDS * i + WT_SLOT1],
                               c = wall[WT_WORDS * i + WT_LINK], lo = w[4 * i + 1] & M, hi = w[4 * i + 2];
      if (a < lo || b < a || b > hi) continue;
      snd.push_back({a, (b - a) / 100.0, c >= b && c <= hi ? (c - b) / 100.0 : -1.0, (unsigned)(w[4 * i + 1] >> 56)});
    }
    const auto quart = [](std::vector<double>& e, const char* what, int c) {
      std::sort(e.begin(), e.end());
      if (!e.empty())
        fprintf(stderr, "exp512: class %d sending waves %zu %s us q1 %.2f med %.2f q3 %.2f max %.2f\n", c, e.size(), what,
                e[e.size() / 4], e[e.size() / 2], e[3 * e.size() / 4], e.back());
    };
    for (int c = 0; c < 4; ++c) {
      std::vector<double> res, lnk;
      for (const Snd& s : snd)
        if (s.cls == (1u << c)) {
          res.push_back(s.res);
          if (s.lnk >= 0) lnk.push_back(s.lnk);
        }
      quart(res, "slot reservation", c);
      quart(lnk, "slot to link exchange", c);
    }
    std::sort(snd.begin(), snd.end(), [](const Snd& x, const Snd& y) { return x.at < y.at; });
    const size_t G = 8;
    for (size_t g = 0; g < G && snd.size() >= G; ++g) {  // eighths of the sending waves in issue order
      const size_t i0 = g * snd.size() / G, i1 = (g + 1) * snd.size() / G;
      std::vector<double> e;
      for (size_t i = i0; i < i1; ++i) e.push_back(snd[i].res);
      std::sort(e.begin(), e.end());
      fprintf(stderr, "exp512: reservations %zu-%zu by issue order, issued %.2f-%.2f us: round trip med %.2f max %.2f\n", i0,
              i1 - 1, (snd[i0].at - t0) / 100.0, (snd[i1 - 1].at - t0) / 100.0, e[e.size() / 2], e.back());
    }
  }
  for (size_t r = 0; r < 8 && r < nw; ++r) {
    const size_t i = ord[r];
    if (r == 0) {  // when the waves of each class finish their bodies (us from the kernel's first wave): quartiles
      for (int c = 0; c < 4; ++c) {
        std::vector<double> e;
        for (size_t j = 0; j < nw; ++j)
          if ((w[4 * j + 1] >> 56) == (1ull << c)) e.push_back((w[4 * j + 2] - t0) / 100.0);
        std::sort(e.begin(), e.end());
        if (!e.empty())
          fprintf(stderr, "exp512: class %d waves %zu body end min %.1f q1 %.1f med %.1f q3 %.1f max %.1f\n", c, e.size(),
                  e[0], e[e.size() / 4], e[e.size() / 2], e[3 * e.size() / 4], e.back());
      }
    }
    fprintf(stderr, "exp512: wave %zu start %.2f triage %.2f body %.2f cow %.2f classes %llx busy %llu\n", i,
            (w[4 * i] - t0) / 100.0, ((w[4 * i + 1] & M) - w[4 * i]) / 100.0, (w[4 * i + 2] - (w[4 * i + 1] & M)) / 100.0,
            (w[4 * i + 3] - w[4 * i + 2]) / 100.0, w[4 * i + 1] >> 56, (w[4 * i + 1] >> 48) & 255);
    if (w[4 * i + 1] >> 56) {  // its lead lane's laps in time order, "slot:us since the previous lap"
      // (slots 0-4: after P0+P1, P2+P3, P4, P5, P6; 5-11: finer laps inside them)
      unsigned long long prev = w[4 * i + 1] & M;
      std::vector<std::pair<unsigned long long, int>> laps;
      for (int j = 0; j < 12; ++j)
        if (w16[16 * i + 4 + j] >= prev && w16[16 * i + 4 + j] <= w[4 * i + 2]) laps.push_back({w16[16 * i + 4 + j], j});
      std::sort(laps.begin(), laps.end());
      fprintf(stderr, "exp512:   laps");
      for (const auto& l : laps)
        fprintf(stderr, " %d:%.2f@%.1f", l.second, (l.first - prev) / 100.0, (l.first - t0) / 100.0), prev = l.first;
      fprintf(stderr, "\n");
    }
  }
  return SWIM_OK;
}

// SWIM_EXP & 4: gossip-send work counters since the last step
int exp_dump_gossip_work(swim_handle* h) {
  const Dev& d = h->d;
  unsigned long long c[5], u[2];
  HIPCK(hipMemcpy(c, d.ctr + 8, sizeof(c), hipMemcpyDeviceToHost));
  HIPCK(hipMemset(d.ctr + 8, 0, sizeof(c)));
  HIPCK(hipMemcpy(u, d.ctr + C_XU, sizeof(u), hipMemcpyDeviceToHost));
  HIPCK(hipMemset(d.ctr + C_XU, 0, sizeof(u)));
  fprintf(stderr, "exp: items %llu contact-bits %llu replayed %llu candidates %llu blocked %llu target-group items %llu "
          "sender words %llu\n", c[0], c[1], c[2], c[3], c[4], u[0], u[1]);
  return SWIM_OK;
}

// W == 1 with SWIM_FLAG_PROFILE: every DIFF_SAMPLE-th tick's k_sync_diff is bracketed by events (the roofline's
// sample); SWIM_DIFF_SAMPLE overrides it (measurements of the sampling's own cost)
static uint64_t diff_sample() {
  static const uint64_t v = [] {
    const char* e = getenv("SWIM_DIFF_SAMPLE");
    const unsigned long x = e ? strtoul(e, nullptr, 0) : 0ul;
    return x >= 1 && x <= 1000 ? (uint64_t)x : (uint64_t)10;
  }();
  return v;
}

// SWIM_FLAG_PROFILE: is this tick's k_sync_diff bracketed by events? On one GPU only every diff_sample()-th (an event
// pair costs GPU time of its own); the timed launches count their own messages (diff_msgs)
bool prof_timed(const swim_handle* h, uint64_t tick) {
  const uint32_t fl = h->cfg.flags;
  return (fl & (SWIM_FLAG_PROFILE | SWIM_FLAG_PROFILE_ALL)) != 0 &&
         ((fl & SWIM_FLAG_PROFILE_ALL) || h->d.W > 1 || tick % diff_sample() == 0);
}

// one event set per tick of a swim_step of n ticks
int prof_prepare(swim_handle* h, uint32_t n) {
  if (!(h->cfg.flags & (SWIM_FLAG_PROFILE | SWIM_FLAG_PROFILE_ALL))) return SWIM_OK;
  while (h->prof.size() < n) {
    TickEvents te;
    te.all = (h->cfg.flags & SWIM_FLAG_PROFILE_ALL) ? 1 : 0;
    for (auto& e : te.ev) HIPCK(hipEventCreate((hipEvent_t*)&e));
    h->prof.push_back(te);
  }
  return SWIM_OK;
}

// after the step (the stream is idle): the timed kernels' event times into prof_ms
int prof_accumulate(swim_handle* h, uint64_t first, uint32_t n) {
  if (!(h->cfg.flags & (SWIM_FLAG_PROFILE | SWIM_FLAG_PROFILE_ALL))) return SWIM_OK;
  for (uint32_t i = 0; i < n; ++i) {
    float ms = 0;
    if (!prof_timed(h, first + i)) continue;
    if (first + i > 0) {
      HIPCK(hipEventElapsedTime(&ms, (hipEvent_t)h->prof[i].ev[0], (hipEvent_t)h->prof[i].ev[1]));
      h->prof_ms[0] += ms;
      h->prof_diff_launches++;
    }
    if (!h->prof[i].all) continue;
    HIPCK(hipEventElapsedTime(&ms, (hipEvent_t)h->prof[i].ev[2], (hipEvent_t)h->prof[i].ev[3]));
    h->prof_ms[1] += ms;
    HIPCK(hipEventElapsedTime(&ms, (hipEvent_t)h->prof[i].ev[4], (hipEvent_t)h->prof[i].ev[5]));
    h->prof_ms[2] += ms;
  }
  return SWIM_OK;
}

}  // namespace swim

// test surface (swim_debug_light): the light path's counters, summed over the member kernel's counter rows, and whether
// the next launch takes the path (the device-side rule: member_light.h light_mode)
extern "C" int swim_debug_light(swim_handle* h, uint64_t* out, size_t n) {
  if (!h || !out || n > SWIM_LT_ON + 1) return SWIM_EINVAL;
  if (h->grp || h->d.W > 1 || h->d.XW > 1) return SWIM_EUNSUPPORTED;
  const Dev& d = h->d;
  HIPCK(hipStreamSynchronize(h->stream));
  std::vector<unsigned long long> sh((size_t)CSH * CSTRIDE);
  HIPCK(hipMemcpy(sh.data(), d.ctr_sh, 8 * sh.size(), hipMemcpyDeviceToHost));
  uint64_t v[SWIM_LT_ON + 1] = {};
  for (uint32_t r = 0; r < CSH; ++r)
    for (uint32_t i = 0; i < SWIM_LT_ON; ++i) v[i] += sh[(size_t)r * CSTRIDE + SH_LIGHT + i];
  v[SWIM_LT_ON] = d.light && !d.dly_on && !d.link_n ? 1u : 0u;
  for (size_t i = 0; i < n; ++i) out[i] = v[i];
  return SWIM_OK;
}

// test surface (swim_debug_light_sure): the light path's dead-lookup counter (member_light.h LS_SKIP: the word behind
// swim_debug_light's in every counter row), the first_dead word, and the minimum of dead_tick it must not exceed
static_assert(SH_LIGHT + SWIM_LT_ON == SH_LIGHT_SURE, "swim_debug_light's entries end where swim_debug_light_sure's begin");
extern "C" int swim_debug_light_sure(swim_handle* h, uint64_t* out, size_t n) {
  if (!h || !out || n > SWIM_LS_MIN_DEAD + 1) return SWIM_EINVAL;
  if (h->grp || h->d.W > 1 || h->d.XW > 1) return SWIM_EUNSUPPORTED;
  const Dev& d = h->d;
  HIPCK(hipStreamSynchronize(h->stream));
  std::vector<unsigned long long> sh((size_t)CSH * CSTRIDE);
  HIPCK(hipMemcpy(sh.data(), d.ctr_sh, 8 * sh.size(), hipMemcpyDeviceToHost));
  uint64_t v[SWIM_LS_MIN_DEAD + 1] = {};
  for (uint32_t r = 0; r < CSH; ++r)
    for (uint32_t i = 0; i < SWIM_LS_FIRST_DEAD; ++i) v[i] += sh[(size_t)r * CSTRIDE + SH_LIGHT_SURE + i];
  uint32_t fd = 0;  // (no word: nothing is known, as first_dead_at reads it)
  if (const uint32_t* w = first_dead_word(d)) HIPCK(hipMemcpy(&fd, w, 4, hipMemcpyDeviceToHost));
  v[SWIM_LS_FIRST_DEAD] = fd;
  if (n > SWIM_LS_MIN_DEAD) {
    std::vector<uint32_t> dt(d.N);
    HIPCK(hipMemcpy(dt.data(), d.dead_tick, 4ull * d.N, hipMemcpyDeviceToHost));
    v[SWIM_LS_MIN_DEAD] = *std::min_element(dt.begin(), dt.end());
  }
  for (size_t i = 0; i < n; ++i) out[i] = v[i];
  return SWIM_OK;
}

namespace swim {

// test surface (swim_debug_holders): per member of [first, first + n): its gossip count, the receipt-ring positions of
// the first held entry and of the end, the popcount of its held-bit row, and the first receipts whose GOSSIP events the
// next P4 folds (RUMOR mode without recorded events)
__global__ void __launch_bounds__(256) k_dbg_holders(const Dev* __restrict__ dp, uint32_t first, uint32_t n, uint32_t* out) {
  const Dev& d = *dp;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t m = first + i;
    const unsigned long long* hb = d.HB + (size_t)m * d.QW;
    uint32_t pop = 0;
    for (uint32_t w = 0; w < d.QW; ++w) pop += (uint32_t)__popcll(hb[w]);
    uint32_t* o = out + 5ull * i;
    o[0] = d.held[m];
    o[1] = d.rhead[m];
    o[2] = d.rtail[m];
    o[3] = pop;
    o[4] = d.evp_n ? d.evp_n[m] : 0u;
  }
}
void launch_dbg_holders(const Dev& d, uint32_t first, uint32_t n, uint32_t* out, void* stream) {
  hipLaunchKernelGGL(k_dbg_holders, dim3(std::min<uint32_t>(4096, (n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     d.self, first, n, out);
}

}  // namespace swim
