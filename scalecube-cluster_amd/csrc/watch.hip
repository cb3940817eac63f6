// watch.hip — the subject watch (include/swimhip_watch.h): the census's reduction turned ninety degrees.
// A watch names K <= 256 subjects; a sample reads those K columns of the key plane over the counted observers.
//
// A lane is an observer: a workgroup (WATCH_ROWS threads) owns the observers [lo + WATCH_ROWS b, lo + WATCH_ROWS (b + 1))
// of this shard, and every lane walks the watched subjects in ascending subject order (neighbouring subjects share the
// lane's cache line), loading its row's key byte from the 8-bit shadow plane (0xFF is the escape: the record is taken
// from the u32 key) or its u32 key where the handle keeps no shadow. Rows that are not counted are never loaded. Per
// subject a wave takes one ballot per status (ABSENT, SUSPECT, DEAD; ALIVE is what remains of the rows counted) and the
// range of its held keys (one compare when the wave agrees, a butterfly otherwise), and lane 0 adds them to the block's
// LDS tallies; the block flushes once, with integer atomics, only what is not zero: the result does not depend on the
// order of arrival. The smallest key is kept as the largest complement, so one memset of zeros prepares a sample.
// Stamps are [3][K][N] words: the lanes of a wave touch consecutive words, read only where the predicate holds and
// written only on the NEVER -> tick change, so a steady cluster stores nothing. Nothing of the engine's state is written.
//
// A recorded sample (swimhip_watch_series.h) is the same launch queued by step.hip behind a tick (watch_record_tick):
// its tallies go to that tick's entry of the series instead of the watch's own block, `now` is the tick it describes,
// and inside a speculative batch it reads the halt words first and returns at once when that state does not exist yet
// (spec.h halted_sample). A sample that ran leaves tick + 1 in its entry's first spare word.
#include <algorithm>
#include <cstring>

#include "../../include/swimhip_watch_series.h"
#include "dev_util.h"
#include "group.h"

using namespace swim;

namespace swim {
namespace {

constexpr uint32_t WATCH_ROWS = SWIM_WATCH_BLOCK_ROWS, WATCH_K = SWIM_WATCH_MAX_SUBJECTS;
constexpr uint32_t WATCH_NEVER = SWIM_WATCH_NEVER;
// the tallies, on the device and in LDS: [K] ABSENT, [K] SUSPECT, [K] DEAD, [K] ~key_min, [K] key_max, then the rows
// counted, then (a series entry) tick + 1 of the sample that filled it, and two words of padding
constexpr uint32_t T_AB = 0, T_SU = 1, T_DE = 2, T_MN = 3, T_MX = 4, T_PLANES = 5;
constexpr uint32_t T_NOBS = 0, T_MARK = 1, T_TAIL = 4;  // the words after the planes

struct WatchIn {
  const uint32_t* rowk;
  const uint8_t* rowk8;
  const uint32_t* dead_tick;
  const uint8_t* sel;    // [N] or null: the running members
  const uint32_t* subj;  // [K] ascending
  const uint32_t* slot;  // [K] the caller's index of subj[j]
  const uint32_t* inc;   // [K] by the same j, or null
  uint32_t* tally;       // [T_PLANES K + 4], zero
  uint32_t* stamps;      // [3 or 2][K][N] or null
  uint32_t N, NS, NS8, NL, lo, now, K;
  // a recorded sample: rec != 0 (tally is the series entry of tick now); queued inside a speculative batch: halt is
  // Dev::halt (lf: of a lister-free batch), else null
  const uint32_t* halt;
  uint32_t rec, lf;
};

__device__ __forceinline__ uint32_t wave_max(uint32_t v) { return ~wave_min(~v); }
__device__ __forceinline__ void stamp(uint32_t* p, uint32_t now) {
  if (*p == WATCH_NEVER) *p = now;
}

template <bool K8>
__global__ __launch_bounds__(WATCH_ROWS) void k_watch(const WatchIn in) {
  __shared__ uint32_t acc[T_PLANES * WATCH_K], nobs;
  // (kernel arguments and halt words: the whole grid decides alike, before the first barrier)
  if (in.halt && halted_sample(in.halt, in.now, in.lf != 0u)) return;
  const uint32_t t = threadIdx.x, lane = t & 63u, K = in.K, N = in.N;
  for (uint32_t i = t; i < T_PLANES * K; i += WATCH_ROWS) acc[i] = 0;
  if (t == 0) nobs = 0;
  __syncthreads();
  const uint32_t row = blockIdx.x * WATCH_ROWS + t, m = in.lo + row;
  bool on = false;
  if (row < in.NL) on = in.sel ? in.sel[m] != 0 : in.dead_tick[m] > in.now;
  const unsigned long long live = __ballot(on);
  if (live) {  // (wave-uniform: every lane of the wave takes part in the ballots below)
    if (lane == 0) atomicAdd(&nobs, (uint32_t)__popcll(live));
    const uint32_t* rk = in.rowk + (size_t)(on ? row : 0u) * in.NS;
    const uint8_t* rk8 = K8 ? in.rowk8 + (size_t)(on ? row : 0u) * in.NS8 : nullptr;
    const size_t KN = (size_t)K * N;
    constexpr uint32_t U = 8;  // subjects whose loads are in flight together
    for (uint32_t j0 = 0; j0 < K; j0 += U) {
      uint32_t k[U];
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const uint32_t s = in.subj[min(j0 + u, K - 1u)];  // (the tail repeats the last subject's load)
        k[u] = !on ? (uint32_t)ST_ALIVE : K8 ? (uint32_t)rk8[s] : rk[s];
      }
      if (K8) {
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
          if (k[u] == 0xFFu) k[u] = rk[in.subj[min(j0 + u, K - 1u)]];  // the escape; any other byte is the key
      }
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const uint32_t j = j0 + u;
        if (j >= K) break;
        const uint32_t sl = in.slot[j], key = k[u], st = key & 3u;
        const bool held = on && st != ST_ABSENT;
        const unsigned long long ab = __ballot(on && st == ST_ABSENT), su = __ballot(on && st == ST_SUSPECT),
                                 de = __ballot(on && st == ST_DEAD), hb = __ballot(held);
        uint32_t mn = 0xFFFFFFFFu, mx = 0u;
        if (hb) {
          const uint32_t k0 = __shfl(key, (int)(__ffsll((long long)hb) - 1));
          if (__ballot(held && key != k0)) {
            mn = wave_min(held ? key : 0xFFFFFFFFu);
            mx = wave_max(held ? key : 0u);
          } else {
            mn = mx = k0;
          }
        }
        if (lane == 0) {
          if (ab) atomicAdd(&acc[T_AB * K + sl], (uint32_t)__popcll(ab));
          if (su) atomicAdd(&acc[T_SU * K + sl], (uint32_t)__popcll(su));
          if (de) atomicAdd(&acc[T_DE * K + sl], (uint32_t)__popcll(de));
          if (hb) {
            atomicMax(&acc[T_MN * K + sl], ~mn);
            atomicMax(&acc[T_MX * K + sl], mx);
          }
        }
        if (in.stamps && on) {
          uint32_t* p = in.stamps + (size_t)sl * N + m;
          if (st != ST_ALIVE) stamp(p + SWIM_STAMP_NOT_ALIVE * KN, in.now);
          if (st == ST_ABSENT || st == ST_DEAD) stamp(p + SWIM_STAMP_GONE * KN, in.now);
          if (in.inc && st != ST_ABSENT && (key >> 2) >= in.inc[j]) stamp(p + SWIM_STAMP_INC_GE * KN, in.now);
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = t; i < T_PLANES * K; i += WATCH_ROWS) {
    const uint32_t v = acc[i];
    if (!v) continue;
    if (i < T_MN * K)
      atomicAdd(&in.tally[i], v);
    else
      atomicMax(&in.tally[i], v);
  }
  if (t == 0 && nobs) atomicAdd(&in.tally[T_PLANES * K + T_NOBS], nobs);
  if (in.rec && t == 0 && blockIdx.x == 0) in.tally[T_PLANES * K + T_MARK] = in.now + 1u;
}

}  // namespace
}  // namespace swim

// one watch: on one shard (dev != null), or over the shards of an n_gpus handle (parts)
struct swim_watch {
  swim_handle* h = nullptr;
  uint32_t K = 0, N = 0, flags = 0;
  bool has_inc = false, has_sel = false;
  std::vector<uint32_t> inc;  // the caller's order
  std::vector<swim_watch*> parts;
  char* dev = nullptr;  // one allocation: tallies, subject tables, mask, stamps
  size_t o_subj = 0, o_slot = 0, o_inc = 0, o_sel = 0, o_stamps = 0, tally_words = 0;
  std::vector<uint32_t> host;  // the tallies as copied back
  swim_watch* owner = nullptr;  // a part's group watch
  // the recording (swimhip_watch_series.h): entry i of the series, tally_words each, is the sample of tick
  // rec_t0 + i rec_every. rec_on: samples are still queued (on the handle's recording list); after a stop rec_n entries
  // are complete. A group watch keeps the parameters, its parts the series.
  uint32_t* series = nullptr;
  uint32_t rec_every = 0, rec_cap = 0, rec_n = 0;
  uint64_t rec_t0 = 0;
  bool rec_on = false;
};

namespace {

struct Tallies {
  uint64_t tick = 0, n_observers = 0;
  uint32_t path = 0;
  std::vector<uint32_t> counts, mn, mx;  // [4K], [K], [K]
};

size_t up64(size_t x) { return (x + 63) & ~(size_t)63; }

void unregister(swim_watch* w) {
  auto& v = w->h->watches;
  v.erase(std::remove(v.begin(), v.end(), w), v.end());
  auto& r = w->h->recording;
  r.erase(std::remove(r.begin(), r.end(), w), r.end());
}

// frees w and its parts; the parts leave their shards' lists
void watch_free(swim_watch* w) {
  for (swim_watch* p : w->parts) {
    p->owner = nullptr;
    unregister(p);
    watch_free(p);
  }
  if (w->dev) {
    hipSetDevice((int)w->h->cfg.device);
    hipFree(w->dev);
    if (w->series) hipFree(w->series);
  }
  delete w;
}

int create_one(swim_handle* h, const uint32_t* subjects, uint32_t k, const uint32_t* inc_target,
               const uint8_t* observers, uint32_t flags, swim_watch** out) {
  const Dev& d = h->d;
  const size_t N = d.N;
  auto* w = new swim_watch();
  w->h = h;
  w->K = k;
  w->N = d.N;
  w->flags = flags;
  w->has_inc = inc_target != nullptr;
  w->has_sel = observers != nullptr;
  if (inc_target) w->inc.assign(inc_target, inc_target + k);
  w->tally_words = T_PLANES * (size_t)k + T_TAIL;
  w->host.assign(w->tally_words, 0u);
  // sorted by subject, remembering the caller's index
  std::vector<uint32_t> ord(k), tab(3 * (size_t)k, 0u);
  for (uint32_t j = 0; j < k; ++j) ord[j] = j;
  std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return subjects[a] < subjects[b]; });
  for (uint32_t j = 0; j < k; ++j) {
    tab[j] = subjects[ord[j]];
    tab[k + j] = ord[j];
    tab[2 * (size_t)k + j] = inc_target ? inc_target[ord[j]] : 0u;
  }
  w->o_subj = up64(4 * w->tally_words);
  w->o_slot = w->o_subj + 4 * (size_t)k;
  w->o_inc = w->o_slot + 4 * (size_t)k;
  w->o_sel = up64(w->o_inc + 4 * (size_t)k);
  w->o_stamps = w->o_sel + (observers ? up64(N) : 0);
  const size_t planes = (flags & SWIM_WATCH_STAMPS) ? (inc_target ? 3 : 2) : 0;
  const size_t bytes = w->o_stamps + planes * 4 * (size_t)k * N;
  hipSetDevice((int)h->cfg.device);
  if (hipMalloc(&w->dev, bytes) != hipSuccess) {
    w->dev = nullptr;
    delete w;
    return fail(h, SWIM_ENOMEM, "swim_watch_create: hipMalloc of " + std::to_string(bytes) + " B failed");
  }
  hipError_t e = hipMemsetAsync(w->dev, 0, w->o_stamps, h->stream);
  if (e == hipSuccess && planes) e = hipMemsetAsync(w->dev + w->o_stamps, 0xFF, bytes - w->o_stamps, h->stream);
  if (e == hipSuccess) e = h2d(h->stream, w->dev + w->o_subj, tab.data(), 4 * tab.size());
  if (e == hipSuccess && observers) e = h2d(h->stream, w->dev + w->o_sel, observers, N);
  if (e != hipSuccess) {
    h->err = std::string("swim_watch_create -> ") + hipGetErrorString(e);
    hipFree(w->dev);
    delete w;
    return SWIM_EDEVICE;
  }
  h->watches.push_back(w);
  *out = w;
  return SWIM_OK;
}

// k_watch of tick `now` into `tally` (zero), queued on the handle's stream; halt: see WatchIn
int launch_watch(swim_watch* w, uint32_t* tally, uint32_t now, bool rec, const uint32_t* halt, bool lf) {
  swim_handle* h = w->h;
  const Dev& d = h->d;
  WatchIn in{};
  in.rowk = d.rowk;
  in.rowk8 = d.rowk8;
  in.dead_tick = d.dead_tick;
  in.sel = w->has_sel ? (const uint8_t*)(w->dev + w->o_sel) : nullptr;
  in.subj = (const uint32_t*)(w->dev + w->o_subj);
  in.slot = (const uint32_t*)(w->dev + w->o_slot);
  in.inc = w->has_inc ? (const uint32_t*)(w->dev + w->o_inc) : nullptr;
  in.tally = tally;
  in.stamps = (w->flags & SWIM_WATCH_STAMPS) ? (uint32_t*)(w->dev + w->o_stamps) : nullptr;
  in.N = d.N, in.NS = d.NS, in.NS8 = d.NS8, in.NL = d.NL, in.lo = d.lo, in.now = now, in.K = w->K;
  in.halt = halt, in.rec = rec ? 1u : 0u, in.lf = lf ? 1u : 0u;
  const uint32_t grid = cdiv(d.NL, WATCH_ROWS);
  if (d.rowk8)
    k_watch<true><<<grid, WATCH_ROWS, 0, h->stream>>>(in);
  else
    k_watch<false><<<grid, WATCH_ROWS, 0, h->stream>>>(in);
  HIPCK(hipGetLastError());
  return SWIM_OK;
}

// a tally block as copied back -> what a sample reports
void decode(const swim_watch* w, const uint32_t* t, uint64_t tick, Tallies* o) {
  const uint32_t K = w->K, rows = t[T_PLANES * K + T_NOBS];
  o->tick = tick;
  o->n_observers = rows;
  o->path = w->h->d.rowk8 ? SWIM_CENSUS_PATH_KEY8 : SWIM_CENSUS_PATH_KEY32;
  o->counts.resize(4 * (size_t)K);
  o->mn.resize(K);
  o->mx.resize(K);
  for (uint32_t j = 0; j < K; ++j) {
    const uint32_t ab = t[T_AB * K + j], su = t[T_SU * K + j], de = t[T_DE * K + j];
    uint32_t* c = &o->counts[4 * (size_t)j];
    c[ST_ABSENT] = ab, c[ST_SUSPECT] = su, c[ST_DEAD] = de;
    c[ST_ALIVE] = rows - ab - su - de;  // ALIVE is what remains of the rows counted
    o->mn[j] = ~t[T_MN * K + j];
    o->mx[j] = t[T_MX * K + j];
  }
}

// one shard's sample: one memset, one kernel, one copy back
int sample_one(swim_watch* w, Tallies* o) {
  swim_handle* h = w->h;
  static_assert(SWIM_WATCH_MAX_SUBJECTS <= 256 && T_PLANES * 4 <= 24, "the copy back is at most 24 K + 16 bytes");
  static_assert(T_MARK < T_TAIL, "the mark is one of the words after the planes");
  hipSetDevice((int)h->cfg.device);
  HIPCK(hipMemsetAsync(w->dev, 0, 4 * w->tally_words, h->stream));
  int rc = launch_watch(w, (uint32_t*)w->dev, (uint32_t)h->tick, false, nullptr, false);
  if (rc != SWIM_OK) return rc;
  HIPCK(hipMemcpyAsync(w->host.data(), w->dev, 4 * w->tally_words, hipMemcpyDeviceToHost, h->stream));
  rc = check_err(h);  // (waits for the stream)
  if (rc != SWIM_OK) return rc;
  decode(w, w->host.data(), h->tick, o);
  return SWIM_OK;
}

// o (zeroed by combine_begin) widened by one shard's partial p: counts add, key ranges widen
void combine_begin(uint32_t K, Tallies* o) {
  o->counts.assign(4 * (size_t)K, 0u);
  o->mn.assign(K, 0xFFFFFFFFu);
  o->mx.assign(K, 0u);
  o->n_observers = 0;
}
void combine_add(uint32_t K, Tallies* o, const Tallies& p) {
  for (size_t i = 0; i < o->counts.size(); ++i) o->counts[i] += p.counts[i];
  for (uint32_t j = 0; j < K; ++j) o->mn[j] = std::min(o->mn[j], p.mn[j]), o->mx[j] = std::max(o->mx[j], p.mx[j]);
  o->n_observers += p.n_observers;
  o->tick = p.tick;
  o->path = p.path;
}

int sample_any(swim_watch* w, Tallies* o) {
  if (w->parts.empty()) return sample_one(w, o);
  // the shards' partial samples combined as the census's: counts add, key ranges widen
  const uint32_t K = w->K;
  combine_begin(K, o);
  Tallies p;
  for (size_t r = 0; r < w->parts.size(); ++r) {
    const int rc = sample_one(w->parts[r], &p);
    if (rc != SWIM_OK) return fail(w->h, rc, "shard " + std::to_string(r) + ": " + w->parts[r]->h->err);
    combine_add(K, o, p);
  }
  return SWIM_OK;
}

void fill(struct swim_watch_sample* out, const Tallies& t) {
  out->tick = t.tick;
  out->n_observers = t.n_observers;
  out->path = t.path;
  std::fill(out->reserved, out->reserved + 3, 0u);
  if (out->counts) std::copy(t.counts.begin(), t.counts.end(), out->counts);
  if (out->key_min) std::copy(t.mn.begin(), t.mn.end(), out->key_min);
  if (out->key_max) std::copy(t.mx.begin(), t.mx.end(), out->key_max);
}

// ---- the recording ----

// entries complete so far: the samples of the ticks <= the handle's tick (a stopped recording: as many as it had)
uint32_t recorded(const swim_watch* w) {
  if (!w->rec_on) return w->rec_n;
  const swim_watch* p = w->parts.empty() ? w : w->parts[0];
  const uint64_t n = (p->h->tick - w->rec_t0) / w->rec_every + 1;
  return (uint32_t)std::min<uint64_t>(n, w->rec_cap);
}
bool armed(const swim_watch* w) { return w->rec_on && recorded(w) < w->rec_cap; }

void record_off(swim_watch* w) {
  w->rec_n = recorded(w);
  w->rec_on = false;
  for (swim_watch* p : w->parts) record_off(p);
  auto& r = w->h->recording;
  r.erase(std::remove(r.begin(), r.end(), w), r.end());
}

// one shard: the series allocated and zeroed, the sample of t0 taken and waited for
int record_one(swim_watch* w, uint32_t every, uint32_t cap) {
  swim_handle* h = w->h;
  hipSetDevice((int)h->cfg.device);
  if (w->rec_on) record_off(w);
  if (w->series) {
    HIPCK(hipStreamSynchronize(h->stream));
    HIPCK(hipFree(w->series));
    w->series = nullptr;
  }
  const size_t bytes = 4 * w->tally_words * (size_t)cap;
  if (hipMalloc(&w->series, bytes) != hipSuccess) {
    w->series = nullptr;
    return fail(h, SWIM_ENOMEM, "swim_watch_record: hipMalloc of " + std::to_string(bytes) + " B failed");
  }
  HIPCK(hipMemsetAsync(w->series, 0, bytes, h->stream));
  w->rec_every = every, w->rec_cap = cap, w->rec_n = 0, w->rec_t0 = h->tick, w->rec_on = true;
  h->recording.push_back(w);
  // the sample of t0: this watch's alone (another armed watch took its sample of this tick when the tick came to rest,
  // before whatever host call may have followed it)
  int rc = launch_watch(w, w->series, (uint32_t)h->tick, true, nullptr, false);
  if (rc == SWIM_OK) rc = check_err(h);  // (waits for the stream)
  if (rc != SWIM_OK) record_off(w);
  return rc;
}

// entries [first, first + n) of one shard's series, decoded; the stream has been waited for
int series_one(swim_watch* w, uint32_t first, uint32_t n, std::vector<Tallies>* out) {
  swim_handle* h = w->h;
  hipSetDevice((int)h->cfg.device);
  const size_t tw = w->tally_words;
  std::vector<uint32_t> buf(tw * n);
  const int rc = check_err(h);  // (waits for the stream)
  if (rc != SWIM_OK) return rc;
  if (n) HIPCK(hipMemcpy(buf.data(), w->series + tw * first, 4 * tw * n, hipMemcpyDeviceToHost));
  out->resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t tick = w->rec_t0 + (uint64_t)(first + i) * w->rec_every;
    const uint32_t* t = &buf[tw * i];
    if (t[T_PLANES * w->K + T_MARK] != (uint32_t)tick + 1u)
      return fail(h, SWIM_EDEVICE, "swim_watch_series: the sample of tick " + std::to_string(tick) + " did not run (entry " +
                                       std::to_string(first + i) + " holds mark " + std::to_string(t[T_PLANES * w->K + T_MARK]) + ")");
    decode(w, t, tick, &(*out)[i]);
  }
  return SWIM_OK;
}

int series_any(swim_watch* w, uint32_t first, uint32_t n, std::vector<Tallies>* out) {
  if (w->parts.empty()) return series_one(w, first, n, out);
  out->assign(n, Tallies());
  for (Tallies& t : *out) combine_begin(w->K, &t);
  std::vector<Tallies> part;
  for (size_t r = 0; r < w->parts.size(); ++r) {
    const int rc = series_one(w->parts[r], first, n, &part);
    if (rc != SWIM_OK) return fail(w->h, rc, "shard " + std::to_string(r) + ": " + w->parts[r]->h->err);
    for (uint32_t i = 0; i < n; ++i) combine_add(w->K, &(*out)[i], part[i]);
  }
  return SWIM_OK;
}

}  // namespace

namespace swim {
// step.hip, where tick t comes to rest: the armed recordings' samples of t (handle.h watch_tick_done)
int watch_record_tick(swim_handle* h, uint32_t t, bool in_batch, bool lf) {
  for (swim_watch* w : h->recording) {
    if (t < w->rec_t0 || (t - w->rec_t0) % w->rec_every) continue;
    const uint64_t idx = (t - w->rec_t0) / w->rec_every;
    if (idx >= w->rec_cap) continue;  // the series fills up in this call (it leaves the list at the next one's start)
    uint32_t* entry = w->series + w->tally_words * idx;
    // the series was zeroed when it was armed, and a void launch stores nothing; outside a batch the entry is zeroed
    // again all the same, so that the host's own launch can never add to an earlier one
    if (!in_batch) HIPCK(hipMemsetAsync(entry, 0, 4 * w->tally_words, h->stream));
    const int rc = launch_watch(w, entry, t, true, in_batch ? h->d.halt : nullptr, lf);
    if (rc != SWIM_OK) return rc;
  }
  return SWIM_OK;
}

// swim_step's start: a series that is full (its last entry's tick is behind the handle's) leaves the list
void watch_record_prune(swim_handle* h) {
  auto& r = h->recording;
  r.erase(std::remove_if(r.begin(), r.end(), [](swim_watch* w) { return !armed(w); }), r.end());
}

void watch_free_all(swim_handle* h) {
  h->recording.clear();
  while (!h->watches.empty()) {
    swim_watch* w = h->watches.back();
    h->watches.pop_back();
    if (w->owner) {  // a part outliving its shard cannot happen through the ABI; keep the owner consistent anyway
      auto& ps = w->owner->parts;
      ps.erase(std::remove(ps.begin(), ps.end(), w), ps.end());
      w->owner = nullptr;
    }
    watch_free(w);
  }
}
}  // namespace swim

extern "C" {

int swim_watch_create(swim_handle* h, const uint32_t* subjects, uint32_t k, const uint32_t* inc_target,
                      const uint8_t* observers, uint32_t flags, swim_watch** out) {
  if (!h || !subjects || !out || k == 0 || k > SWIM_WATCH_MAX_SUBJECTS || (flags & ~SWIM_WATCH_STAMPS))
    return SWIM_EINVAL;
  *out = nullptr;
  const uint32_t N = h->cfg.n_members;
  // every index the kernel trusts is checked here: subjects below N and distinct
  std::vector<uint32_t> s(subjects, subjects + k);
  std::sort(s.begin(), s.end());
  if (s.back() >= N || std::adjacent_find(s.begin(), s.end()) != s.end()) return SWIM_EINVAL;
  if (h->cfg.mode == SWIM_MODE_RUMOR) return fail(h, SWIM_EUNSUPPORTED, "a watch needs SWIM_MODE_FULL: RUMOR views never change");
  if (!h->grp) return create_one(h, subjects, k, inc_target, observers, flags, out);
  auto* w = new swim_watch();
  w->h = h;
  w->K = k;
  w->N = N;
  w->flags = flags;
  w->has_inc = inc_target != nullptr;
  w->has_sel = observers != nullptr;
  if (inc_target) w->inc.assign(inc_target, inc_target + k);
  const int rc = group_all(h, [&](swim_handle* sh) {
    swim_watch* p = nullptr;
    const int r = create_one(sh, subjects, k, inc_target, observers, flags, &p);
    if (r == SWIM_OK) {
      p->owner = w;
      w->parts.push_back(p);
    }
    return r;
  });
  if (rc != SWIM_OK) {
    watch_free(w);
    return rc;
  }
  h->watches.push_back(w);
  *out = w;
  return SWIM_OK;
}

int swim_watch_destroy(swim_watch* w) {
  if (!w || w->owner) return SWIM_EINVAL;  // (a shard's part belongs to its group watch)
  unregister(w);
  watch_free(w);
  return SWIM_OK;
}

int swim_watch_sample(swim_watch* w, struct swim_watch_sample* out) {
  if (!w || !out) return SWIM_EINVAL;
  Tallies t;
  const int rc = sample_any(w, &t);
  if (rc != SWIM_OK) return rc;
  fill(out, t);
  return SWIM_OK;
}

int swim_watch_stamps(swim_watch* w, uint32_t which, uint32_t* out, size_t cap) {
  if (!w || !out || which > SWIM_STAMP_INC_GE || !(w->flags & SWIM_WATCH_STAMPS)) return SWIM_EINVAL;
  const size_t words = (size_t)w->K * w->N;
  if (cap < words) return SWIM_EINVAL;
  swim_handle* h = w->h;
  if (which == SWIM_STAMP_INC_GE && !w->has_inc) {  // no target: never stamped (and no plane kept)
    std::fill(out, out + words, SWIM_WATCH_NEVER);
    return SWIM_OK;
  }
  if (w->parts.empty()) {
    hipSetDevice((int)h->cfg.device);
    HIPCK(hipStreamSynchronize(h->stream));
    HIPCK(hipMemcpy(out, w->dev + w->o_stamps + 4 * words * which, 4 * words, hipMemcpyDeviceToHost));
    return SWIM_OK;
  }
  // stamp rows are disjoint: a shard stamps only its own observers and leaves every other word NEVER
  std::vector<uint32_t> part(words);
  std::fill(out, out + words, SWIM_WATCH_NEVER);
  for (size_t r = 0; r < w->parts.size(); ++r) {
    const int rc = swim_watch_stamps(w->parts[r], which, part.data(), words);
    if (rc != SWIM_OK) return fail(h, rc, "shard " + std::to_string(r) + ": " + w->parts[r]->h->err);
    for (size_t i = 0; i < words; ++i) out[i] = std::min(out[i], part[i]);
  }
  return SWIM_OK;
}

int swim_watch_met(uint32_t cond, uint32_t k, const uint32_t* counts, const uint32_t* key_min, const uint32_t* key_max,
                   const uint32_t* inc_target) {
  if (cond > SWIM_UNTIL_INC_GE || k == 0 || k > SWIM_WATCH_MAX_SUBJECTS || !counts) return SWIM_EINVAL;
  if (cond == SWIM_UNTIL_CONVERGED && (!key_min || !key_max)) return SWIM_EINVAL;
  if (cond == SWIM_UNTIL_INC_GE && (!key_min || !inc_target)) return SWIM_EINVAL;
  for (uint32_t j = 0; j < k; ++j) {
    const uint32_t* c = counts + 4 * (size_t)j;
    bool ok = false;
    switch (cond) {
      case SWIM_UNTIL_CONVERGED: ok = c[ST_ABSENT] == 0 && key_min[j] == key_max[j]; break;
      case SWIM_UNTIL_NOT_ALIVE: ok = c[ST_ALIVE] == 0; break;
      case SWIM_UNTIL_GONE: ok = c[ST_ALIVE] == 0 && c[ST_SUSPECT] == 0; break;
      default: ok = c[ST_ABSENT] == 0 && (key_min[j] >> 2) >= inc_target[j]; break;
    }
    if (!ok) return 0;
  }
  return 1;
}

int swim_run_until(swim_handle* h, swim_watch* w, uint32_t cond, uint32_t max_ticks, uint32_t check_every,
                   uint32_t* ticks_run, uint32_t* met, struct swim_watch_sample* last) {
  if (!h || !w || !ticks_run || !met || w->h != h || check_every == 0 || cond > SWIM_UNTIL_INC_GE) return SWIM_EINVAL;
  if (cond == SWIM_UNTIL_INC_GE && !w->has_inc) return SWIM_EINVAL;
  if (!h->grp && h->d.W > 1)
    return fail(h, SWIM_EUNSUPPORTED, "swim_run_until on one shard: the verdict needs every shard's tallies");
  *ticks_run = 0;
  *met = 0;
  Tallies t;
  for (uint32_t done = 0;;) {
    int rc = sample_any(w, &t);
    if (rc != SWIM_OK) return rc;
    const bool ok = swim_watch_met(cond, w->K, t.counts.data(), t.mn.data(), t.mx.data(),
                                   w->has_inc ? w->inc.data() : nullptr) == 1;
    if (ok || done == max_ticks) {
      *ticks_run = done;
      *met = ok ? 1u : 0u;
      if (last) fill(last, t);
      return SWIM_OK;
    }
    const uint32_t n = std::min(check_every, max_ticks - done);
    rc = swim_step(h, n);
    if (rc != SWIM_OK) return rc;
    done += n;
  }
}

int swim_watch_record(swim_watch* w, uint32_t every, uint32_t cap) {
  if (!w || w->owner || every == 0 || cap == 0) return SWIM_EINVAL;
  if ((uint64_t)cap * (T_PLANES * (uint64_t)w->K + T_TAIL) > SWIM_WATCH_SERIES_MAX_WORDS || armed(w)) return SWIM_EINVAL;
  if (w->parts.empty()) return record_one(w, every, cap);
  if (w->rec_on) record_off(w);
  for (size_t r = 0; r < w->parts.size(); ++r) {
    const int rc = record_one(w->parts[r], every, cap);
    if (rc != SWIM_OK) {
      for (swim_watch* p : w->parts) record_off(p);
      return fail(w->h, rc, "shard " + std::to_string(r) + ": " + w->parts[r]->h->err);
    }
  }
  w->rec_every = every, w->rec_cap = cap, w->rec_n = 0, w->rec_t0 = w->parts[0]->rec_t0, w->rec_on = true;
  return SWIM_OK;
}

int swim_watch_record_stop(swim_watch* w) {
  if (!w || w->owner || w->rec_cap == 0) return SWIM_EINVAL;
  if (w->rec_on) record_off(w);
  return SWIM_OK;
}

int swim_watch_series(swim_watch* w, uint32_t first, uint32_t n, uint64_t* ticks, uint64_t* n_observers,
                      uint32_t* counts, uint32_t* key_min, uint32_t* key_max, uint32_t* n_recorded) {
  if (!w || w->rec_cap == 0) return SWIM_EINVAL;
  const uint32_t have = recorded(w), K = w->K;
  if (n_recorded) *n_recorded = have;
  if ((uint64_t)first + n > have) return SWIM_EINVAL;
  std::vector<Tallies> es;
  const int rc = series_any(w, first, n, &es);
  if (rc != SWIM_OK) return rc;
  for (uint32_t i = 0; i < n; ++i) {
    const Tallies& t = es[i];
    if (ticks) ticks[i] = t.tick;
    if (n_observers) n_observers[i] = t.n_observers;
    if (counts) std::copy(t.counts.begin(), t.counts.end(), counts + 4 * (size_t)K * i);
    if (key_min) std::copy(t.mn.begin(), t.mn.end(), key_min + (size_t)K * i);
    if (key_max) std::copy(t.mx.begin(), t.mx.end(), key_max + (size_t)K * i);
  }
  return SWIM_OK;
}

int swim_run_until_recorded(swim_handle* h, swim_watch* w, uint32_t cond, uint32_t max_ticks, uint32_t chunk,
                            uint64_t* met_tick, uint32_t* met, uint32_t* ticks_run) {
  if (!h || !w || !met_tick || !met || !ticks_run || w->h != h || chunk == 0 || cond > SWIM_UNTIL_INC_GE) return SWIM_EINVAL;
  if (cond == SWIM_UNTIL_INC_GE && !w->has_inc) return SWIM_EINVAL;
  if (!h->grp && h->d.W > 1)
    return fail(h, SWIM_EUNSUPPORTED, "swim_run_until_recorded on one shard: the verdict needs every shard's tallies");
  if (!armed(w)) return SWIM_EINVAL;
  *met_tick = 0;
  *met = 0;
  *ticks_run = 0;
  const uint64_t start = h->tick;
  // the first entry of a tick >= start
  uint32_t next = (uint32_t)((start - w->rec_t0 + w->rec_every - 1) / w->rec_every);
  std::vector<Tallies> es;
  for (uint32_t done = 0;;) {
    const uint32_t have = recorded(w);
    if (have > next) {
      int rc = series_any(w, next, have - next, &es);
      if (rc != SWIM_OK) return rc;
      for (const Tallies& t : es)
        if (swim_watch_met(cond, w->K, t.counts.data(), t.mn.data(), t.mx.data(), w->has_inc ? w->inc.data() : nullptr) == 1) {
          *met_tick = t.tick;
          *met = 1;
          *ticks_run = done;
          return SWIM_OK;
        }
      next = have;
    }
    if (done == max_ticks || next >= w->rec_cap) {
      *ticks_run = done;
      return SWIM_OK;
    }
    const uint32_t n = std::min(chunk, max_ticks - done);
    const int rc = swim_step(h, n);
    if (rc != SWIM_OK) return rc;
    done += n;
  }
}

}  // extern "C"
