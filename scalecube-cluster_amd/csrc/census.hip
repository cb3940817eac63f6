// census.hip — the view census (include/swimhip_census.h): one read-only pass over the key plane that
// counts the records of the selected observers' rows by subject and by observer, and the key range per subject.
//
// A workgroup (256 threads) owns a tile of CENSUS_ROWS observers x CENSUS_COLS subjects and walks its selected rows top
// to bottom; a wave owns 1024 consecutive subjects of each row, a lane 16 of them as four groups of four:
//   8-bit shadow plane (K8): one 16-B load per row, the lane's subjects are consecutive;
//   u32 key plane:           four 16-B loads per row, group j at wave base + 256 j + 4 lane (each load coalesced).
// A group is reduced to a status word (one byte per subject, status in its low two bits) and counted bytewise:
// per subject into packed 8-bit lane registers over the tile's rows (CENSUS_ROWS <= 255), flushed once per tile with one
// global atomic per non-zero (subject, status); per observer by popcounts into LDS words, flushed with one atomic per
// row and status per tile. ABSENT, SUSPECT and DEAD are counted and ALIVE is what remains, so a converged cluster
// issues no per-subject atomic at all. Only integer atomics: the result does not depend on the order of arrival.
// Nothing of the engine's state is written.
#include "dev_util.h"

namespace swim {

static_assert(CENSUS_ROWS <= 255, "per-subject partial counts are bytes");
static_assert(CENSUS_COLS == 4 * 1024, "four waves of 64 lanes x 16 subjects");

namespace {

constexpr uint32_t ONES = 0x01010101u;

struct CensusIn {
  const uint32_t* rowk;
  const uint8_t* rowk8;
  const uint32_t* dead_tick;
  const uint8_t* sel;
  uint32_t N, NS, NS8, NL, lo, now;
};

// a lane's partial results over its tile: byte i of word j = subject sb[j] + i
template <bool KEYS>
struct Lane {
  uint32_t ab[4], su[4], de[4];  // rows that hold the subject ABSENT / SUSPECT / DEAD
  uint32_t mn[KEYS ? 16 : 1], mx[KEYS ? 16 : 1];
};

// one group of one row: w = four status bytes; the row's bit sets ra / rs / rd take bit 8 i + j for subject (j, i)
template <bool KEYS>
__device__ __forceinline__ void tally(Lane<KEYS>& L, int j, uint32_t w, uint32_t& ra, uint32_t& rs, uint32_t& rd) {
  const uint32_t lo = w & ONES, hi = (w >> 1) & ONES;
  const uint32_t a = (lo | hi) ^ ONES, s = hi & ~lo, dd = hi & lo;
  L.ab[j] += a;
  L.su[j] += s;
  L.de[j] += dd;
  ra |= a << j;
  rs |= s << j;
  rd |= dd << j;
}
template <bool KEYS>
__device__ __forceinline__ void key_range(Lane<KEYS>& L, int x, uint32_t k) {
  if (KEYS) {
    const bool held = (k & 3u) != ST_ABSENT;
    L.mn[x] = min(L.mn[x], held ? k : 0xFFFFFFFFu);
    L.mx[x] = max(L.mx[x], held ? k : 0u);
  }
}

template <bool K8, bool KEYS>
__global__ __launch_bounds__(256) void k_census(const CensusIn in, const CensusOut o) {
  __shared__ uint32_t rows[CENSUS_ROWS], nrow, acc[3][CENSUS_ROWS], tot[4];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint32_t r0 = blockIdx.y * CENSUS_ROWS, c0 = blockIdx.x * CENSUS_COLS, N = in.N;
  if (t < 4) tot[t] = 0;
  if (t == 0) nrow = 0;
  if (t < CENSUS_ROWS) acc[0][t] = acc[1][t] = acc[2][t] = 0;
  __syncthreads();
  // the tile's selected rows (rows not selected are never loaded); their order does not matter to integer sums
  if (t < CENSUS_ROWS && r0 + t < in.NL) {
    const uint32_t m = in.lo + r0 + t;
    if (in.sel ? in.sel[m] != 0 : in.dead_tick[m] > in.now) rows[atomicAdd(&nrow, 1u)] = t;
  }
  __syncthreads();
  const uint32_t nr = nrow;
  if (nr == 0) return;

  uint32_t sb[4], vm[4];  // first subject of each group; byte mask of its subjects below N (columns past N: padding)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sb[j] = c0 + wv * 1024u + (K8 ? lane * 16u + 4u * j : 256u * j + lane * 4u);
    const uint32_t nv = sb[j] < N ? min(N - sb[j], 4u) : 0u;
    vm[j] = nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
  }
  Lane<KEYS> L;
#pragma unroll
  for (int j = 0; j < 4; ++j) L.ab[j] = L.su[j] = L.de[j] = 0;
  if (KEYS) {
#pragma unroll
    for (int x = 0; x < 16; ++x) L.mn[x] = 0xFFFFFFFFu, L.mx[x] = 0u;
  }
  uint32_t esc = 0;

  constexpr uint32_t U = K8 ? 4 : 2;  // rows whose loads are in flight together
  if (vm[0]) {  // (vm[0] == 0: the lane's first group starts at or past N, and so do the others)
    for (uint32_t i = 0; i < nr; i += U) {
      uint4 v[U][K8 ? 1 : 4];
      uint32_t lr[U];
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        lr[u] = rows[min(i + u, nr - 1u)];  // (the tail repeats the last row's loads and skips its counts)
        const size_t row = (size_t)(r0 + lr[u]);
        if (K8) {
          v[u][0] = *(const uint4*)(in.rowk8 + row * in.NS8 + sb[0]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[u][j] = vm[j] ? ld_c4(in.rowk + row * in.NS + sb[j]) : make_uint4(0, 0, 0, 0);
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        if (i + u >= nr) break;
        uint32_t ra = 0, rs = 0, rd = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t w;
          if (K8) {
            w = j == 0 ? v[u][0].x : j == 1 ? v[u][0].y : j == 2 ? v[u][0].z : v[u][0].w;
            w = (w & vm[j]) | (ONES & ~vm[j]);  // padding reads as ALIVE and is taken off below
            uint32_t skip = 0;
            if ((~w - ONES) & w & 0x80808080u) {  // some byte is the escape 0xFF: its low bits mean nothing
              const uint32_t* kr = in.rowk + (size_t)(r0 + lr[u]) * in.NS + sb[j];
#pragma unroll
              for (int b = 0; b < 4; ++b)
                if (((w >> (8 * b)) & 0xFFu) == 0xFFu) {
                  const uint32_t k = kr[b];
                  ++esc;
                  key_range(L, 4 * j + b, k);
                  skip |= 1u << b;
                  w = (w & ~(0xFFu << (8 * b))) | ((k & 3u) << (8 * b));
                }
            }
            if (KEYS) {
#pragma unroll
              for (int b = 0; b < 4; ++b)
                if (!((skip >> b) & 1u)) key_range(L, 4 * j + b, (w >> (8 * b)) & 0xFFu);  // key8 below 0xFF is the key
            }
          } else {
            const uint4 k = v[u][j];
            w = (k.x & 3u) | ((k.y & 3u) << 8) | ((k.z & 3u) << 16) | ((k.w & 3u) << 24);
            w = (w & vm[j]) | (ONES & ~vm[j]);
            key_range(L, 4 * j + 0, k.x);
            key_range(L, 4 * j + 1, k.y);
            key_range(L, 4 * j + 2, k.z);
            key_range(L, 4 * j + 3, k.w);
          }
          tally(L, j, w, ra, rs, rd);
        }
        if (ra) atomicAdd(&acc[0][lr[u]], (uint32_t)__popc(ra));
        if (rs) atomicAdd(&acc[1][lr[u]], (uint32_t)__popc(rs));
        if (rd) atomicAdd(&acc[2][lr[u]], (uint32_t)__popc(rd));
      }
    }
    // per subject: once per tile, only what is not zero
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint32_t s = sb[j] + b;
        if (s >= N) continue;
        if (o.by_subject) {
          const uint32_t a = (L.ab[j] >> (8 * b)) & 0xFFu, su = (L.su[j] >> (8 * b)) & 0xFFu,
                         de = (L.de[j] >> (8 * b)) & 0xFFu;
          if (a) atomicAdd(&o.by_subject[4ull * s + ST_ABSENT], a);
          if (su) atomicAdd(&o.by_subject[4ull * s + ST_SUSPECT], su);
          if (de) atomicAdd(&o.by_subject[4ull * s + ST_DEAD], de);
        }
        if (KEYS) {
          // the range only widens: a (possibly older) value already as wide as the tile's spares the atomic
          const uint32_t mn = L.mn[4 * j + b], mx = L.mx[4 * j + b];
          if (mn < __hip_atomic_load(&o.key_min[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&o.key_min[s], mn);
          if (mx > __hip_atomic_load(&o.key_max[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&o.key_max[s], mx);
        }
      }
    }
    if (esc) atomicAdd(&tot[3], esc);
  }
  __syncthreads();
  // per observer: one atomic per row and status of this tile; ALIVE = the tile's subjects less the other three
  if (t < nr) {
    const uint32_t r = rows[t], m = in.lo + r0 + r, a = acc[0][r], s = acc[1][r], dd = acc[2][r];
    if (o.by_observer) {
      uint32_t* bo = o.by_observer + 4ull * m;
      if (a) atomicAdd(&bo[ST_ABSENT], a);
      if (s) atomicAdd(&bo[ST_SUSPECT], s);
      if (dd) atomicAdd(&bo[ST_DEAD], dd);
      atomicAdd(&bo[ST_ALIVE], min(N - c0, CENSUS_COLS) - a - s - dd);
    }
    if (a) atomicAdd(&tot[0], a);
    if (s) atomicAdd(&tot[1], s);
    if (dd) atomicAdd(&tot[2], dd);
  }
  __syncthreads();
  if (t == 0) {
    if (blockIdx.x == 0) atomicAdd(&o.tot[CT_ROWS], (unsigned long long)nr);
    if (tot[0]) atomicAdd(&o.tot[CT_ST + ST_ABSENT], (unsigned long long)tot[0]);
    if (tot[1]) atomicAdd(&o.tot[CT_ST + ST_SUSPECT], (unsigned long long)tot[1]);
    if (tot[2]) atomicAdd(&o.tot[CT_ST + ST_DEAD], (unsigned long long)tot[2]);
    if (tot[3]) atomicAdd(&o.tot[CT_ESC], (unsigned long long)tot[3]);
  }
}

}  // namespace

void launch_census(const Dev& d, const uint8_t* sel, uint32_t now, const CensusOut& o, void* stream) {
  const CensusIn in{d.rowk, d.rowk8, d.dead_tick, sel, d.N, d.NS, d.NS8, d.NL, d.lo, now};
  const dim3 grid(cdiv(d.N, CENSUS_COLS), cdiv(d.NL, CENSUS_ROWS));
  hipStream_t st = (hipStream_t)stream;
  const bool keys = o.key_min != nullptr;  // (both or neither)
  if (d.rowk8) {
    if (keys)
      k_census<true, true><<<grid, 256, 0, st>>>(in, o);
    else
      k_census<true, false><<<grid, 256, 0, st>>>(in, o);
  } else {
    if (keys)
      k_census<false, true><<<grid, 256, 0, st>>>(in, o);
    else
      k_census<false, false><<<grid, 256, 0, st>>>(in, o);
  }
}

}  // namespace swim
