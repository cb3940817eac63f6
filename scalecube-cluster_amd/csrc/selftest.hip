// selftest.hip — swim_selftest_eval (include/swimhip_selftest.h): the device primitives the simulation kernels call,
// evaluated on caller inputs in a gfx950 kernel, so the reference's known answers pin the device code itself; and
// swim_debug_prim_eval (include/swimhip_debug.h): the routing, wave and window primitives and the SYNC diff with its
// lister the same way, and the row-shard exchange codec (shard.hip) and the gossip data plane's per-tick kernels
// (gossip_*.hip) in the engine's own grids (engine only).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/swimhip.h"
#include "../../include/swimhip_debug.h"
#include "../../include/swimhip_selftest.h"
#include "dev_util.h"

namespace swim {

__global__ void k_selftest(uint32_t op, const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (op == SWIM_SELFTEST_OVERRIDES) {
    const uint32_t* a = in + 4ull * i;
    out[i] = overrides(a[0], a[1], a[2], a[3]) ? 1u : 0u;  // swim_common.h, as update_membership calls it
  } else if (op == SWIM_SELFTEST_PHILOX) {
    const uint32_t* a = in + 6ull * i;
    const u32x4 r = philox(a[0], a[1], a[2], a[3], a[4], a[5]);
    out[4ull * i] = r.x;
    out[4ull * i + 1] = r.y;
    out[4ull * i + 2] = r.z;
    out[4ull * i + 3] = r.w;
  } else if (op == SWIM_SELFTEST_LOSS_ROLL) {
    const uint32_t* a = in + 8ull * i;  // the roll lost_msg compares with the link's loss percent (dev_util.h)
    out[i] = loss_roll(a[6], a[7], a[0], a[1], a[2], a[3], a[4], a[5]);
  } else {
    const uint32_t* a = in + 4ull * i;
    Dev d;  // only the fields the ClusterMath helpers read (dev_util.h)
    d.repeatMult = a[1];
    d.suspMult = a[2];
    d.ping_t = a[3];
    const uint32_t sp = spread_of(d, a[0]);
    out[4ull * i] = bitlen(a[0]);
    out[4ull * i + 1] = sp;
    out[4ull * i + 2] = sweep_after(sp);
    out[4ull * i + 3] = suspicion_ticks(d, a[0], a[3]);
  }
}

}  // namespace swim

extern "C" int swim_selftest_eval(uint32_t op, const uint32_t* in, uint32_t* out, size_t n, uint32_t device) {
  if (op > SWIM_SELFTEST_LOSS_ROLL || (n && (!in || !out)) || n > (1u << 24)) return SWIM_EINVAL;
  if (n == 0) return SWIM_OK;
  const size_t win = op == SWIM_SELFTEST_PHILOX ? 6 : op == SWIM_SELFTEST_LOSS_ROLL ? 8 : 4;
  const size_t wout = (op == SWIM_SELFTEST_OVERRIDES || op == SWIM_SELFTEST_LOSS_ROLL) ? 1 : 4;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= (int)device || hipSetDevice((int)device) != hipSuccess)
    return SWIM_EDEVICE;
  uint32_t *din = nullptr, *dout = nullptr;
  int rc = SWIM_OK;
  if (hipMalloc(&din, 4 * win * n) != hipSuccess || hipMalloc(&dout, 4 * wout * n) != hipSuccess) {
    rc = SWIM_ENOMEM;
  } else if (hipMemcpy(din, in, 4 * win * n, hipMemcpyHostToDevice) != hipSuccess) {
    rc = SWIM_EDEVICE;
  } else {
    hipLaunchKernelGGL(swim::k_selftest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, din, dout, (uint32_t)n);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out, dout, 4 * wout * n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = SWIM_EDEVICE;
  }
  if (din) hipFree(din);
  if (dout) hipFree(dout);
  return rc;
}

// ------------------------------------------------------------------------------------------------------------
// swim_debug_prim_eval (include/swimhip_debug.h): the routing, wave and window primitives on caller data. Every kernel
// here only calls the engine's own functions (dev_util.h, engine.h, swim_common.h, route.hip, grow.hip); the host
// side checks every size and index first, so no input reaches a kernel that could index out of an allocation.
namespace swim {

__global__ void __launch_bounds__(256) k_seg_sort(uint64_t* key, uint32_t* val, uint64_t* tkey, uint32_t* tval,
                                                  const uint32_t* off, const uint32_t* cnt, const uint32_t* sg,
                                                  const uint32_t* nsg, uint32_t run, unsigned long long* fb);  // route.hip
__global__ void __launch_bounds__(256) k_pack_all(Dev d, uint32_t b, uint32_t spec);                         // shard.hip
__global__ void __launch_bounds__(256) k_pack_b(Dev d);
__global__ void __launch_bounds__(256) k_inline_out(const uint8_t* send, uint64_t cap, const unsigned long long* scnt,
                                                    uint8_t* isend, uint32_t XI);
__global__ void __launch_bounds__(256) k_inline_in(const uint8_t* irecv, uint8_t* recv, uint64_t cap,
                                                   const unsigned long long* scnt, unsigned long long* rcnt,
                                                   unsigned long long* host, uint32_t W, const uint32_t* halt, uint32_t XI);
__global__ void __launch_bounds__(256) k_unpack_a(Dev d, uint32_t k, uint32_t end, uint32_t spec);

// a, r: [3][T] words per thread, T = gridDim.x * 256
__global__ void __launch_bounds__(256) k_prim_wave(uint32_t sub, const uint32_t* a, uint32_t* r, uint32_t* ctr, uint32_t T) {
  __shared__ uint32_t sh[5];
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  const uint32_t a0 = a[t], a1 = a[T + t], a2 = a[2 * T + t];
  if (sub == SWIM_PRIM_WAVE_APPEND) {
    if (a0) r[t] = wave_append(ctr);  // in a divergent branch, as k_scatter_rc calls it
  } else if (sub == SWIM_PRIM_WAVE_RESERVE) {
    r[t] = wave_reserve(ctr, a0);
  } else if (sub == SWIM_PRIM_WAVE_BLOCK_RESERVE) {
    r[t] = block_reserve(ctr, a0, sh);
    r[T + t] = block_reserve(ctr, a1, sh);
    r[2 * T + t] = block_reserve(ctr, a2, sh);
  } else if (sub == SWIM_PRIM_WAVE_SUM32) {
    r[t] = wave_sum(a0);
  } else if (sub == SWIM_PRIM_WAVE_MIN32) {
    r[t] = wave_min(a0);
  } else {
    const unsigned long long v = wave_sum(((unsigned long long)a1 << 32) | a0);
    r[t] = (uint32_t)v;
    r[T + t] = (uint32_t)(v >> 32);
  }
}

__global__ void __launch_bounds__(256) k_prim_dirty(uint32_t wave, const uint32_t* a, uint64_t* masks, uint32_t MW, uint32_t T) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (wave) {
    dirty_mark_wave(masks + (size_t)(t >> 6) * MW, a[T + t] != 0, a[t]);
  } else {
    for (uint32_t j = 0; j < 3; ++j) {
      const uint32_t s = a[j * T + t];
      if (s != NEVER) dirty_mark(masks + (size_t)t * MW, s);
    }
  }
}

__global__ void __launch_bounds__(256) k_prim_arith(const Dev d, uint32_t sub, const uint32_t* in, uint32_t* out, uint32_t n,
                                                    uint32_t aux) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (sub == SWIM_PRIM_ARITH_DIV_GT) {
    out[i] = div_gt(d, in[i]);
  } else if (sub == SWIM_PRIM_ARITH_S16) {
    out[i] = s16_tick((uint16_t)in[2ull * i], in[2ull * i + 1]);
  } else if (sub == SWIM_PRIM_ARITH_RG) {
    const uint32_t e = rg_entry(in[3ull * i], in[3ull * i + 1]);
    const int64_t p = rg_period(e, in[3ull * i + 2]);
    out[3ull * i] = (uint32_t)p;
    out[3ull * i + 1] = (uint32_t)((uint64_t)p >> 32);
    out[3ull * i + 2] = e & RG_SLOT;
  } else if (sub == SWIM_PRIM_ARITH_KEY8) {
    out[i] = key8(in[i]);
  } else if (sub == SWIM_PRIM_ARITH_DELAY) {
    out[i] = delay_ticks(d, aux, in[i]);
  } else if (sub == SWIM_PRIM_ARITH_EPOCH) {
    out[i] = (uint32_t)epoch_at(d, in[i]);
  } else {
    SyncMsg mm;
    mm.payload = PAY_RX | aux;
    mm.pin = NEVER;
    out[i] = payload_key_at(d, mm, 0, in[i]);
  }
}

__global__ void __launch_bounds__(256) k_prim_feistel(uint32_t n, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3,
                                                      uint32_t* out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = feistel(make_perm(n, k0, k1, k2, k3), i);
}

namespace {

// the call's device buffers: zero-filled, optionally loaded from host words, all freed when the call returns
struct PrimBufs {
  std::vector<void*> all;
  int rc = SWIM_OK;
  template <typename T>
  T* get(size_t n, const void* src = nullptr, size_t n_src = 0) {
    void* p = nullptr;
    if (rc != SWIM_OK) return nullptr;
    if (hipMalloc(&p, sizeof(T) * (n ? n : 1)) != hipSuccess) {
      rc = SWIM_ENOMEM;
      return nullptr;
    }
    all.push_back(p);
    if (hipMemset(p, 0, sizeof(T) * (n ? n : 1)) != hipSuccess ||
        (src && n_src && hipMemcpy(p, src, sizeof(T) * n_src, hipMemcpyHostToDevice) != hipSuccess))
      rc = SWIM_EDEVICE;
    return (T*)p;
  }
  bool back(void* dst, const void* src, size_t bytes) {
    if (rc == SWIM_OK && bytes && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = SWIM_EDEVICE;
    return rc == SWIM_OK;
  }
  bool ran() {  // after the launches
    if (rc == SWIM_OK && (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)) rc = SWIM_EDEVICE;
    return rc == SWIM_OK;
  }
  ~PrimBufs() {
    for (void* p : all) hipFree(p);
  }
};

bool pow2(uint32_t x) { return x && !(x & (x - 1)); }
constexpr uint64_t PRIM_MAX = 1ull << 22;  // elements of the largest array an op takes

int prim_scan(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 1 || P[0] < 1 || P[0] > (1u << 20) || inb != 4ull * P[0] || outb != 4ull * (P[0] + 64)) return SWIM_EINVAL;
  const uint32_t n = P[0];
  PrimBufs b;
  uint32_t* v = b.get<uint32_t>(n, in, n);
  uint32_t* x = b.get<uint32_t>(n + 64, out, n + 64);
  uint32_t* part = b.get<uint32_t>(1024);  // Dev::scan_part
  if (b.rc == SWIM_OK) {
    launch_scan(v, x, part, n, 0);
    if (b.ran()) b.back(out, x, outb);
  }
  return b.rc;
}

int prim_seg_sort(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 5) return SWIM_EINVAL;
  const uint64_t total = P[0], nmem = P[1], nlist = P[2];
  const uint32_t run = P[3];
  if (total < 1 || total > PRIM_MAX || nmem < 1 || nmem > (1u << 20) || nlist > (1u << 20) || !pow2(run) || run < 2 ||
      run > SORT_MAX || inb != 12 * total + 8 * nmem + 4 * nlist || outb != 8 + 12 * total)
    return SWIM_EINVAL;
  const uint32_t *val = in + 2 * total, *off = val + total, *cnt = off + nmem, *sg = cnt + nmem;
  for (uint64_t i = 0; i < nmem; ++i)
    if ((uint64_t)off[i] + cnt[i] > total) return SWIM_EINVAL;
  for (uint64_t i = 0; i < nlist; ++i)
    if (sg[i] >= nmem) return SWIM_EINVAL;
  const uint32_t nl = (uint32_t)nlist;
  PrimBufs b;
  uint64_t* dk = b.get<uint64_t>(total, in, total);
  uint32_t* dv = b.get<uint32_t>(total, val, total);
  uint64_t* tk = b.get<uint64_t>(total);
  uint32_t* tv = b.get<uint32_t>(total);
  uint32_t* doff = b.get<uint32_t>(nmem, off, nmem);
  uint32_t* dcnt = b.get<uint32_t>(nmem, cnt, nmem);
  uint32_t* dsg = b.get<uint32_t>(nlist, sg, nlist);
  uint32_t* dn = b.get<uint32_t>(1, &nl, 1);
  unsigned long long* fb = b.get<unsigned long long>(FB_N);
  if (b.rc == SWIM_OK) {
    hipLaunchKernelGGL(k_seg_sort, dim3(1024), dim3(256), 0, 0, dk, dv, tk, tv, doff, dcnt, dsg, dn, run,
                       P[4] ? fb : nullptr);
    if (b.ran() && b.back(out, fb + FB_SORT_MERGE, 8) && b.back(out + 2, dk, 8 * total)) b.back(out + 2 + 2 * total, dv, 4 * total);
  }
  return b.rc;
}

int prim_routing(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 6) return SWIM_EINVAL;
  const uint64_t N = P[0], RCAP = P[1], SLOTS = P[3], nraw = P[2] < RCAP ? P[2] : RCAP;
  if (N < 1 || N > (1u << 20) || RCAP < 1 || RCAP > PRIM_MAX || SLOTS < 1 || SLOTS > PRIM_MAX || !pow2(P[4]) || P[4] < 2 ||
      P[4] > SORT_MAX || inb != 8 * nraw + 8 * SLOTS || outb != 8 * RCAP + 8 + 4 * RCAP + 12 * N + 8)
    return SWIM_EINVAL;
  const uint64_t* raw = (const uint64_t*)in;
  for (uint64_t i = 0; i < nraw; ++i)
    if ((raw[i] >> 32) >= N || (uint32_t)raw[i] >= SLOTS) return SWIM_EINVAL;
  uint32_t *o_slot = out + 2 * RCAP + 2, *o_off = o_slot + RCAP, *o_cnt = o_off + N, *o_sg = o_cnt + N, *o_nsg = o_sg + N;
  PrimBufs b;
  Dev d;  // only the fields the routing kernels read (route.hip)
  memset(&d, 0, sizeof d);
  d.N = (uint32_t)N;
  d.RCAP = (uint32_t)RCAP;
  d.sort_cap = P[4];
  d.rc_raw = b.get<uint64_t>(RCAP, raw, nraw);
  d.rc_n = b.get<uint32_t>(1, &P[2], 1);
  d.slot_gid = b.get<uint64_t>(SLOTS, raw + nraw, SLOTS);
  d.rc_cnt = b.get<uint32_t>(N);
  d.rc_fill = b.get<uint32_t>(N);
  d.rc_off = b.get<uint32_t>(N, o_off, N);
  d.scan_part = b.get<uint32_t>(1024);
  d.rc_key = b.get<uint64_t>(RCAP, out, RCAP);
  d.rc_slot = b.get<uint32_t>(RCAP, o_slot, RCAP);
  d.rc_key2 = b.get<uint64_t>(RCAP);
  d.rc_slot2 = b.get<uint32_t>(RCAP);
  d.sg_list = b.get<uint32_t>(N, o_sg, N);
  d.nsg = b.get<uint32_t>(1);
  unsigned long long* fb = b.get<unsigned long long>(FB_N);
  d.fb = P[5] ? fb : nullptr;
  if (b.rc == SWIM_OK) {
    launch_receipt_routing(d, 0);
    o_nsg[1] = 0;
    if (b.ran() && b.back(out, d.rc_key, 8 * RCAP) && b.back(out + 2 * RCAP, fb + FB_SORT_MERGE, 8) &&
        b.back(o_slot, d.rc_slot, 4 * RCAP) && b.back(o_off, d.rc_off, 4 * N) && b.back(o_cnt, d.rc_cnt, 4 * N) &&
        b.back(o_sg, d.sg_list, 4 * N))
      b.back(o_nsg, d.nsg, 4);
  }
  return b.rc;
}

int prim_wave(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 2 || P[0] > SWIM_PRIM_WAVE_SUM64 || P[1] < 1 || P[1] > 64) return SWIM_EINVAL;
  const uint32_t T = P[1] * 256;
  if (inb != 12ull * T || outb != 12ull * T + 16) return SWIM_EINVAL;
  PrimBufs b;
  uint32_t* a = b.get<uint32_t>(3 * T, in, 3 * T);
  uint32_t* r = b.get<uint32_t>(3 * T + 4, out, 3 * T + 4);
  if (b.rc == SWIM_OK) {
    hipLaunchKernelGGL(k_prim_wave, dim3(P[1]), dim3(256), 0, 0, P[0], a, r, r + 3 * T, T);
    if (b.ran()) b.back(out, r, outb);
  }
  return b.rc;
}

int prim_dirty(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 3 || P[0] > 1 || P[1] < 1 || P[1] > 64 || P[2] < 1 || P[2] > MSW) return SWIM_EINVAL;
  const uint32_t T = P[1] * 256, MW = P[2], rows = P[0] ? T / 64 : T, lim = MW * 64 * CH;
  if (inb != 12ull * T || outb != 8ull * rows * MW) return SWIM_EINVAL;
  for (uint32_t i = 0; i < (P[0] ? T : 3 * T); ++i)  // wave = 1: every lane's subject, written or not
    if (in[i] >= lim && (P[0] || in[i] != NEVER)) return SWIM_EINVAL;
  PrimBufs b;
  uint32_t* a = b.get<uint32_t>(3 * T, in, 3 * T);
  uint64_t* m = b.get<uint64_t>((size_t)rows * MW, out, (size_t)rows * MW);
  if (b.rc == SWIM_OK) {
    hipLaunchKernelGGL(k_prim_dirty, dim3(P[1]), dim3(256), 0, 0, P[0], a, m, MW, T);
    if (b.ran()) b.back(out, m, outb);
  }
  return b.rc;
}

int prim_arith(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np < 2 || P[0] > SWIM_PRIM_ARITH_PAYKEY || P[1] < 1 || P[1] > (1u << 20)) return SWIM_EINVAL;
  const uint32_t sub = P[0], n = P[1];
  static const size_t NP[] = {3, 2, 2, 2, 4, 2, 7};
  if (np != NP[sub]) return SWIM_EINVAL;
  PrimBufs b;
  Dev d;  // only the fields the helper under test reads (dev_util.h)
  memset(&d, 0, sizeof d);
  uint64_t win = n, wout = n;  // words of in that are per-case inputs (they follow the op's tables), words of out
  uint32_t aux = 0;
  const uint32_t* cases = in;
  if (sub == SWIM_PRIM_ARITH_DIV_GT) {
    if (P[2] < 1) return SWIM_EINVAL;
    d.gossip_t = P[2];
    d.gt_mul = gt_mul_of(P[2]);
    wout = (uint64_t)n + 1;
  } else if (sub == SWIM_PRIM_ARITH_S16) {
    win = 2ull * n;
  } else if (sub == SWIM_PRIM_ARITH_RG) {
    win = wout = 3ull * n;
  }
  if (sub <= SWIM_PRIM_ARITH_KEY8 && inb != 4 * win) return SWIM_EINVAL;
  if (sub == SWIM_PRIM_ARITH_DELAY) {
    const uint32_t di = P[2], len = P[3];
    if (di >= DTAB || len > 256 || inb != 4ull * (len + n)) return SWIM_EINVAL;
    std::vector<uint32_t> thr(DTAB * 256, 0), ln(DTAB, 0);
    memcpy(thr.data() + di * 256, in, 4ull * len);
    ln[di] = len;
    d.dly_thr = b.get<uint32_t>(DTAB * 256, thr.data(), DTAB * 256);
    d.dly_len = b.get<uint32_t>(DTAB, ln.data(), DTAB);
    aux = di;
    cases = in + len;
  } else if (sub == SWIM_PRIM_ARITH_EPOCH) {
    if (inb != 4ull * (MAX_EPOCHS + n)) return SWIM_EINVAL;
    memcpy(d.ep_from, in, 4 * MAX_EPOCHS);
    cases = in + MAX_EPOCHS;
  } else if (sub == SWIM_PRIM_ARITH_PAYKEY) {
    const uint32_t MW = P[2], NS = P[3], ri = P[4], RXCAP = P[5], off = P[6];
    if (MW < 1 || MW > MSW || NS < 1 || NS > MW * 64 * CH || ri >= RXCAP || RXCAP > 1024 || (off & 3u) || off > (1u << 20) ||
        inb < 8ull * MW)
      return SWIM_EINVAL;
    const uint64_t* mask = (const uint64_t*)in;
    uint64_t nship = 0;
    for (uint32_t q = 0; q < MW; ++q) nship += (uint64_t)__builtin_popcountll(mask[q]);
    if (inb != 4 * (2ull * MW + NS + nship * CH + n)) return SWIM_EINVAL;
    const uint32_t *base = in + 2 * MW, *ship = base + NS;
    cases = ship + nship * CH;
    for (uint32_t i = 0; i < n; ++i)
      if (cases[i] >= NS) return SWIM_EINVAL;
    std::vector<uint64_t> rm((size_t)RXCAP * MW, 0), ro(RXCAP, 0);
    memcpy(rm.data() + (size_t)ri * MW, mask, 8ull * MW);
    ro[ri] = off;
    d.MW = MW;
    d.rx_mask = b.get<uint64_t>(rm.size(), rm.data(), rm.size());
    d.rx_off = b.get<uint64_t>(RXCAP, ro.data(), RXCAP);
    d.base_row = b.get<uint32_t>(NS, base, NS);
    d.xa_recv = b.get<uint8_t>(off + 4 * nship * CH);
    if (b.rc == SWIM_OK && nship && hipMemcpy(d.xa_recv + off, ship, 4 * nship * CH, hipMemcpyHostToDevice) != hipSuccess)
      b.rc = SWIM_EDEVICE;
    aux = ri;
  }
  if (outb != 4 * wout) return SWIM_EINVAL;
  uint32_t* din = b.get<uint32_t>(win, cases, win);
  uint32_t* dout = b.get<uint32_t>(wout);
  if (b.rc == SWIM_OK) {
    hipLaunchKernelGGL(k_prim_arith, dim3(cdiv(n, 256)), dim3(256), 0, 0, d, sub, din, dout, n, aux);
    if (b.ran() && b.back(out, dout, 4ull * n * (sub == SWIM_PRIM_ARITH_RG ? 3 : 1)) && sub == SWIM_PRIM_ARITH_DIV_GT)
      out[n] = d.gt_mul;
  }
  return b.rc;
}

int prim_feistel(const uint32_t* P, size_t np, size_t inb, uint32_t* out, size_t outb) {
  if (np != 5 || P[0] < 1 || P[0] > (1u << 20) || inb != 0 || outb != 8ull * P[0]) return SWIM_EINVAL;
  const uint32_t n = P[0];
  PrimBufs b;
  uint32_t* o = b.get<uint32_t>(n);
  if (b.rc == SWIM_OK) {
    hipLaunchKernelGGL(k_prim_feistel, dim3(cdiv(n, 256)), dim3(256), 0, 0, n, P[1], P[2], P[3], P[4], o);
    if (b.ran() && b.back(out, o, 4ull * n)) {
      const FeistelPerm p = make_perm(n, P[1], P[2], P[3], P[4]);
      for (uint32_t i = 0; i < n; ++i) out[n + i] = feistel(p, i);
    }
  }
  return b.rc;
}

int prim_ring_move(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 3) return SWIM_EINVAL;
  const uint64_t N = P[0], B = P[1], B2 = P[2];
  if (N < 1 || N > (1u << 16) || !pow2(P[1]) || !pow2(P[2]) || B > B2 || N * B2 > PRIM_MAX || inb != 4 * (N * B + 2 * N) ||
      outb != 4 * N * B2)
    return SWIM_EINVAL;
  const uint32_t *rh = in + N * B, *rt = rh + N;
  for (uint64_t m = 0; m < N; ++m)
    if (rt[m] - rh[m] > B) return SWIM_EINVAL;  // positions are absolute and wrap
  PrimBufs b;
  uint32_t* rg = b.get<uint32_t>(N * B, in, N * B);
  uint32_t* rg2 = b.get<uint32_t>(N * B2, out, N * B2);
  uint32_t* dh = b.get<uint32_t>(N, rh, N);
  uint32_t* dt = b.get<uint32_t>(N, rt, N);
  if (b.rc == SWIM_OK) {
    launch_ring_move(rg, rg2, dh, dt, (uint32_t)N, (uint32_t)B, (uint32_t)B2, nullptr);
    if (b.ran()) b.back(out, rg2, outb);
  }
  return b.rc;
}

// k_sync_diff and k_ack_resolve on a Dev that holds only what the two kernels read (sync_diff.hip), launched through
// launch_diff / launch_diff_listed as step.hip launches them. Layout: include/swimhip_debug.h.
int prim_sync_diff(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 15) return SWIM_EINVAL;
  const uint32_t N = P[0], R = P[1], fl = P[2], nmsg = P[3], MSGCAP = P[4], AR = P[5], POOLCAP = P[6], k = P[7], grid = P[8],
                 sent = P[9], nnar = P[10], nwide = P[11], lo = P[12], nrx = P[13], ls = P[14];
  const bool k8 = fl & SWIM_PRIM_SD_K8, lister = fl & SWIM_PRIM_SD_LISTER, lists = fl & SWIM_PRIM_SD_LISTS,
             sharded = fl & SWIM_PRIM_SD_SHARDED, dirty = fl & SWIM_PRIM_SD_DIRTY;
  if (N < 1 || N > MSW * 64 * CH || R < 1 || R > 64 || fl > 31 || MSGCAP < 1 || MSGCAP > 4096 || nmsg > MSGCAP || AR > 64 ||
      POOLCAP > (1u << 22) || k < 1 || k >= (1u << 31) || grid > 4096 || ls > (LS_SPEC | LS_NODIFF) || nrx > 64 ||
      (uint64_t)lo + R > N)
    return SWIM_EINVAL;
  if ((lister && (lists || sharded)) || (!lister && (dirty || ls)) || (!lists && (nnar || nwide)) ||
      (!sharded && (lo || nrx)) || (nnar && !k8))
    return SWIM_EINVAL;
  const KeyPlaneSizes z = key_plane_sizes(N);
  const uint32_t NS = z.NS, NS8 = z.NS8, NCHUNK = z.NCHUNK, NMETA = z.NMETA, MW = z.MW;
  const uint32_t nit = (NCHUNK + NPER - 1) / NPER, b = (k - 1) & 1u;
  const uint64_t ncap = sharded ? MSGCAP : (uint64_t)MSGCAP * nit;  // narrow entries: per message, or per item
  if (nnar > ncap || nwide > MSGCAP) return SWIM_EINVAL;

  // ---- the input's parts ----
  const uint64_t w_dirty = 2ull * MSW * R, w_rx = sharded ? 2ull * MW * nrx + 2ull * nrx : 0, w_rows = (uint64_t)R * NS,
                 w_arena = (uint64_t)AR * NS, w_msgs = 6ull * nmsg, w_lists = 4ull * nnar + 4ull * nwide,
                 w_log = lister ? 4ull * R + 2ull * R * TL + R + nmsg : 0, w_base = sharded ? NS : 0;
  const uint64_t fixed = w_dirty + w_rx + w_rows + w_arena + w_msgs + w_lists + w_log + w_base;
  if ((inb & 3u) || inb / 4 < fixed || (inb / 4 - fixed) % CH || (!sharded && inb / 4 != fixed)) return SWIM_EINVAL;
  const uint64_t nship = (inb / 4 - fixed) / CH;  // shipped chunks in the receive buffer
  if (nship > 1024) return SWIM_EINVAL;
  const uint64_t w_out = 2ull * (POOLCAP + 64) + 24 + 6ull * NCHUNK + 2ull * NMETA * nmsg + 3ull * nmsg + w_arena + 4 * ncap +
                         4ull * MSGCAP + 8;
  if (outb != 4 * w_out) return SWIM_EINVAL;
  const uint64_t* i_dirty = (const uint64_t*)in;
  const uint64_t *i_rxm = i_dirty + (size_t)MSW * R, *i_rxo = i_rxm + (sharded ? (size_t)MW * nrx : 0);
  const uint32_t* i_rows = in + w_dirty + w_rx;
  const uint32_t *i_arena = i_rows + w_rows, *i_msgs = i_arena + w_arena, *i_nar = i_msgs + w_msgs, *i_wide = i_nar + 4ull * nnar;
  const uint32_t *i_tick = i_wide + 4ull * nwide, *i_tln = i_tick + 2ull * R, *i_tlog = i_tln + 2ull * R,
                 *i_head = i_tlog + 2ull * R * TL, *i_next = i_head + R;
  const uint32_t *i_base = in + (fixed - w_base), *i_ship = in + fixed;

  // ---- host checks: nothing below may let a kernel index outside an allocation ----
  for (uint32_t r = 0; r < R + AR + (sharded ? 1u : 0u); ++r) {  // padding keys are 0 (absent)
    const uint32_t* row = r < R ? i_rows + (size_t)r * NS : r < R + AR ? i_arena + (size_t)(r - R) * NS : i_base;
    for (uint32_t s = N; s < NS; ++s)
      if (row[s]) return SWIM_EINVAL;
  }
  const auto row_of = [&](uint32_t m) { return m >= lo && m - lo < R; };
  const auto pay_ok = [&](uint32_t pay) {  // a message's payload, or a list entry's place without its flag values
    if (pay & PAY_RX) return sharded && !(pay & DESC_PIN) && (pay & ~PAY_RX) < nrx;
    return pay < AR;
  };
  for (uint32_t i = 0; i < nmsg; ++i) {
    const uint32_t *m = i_msgs + 6ull * i, src = m[0], dst = m[1], pay = m[3], pin = m[4];
    const bool rx = pay != NEVER && (pay & PAY_RX);
    if (!(rx ? src < N : row_of(src)) || !row_of(dst) || (pay != NEVER && !pay_ok(pay)) || (pin != NEVER && pin >= AR))
      return SWIM_EINVAL;
  }
  for (uint32_t i = 0; i < nnar + nwide; ++i) {
    const uint32_t *e = i_nar + 4ull * i, w = e[3];
    const bool nar = i < nnar, rx = sharded && w != NEVER && w != DESC_DEFER && !(w & DESC_PIN) && (w & PAY_RX);
    if (e[0] >= nmsg || !(rx ? e[1] < N : row_of(e[1])) || !row_of(e[2])) return SWIM_EINVAL;
    if (nar && !sharded) {  // item index << 4 | the item's chunks to stream
      const uint32_t t = w >> 4, m4 = w & 15u;
      if (t >= nit || (m4 >> (NCHUNK - NPER * t < NPER ? NCHUNK - NPER * t : NPER))) return SWIM_EINVAL;
    } else if (nar) {  // a local sender's live row, or a peer's payload
      if (w != NEVER && !rx) return SWIM_EINVAL;
      if (rx && !pay_ok(w)) return SWIM_EINVAL;
    } else if (w != NEVER && w != DESC_DEFER) {
      if (w & DESC_PIN ? (w & ~DESC_PIN) >= AR : !pay_ok(w)) return SWIM_EINVAL;
    }
  }
  if (lister) {
    for (uint64_t i = 0; i < 2ull * R * TL; ++i)
      if (i_tlog[i] >= N) return SWIM_EINVAL;
    for (uint32_t i = 0; i < nmsg; ++i)
      if (i_next[i] != NEVER && i_next[i] >= nmsg) return SWIM_EINVAL;
    for (uint32_t r = 0; r < R; ++r) {  // every inbound list ends within nmsg links
      uint32_t q = i_head[r], n = 0;
      if (q != NEVER && q >= nmsg) return SWIM_EINVAL;
      for (; q != NEVER && n <= nmsg; ++n) q = i_next[q];
      if (q != NEVER) return SWIM_EINVAL;
    }
  }
  // the shipped chunks of every received payload lie in the receive buffer, 16-B aligned (diff_fetch loads 16 B)
  for (uint32_t ri = 0; ri < nrx; ++ri) {
    uint64_t cnt = 0;
    for (uint32_t q = 0; q < MW; ++q) {
      const uint64_t m = i_rxm[(size_t)ri * MW + q];
      const uint32_t top = NCHUNK - 64 * q >= 64 ? 64 : NCHUNK - 64 * q;
      if (top < 64 && (m >> top)) return SWIM_EINVAL;
      cnt += (uint64_t)__builtin_popcountll(m);
    }
    if ((i_rxo[ri] & 15u) || i_rxo[ri] > 4ull * CH * nship || i_rxo[ri] + 4ull * CH * cnt > 4ull * CH * nship) return SWIM_EINVAL;
  }

  // ---- the Dev: only the fields k_sync_diff and k_ack_resolve (and their launchers) read ----
  PrimBufs bf;
  Dev d;
  memset(&d, 0, sizeof d);
  d.N = N, d.NS = NS, d.NS8 = NS8, d.NCHUNK = NCHUNK, d.NMETA = NMETA, d.MW = MW;
  d.W = sharded ? 2u : 1u, d.lo = lo, d.hi = lo + R, d.NL = R;
  d.MSGCAP = MSGCAP, d.POOLCAP = POOLCAP, d.ARENA_ROWS = AR;
  d.ackres = lister ? (ACKRES_ON | (dirty ? ACKRES_DIRTY : 0u)) : lists ? ACKRES_ON : 0u;
  d.rowk = bf.get<uint32_t>(w_rows, i_rows, w_rows);
  if (k8) {
    std::vector<uint8_t> r8((size_t)R * NS8, 0), b8(NS8, 0);
    for (uint32_t r = 0; r < R; ++r)
      for (uint32_t s = 0; s < NS; ++s) r8[(size_t)r * NS8 + s] = key8(i_rows[(size_t)r * NS + s]);
    d.rowk8 = bf.get<uint8_t>(r8.size(), r8.data(), r8.size());
    if (sharded) {
      for (uint32_t s = 0; s < NS; ++s) b8[s] = key8(i_base[s]);
      d.base_row8 = bf.get<uint8_t>(NS8, b8.data(), NS8);
    }
  }
  const size_t nms = std::max<size_t>(R, (size_t)NPER * nit);  // indexed by member (dirty) and by chunk (cstat)
  if (!sharded) {
    std::vector<MS> ms(nms);
    memset(ms.data(), 0, sizeof(MS) * nms);
    for (uint32_t r = 0; r < R; ++r)
      for (uint32_t q = 0; q < MSW; ++q) ms[r].dirty[q] = i_dirty[(size_t)r * MSW + q];
    d.ms = bf.get<MS>(nms, ms.data(), nms);
  }
  {
    std::vector<SyncMsg> mv(nmsg ? nmsg : 1);
    memset(mv.data(), 0, sizeof(SyncMsg) * mv.size());
    for (uint32_t i = 0; i < nmsg; ++i) {
      const uint32_t* m = i_msgs + 6ull * i;
      mv[i].src = m[0], mv[i].dst = m[1], mv[i].kind = m[2], mv[i].payload = m[3], mv[i].pin = m[4], mv[i].tln = m[5];
    }
    d.msgs[b] = bf.get<SyncMsg>(MSGCAP, mv.data(), nmsg);
    uint32_t nm[2] = {0, 0};
    nm[b] = nmsg;
    d.nmsg = bf.get<uint32_t>(2, nm, 2);
  }
  d.arena[b] = bf.get<uint32_t>(w_arena, i_arena, w_arena);
  std::vector<uint32_t> fill(std::max<uint64_t>({2ull * (POOLCAP + 64), 2ull * MSGCAP * NMETA, 4 * ncap, 4ull * MSGCAP, 2ull * N}), sent);
  d.pool = bf.get<uint64_t>(POOLCAP + 64, fill.data(), POOLCAP + 64);
  d.chunk_meta = bf.get<uint32_t>(2ull * MSGCAP * NMETA, fill.data(), 2ull * MSGCAP * NMETA);
  d.dlist = bf.get<uint32_t>(4 * ncap, fill.data(), 4 * ncap);
  d.dlist_w = bf.get<uint32_t>(4ull * MSGCAP, fill.data(), 4ull * MSGCAP);
  d.ndl = bf.get<uint32_t>(1, &nnar, 1);
  d.ndlw = bf.get<uint32_t>(1, &nwide, 1);
  d.pool_used = bf.get<uint32_t>(1);
  d.err = bf.get<uint32_t>(8);
  d.ctr = bf.get<unsigned long long>(32);
  d.ctr_sh = bf.get<unsigned long long>((size_t)CSH * CSTRIDE);
  d.halt = (uint32_t*)(d.ctr_sh + SH_HALT);
  d.hflag = bf.get<uint32_t>(HF_BYTES / 4);
  if (lister) {
    d.tl_tick = bf.get<uint32_t>(2ull * R, i_tick, 2ull * R);
    d.tl_n = bf.get<uint32_t>(2ull * R, i_tln, 2ull * R);
    d.tlog = bf.get<uint32_t>(2ull * R * TL, i_tlog, 2ull * R * TL);
    std::fill(fill.begin(), fill.end(), NEVER);
    d.m_head = bf.get<uint32_t>(2ull * N, fill.data(), 2ull * N);
    d.m_next = bf.get<uint32_t>(2ull * MSGCAP, fill.data(), 2ull * MSGCAP);
    if (bf.rc == SWIM_OK && (hipMemcpy(d.m_head + (size_t)b * N, i_head, 4ull * R, hipMemcpyHostToDevice) != hipSuccess ||
                             (nmsg && hipMemcpy(d.m_next + (size_t)b * MSGCAP, i_next, 4ull * nmsg, hipMemcpyHostToDevice) != hipSuccess)))
      bf.rc = SWIM_EDEVICE;
  }
  if (sharded) {
    d.rx_mask = bf.get<uint64_t>((size_t)MW * nrx, i_rxm, (size_t)MW * nrx);
    d.rx_off = bf.get<uint64_t>(nrx, i_rxo, nrx);
    d.base_row = bf.get<uint32_t>(NS, i_base, NS);
    d.xa_recv = bf.get<uint8_t>(4ull * CH * nship, i_ship, 4ull * CH * nship);
  }
  if (bf.rc == SWIM_OK && (nnar + nwide) &&
      (hipMemcpy(d.dlist, i_nar, 16ull * nnar, hipMemcpyHostToDevice) != hipSuccess ||
       hipMemcpy(d.dlist_w, i_wide, 16ull * nwide, hipMemcpyHostToDevice) != hipSuccess))
    bf.rc = SWIM_EDEVICE;
  Dev* self = bf.get<Dev>(1);
  d.self = self;
  if (bf.rc == SWIM_OK && hipMemcpy(self, &d, sizeof d, hipMemcpyHostToDevice) != hipSuccess) bf.rc = SWIM_EDEVICE;
  if (bf.rc != SWIM_OK) return bf.rc;

  if (lister)
    launch_diff(d, k, nullptr, nullptr, ls, grid);
  else
    launch_diff_listed(d, k, nullptr, grid);
  if (!bf.ran()) return bf.rc;

  // ---- results ----
  uint32_t* o = out;
  bf.back(o, d.pool, 8ull * (POOLCAP + 64));
  o += 2ull * (POOLCAP + 64);
  {
    unsigned long long c[32], pind = 0;
    static const uint32_t order[10] = {C_DIFFMSG, C_DIFFMSG_ALL, C_DIFFWIDE, C_DIFFWIDE_ALL, C_ACKRES, C_ACKRES_ALL,
                                       C_DSTREAM, C_DSUBJ,       C_DSUBJ_ALL, C_DMSGSKIP};
    if (bf.back(c, d.ctr, sizeof c) && bf.back(&pind, d.ctr_sh + SH_PINDEC, 8)) {
      unsigned long long r[12] = {0};
      for (int i = 0; i < 10; ++i) r[i] = c[order[i]];
      r[10] = pind;
      memcpy(o, r, sizeof r);
    }
    o += 24;
  }
  {
    std::vector<MS> ms(d.ms ? nms : 0);
    if (d.ms) bf.back(ms.data(), d.ms, sizeof(MS) * nms);
    for (uint32_t c = 0; c < NCHUNK; ++c) {
      unsigned long long cs[3] = {0, 0, 0};
      if (d.ms) memcpy(cs, ms[c].cstat, sizeof cs);
      memcpy(o + 6ull * c, cs, sizeof cs);
    }
    o += 6ull * NCHUNK;
  }
  bf.back(o, d.chunk_meta, 8ull * NMETA * nmsg);
  o += 2ull * NMETA * nmsg;
  {
    std::vector<SyncMsg> mv(nmsg ? nmsg : 1);
    bf.back(mv.data(), d.msgs[b], sizeof(SyncMsg) * nmsg);
    for (uint32_t i = 0; i < nmsg; ++i) o[3ull * i] = mv[i].kind, o[3ull * i + 1] = mv[i].ncand, o[3ull * i + 2] = mv[i].pin;
    o += 3ull * nmsg;
  }
  bf.back(o, d.arena[b], 4 * w_arena);
  o += w_arena;
  bf.back(o, d.dlist, 16 * ncap);
  o += 4 * ncap;
  bf.back(o, d.dlist_w, 16ull * MSGCAP);
  o += 4ull * MSGCAP;
  bf.back(o, d.pool_used, 4);
  bf.back(o + 1, d.err, 4);
  bf.back(o + 2, d.ndl, 4);
  bf.back(o + 3, d.ndlw, 4);
  bf.back(o + 4, d.halt, 4 * (HALT_LISTED + 1));  // (the words the lister and the diff write)
  bf.back(o + 7, d.hflag + HF_STREAMED, 4);
  return bf.rc;
}

// ---- the row-shard exchange codec (shard.hip) on a Dev that holds only what its kernels read, in the engine's grids.
// Layouts: include/swimhip_debug.h. The kernels trust their inputs (a peer is the same program), so everything the
// layouts do not allow is refused here; a capacity overflow is no such thing and reaches the kernel.
constexpr uint32_t SMW = sizeof(SyncMsg) / 4;  // a whole record, as words

int prim_xpack(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 22) return SWIM_EINVAL;
  const uint32_t N = P[0], W = P[1], rank = P[2], R = P[3], b = P[4], fl = P[5], nmsg = P[6], MSGCAP = P[7], AR = P[8],
                 NSCAP = P[9], RRCAP = P[10], RQCAP = P[11], CHCAP = P[12], XA = P[13], XI = P[14], used = P[15], xn0 = P[16],
                 xn1 = P[17], nsr = P[18], nrr = P[19], xn4 = P[20], sent = P[21];
  const bool ackres = fl & SWIM_PRIM_XP_ACKRES, inl = fl & SWIM_PRIM_XP_INLINE, spec = fl & SWIM_PRIM_XP_SPEC,
             halt = fl & SWIM_PRIM_XP_HALTED, has_log = fl & SWIM_PRIM_XP_TLOG, iout = fl & SWIM_PRIM_XP_INLINE_OUT;
  if (W < 2 || W > 8 || rank >= W || N < W || N > MSW * 64 * CH || R < 1 || R > 64 || b > 1 || fl > 63 || MSGCAP < 1 ||
      MSGCAP > 4096 || nmsg > MSGCAP || AR > 64 || NSCAP < 1 || NSCAP > 1024 || RRCAP < 1 || RRCAP > 1024 || RQCAP > (1u << 20) ||
      CHCAP > (1u << 20) || (XA & 15u) || XA < 32 || XA > (1u << 26) || (XI & 7u) || XI < 64 || XI > (1u << 20) ||
      used > (1u << 20) || xn4 > (1u << 20) || nsr > NSCAP || nrr > RRCAP || std::min(xn0, NSCAP) > nsr ||
      std::min(xn1, RRCAP) > nrr || (halt && !spec) || (iout && (uint64_t)XA + 8 < XI))
    return SWIM_EINVAL;
  const uint32_t lo = shard_lo(N, W, rank), hi = shard_lo(N, W, rank + 1);
  if ((uint64_t)lo + R > hi) return SWIM_EINVAL;
  const KeyPlaneSizes z = key_plane_sizes(N);
  const uint32_t NS = z.NS, NCHUNK = z.NCHUNK, MW = z.MW;
  const uint64_t w_rd = 2ull * R * MW, w_ad = 2ull * AR * MW, w_rows = (uint64_t)R * NS, w_arena = (uint64_t)AR * NS,
                 w_msgs = (uint64_t)SMW * nmsg, w_log = has_log ? (uint64_t)R * TL : 0, w_ns = (uint64_t)NSW * nsr,
                 w_rr = (uint64_t)RRW * nrr;
  if (inb != 4 * (w_rd + w_ad + w_rows + w_arena + w_msgs + w_log + w_ns + w_rr)) return SWIM_EINVAL;
  const uint64_t b_xa = (uint64_t)W * XA, b_xi = (uint64_t)W * XI, w_mtmp = (uint64_t)SMW * MSGCAP, w_mlog = (uint64_t)TL * MSGCAP;
  if (outb != b_xa + 8ull * W + 2 * b_xi + 4 * (w_mtmp + w_mlog + 10)) return SWIM_EINVAL;
  const uint64_t *i_rd = (const uint64_t*)in, *i_ad = i_rd + (size_t)R * MW;
  const uint32_t *i_rows = in + w_rd + w_ad, *i_arena = i_rows + w_rows, *i_msgs = i_arena + w_arena, *i_log = i_msgs + w_msgs,
                 *i_ns = i_log + w_log, *i_rr = i_ns + w_ns;
  for (uint32_t r = 0; r < R + AR; ++r)  // mask bits past NCHUNK
    for (uint32_t q = 0; q < MW; ++q) {
      const uint32_t top = NCHUNK - 64 * q >= 64 ? 64 : NCHUNK - 64 * q;
      if (top < 64 && (i_rd[(size_t)r * MW + q] >> top)) return SWIM_EINVAL;
    }
  for (uint32_t i = 0; i < nmsg; ++i) {
    SyncMsg mm;
    memcpy(&mm, i_msgs + (size_t)SMW * i, sizeof mm);
    if (mm.src < lo || mm.src - lo >= R || mm.dst >= N || (mm.payload != NEVER && mm.payload >= AR)) return SWIM_EINVAL;
    if (ackres && (mm.kind & KF_RES) && mm.tln >= 1 && mm.tln <= TL && !has_log) return SWIM_EINVAL;
  }
  uint8_t* o8 = (uint8_t*)out;
  uint8_t *o_xa = o8, *o_scnt = o_xa + b_xa, *o_xi = o_scnt + 8ull * W, *o_xo = o_xi + b_xi, *o_mtmp = o_xo + b_xi,
          *o_mlog = o_mtmp + 4 * w_mtmp, *o_xn = o_mlog + 4 * w_mlog;

  PrimBufs bf;
  Dev d;  // only the fields k_pack_all reads
  memset(&d, 0, sizeof d);
  d.N = N, d.NS = NS, d.NCHUNK = NCHUNK, d.MW = MW, d.W = W, d.rank = rank, d.lo = lo, d.hi = hi, d.NL = R;
  d.MSGCAP = MSGCAP, d.ARENA_ROWS = AR, d.NSCAP = NSCAP, d.RRCAP = RRCAP, d.RQCAP = RQCAP, d.CHCAP = CHCAP, d.XA_PEER = XA;
  d.XI = XI, d.inl = inl ? 1u : 0u, d.ackres = ackres ? ACKRES_ON : 0u, d.SPR = used;
  d.rdirty = bf.get<uint64_t>((size_t)R * MW, i_rd, (size_t)R * MW);
  d.arena_dirty[b] = bf.get<uint64_t>((size_t)AR * MW, i_ad, (size_t)AR * MW);
  d.rowk = bf.get<uint32_t>(w_rows, i_rows, w_rows);
  d.arena[b] = bf.get<uint32_t>(w_arena, i_arena, w_arena);
  d.msgs[b] = (SyncMsg*)bf.get<uint32_t>((uint64_t)SMW * MSGCAP, i_msgs, w_msgs);
  uint32_t nm[2] = {0, 0};
  nm[b] = nmsg;
  d.nmsg = bf.get<uint32_t>(2, nm, 2);
  d.tlog = bf.get<uint32_t>(2ull * R * TL);
  if (bf.rc == SWIM_OK && has_log && hipMemcpy(d.tlog + (size_t)b * R * TL, i_log, 4 * w_log, hipMemcpyHostToDevice) != hipSuccess)
    bf.rc = SWIM_EDEVICE;
  d.ns_rec = bf.get<uint32_t>((uint64_t)NSW * NSCAP, i_ns, w_ns);
  d.rr_rec = bf.get<uint32_t>((uint64_t)RRW * RRCAP, i_rr, w_rr);
  d.free_top = bf.get<int32_t>(1);
  const uint32_t xn[8] = {xn0, xn1, sent, sent, xn4, sent, sent, sent};
  d.xn = bf.get<uint32_t>(8, xn, 8);
  d.xdone = bf.get<uint32_t>(2ull * W);
  d.err = bf.get<uint32_t>(8);
  d.ctr_sh = bf.get<unsigned long long>((size_t)CSH * CSTRIDE);
  d.halt = (uint32_t*)(d.ctr_sh + SH_HALT);
  const uint32_t h1 = 1;
  if (bf.rc == SWIM_OK && halt && hipMemcpy(d.halt, &h1, 4, hipMemcpyHostToDevice) != hipSuccess) bf.rc = SWIM_EDEVICE;
  d.xa_send = bf.get<uint8_t>(b_xa, o_xa, b_xa);
  d.xa_scnt = bf.get<unsigned long long>(W, o_scnt, W);
  d.xi_send = bf.get<uint8_t>(b_xi, o_xi, b_xi);
  uint8_t* xo = bf.get<uint8_t>(b_xi, o_xo, b_xi);
  d.mtmp = (SyncMsg*)bf.get<uint32_t>(w_mtmp, o_mtmp, w_mtmp);
  d.mlog = bf.get<uint32_t>(w_mlog, o_mlog, w_mlog);
  if (bf.rc != SWIM_OK) return bf.rc;

  hipLaunchKernelGGL(k_pack_all, dim3(16, W), dim3(256), 0, 0, d, b, spec ? 1u : 0u);  // launch_tick_a's grid
  if (iout) hipLaunchKernelGGL(k_inline_out, dim3(W), dim3(256), 0, 0, d.xa_send, (uint64_t)XA, d.xa_scnt, xo, XI);
  if (!bf.ran()) return bf.rc;
  bf.back(o_xa, d.xa_send, b_xa);
  bf.back(o_scnt, d.xa_scnt, 8ull * W);
  bf.back(o_xi, d.xi_send, b_xi);
  bf.back(o_xo, xo, b_xi);
  bf.back(o_mtmp, d.mtmp, 4 * w_mtmp);
  bf.back(o_mlog, d.mlog, 4 * w_mlog);
  bf.back(o_xn, d.xn, 32);
  bf.back(o_xn + 32, d.err, 4);
  bf.back(o_xn + 36, d.halt, 4);
  return bf.rc;
}

int prim_pack_b(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 5) return SWIM_EINVAL;
  const uint32_t W = P[0], rank = P[1], DCAP = P[2], xd_n = P[3], XB = P[4];
  const uint64_t nd = std::min(xd_n, DCAP);
  if (W < 2 || W > 8 || rank >= W || DCAP < 1 || DCAP > (1u << 20) || (XB & 7u) || XB < 16 || XB > (1u << 24) || inb != 8 * nd ||
      outb != (uint64_t)W * XB + 8ull * W + 8)
    return SWIM_EINVAL;
  uint8_t* o8 = (uint8_t*)out;
  PrimBufs bf;
  Dev d;  // only the fields k_pack_b reads
  memset(&d, 0, sizeof d);
  d.W = W, d.rank = rank, d.DCAP = DCAP, d.XB_PEER = XB;
  d.xd = bf.get<uint64_t>(DCAP, in, nd);
  d.xd_n = bf.get<uint32_t>(1, &xd_n, 1);
  d.err = bf.get<uint32_t>(8);
  d.xb_send = bf.get<uint8_t>((uint64_t)W * XB, o8, (uint64_t)W * XB);
  d.xb_scnt = bf.get<unsigned long long>(W, o8 + (uint64_t)W * XB, W);
  if (bf.rc != SWIM_OK) return bf.rc;
  hipLaunchKernelGGL(k_pack_b, dim3(64, W), dim3(256), 0, 0, d);  // launch_tick_b's grid
  if (bf.ran() && bf.back(o8, d.xb_send, (uint64_t)W * XB) && bf.back(o8 + (uint64_t)W * XB, d.xb_scnt, 8ull * W)) {
    uint32_t e[2] = {0, 0};
    if (bf.back(e, d.err, 4)) memcpy(o8 + (uint64_t)W * XB + 8ull * W, e, 8);
  }
  return bf.rc;
}

// a walk over a byte buffer in the order a layout lists its parts
struct Cursor {
  uint8_t* p;
  uint8_t* take(uint64_t bytes) {
    uint8_t* r = p;
    p += bytes;
    return r;
  }
};

// k_unpack_a (with msgs_commit and tick_end), optionally after k_inline_in, on caller-built receive regions
int prim_xunpack(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 18) return SWIM_EINVAL;
  const uint32_t N = P[0], W = P[1], rank = P[2], k = P[3], fl = P[4], MSGCAP = P[5], RXCAP = P[6], AR = P[7], XA = P[8],
                 XI = P[9], nloc = P[10], SLOTS = P[11], BCAP = P[12], LOGW = P[13], F = P[14], EXPB = P[15], gossip_t = P[16],
                 sent = P[17];
  const bool end = fl & SWIM_PRIM_XU_END, spec = fl & SWIM_PRIM_XU_SPEC, halt = fl & SWIM_PRIM_XU_HALTED,
             ackres = fl & SWIM_PRIM_XU_ACKRES, iin = fl & SWIM_PRIM_XU_INLINE_IN, gossip = fl & SWIM_PRIM_XU_GOSSIP;
  if (W < 2 || W > 8 || rank >= W || N < W || N > MSW * 64 * CH || k >= (1u << 31) || fl > 63 || (halt && !spec) || MSGCAP < 1 ||
      MSGCAP > 4096 || RXCAP > 4096 || AR > 64 || (XA & 15u) || XA < 32 || XA > (1u << 26) || (XI & 7u) || XI < 64 ||
      XI > (1u << 20) || (uint64_t)XA + 8 < XI || nloc > MSGCAP)
    return SWIM_EINVAL;
  if (gossip && ((SLOTS & 63u) || SLOTS < 64 || SLOTS > 4096 || !pow2(BCAP) || BCAP > 64 || LOGW < 1 || LOGW > 8 || F < 1 || F > 8 ||
                 gossip_t < 1 || EXPB > (1u << 20) || N > (1u << 16)))
    return SWIM_EINVAL;
  const KeyPlaneSizes z = key_plane_sizes(N);
  const uint32_t NCHUNK = z.NCHUNK, MW = z.MW, b = k & 1u, QW = SLOTS / 64;
  const uint64_t SE = sync_entry_size(MW), b_reg = (uint64_t)W * (iin ? XI : XA);
  const uint64_t b_in = b_reg + 16ull * W + 4ull * SMW * nloc + (gossip ? 4ull * N * (4 + LOGW) : 0);
  if (inb != b_in) return SWIM_EINVAL;
  const uint8_t* i8 = (const uint8_t*)in;
  const uint8_t *i_reg = i8, *i_rcnt = i_reg + b_reg, *i_scnt = i_rcnt + 8ull * W, *i_mtmp = i_scnt + 8ull * W,
                *i_first = i_mtmp + 4ull * SMW * nloc, *i_rhead = i_first + 4ull * N, *i_rtail = i_rhead + 4ull * N,
                *i_lpos = i_rtail + 4ull * N, *i_lspread = i_lpos + 4ull * N;
  const uint64_t b_core = 4ull * SMW * MSGCAP + 4ull * N + 4ull * MSGCAP + 8ull * RXCAP * MW + 8ull * RXCAP + 4ull * TL * MSGCAP +
                          4 * 18 + 8ull * W * 2 + 8ull * W + 8ull * W + 16ull * W;
  const uint64_t b_gos = gossip ? 32ull * SLOTS + 16ull * QW + 2ull * N * SLOTS + 8ull * N * QW + 4ull * N * BCAP + 4ull * N * 8 +
                                      4ull * N * F + 12ull * N * LOGW + 4ull * N * LOGW * F
                                : 0;
  if (outb != b_core + b_gos) return SWIM_EINVAL;

  // ---- host checks: the count words, and every region k_unpack_a will parse, against its byte count ----
  unsigned long long rcnt[8], scnt[8];
  memcpy(scnt, i_scnt, 8ull * W);
  for (uint32_t p = 0; p < W; ++p) {
    if (iin)
      memcpy(&rcnt[p], i_reg + (size_t)p * XI, 8);
    else
      memcpy(&rcnt[p], i_rcnt + 8ull * p, 8);
  }
  bool gate = false, cut = false;  // cut: an inline block that does not hold its whole region
  for (uint32_t p = 0; p < W; ++p) {
    if ((rcnt[p] | scnt[p]) & (XFLAG_GOSSIP | XFLAG_OVER) || (scnt[p] & XCNT_MASK) > XI - 8) gate = true;
    if (p != rank && iin && (rcnt[p] & XCNT_MASK) > XI - 8) cut = true;
  }
  if (cut && !(spec && gate)) return SWIM_EINVAL;  // the engine fetches the rest by a send / recv group first
  const bool parsed = !(spec && (halt || gate));
  for (uint32_t i = 0; i < nloc; ++i) {
    SyncMsg mm;
    memcpy(&mm, i_mtmp + sizeof(SyncMsg) * (size_t)i, sizeof mm);
    if (mm.dst >= N || mm.src >= N) return SWIM_EINVAL;
  }
  if (gossip)
    for (uint32_t m = 0; m < N; ++m) {
      uint32_t h, t;
      memcpy(&h, i_rhead + 4ull * m, 4);
      memcpy(&t, i_rtail + 4ull * m, 4);
      if (t - h > BCAP) return SWIM_EINVAL;
    }
  for (uint32_t p = 0; parsed && p < W; ++p) {
    const uint64_t bytes = rcnt[p] & XCNT_MASK;
    if (p == rank || bytes < 32) continue;
    if (bytes > XA || (bytes & 7u)) return SWIM_EINVAL;
    const uint8_t* Rg = i_reg + (size_t)p * (iin ? XI : XA) + (iin ? 8 : 0);
    uint32_t H[8];
    memcpy(H, Rg, 32);
    const uint64_t nslot = H[0], nround = H[1], nsync = H[2], nchunk = H[3], data_off = H[4];
    if (nslot > 1024 || nround > 1024 || nsync > 4096 || nchunk > (1u << 20) || ((nslot || nround) && !gossip)) return SWIM_EINVAL;
    const uint64_t e0 = 32 + 4ull * NSW * nslot + 4ull * RRW * nround;
    if (e0 + SE * nsync > data_off || (data_off & 15u) || data_off + nchunk * CH * 4 > bytes) return SWIM_EINVAL;
    for (uint64_t i = 0; i < nslot; ++i) {
      uint32_t r[NSW];
      memcpy(r, Rg + 32 + 4ull * NSW * i, sizeof r);
      if (r[0] >= SLOTS || r[7] >= N) return SWIM_EINVAL;
    }
    for (uint64_t i = 0; i < nround; ++i) {
      uint32_t r[RRW];
      memcpy(r, Rg + 32 + 4ull * NSW * nslot + 4ull * RRW * i, sizeof r);
      if (r[0] >= N || r[1] > F) return SWIM_EINVAL;
      for (uint32_t j = 0; j < r[1]; ++j)
        if (r[4 + j] >= N) return SWIM_EINVAL;
    }
    for (uint64_t i = 0; i < nsync; ++i) {
      const uint8_t* e = Rg + e0 + SE * i;
      SyncMsg mm;
      uint32_t base;
      memcpy(&mm, e, sizeof mm);
      memcpy(&base, e + sizeof mm, 4);
      if (mm.dst >= N || mm.src >= N) return SWIM_EINVAL;
      uint64_t cnt = 0;
      for (uint32_t q = 0; q < MW; ++q) {
        uint64_t mk;
        memcpy(&mk, e + sizeof mm + 8 + 8ull * q, 8);
        const uint32_t top = NCHUNK - 64 * q >= 64 ? 64 : NCHUNK - 64 * q;
        if (top < 64 && (mk >> top)) return SWIM_EINVAL;
        cnt += (uint64_t)__builtin_popcountll(mk);
      }
      if (base + cnt > nchunk) return SWIM_EINVAL;
    }
  }

  // ---- the Dev: only the fields k_inline_in, k_unpack_a, msgs_commit, slot_create and tick_end read ----
  Cursor o{(uint8_t*)out};
  uint8_t *o_msgs = o.take(4ull * SMW * MSGCAP), *o_head = o.take(4ull * N), *o_next = o.take(4ull * MSGCAP),
          *o_rxm = o.take(8ull * RXCAP * MW), *o_rxo = o.take(8ull * RXCAP), *o_mlog = o.take(4ull * TL * MSGCAP),
          *o_sc = o.take(4 * 18), *o_scnt = o.take(8ull * W), *o_bscnt = o.take(8ull * W), *o_xdone = o.take(8ull * W),
          *o_rcnt = o.take(8ull * W), *o_host = o.take(16ull * W);
  PrimBufs bf;
  Dev d;
  memset(&d, 0, sizeof d);
  d.N = N, d.NS = z.NS, d.NCHUNK = NCHUNK, d.MW = MW, d.W = W, d.rank = rank, d.lo = shard_lo(N, W, rank), d.hi = shard_lo(N, W, rank + 1);
  d.NL = d.hi - d.lo, d.MSGCAP = MSGCAP, d.RXCAP = RXCAP, d.ARENA_ROWS = AR, d.XA_PEER = XA, d.XI = XI;
  d.ackres = ackres ? ACKRES_ON : 0u;
  d.xa_recv = bf.get<uint8_t>((uint64_t)W * XA, iin ? nullptr : i_reg, iin ? 0 : (uint64_t)W * XA);
  uint8_t* irecv = iin ? bf.get<uint8_t>(b_reg, i_reg, b_reg) : nullptr;
  if (iin && bf.rc == SWIM_OK && hipMemset(d.xa_recv, (int)(sent & 0xFF), (uint64_t)W * XA) != hipSuccess) bf.rc = SWIM_EDEVICE;
  d.xa_rcnt = bf.get<unsigned long long>(W, iin ? o_rcnt : i_rcnt, W);
  d.xa_scnt = bf.get<unsigned long long>(W, i_scnt, W);
  d.xb_scnt = bf.get<unsigned long long>(W, o_bscnt, W);
  d.xi_host = bf.get<unsigned long long>(2ull * W, o_host, 2ull * W);
  d.xdone = bf.get<uint32_t>(2ull * W, o_xdone, 2ull * W);
  d.mtmp = (SyncMsg*)bf.get<uint32_t>((uint64_t)SMW * MSGCAP, i_mtmp, (uint64_t)SMW * nloc);
  d.msgs[b] = (SyncMsg*)bf.get<uint32_t>((uint64_t)SMW * MSGCAP, o_msgs, (uint64_t)SMW * MSGCAP);
  std::vector<uint32_t> never(std::max<uint64_t>(2ull * N, 2ull * MSGCAP), NEVER);
  d.m_head = bf.get<uint32_t>(2ull * N, never.data(), 2ull * N);  // reset by the consumer: every list is empty
  d.m_next = bf.get<uint32_t>(2ull * MSGCAP, o_next, MSGCAP);
  if (bf.rc == SWIM_OK && hipMemcpy(d.m_next + MSGCAP, o_next, 4ull * MSGCAP, hipMemcpyHostToDevice) != hipSuccess) bf.rc = SWIM_EDEVICE;
  d.rx_mask = bf.get<uint64_t>((uint64_t)RXCAP * MW, o_rxm, (uint64_t)RXCAP * MW);
  d.rx_off = bf.get<uint64_t>(RXCAP, o_rxo, RXCAP);
  d.mlog = bf.get<uint32_t>((uint64_t)TL * MSGCAP, o_mlog, (uint64_t)TL * MSGCAP);
  // the counters: the words the launch owns start where a tick leaves them, the ones it may reset at the sentinel
  uint32_t sc[18] = {sent, sent, 0, 0, sent, sent, sent, sent, nloc, 0, 0, sent, 0, 0, sent, sent, sent, sent};
  sc[2 + b] = 0, sc[2 + (b ^ 1u)] = sent;  // arena_used: this tick's pins count from 0
  d.nmsg = bf.get<uint32_t>(2, sc, 2);
  d.arena_used = bf.get<uint32_t>(2, sc + 2, 2);
  d.xn = bf.get<uint32_t>(8, sc + 4, 8);
  d.err = bf.get<uint32_t>(8);
  d.ctr_sh = bf.get<unsigned long long>((size_t)CSH * CSTRIDE);
  d.halt = (uint32_t*)(d.ctr_sh + SH_HALT);
  const uint32_t h1 = halt ? 1u : 0u;
  if (bf.rc == SWIM_OK && hipMemcpy(d.halt, &h1, 4, hipMemcpyHostToDevice) != hipSuccess) bf.rc = SWIM_EDEVICE;
  d.pool_used = bf.get<uint32_t>(1, sc + 14, 1);
  d.rc_n = bf.get<uint32_t>(1, sc + 15, 1);
  d.ndl = bf.get<uint32_t>(1, sc + 16, 1);
  d.ndlw = bf.get<uint32_t>(1, sc + 17, 1);
  uint8_t *o_gid = nullptr, *o_key = nullptr, *o_slot4 = nullptr, *o_gu = nullptr, *o_S = nullptr, *o_hb = nullptr, *o_rg = nullptr,
          *o_mem = nullptr, *o_T = nullptr, *o_log = nullptr, *o_tg = nullptr;
  uint32_t* mem8 = nullptr;  // [8][N]: rtail, held, tround, tcnt, tspread, tperiod, spchg, log_pos
  uint32_t* slot4 = nullptr;  // [4][SLOTS]: subj, ctick, exp, used
  uint32_t* log3 = nullptr;  // [3][N][LOGW]: tick, spread, cnt
  if (gossip) {
    o_gid = o.take(8ull * SLOTS), o_key = o.take(8ull * SLOTS), o_slot4 = o.take(16ull * SLOTS), o_gu = o.take(16ull * QW);
    o_S = o.take(2ull * N * SLOTS), o_hb = o.take(8ull * N * QW), o_rg = o.take(4ull * N * BCAP), o_mem = o.take(32ull * N);
    o_T = o.take(4ull * N * F), o_log = o.take(12ull * N * LOGW), o_tg = o.take(4ull * N * LOGW * F);
    d.SLOTS = SLOTS, d.QW = QW, d.BCAP = BCAP, d.LOGW = LOGW, d.F = F, d.EXPB = EXPB, d.gossip_t = gossip_t, d.gt_mul = gt_mul_of(gossip_t);
    d.slot_gid = bf.get<uint64_t>(SLOTS, o_gid, SLOTS);
    d.slot_key = bf.get<uint64_t>(SLOTS, o_key, SLOTS);
    slot4 = bf.get<uint32_t>(4ull * SLOTS, o_slot4, 4ull * SLOTS);
    d.slot_subj = slot4, d.slot_ctick = slot4 + SLOTS, d.slot_exp = slot4 + 2 * SLOTS, d.slot_used = slot4 + 3 * SLOTS;
    d.GU = bf.get<unsigned long long>(2ull * QW);  // the bit planes are set with atomicOr: they start empty
    d.DM = d.GU + QW;
    d.S = bf.get<uint16_t>((uint64_t)N * SLOTS, o_S, (uint64_t)N * SLOTS);
    d.HB = bf.get<unsigned long long>((uint64_t)N * QW);
    d.rg = bf.get<uint32_t>((uint64_t)N * BCAP, o_rg, (uint64_t)N * BCAP);
    d.firstGossip = bf.get<uint32_t>(N, i_first, N);
    d.rhead = bf.get<uint32_t>(N, i_rhead, N);
    mem8 = bf.get<uint32_t>(8ull * N, o_mem, 8ull * N);
    d.rtail = mem8, d.held = mem8 + N, d.tround = mem8 + 2ull * N, d.tcnt = mem8 + 3ull * N, d.tspread = mem8 + 4ull * N;
    d.tperiod = mem8 + 5ull * N, d.spchg = mem8 + 6ull * N, d.log_pos = mem8 + 7ull * N;
    if (bf.rc == SWIM_OK && (hipMemcpy(d.rtail, i_rtail, 4ull * N, hipMemcpyHostToDevice) != hipSuccess ||
                             hipMemset(d.held, 0, 4ull * N) != hipSuccess ||
                             hipMemcpy(d.log_pos, i_lpos, 4ull * N, hipMemcpyHostToDevice) != hipSuccess))
      bf.rc = SWIM_EDEVICE;
    d.T = bf.get<uint32_t>((uint64_t)N * F, o_T, (uint64_t)N * F);
    log3 = bf.get<uint32_t>(3ull * N * LOGW, o_log, 3ull * N * LOGW);
    d.log_tick = log3, d.log_spread = log3 + (uint64_t)N * LOGW, d.log_cnt = log3 + 2ull * N * LOGW;
    if (bf.rc == SWIM_OK && hipMemcpy(d.log_spread, i_lspread, 4ull * N * LOGW, hipMemcpyHostToDevice) != hipSuccess) bf.rc = SWIM_EDEVICE;
    d.log_tg = bf.get<uint32_t>((uint64_t)N * LOGW * F, o_tg, (uint64_t)N * LOGW * F);
  }
  if (bf.rc != SWIM_OK) return bf.rc;

  if (iin)  // launch_inline_in's grid and arguments
    hipLaunchKernelGGL(k_inline_in, dim3(W), dim3(256), 0, 0, irecv, d.xa_recv, (uint64_t)XA, d.xa_scnt, d.xa_rcnt, d.xi_host, W,
                       spec ? (const uint32_t*)d.halt : nullptr, XI);
  hipLaunchKernelGGL(k_unpack_a, dim3(32, W), dim3(256), 0, 0, d, k, end ? 1u : 0u, spec ? 1u : 0u);  // launch_tick_b's grid
  if (!bf.ran()) return bf.rc;

  bf.back(o_msgs, d.msgs[b], 4ull * SMW * MSGCAP);
  bf.back(o_head, d.m_head + (size_t)b * N, 4ull * N);
  bf.back(o_next, d.m_next + (size_t)b * MSGCAP, 4ull * MSGCAP);
  bf.back(o_rxm, d.rx_mask, 8ull * RXCAP * MW);
  bf.back(o_rxo, d.rx_off, 8ull * RXCAP);
  bf.back(o_mlog, d.mlog, 4ull * TL * MSGCAP);
  bf.back(sc, d.nmsg, 8);
  bf.back(sc + 2, d.arena_used, 8);
  bf.back(sc + 4, d.xn, 32);
  bf.back(sc + 12, d.err, 4);
  bf.back(sc + 13, d.halt, 4);
  bf.back(sc + 14, d.pool_used, 4);
  bf.back(sc + 15, d.rc_n, 4);
  bf.back(sc + 16, d.ndl, 4);
  bf.back(sc + 17, d.ndlw, 4);
  memcpy(o_sc, sc, sizeof sc);
  bf.back(o_scnt, d.xa_scnt, 8ull * W);
  bf.back(o_bscnt, d.xb_scnt, 8ull * W);
  bf.back(o_xdone, d.xdone, 8ull * W);
  bf.back(o_rcnt, d.xa_rcnt, 8ull * W);
  bf.back(o_host, d.xi_host, 16ull * W);
  if (gossip) {
    bf.back(o_gid, d.slot_gid, 8ull * SLOTS);
    bf.back(o_key, d.slot_key, 8ull * SLOTS);
    bf.back(o_slot4, slot4, 16ull * SLOTS);
    bf.back(o_gu, d.GU, 16ull * QW);
    bf.back(o_S, d.S, 2ull * N * SLOTS);
    bf.back(o_hb, d.HB, 8ull * N * QW);
    bf.back(o_rg, d.rg, 4ull * N * BCAP);
    bf.back(o_mem, mem8, 32ull * N);
    bf.back(o_T, d.T, 4ull * N * F);
    bf.back(o_log, log3, 12ull * N * LOGW);
    bf.back(o_tg, d.log_tg, 4ull * N * LOGW * F);
  }
  return bf.rc;
}

int prim_inline_in(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 4) return SWIM_EINVAL;
  const uint32_t W = P[0], XI = P[1], cap = P[2], fl = P[3];  // fl: 1 a speculative launch, 2 its halt word is raised
  if (W < 2 || W > 8 || (XI & 7u) || XI < 64 || XI > (1u << 20) || (cap & 7u) || (uint64_t)cap + 8 < XI || cap > (1u << 24) ||
      fl > 3 || fl == 2 || inb != (uint64_t)W * XI + 8ull * W || outb != (uint64_t)W * cap + 24ull * W)
    return SWIM_EINVAL;
  const uint8_t* i8 = (const uint8_t*)in;
  uint8_t* o8 = (uint8_t*)out;
  PrimBufs bf;
  uint8_t* irecv = bf.get<uint8_t>((uint64_t)W * XI, i8, (uint64_t)W * XI);
  unsigned long long* scnt = bf.get<unsigned long long>(W, i8 + (uint64_t)W * XI, W);
  uint8_t* recv = bf.get<uint8_t>((uint64_t)W * cap, o8, (uint64_t)W * cap);
  unsigned long long* rcnt = bf.get<unsigned long long>(W, o8 + (uint64_t)W * cap, W);
  unsigned long long* host = bf.get<unsigned long long>(2ull * W, o8 + (uint64_t)W * cap + 8ull * W, 2ull * W);
  const uint32_t hw[HALT_WORDS] = {fl & 2u ? 1u : 0u, 0, 0, 0, 0};
  uint32_t* halt = bf.get<uint32_t>(HALT_WORDS, hw, HALT_WORDS);
  if (bf.rc != SWIM_OK) return bf.rc;
  hipLaunchKernelGGL(k_inline_in, dim3(W), dim3(256), 0, 0, irecv, recv, (uint64_t)cap, scnt, rcnt, host, W,
                     fl & 1u ? (const uint32_t*)halt : nullptr, XI);  // launch_inline_in's grid
  if (bf.ran() && bf.back(o8, recv, (uint64_t)W * cap) && bf.back(o8 + (uint64_t)W * cap, rcnt, 8ull * W))
    bf.back(o8 + (uint64_t)W * cap + 8ull * W, host, 16ull * W);
  return bf.rc;
}

// launch_gossip_send and (GS_APPLY) launch_gossip_apply for one tick on caller-built holder state (one GPU, no link delays)
int prim_gossip(const uint32_t* P, size_t np, const uint32_t* in, size_t inb, uint32_t* out, size_t outb) {
  if (np != 27) return SWIM_EINVAL;
  const uint32_t N = P[0], F = P[1], SLOTS = P[2], BCAP = P[3], LOGW = P[4], lat = P[5], gossip_t = P[6], EXPB = P[7], k = P[8],
                 rr_atomic = P[11], cev_cap = P[12], CRCAP = P[13], RPCAP = P[14], SLOWCAP = P[15], RCAP = P[16], HCAP = P[17],
                 sort_cap = P[18], rank = P[19], SPR = P[20], fl = P[21], ep_loss = P[25], ep_part = P[26];
  const GossipChunks chunks{P[22], P[23], P[24]};
  const bool apply = fl & SWIM_PRIM_GS_APPLY;
  if (N < 1 || N > 4096 || F < 1 || F > 8 || (SLOTS & 63u) || SLOTS < 64 || SLOTS > (1u << 18) || (uint64_t)N * SLOTS > (1u << 21) ||
      !pow2(BCAP) || BCAP > 16384 || (uint64_t)N * BCAP > PRIM_MAX || !pow2(LOGW) || LOGW > 256 || lat > (1u << 16) || gossip_t < 1 ||
      gossip_t > (1u << 16) || EXPB > (1u << 20) || k < 1 || k >= (1u << 30) || cev_cap > CEV || CRCAP < 1 || CRCAP > 4096 ||
      (uint64_t)CRCAP * (SLOTS / 64) > PRIM_MAX || RPCAP < 1 || RPCAP > (1u << 20) || SLOWCAP < 1 || SLOWCAP > (1u << 20) || RCAP < 1 ||
      RCAP > PRIM_MAX || !pow2(HCAP) || HCAP > (1u << 16) || !pow2(sort_cap) || sort_cap < 2 || sort_cap > SORT_MAX || SPR < 1 ||
      rank >= 64 || fl > 7 || ep_loss > 100 || ep_part > 1 ||
      // the staged kernels' dynamic LDS (64 KB per workgroup): 4 waves x 2 rows x cw, 2 rows x cb, 1 row x cx words
      chunks.cw > 1024 || chunks.cb > 4096 || chunks.cx > 8192)
    return SWIM_EINVAL;
  const uint32_t QW = SLOTS / 64, NS = key_plane_sizes(N).NS;
  const uint64_t NF = (uint64_t)N * F, NL = (uint64_t)N * LOGW;
  auto pad8 = [](uint64_t b) { return (b + 7u) & ~7ull; };

  // ---- the layouts: every array starts 8-byte aligned (its bytes rounded up to a multiple of 8) ----
  const uint64_t b_in = 16ull * SLOTS + 2 * pad8(4ull * SLOTS) + 7 * pad8(4ull * N) + pad8(4 * NF) + 3 * pad8(4 * NL) +
                        pad8(4 * NL * F) + 2 * pad8(4ull * N) + (apply ? pad8(4ull * N * NS) : 0);
  const uint64_t b_out = 16ull * QW + 16ull * N * QW + 8ull * CRCAP * QW + 8ull * RPCAP + 8ull * SLOWCAP + 8ull * HCAP * HREC +
                         16ull * RCAP + 8 + 16ull * N + 8ull * FB_N + pad8(2ull * N * SLOTS) + pad8(4ull * N * BCAP) +
                         21 * pad8(4ull * N) + 4 * pad8(4ull * SLOTS) + pad8(4ull * QW) + 4 * pad8(4 * NF) + pad8(4 * NF * CEVW) +
                         pad8(12ull * CRCAP) + pad8(4ull * RCAP) + 64 + 32;
  if (inb != b_in || outb != b_out) return SWIM_EINVAL;
  Cursor ci{(uint8_t*)in}, co{(uint8_t*)out};
  auto in4 = [&](uint64_t n) { return (const uint32_t*)ci.take(pad8(4 * n)); };
  const uint64_t* i_gid = (const uint64_t*)ci.take(8ull * SLOTS);
  const uint64_t* i_key = (const uint64_t*)ci.take(8ull * SLOTS);
  const uint32_t *i_subj = in4(SLOTS), *i_ctick = in4(SLOTS), *i_first = in4(N), *i_tround = in4(N), *i_tcnt = in4(N),
                 *i_tspread = in4(N), *i_tperiod = in4(N), *i_spchg = in4(N), *i_lpos = in4(N), *i_T = in4(NF), *i_ltick = in4(NL),
                 *i_lspread = in4(NL), *i_lcnt = in4(NL), *i_ltg = in4(NL * F), *i_group = in4(N), *i_leaving = in4(N),
                 *i_rowk = apply ? in4((uint64_t)N * NS) : nullptr;
  auto out8 = [&](uint64_t n) { return (uint64_t*)co.take(8 * n); };
  auto out4 = [&](uint64_t n) { return (uint32_t*)co.take(pad8(4 * n)); };
  uint64_t *o_gu = out8(QW), *o_dm = out8(QW), *o_hb = out8((uint64_t)N * QW), *o_wb = out8((uint64_t)N * QW),
           *o_rx = out8((uint64_t)CRCAP * QW), *o_rp = out8(RPCAP), *o_slow = out8(SLOWCAP), *o_hist = out8((uint64_t)HCAP * HREC),
           *o_raw = out8(RCAP), *o_rkey = out8(RCAP), *o_ctr = out8(1), *o_em = out8(2ull * N), *o_fb = out8(FB_N);
  uint16_t* o_S = (uint16_t*)co.take(pad8(2ull * N * SLOTS));
  uint32_t *o_rg = out4((uint64_t)N * BCAP), *o_dead = out4(N), *o_rhead = out4(N), *o_rtail = out4(N), *o_rwin = out4(N),
           *o_rseen = out4(N), *o_held = out4(N), *o_rsend = out4(N), *o_rwnew = out4(N), *o_rt0 = out4(N), *o_tcs = out4(N),
           *o_tcnt = out4(N), *o_tfill = out4(N), *o_toff = out4(N), *o_drx = out4(N), *o_ndrop = out4(N), *o_rwl = out4(N),
           *o_tlist = out4(N), *o_ap = out4(N), *o_roff = out4(N), *o_rcnt = out4(N), *o_sg = out4(N), *o_exp = out4(SLOTS),
           *o_used = out4(SLOTS), *o_fexp = out4(SLOTS), *o_free = out4(SLOTS), *o_agroup = out4(QW), *o_tin = out4(NF),
           *o_tcontact = out4(NF), *o_cin = out4(NF), *o_crow = out4(NF), *o_cev = out4(NF * CEVW), *o_rxl = out4(3ull * CRCAP),
           *o_rslot = out4(RCAP), *o_sc = out4(16), *o_err = out4(8);

  // ---- host checks: everything the kernels index with ----
  uint64_t used = 0;
  for (uint32_t q = 0; q < QW; ++q) used += (uint64_t)__builtin_popcountll(o_gu[q]);
  const int32_t free_top = (int32_t)o_sc[11];
  if (free_top < 0 || (uint64_t)free_top + used > SLOTS || o_sc[7] != 0) return SWIM_EINVAL;  // sc[7]: rc_n starts a tick at 0
  for (uint32_t g = 0; g < SLOTS; ++g)
    if (i_subj[g] != USER_SUBJ && i_subj[g] >= N) return SWIM_EINVAL;
  for (uint32_t m = 0; m < N; ++m) {
    if (i_tcnt[m] > F) return SWIM_EINVAL;
    for (uint32_t s = 0; s < i_tcnt[m]; ++s)
      if (i_T[(uint64_t)m * F + s] >= N) return SWIM_EINVAL;
    for (uint32_t e = 0; e < LOGW; ++e) {
      const uint64_t li = (uint64_t)m * LOGW + e;
      if (i_lcnt[li] > F) return SWIM_EINVAL;
      for (uint32_t s = 0; s < i_lcnt[li]; ++s)
        if (i_ltg[li * F + s] >= N) return SWIM_EINVAL;
    }
    const uint32_t h = o_rhead[m], len = o_rtail[m] - h;  // positions are absolute and may wrap: differences only
    if (len > BCAP || o_rwin[m] - h > len || o_rseen[m] - h > len) return SWIM_EINVAL;
    for (uint32_t j = 0; j < len; ++j)
      if ((o_rg[(uint64_t)m * BCAP + ((h + j) & (BCAP - 1))] & RG_SLOT) >= SLOTS) return SWIM_EINVAL;
  }

  // ---- the Dev: only the fields the two launchers' kernels read ----
  PrimBufs bf;
  Dev d;
  memset(&d, 0, sizeof d);
  d.N = N, d.NS = NS, d.F = F, d.SLOTS = SLOTS, d.QW = QW, d.BCAP = BCAP, d.LOGW = LOGW, d.lat = lat, d.gossip_t = gossip_t;
  d.gt_mul = gt_mul_of(gossip_t), d.EXPB = EXPB, d.seed_lo = P[9], d.seed_hi = P[10], d.rr_atomic = rr_atomic, d.cev_cap = cev_cap;
  d.CRCAP = CRCAP, d.RPCAP = RPCAP, d.SLOWCAP = SLOWCAP, d.RCAP = RCAP, d.HCAP = HCAP, d.sort_cap = sort_cap, d.rank = rank, d.SPR = SPR;
  d.W = d.XW = 1, d.lo = 0, d.hi = N, d.NL = N;
  for (uint32_t e = 0; e < MAX_EPOCHS; ++e) d.ep_from[e] = e ? NEVER : 0u;  // one settings epoch
  d.ep_loss[0] = ep_loss, d.ep_part[0] = ep_part;
  d.slot_gid = bf.get<uint64_t>(SLOTS, i_gid, SLOTS);
  d.slot_key = bf.get<uint64_t>(SLOTS, i_key, SLOTS);
  d.slot_subj = bf.get<uint32_t>(SLOTS, i_subj, SLOTS);
  d.slot_ctick = bf.get<uint32_t>(SLOTS, i_ctick, SLOTS);
  d.firstGossip = bf.get<uint32_t>(N, i_first, N);
  d.tround = bf.get<uint32_t>(N, i_tround, N);
  d.tcnt = bf.get<uint32_t>(N, i_tcnt, N);
  d.tspread = bf.get<uint32_t>(N, i_tspread, N);
  d.tperiod = bf.get<uint32_t>(N, i_tperiod, N);
  d.spchg = bf.get<uint32_t>(N, i_spchg, N);
  d.log_pos = bf.get<uint32_t>(N, i_lpos, N);
  d.T = bf.get<uint32_t>(NF, i_T, NF);
  d.log_tick = bf.get<uint32_t>(NL, i_ltick, NL);
  d.log_spread = bf.get<uint32_t>(NL, i_lspread, NL);
  d.log_cnt = bf.get<uint32_t>(NL, i_lcnt, NL);
  d.log_tg = bf.get<uint32_t>(NL * F, i_ltg, NL * F);
  d.ep_group = bf.get<uint32_t>((uint64_t)MAX_EPOCHS * N, i_group, N);
  d.leaving = bf.get<uint32_t>(N, i_leaving, N);
  d.rowk = apply ? bf.get<uint32_t>((uint64_t)N * NS, i_rowk, (uint64_t)N * NS) : nullptr;
  // in/out: loaded from the caller's words, copied back after the launches
  struct Back {
    void* host;
    const void* dev;
    uint64_t bytes;
  };
  std::vector<Back> backs;
  auto io8 = [&](uint64_t* h, uint64_t n) {
    unsigned long long* p = bf.get<unsigned long long>(n, h, n);
    backs.push_back({h, p, 8 * n});
    return p;
  };
  auto io4 = [&](uint32_t* h, uint64_t n) {
    uint32_t* p = bf.get<uint32_t>(n, h, n);
    backs.push_back({h, p, 4 * n});
    return p;
  };
  d.GU = io8(o_gu, QW), d.DM = io8(o_dm, QW), d.HB = io8(o_hb, (uint64_t)N * QW), d.WB = io8(o_wb, (uint64_t)N * QW);
  d.RX = io8(o_rx, (uint64_t)CRCAP * QW);
  d.rp = (uint64_t*)io8(o_rp, RPCAP), d.slow = (uint64_t*)io8(o_slow, SLOWCAP), d.hist = (uint64_t*)io8(o_hist, (uint64_t)HCAP * HREC);
  d.rc_raw = (uint64_t*)io8(o_raw, RCAP), d.rc_key = (uint64_t*)io8(o_rkey, RCAP);
  d.ctr = bf.get<unsigned long long>(C_NCTR);
  unsigned long long* em = bf.get<unsigned long long>(2ull * N, o_em, 2ull * N);
  unsigned long long* fb = bf.get<unsigned long long>(FB_N, o_fb, FB_N);
  d.em = fl & SWIM_PRIM_GS_EM ? em : nullptr;
  d.fb = fl & SWIM_PRIM_GS_FB ? fb : nullptr;
  backs.push_back({o_em, em, 16ull * N});
  backs.push_back({o_fb, fb, 8ull * FB_N});
  d.S = bf.get<uint16_t>((uint64_t)N * SLOTS, o_S, (uint64_t)N * SLOTS);
  backs.push_back({o_S, d.S, 2ull * N * SLOTS});
  d.rg = io4(o_rg, (uint64_t)N * BCAP);
  d.dead_tick = io4(o_dead, N), d.rhead = io4(o_rhead, N), d.rtail = io4(o_rtail, N), d.rwin = io4(o_rwin, N), d.rseen = io4(o_rseen, N);
  d.held = io4(o_held, N), d.rsend = io4(o_rsend, N), d.rwnew = io4(o_rwnew, N), d.rt0 = io4(o_rt0, N);
  d.tin_cnt = bf.get<uint32_t>(N);  // the senders' lists are empty between ticks
  d.tin_fill = bf.get<uint32_t>(N);
  backs.push_back({o_tcnt, d.tin_cnt, 4ull * N});
  backs.push_back({o_tfill, d.tin_fill, 4ull * N});
  d.tin_off = io4(o_toff, N), d.dead_rx = io4(o_drx, N), d.rc_ndrop = io4(o_ndrop, N), d.rwl = io4(o_rwl, N), d.tlist = io4(o_tlist, N);
  d.ap_list = io4(o_ap, N), d.rc_off = io4(o_roff, N);
  d.rc_cnt = bf.get<uint32_t>(N);
  d.rc_fill = bf.get<uint32_t>(N);
  backs.push_back({o_rcnt, d.rc_cnt, 4ull * N});
  d.sg_list = io4(o_sg, N);
  d.slot_exp = io4(o_exp, SLOTS), d.slot_used = io4(o_used, SLOTS), d.fexp = io4(o_fexp, SLOTS), d.free_list = io4(o_free, SLOTS);
  d.agroup = io4(o_agroup, QW), d.tin = io4(o_tin, NF), d.tcontact = io4(o_tcontact, NF), d.cin = io4(o_cin, NF), d.crow = io4(o_crow, NF);
  d.cev = io4(o_cev, NF * CEVW), d.rxl = io4(o_rxl, 3ull * CRCAP), d.rc_slot = io4(o_rslot, RCAP);
  uint32_t* sc = io4(o_sc, 16);  // nagroup[2], nrwl, ntl, nrx, rp_n, slow_n, rc_n, nap, nsg, nfexp, free_top, hist_n, ncfl, xd_n, 0
  d.nagroup = sc, d.nrwl = sc + 2, d.ntl = sc + 3, d.nrx = sc + 4, d.rp_n = sc + 5, d.slow_n = sc + 6, d.rc_n = sc + 7, d.nap = sc + 8;
  d.nsg = sc + 9, d.nfexp = sc + 10, d.free_top = (int32_t*)(sc + 11), d.hist_n = sc + 12, d.ncfl = sc + 13, d.xd_n = sc + 14;
  d.err = bf.get<uint32_t>(8);
  d.cfl = bf.get<uint32_t>(NF);
  d.scan_part = bf.get<uint32_t>(1024);
  d.rc_key2 = bf.get<uint64_t>(RCAP);
  d.rc_slot2 = bf.get<uint32_t>(RCAP);
  Dev* self = bf.get<Dev>(1);
  d.self = self;
  if (bf.rc == SWIM_OK && hipMemcpy(self, &d, sizeof d, hipMemcpyHostToDevice) != hipSuccess) bf.rc = SWIM_EDEVICE;
  if (bf.rc != SWIM_OK) return bf.rc;

  launch_gossip_send(d, k, 0, nullptr, &chunks);
  if (!bf.ran() || !bf.back(o_tcs, d.tin_cnt, 4ull * N)) return bf.rc;  // before k_gossip_apply clears it
  if (apply) {
    launch_gossip_apply(d, k, 0);
    if (!bf.ran()) return bf.rc;
  }
  for (const Back& b : backs)
    if (!bf.back(b.host, b.dev, b.bytes)) return bf.rc;
  if (bf.back(o_ctr, d.ctr + C_G, 8)) bf.back(o_err, d.err, 32);
  return bf.rc;
}

}  // namespace
}  // namespace swim

extern "C" int swim_debug_prim_eval(uint32_t op, const uint32_t* params, size_t n_params, const void* in, size_t in_bytes,
                                    void* out, size_t out_bytes, uint32_t device) {
  using namespace swim;
  if (op > SWIM_PRIM_GOSSIP || !params || n_params > 32 || !out || (in_bytes && !in) || ((uintptr_t)in & 7u) ||
      ((uintptr_t)out & 7u))
    return SWIM_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= (int)device || hipSetDevice((int)device) != hipSuccess)
    return SWIM_EDEVICE;
  const uint32_t* i32 = (const uint32_t*)in;
  uint32_t* o32 = (uint32_t*)out;
  switch (op) {
    case SWIM_PRIM_SCAN: return prim_scan(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_SEG_SORT: return prim_seg_sort(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_ROUTING: return prim_routing(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_WAVE: return prim_wave(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_DIRTY: return prim_dirty(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_ARITH: return prim_arith(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_FEISTEL: return prim_feistel(params, n_params, in_bytes, o32, out_bytes);
    case SWIM_PRIM_RING_MOVE: return prim_ring_move(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_SYNC_DIFF: return prim_sync_diff(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_XPACK: return prim_xpack(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_PACK_B: return prim_pack_b(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_INLINE_IN: return prim_inline_in(params, n_params, i32, in_bytes, o32, out_bytes);
    case SWIM_PRIM_XUNPACK: return prim_xunpack(params, n_params, i32, in_bytes, o32, out_bytes);
    default: return prim_gossip(params, n_params, i32, in_bytes, o32, out_bytes);
  }
}
