// route.hip — receipt routing: the exclusive scan and the per-member sort of first receipts by gossip id.
#include <hip/hip_runtime.h>

#include "dev_util.h"

namespace swim {

// ------------------------------------------------------------------------------------------------------------
// receipt routing: counting sort of first receipts by member, then per-member sort by gossip id
__global__ void k_count_rc(const uint64_t* raw, const uint32_t* n_, uint32_t cap, uint32_t* cnt) {
  uint32_t n = *n_ < cap ? *n_ : cap;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    atomicAdd(&cnt[(uint32_t)(raw[i] >> 32)], 1u);
}
__global__ void k_scatter_rc(const Dev d, const uint64_t* raw, const uint32_t* n_, uint32_t cap, const uint32_t* off,
                             uint32_t* fill, uint32_t* idx, uint64_t* key) {
  uint32_t n = *n_ < cap ? *n_ : cap;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    uint32_t t = (uint32_t)(raw[i] >> 32), g = (uint32_t)raw[i];
    const uint32_t f = atomicAdd(&fill[t], 1u);
    if (f == 1u) d.sg_list[wave_append(d.nsg)] = t;  // a segment with two receipts or more: k_seg_sort sorts it
    uint32_t p = off[t] + f;
    idx[p] = g;
    key[p] = d.slot_gid[g];
  }
}

// exclusive scan of n counts: per-1024 block scans, a scan of the block sums, then the add-back
__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t v, uint32_t* sh, uint32_t* total) {
  uint32_t t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (uint32_t o = 1; o < 256; o <<= 1) {
    uint32_t a = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  uint32_t incl = sh[t];
  *total = sh[255];
  __syncthreads();
  return incl - v;
}
__global__ void __launch_bounds__(256) k_scan_blocks(const uint32_t* in, uint32_t* out, uint32_t* part, uint32_t n) {
  __shared__ uint32_t sh[256];
  uint32_t base = blockIdx.x * 1024 + threadIdx.x * 4;
  uint32_t v[4], s = 0;
  for (int j = 0; j < 4; ++j) {
    v[j] = base + j < n ? in[base + j] : 0;
    s += v[j];
  }
  uint32_t tot;
  uint32_t run = block_excl_scan_256(s, sh, &tot);
  for (int j = 0; j < 4; ++j) {
    if (base + j < n) out[base + j] = run;
    run += v[j];
  }
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(256) k_scan_top(uint32_t* part, uint32_t nb) {  // nb <= 1024
  __shared__ uint32_t sh[256];
  uint32_t base = threadIdx.x * 4;
  uint32_t v[4], s = 0;
  for (int j = 0; j < 4; ++j) {
    v[j] = base + j < nb ? part[base + j] : 0;
    s += v[j];
  }
  uint32_t tot;
  uint32_t run = block_excl_scan_256(s, sh, &tot);
  for (int j = 0; j < 4; ++j) {
    if (base + j < nb) part[base + j] = run;
    run += v[j];
  }
}
__global__ void k_scan_add(uint32_t* out, const uint32_t* part, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] += part[i / 1024];
}

// per-segment sort of (key, val) by key (keys are unique within a segment): one block per segment. Segments of
// up to SORT_MAX entries are sorted bitonically in LDS; larger ones (a member receiving thousands of new gossips in
// one tick, C2-style storms) sort SORT_MAX runs in LDS and then merge run pairs through the scratch arrays, each
// element finding its output position by a binary search in the partner run (merge path, no atomics).
// (SORT_MAX: engine.h; the runtime run length is Dev::sort_cap <= SORT_MAX)
__device__ void lds_bitonic(uint64_t* K, uint32_t* V, const uint64_t* key, const uint32_t* val, uint32_t n,
                            uint64_t* okey, uint32_t* oval) {
  uint32_t p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (uint32_t i = threadIdx.x; i < p2; i += blockDim.x) {
    K[i] = i < n ? key[i] : ~0ull;
    V[i] = i < n ? val[i] : 0;
  }
  __syncthreads();
  for (uint32_t size = 2; size <= p2; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t i = threadIdx.x; i < p2; i += blockDim.x) {
        uint32_t j = i ^ stride;
        if (j > i) {
          bool up = (i & size) == 0;
          if ((K[i] > K[j]) == up) {
            uint64_t tk = K[i];
            K[i] = K[j];
            K[j] = tk;
            uint32_t tv = V[i];
            V[i] = V[j];
            V[j] = tv;
          }
        }
      }
      __syncthreads();
    }
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    okey[i] = K[i];
    oval[i] = V[i];
  }
  __syncthreads();
}

// number of entries of the sorted run r[0..n) that are < x
__device__ __forceinline__ uint32_t lower_rank(const uint64_t* r, uint32_t n, uint64_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (r[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// the segments listed in sg (nsg of them: members with two receipts or more, k_scatter_rc), not all N
__global__ void __launch_bounds__(256) k_seg_sort(uint64_t* key, uint32_t* val, uint64_t* tkey, uint32_t* tval,
                                                  const uint32_t* off, const uint32_t* cnt, const uint32_t* sg,
                                                  const uint32_t* nsg, uint32_t run, unsigned long long* fb) {
  __shared__ uint64_t K[SORT_MAX];
  __shared__ uint32_t V[SORT_MAX];
  const uint32_t nseg = *nsg;
  for (uint32_t li = blockIdx.x; li < nseg; li += gridDim.x) {
    const uint32_t sgi = sg[li];
    const uint32_t n = cnt[sgi];
    if (n <= 1) continue;
    const uint32_t o = off[sgi];
    if (n <= run) {
      lds_bitonic(K, V, key + o, val + o, n, key + o, val + o);
      continue;
    }
    if (fb && threadIdx.x == 0) atomicAdd(&fb[FB_SORT_MERGE], 1ull);
    for (uint32_t c = 0; c < n; c += run)
      lds_bitonic(K, V, key + o + c, val + o + c, min(run, n - c), key + o + c, val + o + c);
    uint64_t *sk = key + o, *dk = tkey + o;
    uint32_t *sv = val + o, *dv = tval + o;
    for (uint32_t w = run; w < n; w <<= 1) {
      for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t base = i / (2 * w) * (2 * w), mid = min(base + w, n), end = min(base + 2 * w, n);
        const uint64_t x = sk[i];
        uint32_t pos;
        if (i < mid)  // run A element: its index in A plus the B entries below it
          pos = i + lower_rank(sk + mid, end - mid, x);
        else  // run B element: its index in B plus the A entries below it
          pos = base + (i - mid) + lower_rank(sk + base, mid - base, x);
        dk[pos] = x;
        dv[pos] = sv[i];
      }
      __syncthreads();
      uint64_t* tk = sk;
      sk = dk;
      dk = tk;
      uint32_t* tv = sv;
      sv = dv;
      dv = tv;
    }
    if (sk != key + o) {
      for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        key[o + i] = sk[i];
        val[o + i] = sv[i];
      }
      __syncthreads();
    }
  }
}

// exclusive scan of n counts (n <= 2^20)
void launch_scan(const uint32_t* in, uint32_t* out, uint32_t* part, uint32_t n, hipStream_t st) {
  uint32_t nb = cdiv(n, 1024);
  hipLaunchKernelGGL(k_scan_blocks, dim3(nb), dim3(256), 0, st, in, out, part, n);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(256), 0, st, part, nb);
  hipLaunchKernelGGL(k_scan_add, dim3(cdiv(n, 256)), dim3(256), 0, st, out, part, n);
}

// receipts routed to P4: counting sort by member, then each member's receipts by gossip id
void launch_receipt_routing(const Dev& d, hipStream_t st) {
  hipLaunchKernelGGL(k_count_rc, dim3(256), dim3(256), 0, st, d.rc_raw, d.rc_n, d.RCAP, d.rc_cnt);
  launch_scan(d.rc_cnt, d.rc_off, d.scan_part, d.N, st);
  hipLaunchKernelGGL(k_scatter_rc, dim3(256), dim3(256), 0, st, d, d.rc_raw, d.rc_n, d.RCAP, d.rc_off, d.rc_fill,
                     d.rc_slot, d.rc_key);
  hipLaunchKernelGGL(k_seg_sort, dim3(1024), dim3(256), 0, st, d.rc_key, d.rc_slot, d.rc_key2, d.rc_slot2, d.rc_off,
                     d.rc_cnt, d.sg_list, d.nsg, d.sort_cap, d.fb);
}

}  // namespace swim
