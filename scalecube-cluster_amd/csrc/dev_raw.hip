// dev_raw.hip — the device-allocation registry's way to the GPU (dev_alloc.h)
#include <hip/hip_runtime.h>

#include "dev_alloc.h"

namespace swim {

const char* dev_raw_alloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

void dev_raw_free(void* p) { (void)hipFree(p); }

void dev_raw_fill(void* p, int byte, size_t bytes, void* stream) {
  (void)hipMemsetAsync(p, byte, bytes, (hipStream_t)stream);
}

}  // namespace swim
