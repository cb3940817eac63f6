// dev_alloc.cpp — DevAllocs and Staged (dev_alloc.h)
#include "dev_alloc.h"

#include <cstdlib>
#include <cstring>

namespace swim {

DevAllocs::DevAllocs() {
  guard = getenv("SWIM_GUARD") != nullptr;
  poison = getenv("SWIM_POISON") != nullptr;
  const char* po = getenv("SWIM_POISON_ONLY");
  poison_only = po ? atol(po) : -1;
}

void* DevAllocs::alloc(size_t n) {
  Entry e{nullptr, nullptr, n, n + (guard ? 2 * GUARD : 0)};
  if (const char* why = dev_raw_alloc(&e.raw, e.gbytes)) {
    err = "hipMalloc(" + std::to_string(n) + ") failed: " + why;
    return nullptr;
  }
  e.user = e.raw;
  if (guard) {
    dev_raw_fill(e.raw, 0x5A, GUARD, stream);
    dev_raw_fill((char*)e.raw + GUARD + n, 0x5A, GUARD, stream);
    e.user = (char*)e.raw + GUARD;
  }
  if (poison || poison_only == (long)live.size()) dev_raw_fill(e.user, 0xA5, n, stream);
  live.push_back(e);
  bytes += n;
  return e.user;
}

void DevAllocs::free(void* user) {
  for (size_t i = 0; i < live.size(); ++i)
    if (live[i].user == user) {
      dev_raw_free(live[i].raw);
      bytes -= live[i].bytes;
      live.erase(live.begin() + (long)i);
      return;
    }
}

void DevAllocs::free_all() {
  for (const Entry& e : live) dev_raw_free(e.raw);
  live.clear();
  bytes = 0;
}

void* Staged::add_bytes(void* field, size_t bytes) {
  if (!ok_) return nullptr;
  void* p = a_->alloc(bytes);
  if (!p) {
    ok_ = false;
    return nullptr;
  }
  items_.push_back({field, p});
  return p;
}

void Staged::commit() {
  for (const Item& it : items_) {
    void* old;
    std::memcpy(&old, it.field, sizeof(old));  // (the field is a T* of some T)
    a_->free(old);
    std::memcpy(it.field, &it.fresh, sizeof(old));
  }
  items_.clear();
}

Staged::~Staged() {
  for (const Item& it : items_) a_->free(it.fresh);
}

}  // namespace swim
