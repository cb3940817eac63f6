// dev_alloc.h — the registry of a handle's device allocations, and the staged replacement that capacity growth uses.
// Plain C++: the registry reaches the GPU only through the three dev_raw_* functions below (dev_raw.hip defines them
// over hipMalloc / hipFree / hipMemsetAsync; the stand-alone check alloc_check.cpp links malloc-backed ones).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace swim {
#pragma GCC visibility push(hidden)

// nullptr, or why the allocation failed
const char* dev_raw_alloc(void** p, size_t bytes);
void dev_raw_free(void* p);
void dev_raw_fill(void* p, int byte, size_t bytes, void* stream);  // ordered on the stream

constexpr size_t GUARD = 4096;  // SWIM_GUARD: guard bytes on each side of every device allocation

struct DevAllocs {
  struct Entry {
    void* raw;      // what dev_raw_alloc returned
    void* user;     // what the caller holds: raw, or raw + GUARD
    size_t bytes;   // as asked for
    size_t gbytes;  // as allocated: bytes, or bytes + 2 GUARD
  };
  std::vector<Entry> live;  // in allocation order
  size_t bytes = 0;         // sum of live[i].bytes (swim_counters.device_bytes)
  std::string err;          // the latest failure
  void* stream = nullptr;   // the guard and poison fills are ordered on it
  // debugging aids, read from the environment once, when the handle is made: SWIM_GUARD puts GUARD bytes of 0x5A
  // before and after every allocation (checked after every step); SWIM_POISON fills every fresh allocation with 0xA5,
  // SWIM_POISON_ONLY=i only the one that becomes live[i], to catch state that is read without having been written
  bool guard, poison;
  long poison_only;
  DevAllocs();
  DevAllocs(const DevAllocs&) = delete;
  DevAllocs& operator=(const DevAllocs&) = delete;

  void* alloc(size_t bytes);  // nullptr: err says why
  void free(void* user);      // (a pointer that is not live, nullptr included: nothing)
  void free_all();
};

// Replacements for several buffers of one structure, all or none: add() allocates a replacement and remembers the
// field it is for; commit() frees the old buffers and stores the new pointers; leaving the scope without commit()
// frees the replacements, so the fields (and DevAllocs::bytes) are as before. After a failed add() the later ones
// allocate nothing and ok() is false.
class Staged {
 public:
  explicit Staged(DevAllocs* a) : a_(a) {}
  ~Staged();
  Staged(const Staged&) = delete;
  Staged& operator=(const Staged&) = delete;
  // the replacement of `count` elements (at least one) for *field, or nullptr
  template <class T>
  T* add(T** field, size_t count) {
    return (T*)add_bytes(field, (count ? count : 1) * sizeof(T));
  }
  bool ok() const { return ok_; }
  void commit();

 private:
  void* add_bytes(void* field, size_t bytes);
  struct Item {
    void* field;  // address of the pointer to replace
    void* fresh;
  };
  DevAllocs* a_;
  std::vector<Item> items_;
  bool ok_ = true;
};

#pragma GCC visibility pop
}  // namespace swim
