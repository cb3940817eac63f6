// alloc_check.cpp — stand-alone CPU check of DevAllocs and Staged (dev_alloc.h) over malloc-backed raw functions,
// built with ASan + UBSan (make alloc_check): a leak, a double free or a write outside an allocation ends it non-zero.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "dev_alloc.h"

namespace swim {
static long g_fail_at = -1;  // the g_calls-th dev_raw_alloc from now fails (-1: none)
static long g_calls = 0;
static std::set<void*> g_raw;  // what the registry holds of ours
const char* dev_raw_alloc(void** p, size_t bytes) {
  if (g_calls++ == g_fail_at) return "out of memory (injected)";
  *p = malloc(bytes);
  g_raw.insert(*p);
  return nullptr;
}
void dev_raw_free(void* p) {
  if (!g_raw.erase(p)) {
    fprintf(stderr, "dev_raw_free of a pointer that is not allocated\n");
    abort();
  }
  free(p);
}
void dev_raw_fill(void* p, int byte, size_t bytes, void*) { memset(p, byte, bytes); }
}  // namespace swim

using namespace swim;

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

static size_t live_sum(const DevAllocs& a) {
  size_t s = 0;
  for (const auto& e : a.live) s += e.bytes;
  return s;
}

static bool all_bytes(const void* p, int byte, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (((const unsigned char*)p)[i] != (unsigned char)byte) return false;
  return true;
}

// alloc / free / bytes, zero count included (dalloc's rule: at least one element)
static void bookkeeping(bool guard, bool poison) {
  DevAllocs a;
  a.guard = guard, a.poison = poison, a.poison_only = -1;
  uint32_t* p = (uint32_t*)a.alloc(100 * sizeof(uint32_t));
  uint64_t* z = (uint64_t*)a.alloc(1 * sizeof(uint64_t));  // a zero count rounds up to one element
  char* q = (char*)a.alloc(7);
  CHECK(p && z && q && a.live.size() == 3 && a.bytes == 400 + 8 + 7 && a.bytes == live_sum(a));
  CHECK(g_raw.size() == 3);
  for (const auto& e : a.live) {
    CHECK(e.gbytes == e.bytes + (guard ? 2 * GUARD : 0));
    CHECK((char*)e.user == (char*)e.raw + (guard ? GUARD : 0));
    if (guard) CHECK(all_bytes(e.raw, 0x5A, GUARD) && all_bytes((char*)e.user + e.bytes, 0x5A, GUARD));
    if (poison) CHECK(all_bytes(e.user, 0xA5, e.bytes));
  }
  memset(p, 1, 400), memset(z, 2, 8), memset(q, 3, 7);  // the whole user range is writable
  if (guard) CHECK(all_bytes(a.live[0].raw, 0x5A, GUARD) && all_bytes((char*)p + 400, 0x5A, GUARD));
  a.free(z);  // by user pointer, with or without guards
  CHECK(a.live.size() == 2 && a.bytes == 407 && a.bytes == live_sum(a) && g_raw.size() == 2);
  a.free(z), a.free(nullptr);  // not live: nothing
  CHECK(a.live.size() == 2 && a.bytes == 407);
  a.free(p), a.free(q);
  CHECK(a.live.empty() && a.bytes == 0 && g_raw.empty());
}

static void poison_only() {
  DevAllocs a;
  a.guard = a.poison = false, a.poison_only = 1;
  char* p0 = (char*)a.alloc(16);
  memset(p0, 0, 16);
  char* p1 = (char*)a.alloc(16);
  CHECK(all_bytes(p1, 0xA5, 16) && all_bytes(p0, 0, 16));
  a.free_all();
}

struct Five {
  uint32_t* a = nullptr;
  uint64_t* b = nullptr;
  uint16_t* c = nullptr;
  unsigned long long* d = nullptr;
  uint8_t* e = nullptr;
};

static void stage_five(Staged& s, Five& f, size_t n) {
  s.add(&f.a, n), s.add(&f.b, n), s.add(&f.c, n), s.add(&f.d, n), s.add(&f.e, n);
}

static void staged(bool guard) {
  DevAllocs a;
  a.guard = guard, a.poison = false, a.poison_only = -1;
  Five f;
  {
    Staged s(&a);
    stage_five(s, f, 8);
    CHECK(s.ok());
    s.commit();  // (the old pointers are null: nothing to free)
  }
  CHECK(f.a && f.b && f.c && f.d && f.e && a.live.size() == 5 && a.bytes == 8 * (4 + 8 + 2 + 8 + 1));
  memset(f.c, 7, 16);
  const Five before = f;
  const size_t bytes0 = a.bytes;
  std::set<void*> live0;
  for (const auto& e : a.live) live0.insert(e.user);
  // committed: new pointers stored, old buffers freed
  {
    Staged s(&a);
    stage_five(s, f, 16);
    CHECK(s.ok() && f.a == before.a && a.live.size() == 10);  // the fields change only at commit
    s.commit();
  }
  CHECK(f.a != before.a && f.e != before.e && a.live.size() == 5 && a.bytes == 2 * bytes0 && a.bytes == live_sum(a));
  CHECK(g_raw.size() == 5);
  // abandoned at the k-th raw allocation, every k: the fields, bytes and the live set are as before
  const Five kept = f;
  const size_t bytes1 = a.bytes;
  std::set<void*> live1;
  for (const auto& e : a.live) live1.insert(e.user);
  for (long k = 0; k < 5; ++k) {
    {
      Staged s(&a);
      g_calls = 0, g_fail_at = k;
      stage_five(s, f, 32);
      g_fail_at = -1;
      CHECK(!s.ok() && !a.err.empty() && a.live.size() == 5 + (size_t)k);
    }
    std::set<void*> now;
    for (const auto& e : a.live) now.insert(e.user);
    CHECK(now == live1 && a.bytes == bytes1 && a.bytes == live_sum(a) && g_raw.size() == 5);
    CHECK(f.a == kept.a && f.b == kept.b && f.c == kept.c && f.d == kept.d && f.e == kept.e);
  }
  // abandoned with every allocation made (a later step of the stage failed)
  {
    Staged s(&a);
    stage_five(s, f, 32);
    CHECK(s.ok());
  }
  CHECK(a.live.size() == 5 && a.bytes == bytes1 && g_raw.size() == 5);
  a.free_all();  // destroy with live entries
  CHECK(a.live.empty() && a.bytes == 0 && g_raw.empty());
}

int main() {
  for (int g = 0; g < 2; ++g)
    for (int p = 0; p < 2; ++p) bookkeeping(g, p);
  poison_only();
  staged(false);
  staged(true);
  {  // a failed plain allocation changes nothing
    DevAllocs a;
    a.guard = a.poison = false, a.poison_only = -1;
    g_calls = 0, g_fail_at = 0;
    CHECK(a.alloc(64) == nullptr && a.live.empty() && a.bytes == 0 && a.err.find("hipMalloc(64) failed") == 0);
    g_fail_at = -1;
  }
  {  // a zero count is one element, at add and at free alike
    DevAllocs a;
    a.guard = a.poison = false, a.poison_only = -1;
    uint64_t* z = nullptr;
    {
      Staged s(&a);
      CHECK(s.add(&z, 0) != nullptr);
      s.commit();
    }
    CHECK(z && a.bytes == 8);
    a.free(z);
    CHECK(a.bytes == 0 && g_raw.empty());
  }
  printf("alloc_check ok\n");
  return 0;
}
