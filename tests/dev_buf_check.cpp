// Stand-alone host check of srsran_4g_amd/csrc/dev_buf.h (built and run by test_dev_buf_host.py).
// hipMalloc / hipFree / hipHostMalloc / hipHostFree are counting wrappers over malloc / free defined here,
// with a switch that fails the next allocation; no HIP runtime is linked.
#include "dev_buf.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <type_traits>

static int      g_live = 0, g_allocs = 0, g_frees = 0, g_host_live = 0, g_host_frees = 0;
static bool     g_fail_next = false;
static size_t   g_last_bytes = 0;
static unsigned g_last_flags = 0;

static hipError_t fake_alloc(void** p, size_t bytes, int* live) {
  if (g_fail_next) {
    g_fail_next = false;
    *p          = nullptr;
    return hipErrorOutOfMemory;
  }
  *p           = malloc(bytes ? bytes : 1);
  g_last_bytes = bytes;
  g_allocs++, (*live)++;
  return hipSuccess;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes, &g_live); }
extern "C" hipError_t hipFree(void* p) {
  if (p) g_live--, g_frees++;
  free(p);
  return hipSuccess;
}
extern "C" hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) {
  g_last_flags = flags;
  return fake_alloc(p, bytes, &g_host_live);
}
extern "C" hipError_t hipHostFree(void* p) {
  if (p) g_host_live--, g_host_frees++;
  free(p);
  return hipSuccess;
}

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

using srsran_amd::DevBuf;
using srsran_amd::PinBuf;

static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_assignable<DevBuf<float>>::value, "");
static_assert(!std::is_copy_constructible<PinBuf<int>>::value && !std::is_copy_assignable<PinBuf<int>>::value, "");

struct Several {
  DevBuf<float>   a;
  DevBuf<uint8_t> b;
  PinBuf<int>     c{hipHostMallocDefault};
};

template <typename B>
static void common(int* live, int* frees) {
  const int live0 = *live;
  {
    B b;
    CHECK(b.get() == nullptr && b.cap() == 0);
    CHECK(b.reserve(0) && b.get() == nullptr);  // n <= cap: nothing done
    CHECK(b.reserve(10) && b.get() && b.cap() == 10 && *live == live0 + 1);
    CHECK(g_last_bytes == 10 * sizeof(*b.get()));
    b.get()[9] = 1;                              // the whole block is writable (ASan checks the size)
    auto* p = b.get();
    int   f = *frees, a = g_allocs;
    CHECK(b.reserve(10) && b.reserve(3) && b.get() == p && b.cap() == 10);  // n <= cap keeps the pointer
    CHECK(*frees == f && g_allocs == a);
    CHECK(b.reserve(11) && b.cap() == 11 && *frees == f + 1 && g_allocs == a + 1 && *live == live0 + 1);  // growth frees once
    b.get()[10] = 1;
    CHECK(b.reserve(12, 64) && b.cap() == 64 && g_last_bytes == 64 * sizeof(*b.get()));  // floor applied
    b.get()[63] = 1;
    CHECK(b.reserve(100, 64) && b.cap() == 100);                                         // ... only as a minimum
    // failed allocation: empty buffer, old block released, a later reserve works
    g_fail_next = true;
    CHECK(!b.reserve(200) && b.get() == nullptr && b.cap() == 0 && *live == live0);
    CHECK(b.reserve(5) && b.get() && b.cap() == 5 && *live == live0 + 1);
    // move construction leaves the source empty
    p = b.get();
    B c(std::move(b));
    CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == p && c.cap() == 5 && *live == live0 + 1);
    // move assignment frees the destination's old block
    B d;
    CHECK(d.reserve(7) && *live == live0 + 2);
    f = *frees;
    d = std::move(c);
    CHECK(c.get() == nullptr && c.cap() == 0 && d.get() == p && d.cap() == 5 && *frees == f + 1 && *live == live0 + 1);
    d.reset();
    CHECK(d.get() == nullptr && d.cap() == 0 && *live == live0);
    d.reset();                                   // idempotent
    CHECK(d.reserve(2));
  }                                              // destructor releases
  CHECK(*live == live0);
}

int main() {
  common<DevBuf<float>>(&g_live, &g_frees);
  common<DevBuf<uint8_t>>(&g_live, &g_frees);
  common<PinBuf<int>>(&g_host_live, &g_host_frees);
  CHECK(g_host_frees > 0 && g_live == 0 && g_host_live == 0);
  {
    PinBuf<int> w(hipHostMallocWriteCombined);  // the flags reach hipHostMalloc
    CHECK(w.reserve(4) && g_last_flags == hipHostMallocWriteCombined);
    PinBuf<int> m(std::move(w));
    g_last_flags = 0;
    CHECK(m.reserve(8) && g_last_flags == hipHostMallocWriteCombined);
  }
  {
    std::map<int, DevBuf<float>> m;
    for (int i = 0; i < 5; i++) CHECK(m[i].reserve(i + 1));
    CHECK(g_live == 5);
    m.erase(2);
    CHECK(g_live == 4);
    auto* s = new Several;
    CHECK(s->a.reserve(3) && s->b.reserve(100) && s->c.reserve(2) && g_live == 6 && g_host_live == 1);
    g_fail_next = true;                          // a half-built object still releases what it has
    CHECK(!s->a.reserve(1000) && g_live == 5);
    delete s;
    CHECK(g_live == 4 && g_host_live == 0);
  }
  CHECK(g_live == 0 && g_host_live == 0);
  printf("dev_buf OK: %d allocations, %d + %d frees, 0 live\n", g_allocs, g_frees, g_host_frees);
  return g_live | g_host_live;
}
