// Host check of csrc/lip_bindcache.h (the bookkeeping of the engine's Winograd-transform cache), no GPU and no HIP:
// the allocator is a counting malloc.  Built and run by tests/test_bind_cache_cpu.py; exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include "lip_bindcache.h"

using lip::BindCache;
using lip::BindKey;

static int g_allocs = 0, g_frees = 0, g_fail_next = 0;
static std::set<void*> g_live;

static void* test_alloc(size_t bytes) {
  if (g_fail_next > 0) { --g_fail_next; return nullptr; }
  void* p = malloc(bytes);
  ++g_allocs;
  g_live.insert(p);
  return p;
}
static void test_free(void* p) {
  if (!g_live.erase(p)) { fprintf(stderr, "free of a pointer the cache does not own\n"); exit(2); }
  ++g_frees;
  free(p);
}

static int g_failed = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

int main() {
  int w0, w1, act;                                        // three "device tensors": only their addresses matter
  const void* sA = (const void*)0x10;
  const void* sB = (const void*)0x20;
  const BindKey kU{&w0, 0, {32, 32, 0, 0, 0}}, kUflip{&w0, 1, {32, 32, 0, 0, 0}}, kU1{&w1, 0, {32, 64, 0, 0, 0}};
  const BindKey kV{&act, 2, {8, 8, 32, 64, 64}}, kV2{&act, 2, {8, 8, 32, 64, 128}};
  {
    BindCache c(test_alloc, test_free, 1 << 20);
    // first use: allocated, to be filled; second use: the same buffer, filled
    BindCache::Hit h = c.get(kU, 1000, sA);
    CHECK(h.buf && h.fill && c.entries() == 1 && c.bytes() == 4000);
    float* u = h.buf;
    h = c.get(kU, 1000, sA);
    CHECK(h.buf == u && !h.fill && g_allocs == 1);
    // the key tells the forms, the sources and the geometry apart
    BindCache::Hit f = c.get(kUflip, 1000, sA), u1 = c.get(kU1, 2000, sA), v = c.get(kV, 3000, sA), v2 = c.get(kV2, 6000, sA);
    CHECK(f.buf && f.fill && f.buf != u && u1.buf && u1.fill && v.buf && v.fill && v2.buf && v2.fill && v2.buf != v.buf);
    CHECK(c.entries() == 5 && c.bytes() == 4 * (1000 + 1000 + 2000 + 3000 + 6000));
    // a second stream never sees the first stream's buffers, and allocates nothing
    h = c.get(kU, 1000, sB);
    CHECK(!h.buf && !h.fill && c.entries() == 5);
    h = c.get(BindKey{&w1, 1, {32, 64, 0, 0, 0}}, 2000, sB);
    CHECK(!h.buf && g_allocs == 5);
    // primal pass: invalidate BEFORE its launches and AFTER them.  Every entry asks for one refill, in place
    c.invalidate();
    h = c.get(kV, 3000, sA);                              // (a sweep that raced the pass: filled from half-written activations)
    CHECK(h.buf == v.buf && h.fill);
    c.invalidate();
    h = c.get(kV, 3000, sA);
    CHECK(h.buf == v.buf && h.fill);                      // ... is stale again after the pass
    h = c.get(kV, 3000, sA);
    CHECK(h.buf == v.buf && !h.fill);
    h = c.get(kU, 1000, sA);
    CHECK(h.buf == u && h.fill);
    h = c.get(kU, 1000, sA);
    CHECK(h.buf == u && !h.fill && g_allocs == 5 && g_frees == 0);
    // the owning stream survives a primal pass: the refill is ordered behind the old readers
    h = c.get(kUflip, 1000, sB);
    CHECK(!h.buf);
    // a fill that could not be launched
    c.forget(u);
    h = c.get(kU, 1000, sA);
    CHECK(h.buf == u && h.fill);
    // cap: 1 MiB = 262144 floats; 13000 are held
    h = c.get(BindKey{&w1, 2, {1, 0, 0, 0, 0}}, 262144 - 13000 + 1, sA);
    CHECK(!h.buf && c.entries() == 5 && g_allocs == 5);
    h = c.get(BindKey{&w1, 2, {1, 0, 0, 0, 0}}, 262144 - 13000, sA);
    CHECK(h.buf && h.fill && c.bytes() == (size_t)1 << 20);
    h = c.get(BindKey{&w1, 2, {2, 0, 0, 0, 0}}, 1, sA);
    CHECK(!h.buf);
    h = c.get(kV2, 6000, sA);                             // what is held stays usable at the cap
    CHECK(h.buf == v2.buf && h.fill);                     // (stale since the pass above, never refilled until now)
    // re-binding: everything freed, the stream forgotten
    c.release();
    CHECK(c.entries() == 0 && c.bytes() == 0 && g_frees == 6 && g_live.empty());
    h = c.get(kU, 1000, sB);
    CHECK(h.buf && h.fill);
    h = c.get(kU, 1000, sA);
    CHECK(!h.buf);
    // a failed allocation: no entry, no stream taken, the next call may succeed
    c.release();
    g_fail_next = 1;
    h = c.get(kU, 1000, sA);
    CHECK(!h.buf && c.entries() == 0);
    h = c.get(kU, 1000, sB);
    CHECK(h.buf && h.fill);
    // huge requests do not wrap the cap arithmetic
    h = c.get(kV, ((size_t)-1) / 4, sB);
    CHECK(!h.buf);
    h = c.get(kV, (size_t)-1, sB);
    CHECK(!h.buf);
  }
  CHECK(g_live.empty() && g_allocs == g_frees);           // the destructor released the rest
  {
    BindCache zero(test_alloc, test_free, 0);             // LIP_BINDCACHE_MB=0: never allocates
    const int before = g_allocs;
    CHECK(!zero.get(kU, 1000, sA).buf && !zero.get(kU, 1000, sA).buf && g_allocs == before && zero.entries() == 0);
  }
  if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
  printf("bind cache host check ok: %d allocations, %d frees\n", g_allocs, g_frees);
  return 0;
}
