// Per-engine cache of the Winograd transforms that depend only on the binding: the transformed shared 3x3 kernels U
// (forward and flipped) of run_igemm_wino and the transformed primal activations Vt of run_wgrad_wino.  Host-side
// bookkeeping only (no HIP call of its own: the allocator is handed in, so a host program can drive it).
//
//   get()         an entry's buffer and whether the caller has to fill it (on `stream`, before the kernel that reads it).
//                 The first stream that fills an entry owns the cache: kernels of one stream are ordered, so a refill
//                 cannot overtake a reader.  Any other stream, a full cache or a failed allocation get a null buffer
//                 and the caller takes its per-launch transform.
//   invalidate()  the primal pass ran (the only point where weights or activations change): every entry is stale,
//                 buffers and the owning stream are kept, the next get() of a key asks for a refill in place.
//   release()     re-binding or destruction: buffers go back through the allocator's free (which must not return while
//                 the device still reads them: hipFree waits), the stream is forgotten.
//
// Policy (read once per process, like every other LIP_* variable; they pick no kernel route, so their A/B test is
// tests/test_bind_cache.py, which starts one child process per setting):
//   LIP_NOBINDCACHE     engines get no cache: the transforms run on every launch
//   LIP_BINDCACHE_MB    cap of ONE engine's cache in MiB, default 512 (the CIFAR binding of the benchmark holds ~270 MB
//                       of U and Vt; an ExampleChunkedGGN holds one engine per example chunk).  0: nothing is ever cached
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <vector>

namespace lip {

struct BindCachePolicy {
  bool off;
  size_t cap_bytes;
};
inline const BindCachePolicy& bind_cache_policy() {
  static const BindCachePolicy pol = [] {
    const char* mb = getenv("LIP_BINDCACHE_MB");
    const long v = mb ? atol(mb) : 512;
    return BindCachePolicy{getenv("LIP_NOBINDCACHE") != nullptr, (size_t)(v > 0 ? v : 0) << 20};
  }();
  return pol;
}

struct BindKey {
  const void* src;      // device pointer of the untransformed tensor
  int kind;             // 0: U of the forward form, 1: U of the flipped form, 2: Vt
  int d[5];             // the geometry that fixes the transform's output (unused fields 0)
  bool operator==(const BindKey& o) const {
    return src == o.src && kind == o.kind && d[0] == o.d[0] && d[1] == o.d[1] && d[2] == o.d[2] && d[3] == o.d[3] && d[4] == o.d[4];
  }
};

class BindCache {
 public:
  typedef void* (*AllocFn)(size_t bytes);
  typedef void (*FreeFn)(void* ptr);
  struct Hit { float* buf; bool fill; };

  BindCache(AllocFn alloc, FreeFn free_fn, size_t cap_bytes) : alloc_(alloc), free_(free_fn), cap_(cap_bytes) {}
  ~BindCache() { release(); }
  BindCache(const BindCache&) = delete;
  BindCache& operator=(const BindCache&) = delete;

  Hit get(const BindKey& key, size_t floats, const void* stream) {
    if (has_stream_ && stream != stream_) return Hit{nullptr, false};
    for (Entry& e : entries_)
      if (e.key == key && e.floats == floats) {
        const bool fill = !e.valid;
        e.valid = true;
        return Hit{e.buf, fill};
      }
    if (floats == 0 || floats > cap_ / sizeof(float)) return Hit{nullptr, false};
    const size_t bytes = floats * sizeof(float);
    if (bytes_ > cap_ - bytes) return Hit{nullptr, false};
    float* buf = static_cast<float*>(alloc_(bytes));
    if (!buf) return Hit{nullptr, false};
    entries_.push_back(Entry{key, floats, buf, true});
    bytes_ += bytes;
    has_stream_ = true; stream_ = stream;
    return Hit{buf, true};
  }
  // the fill of an entry get() handed out could not be launched: it holds nothing
  void forget(const float* buf) {
    for (Entry& e : entries_)
      if (e.buf == buf) e.valid = false;
  }
  void invalidate() {
    for (Entry& e : entries_) e.valid = false;
  }
  void release() {
    for (Entry& e : entries_) free_(e.buf);
    entries_.clear();
    bytes_ = 0; has_stream_ = false; stream_ = nullptr;
  }
  size_t bytes() const { return bytes_; }
  size_t entries() const { return entries_.size(); }

 private:
  struct Entry { BindKey key; size_t floats; float* buf; bool valid; };
  AllocFn alloc_; FreeFn free_;
  size_t cap_, bytes_ = 0;
  std::vector<Entry> entries_;
  bool has_stream_ = false;
  const void* stream_ = nullptr;
};

}  // namespace lip
