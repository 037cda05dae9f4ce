// dev_mem.h — who owns a block of device memory, and through which door it leaves.  Plain C++ (no HIP header: the host
// check of examples/ compiles it with g++ over malloc / free); the runtime is reached through the four functions below,
// which api.hip defines.  Their results are hipError_t values as ints (0 = hipSuccess), which AGP_HIP_CHECK accepts.
#pragma once
#include <cstddef>

namespace agp {
// Device allocations of the entry points that build several medium-sized objects per call (sparse GP fits, dense factors,
// cross validation): a hipMalloc / hipFree of tens of MB is 1-6 ms on this runtime, a sparse fit did ~40 of them (20 ms in
// its first stage alone).  dev_free parks the block (after the device-wide synchronisation hipFree implies) and
// dev_malloc hands out a parked block of exactly the requested size; at most DEV_CACHE_BYTES are kept, the oldest
// blocks go first; agp_context_destroy empties the cache.  Pointers that did not come from dev_malloc are hipFree'd: so
// dev_free is a correct way to free ANY device block, and the one door of the owners below.
// A block that leaves through any other door (a context slot that is closed or takes another size) goes through
// dev_release, and a block of dev_malloc that moves INTO a context slot is dropped from the table there (api.hip:
// dev_forget), so that the table of live blocks never holds an address the runtime may hand out again.
int dev_malloc_bytes(void **p, size_t bytes);        // the cached allocator
int dev_malloc_plain_bytes(void **p, size_t bytes);  // hipMalloc
template <class T>
inline int dev_malloc(T **p, size_t bytes) { return dev_malloc_bytes(reinterpret_cast<void **>(p), bytes); }
int dev_free(void *p);
// plain hipFree of a block that may have come from dev_malloc (forgets it first; never parks)
int dev_release(void *p);

// The unique owner of one device block.  A site chooses its allocator - alloc_cached for the medium-sized blocks of the
// entry points named above, alloc_plain otherwise - and the block leaves through dev_free either way.  Scope exit frees;
// an explicit reset() marks a free whose POSITION matters (hipFree and the parking dev_free synchronise the whole device).
template <class T>
class DevMem {
 public:
  DevMem() = default;
  DevMem(DevMem &&o) noexcept : p_(o.release()) {}
  DevMem &operator=(DevMem &&o) noexcept {
    if (this != &o) { reset(); p_ = o.release(); }
    return *this;
  }
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
  ~DevMem() { reset(); }
  int alloc_cached(size_t bytes) { return alloc(dev_malloc_bytes, bytes); }
  int alloc_plain(size_t bytes) { return alloc(dev_malloc_plain_bytes, bytes); }
  void adopt(T *p) { reset(); p_ = p; }
  T *release() { T *p = p_; p_ = nullptr; return p; }
  void reset() { if (p_) (void)dev_free(release()); }
  T *get() const { return p_; }
  operator T *() const { return p_; }

 private:
  int alloc(int (*how)(void **, size_t), size_t bytes) {
    reset();
    void *p = nullptr;
    const int e = how(&p, bytes);
    if (e == 0) p_ = static_cast<T *>(p);
    return e;
  }
  T *p_ = nullptr;
};

// One exact-size parking place of a context: the block an object of a recurring size leaves behind for the next one
// (hipMalloc + hipFree of a factor are 0.2 ms of an N = 512 fit that takes 0.17 ms).  The most recent size wins the slot.
class ParkSlot {
 public:
  ParkSlot() = default;
  ParkSlot(const ParkSlot &) = delete;
  ParkSlot &operator=(const ParkSlot &) = delete;
  ~ParkSlot() { clear(); }
  // the occupant when it has exactly `bytes`, else nullptr and the occupant stays
  void *take(size_t bytes) {
    if (!p_ || bytes_ != bytes) return nullptr;
    void *p = p_;
    p_ = nullptr;
    bytes_ = 0;
    return p;
  }
  // An occupant of another size is released and p moves in (evict = false, the sharded fit: it stays); an empty slot keeps
  // p; a slot that is still occupied refuses (false): p stays the caller's.
  bool park(void *p, size_t bytes, bool evict = true) {
    if (evict && p_ && bytes_ != bytes) clear();
    if (p_) return false;
    p_ = p;
    bytes_ = bytes;
    return true;
  }
  void clear() {
    if (p_) (void)dev_release(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void *p_ = nullptr;
  size_t bytes_ = 0;
};

// Grow-only scratch of a context, never handed to another owner.  reserve() leaves a buffer that is large enough alone;
// otherwise it frees, THEN allocates (plain: these blocks never enter the cache), and a failure leaves the buffer empty.
// What goes with growing - waiting for the stream that may still read the old block, reporting or swallowing the error -
// is the caller's (api.hip: reserve_ws; the mixed fit's and the panel kernels' buffers, whose callers fall back instead).
template <class T>
class GrowBuf {
 public:
  GrowBuf() = default;
  GrowBuf(const GrowBuf &) = delete;
  GrowBuf &operator=(const GrowBuf &) = delete;
  ~GrowBuf() { clear(); }
  int reserve(size_t bytes) {
    if (bytes_ >= bytes) return 0;
    clear();
    void *p = nullptr;
    const int e = dev_malloc_plain_bytes(&p, bytes);
    if (e != 0) return e;
    p_ = static_cast<T *>(p);
    bytes_ = bytes;
    return 0;
  }
  void clear() {
    if (p_) (void)dev_free(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  size_t bytes() const { return bytes_; }
  T *get() const { return p_; }
  operator T *() const { return p_; }

 private:
  T *p_ = nullptr;
  size_t bytes_ = 0;
};
}  // namespace agp
