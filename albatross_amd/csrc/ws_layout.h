// ws_layout.h — a workspace stated once.  A layout is a function that takes its regions from a WsLayout in order: over
// a null base that yields the size to allocate, over the allocation the pointers.  Plain C++: the layouts
// (batch_layout.h) are checked on the host under the sanitizers (examples/host_sanitize_check.cpp).
#pragma once
#include <cstddef>

namespace agp {
struct WsLayout {  // bump allocator over a base that may be null
  char *base;
  size_t off = 0;
  explicit WsLayout(void *b = nullptr) : base(static_cast<char *>(b)) {}
  template <class T>
  T *take(size_t count) {  // the next `count` elements of T, 16-byte aligned; nullptr on a null base
    off = (off + 15) / 16 * 16;
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += sizeof(T) * count;
    return p;
  }
  size_t bytes() const { return (off + 15) / 16 * 16; }
};
}  // namespace agp
